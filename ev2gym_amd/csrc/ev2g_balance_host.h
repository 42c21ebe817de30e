// ev2g_balance_host.h -- which env group every workgroup of a persistent launch steps, so that a CU's workgroups have about the same work in sum.
//
// A persistent launch of ev2g_step_wave that fast-forwards EV-free stretches is as long as its busiest CU, and a live step costs more the more
// workgroups its CU still holds (profiles/r25_cu_balance.txt: 1.00 / 0.91 / 0.83 / 0.78 at 4 / 3 / 2 / 1).  Today's map, a function of blockIdx.x,
// puts similar scenarios on one CU; re-ordering the scenarios so that heavy and light groups share a CU shortened the benchmark's launch by 6.5 %.
// This header is that re-ordering as a map blockIdx.x -> env group:
//   * a group's weight is its number of LIVE steps in the episode -- steps in which one of its envs holds an EV or receives one at the step's end
//     (a session with t_arr - 1 <= t <= t_dep): a function of the scenarios alone, not of the actions;
//   * workgroups are placed as observed: block b runs on XCD b % 8, and an XCD deals its blocks j = b / 8 round-robin to its CUs -- block b is the
//     (j / cpx)-th arrival on CU (b % 8) * cpx + j % cpx;
//   * the groups, heaviest first, are dealt to the CUs as a snake: forth over the first arrivals, back over the second ones, and so on.
// A map is a permutation of the groups whatever the placement really is: where workgroups land decides the launch's time, never its results (all
// state is indexed by env).  Plain C++17, no HIP, no handle: tests/host/balance_check.cpp runs the same functions against brute force.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

constexpr int BALANCE_MAX_T = 256;                       // steps per episode a live-step bitset holds
constexpr int BALANCE_WORDS = BALANCE_MAX_T / 64;       // 64-bit words per scenario

// the live steps of one scenario from its sessions' windows: bit t of out[t / 64]
inline void balance_live_bits(const int32_t *t_arr, const int32_t *t_dep, int64_t n_sessions, int T, uint64_t out[BALANCE_WORDS]) {
    for (int i = 0; i < BALANCE_WORDS; i++) out[i] = 0;
    const int last = std::min(T, BALANCE_MAX_T) - 1;
    for (int64_t s = 0; s < n_sessions; s++) {
        const long long lo = std::max<long long>((long long)t_arr[s] - 1, 0), hi = std::min<long long>(t_dep[s], last);
        for (long long t = lo; t <= hi; t++) out[t >> 6] |= 1ull << (t & 63);
    }
}

inline int balance_popcount(uint64_t x) {
    int n = 0;
    for (; x; x &= x - 1) n++;
    return n;
}

// weight[g] of the n_groups groups of `per_group` consecutive envs when env e runs scenario (e + off) mod M; bits: [M][BALANCE_WORDS]
inline void balance_group_weights(const std::vector<uint64_t> &bits, long long M, long long off, int E, int per_group, std::vector<int> &weight) {
    const int n_groups = (E + per_group - 1) / per_group;
    weight.assign((size_t)n_groups, 0);
    for (int g = 0; g < n_groups; g++) {
        uint64_t u[BALANCE_WORDS] = {};
        for (int e = g * per_group; e < std::min(E, (g + 1) * per_group); e++) {
            const uint64_t *w = &bits[(size_t)(((long long)e + off) % M) * BALANCE_WORDS];
            for (int i = 0; i < BALANCE_WORDS; i++) u[i] |= w[i];
        }
        for (int i = 0; i < BALANCE_WORDS; i++) weight[(size_t)g] += balance_popcount(u[i]);
    }
}

// the group workgroup b steps without a map (ev2g_step_wave.h: each XCD a contiguous range of groups)
inline int balance_default_group(int b, int nb) { return (nb & 7) == 0 ? (b & 7) * (nb >> 3) + (b >> 3) : b; }

// the order in which the workgroups take groups from the heavy end: by arrival round on their CU, inside a round along the snake over the CUs
inline void balance_block_order(int nb, int n_cu, std::vector<int> &blocks) {
    const int cpx = std::max(1, n_cu / 8), cus = 8 * cpx;
    std::vector<long long> key((size_t)nb);
    for (int b = 0; b < nb; b++) {
        const int x = b & 7, j = b >> 3, round = j / cpx, cu = x * cpx + j % cpx;
        key[(size_t)b] = (long long)round * cus + ((round & 1) ? cus - 1 - cu : cu);
    }
    blocks.resize((size_t)nb);
    std::iota(blocks.begin(), blocks.end(), 0);
    std::sort(blocks.begin(), blocks.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });   // (keys are distinct)
}

// map[b] = the group workgroup b steps; returns how many workgroups step another group than balance_default_group's
inline int balance_map(const std::vector<int> &weight, int n_cu, std::vector<int> &map) {
    const int nb = (int)weight.size();
    std::vector<int> groups((size_t)nb), blocks;
    std::iota(groups.begin(), groups.end(), 0);
    std::stable_sort(groups.begin(), groups.end(), [&](int a, int b) { return weight[(size_t)a] > weight[(size_t)b]; });
    balance_block_order(nb, n_cu, blocks);
    map.assign((size_t)nb, 0);
    int moved = 0;
    for (int i = 0; i < nb; i++) {
        map[(size_t)blocks[(size_t)i]] = groups[(size_t)i];
        moved += groups[(size_t)i] != balance_default_group(blocks[(size_t)i], nb);
    }
    return moved;
}
