// balance_check.cpp -- the CU-balance maps (ev2gym_amd/csrc/ev2g_balance_host.h) against brute force.  Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 tests/host/balance_check.cpp -o balance_check && ./balance_check
//
// (tests/test_cu_balance_cpu.py does exactly that, and once more with -fsanitize=address,undefined.)
//   * balance_live_bits / balance_group_weights: against a step-by-step count from the sessions' windows, random sessions (windows that start before
//     step 0, end behind the episode, lie outside it, empty envs), every pool offset, partial last groups, T up to 256;
//   * balance_block_order: a permutation of the workgroups for every grid of 1 .. 2100 workgroups and several CU counts; consecutive entries of a
//     round lie on neighbouring CUs, and the round's direction alternates;
//   * balance_map: a permutation of the groups for every weight shape with n <= 64 groups (all equal, one heavy, strictly falling, strictly rising,
//     two values, random) and random ones up to 2048; the i-th workgroup of the order gets the i-th heaviest group (sort, then index; ties by group
//     index); `moved` counts the differences from the default map; and for grids that fill the CUs evenly, the CUs' weight sums differ by no more
//     than the heaviest group's weight (what the snake is for).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ev2gym_amd/csrc/ev2g_balance_host.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAIL line %d: %s (%s)\n", __LINE__, #cond, g_case); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)
static char g_case[256] = "";

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {   // [0, n)
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 33) % n);
}

static bool is_permutation(const std::vector<int> &v) {
    std::vector<char> seen(v.size(), 0);
    for (int x : v) {
        if (x < 0 || (size_t)x >= v.size() || seen[(size_t)x]) return false;
        seen[(size_t)x] = 1;
    }
    return true;
}

static void check_weights() {
    for (int rep = 0; rep < 200; rep++) {
        const int T = rep < 4 ? (rep == 0 ? 1 : rep == 1 ? 64 : rep == 2 ? 65 : 256) : 1 + (int)rnd(256);
        const int M = 1 + (int)rnd(40), E = 1 + (int)rnd((uint32_t)M);
        std::snprintf(g_case, sizeof g_case, "weights: T %d M %d E %d", T, M, E);
        std::vector<int32_t> ta, td;
        std::vector<int64_t> start(1, 0);
        for (int m = 0; m < M; m++) {
            const int n = (int)rnd(6);   // (empty envs among them)
            for (int s = 0; s < n; s++) {
                const int a = (int)rnd((uint32_t)T + 20) - 10;
                ta.push_back(a);
                td.push_back(a + (int)rnd(40) - 2);   // (t_dep < t_arr - 1: an empty window)
            }
            start.push_back((int64_t)ta.size());
        }
        std::vector<uint64_t> bits((size_t)M * BALANCE_WORDS);
        std::vector<std::vector<char>> live((size_t)M, std::vector<char>((size_t)T, 0));
        for (int m = 0; m < M; m++) {
            balance_live_bits(ta.data() + start[(size_t)m], td.data() + start[(size_t)m], start[(size_t)m + 1] - start[(size_t)m], T, &bits[(size_t)m * BALANCE_WORDS]);
            for (int64_t s = start[(size_t)m]; s < start[(size_t)m + 1]; s++)
                for (int t = 0; t < T; t++)
                    if (ta[(size_t)s] - 1 <= t && t <= td[(size_t)s]) live[(size_t)m][(size_t)t] = 1;
            for (int t = 0; t < BALANCE_MAX_T; t++)
                CHECK(((bits[(size_t)m * BALANCE_WORDS + (size_t)(t >> 6)] >> (t & 63)) & 1) == (uint64_t)(t < T ? live[(size_t)m][(size_t)t] : 0));
        }
        for (int off = 0; off < M; off++) {
            std::vector<int> w;
            balance_group_weights(bits, M, off, E, 4, w);
            CHECK((int)w.size() == (E + 3) / 4);
            for (int g = 0; g < (int)w.size(); g++) {
                int want = 0;
                for (int t = 0; t < T; t++) {
                    bool any = false;
                    for (int e = 4 * g; e < 4 * g + 4 && e < E; e++) any = any || live[(size_t)((e + off) % M)][(size_t)t];
                    want += any;
                }
                CHECK(w[(size_t)g] == want);
            }
        }
    }
}

static void check_order() {
    const int cu_counts[] = {256, 304, 8, 64, 0, 5};
    for (int n_cu : cu_counts)
        for (int nb = 1; nb <= 2100; nb++) {
            std::snprintf(g_case, sizeof g_case, "order: nb %d n_cu %d", nb, n_cu);
            std::vector<int> blocks;
            balance_block_order(nb, n_cu, blocks);
            CHECK((int)blocks.size() == nb && is_permutation(blocks));
            const int cpx = n_cu / 8 > 1 ? n_cu / 8 : 1, cus = 8 * cpx;
            long long prev = -1;
            for (int b : blocks) {   // rounds in order; inside a round the CUs forth (even rounds) or back (odd ones)
                const int round = (b >> 3) / cpx, cu = (b & 7) * cpx + (b >> 3) % cpx;
                const long long pos = (long long)round * cus + ((round & 1) ? cus - 1 - cu : cu);
                CHECK(pos > prev);
                prev = pos;
            }
        }
}

static void check_map_one(const std::vector<int> &w, int n_cu) {
    const int nb = (int)w.size();
    std::vector<int> map, blocks;
    const int moved = balance_map(w, n_cu, map);
    CHECK((int)map.size() == nb && is_permutation(map));
    balance_block_order(nb, n_cu, blocks);
    // brute force: the heaviest group not yet taken (the lowest index among equals), nb times
    std::vector<char> taken((size_t)nb, 0);
    int diff = 0;
    for (int i = 0; i < nb; i++) {
        int best = -1;
        for (int g = 0; g < nb; g++)
            if (!taken[(size_t)g] && (best < 0 || w[(size_t)g] > w[(size_t)best])) best = g;
        taken[(size_t)best] = 1;
        CHECK(map[(size_t)blocks[(size_t)i]] == best);
        diff += best != balance_default_group(blocks[(size_t)i], nb);
    }
    CHECK(moved == diff);
    const int cpx = n_cu / 8 > 1 ? n_cu / 8 : 1, cus = 8 * cpx;
    if (nb % (2 * cus) == 0) {   // whole pairs of rounds: a forth-and-back pair hands every CU the same sum up to the heaviest group's weight
        std::vector<long long> sum((size_t)cus, 0);
        int wmax = 0;
        for (int b = 0; b < nb; b++) {
            sum[(size_t)((b & 7) * cpx + (b >> 3) % cpx)] += w[(size_t)map[(size_t)b]];
            wmax = w[(size_t)map[(size_t)b]] > wmax ? w[(size_t)map[(size_t)b]] : wmax;
        }
        long long lo = sum[0], hi = sum[0];
        for (long long s : sum) { lo = s < lo ? s : lo; hi = s > hi ? s : hi; }
        CHECK(hi - lo <= wmax);
    }
}

static void check_map() {
    for (int n = 1; n <= 64; n++)
        for (int shape = 0; shape < 6; shape++)
            for (int n_cu : {256, 8, 16}) {
                std::snprintf(g_case, sizeof g_case, "map: n %d shape %d n_cu %d", n, shape, n_cu);
                std::vector<int> w((size_t)n);
                for (int g = 0; g < n; g++)
                    w[(size_t)g] = shape == 0 ? 60 : shape == 1 ? (g == n / 2 ? 112 : 3) : shape == 2 ? 255 - g : shape == 3 ? g : shape == 4 ? (g & 1 ? 70 : 50) : (int)rnd(257);
                check_map_one(w, n_cu);
            }
    const int sizes[] = {65, 127, 128, 255, 256, 257, 512, 1000, 1024, 1025, 1536, 2047, 2048};
    for (int n : sizes)
        for (int rep = 0; rep < 3; rep++) {
            std::snprintf(g_case, sizeof g_case, "map: n %d random %d", n, rep);
            std::vector<int> w((size_t)n);
            for (int g = 0; g < n; g++) w[(size_t)g] = rep == 0 ? 45 + (int)rnd(31) : (int)rnd(257);
            check_map_one(w, rep == 2 ? 64 : 256);
        }
    // the default map itself is a permutation for every grid
    for (int nb = 1; nb <= 2100; nb++) {
        std::snprintf(g_case, sizeof g_case, "default map: nb %d", nb);
        std::vector<int> d((size_t)nb);
        for (int b = 0; b < nb; b++) d[(size_t)b] = balance_default_group(b, nb);
        CHECK(is_permutation(d));
    }
}

int main() {
    check_weights();
    check_order();
    check_map();
    std::printf("balance_check: ok\n");
    return 0;
}
