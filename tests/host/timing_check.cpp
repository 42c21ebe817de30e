// timing_check.cpp -- the ring of timed calls and the stamp arithmetic (ev2gym_amd/csrc/ev2g_timing_host.h) against a model that keeps every call.
// Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 tests/host/timing_check.cpp -o timing_check && ./timing_check
//
// (tests/test_launch_timing_cpu.py does exactly that, and once more with -fsanitize=address,undefined.)
//   * slot arithmetic: `back` = 0 .. 40 after every one of 200 calls (six wraps of the 32 slots) names the slot of that call, or -1 past the ring,
//     past the first call, for a call that failed, and for everything after an untimed step;
//   * error exits: a call that takes its slot and returns before it is closed -- with or without having been opened -- reads -1 and moves the
//     earlier readings one place back; the next successful call makes them readable again;
//   * kinds: each slot keeps the kind it was opened with through the wraps; last_kind is the last call's, TIMING_NONE where its reading is -1;
//   * ticks to milliseconds at 100 000 kHz and at 1 kHz, large counter values, a pair never written (zeros), end < start, no clock rate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ev2gym_amd/csrc/ev2g_timing_host.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAIL line %d: %s (%s)\n", __LINE__, #cond, g_case); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)
static char g_case[256] = "";

static unsigned long long g_rng = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {   // [0, n)
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (unsigned)((g_rng >> 33) % n);
}

struct Call { bool closed; int kind; };   // the model: every timed call so far, oldest first

static void against_model(const TimingRing &r, const std::vector<Call> &calls, bool timed) {
    const int n = (int)calls.size();
    for (int back = -2; back <= TIMING_RING + 8; back++) {
        const int s = r.slot_of(back);
        const bool readable = timed && back >= 0 && back < TIMING_RING && back < n && calls[(size_t)(n - 1 - back)].closed;
        if (!readable) { CHECK(s == -1); continue; }
        CHECK(s == (n - back) % TIMING_RING);   // (the first call takes slot 1)
        CHECK(r.valid[s] && r.kind[s] == calls[(size_t)(n - 1 - back)].kind);
    }
    const int want = (timed && n > 0 && calls.back().closed) ? calls.back().kind : TIMING_NONE;
    CHECK(r.last_kind() == want);
    CHECK(std::strcmp(timing_kind_name(r.last_kind()), want == TIMING_STAMPS ? "stamps" : (want == TIMING_EVENTS ? "events" : "")) == 0);
}

static void ring_checks() {
    TimingRing r;
    std::vector<Call> calls;
    bool timed = false;
    std::snprintf(g_case, sizeof g_case, "fresh ring");
    against_model(r, calls, timed);
    for (int i = 0; i < 200; i++) {
        const unsigned what = rnd(10);
        const int kind = rnd(2) ? TIMING_STAMPS : TIMING_EVENTS;
        std::snprintf(g_case, sizeof g_case, "call %d, what %u, kind %d", i, what, kind);
        const int s = r.take();
        CHECK(s == r.slot && s == (i + 1) % TIMING_RING && !r.valid[s] && r.kind[s] == TIMING_NONE);
        if (what == 0) {   // refused before it knew what it launches
            calls.push_back({false, TIMING_NONE});
        } else if (what == 1) {   // failed behind the opening
            r.open(kind);
            calls.push_back({false, kind});
        } else {
            r.open(kind); r.close();
            timed = true;
            calls.push_back({true, kind});
        }
        against_model(r, calls, timed);
        if (what == 9) {   // a plain step behind it: every reading is -1 until the next timed call closes
            r.untimed(); timed = false;
            against_model(r, calls, timed);
        }
    }
    CHECK(r.calls == 200);
    // a failed call between two good ones, spelled out
    TimingRing q;
    std::snprintf(g_case, sizeof g_case, "good, refused, good");
    q.take(); q.open(TIMING_STAMPS); q.close();
    const int first = q.slot_of(0);
    CHECK(first == 1 && q.last_kind() == TIMING_STAMPS);
    q.take();
    CHECK(q.slot_of(0) == -1 && q.slot_of(1) == first && q.last_kind() == TIMING_NONE);
    q.take(); q.open(TIMING_EVENTS); q.close();
    CHECK(q.slot_of(0) == 3 && q.slot_of(1) == -1 && q.slot_of(2) == first && q.slot_of(3) == -1 && q.last_kind() == TIMING_EVENTS);
    CHECK(q.kind[first] == TIMING_STAMPS);
}

static void stamp_checks() {
    std::snprintf(g_case, sizeof g_case, "ticks to milliseconds");
    CHECK(timing_stamp_ms(1000, 1000 + 100000, 100000) == 1.0);          // 100 MHz: 100 000 ticks are a millisecond
    CHECK(timing_stamp_ms(1000, 1000 + 28950, 100000) == 0.2895);
    CHECK(timing_stamp_ms(5, 6, 100000) == 1.0 / 100000.0);
    CHECK(timing_stamp_ms(7, 7 + 250, 1) == 250.0);                       // 1 kHz: a tick is a millisecond
    CHECK(timing_stamp_ms(7, 7, 1) == 0.0);
    const unsigned long long big = 0xfffffff000000000ull;                  // counters near the top of 64 bits: the difference is what counts
    CHECK(timing_stamp_ms(big, big + 31100, 100000) == 0.311);
    CHECK(timing_stamp_ms(0, 0, 100000) == -1.0);                         // a pair no launch wrote
    CHECK(timing_stamp_ms(0, 123456, 100000) == -1.0);
    CHECK(timing_stamp_ms(2000, 1999, 100000) == -1.0);                   // the start word of a launch whose end word is still an older launch's
    CHECK(timing_stamp_ms(2000, 0, 1) == -1.0);
    CHECK(timing_stamp_ms(1000, 2000, 0) == -1.0 && timing_stamp_ms(1000, 2000, -5) == -1.0);   // a device that reports no clock rate
}

int main() {
    ring_checks();
    stamp_checks();
    std::printf("timing_check: ok\n");
    return 0;
}
