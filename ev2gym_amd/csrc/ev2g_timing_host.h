// ev2g_timing_host.h -- the host-only half of a timed call: the ring of the last TIMING_RING durations and what a slot of it holds.
//
// A timed call (ev2g_step_n, ev2g_rollout, ev2g_collect, run_chain's callers) takes the next slot of the ring once its arguments are accepted and
// closes it on the success path; a call that returns an error in between leaves its slot invalid (it reads -1) and the earlier readings one
// place further back.  A slot is timed in one of two ways:
//   * TIMING_EVENTS: a pair of HIP events recorded on the stream around the call's launches.  Each record is a barrier packet with a completion
//     signal and a system-scope release: the queue drains for it, and the next kernel starts cold (profiles/r28_launch_stamps.txt).
//   * TIMING_STAMPS: the one kernel of the call reads the constant-rate wall clock itself (ev2g_step_wave.h: WaveArgs::stamp) -- workgroup 0 in its
//     prologue into word 0 of the slot's pair, every workgroup at its exit -- behind a barrier, so not before its last wavefront -- as ONE atomic maximum into
//     word 1 (one per wavefront queued at the memory side and made the launch longer: profiles/r28_launch_stamps.txt).  Nothing but the kernel stands on the
//     stream.  The clock is monotonic, so a pair that is reused TIMING_RING calls later needs no clearing: the start word is overwritten, the end
//     word only grows.
// Plain C++17, no HIP, no handle: tests/host/timing_check.cpp runs the same functions.
#pragma once

constexpr int TIMING_RING = 32;   // timed calls whose durations stay readable

// Which instantiations of ev2g_step_wave carry the two stamp sites, by their FULLK: the wide stride-0 ones.  The kernel's STAMPED and route_step's
// StepRoute::stamps are both this function (tests/host/stamp_rule_check.cpp holds route_step to it): a slot opened as stamps whose kernel has no sites
// would never be written and read -1.
constexpr bool timing_wave_stamped(int fullk) { return fullk == 2; }

enum TimingKind { TIMING_NONE = 0, TIMING_EVENTS = 1, TIMING_STAMPS = 2 };

inline const char *timing_kind_name(int kind) { return kind == TIMING_STAMPS ? "stamps" : (kind == TIMING_EVENTS ? "events" : ""); }

struct TimingRing {
    int slot = 0;                    // the slot of the last timed call
    long long calls = 0;             // timed calls so far (slots further back than that were never taken)
    bool timed = false;              // the last call that stepped was a timed one (a plain ev2g_step clears it: every reading is -1 until the next timed call)
    bool valid[TIMING_RING] = {};    // the slot was closed (a call that failed half-way leaves it false: its duration reads -1)
    unsigned char kind[TIMING_RING] = {};   // TimingKind of the slot (TIMING_NONE between take and open)

    // the next slot, invalid until it is closed; returns it
    int take() {
        slot = (slot + 1) % TIMING_RING; calls += 1;
        valid[slot] = false; kind[slot] = TIMING_NONE;
        return slot;
    }
    // how the slot taken last is timed: decided once the call knows what it launches
    void open(int k) { kind[slot] = (unsigned char)k; }
    // the success path's end
    void close() { valid[slot] = true; timed = true; }
    // a call that steps without being timed
    void untimed() { timed = false; }
    // the slot of the call `back` timed calls ago (0: the last one), -1 where its reading is -1
    int slot_of(int back) const {
        if (!timed || back < 0 || back >= TIMING_RING || back >= calls) return -1;
        const int s = ((slot - back) % TIMING_RING + TIMING_RING) % TIMING_RING;
        return valid[s] ? s : -1;
    }
    // the kind of the last timed call (TIMING_NONE: none yet, it failed, or an untimed step came behind it)
    int last_kind() const { const int s = slot_of(0); return s < 0 ? TIMING_NONE : kind[s]; }
};

// a stamp pair in milliseconds at a clock of rate_khz ticks per millisecond; -1 for a pair that no launch wrote (zeroed at creation, or an end
// word older than its start word)
inline double timing_stamp_ms(unsigned long long start, unsigned long long end, int rate_khz) {
    if (rate_khz <= 0 || start == 0 || end < start) return -1.0;
    return (double)(end - start) / (double)rate_khz;
}
