// sampler.hpp — the tick counter of a recorder that takes a sample every `every` ticks.  Plain C++, nothing of HIP and nothing
// of the handle: tests/sampler_check.cpp builds it alone.
//
// `k` counts the ticks LAUNCHED since the recorder was attached (plus a head start, see start()); a sample is due whenever it
// lands on a multiple of `every`, and that sample's slot is k / every - 1.  No launch spans a sample tick (room() bounds every
// launch), so the counter never steps over one.  The slot is always computed from the counter and never kept anywhere else:
// that is why rewind() is all a recovery has to do — the replay issues the same slots again.
#pragma once
#include <climits>

struct Sampler {
    bool on;
    bool before_slow;       // set at attach: a sample reads what a deferred update of the state (Courtemanche's 'slow') assigns,
                            // so it is taken before that update rides on its tick (sched.inc slow_sample_due)
    int every;
    long long k;
    long long cap;          // samples the recorder holds; LLONG_MAX: it never fills up

    // attach: the first sample follows tick every - k0 (the frame recorder's `first`), the later ones `every` ticks apart
    void start(int every_, long long cap_, long long k0 = 0) { every = every_; cap = cap_; k = k0; }
    // ticks up to and including the next sample tick (INT_MAX: not attached)
    int room() const { return on ? every - (int)(k % every) : INT_MAX; }
    // is a sample due right behind `pending` further ticks?
    bool due_after(long long pending) const { return (k + pending) % every == 0; }
    // samples taken so far / once `pending` further ticks have been launched
    long long taken() const { return k / every; }
    long long taken_with(long long pending) const { return (k + pending) / every; }
    // a launch of `ticks` ticks (<= room()) has been issued: is a sample due behind it, and in which slot?
    bool advance(int ticks, long long *slot)
    {
        k += ticks;
        if (k % every) return false;
        *slot = k / every - 1;
        return true;
    }
    // would the samples of `more` further ticks overflow the recorder?
    bool full_after(long long more) const { return (k + more) / every > cap; }
    // the last `lost` ticks are void and will be launched again
    void rewind(long long lost) { k -= lost; }
};
