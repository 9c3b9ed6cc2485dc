// sampler_check — csrc/sampler.hpp against a model that walks tick by tick.  A stand-alone program (tests/test_sampler_cpu.py
// builds it with the host compiler and the address and undefined-behaviour sanitizers, and runs it): exit status 0 and
// "sampler_check: ok", or the first difference and status 1.
//
// For every stride, head start and capacity: a fixed-seed sequence of launches, each cut to room() as the scheduler cuts them,
// with rewinds in between that are replayed one tick per launch, as a recovery replays them.  Checked against the model:
//   * no launch spans a sample tick;
//   * the slots issued are 0, 1, 2, ...; after a rewind of `lost` ticks exactly the slots of those ticks are issued again, in order;
//   * full_after(more) is true exactly when the model, walking `more` further ticks, would issue a slot >= cap;
//   * room(), due_after(), taken() and taken_with() say what the walk says.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fib_tf_amd/csrc/sampler.hpp"

struct Model {
    int every;
    long long k0, ticks = 0;                    // ticks launched so far
    bool sample_after(long long t) const { return (k0 + t) % every == 0; }      // is tick t (1-based) a sample tick?
    std::vector<long long> count = {0};         // count[t]: sample ticks among 1 .. t, counted one by one
    long long samples_upto(long long t)
    {
        while ((long long)count.size() <= t) count.push_back(count.back() + sample_after((long long)count.size()));
        return count[t];
    }
};

static unsigned rng_state;
static unsigned rnd(unsigned n)                 // 0 .. n - 1
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % n;
}

#define CHECK(cond, ...)                                                                              \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "sampler_check: every %d k0 %lld cap %lld, tick %lld: ", m.every, m.k0, cap, m.ticks); \
            fprintf(stderr, __VA_ARGS__);                                                             \
            fprintf(stderr, " (%s)\n", #cond);                                                        \
            return false;                                                                             \
        }                                                                                             \
    } while (0)

// one launch of up to `want` ticks; `slots`: slot issued behind tick t, or -1 (slots[0] unused)
static bool launch(Sampler &s, Model &m, long long cap, int want, std::vector<long long> &slots, const std::vector<long long> *replay)
{
    const int room = s.room();
    long long walk = 1;
    while (!m.sample_after(m.ticks + walk)) ++walk;
    CHECK(room == walk, "room() %d, the next sample tick is %lld ticks away", room, walk);
    const int T = want < room ? want : room;
    for (int t = 1; t < T; ++t) CHECK(!m.sample_after(m.ticks + t), "a launch of %d ticks spans the sample tick %lld", T, m.ticks + t);
    CHECK(s.due_after(T) == m.sample_after(m.ticks + T), "due_after(%d)", T);
    CHECK(s.taken_with(T) == m.samples_upto(m.ticks + T), "taken_with(%d) = %lld", T, s.taken_with(T));
    long long slot = -2;
    const bool due = s.advance(T, &slot);
    m.ticks += T;
    CHECK(due == m.sample_after(m.ticks), "advance(%d) says %d", T, (int)due);
    CHECK(s.taken() == m.samples_upto(m.ticks), "taken() = %lld", s.taken());
    if ((long long)slots.size() <= m.ticks) slots.resize(m.ticks + 1, -1);
    if (due) {
        CHECK(slot == m.samples_upto(m.ticks) - 1, "slot %lld, the model's is %lld", slot, m.samples_upto(m.ticks) - 1);
        if (replay) CHECK(slot == (*replay)[m.ticks], "the replay issued slot %lld, the lost launch had issued %lld", slot, (*replay)[m.ticks]);
        slots[m.ticks] = slot;
    } else if (replay) {
        CHECK((*replay)[m.ticks] == -1, "the replay issued no slot behind tick %lld, the lost launch had issued %lld", m.ticks, (*replay)[m.ticks]);
    }
    return true;
}

static bool run(int every, long long k0, long long cap, unsigned seed)
{
    Sampler s = {};
    Model m = {every, k0};
    CHECK(s.room() == INT_MAX, "room() of a sampler that is off");
    s.on = true;
    s.start(every, cap, k0);
    rng_state = seed;
    std::vector<long long> slots(1, -1);
    for (int step = 0; step < 300; ++step) {
        // would the samples of `more` further ticks overflow?  The model walks them
        for (int more = 0; more <= 2 * every + 3; ++more) {
            const long long last_slot = m.samples_upto(m.ticks + more) - 1;
            CHECK(s.full_after(more) == (last_slot >= cap), "full_after(%d) with the model's slot %lld", more, last_slot);
        }
        const int want = 1 + (int)rnd(40);
        const int T = want < s.room() ? want : s.room();
        if (s.full_after(T)) break;                                 // (the scheduler refuses these ticks)
        if (!launch(s, m, cap, want, slots, nullptr)) return false;
        if (rnd(4) == 0 && m.ticks > 0) {                           // a launch gave up: the last `lost` ticks are void and are replayed
            const long long lost = 1 + rnd((unsigned)(m.ticks < 70 ? m.ticks : 70));
            const std::vector<long long> before = slots;
            s.rewind(lost);
            m.ticks -= lost;
            for (long long t = m.ticks + 1; t <= m.ticks + lost; ++t) slots[t] = -1;
            const long long end = m.ticks + lost;
            while (m.ticks < end)
                if (!launch(s, m, cap, 1, slots, &before)) return false;
            CHECK(slots == before, "after the replay of %lld ticks the slots differ", lost);
        }
    }
    long long next = 0;                                             // all in all: 0, 1, 2, ... in tick order
    for (long long t = 1; t <= m.ticks; ++t)
        if (slots[t] >= 0) {
            CHECK(slots[t] == next, "slot %lld behind tick %lld, expected %lld", slots[t], t, next);
            ++next;
        }
    return true;
}

int main()
{
    const int everys[] = {1, 2, 3, 7, 32};
    const long long caps[] = {1, 5, LLONG_MAX};
    int runs = 0;
    for (int every : everys)
        for (long long k0 : {0LL, (long long)every - 1})
            for (long long cap : caps)
                for (unsigned seed = 1; seed <= 4; ++seed, ++runs)
                    if (!run(every, k0, cap, seed * 2654435761u)) return 1;
#if defined(__SANITIZE_ADDRESS__)
    const char *build = "address sanitizer on";
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
    const char *build = "address sanitizer on";
#else
    const char *build = "no sanitizer";
#endif
#else
    const char *build = "no sanitizer";
#endif
    printf("sampler_check: ok (%d runs, %s)\n", runs, build);
    return 0;
}
