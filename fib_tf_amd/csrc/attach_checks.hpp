// attach_checks.hpp — the argument checks the recorders' entry points share (record.inc): what every _begin asks of `var`,
// `every` and `capacity`, of a plane, a rectangle and a window, and what every ranged _read asks of its range.  Plain C++,
// nothing of HIP and nothing of the handle: the grid comes in as H, W and nvar, a sample as its size in bytes, and
// tests/attach_checks_check.cpp builds the header alone.  Whoever includes it provides fail() and the FIBHIP_E* codes
// (host_util.hpp, include/fibhip.h); `who` names the entry point in every message.
#pragma once
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

// `var` names one of the model's `nvar` arrays; `who` is printf's ("stats_begin: column %d")
static int var_check(int var, int nvar, const char *who, ...)
{
    if (var >= 0 && var < nvar) return 0;
    char name[128];
    va_list ap;
    va_start(ap, who);
    vsnprintf(name, sizeof name, who, ap);
    va_end(ap);
    return fail(FIBHIP_EINVAL, "%s: bad var %d", name, var);
}
static inline int every_check(const char *who, int every)
{
    if (every < 1) return fail(FIBHIP_EINVAL, "%s: every must be >= 1 (got %d)", who, every);
    return 0;
}
// `capacity` samples of `bytes` each (> 0) must be at least one and fit `budget` bytes — SIZE_MAX, the frame recorder keeps to
// half of it — and stay within `most` where a kernel takes the sample index as an int (the potential map, the trigger program)
static inline int capacity_check(const char *who, long long capacity, size_t bytes, long long most = LLONG_MAX, size_t budget = SIZE_MAX)
{
    if (capacity < 1 || capacity > most || (unsigned long long)capacity > budget / bytes)
        return fail(FIBHIP_EINVAL, "%s: bad capacity %lld", who, capacity);
    return 0;
}
// every value of a plane of `rows` x `cols` floats is finite, or "<who>: <what> has a value that is not finite (row, column)";
// `what` is printf's ("the weight plane", "table %d")
static int finite_check(const char *who, const float *plane, size_t rows, size_t cols, const char *what, ...)
{
    for (size_t i = 0; i < rows * cols; ++i)
        if (!std::isfinite(plane[i])) {
            char name[128];
            va_list ap;
            va_start(ap, what);
            vsnprintf(name, sizeof name, what, ap);
            va_end(ap);
            return fail(FIBHIP_EINVAL, "%s: %s has a value that is not finite (row %zu, column %zu)", who, name, i / cols, i % cols);
        }
    return 0;
}
// "<prefix>rows [r0, r1) x columns [c0, c1) is empty or outside the H x W grid"; the prefix is printf's
static int rect_check(int H, int W, int r0, int r1, int c0, int c1, const char *prefix, ...)
{
    if (r0 >= 0 && r1 <= H && c0 >= 0 && c1 <= W && r0 < r1 && c0 < c1) return 0;
    char who[128];
    va_list ap;
    va_start(ap, prefix);
    vsnprintf(who, sizeof who, prefix, ap);
    va_end(ap);
    return fail(FIBHIP_EINVAL, "%srows [%d, %d) x columns [%d, %d) is empty or outside the %d x %d grid", who, r0, r1, c0, c1, H, W);
}
// the pixel plane of the frame, spectrum and beat recorders from the caller's window, block and reduction: oh x ow pixels
static int window_check(const char *who, int H, int W, const int *window, int by, int bx, int reduce, int &oh, int &ow)
{
    const int r0 = window[0], r1 = window[1], c0 = window[2], c1 = window[3];
    if (int rc = rect_check(H, W, r0, r1, c0, c1, "%s: the window ", who)) return rc;
    if (by < 1 || by > FIBHIP_MAX_FRAME_BLOCK || bx < 1 || bx > FIBHIP_MAX_FRAME_BLOCK)
        return fail(FIBHIP_EINVAL, "%s: a block is 1 .. %d cells each way (got %d x %d)", who, FIBHIP_MAX_FRAME_BLOCK, by, bx);
    oh = (r1 - r0) / by;
    ow = (c1 - c0) / bx;
    if (oh < 1 || ow < 1) return fail(FIBHIP_EINVAL, "%s: a window of %d x %d cells holds no block of %d x %d", who, r1 - r0, c1 - c0, by, bx);
    if (reduce != FIBHIP_FRAME_POINT && reduce != FIBHIP_FRAME_MEAN) return fail(FIBHIP_EINVAL, "%s: bad reduction %d", who, reduce);
    return 0;
}
// "[first, first + count) of `taken`": the range a _read may ask for (`what`: "samples", "frames")
static int range_check(const char *who, const char *what, long long first, long long count, long long taken)
{
    if (first < 0 || count < 0 || first + count > taken)
        return fail(FIBHIP_EINVAL, "%s: %s [%lld, %lld) of %lld taken", who, what, first, first + count, taken);
    return 0;
}
