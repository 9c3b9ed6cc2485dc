// attach_checks_check — csrc/attach_checks.hpp, check by check: the exact message and return code of every refusal, and the
// edges on either side of each.  A stand-alone program (tests/test_attach_checks_cpu.py builds it with the host compiler and
// the address and undefined-behaviour sanitizers, and runs it): exit status 0 and "attach_checks_check: ok", or every
// difference and status 1.  The expected strings are the literals the entry points of csrc/record.inc have always printed.
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/fibhip.h"

// the library's fail() (csrc/host_util.hpp), recording the formatted message
static char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#include "../fib_tf_amd/csrc/attach_checks.hpp"

static int checks = 0, failures = 0;
// `rc` is FIBHIP_EINVAL and the message is `want`
static void refused(int rc, const char *want, int line)
{
    ++checks;
    if (rc == FIBHIP_EINVAL && strcmp(g_err, want) == 0) return;
    fprintf(stderr, "attach_checks_check: line %d: rc %d, message \"%s\"; expected rc %d, \"%s\"\n", line, rc, g_err, (int)FIBHIP_EINVAL, want);
    ++failures;
}
// `rc` is 0 and no message was written
static void accepted(int rc, int line)
{
    ++checks;
    if (rc == 0 && g_err[0] == 0) return;
    fprintf(stderr, "attach_checks_check: line %d: rc %d, message \"%s\"; expected acceptance\n", line, rc, g_err);
    ++failures;
}
#define REFUSED(call, want) (g_err[0] = 0, refused(call, want, __LINE__))
#define ACCEPTED(call) (g_err[0] = 0, accepted(call, __LINE__))

int main()
{
    // var
    ACCEPTED(var_check(0, 4, "electrode_begin"));
    ACCEPTED(var_check(3, 4, "electrode_begin"));
    REFUSED(var_check(4, 4, "electrode_begin"), "electrode_begin: bad var 4");
    REFUSED(var_check(-1, 4, "pmap_begin"), "pmap_begin: bad var -1");
    REFUSED(var_check(21, 21, "stats_begin: column %d", 3), "stats_begin: column 3: bad var 21");
    REFUSED(var_check(-2, 4, "%s: %s %d", "trig_begin", "rule", 0), "trig_begin: rule 0: bad var -2");

    // every
    ACCEPTED(every_check("leads_begin", 1));
    ACCEPTED(every_check("leads_begin", INT_MAX));
    REFUSED(every_check("leads_begin", 0), "leads_begin: every must be >= 1 (got 0)");
    REFUSED(every_check("trig_begin", -2), "trig_begin: every must be >= 1 (got -2)");

    // capacity: SIZE_MAX / bytes for most (here a sample of 3 float64 values) ...
    const long long most24 = (long long)(SIZE_MAX / 24);
    ACCEPTED(capacity_check("stats_begin", 1, 24));
    ACCEPTED(capacity_check("stats_begin", most24, 24));
    REFUSED(capacity_check("stats_begin", most24 + 1, 24), "stats_begin: bad capacity 768614336404564651");
    REFUSED(capacity_check("stats_begin", 0, 24), "stats_begin: bad capacity 0");
    REFUSED(capacity_check("waves_begin", -1, 40), "waves_begin: bad capacity -1");
    REFUSED(capacity_check("tips_begin", LLONG_MAX, 16), "tips_begin: bad capacity 9223372036854775807");
    // ... SIZE_MAX / 2 / per for frames (a frame of 4 x 5 float32 pixels; one of a single 8-bit pixel: every capacity fits) ...
    const long long most80 = (long long)(SIZE_MAX / 2 / 80);
    ACCEPTED(capacity_check("frames_begin", most80, 80, LLONG_MAX, SIZE_MAX / 2));
    REFUSED(capacity_check("frames_begin", most80 + 1, 80, LLONG_MAX, SIZE_MAX / 2), "frames_begin: bad capacity 115292150460684698");
    ACCEPTED(capacity_check("frames_begin", LLONG_MAX, 1, LLONG_MAX, SIZE_MAX / 2));
    REFUSED(capacity_check("frames_begin", 0, 1, LLONG_MAX, SIZE_MAX / 2), "frames_begin: bad capacity 0");
    // ... and INT_MAX besides for the potential map and the trigger program
    ACCEPTED(capacity_check("pmap_begin", INT_MAX, 160, INT_MAX));
    REFUSED(capacity_check("pmap_begin", (long long)INT_MAX + 1, 160, INT_MAX), "pmap_begin: bad capacity 2147483648");
    REFUSED(capacity_check("trig_begin", (long long)INT_MAX + 1, 24, INT_MAX), "trig_begin: bad capacity 2147483648");
    REFUSED(capacity_check("trig_begin", 0, 24, INT_MAX), "trig_begin: bad capacity 0");
    const long long most_pix = (long long)(SIZE_MAX / ((size_t)8 << 40));       // (a lattice so large that SIZE_MAX binds below INT_MAX)
    ACCEPTED(capacity_check("pmap_begin", most_pix, (size_t)8 << 40, INT_MAX));
    REFUSED(capacity_check("pmap_begin", most_pix + 1, (size_t)8 << 40, INT_MAX), "pmap_begin: bad capacity 2097152");

    // a rectangle: touching each side of a 6 x 8 grid, one cell outside each side, empty
    ACCEPTED(rect_check(6, 8, 0, 6, 0, 8, "x: "));
    ACCEPTED(rect_check(6, 8, 0, 1, 3, 4, "x: "));
    ACCEPTED(rect_check(6, 8, 5, 6, 3, 4, "x: "));
    ACCEPTED(rect_check(6, 8, 2, 3, 0, 1, "x: "));
    ACCEPTED(rect_check(6, 8, 2, 3, 7, 8, "x: "));
    REFUSED(rect_check(6, 8, -1, 1, 3, 4, "electrode_begin: electrode %d: ", 3),
            "electrode_begin: electrode 3: rows [-1, 1) x columns [3, 4) is empty or outside the 6 x 8 grid");
    REFUSED(rect_check(6, 8, 5, 7, 3, 4, "%s: %s %d: ", "stim_begin", "entry", 0),
            "stim_begin: entry 0: rows [5, 7) x columns [3, 4) is empty or outside the 6 x 8 grid");
    REFUSED(rect_check(6, 8, 2, 3, -1, 1, "trig_begin: sensor %d: ", 7),
            "trig_begin: sensor 7: rows [2, 3) x columns [-1, 1) is empty or outside the 6 x 8 grid");
    REFUSED(rect_check(6, 8, 2, 3, 7, 9, "pmap_begin: the window "), "pmap_begin: the window rows [2, 3) x columns [7, 9) is empty or outside the 6 x 8 grid");
    REFUSED(rect_check(6, 8, 2, 2, 0, 8, "lesion_begin: entry %d: ", 1),
            "lesion_begin: entry 1: rows [2, 2) x columns [0, 8) is empty or outside the 6 x 8 grid");
    REFUSED(rect_check(6, 8, 0, 6, 5, 4, "x: "), "x: rows [0, 6) x columns [5, 4) is empty or outside the 6 x 8 grid");

    // a window, its block and reduction
    int oh = -1, ow = -1;
    const int whole[4] = {0, 64, 0, 80}, low[4] = {0, 3, 0, 80}, narrow[4] = {0, 64, 8, 13}, outside[4] = {0, 65, 0, 80};
    ACCEPTED(window_check("frames_begin", 64, 80, whole, 16, 16, FIBHIP_FRAME_MEAN, oh, ow));
    if (oh != 4 || ow != 5) fprintf(stderr, "attach_checks_check: a window of 64 x 80 in blocks of 16 x 16 gave %d x %d pixels\n", oh, ow), ++failures;
    ACCEPTED(window_check("frames_begin", 64, 80, whole, 5, 3, FIBHIP_FRAME_POINT, oh, ow));
    if (oh != 12 || ow != 26) fprintf(stderr, "attach_checks_check: a window of 64 x 80 in blocks of 5 x 3 gave %d x %d pixels\n", oh, ow), ++failures;
    REFUSED(window_check("beats_begin", 64, 80, outside, 1, 1, 1, oh, ow),
            "beats_begin: the window rows [0, 65) x columns [0, 80) is empty or outside the 64 x 80 grid");
    REFUSED(window_check("frames_begin", 64, 80, whole, 0, 1, 1, oh, ow), "frames_begin: a block is 1 .. 16 cells each way (got 0 x 1)");
    REFUSED(window_check("frames_begin", 64, 80, whole, 1, 17, 1, oh, ow), "frames_begin: a block is 1 .. 16 cells each way (got 1 x 17)");
    REFUSED(window_check("spectrum_begin", 64, 80, low, 4, 1, 1, oh, ow), "spectrum_begin: a window of 3 x 80 cells holds no block of 4 x 1");
    REFUSED(window_check("spectrum_begin", 64, 80, narrow, 1, 6, 1, oh, ow), "spectrum_begin: a window of 64 x 5 cells holds no block of 1 x 6");
    REFUSED(window_check("frames_begin", 64, 80, whole, 1, 1, 2, oh, ow), "frames_begin: bad reduction 2");
    REFUSED(window_check("frames_begin", 64, 80, whole, 1, 1, -1, oh, ow), "frames_begin: bad reduction -1");

    // a range: empty ones, the last sample, one beyond
    ACCEPTED(range_check("stats_read", "samples", 0, 0, 0));
    ACCEPTED(range_check("stats_read", "samples", 3, 0, 3));
    ACCEPTED(range_check("stats_read", "samples", 0, 3, 3));
    ACCEPTED(range_check("stats_read", "samples", 2, 1, 3));
    REFUSED(range_check("stats_read", "samples", 2, 2, 3), "stats_read: samples [2, 4) of 3 taken");
    REFUSED(range_check("frames_read", "frames", 0, 4, 3), "frames_read: frames [0, 4) of 3 taken");
    REFUSED(range_check("trig_read", "samples", 4, 0, 3), "trig_read: samples [4, 4) of 3 taken");
    REFUSED(range_check("tips_read", "samples", -1, 1, 3), "tips_read: samples [-1, 0) of 3 taken");
    REFUSED(range_check("waves_links_read", "samples", 1, -1, 3), "waves_links_read: samples [1, 0) of 3 taken");
    REFUSED(range_check("pmap_summary", "samples", 0, 1, 0), "pmap_summary: samples [0, 1) of 0 taken");

    // a plane: the only bad value in the last cell (NaN), in the first (inf), somewhere in between
    std::vector<float> plane(3 * 5, 0.25f);
    ACCEPTED(finite_check("stats_begin", plane.data(), 3, 5, "the weight plane"));
    plane[14] = std::numeric_limits<float>::quiet_NaN();
    REFUSED(finite_check("stats_begin", plane.data(), 3, 5, "the weight plane"),
            "stats_begin: the weight plane has a value that is not finite (row 2, column 4)");
    ACCEPTED(finite_check("stats_begin", plane.data(), 2, 7, "the weight plane"));           // (a plane that ends in front of it)
    plane[14] = 1.0f;
    plane[0] = std::numeric_limits<float>::infinity();
    REFUSED(finite_check("leads_begin", plane.data(), 3, 5, "table %d", 2), "leads_begin: table 2 has a value that is not finite (row 0, column 0)");
    plane[0] = 1.0f;
    plane[7] = -std::numeric_limits<float>::infinity();
    REFUSED(finite_check("pmap_begin", plane.data(), 3, 5, "the weight plane"),
            "pmap_begin: the weight plane has a value that is not finite (row 1, column 2)");
    REFUSED(finite_check("pmap_begin", plane.data(), 4, 3, "the table"), "pmap_begin: the table has a value that is not finite (row 2, column 1)");
    plane[7] = std::numeric_limits<float>::max();
    ACCEPTED(finite_check("pmap_begin", plane.data(), 3, 5, "the table"));

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
    if (failures) {
        fprintf(stderr, "attach_checks_check: %d of %d checks failed\n", failures, checks);
        return 1;
    }
    printf("attach_checks_check: ok (%d checks, %s)\n", checks, build);
    return 0;
}
