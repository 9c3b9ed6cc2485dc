// host_util.hpp — what every host file of the library leans on: the error string, HIPCHK, and the host-visible waits.
#pragma once

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(...)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (__VA_ARGS__);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(FIBHIP_EHIP, "%s failed: %s (%s:%d)", #__VA_ARGS__, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                  \
    } while (0)

extern "C" const char *fibhip_last_error(void) { return g_err; }

static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

// ---- host-visible waits ---------------------------------------------------------------------------------
// A blocking hipStreamSynchronize parks the thread on an interrupt: 5-10 us until it runs again, a tenth of a 20-tick
// region of the 512x512 benchmark and a third of one image() read-back.  Poll instead for as long as short waits last
// (FIBHIP_SPIN_US, default 2000 us; 0 = always block), then block.
static long spin_us()
{
    static const long v = [] {
        const char *e = getenv("FIBHIP_SPIN_US");
        return e ? atol(e) : 2000L;
    }();
    return v;
}
static hipError_t wait_stream(hipStream_t s)
{
    const long lim = spin_us();
    if (lim <= 0) return hipStreamSynchronize(s);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        (void)hipGetLastError();                                  // hipErrorNotReady is not an error to report later
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(lim)) return hipStreamSynchronize(s);
    }
}
static hipError_t wait_event(hipEvent_t ev)
{
    const long lim = spin_us();
    if (lim <= 0) return hipEventSynchronize(ev);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        (void)hipGetLastError();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(lim)) return hipEventSynchronize(ev);
    }
}

// The end of everything enqueued on a stream (any handle: single device or shard, whatever the launch plan), noticed
// through a word of page-locked host memory that the stream itself
// writes when it gets there (hipStreamWriteValue32 behind the work) instead of through hipStreamQuery: the host spins on its own
// memory, and knows 3 us sooner (tools/ubench/notice.hip: launch call -> notice, minus the kernel: 8.5 us by hipStreamQuery spin,
// 7.6 by hipStreamSynchronize, 5.3 this way) — 1 % of a 20-tick region of the benchmark, and of every read-back of a driver loop.
struct DoneWord {
    unsigned *word = nullptr, *word_dev = nullptr;  // a word of page-locked memory of its own (host / device address) ...
    unsigned seq = 0;                               // ... and the value the stream writes into it when it has got that far
    bool off = false;                               // FIBHIP_STREAM_WRITE=0, or a runtime / stream that cannot: hipStreamQuery, as before
};
static hipError_t wait_done(DoneWord &d, hipStream_t s)
{
    const long lim = spin_us();
    if (lim <= 0 || d.off) return wait_stream(s);
    if (!d.word) {                                     // (first use: 64 bytes of page-locked memory per handle)
        if (hipHostMalloc((void **)&d.word, 64, hipHostMallocDefault) != hipSuccess ||
            hipHostGetDevicePointer((void **)&d.word_dev, d.word, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (d.word) hipHostFree(d.word);
            d.word = nullptr;
            d.off = true;
            return wait_stream(s);
        }
        *d.word = 0u;
    }
    const unsigned seq = ++d.seq;
    volatile unsigned *w = d.word;
    if (hipStreamWriteValue32(s, d.word_dev, seq, 0) != hipSuccess) {
        (void)hipGetLastError();
        d.off = true;                                  // (a runtime or a stream that cannot: the old way from now on)
        return wait_stream(s);
    }
    const auto t0 = std::chrono::steady_clock::now();
    long spins = 0;
    while (__atomic_load_n(w, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(lim)) return hipStreamSynchronize(s);
    }
    return hipSuccess;
}
