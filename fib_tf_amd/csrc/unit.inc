// unit.inc — entry points that need no handle: the unit-level array ops of the parity tests and the device yardsticks.
// (included by fibhip.hip)

// IonicModel's building blocks as array ops on HOST arrays (copied through the device), for the
// unit-level parity tests: op 0 enforce_boundary(a), 1 laplace(a [, phi]), 2 phase_field(pad(a), phi),
// 3 rush_larsen(a=g, b=g_inf, c=tau, dt).
extern "C" int fibhip_unit_op(int device, int op, int H, int W, const float *a, const float *b, const float *c,
                              const float *phi, double dt, int fast, float *out)
{
    if (!a || !out || H < 3 || W < 3 || op < 0 || op > 3) return fail(FIBHIP_EINVAL, "unit_op: bad argument");
    if (op == OP_RUSH_LARSEN && (!b || !c)) return fail(FIBHIP_EINVAL, "unit_op: rush_larsen needs g_inf and tau");
    if (op == OP_PHASE && !phi) return fail(FIBHIP_EINVAL, "unit_op: phase_field needs phi");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)H * W, B = n * sizeof(float);
    float *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, 9 * B));          // a b c phi ph3[4] out
    float *da = d, *db = d + n, *dc = d + 2 * n, *dphi = d + 3 * n, *dph3 = d + 4 * n, *dout = d + 8 * n;
    int rc = 0;
    do {
        if (hipMemcpy(da, a, B, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(FIBHIP_EHIP, "unit_op: H2D failed"); break; }
        if (b && hipMemcpy(db, b, B, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(FIBHIP_EHIP, "unit_op: H2D failed"); break; }
        if (c && hipMemcpy(dc, c, B, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(FIBHIP_EHIP, "unit_op: H2D failed"); break; }
        if (phi) {
            if (hipMemcpy(dphi, phi, B, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(FIBHIP_EHIP, "unit_op: H2D failed"); break; }
            Geo g;
            g.H = g.Hg = H; g.W = W; g.pitch = W; g.row_off = 0; g.r0 = 0; g.r1 = H; g.rb0 = g.rb1 = g.ty_a = 0; g.tiles_x = g.ntiles = 0;
            hipLaunchKernelGGL(phase_prep_kernel, dim3(256), dim3(256), 0, 0, g, dphi, dph3, dph3 + n, dph3 + 2 * n, dph3 + 3 * n,
                               (float *)nullptr, (float *)nullptr);
        }
        const float mdt = (float)(-dt);
        if (fast)
            hipLaunchKernelGGL(unit_op_kernel<Fast>, dim3(256), dim3(256), 0, 0, op, H, W, da, db, dc, phi ? dph3 : nullptr, mdt, dout);
        else
            hipLaunchKernelGGL(unit_op_kernel<Exact>, dim3(256), dim3(256), 0, 0, op, H, W, da, db, dc, phi ? dph3 : nullptr, mdt, dout);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout, B, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(FIBHIP_EHIP, "unit_op: kernel or D2H failed");
            break;
        }
    } while (0);
    hipFree(d);
    return rc;
}

// The tensor operator of a handle with per-cell diffusion tensors (fibhip_set_tensor) on HOST arrays: laplace(a) with the
// tensor D = [[dyy, dxy], [dxy, dxx]] and the phase field phi (null: 1 everywhere) — tensor_prep_kernel's planes, then
// lap9_tensor and the first-order term under the policy asked for, as tick_kernel's tensor variants run them.
extern "C" int fibhip_unit_laplace_tensor(int device, int H, int W, const float *a, const float *phi, const float *dyy, const float *dxx,
                                          const float *dxy, int fast, float *out)
{
    if (!a || !dyy || !dxx || !dxy || !out || H < 3 || W < 3 || (long long)H * W > INT_MAX / 16)
        return fail(FIBHIP_EINVAL, "unit_laplace_tensor: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(FIBHIP_EINVAL, "device %d out of range", device);
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)H * W, B = n * sizeof(float);
    float *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, 17 * B));         // a phi out | dyy dxx dxy | wy wx wa wb wc | gy gx q4 r4 pyr pxr
    float *da = d, *dphi = d + n, *dout = d + 2 * n, *dt = d + 3 * n, *dw = d + 6 * n, *dp = d + 11 * n;
    int rc = 0;
    do {
        if (hipMemcpy(da, a, B, hipMemcpyHostToDevice) != hipSuccess || (phi && hipMemcpy(dphi, phi, B, hipMemcpyHostToDevice) != hipSuccess) ||
            hipMemcpy(dt, dyy, B, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dt + n, dxx, B, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dt + 2 * n, dxy, B, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(FIBHIP_EHIP, "unit_laplace_tensor: H2D failed");
            break;
        }
        Geo g;
        g.H = g.Hg = H; g.W = W; g.pitch = W; g.row_off = 0; g.r0 = 0; g.r1 = H; g.rb0 = g.rb1 = g.ty_a = 0; g.tiles_x = g.ntiles = 0;
        TensorPlanes t;
        t.dyy = dt; t.dxx = dt + n; t.dxy = dt + 2 * n;
        t.wy = dw; t.wx = dw + n; t.wa = dw + 2 * n; t.wb = dw + 3 * n; t.wc = dw + 4 * n;
        PhaseTab ph;
        ph.dpy = dp; ph.dpx = dp + n; ph.q4 = dp + 2 * n; ph.r4 = dp + 3 * n; ph.pyr = dp + 4 * n; ph.pxr = dp + 5 * n; ph.phi = dphi;
        hipLaunchKernelGGL(tensor_prep_kernel, dim3(256), dim3(256), 0, 0, g, phi ? (const float *)dphi : (const float *)nullptr, t, dp, dp + n,
                           dp + 2 * n, dp + 3 * n, dp + 4 * n, dp + 5 * n);
        if (fast)
            hipLaunchKernelGGL(unit_tensor_kernel<Fast>, dim3(256), dim3(256), 0, 0, H, W, da, t, ph, dout);
        else
            hipLaunchKernelGGL(unit_tensor_kernel<Exact>, dim3(256), dim3(256), 0, 0, H, W, da, t, ph, dout);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout, B, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(FIBHIP_EHIP, "unit_laplace_tensor: kernel or D2H failed");
            break;
        }
    } while (0);
    hipFree(d);
    return rc;
}

extern "C" int fibhip_court_inter(int device, int n, const float *V, int fast, float *out)
{
    if (!V || !out || n <= 0) return fail(FIBHIP_EINVAL, "court_inter: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    float *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)(1 + COURT_NINTER) * n * sizeof(float)));
    int rc = 0;
    do {
        if (hipMemcpy(d, V, (size_t)n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { rc = fail(FIBHIP_EHIP, "court_inter: H2D failed"); break; }
        const int blocks = (n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048;
        if (fast)
            hipLaunchKernelGGL(court_inter_kernel<Fast>, dim3(blocks), dim3(256), 0, 0, n, d, d + n);
        else
            hipLaunchKernelGGL(court_inter_kernel<Exact>, dim3(blocks), dim3(256), 0, 0, n, d, d + n);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpy(out, d + n, (size_t)COURT_NINTER * n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(FIBHIP_EHIP, "court_inter: kernel or D2H failed");
            break;
        }
    } while (0);
    hipFree(d);
    return rc;
}

// the velocity fit (record.inc vel_*, velocity_fit_kernel) on HOST planes: how the tests reach the kernel with rings no run makes
extern "C" int fibhip_velocity_fit(int device, int depth, int oh, int ow, const float *t, const int *count, int back, int radius, float max_dt,
                                   int min_cells, const unsigned char *mask, int *nfit, float *gy, float *gx, float *rms)
{
    if (!t || !count) return fail(FIBHIP_EINVAL, "velocity_fit: null argument (t and count are required)");
    if (oh < 1 || ow < 1 || (long long)oh * ow > INT_MAX) return fail(FIBHIP_EINVAL, "velocity_fit: bad shape %d x %d", oh, ow);
    if (int rc = vel_refusals("velocity_fit", depth, back, radius, max_dt, min_cells)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    const size_t npix = (size_t)oh * (size_t)ow, B = npix * sizeof(float);
    float *d = nullptr;                             // t[depth] | count | the four maps | mask
    HIPCHK(hipMalloc((void **)&d, ((size_t)depth + 5) * B + npix));
    float *dt = d, *dn = d + (size_t)depth * npix, *maps = dn + npix;
    unsigned char *dmask = reinterpret_cast<unsigned char *>(maps + 4 * npix);
    void *const dst[4] = {nfit, gy, gx, rms};
    int rc = 0;
    do {
        if (hipMemcpy(dt, t, (size_t)depth * B, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dn, count, B, hipMemcpyHostToDevice) != hipSuccess ||
            (mask && hipMemcpy(dmask, mask, npix, hipMemcpyHostToDevice) != hipSuccess)) {
            rc = fail(FIBHIP_EHIP, "velocity_fit: H2D failed");
            break;
        }
        vel_launch(vel_args(dt, reinterpret_cast<const int *>(dn), mask ? dmask : nullptr, depth, oh, ow, back, radius, max_dt, min_cells, maps), 0);
        if (hipGetLastError() != hipSuccess) { rc = fail(FIBHIP_EHIP, "velocity_fit: the launch failed"); break; }
        for (int i = 0; i < 4 && !rc; ++i)
            if (dst[i] && hipMemcpy(dst[i], maps + (size_t)i * npix, B, hipMemcpyDeviceToHost) != hipSuccess)
                rc = fail(FIBHIP_EHIP, "velocity_fit: kernel or D2H failed");
    } while (0);
    hipFree(d);
    return rc;
}

extern "C" int fibhip_warm(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(FIBHIP_EINVAL, "device %d out of range", device);
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(copy_kernel, dim3(1), dim3(256), 0, 0, (const fib_v4f *)nullptr, (fib_v4f *)nullptr, (size_t)0);   // n = 0: touches nothing
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(0));
    return 0;
}

extern "C" int fibhip_copy_bandwidth(int device, size_t nbytes, int reps, float *gbs)
{
    if (!gbs || nbytes < (1u << 20) || reps < 1) return fail(FIBHIP_EINVAL, "copy_bandwidth: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    const size_t n = nbytes / sizeof(fib_v4f);
    fib_v4f *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    do {
        if (hipMalloc((void **)&a, n * sizeof(fib_v4f)) != hipSuccess || hipMalloc((void **)&b, n * sizeof(fib_v4f)) != hipSuccess ||
            hipMemset(a, 0, n * sizeof(fib_v4f)) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
            hipEventCreate(&e1) != hipSuccess) {
            rc = fail(FIBHIP_EHIP, "copy_bandwidth: allocation failed");
            break;
        }
        const unsigned grid = (unsigned)((n + 255) / 256);  // one 16-byte element per thread
        hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, 0, a, b, n);   // warm-up
        float best = 1e30f;
        for (int r = 0; r < reps; ++r) {
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, 0, a, b, n);
            hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(FIBHIP_EHIP, "copy_bandwidth: kernel failed"); break; }
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        if (!rc) *gbs = (float)(2.0 * (double)(n * sizeof(fib_v4f)) / (best * 1e-3) / 1e9);   // bytes read + written
    } while (0);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (a) hipFree(a);
    if (b) hipFree(b);
    return rc;
}
