"""cost of the beat recorder (fib_tf_amd/beats.py, csrc/record_kernels.inc beat_kernel) against what it replaces:

    python tools/bench_beats.py [--ticks K] [--configs fenton512,fenton4096] [--strides 1,10] [--depth D] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON
line.  Every wall figure is host time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by
the call that makes the result visible; best of 3, the recorder attached outside the clock:
  none_us / none_again_us   no recorder, a sync() at the end; measured before and after the other columns
  device_us[shape][stride]  BeatRecorder at that stride, samples() at the end (everything stays on the device); shape
                            'full' = full resolution, 'mean4x4' = under a 4 x 4 mean
  activation_us             the activation recorder (one plain launch per tick, one APD per cell), a sync() at the end
  frames_host_us[stride]    the alternative: a float32 FrameRecorder at full resolution at that stride, its cube read back and
                            the beats detected on the host with NumPy (the two comparisons, the interpolated upstroke and
                            downstroke times of every crossing; no ring is kept) — the same wall clock, the detection included;
                            null where the cube would not fit the budget --cube-mib
  beat_kernel_us[shape]     beat_kernel alone, median of its HIP-event-bracketed launches (fibhip_trace_begin/_end) at stride 1,
                            beside beat_bytes[shape], the bytes one sample must move in the steady state — 20 per pixel at
                            full resolution (x read, xp and pk read and written), 16 + 4 * by * bx under a block —, and
                            copy_us[shape]: copy_kernel moving that many bytes at the rate fibhip_copy_bandwidth measures in
                            this run
  summary_us[shape]         beats_summary's launch and its four read-backs, wall, best of 3
  launch_stats              (structural) launches and multi-tick launches of the stride-10 full-resolution run
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fib_tf_amd import _lib  # noqa: E402
from bench_activation import CONFIGS, make  # noqa: E402
from bench_electrodes import wall  # noqa: E402

SHAPES = {'full': dict(block=(1, 1)), 'mean4x4': dict(block=(4, 4))}


def host_beats(cube, up, down, step):
    """upstroke and downstroke times of every crossing in a [frames, H, W] cube, as the recorder interpolates them"""
    xp, xc = cube[:-1], cube[1:]
    t0 = (np.arange(len(xp), dtype=np.float32) * np.float32(step))[:, None, None]
    with np.errstate(all='ignore'):
        rise = (xp < up) & (xc >= up)
        fall = (xp >= down) & (xc < down)
        t_up = np.where(rise, t0 + (up - xp) / (xc - xp) * np.float32(step), np.float32(np.nan))
        t_down = np.where(fall, t0 + (xp - down) / (xp - xc) * np.float32(step), np.float32(np.nan))
    return t_up, t_down, rise.sum(axis=0)


def one(name, ticks, strides, depth, cube_mib):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()

    def none():
        for _ in range(ticks):
            st.step(1)
        st.sync()

    def device(rec):
        for _ in range(ticks):
            st.step(1)
        assert rec.samples() == ticks // rec.every

    def activation(rec):
        for _ in range(ticks):
            st.step(1)
        assert rec.ticks() == ticks
        st.sync()                                            # (ticks() counts on the host: the stream has to drain inside the clock)

    def frames_host(rec):
        for _ in range(ticks):
            st.step(1)
        cube = rec.frames()
        return host_beats(cube, np.float32(0.5), np.float32(0.1), rec.every * m.dt_per_step * m.dt)

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'depth': depth, 'none_us': wall(none, ticks), 'device_us': {}, 'beat_kernel_us': {},
           'beat_bytes': {}, 'copy_us': {}, 'copy_gbs': {}, 'summary_us': {}, 'frames_host_us': {}}
    for shape, kw in SHAPES.items():
        out['device_us'][shape] = {}
        for s in strides:
            stats = {}

            def attach(s=s, kw=kw):
                rec = m.record_beats(every=s, depth=depth, **kw)
                stats['before'] = st.launch_stats()
                return rec

            def detach(rec):
                stats['after'] = st.launch_stats()
                rec.close()
            out['device_us'][shape][str(s)] = wall(device, ticks, before=attach, after=detach)
            if s == 10 and shape == 'full':
                out['launch_stats'] = {k: stats['after'][k] - stats['before'][k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    out['activation_us'] = wall(activation, ticks, before=lambda: m.record_activation(), after=lambda rec: rec.close())
    for s in strides:
        frames = ticks // s
        if frames * n * n * 4 > cube_mib << 20:
            out['frames_host_us'][str(s)] = None
            continue
        out['frames_host_us'][str(s)] = wall(frames_host, ticks, before=lambda s=s: m.record_frames(every=s, capacity=ticks // s, weight=None),
                                             after=lambda rec: rec.close())
    out['none_again_us'] = wall(none, ticks)
    for shape, kw in SHAPES.items():
        with m.record_beats(every=1, depth=depth, **kw) as rec:
            st.step(4)
            st.trace_begin()
            st.step(64)
            ev = st.trace_end()
            oh, ow = rec.shape
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                rec.summary(last=min(4, depth))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            out['summary_us'][shape] = round(best * 1e6, 1)
        out['beat_kernel_us'][shape] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'beat_kernel'])), 2)
        by, bx = kw['block']
        moved = oh * ow * (16 + 4 * by * bx)
        out['beat_bytes'][shape] = moved
        gbs = _lib.copy_bandwidth(nbytes=max(moved // 2 // 16 * 16, 1 << 20), reps=20, device=0)     # a copy reads and writes its size
        out['copy_gbs'][shape] = round(float(gbs), 1)
        out['copy_us'][shape] = round(moved / (gbs * 1e9) * 1e6, 2)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=1280)
    ap.add_argument('--configs', default='fenton512')
    ap.add_argument('--strides', default='1,10')
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--cube-mib', type=int, default=2048)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(',')]
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, strides, args.depth, args.cube_mib)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
