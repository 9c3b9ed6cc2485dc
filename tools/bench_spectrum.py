"""cost of the spectrum recorder (fib_tf_amd/spectrum.py, csrc/record_kernels.inc spectrum_*_kernel) against what it replaces:

    python tools/bench_spectrum.py [--ticks K] [--configs fenton512,fenton4096] [--strides 1,10] [--nfft N] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON
line.  Every wall figure is host time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by
the call that makes the result visible; best of 3, the recorder attached outside the clock:
  none_us / none_again_us   no recorder, a sync() at the end; measured before and after the other columns
  device_us[shape][stride]  SpectrumRecorder at that stride, samples() at the end (everything stays on the device); shape
                            'full' = full resolution, 'mean4x4' = under a 4 x 4 mean; the default band (indices 2 .. nfft / 2)
  fold_kernel_us[shape]     spectrum_fold_kernel alone, median of its HIP-event-bracketed launches (fibhip_trace_begin/_end),
                            beside fold_bytes[shape], the bytes one fold must move — (chunk * 4 + nb * 16) per pixel, plus 8 per
                            bin at a segment end — and copy_us[shape], copy_kernel moving that many bytes at the rate
                            fibhip_copy_bandwidth measures in this run
  cube_fft_us[stride]       the alternative: a float32 FrameRecorder at full resolution at that stride, its cube read back and
                            numpy.fft.rfft over the same segments, |.|^2 summed (the same wall clock, the transform included;
                            null where the cube would not fit the budget --cube-mib)
  launch_stats              (structural) launches and multi-tick launches of the stride-10 full-resolution run
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fib_tf_amd import _lib  # noqa: E402
from bench_activation import CONFIGS, make  # noqa: E402
from bench_electrodes import wall  # noqa: E402

SHAPES = {'full': dict(block=(1, 1)), 'mean4x4': dict(block=(4, 4))}


def one(name, ticks, strides, nfft, cube_mib):
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

    def cube_fft(rec):
        for _ in range(ticks):
            st.step(1)
        cube = rec.frames()
        segs = len(cube) // nfft
        P = np.zeros((nfft // 2 + 1,) + cube.shape[1:], np.float32)
        w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)[:, None, None]
        for g in range(segs):
            P += np.abs(np.fft.rfft(cube[g * nfft:(g + 1) * nfft] * w, axis=0)) ** 2
        return P

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'nfft': nfft, 'none_us': wall(none, ticks), 'device_us': {}, 'fold_kernel_us': {},
           'fold_bytes': {}, 'copy_us': {}, 'copy_gbs': {}, 'cube_fft_us': {}}
    for shape, kw in SHAPES.items():
        out['device_us'][shape] = {}
        for s in strides:
            stats = {}

            def attach(s=s, kw=kw):
                stats['before'] = st.launch_stats()
                return m.record_spectrum(every=s, nfft=nfft, **kw)

            def detach(rec):
                stats['after'] = st.launch_stats()
                rec.close()
            out['device_us'][shape][str(s)] = wall(device, ticks, before=attach, after=detach)
            if s == 10 and shape == 'full':
                out['launch_stats'] = {k: stats['after'][k] - stats['before'][k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    for s in strides:
        frames = ticks // s
        if frames < nfft or frames * n * n * 4 > cube_mib << 20:
            out['cube_fft_us'][str(s)] = None
            continue
        out['cube_fft_us'][str(s)] = wall(cube_fft, ticks, before=lambda s=s: m.record_frames(every=s, capacity=ticks // s, weight=None),
                                          after=lambda rec: rec.close())
    out['none_again_us'] = wall(none, ticks)
    for shape, kw in SHAPES.items():
        with m.record_spectrum(every=1, nfft=nfft, **kw) as rec:
            st.step(rec.chunk)
            st.trace_begin()
            st.step(nfft)                                    # nfft / chunk folds, the last one ends a segment
            ev = st.trace_end()
            oh, ow = rec.shape
            nb, chunk = len(rec.bins), rec.chunk
        out['fold_kernel_us'][shape] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'spectrum_fold_kernel'])), 2)
        moved = oh * ow * (chunk * 4 + nb * 16)              # (the median fold ends no segment)
        out['fold_bytes'][shape] = moved
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
    ap.add_argument('--nfft', type=int, default=128)
    ap.add_argument('--cube-mib', type=int, default=2048)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(',')]
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, strides, args.nfft, args.cube_mib)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
