"""cost of the frame recorder (fib_tf_amd/frames.py, csrc/record_kernels.inc frame_kernel) against polling:

    python tools/bench_frames.py [--ticks K] [--configs fenton512,fenton4096,br512] [--strides 1,10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON
line.  Every figure is host wall time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by
the call that makes the result visible; best of 3, the recorder attached outside the clock:
  none_us / none_again_us   no recorder, a sync() at the end; measured before and after the other columns
  device_us[shape][stride]  FrameRecorder at that stride, count() at the end (the cube stays on the device); shape 'f32' =
                            float32 at full resolution, 'u8_2x2' = 8-bit grey under a 2 x 2 mean
  polled_us[stride]         polling: image() * phase at the same ticks, the way run(im) paints
  frame_kernel_us[shape]    the kernel alone, median of its HIP-event-bracketed launches (fibhip_trace_begin/_end)
  copy_us[shape]            copy_kernel moving the bytes frame_kernel reads and writes (state window + weight plane + frame),
                            at the rate fibhip_copy_bandwidth measures in this run for that many bytes
  launch_stats              (structural) launches and multi-tick launches of the stride-10 float32 run
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_frames.py ...` the profiler's own frame_kernel time is the figure
DESIGN.md section 13 quotes.  One process; stops at the first failure.
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

SHAPES = {'f32': dict(block=(1, 1), fmt='float32'), 'u8_2x2': dict(block=(2, 2), fmt='uint8')}


def one(name, ticks, strides):
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
        assert rec.count() == rec.capacity

    def polled(stride):
        def run():
            for i in range(ticks):
                st.step(1)
                if (i + 1) % stride == 0:
                    image = m.image()
                    if m.phase is not None:
                        image *= m.phase
            st.sync()
        return run

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'device_us': {}, 'polled_us': {},
           'frame_kernel_us': {}, 'copy_us': {}, 'copy_gbs': {}}
    for shape, kw in SHAPES.items():
        out['device_us'][shape] = {}
        for s in strides:
            stats = {}

            def attach(s=s, kw=kw):
                stats['before'] = st.launch_stats()
                return m.record_frames(every=s, capacity=ticks // s, **kw)

            def detach(rec):
                stats['after'] = st.launch_stats()
                rec.close()
            out['device_us'][shape][str(s)] = wall(device, ticks, before=attach, after=detach)
            if s == 10 and shape == 'f32':
                out['launch_stats'] = {k: stats['after'][k] - stats['before'][k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    for s in strides:
        out['polled_us'][str(s)] = wall(polled(s), ticks)
    out['none_again_us'] = wall(none, ticks)
    weighted = m.phase is not None
    for shape, kw in SHAPES.items():
        with m.record_frames(every=1, capacity=52, **kw) as rec:
            st.step(1)
            st.trace_begin()
            st.step(50)
            ev = st.trace_end()
            oh, ow = rec.shape
            frame_bytes = oh * ow * rec.dtype.itemsize
        out['frame_kernel_us'][shape] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'frame_kernel'])), 2)
        moved = n * n * 4 * (2 if weighted else 1) + frame_bytes      # the state window, the weight plane, the frame
        gbs = _lib.copy_bandwidth(nbytes=moved // 2 // 16 * 16, reps=20, device=0)     # a copy reads and writes its size
        out['copy_gbs'][shape] = round(float(gbs), 1)
        out['copy_us'][shape] = round(moved / (gbs * 1e9) * 1e6, 2)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512,fenton4096,br512')
    ap.add_argument('--strides', default='1,10')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(',')]
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, strides)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
