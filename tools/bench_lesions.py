"""cost of a lesion event (fib_tf_amd/lesions.py, csrc/record_kernels.inc lesion_apply_kernel / lesion_prep_kernel):

    python tools/bench_lesions.py [--size N] [--ticks K] [--lesions L] [--repeats R] [--out FILE]

Three figures on one Fenton sheet of N x N cells with a hole, K ticks stepped one call per tick as a driver loop steps and ended
by a sync(), L disc lesions of radius 3 spread evenly over the run:
  (a) program_ms      the lesions from a program on the device (attached before the clock starts)
                      Every run of (a) and (b) starts alike: field and state put back, one untimed tick (the plan is chosen
                      there, not inside the clock), the state put back again
  (b) none_ms         the same handle and run with no program (taken before and after (a): none_ms is their median, the
                      difference of the two is the spread of the run)
  (c) host_route_ms   what changing the geometry cost before: per lesion the whole state read back, the field changed on the
                      host, a new handle with the new field, define(state=...) — every recorder would be detached
Host wall time (time.perf_counter around the loop and its sync), one warm-up run of each, then `repeats` runs, medians.  Beside
them the launch counts of fibhip_launch_stats: the program's run makes the launches of the plain run, two more per event, and
what cutting the multi-tick launches at the events adds (extra_tick_launches).  event_us = (program_ms - none_ms) / L.
The last line written to FILE is the JSON record; the lines above it say how the figures were taken.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(n, phase=None, state=None):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000, 'diff': 1.5})
    if phase is None:
        m.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    else:
        m.phase = phase
    if state is None:
        m.define()
    else:
        m.define(state=dict(zip(m.VAR_NAMES, state)))
    return m


def sites(n, count):
    """disc lesions of radius 3 along the sheet's diagonal band, clear of the hole"""
    return [('disc', n / 8.0 + (n * 3 / 4.0) * i / max(1, count - 1), n / 4.0, 3.0) for i in range(count)]


def run(st, ticks, reset, field, attach=None):
    """one timed run.  Both arms start alike: the field and the state are put back, then ONE tick runs and is waited for before
    the clock starts — fibhip_set_phase drops the launch plan, and the first tick after it chooses the plan again by timing the
    candidate shapes, which is no part of what a lesion costs — and the state is put back once more.  `attach`: called then,
    still in front of the clock (the program's tick 0 is the first timed tick)"""
    st.set_phase(field)
    st.set_state(-1, reset)
    st.step(1)
    st.sync()
    st.set_state(-1, reset)
    if attach:
        attach()
    st.sync()
    s0 = st.launch_stats()
    t0 = time.perf_counter()
    for _ in range(ticks):
        st.step(1)
    st.sync()
    dt = time.perf_counter() - t0
    s1 = st.launch_stats()
    return dt * 1e3, {k: s1[k] - s0[k] for k in ('launches', 'mt_launches', 'mt_ticks')}


def main(argv=None):
    from fib_tf_amd import lesions
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ticks', type=int, default=3000)
    ap.add_argument('--lesions', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lesion_cost.txt'))
    args = ap.parse_args(argv)
    n, ticks, count = args.size, args.ticks, args.lesions
    if n < 32 or ticks < 2 * count or count < 1:
        raise ValueError('bench_lesions: a sheet of at least 32 x 32 cells and at least two ticks per lesion (got %d, %d ticks, %d lesions)' % (n, ticks, count))
    m = make(n)
    st = m._stepper
    st.step(50)
    start = st.get_state(-1)
    field0 = m.phase.copy()
    at = [(i + 1) * ticks // (count + 1) for i in range(count)]
    program = [lesions.Lesion(s, at_tick=t) for s, t in zip(sites(n, count), at)]

    def plain():
        return run(st, ticks, start, field0)

    def programmed():
        box = []
        ms, launches = run(st, ticks, start, field0, lambda: box.append(m.program_lesions(program)))   # the same tissue every repeat
        applied = box[0].applied()
        box[0].end()
        return ms, launches, applied

    def host_route():
        """the run split at every lesion: read-back, new field on the host, new handle, define(state=...)"""
        cur = make(n, field0, start)
        t0 = time.perf_counter()
        done = 0
        for (s, t) in zip(sites(n, count), at):
            cur._stepper.step(t + 1 - done)
            done = t + 1
            state = cur._stepper.get_state(-1)
            field = lesions.apply_host(cur.phase, *lesions.patch(cur, s))
            cur._stepper.close()
            cur = make(n, field, state)
        cur._stepper.step(ticks - done)
        cur._stepper.sync()
        ms = (time.perf_counter() - t0) * 1e3
        cur._stepper.close()
        return ms

    plain()                                               # warm-up: the plan is chosen, the buffers exist
    none_a = [plain() for _ in range(args.repeats)]
    programmed()
    prog_runs = [programmed() for _ in range(args.repeats)]
    m.phase = field0
    none_b = [plain() for _ in range(args.repeats)]
    host_route()
    host = [host_route() for _ in range(args.repeats)]
    st.close()
    none_ms = statistics.median([r[0] for r in none_a + none_b])
    program_ms = statistics.median([r[0] for r in prog_runs])
    host_ms = statistics.median(host)
    none_l, prog_l = none_a[-1][1], prog_runs[-1][1]
    r = {'config': 'fenton%d' % n, 'cells': n * n, 'ticks': ticks, 'lesions': count, 'applied': prog_runs[-1][2], 'repeats': args.repeats,
         'clock': 'time.perf_counter around %d single-tick calls and a sync; medians' % ticks,
         'none_ms': none_ms, 'none_before_ms': statistics.median([r_[0] for r_ in none_a]), 'none_after_ms': statistics.median([r_[0] for r_ in none_b]),
         'program_ms': program_ms, 'event_us': (program_ms - none_ms) * 1e3 / count,
         'host_route_ms': host_ms, 'host_route_per_lesion_ms': (host_ms - none_ms) / count,
         'none_launches': none_l['launches'], 'program_launches': prog_l['launches'],
         'none_mt_launches': none_l['mt_launches'], 'program_mt_launches': prog_l['mt_launches'],
         'extra_tick_launches': prog_l['launches'] - none_l['launches'] - 2 * count}
    lines = ['# tools/bench_lesions.py --size %d --ticks %d --lesions %d --repeats %d' % (n, ticks, count, args.repeats),
             '# Fenton %d x %d with a hole; %d ticks, one fibhip_step call per tick, ended by a sync; %d disc lesions of radius 3' % (n, n, ticks, count),
             '# host wall time (time.perf_counter), one warm-up run of each, then %d runs: medians; before every run of (a) and (b) the field and' % args.repeats,
             '# the state are put back and one untimed tick runs, so that the launch plan is chosen outside the clock',
             '# (a) program_ms: lesions from the program   (b) none_ms: no program, before and after (a)',
             '# (c) host_route_ms: per lesion read-back, new field, new handle, define(state=)',
             '# event_us = (a - b) / lesions; launches from fibhip_launch_stats',
             json.dumps(r)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return r


if __name__ == '__main__':
    main()
