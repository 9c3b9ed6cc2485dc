#!/usr/bin/env python3
"""br_singular_hits.py [--size 192] [--substeps 22000] [--oracle PATH] — how often a Beeler-Reuter sheet stands EXACTLY on
one of the two potentials where the reference's float32 formulas are 0/0 (V == -47.0f: alpha_m; V == -23.0f: the second
quotient of i_K1), and what a sub-step then does to the cell.  CPU only, the oracle only (oracle/fib_oracle.c); --oracle
names another build of it (the parent commit's, for the record in profiles/br_singular_hits.txt).

A sheet at rest with a disc of radius 9 at (37.3, 51.7) set to 10 mV, diff 0.809, dt 0.1, direct gates, one action
potential sub-step by sub-step.  Before each sub-step: the cells whose boundary-enforced potential is exactly -47.0f or
-23.0f.  After it: the cells that went onto a clip bound in that ONE sub-step from well inside — onto V = -85 mV from above
-80, onto V = 25 mV from below 20 (the upstroke beside a stimulus can do that on its own), onto M = 1e-5 from above 1e-3."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--substeps', type=int, default=22000)
    ap.add_argument('--oracle', default=None)
    a = ap.parse_args()
    if a.oracle:
        os.environ['FIB_ORACLE_LIB'] = os.path.abspath(a.oracle)
    import oracle as orc
    N = a.size
    st = np.empty((8, N, N), np.float32)
    for i, x in enumerate((-84.624, 1e-4, 0.01, 0.988, 0.975, 0.003, 0.994, 0.0001)):     # br.py:71-78
        st[i] = x
    r, c = np.mgrid[0:N, 0:N]
    st[0][np.hypot(c - 37.3, r - 51.7) <= 9.0] = 10.0
    S47, S23 = np.float32(-47.0), np.float32(-23.0)
    n47 = n23 = 0
    jumps = {'V -> -85': 0, 'V -> 25': 0, 'M -> 1e-5': 0}
    events = []
    for k in range(a.substeps):
        V0 = orc.enforce_boundary(st[0])
        at47, at23 = V0 == S47, V0 == S23
        new = orc.br_step(st, 0.1, 0.809, None, None, 1)
        assert np.isfinite(new).all()
        j = {'V -> -85': (new[0] == np.float32(-85.0)) & (V0 > -80.0),
             'V -> 25': (new[0] == np.float32(25.0)) & (V0 < 20.0),
             'M -> 1e-5': (new[2] == np.float32(0.00001)) & (st[2] > 1e-3)}
        n47 += int(at47.sum())
        n23 += int(at23.sum())
        for name, m in j.items():
            jumps[name] += int(m.sum())
        for name, m in (('at -47.0f', at47), ('at -23.0f', at23)):
            for cell in np.argwhere(m):
                cell = tuple(int(x) for x in cell)
                events.append('sub-step %5d  cell %-10s %s: V %.6f -> %.6f  M %.6f -> %.6f' % (
                    k, cell, name, V0[cell], new[0][cell], st[2][cell], new[2][cell]))
        st = new
    print('%d x %d, %d sub-steps, oracle %s' % (N, N, a.substeps, a.oracle or 'of this tree'))
    print('cell-sub-steps exactly on -47.0f: %d, on -23.0f: %d' % (n47, n23))
    for name, n in jumps.items():
        print('one-sub-step jumps %-10s: %d' % (name, n))
    for e in events:
        print(e)


if __name__ == '__main__':
    main()
