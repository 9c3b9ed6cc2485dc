#!/usr/bin/env python3
"""op_accuracy — per-op accuracy of what the traced-model code generator emits, measured on the device.

Runs the sweeps of tests/test_gpu_traced_ops.py (the op tables and argument sets of tests/op_tables.py) under both
policies and prints, per op: the sample count, the worst error in true ulps against float64 with its argument, the share
of results more than 1 ulp off — for the forms whose accuracy is absolute (tanh under the fast policy, 1 + tanh, sigmoid)
the worst absolute error in units of 2^-24.  The tests keep derived or recorded
bounds; the measured values live in profiles/traced_ops_accuracy.txt:

    python tools/op_accuracy.py > profiles/traced_ops_accuracy.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import op_tables as T  # noqa: E402


def main():
    os.environ['FIBHIP_AUTOTUNE'] = '0'
    os.environ['FIBHIP_MT'] = '0'
    print('# tools/op_accuracy.py: generated code (tests/op_tables.py), one op per output, fused strip kernel, 128 x 512 cells per plane')
    print('# error in true ulps: |got - f64| / 2^(max(floor(log2 |f64|), -126) - 23); absolute error in units of 2^-24')
    for fast in (False, True):
        policy = 'fast ' if fast else 'exact'
        runs = {}
        for table, op, label, fn, dom, *kind in T.ACCURACY:
            if table not in runs:
                x = T.SAMPLES[table]()
                out, info = T.run_device(table, x, fast=fast)
                assert info['plan'] == (2, 1), info
                runs[table] = (x, out)
            x, out = runs[table]
            d = dom(x)
            with np.errstate(all='ignore'):
                want = fn(np.where(d, x.astype(np.float64), 1.0))
            got = out[op][d]
            err = T.ulp_err(got, want[d])
            i = int(np.argmax(err))
            ab = np.abs(got.astype(np.float64) - want[d]) / 2.0 ** -24
            j = int(np.argmax(ab))
            line = '%s  %-18s %8d samples: ' % (policy, label, int(d.sum()))
            if kind:            # a sum or a difference near 0: the form's accuracy is absolute, ulps of the result say nothing
                line += 'worst absolute error %6.3f x 2^-24 at x = %-16.9g' % (ab[j], x[d][j])
                if label == 'tanh':
                    line += ' worst %9.3f ulp at x = %.9g' % (err[i], x[d][i])
            else:
                line += 'worst %7.3f ulp at x = %-16.9g above 1 ulp: %8.4f %%' % (err[i], x[d][i], 100.0 * float(np.mean(err > 1.0)))
            print(line)
            sys.stdout.flush()


if __name__ == '__main__':
    main()
