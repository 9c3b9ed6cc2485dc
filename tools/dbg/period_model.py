#!/usr/bin/env python3
"""period_model.py [W H] — the cost model behind Fenton's exchange-period rows (csrc/launch.hpp S4P).

A multi-tick launch that exchanges its rims every E sub-steps has a rim E - 1 deep, tiles TX = 64 - 2E wide (the 62-column box)
and the lowest tile that still gives every compute unit at most one tile.  A sub-step costs the busiest SIMD's live rows x `row`
cycles (wave w sits on SIMD w mod 4; the box loses one ring of rows per sub-step); a period boundary costs `bnd` cycles.  Printed
per candidate (E, rows per wave R): tile, strips, the busiest SIMD's row-steps per period and the modelled us per 10 sub-steps.

The model is about 10 % low on absolute time and says nothing about how the boundary's cost moves with the rim: it ranks
candidates for measurement (profiles/exchange_period_ab.txt holds what the device said)."""
import math
import sys


def cost(E, R, W=512, H=512, cu=256, row=188, bnd=7200, mhz=2400):
    TX = 64 - 2 * E
    if TX <= 0:
        return None
    tx = math.ceil(W / TX)
    for TY in range(E, 200):
        if tx * math.ceil(H / TY) <= cu:
            break
    else:
        return None
    CY = TY + 2 * (E - 1)
    NW = math.ceil(CY / R)
    if NW > 16:
        return None
    tot = 0
    for st in range(E):
        lo, hi = st, CY - st
        loads = [0] * 4
        for w in range(NW):
            a, b = max(lo, w * R), min(hi, w * R + R)
            if b > a:
                loads[w % 4] += b - a
        tot += max(loads)
    per = (tot * row + bnd) / E
    return dict(E=E, R=R, TX=TX, TY=TY, tiles=tx * math.ceil(H / TY), strips=NW, rowsteps=tot, rows_per_substep=round(tot / E, 2),
                boundaries_per_tick=round(10 / E, 2), us_per_10=round(per * 10 / mhz, 2))


if __name__ == '__main__':
    W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (512, 512)
    for E in range(3, 11):
        for R in (2, 3, 4):
            c = cost(E, R, W, H)
            if c:
                print(c)
