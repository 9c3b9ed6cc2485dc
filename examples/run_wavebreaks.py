#!/usr/bin/env python3
"""Wavebreaks of a spiral wave: the Fenton 4-variable sheet with a circular obstacle, S1 from the left edge, S2 in the upper-left
quadrant.  Every `--every` ticks the device labels the excited domains and links them to the domains of the sample before
(fib_tf_amd/waves.py, `links=True`); nothing is read back between the samples.  From the links the host counts, per sample, the
waves that split (wavebreak), merged (coalescence), were born and died, and follows every wave from its first sample to its
last.  The PNG shows, through the headless Screen, on top the wavelet count (bright) with the cumulative splits + births and
merges + deaths (dim) over time, in the middle the four event rates per `--window` ms (splits, merges, births, deaths, bright
to dim), and at the bottom a histogram of the waves' lifetimes.

    python examples/run_wavebreaks.py [--size N] [--ms T] [--every K] [--window MS] [--out FILE]

Choose --every so that a wave overlaps itself from one sample to the next: a front thinner than its travel per sample reads as
a death beside a birth.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen


def steps(panel, values, top, grey):
    """draws the series `values` left to right into the [h, w] panel, `top` at its upper edge"""
    h, w = panel.shape
    if len(values) == 0:
        return
    cols = np.linspace(0, w - 1, len(values)).astype(int)
    rows = (h - 1) * (1.0 - np.minimum(np.asarray(values, np.float64), top) / max(top, 1e-30))
    panel[rows.astype(int), cols] = grey


def bars(panel, values, grey):
    """a histogram: one bar per value across the [h, w] panel, the largest value at its upper edge"""
    h, w = panel.shape
    top = max(float(np.max(values)), 1.0) if len(values) else 1.0
    for k, v in enumerate(values):
        c0, c1 = k * w // len(values), max((k + 1) * w // len(values) - 1, k * w // len(values) + 1)
        panel[h - 1 - int((h - 1) * v / top):, c0:c1] = grey


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--ms', type=float, default=600.0)
    ap.add_argument('--every', type=int, default=5)
    ap.add_argument('--window', type=float, default=50.0)
    ap.add_argument('--out', default='wavebreaks.png')
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': args.ms})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    with sheet.record_waves(every=args.every, links=True) as waves:
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        if waves.count() == 0:
            print('no sample was taken (--ms shorter than --every ticks)')
            return None
        cut = waves.links_truncated()
        if len(cut) or len(waves.truncated()):
            print('%d samples have more waves or links than the lists hold: raise max_waves / max_links' % (len(cut) + len(waves.truncated())))
            return None
        ev = waves.events()
        tracks = waves.tracks()
    t = ev['t_ms']
    lifetimes = np.array([k.lifetime_ms for k in tracks if k.ended != 'end'])
    print('%d samples up to %.1f ms, up to %d waves at a time: %d splits, %d merges, %d births, %d deaths; %d tracks, %d of them ended, '
          'median lifetime %.1f ms' % (len(t), t[-1], ev['waves'].max(), ev['splits'].sum(), ev['merges'].sum(), ev['births'].sum(),
                                       ev['deaths'].sum(), len(tracks), len(lifetimes), np.median(lifetimes) if len(lifetimes) else 0.0))
    # the rates: events per window, at every sample (a running sum over the samples of the last `window` ms)
    per = max(1, int(round(args.window / (t[1] - t[0])))) if len(t) > 1 else 1
    kernel = np.ones(per)
    rate = {k: np.convolve(ev[k].astype(np.float64), kernel)[:len(t)] for k in ('splits', 'merges', 'births', 'deaths')}
    h, w = 64, max(n, 256)
    frame = np.full((3 * h + 2, w), 0.1, np.float32)
    made, gone = np.cumsum(ev['splits'] + ev['births']), np.cumsum(ev['merges'] + ev['deaths'])
    top = max(int(ev['waves'].max()), int(made.max()), int(gone.max()), 1)
    steps(frame[:h], made, top, 0.5)
    steps(frame[:h], gone, top, 0.35)
    steps(frame[:h], ev['waves'], top, 1.0)
    frame[h] = 0.0
    top = max(max(float(r.max()) for r in rate.values()), 1.0)
    for k, grey in (('deaths', 0.3), ('births', 0.5), ('merges', 0.7), ('splits', 1.0)):
        steps(frame[h + 1:2 * h + 1], rate[k], top, grey)
    frame[2 * h + 1] = 0.0
    hist = np.histogram(lifetimes, bins=32, range=(0.0, max(float(t[-1]), 1.0)))[0] if len(lifetimes) else np.zeros(32)
    bars(frame[2 * h + 2:], hist, 0.8)
    screen = Screen(frame.shape[0], frame.shape[1], 'waves, made and gone; splits, merges, births, deaths per %g ms; lifetimes' % args.window)
    screen.imshow(frame)
    screen.save(args.out)
    print('written to %s' % args.out)
    return ev, tracks


if __name__ == '__main__':
    main()
