"""the wave recorder's links without a device: the restatement (tests/wave_link_ref.py) on literal planes, `waves.events` and
`waves.track` on literal sequences, the crafted frames the device tests play, the declarations, the bindings, the Python guards,
and — by the reference alone, on the CPU oracle — that the dynamic run the device tests use does contain splits and merges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_link_ref as lref  # noqa: E402
import wave_ref as ref  # noqa: E402
from test_waves_cpu import TILE, _Model, checkerboard  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('fibhip_waves_links_begin', 'fibhip_waves_links_read')


# ---- the crafted frames (shared with tests/test_gpu_wave_links.py) -----------------------------------------------------------
def interior(H, W):
    """everything but the outer ring of the grid (the ghost copies): the mask the crafted device tests give the recorder"""
    m = np.zeros((H, W), bool)
    m[1:-1, 1:-1] = True
    return m


def bars(H, W, spans):
    """bands across the interior's shorter side, each [a, b) along its longer side (interior coordinates)"""
    s = np.zeros((H, W), bool)
    for a, b in spans:
        if H >= W:
            s[1 + a:1 + b, 1:-1] = True
        else:
            s[1:-1, 1 + a:1 + b] = True
    return s


def cells(H, W, where):
    s = np.zeros((H, W), bool)
    for r, c in where:
        s[r, c] = True
    return s


def frames(H, W):
    """[(name, plane)]: the sequence of set planes of a crafted run, none with a cell on the outer ring.  n: the interior's
    longer side.  Three separate waves need n >= 5, so the 5 x 3 grid (a column of three cells) plays what fits"""
    n = max(H, W) - 2
    full, empty = interior(H, W), np.zeros((H, W), bool)
    out = [('empty', empty), ('full', full), ('empty again', empty)]
    if n < 9:
        assert (H, W) == (5, 3)
        col = lambda rows: cells(H, W, [(r, 1) for r in rows])  # noqa: E731
        out += [('one', col([1, 2])), ('moved', col([2, 3])), ('gone', empty), ('two', col([1, 3])), ('merged', col([1, 2, 3])),
                ('split in two', col([1, 3])), ('one dies', col([3])), ('a birth beside it', col([1, 3]))]
    else:
        a = n // 3
        out += [('a bar', bars(H, W, [(0, a)])), ('moved', bars(H, W, [(1, a + 1)])),
                ('a birth beside it', bars(H, W, [(1, a + 1), (n - 2, n)])), ('merged', bars(H, W, [(1, n)])),
                ('split in three', bars(H, W, [(1, a), (a + 1, 2 * a), (2 * a + 1, n)])),
                ('the middle dies', bars(H, W, [(1, a), (2 * a + 1, n)])), ('gone', empty)]
    ty, tx = TILE
    if H > 3 * ty + 8 and W > tx + 2:
        # two waves whose only common cell, (50, 5) in tile (3, 0), lies in another tile than either seed: (1, 5) in tile (0, 0)
        # and (17, 64) in tile (1, 1)
        p = cells(H, W, [(r, 5) for r in range(1, 56)])
        q = cells(H, W, [(17, 64), (17, 65)] + [(r, 65) for r in range(17, 51)] + [(50, c) for c in range(5, 66)])
        out += [('far from its seed', p), ('far from both seeds', q), ('gone', empty)]
        # the two diagonal pairs at the corner of four tiles: one wave under conn = 8, two under conn = 4
        d, ad = cells(H, W, [(ty - 1, tx - 1), (ty, tx)]), cells(H, W, [(ty - 1, tx), (ty, tx - 1)])
        out += [('corner diagonal', d), ('corner diagonal stays', d), ('corner anti-diagonal', ad), ('corner anti-diagonal stays', ad)]
    for name, plane in out:
        assert not (plane & ~full).any(), name
    return out


def what_happens(H, W, conn):
    """the reference's own account of frames(H, W): (samples, event rows, the set of things seen)"""
    samples = lref.sequence([p for _, p in frames(H, W)], conn)
    seeds, links = lref.lists_of(samples)
    rows = lref.events(seeds, links)
    seen = set()
    for s, (n, births, deaths, splits, merges, cont) in enumerate(rows):
        if s == 0 and samples[0][3].tolist() == [0, 0, 0, 0]:
            seen.add('sample 0 without links')
        if births:
            seen.add('birth')
        if deaths:
            seen.add('death')
        if cont and s and not np.array_equal(samples[s][2], samples[s - 1][2]):
            moved = [(p, q) for p, q, o in links[s] if p != q]
            if moved:
                seen.add('a continuation that moves')
        dplus, dminus = {}, {}
        for p, q, o in links[s]:
            dplus[p] = dplus.get(p, 0) + 1
            dminus[q] = dminus.get(q, 0) + 1
        if 2 in dminus.values():
            seen.add('a merge of two')
        if 3 in dplus.values():
            seen.add('a split into three')
        if 2 in dplus.values():
            seen.add('a split into two')
    cellcount = [int(r[0][2]) for r in samples]
    area = (H - 2) * (W - 2)
    if any(cellcount[i:i + 3] == [0, area, 0] for i in range(len(cellcount))):
        seen.add('empty, full, empty')
    return samples, rows, seen


EVERYWHERE = {'sample 0 without links', 'birth', 'death', 'a continuation that moves', 'a merge of two', 'empty, full, empty'}


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', [(5, 3), (4, 64), (37, 53), (64, 64), (130, 67)], ids=lambda s: '%dx%d' % s)
def test_crafted_frames_contain_what_they_claim(shape, conn):
    H, W = shape
    samples, rows, seen = what_happens(H, W, conn)
    want = EVERYWHERE | ({'a split into two'} if shape == (5, 3) else {'a split into three'})
    assert want <= seen, (want - seen, rows)
    if shape == (130, 67):
        names = [n for n, _ in frames(H, W)]
        s = names.index('far from both seeds')
        assert samples[s][4].tolist() == [(1 * W + 5, 17 * W + 64, 1)]
        tile = lambda i: (i // W // TILE[0], i % W // TILE[1])  # noqa: E731
        assert len({tile(1 * W + 5), tile(17 * W + 64), tile(50 * W + 5)}) == 3
        s = names.index('corner diagonal stays')
        assert len(samples[s][4]) == (2 if conn == 4 else 1) and len(samples[s + 2][4]) == (2 if conn == 4 else 1)
        assert len(samples[s + 1][4]) == 0                   # (the two diagonals share no cell)


# ---- the restatement on literal planes ---------------------------------------------------------------------------------------
def test_links_of_literal_planes():
    a = np.array([[0, 0, -1, 3],
                  [0, -1, -1, 3],
                  [-1, -1, 10, -1]], np.int32)
    b = np.array([[0, -1, 2, 2],
                  [0, -1, -1, 2],
                  [8, 8, -1, -1]], np.int32)
    counts, rec = lref.links(a, b)
    assert counts.tolist() == [2, 2, 4, 0]
    assert rec.tolist() == [(0, 0, 2), (3, 2, 2)]
    counts, rec = lref.links(b, a)
    assert counts.tolist() == [2, 2, 4, 0] and rec.tolist() == [(0, 0, 2), (2, 3, 2)]
    counts, rec = lref.links(None, a)
    assert counts.tolist() == [0, 0, 0, 0] and len(rec) == 0
    counts, rec = lref.links(a, b, max_links=1)
    assert counts.tolist() == [2, 1, 4, 0] and len(rec) == 2
    # one wave before, three after, and a fourth that touches nothing
    a = np.array([[0, 0, 0, 0, 0, -1, -1]], np.int32)
    b = np.array([[0, -1, 2, -1, 4, -1, 6]], np.int32)
    assert lref.links(a, b)[1].tolist() == [(0, 0, 1), (0, 2, 1), (0, 4, 1)]
    dev = np.array([(3, 2, 2), (0, 0, 2), (9, 9, 9)], lref.LINK_DTYPE)
    assert lref.sorted_links(dev, 2).tolist() == [(0, 0, 2), (3, 2, 2)]


def test_sequence_of_set_planes():
    planes = [np.array([[1, 1, 0, 0, 0]], bool), np.array([[0, 1, 1, 0, 1]], bool), np.array([[0, 0, 0, 0, 0]], bool)]
    s = lref.sequence(planes)
    assert [r[3].tolist() for r in s] == [[0, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    assert s[1][4].tolist() == [(0, 1, 1)]
    assert lref.lists_of(s) == ([[0], [1, 4], []], [[], [(0, 1, 1)], []])


# ---- events and tracks on literal sequences ----------------------------------------------------------------------------------
def _lists(seeds, links, dt=2.0):
    """what WaveRecorder.waves() and .links() would return for these seeds and (prev, seed, overlap) lists"""
    from fib_tf_amd import waves
    W, L = [], []
    for s, (Q, K) in enumerate(zip(seeds, links)):
        w = np.zeros(len(Q), waves.WAVE_DTYPE)
        w['t_ms'] = (s + 1) * dt
        w['seed'] = Q
        w['area'] = [10 + q for q in Q]
        w['cy'] = [q // 10 for q in Q]
        w['cx'] = [q % 10 for q in Q]
        W.append(w)
        k = np.zeros(len(K), waves.LINK_DTYPE)
        k['t_ms'] = (s + 1) * dt
        for i, (p, q, o) in enumerate(K):
            k[i] = ((s + 1) * dt, p, q, o)
        L.append(k)
    return W, L


SEQUENCE = ([[5, 40],                     # two waves at the start
             [5, 40, 77],                 # 77 is born
             [6, 41],                     # 77 dies; the others move on
             [6, 12, 30, 41],             # 6 splits into three
             [6, 30],                     # 6 and 12 merge; 41 dies
             [3, 9, 30],                  # 6 splits into 3 and 9, and 9 takes 30's cells too, while 30 goes on: a split and a merge
             []],
            [[],
             [(5, 5, 9), (40, 40, 7)],
             [(5, 6, 8), (40, 41, 1)],
             [(6, 6, 3), (6, 12, 2), (6, 30, 2), (41, 41, 5)],
             [(6, 6, 3), (12, 6, 2), (30, 30, 2)],
             [(6, 3, 2), (6, 9, 1), (30, 9, 1), (30, 30, 4)],
             []])
#            waves births deaths splits merges continued
ROWS = [(2, 0, 0, 0, 0, 0),
        (3, 1, 0, 0, 0, 2),
        (2, 0, 1, 0, 0, 2),
        (4, 0, 0, 1, 0, 1),
        (2, 0, 1, 0, 1, 1),
        (3, 0, 0, 2, 1, 0),
        (0, 0, 3, 0, 0, 0)]


def test_events_on_a_literal_sequence():
    from fib_tf_amd import waves
    seeds, links = SEQUENCE
    assert lref.events(seeds, links) == ROWS
    W, L = _lists(seeds, links)
    ev = waves.events(W, L)
    assert ev.dtype.names == ('t_ms', 'waves', 'births', 'deaths', 'splits', 'merges', 'continued')
    assert [tuple(int(x) for x in list(r)[1:]) for r in ev] == ROWS
    assert ev['t_ms'][:6].tolist() == [2.0, 4.0, 6.0, 8.0, 10.0, 12.0] and np.isnan(ev['t_ms'][6])
    assert waves.events(W, L, times_ms=2.0 * np.arange(1, 8))['t_ms'][6] == 14.0
    # min_overlap = 2 drops (40, 41, 1), (6, 9, 1) and (30, 9, 1): 41 is a birth and 40 a death, 9 a birth, no merge in row 5
    want = list(ROWS)
    want[2] = (2, 1, 2, 0, 0, 1)
    want[5] = (3, 1, 0, 0, 0, 2)
    assert lref.events(seeds, links, 2) == want
    assert [tuple(int(x) for x in list(r)[1:]) for r in waves.events(W, L, min_overlap=2)] == want


def test_tracks_on_a_literal_sequence():
    from fib_tf_amd import waves
    seeds, links = SEQUENCE
    W, L = _lists(seeds, links)
    tr = waves.track(W, L)
    want = lref.tracks(seeds, links)
    assert len(tr) == len(want) == 10
    for t, w in zip(tr, want):
        assert (t.id, t.born, t.ended, t.parents, t.children) == (w['id'], w['born'], w['ended'], w['parents'], w['children']), (t, w)
        assert [(round(p['t_ms'] / 2.0) - 1, int(p['seed'])) for p in t.points] == w['path'], (t, w)
        assert t.points.dtype.names == ('t_ms', 'seed', 'area', 'cy', 'cx')
    # ... and by hand: (born, ended, parents, children, seeds along the way)
    by_hand = [('start', 'split', [], [3, 4, 5], [5, 5, 6]), ('start', 'death', [], [], [40, 40, 41, 41]), ('birth', 'death', [], [], [77]),
               ('split', 'merge', [0], [6], [6]), ('split', 'merge', [0], [6], [12]), ('split', 'split', [0], [8, 9], [30, 30]),
               ('merge', 'split', [3, 4], [7, 8], [6]), ('split', 'death', [6], [], [3]), ('merge', 'death', [5, 6], [], [9]),
               ('split', 'death', [5], [], [30]), ]
    assert len(tr) == len(by_hand)
    for t, (born, ended, parents, children, path) in zip(tr, by_hand):
        assert (t.born, t.ended, t.parents, t.children, t.points['seed'].tolist()) == (born, ended, parents, children, path), t
    assert tr[1].lifetime_ms == 6.0 and tr[2].lifetime_ms == 0.0 and tr[0].points['area'].tolist() == [15, 15, 16]
    # a track that is alive at the last sample ends with 'end'
    tr = waves.track(W[:2], L[:2])
    assert [(t.born, t.ended) for t in tr] == [('start', 'end'), ('start', 'end'), ('birth', 'end')]


def test_a_cut_list_is_refused():
    from fib_tf_amd import waves
    seeds, links = SEQUENCE
    W, L = _lists(seeds, links)
    wc = np.array([[len(w), len(w), 50] for w in W], np.int32)
    lc = np.array([[len(k), len(k), 40, 0] for k in L], np.int32)
    assert len(waves.events(W, L, wave_counts=wc, link_counts=lc)) == 7 and len(waves.track(W, L, wave_counts=wc, link_counts=lc)) == 10
    for f in (waves.events, waves.track):
        cut = wc.copy()
        cut[3] = (5, 4, 50)
        with pytest.raises(ValueError, match='sample 3: the wave list was cut'):
            f(W, L, wave_counts=cut, link_counts=lc)
        cut = lc.copy()
        cut[4] = (4, 3, 40, 0)
        with pytest.raises(ValueError, match='sample 4: the link list was cut'):
            f(W, L, wave_counts=wc, link_counts=cut)
        cut = lc.copy()
        cut[5, 3] = 2
        with pytest.raises(ValueError, match='sample 5: the link list was cut'):
            f(W, L, wave_counts=wc, link_counts=cut)
        # without counts: a link that names a wave no list holds
        with pytest.raises(ValueError, match='sample 3: the link .* names a wave'):
            f(W[:3] + [W[3][:3]] + W[4:], L)
        with pytest.raises(ValueError, match='sample 0: the first sample has no links'):
            f(W, [L[1]] + L[1:])


# ---- declarations, bindings, guards ------------------------------------------------------------------------------------------
def test_declarations_and_binding():
    from fib_tf_amd import _lib, waves
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in ENTRY_POINTS:
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert len(_lib.SYMBOLS['fibhip_waves_links_begin'][0]) == 2 and len(_lib.SYMBOLS['fibhip_waves_links_read'][0]) == 5
    assert len(_lib.SYMBOLS['fibhip_waves_begin'][0]) == 12
    assert '#define FIBHIP_MAX_WAVE_LINKS %d\n' % _lib.MAX_WAVE_LINKS in src and _lib.MAX_WAVE_LINKS == 65536
    assert 'typedef struct { int prev, seed, overlap; } fibhip_wave_link;' in src
    assert _lib.WAVE_LINK_DTYPE.itemsize == 12 and _lib.WAVE_LINK_DTYPE == lref.LINK_DTYPE
    for s in ('waves_links_begin', 'waves_links_read'):
        assert callable(getattr(_lib.Stepper, s))
    for s in ('links', 'link_counts', 'links_raw', 'links_truncated', 'events', 'tracks'):
        assert callable(getattr(waves.WaveRecorder, s))


def test_library_exports_the_entry_points():
    from fib_tf_amd import _lib
    L = _lib.C.CDLL(_lib.SO)
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None, name


class _Quiet:
    """a stand-in for the handle that attaches anything and knows nothing"""
    def waves_begin(self, *a):
        pass

    def waves_links_begin(self, *a):
        raise AssertionError('links were asked of the library')

    def waves_links_read(self, *a, **k):
        raise AssertionError('links were read from the library')

    def waves_end(self):
        pass


def test_python_guards():
    """nothing reaches the library"""
    from fib_tf_amd import waves
    from fib_tf_amd.sharded import ShardedStepper
    for bad in (0, -1, 65537):
        with pytest.raises(ValueError, match='max_links is 1 .. 65536'):
            waves.WaveRecorder(_Model, links=True, max_links=bad)

    class Sharded(_Model):
        _stepper = ShardedStepper.__new__(ShardedStepper)
    Sharded._stepper.world = 2
    with pytest.raises(NotImplementedError, match='single device'):
        waves.WaveRecorder(Sharded, links=True)

    class Plain(_Model):
        _stepper = _Quiet()
    rec = waves.WaveRecorder(Plain)                          # links=False: the library is not asked for links
    assert rec.max_links == 0
    for call in (rec.links, rec.link_counts, rec.links_raw, rec.links_truncated, rec.events, rec.tracks):
        with pytest.raises(ValueError, match='keeps no links'):
            call()
    rec.close()
    with pytest.raises(AssertionError, match='links were asked of the library'):     # (the default: 2 * max_waves, capped)
        waves.WaveRecorder(Plain, links=True)

    class Asked(_Quiet):
        def waves_links_begin(self, n):
            self.n = n

    class Counting(_Model):
        _stepper = Asked()
    assert waves.WaveRecorder(Counting, links=True, max_waves=100).max_links == 200 and Counting._stepper.n == 200
    assert waves.WaveRecorder(Counting, links=True, max_waves=65536).max_links == 65536
    assert waves.WaveRecorder(Counting, links=True, max_links=7).max_links == 7


# ---- the dynamic run of the device tests, by the reference alone ------------------------------------------------------------
DYN_TICKS = 70


def oracle_planes(H, W):
    """the set planes behind each of DYN_TICKS ticks of the run tests/test_gpu_wave_links.py records — Fenton, diff 1.5, the hole
    of test_gpu_waves.fenton_hole, define()'s initial state under test_gpu_waves.blobs — on the CPU oracle, under the recorder's
    default mask (phase > 0.5, the ring cleared) and level (0.5)"""
    import oracle
    from test_gpu_waves import blobs
    cols, rows = np.arange(W)[np.newaxis, :] - (W - 14), np.arange(H)[:, np.newaxis] - (H - 14)
    phase = np.maximum(np.array(0.5 * (np.tanh(np.hypot(cols, rows) - 5) + 1.0), dtype=np.float32), 1e-5)      # add_hole_to_phase_field
    state = np.stack([np.zeros((H, W), np.float32), np.ones((H, W), np.float32), np.ones((H, W), np.float32), np.zeros((H, W), np.float32)])
    state[0][:, 1] = 1.0
    state = np.ascontiguousarray(blobs(H, W, state))
    mask = (phase > 0.5) & interior(H, W)
    planes = []
    for _ in range(DYN_TICKS):
        oracle.fenton_run(state, 0.1, 1.5, phase, 10)
        planes.append(ref.set_plane(state[0], 0.5, 'above', mask))
    return planes


_LABELS = {}


def oracle_events(shape, every):
    """(event rows, link lists) of the oracle's run sampled every `every` ticks"""
    if shape not in _LABELS:
        _LABELS[shape] = [ref.sample(p, 4) for p in oracle_planes(*shape)]
    taken = _LABELS[shape][every - 1::every]
    seeds = [r[1]['seed'].tolist() for r in taken]
    links, before = [], None
    for r in taken:
        rec = lref.links(before, r[2])[1]
        links.append([(int(p), int(q), int(o)) for p, q, o in rec.tolist()])
        before = r[2]
    return lref.events(seeds, links), links


# splits, merges, deaths, births, the most links in a sample, samples with two links or more: what the run held when it was chosen
ADEQUATE = {((64, 64), 1): (1, 2, 1, 0, 3, 11), ((130, 67), 1): (2, 2, 1, 0, 3, 18),
            ((130, 67), 7): (1, 1, 0, 0, 0, 0), ((130, 67), 10): (1, 1, 0, 0, 0, 0)}


@pytest.mark.parametrize('case', sorted(ADEQUATE), ids=lambda c: '%dx%d-every-%d' % (c[0] + (c[1],)))
def test_the_dynamic_run_has_splits_and_merges(case):
    shape, every = case
    rows, links = oracle_events(shape, every)
    got = (sum(r[3] for r in rows), sum(r[4] for r in rows), sum(r[2] for r in rows), sum(r[1] for r in rows),
           max(len(k) for k in links), sum(1 for k in links if len(k) >= 2))
    print('%s every %d: splits %d merges %d deaths %d births %d, at most %d links, %d samples with >= 2' % ((shape, every) + got))
    assert all(g >= w for g, w in zip(got, ADEQUATE[case])), (got, ADEQUATE[case])


def test_checkerboard_behind_a_full_plane():
    """the planes of the device's cut tests: one wave before, every other cell of the interior a wave of one cell after"""
    H, W = 37, 53
    s = lref.sequence([interior(H, W), checkerboard(H, W) & interior(H, W)], 4)
    n = int((checkerboard(H, W) & interior(H, W)).sum())
    assert s[1][3].tolist() == [n, n, n, 0] and set(s[1][4]['prev'].tolist()) == {W + 1} and set(s[1][4]['overlap'].tolist()) == {1}
