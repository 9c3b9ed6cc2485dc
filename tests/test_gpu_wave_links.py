"""-m gpu: the wave recorder's links (include/fibhip.h fibhip_waves_links_*, fib_tf_amd/waves.py) on the device.

Links are integer arithmetic on two label planes, so counts, records (sorted by (prev, seed)) and `events()` must EQUAL the
restatement (tests/wave_link_ref.py).  Crafted sequences are played through the state: a Fenton handle without diffusion, U set
to the crafted plane in front of every tick (V = W = 1, S = 0) and read back behind it — the reference is taken from what was
read back, and the test asserts that this IS the crafted plane.  The recorder's mask clears the outer ring, which takes ghost
copies.  On the dynamics the reference is computed from the states polled at the sample ticks."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_link_ref as lref  # noqa: E402
import wave_ref as ref  # noqa: E402
from test_gpu_frames import wave  # noqa: E402
from test_gpu_waves import DYN_GRIDS, DYN_TICKS, FORCED, blobs, fenton_hole, plan_env, raw_stepper  # noqa: E402
from test_wave_links_cpu import ADEQUATE, EVERYWHERE, frames, interior, what_happens  # noqa: E402
from test_waves_cpu import checkerboard  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(5, 3), (4, 64), (37, 53), (64, 64), (130, 67)]
ROOMY = 8192                                                  # more records than any plane here has waves or links


def crafted_stepper(gpu_lib, H, W):
    """Fenton without diffusion: a cell's U stays on its side of 0.5 over one tick whatever its neighbours do"""
    return gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 0.0, flags=gpu_lib.FAST)


def play(st, planes, conn, max_waves, max_links):
    """attaches the recorder with links, sets each plane in front of a single-tick call and reads the state back behind it ->
    (wave counts, wave records, link counts, link records, the planes read back under the recorder's mask)"""
    H, W = planes[0].shape
    mask = interior(H, W)
    st.waves_begin(0, 0, 0.5, -1, 0, 0.0, conn, mask.astype(np.uint8), max_waves, 1, len(planes))
    st.waves_links_begin(max_links)
    back = []
    for plane in planes:
        state = np.zeros((4, H, W), np.float32)
        state[0] = plane
        state[1] = state[2] = 1.0
        st.set_state(-1, state)
        st.step(1)
        seen = (st.get_state(0) > np.float32(0.5)) & mask
        assert np.array_equal(seen, plane), np.argwhere(seen != plane)[:8]
        back.append(seen)
    assert st.waves_count() == len(planes)
    counts, records = st.waves_read()
    lcounts, lrecords = st.waves_links_read()
    st.waves_end()
    return counts, records, lcounts, lrecords, back


def same_links(got, want, what):
    assert got.dtype == want.dtype == lref.LINK_DTYPE and got.tolist() == want.tolist(), (what, got[:8], want[:8])


def check_against(samples, counts, records, lcounts, lrecords, what):
    """every device sample against the restatement's `samples` (wave_link_ref.sequence); the lists are not cut"""
    assert lcounts.dtype == np.int32 and lcounts.shape == (len(samples), 4)
    for s, (wc, wrec, _, lc, lrec) in enumerate(samples):
        print('%s sample %d: device links %s reference %s' % (what, s, lcounts[s].tolist(), lc.tolist()))
        assert counts[s].tolist() == wc.tolist(), (what, s)
        assert ref.sorted_records(records[s], counts[s, 1]).tobytes() == wrec.tobytes(), (what, s)
        assert lcounts[s].tolist() == lc.tolist(), (what, s, lcounts[s], lc)
        same_links(lref.sorted_links(lrecords[s], lcounts[s, 1]), lrec, (what, s))


def same_events(samples, counts, records, lcounts, lrecords, what):
    """fib_tf_amd.waves.events and .track on the device's lists against the restatement's on the reference's"""
    from fib_tf_amd import waves
    W = [ref.sorted_records(records[s], counts[s, 1]) for s in range(len(counts))]
    L = [lref.sorted_links(lrecords[s], lcounts[s, 1]) for s in range(len(counts))]
    ev = waves.events(W, L, wave_counts=counts, link_counts=lcounts)
    seeds, links = lref.lists_of(samples)
    want = lref.events(seeds, links)
    assert [tuple(int(x) for x in list(r)[1:]) for r in ev] == want, what
    tr, wtr = waves.track(W, L, wave_counts=counts, link_counts=lcounts), lref.tracks(seeds, links)
    assert [(t.id, t.born, t.ended, t.parents, t.children, t.points['seed'].tolist()) for t in tr] == \
        [(t['id'], t['born'], t['ended'], t['parents'], t['children'], [q for _, q in t['path']]) for t in wtr], what
    return want


# ---- crafted sequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: '%dx%d' % s)
def test_crafted_sequences_equal_the_restatement(gpu_lib, shape, conn):
    H, W = shape
    planes = [p for _, p in frames(H, W)]
    st = crafted_stepper(gpu_lib, H, W)
    counts, records, lcounts, lrecords, back = play(st, planes, conn, ROOMY, ROOMY)
    st.close()
    samples = lref.sequence(back, conn)
    what = '%dx%d conn %d' % (H, W, conn)
    check_against(samples, counts, records, lcounts, lrecords, what)
    same_events(samples, counts, records, lcounts, lrecords, what)
    # ... and by the reference's own output the sequence holds what it is there for (test_wave_links_cpu.py says why 5 x 3
    # can hold no split into three)
    _, _, seen = what_happens(H, W, conn)
    assert EVERYWHERE | ({'a split into two'} if shape == (5, 3) else {'a split into three'}) <= seen
    assert lcounts[0].tolist() == [0, 0, 0, 0] and lcounts[:, 3].max() == 0 and lcounts[:, 0].max() >= 2


def test_conn_changes_the_links_at_a_tile_corner(gpu_lib):
    """the diagonal pairs at the corner of four tiles: two waves and two links under conn = 4, one and one under conn = 8"""
    H, W = 130, 67
    names = [n for n, _ in frames(H, W)]
    at = names.index('corner diagonal')
    planes = [p for _, p in frames(H, W)][at:at + 4]
    n = {}
    for conn in (4, 8):
        st = crafted_stepper(gpu_lib, H, W)
        counts, records, lcounts, lrecords, back = play(st, planes, conn, 16, 16)
        st.close()
        check_against(lref.sequence(back, conn), counts, records, lcounts, lrecords, 'corner conn %d' % conn)
        n[conn] = lcounts[:, 0].tolist()
    assert n[4] == [0, 2, 0, 2] and n[8] == [0, 1, 0, 1]


# ---- cuts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(4, 64), (37, 53), (130, 67)], ids=lambda s: '%dx%d' % s)
def test_cuts(gpu_lib, shape):
    """a full plane, then the checkerboard under conn = 4: one wave before, n waves of one cell after — n pairs of one cell.
    max_links = 8: a table of 32 entries, which every probe sequence covers whole (an odd step modulo a power of two), so it
    fills up: links = 32, stored = 8, lost = n - 32, cells = n, exactly.  max_links = m < n <= 2 m: a table of >= 4 m >= 2 n
    entries, load <= 1/2 at any time, so a pair is lost only if 32 probed entries are all taken — at most 2^-32 per pair, n of
    them: nothing is lost, links = n, stored = m.  max_links = n: the whole list, which equals the reference"""
    H, W = shape
    planes = [interior(H, W), checkerboard(H, W) & interior(H, W)]
    n = int(planes[1].sum())
    assert n > 32
    samples = lref.sequence(planes, 4)
    want = samples[1][4]
    assert len(want) == n and set(want['overlap'].tolist()) == {1}
    m = 1
    while 2 * m < n:
        m *= 2
    assert m < n <= 2 * m
    st = crafted_stepper(gpu_lib, H, W)
    for max_links, expect in ((8, [32, 8, n, n - 32]), (m, [n, m, n, 0]), (n, [n, n, n, 0])):
        counts, records, lcounts, lrecords, back = play(st, planes, 4, 16, max_links)
        print('%dx%d max_links %d: device %s expected %s' % (H, W, max_links, lcounts[1].tolist(), expect))
        assert lcounts[0].tolist() == [0, 0, 0, 0] and lcounts[1].tolist() == expect, (max_links, lcounts, expect)
        assert counts[1].tolist() == [n, 16, n] and lrecords.shape == (2, max_links)
        got = lref.sorted_links(lrecords[1], lcounts[1, 1])
        # every stored record is one of the reference's, whole, and none appears twice
        assert len(got) == expect[1] and len(set(got.tolist())) == len(got)
        assert set(got.tolist()) <= set(want.tolist())
        if max_links >= n:
            same_links(got, want, 'the whole list')
    st.close()


# ---- dynamics --------------------------------------------------------------------------------------------------------------------
def dyn_run(shape, env, every, poll=False, fast=True, **kw):
    """test_gpu_waves.dyn_run with links: Fenton with a hole, three blobs, DYN_TICKS single-tick calls -> a dict"""
    H, W = shape
    with plan_env(env), warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        m = fenton_hole(H, W, fast)
        st = m._stepper
        st.set_state(-1, blobs(H, W, st.get_state(-1)))
        out = {'polled': []}
        with m.record_waves(every=every, capacity=DYN_TICKS // every, **kw) as rec:
            for i in range(DYN_TICKS):
                st.step(1)
                if poll and (i + 1) % every == 0:
                    out['polled'].append(st.get_state(-1).copy())
            assert rec.count() == DYN_TICKS // every
            out['waves'] = rec.raw()
            out['labels'] = rec.labels()
            if rec.max_links:
                out['links'] = rec.links_raw()
                out['lists'] = (rec.waves(), rec.links(), rec.events(), rec.tracks(), rec.link_counts(), rec.links_truncated())
            out['mask'], out['level'], out['tick_ms'] = rec.mask, rec.level, rec.tick_ms
        out['state'] = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
        st.close()
    return out


def reference_of(states, mask, level, conn=4):
    return lref.sequence([ref.set_plane(X[0], level, 'above', mask) for X in states], conn)


def links_bytes(run):
    lcounts, lrecords = run['links']
    return lcounts.tobytes() + b''.join(lref.sorted_links(lrecords[s], lcounts[s, 1]).tobytes() for s in range(len(lcounts)))


@pytest.fixture(scope='module', params=DYN_GRIDS, ids=lambda s: '%dx%d' % s)
def polled_run(request, gpu_lib):
    """every = 1, the state read back behind every tick: each sample's links equal the reference from consecutive states"""
    shape = request.param
    run = dyn_run(shape, {'FIBHIP_VARIANT': FORCED}, 1, poll=True, links=True)
    assert run['level'] == 0.5 and len(run['polled']) == DYN_TICKS
    samples = reference_of(run['polled'], run['mask'], run['level'])
    what = '%dx%d every 1' % shape
    check_against(samples, *run['waves'], *run['links'], what)
    rows = same_events(samples, *run['waves'], *run['links'], what)
    # by the reference: the run holds what tests/test_wave_links_cpu.py found on the CPU oracle, at the least
    got = (sum(r[3] for r in rows), sum(r[4] for r in rows), sum(r[2] for r in rows), sum(r[1] for r in rows),
           max(len(r[4]) for r in samples), sum(1 for r in samples if len(r[4]) >= 2))
    assert all(g >= w for g, w in zip(got, ADEQUATE[shape, 1])), (got, ADEQUATE[shape, 1])
    return shape, run, samples


def test_dynamics_equal_the_restatement(polled_run):
    """... and the recorder's own lists say the same as the raw read: links() sorted with their times, events(), tracks()"""
    shape, run, samples = polled_run
    waves, links, ev, tracks, lcounts, cut = run['lists']
    assert len(cut) == 0 and np.array_equal(lcounts, run['links'][0])
    for s, r in enumerate(samples):
        assert links[s].dtype.names == ('t_ms', 'prev', 'seed', 'overlap')
        assert [tuple(x)[1:] for x in links[s].tolist()] == r[4].tolist(), s
        assert np.all(links[s]['t_ms'] == (s + 1) * run['tick_ms'])
    seeds, lk = lref.lists_of(samples)
    assert [tuple(int(x) for x in list(r)[1:]) for r in ev] == lref.events(seeds, lk)
    assert ev['t_ms'].tolist() == [(s + 1) * run['tick_ms'] for s in range(DYN_TICKS)]
    want = lref.tracks(seeds, lk)
    assert [(t.born, t.ended, t.parents, t.children) for t in tracks] == [(t['born'], t['ended'], t['parents'], t['children']) for t in want]
    assert max(t.lifetime_ms for t in tracks) > 0 and sum(len(t.points) for t in tracks) == sum(len(q) for q in seeds)


@pytest.mark.parametrize('env', [{'FIBHIP_VARIANT': FORCED, 'FIBHIP_MT': '0'}, {}, {'FIBHIP_VARIANT': '1,64,4,256'}, {'FIBHIP_VARIANT': FORCED}],
                         ids=['one-launch-per-tick', 'unforced', 'flat-tiles', 'forced-small'])
@pytest.mark.parametrize('every', [7, 10])
def test_links_do_not_depend_on_the_launch_plan(gpu_lib, polled_run, every, env):
    """strides 7 and 10, nothing read back in between, under four launch plans: the links are the reference's between the polled
    states `every` ticks apart (the state does not depend on the plan), and so the same bytes under every plan"""
    shape, base, _ = polled_run
    run = dyn_run(shape, env, every, links=True)
    assert run['state'] == base['state'], env
    samples = reference_of(base['polled'][every - 1::every], base['mask'], base['level'])
    check_against(samples, *run['waves'], *run['links'], '%dx%d every %d %s' % (shape + (every, env)))
    if (shape, every) in ADEQUATE:
        rows = same_events(samples, *run['waves'], *run['links'], env)
        assert sum(r[3] for r in rows) >= ADEQUATE[shape, every][0] and sum(r[4] for r in rows) >= ADEQUATE[shape, every][1]


def test_exact_policy(gpu_lib):
    """the exact arithmetic policy (the runs above are the fast one's): against the reference from its own polled states"""
    shape = (64, 64)
    run = dyn_run(shape, {}, 1, poll=True, fast=False, links=True, conn=8, max_links=7)
    samples = reference_of(run['polled'], run['mask'], run['level'], 8)
    check_against(samples, *run['waves'], *run['links'], 'exact policy')
    assert max(len(r[4]) for r in samples) >= 2


def test_beeler_reuter(gpu_lib):
    from test_gpu_leads import hole_model
    H, W = 37, 53
    m = hole_model('br', H, W)
    wave(m, 'br')
    st = m._stepper
    states = []
    with m.record_waves(level=-40, every=2, capacity=6, links=True) as rec:
        for i in range(12):
            st.step(1)
            if i % 2 == 1:
                states.append(st.get_state(-1).copy())
        samples = reference_of(states, rec.mask, -40)
        check_against(samples, *rec.raw(), *rec.links_raw(), 'Beeler-Reuter')
        assert all(len(r[4]) >= 1 for r in samples[1:]) and len({int(r[4]['overlap'].sum()) for r in samples[1:]}) >= 2
        assert rec.events()['waves'].tolist() == [len(r[1]) for r in samples]
    st.close()


# ---- links off -------------------------------------------------------------------------------------------------------------------
def test_links_off_changes_nothing(gpu_lib):
    """the recorder without links beside the recorder with them: counts, records, labels and state are the same bytes"""
    shape = (130, 67)
    off, on = dyn_run(shape, {}, 10), dyn_run(shape, {}, 10, links=True)
    assert 'links' not in off and off['state'] == on['state'] and off['labels'].tobytes() == on['labels'].tobytes()
    assert off['waves'][0].tobytes() == on['waves'][0].tobytes()
    for s in range(len(off['waves'][0])):
        n = off['waves'][0][s, 1]
        assert ref.sorted_records(off['waves'][1][s], n).tobytes() == ref.sorted_records(on['waves'][1][s], n).tobytes(), s
    assert on['links'][0][1:, 0].min() >= 1


def test_timeline_and_the_refused_read(gpu_lib):
    four = ['wave_label_kernel', 'wave_merge_kernel', 'wave_root_kernel', 'wave_reduce_kernel']
    for links in (False, True):
        st = raw_stepper(gpu_lib, 130, 67)
        st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 64, 2, 4)
        if links:
            st.waves_links_begin(64)
        st.step(1)
        st.trace_begin()
        st.step(1)
        names = [e['name'].split('<')[0] for e in st.trace_end()]
        if links:
            assert names[-6:] == four + ['wave_link_kernel', 'wave_link_pack_kernel'], names
            assert st.waves_links_read()[0].shape == (1, 4)
        else:
            assert names[-4:] == four and not [n for n in names if n.startswith('wave_link')], names
            with pytest.raises(gpu_lib.FibhipError, match='links are off'):
                st.waves_links_read()
        st.close()


# ---- refusals and ranges ---------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    for call in (lambda: st.waves_links_begin(16), lambda: st.waves_links_read(0, 0)):
        with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
            call()
    begin = lambda every=1, cap=4: st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 16, every, cap)  # noqa: E731
    begin()
    for bad in (0, -3, 65537):
        with pytest.raises(gpu_lib.FibhipError, match=r'1 \.\. 65536 links per sample \(got %d\)' % bad):
            st.waves_links_begin(bad)
    with pytest.raises(gpu_lib.FibhipError, match='links are off'):
        st.waves_links_read(0, 0)
    st.waves_links_begin(16)
    with pytest.raises(gpu_lib.FibhipError, match='links are on already'):
        st.waves_links_begin(16)
    st.waves_end()
    with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
        st.waves_links_read(0, 0)
    # behind a tick the recorder has seen: links start with the recorder or not at all
    begin(every=3)
    st.step(1)
    with pytest.raises(gpu_lib.FibhipError, match='has seen ticks already'):
        st.waves_links_begin(16)
    begin()                                                   # (attaching again drops the links with the lists)
    st.waves_links_begin(4)
    begin()
    with pytest.raises(gpu_lib.FibhipError, match='links are off'):
        st.waves_links_read(0, 0)
    st.step_edges()
    with pytest.raises(gpu_lib.FibhipError, match='inside an open tick'):
        st.waves_links_begin(4)
    st.step_interior()
    st.step_commit()
    st.waves_end()
    st.close()


def test_count_and_read_ranges(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 64, 2, 3)
    st.waves_links_begin(5)
    assert st.waves_links_read()[0].shape == (0, 4) and st.waves_links_read()[1].shape == (0, 5)
    states = []
    for i in range(6):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(-1).copy())
    lcounts, lrecords = st.waves_links_read()
    assert lcounts.shape == (3, 4) and lrecords.shape == (3, 5) and lrecords.dtype == gpu_lib.WAVE_LINK_DTYPE
    samples = lref.sequence([ref.set_plane(X[0], 0.5) for X in states], 4)
    check_against(samples, *st.waves_read(), lcounts, lrecords, 'ranges')
    assert lcounts[1:, 0].min() >= 1
    c12, r12 = st.waves_links_read(1, 2)
    assert c12.tobytes() == lcounts[1:].tobytes() and r12.tobytes() == lrecords[1:].tobytes()
    only, none = st.waves_links_read(2, 1, records=False)
    assert none is None and only.tobytes() == lcounts[2:].tobytes()
    assert st.waves_links_read(3, 0)[0].shape == (0, 4)
    with pytest.raises(gpu_lib.FibhipError, match=r'waves_links_read: samples \[2, 4\) of 3 taken'):
        st.waves_links_read(2, 2)
    with pytest.raises(gpu_lib.FibhipError, match=r'samples \[-1, 0\) of 3 taken'):
        st.waves_links_read(-1, 1)
    st.step(1)
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(1)
    again = st.waves_links_read()
    assert again[0].tobytes() == lcounts.tobytes() and again[1].tobytes() == lrecords.tobytes()
    st.waves_end()
    st.close()


# ---- together --------------------------------------------------------------------------------------------------------------------
def test_beside_every_other_recorder(gpu_lib, monkeypatch):
    """every recorder and both programs beside a wave recorder with links, each with a stride of its own: the links, and the
    waves, are those of a run with the wave recorder (and the two programs, which write the state) alone"""
    import test_gpu_waves_together as tg
    taken = {}
    begin, read = gpu_lib.Stepper.waves_begin, gpu_lib.Stepper.waves_read

    def begin_with_links(self, *a, **k):
        begin(self, *a, **k)
        self.waves_links_begin(2 * tg.WAVE['max_waves'])

    def read_with_links(self, *a, **k):
        taken['links'] = self.waves_links_read()
        return read(self, *a, **k)
    monkeypatch.setattr(gpu_lib.Stepper, 'waves_begin', begin_with_links)
    monkeypatch.setattr(gpu_lib.Stepper, 'waves_read', read_with_links)
    out = []
    for which in (tg.RECORDERS, ('wv',)):
        got = tg._run(monkeypatch, which, poll=which == ('wv',))
        lcounts, lrecords = taken.pop('links')
        out.append((got, lcounts, lrecords))
    (together, lc, lr), (solo, slc, slr) = out
    assert together['wv'] == solo['wv'] and together['state'] == solo['state']
    assert lc.tobytes() == slc.tobytes()
    for s in range(len(lc)):
        assert lref.sorted_links(lr[s], lc[s, 1]).tobytes() == lref.sorted_links(slr[s], slc[s, 1]).tobytes(), s
    planes = [ref.set_plane(X[0], tg.WAVE['level'], 'above', solo['mask'], (X[1], 'below', tg.WAVE['level2'])) for X in solo['polled']]
    samples = lref.sequence(planes, tg.WAVE['conn'])
    counts, records, _ = together['wv-raw']
    check_against(samples, counts, records, lc, lr, 'together')
    assert lc[1:, 0].min() >= 1 and len(set(lc[:, 2].tolist())) > 2


# ---- the example -----------------------------------------------------------------------------------------------------------------
def test_example_runs_headless(gpu_lib, tmp_path):
    """examples/run_wavebreaks.py end to end at a tiny size, in this process: the events over time, the tracks, a PNG"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('run_wavebreaks_under_test', os.path.join(root, 'examples', 'run_wavebreaks.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = tmp_path / 'wavebreaks.png'
    ev, tracks = ex.main(['--size', '64', '--ms', '40', '--every', '5', '--out', str(out)])
    assert ev.shape == (8,) and ev['waves'].max() >= 1 and ev['continued'].sum() >= 1
    assert len(tracks) >= 1 and max(t.lifetime_ms for t in tracks) > 0 and out.exists()
