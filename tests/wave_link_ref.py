"""wave_link_ref — the wave recorder's links (include/fibhip.h, fibhip_waves_links_*) restated for the tests, on top of wave_ref.

With L[s] the label plane of sample s (wave_ref.label), a link of sample s >= 1 is a pair (prev, seed) such that some cell has
L[s - 1] = prev >= 0 and L[s] = seed >= 0, and its overlap is the number of such cells.  `links` counts them with a dict over the
cells; `events` and `tracks` restate fib_tf_amd/waves.py's host code in plain Python over dicts and tuples, sharing nothing
with it."""
import numpy as np

import wave_ref as ref

LINK_DTYPE = np.dtype([('prev', np.int32), ('seed', np.int32), ('overlap', np.int32)])


def links(prev_labels, labels, max_links=None):
    """(counts int32 [4] = links, stored, cells, lost = 0; records sorted by (prev, seed) — ALL of them) between two label planes;
    prev_labels None: the first sample, which has no links"""
    labels = np.asarray(labels)
    if prev_labels is None:
        return np.zeros(4, np.int32), np.zeros(0, LINK_DTYPE)
    prev_labels = np.asarray(prev_labels)
    assert prev_labels.shape == labels.shape
    pairs = {}
    for p, q in zip(prev_labels.ravel().tolist(), labels.ravel().tolist()):
        if p >= 0 and q >= 0:
            pairs[(p, q)] = pairs.get((p, q), 0) + 1
    rec = np.array([(p, q, n) for (p, q), n in sorted(pairs.items())], LINK_DTYPE) if pairs else np.zeros(0, LINK_DTYPE)
    n = len(rec)
    stored = n if max_links is None else min(n, int(max_links))
    return np.array([n, stored, sum(pairs.values()), 0], np.int32), rec


def sequence(planes, conn=4):
    """the samples of a sequence of set planes: a list of (wave counts, wave records, labels, link counts, link records)"""
    out, before = [], None
    for s in planes:
        counts, rec, lab = ref.sample(s, conn)
        lc, lr = links(before, lab)
        out.append((counts, rec, lab, lc, lr))
        before = lab
    return out


def sorted_links(records, stored):
    """the first `stored` device records, sorted by (prev, seed)"""
    r = np.asarray(records)[:int(stored)]
    return r[np.lexsort((r['seed'], r['prev']))]


def _degrees(P, Q, L, min_overlap):
    kept = [(p, q) for p, q, o in L if o >= min_overlap]
    dplus = {p: 0 for p in P}
    dminus = {q: 0 for q in Q}
    for p, q in kept:
        dplus[p] += 1
        dminus[q] += 1
    return kept, dplus, dminus


def events(seeds_per_sample, links_per_sample, min_overlap=1):
    """rows (waves, births, deaths, splits, merges, continued) as tuples; `seeds_per_sample`: a list of lists of seeds,
    `links_per_sample`: a list of lists of (prev, seed, overlap)"""
    rows = []
    for s, Q in enumerate(seeds_per_sample):
        if s == 0:
            rows.append((len(Q), 0, 0, 0, 0, 0))
            continue
        P = seeds_per_sample[s - 1]
        kept, dplus, dminus = _degrees(P, Q, links_per_sample[s], min_overlap)
        births = len([q for q in Q if dminus[q] == 0])
        deaths = len([p for p in P if dplus[p] == 0])
        splits = len([p for p in P if dplus[p] >= 2])
        merges = len([q for q in Q if dminus[q] >= 2])
        continued = len([1 for p, q in kept if dplus[p] == 1 and dminus[q] == 1])
        rows.append((len(Q), births, deaths, splits, merges, continued))
    return rows


def tracks(seeds_per_sample, links_per_sample, min_overlap=1):
    """a list of dicts {id, born, ended, parents, children, path}: path is the list of (sample, seed) the track visits.  The
    tracks are the connected pieces of the graph whose nodes are the (sample, seed) and whose edges are the continued links"""
    nodes = [(s, q) for s, Q in enumerate(seeds_per_sample) for q in sorted(Q)]
    nxt, prv, ins, outs = {}, {}, {n: [] for n in nodes}, {n: [] for n in nodes}
    for s in range(1, len(seeds_per_sample)):
        kept, dplus, dminus = _degrees(seeds_per_sample[s - 1], seeds_per_sample[s], links_per_sample[s], min_overlap)
        for p, q in kept:
            outs[(s - 1, p)].append((s, q))
            ins[(s, q)].append((s - 1, p))
            if dplus[p] == 1 and dminus[q] == 1:
                nxt[(s - 1, p)] = (s, q)
                prv[(s, q)] = (s - 1, p)
    out, of = [], {}
    for n in nodes:                                      # (sample, then seed: the order of first appearance)
        if n in prv:
            continue
        path = [n]
        while path[-1] in nxt:
            path.append(nxt[path[-1]])
        for m in path:
            of[m] = len(out)
        head, tail = path[0], path[-1]
        born = 'start' if head[0] == 0 else 'birth' if not ins[head] else 'merge' if len(ins[head]) >= 2 else 'split'
        if tail[0] == len(seeds_per_sample) - 1:
            ended = 'end'
        elif not outs[tail]:
            ended = 'death'
        else:
            ended = 'split' if len(outs[tail]) >= 2 else 'merge'
        out.append({'id': len(out), 'born': born, 'ended': ended, 'path': path, 'head': head, 'tail': tail})
    for t in out:
        t['parents'] = sorted(of[m] for m in ins[t.pop('head')])
        t['children'] = sorted(of[m] for m in outs[t.pop('tail')]) if t['ended'] in ('split', 'merge') else []
    return out


def lists_of(samples):
    """(seeds per sample, links per sample) as plain lists, from what `sequence` returns"""
    return ([r[1]['seed'].tolist() for r in samples],
            [[(int(p), int(q), int(o)) for p, q, o in zip(r[4]['prev'], r[4]['seed'], r[4]['overlap'])] for r in samples])
