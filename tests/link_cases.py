"""Shared by tests/test_link_host.py (g++ twin) and tests/test_gpu_link.py (HIP): the yardstick of the components linked across
frames (include/ext/occ4d_link.h) -- a numpy / Python-integer restatement of both entry points and of a multi-frame tracker built
on them --, the case matrix, and the comparison, which is EQUAL everywhere: integers only, no tolerance.

The overlap is np.unique on the packed keys with return_index and return_counts, ordered by first index; the order relation of the
match is written in Python integers, which never wrap.  Grids: (1, 1, 255 / 256 / 257) are the numbering tile's edge, (1, 1, 300)
with one pair throughout has runs that cross wave and workgroup boundaries, (40, 24, 20) = 19 200 points is the largest."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import components_cases as cc
import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_link_match_i32', 'occ4d_link_overlap_i32']
GRIDS = [(1, 1, 1), (1, 1, 5), (1, 1, 255), (1, 1, 256), (1, 1, 257), (1, 1, 300), (2, 3, 70), (7, 8, 7), (17, 9, 33), (40, 24, 20)]
BIG = ((17, 9, 33), (40, 24, 20))
CANARY = -0x0123456789ABCDEF
THRESHOLDS = ((0, 1), (1, 2), (1, 1))
NEXT_IN = 1000
MIN_SLOTS, TILE = 64, 256


# ---------------------------------------------------------------------------------------------------------------- the restatement
def slots_for(n, cap):
    slots = MIN_SLOTS
    while slots < 2 * min(cap, n) and slots < 2 ** 31:
        slots *= 2
    return slots


def work_len(n, cap):
    return 4 * slots_for(n, cap) + n + 2 * ((n + TILE - 1) // TILE)


def restate_overlap(la, lb, k_a, k_b):
    """-> (pairs (P, 4) int64, ALL of them, in the order of their roots; member points)."""
    la, lb = np.asarray(la, np.int64), np.asarray(lb, np.int64)
    idx = np.flatnonzero((la >= 0) & (la < k_a) & (lb >= 0) & (lb < k_b))
    keys = (la[idx] << 32) | lb[idx]
    u, first, counts = np.unique(keys, return_index=True, return_counts=True)
    order = np.argsort(first, kind='stable')
    rows = np.stack([u >> 32, u & 0xffffffff, counts, idx[first] if len(idx) else first], axis=1).astype(np.int64).reshape(-1, 4)
    return rows[order], len(idx)


def beats(x, y, tie):
    """x, y = (count, union, a, b) in Python integers; tie: 2 for a fixed b (the lower a), 3 for a fixed a (the lower b)."""
    left, right = x[0] * y[1], y[0] * x[1]
    return left > right or (left == right and x[tie] < y[tie])


def restate_match(pairs, size_a, size_b, track_a, next_in, num, den):
    """pairs: the rows the match may read -> (link (k_b, 4) int32, best_a (k_a, 2) int32, next_out)."""
    k_a, k_b = len(size_a), len(size_b)
    best_of_b, best_of_a = {}, {}
    for a, b, count, _ in np.asarray(pairs, np.int64).reshape(-1, 4).tolist():
        if not (0 <= a < k_a and 0 <= b < k_b):
            continue
        cand = (count, int(size_a[a]) + int(size_b[b]) - count, a, b)
        if b not in best_of_b or beats(cand, best_of_b[b], 2):
            best_of_b[b] = cand
        if a not in best_of_a or beats(cand, best_of_a[a], 3):
            best_of_a[a] = cand
    link, best_a = np.zeros((k_b, 4), np.int32), np.zeros((k_a, 2), np.int32)
    nxt = int(next_in)
    for b in range(k_b):
        count, union, a, _ = best_of_b.get(b, (0, 0, -1, b))
        linked = a >= 0 and best_of_a[a][3] == b and count * den >= num * union
        link[b] = (int(track_a[a]) if linked else nxt, a if linked else -1, a, count)
        nxt += not linked
    for a in range(k_a):
        best_a[a] = (best_of_a[a][3], best_of_a[a][0]) if a in best_of_a else (-1, 0)
    return link, best_a, nxt


def restate_tracker(frames, num, den):
    """frames: [(labels, table)] -> the link array of every frame, the number of tracks."""
    links, prev, nxt = [], None, 0
    for labels, table in frames:
        if prev is None:
            pairs, size_a, track_a = np.zeros((0, 4), np.int64), [], []
        else:
            assert len(labels) == len(prev[0])
            pairs, size_a, track_a = restate_overlap(prev[0], labels, len(prev[1]), len(table))[0], prev[1][:, 0], prev[2]
        link, _, nxt = restate_match(pairs, size_a, table[:, 0], track_a, nxt, num, den)
        links.append(link)
        prev = (labels, table, link[:, 0])
    return links, nxt


# ---------------------------------------------------------------------------------------------------------------- the matrix
@functools.lru_cache(maxsize=None)
def labelling(counts, kind, connectivity=6):
    """(labels (n,) int32, k) of a field, by the components' own restatement (computed once per process, read-only)."""
    n = counts[0] * counts[1] * counts[2]
    if kind == 'solid':
        field = np.ones(n, np.float32)
    elif kind == 'checker':
        field = cc.checkerboard(counts)
    elif kind == 'shifted':                                                # the 0.3 field moved by a voxel along z
        field = np.roll((cc.random_field(counts, 0.3, 21) >= 0.7).astype(np.float32).reshape(counts), 1, axis=2).reshape(-1)
    else:
        density, seed = kind
        field = (cc.random_field(counts, density, seed) >= 1.0 - density).astype(np.float32)
    labels, totals, table = cc.restate(field, counts, 0.5, connectivity)
    labels.setflags(write=False)
    return labels, int(totals[0])


def sizes_of(labels, k):
    return np.bincount(labels[(labels >= 0) & (labels < k)], minlength=k)[:k].astype(np.int64) if k else np.zeros(0, np.int64)


def case(name, la, lb, k_a, k_b, cap=None):
    la, lb = np.ascontiguousarray(la, np.int32), np.ascontiguousarray(lb, np.int32)
    return dict(name=name, la=la, lb=lb, k_a=k_a, k_b=k_b, cap=cap)


def _cases():
    out = []
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        a, k_a = labelling(counts, (0.3, 21))
        b, k_b = labelling(counts, (0.6, 22))
        out.append(case(g + '-random-6', a, b, k_a, k_b))
        out.append(case(g + '-identical', b, b, k_b, k_b))
        disjoint = np.where(a >= 0, -1, b)
        out.append(case(g + '-disjoint', a, disjoint, k_a, k_b))
        solid = np.zeros(n, np.int32)
        out.append(case(g + '-solid', solid, solid, 1, 1))
        ch, k_ch = labelling(counts, 'checker')
        out.append(case(g + '-checker-solid', ch, solid, k_ch, 1))
        out.append(case(g + '-foreign', np.arange(n), np.arange(n), n, n, cap=n))
        rng = np.random.default_rng(23)
        wild_a, wild_b = a.astype(np.int64), b.astype(np.int64)
        pick = rng.integers(0, 6, n)
        wild_a[pick == 0], wild_a[pick == 1], wild_b[pick == 2], wild_b[pick == 3] = k_a, -7, k_b + 5, -2 ** 31
        out.append(case(g + '-outside', wild_a, wild_b, k_a, k_b))
        out.append(case(g + '-no-a', a, b, 0, k_b))
        out.append(case(g + '-no-b', a, b, k_a, 0))
        out.append(case(g + '-foreign-cap-1', np.arange(n), np.arange(n), n, n, cap=1))             # n > 64 pairs: the table overflows
    for counts in BIG:
        g = '%dx%dx%d' % counts
        a, k_a = labelling(counts, (0.3, 21), 26)
        b, k_b = labelling(counts, (0.6, 22), 26)
        out.append(case(g + '-random-26', a, b, k_a, k_b))
        for c in (6, 26):
            a, k_a = labelling(counts, (0.3, 21), c)
            s, k_s = labelling(counts, 'shifted', c)
            out.append(case('%s-shifted-%d' % (g, c), a, s, k_a, k_s))
        a, k_a = labelling(counts, (0.3, 21))
        b, k_b = labelling(counts, (0.6, 22))
        pairs = len(restate_overlap(a, b, k_a, k_b)[0])
        out.append(case(g + '-cap-half', a, b, k_a, k_b, cap=(pairs + 1) // 2))                     # cap < pairs <= slots
        out.append(case(g + '-cap-one', a, b, k_a, k_b, cap=1))                                     # pairs > slots = 64
        out.append(case(g + '-cap-zero', a, b, k_a, k_b, cap=0))
    out.append(case('empty-grid', np.zeros(0), np.zeros(0), 0, 0))
    out.append(case('empty-grid-with-k', np.zeros(0), np.zeros(0), 3, 4, cap=5))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)


def cap_of(c):
    return min(len(c['la']), c['k_a'] * c['k_b']) if c['cap'] is None else c['cap']


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement of a case, computed once per process: (all pairs, totals, {threshold: (link, best_a, next_out)})."""
    c = BY_NAME[name]
    n, cap = len(c['la']), cap_of(c)
    pairs, members = restate_overlap(c['la'], c['lb'], c['k_a'], c['k_b'])
    overflow = len(pairs) > slots_for(n, cap)
    totals = np.array([len(pairs), members, int(overflow)], np.int32)
    size_a, size_b = sizes_of(c['la'], c['k_a']), sizes_of(c['lb'], c['k_b'])
    readable = pairs[:0] if overflow else pairs[:cap]
    matches = {t: restate_match(readable, size_a, size_b, track_of(c['k_a']), NEXT_IN, *t) for t in THRESHOLDS}
    pairs.setflags(write=False)
    return pairs, totals, matches


def track_of(k_a):
    return (np.arange(k_a, dtype=np.int64) * 3 + 5).astype(np.int32)


def table_of(sizes):
    """A (k, 12) table whose column 0 holds the sizes; the match must read nothing else."""
    t = np.full((len(sizes), 12), CANARY, np.int64)
    t[:, 0] = sizes
    return t


# ---------------------------------------------------------------------------------------------------------------- the comparison
def run(c, device):
    """The case through ops.components_overlap / components_match -> numpy (pair buffer with two canary rows behind it, totals,
    {threshold: (link, best_a, next_out)})."""
    cap = cap_of(c)
    to = lambda a: torch.from_numpy(np.array(a)).to(device)                 # (a copy: the cases' arrays are read-only)
    buffer = torch.full((cap + 2, 4), CANARY, dtype=torch.int64, device=device)
    pairs, totals = pk.ops.components_overlap(to(c['la']), to(c['lb']), c['k_a'], c['k_b'], cap=c['cap'], pairs=buffer)
    assert pairs.shape == (cap, 4) and pairs.dtype == torch.int64 and totals.dtype == torch.int32 and totals.shape == (3,)
    size_a, size_b = sizes_of(c['la'], c['k_a']), sizes_of(c['lb'], c['k_b'])
    matches = {}
    for t in THRESHOLDS:
        link, best_a, nxt = pk.ops.components_match(pairs, totals, to(table_of(size_a)), to(table_of(size_b)), to(track_of(c['k_a'])),
                                                    to(np.array([NEXT_IN], np.int32)), t)
        assert link.dtype == best_a.dtype == nxt.dtype == torch.int32
        matches[t] = (link.cpu().numpy(), best_a.cpu().numpy(), int(nxt.item()))
    return buffer.cpu().numpy(), totals.cpu().numpy(), matches


def same(got, name):
    """Whether a run equals the restatement: the rows below min(cap, pairs), the canary from there on, the totals, every match.
    When the table overflows (totals[2] == 1) only that word, the canary from row cap on and the match (no pair is read) are set."""
    c = BY_NAME[name]
    buffer, totals, matches = got
    pairs, want_totals, want_matches = expected(name)
    cap = cap_of(c)
    ok = len(buffer) == cap + 2
    if want_totals[2]:
        ok = ok and totals[2] == 1 and bool((buffer[cap:] == CANARY).all())
    else:
        rows = min(cap, len(pairs))
        ok = ok and np.array_equal(totals, want_totals) and np.array_equal(buffer[:rows], pairs[:rows]) \
            and bool((buffer[rows:] == CANARY).all())
    for t in THRESHOLDS:
        ok = ok and np.array_equal(matches[t][0], want_matches[t][0]) and np.array_equal(matches[t][1], want_matches[t][1]) \
            and matches[t][2] == want_matches[t][2]
    return bool(ok)


def check(name, device):
    assert same(run(BY_NAME[name], device), name), name


def bits(got):
    buffer, totals, matches = got
    return [buffer.tobytes(), totals.tobytes()] + [x.tobytes() if isinstance(x, np.ndarray) else x for t in THRESHOLDS for x in matches[t]]


def run_raw(L, c):
    """The case on HOST arrays through the two entry points of a plain library handle `L` (the g++ twin loaded beside the HIP
    library, never enabled) -> what run() returns."""
    ptr = lambda a: None if a is None or a.size == 0 else ctypes.c_void_p(a.ctypes.data)
    n, cap = len(c['la']), cap_of(c)
    buffer = np.full((cap + 2, 4), CANARY, np.int64)
    totals, work = np.zeros(3, np.int32), np.zeros(work_len(n, cap) + 2, np.int32)
    work = work[(work.ctypes.data % 8) // 4:]
    assert L.occ4d_link_overlap_i32(ptr(c['la']), ptr(c['lb']), c['k_a'], c['k_b'], n, ptr(work), ptr(buffer) if cap else None, cap,
                                    ptr(totals), None) == pk._lib.OK
    ta, tb = table_of(sizes_of(c['la'], c['k_a'])), table_of(sizes_of(c['lb'], c['k_b']))
    track, nxt = track_of(c['k_a']), np.array([NEXT_IN], np.int32)
    matches = {}
    for t in THRESHOLDS:
        link, best_a, out = np.zeros((c['k_b'], 4), np.int32), np.zeros((c['k_a'], 2), np.int32), np.zeros(1, np.int32)
        assert L.occ4d_link_match_i32(ptr(buffer) if cap else None, ptr(totals), cap, ptr(ta), 12, ptr(tb), 12, c['k_a'], c['k_b'],
                                      ptr(track), t[0], t[1], ptr(nxt), ptr(link), ptr(best_a), ptr(out), None) == pk._lib.OK
        matches[t] = (link, best_a, int(out[0]))
    return buffer, totals, matches


def check_expectations_by_hand():
    """What the patterns are there for, checked on the restatement itself."""
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        pairs, totals, matches = expected(g + '-solid')
        assert pairs.tolist() == [[0, 0, n, 0]] and totals.tolist() == [1, n, 0]
        assert matches[(1, 1)][0].tolist() == [[5, 0, 0, n]] and matches[(1, 1)][2] == NEXT_IN
        pairs, totals, matches = expected(g + '-identical')
        k = BY_NAME[g + '-identical']['k_b']
        assert totals[0] == k and (pairs[:, 0] == pairs[:, 1]).all() and (pairs[:, 0] == np.arange(k)).all()
        assert (matches[(1, 1)][0][:, 1] == np.arange(k)).all() and matches[(1, 1)][2] == NEXT_IN          # every b links at IoU 1
        assert expected(g + '-disjoint')[1].tolist() == [0, 0, 0]
        assert expected(g + '-disjoint')[2][(0, 1)][0][:, 0].tolist() == list(range(NEXT_IN, NEXT_IN + BY_NAME[g + '-disjoint']['k_b']))
        pairs, totals, _ = expected(g + '-checker-solid')
        assert totals.tolist() == [(n + 1) // 2] * 2 + [0] and (pairs[:, 2] == 1).all()
        pairs, totals, _ = expected(g + '-foreign')
        assert totals.tolist() == [n, n, 0] and np.array_equal(pairs[:, 3], np.arange(n))                   # the fullest table, no overflow
        assert expected(g + '-no-a')[1].tolist() == [0, 0, 0] and expected(g + '-no-b')[1].tolist() == [0, 0, 0]
        assert expected(g + '-foreign-cap-1')[1][2] == (1 if n > 64 else 0)
    for counts in BIG:
        g = '%dx%dx%d' % counts
        c = BY_NAME[g + '-cap-half']
        assert c['cap'] < expected(g + '-cap-half')[1][0] <= slots_for(len(c['la']), c['cap']) and expected(g + '-cap-half')[1][2] == 0
        assert expected(g + '-cap-one')[1].tolist()[::2] == [expected(g + '-random-6')[1][0], 1]
        assert expected(g + '-shifted-6')[1][0] > 20


# ---------------------------------------------------------------------------------------------------------------- the rejected calls
def check_argument_errors(device):
    """ops.components_overlap / components_match: rejected arguments raise AssertionError with the library's text (the table of
    both libraries' texts is tests/test_gpu_link_contract_texts.py)."""
    z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=device)
    over = lambda **k: pk.ops.components_overlap(**dict(dict(labels_a=z(30), labels_b=z(30), k_a=2, k_b=2), **k))
    for kw, text in ((dict(k_a=-1, cap=3), 'k_a = -1, k_b = 2 must be >= 0'), (dict(cap=-1), 'cap = -1 must be >= 0'),
                     (dict(labels_b=z(29)), 'one length'), (dict(labels_a=z(30, dtype=torch.int64)), 'labels_a must be torch.int32'),
                     (dict(cap=3, pairs=z(2, 4, dtype=torch.int64)), 'pairs must be a contiguous')):
        with pytest.raises(AssertionError, match=text):
            over(**kw)
    pairs, totals = over()
    match = lambda **k: pk.ops.components_match(**dict(dict(pairs=pairs, totals=totals, table_a=z(2, 12, dtype=torch.int64) + 30,
                                                            table_b=z(2, 12, dtype=torch.int64) + 30, track_a=z(2), next_id=z(1)), **k))
    for kw, text in ((dict(min_iou=(1, 0)), r'iou_den = 0 must be in \[1, 1048576\]'), (dict(min_iou=(1, 2 ** 20 + 1)), 'iou_den = 1048577'),
                     (dict(min_iou=(3, 2)), r'iou_num = 3 must be in \[0, iou_den = 2\]'), (dict(min_iou=(-1, 2)), 'iou_num = -1'),
                     (dict(track_a=z(3)), 'track_a must be a contiguous'), (dict(next_id=z(2)), 'next_id must hold one element'),
                     (dict(totals=z(2)), 'totals must be a contiguous')):
        with pytest.raises(AssertionError, match=text):
            match(**kw)
    link, best_a, nxt = match(min_iou=0.5)
    assert link.tolist() == [[0, 0, 0, 30], [0, -1, -1, 0]] and best_a.tolist() == [[0, 30], [-1, 0]] and nxt.tolist() == [1]
    pairs, totals = pk.ops.components_overlap(z(0), z(0), 3, 4, cap=5, trim=True)
    assert pairs.shape == (0, 4) and totals.tolist() == [0, 0, 0]
    pairs, totals = over(trim=True)
    assert pairs.tolist() == [[0, 0, 30, 0]] and totals.tolist() == [1, 30, 0]
    assert pk.ops.link_work_len(1000, 100) == 4 * 256 + 1000 + 2 * 4 == work_len(1000, 100) and pk.ops.link_work_len(10, 1000) == 4 * 64 + 10 + 2


# ---------------------------------------------------------------------------------------------------------------- the tracker
GRID = (17, 9, 33)


def box(x0, x1, y0=2, y1=6, z0=4, z1=12):
    return ((x0, x1), (y0, y1), (z0, z1))


SEQUENCES = {
    # a box that moves one voxel per frame (IoU 3 / 5), then a second box appears in front of it in raster order
    'move-appear': [[box(2, 6)], [box(3, 7)], [box(4, 8)], [box(5, 9), box(0, 2, z0=20, z1=30)], [box(6, 10), box(0, 2, z0=20, z1=30)]],
    # a large and a small box, then one box over both and the gap between them, then the same again
    'merge': [[box(2, 8), box(10, 12)], [box(2, 12)], [box(2, 12)]],
    # one box, then cut in two by an empty plane: the larger part continues
    'split': [[box(2, 12)], [box(2, 8), box(9, 12)], [box(2, 8), box(9, 12)]],
    # an empty frame in the middle: afterwards everything is new
    'empty-middle': [[box(2, 6), box(10, 12)], [], [box(2, 6), box(10, 12)]],
}


@functools.lru_cache(maxsize=None)
def sequence(name):
    """[(labels, table)] of a sequence, by the components' own restatement."""
    return [cc.restate(cc.boxes(GRID, *frame), GRID, 0.5)[::2] for frame in SEQUENCES[name]]


def check_tracker_expectations_by_hand():
    ids = lambda name, t: [link[:, 0].tolist() for link in restate_tracker(sequence(name), *t)[0]]
    assert ids('move-appear', (0, 1)) == ids('move-appear', (1, 2)) == [[0], [0], [0], [1, 0], [1, 0]]      # the new box's root comes first
    assert ids('move-appear', (1, 1)) == [[0], [1], [2], [3, 4], [3, 5]]                                    # only the box that rests links
    assert ids('merge', (0, 1)) == [[0, 1], [0], [0]] and restate_tracker(sequence('merge'), 0, 1)[0][1].tolist() == [[0, 0, 0, 6 * 32]]
    assert ids('merge', (1, 1)) == [[0, 1], [2], [2]]
    assert ids('split', (0, 1)) == [[0], [0, 1], [0, 1]] and ids('split', (1, 1)) == [[0], [1, 2], [1, 2]]
    assert restate_tracker(sequence('split'), 0, 1)[0][1].tolist() == [[0, 0, 0, 6 * 32], [1, -1, 0, 3 * 32]]
    assert ids('empty-middle', (0, 1)) == [[0, 1], [], [2, 3]] and restate_tracker(sequence('empty-middle'), 0, 1)[1] == 4


def check_tracker(device):
    """components.Tracker over the sequences, at the three thresholds: every link equals the restatement; reset() starts again."""
    to = lambda a: torch.from_numpy(np.array(a)).to(device)                 # (a copy: the cases' arrays are read-only)
    for name in SEQUENCES:
        for t in THRESHOLDS:
            want, want_tracks = restate_tracker(sequence(name), *t)
            tracker = pk.components.Tracker(min_iou=t)
            for _ in range(2):
                assert tracker.n_tracks() == 0
                for (labels, table), link in zip(sequence(name), want):
                    got = tracker.add_frame(to(labels), to(table))
                    assert got.dtype == torch.int32 and got.device.type == torch.device(device).type
                    assert np.array_equal(got.cpu().numpy(), link), (name, t)
                assert tracker.n_tracks() == want_tracks
                tracker.reset()
    tracker = pk.components.Tracker(min_iou=0.5)
    assert tracker.min_iou == (1, 2) and pk.components.Tracker().min_iou == (0, 1) and pk.components.Tracker(1).min_iou == (1, 1)
    labels, table = sequence('merge')[0]
    tracker.add_frame(to(labels), to(table))
    with pytest.raises(ValueError, match='labels of 7 points after a frame of %d' % len(labels)):
        tracker.add_frame(to(labels[:7]), to(table))
    for bad in (1.5, -0.1, (3, 2), (1, 0), (1, 2 ** 20 + 1)):
        with pytest.raises(ValueError, match='min_iou'):
            pk.components.Tracker(min_iou=bad)


def check_tracks_summary():
    """components.tracks on the host: per track id its frames, component numbers, sizes, centroids and boxes."""
    frames = sequence('move-appear')
    links = restate_tracker(frames, 0, 1)[0]
    objects = [dict(labels=f[0], table=f[1], link=l) for f, l in zip(frames, links)]
    got = pk.components.tracks(objects, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert sorted(got) == [0, 1] and got[0]['frames'].tolist() == [0, 1, 2, 3, 4] and got[1]['frames'].tolist() == [3, 4]
    assert got[0]['components'].tolist() == [0, 0, 0, 1, 1] and got[1]['components'].tolist() == [0, 0]
    assert got[0]['size'].tolist() == [4 * 4 * 8] * 5 and got[0]['centroid'].dtype == np.float64
    assert got[0]['centroid'][:, 0].tolist() == [4.0, 5.0, 6.0, 7.0, 8.0] and got[0]['box_min'][:, 0].tolist() == [2.5, 3.5, 4.5, 5.5, 6.5]
    assert got[1]['box_max'].tolist() == [[1.5, 5.5, 29.5]] * 2 and pk.components.tracks([], (0, 0, 0), (1, 1, 1)) == {}


# ---------------------------------------------------------------------------------------------------------------- end to end
def restate_links(results, num, den):
    return restate_tracker([(r['components']['labels'], r['components']['table']) for r in results], num, den)[0]


def check_end_to_end(shared):
    """perform_inference(components=..., tracker=...): three calls at different levels stand in for three frames; `link` equals the
    restatement run over the returned labels and tables, and everything else is the call's without a tracker."""
    tracker = pk.components.Tracker(min_iou=0.25)
    options = [pk.components.Components(level=level, connectivity=c) for level, c in ((0.5, 6), (0.47, 26), (0.53, 6))]
    results = [rc.infer(shared.device, shared.inputs, components=o, tracker=tracker) for o in options]
    for got, link in zip(results, restate_links(results, 1, 4)):
        comp = got['components']
        assert sorted(comp) == ['labels', 'link', 'table'] and comp['link'].dtype == np.int32 and comp['link'].shape == (len(comp['table']), 4)
        assert np.array_equal(comp['link'], link)
        rc.same_result({k: v for k, v in got.items() if k != 'components'}, shared.dense)
    assert results[0]['components']['link'][:, 0].tolist() == list(range(len(results[0]['components']['table'])))
    assert len(results[0]['components']['table']) >= 1 and (results[1]['components']['link'][:, 1] >= 0).any()
    plain = rc.infer(shared.device, shared.inputs, components=options[1])
    for key in ('labels', 'table'):
        assert np.array_equal(plain['components'][key], results[1]['components'][key])
    # track_mode 'all' and refine: the labels are those of the merged, expanded array
    tracker.reset()
    results = [rc.infer(shared.device, shared.inputs, track_mode='all', components=options[0], tracker=tracker),
               rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), components=options[1], tracker=tracker)]
    for got, link in zip(results, restate_links(results, 1, 4)):
        assert np.array_equal(got['components']['link'], link)
    assert tracker.n_tracks() == max(int(r['components']['link'][:, 0].max()) for r in results) + 1


def check_clip(shared):
    """evaluate_clip(components=..., objects=[], tracker=...) over three frames: the tracker is reset first, every dict gains
    `link`, the tuples of pcl_all keep their contract."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared, n_frames=3)
    option, tracker = pk.components.Components(connectivity=26), pk.components.Tracker(min_iou=(1, 3))
    tracker.add_frame(torch.zeros(5, dtype=torch.int32, device=shared.device), torch.full((1, 12), 5, dtype=torch.int64, device=shared.device))
    objects = []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, components=option, objects=objects,
                                       tracker=tracker)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(objects) == 3
    for t in range(3):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    links = restate_tracker([(o['labels'], o['table']) for o in objects], 1, 3)
    for o, link in zip(objects, links[0]):
        assert sorted(o) == ['labels', 'link', 'table'] and np.array_equal(o['link'], link)
    assert tracker.n_tracks() == links[1] and objects[0]['link'][:, 0].tolist() == list(range(len(objects[0]['table'])))
    counts, mins, spacings = pk.geometry.grid_frame(rc.CASE['num_sample'], inf['min_z'], inf['cube_bounds'], 'greater', 4)
    tracks = pk.components.tracks(objects, mins, spacings)
    assert sorted(tracks) == list(range(links[1])) and sum(len(v['frames']) for v in tracks.values()) == sum(len(o['table']) for o in objects)
    for kw, text in ((dict(tracker=tracker), 'tracker needs components'), (dict(components=option, objects=[], tracker=0.5), 'tracker must be')):
        with pytest.raises(ValueError, match=text):
            pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', **kw)


def check_none_is_untouched(shared, monkeypatch):
    """tracker=None: the result's keys and arrays are exactly those of before, the entry points are not called; with a tracker
    still one host wait."""
    def forbidden(*a, **k):
        raise AssertionError('tracker=None must not reach the linking')
    before = rc.infer(shared.device, shared.inputs, components=pk.components.Components())
    monkeypatch.setattr(pk.ops, 'components_overlap', forbidden)
    monkeypatch.setattr(pk.ops, 'components_match', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, components=pk.components.Components(), tracker=None)
    assert sorted(res) == sorted(before) and sorted(res['components']) == ['labels', 'table']
    for key in ('labels', 'table'):
        assert np.array_equal(res['components'][key], before['components'][key])
    rc.same_result({k: v for k, v in res.items() if k != 'components'}, shared.dense)
    assert 'components' not in rc.infer(shared.device, shared.inputs)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, components=pk.components.Components(), tracker=pk.components.Tracker())
    assert calls['wait'] == 1


def check_value_errors(shared):
    with pytest.raises(ValueError, match='tracker needs components'):
        rc.infer(shared.device, shared.inputs, tracker=pk.components.Tracker())
    for bad in (0.5, pk.components.Components(), 'yes'):
        with pytest.raises(ValueError, match='tracker must be a components.Tracker or None'):
            rc.infer(shared.device, shared.inputs, components=pk.components.Components(), tracker=bad)
