"""The yardstick of the instance statistics (include/occ4d_inst.h): a plain numpy restatement of the frame table (the confusion
through np.add.at, the fixed-point sums as np.rint(x.astype(np.float64) * 2**20).astype(np.int64)) and of the fold (a Python loop
over the ids in float64), the seeded case generator of the kernel-level matrix and the checks shared by tests/test_inst_host.py
(the g++ twin) and tests/test_gpu_inst.py (the HIP kernels).  The restatement never calls the code under test; the layout offsets
are written out here and compared with the header's defines by a test.

What is compared how: frame tables and accumulated counts are integers and must be EQUAL.  The double sums are compared within
1e-9 relative (the `same_stats` figure of tests/eval_cases.py): a term is a quotient of two integers below 2^53, or a square root
of a sum of three squares, each correctly rounded in both implementations, and at most 64 non-negative terms are added in the
same order, so the true difference is a few ulp (2e-16); 1e-9 leaves room for a libm whose sqrt is off by an ulp and no more."""
import itertools

import numpy as np
import pytest
import torch

import occlusions4d_amd as pk

MAX_IDS, MAX_GROUPS = 64, 8
BAD_ROWS, FRAME_HEAD, POINT_WORDS, HEAD, GROUP_COUNTS, GROUP_SUMS = 0, 1, 4, 1, 8, 4
N_GT, N_PRED, N_MATCH, SUM_INTER, SUM_UNION, N_CENTROID = range(6)
SUM_IOU, SUM_IOU_MATCHED, SUM_CENTROID_D, SUM_CENTROID_D2 = range(4)
SIDE_PRED, SIDE_GT = 0, 1
SCALE = 2.0 ** 20
PAD = 3                                   # a strided operand of width d has ld = d + PAD
THRESHOLD, RADIUS = np.float32(0.5), np.float32(0.2)
GRID_CAP_ROWS = 1024 * 256                # rows one trip of the kernels' grid-stride loop covers (csrc/inststats.hip)
F32 = np.float32


def frame_len(n_ids):
    return FRAME_HEAD + (n_ids + 1) ** 2 + 2 * n_ids * POINT_WORDS


# ------------------------------------------------------------------------------------------------------------ the restatement
def id_class(v, n_ids):
    """int64 class per element of the float32 array v: i in [0, n_ids), n_ids = NONE, -1 = OTHER."""
    v = np.asarray(v, F32)
    out = np.full(v.shape, -1, np.int64)
    with np.errstate(invalid='ignore'):
        integral = (v >= 0) & (v < F32(n_ids)) & (v == np.floor(v))          # (-0.0 >= 0: class 0)
        out[v < 0] = n_ids
    out[integral] = v[integral].astype(np.int64)
    return out


def restate_confusion(frame, density, pred_id, nn_idx, nn_dist, target_id, n_ids, threshold=THRESHOLD, radius=RADIUS):
    m = len(target_id)
    idx = np.asarray(nn_idx, np.int64)
    bad = (idx < 0) | (idx >= m)
    safe = np.where(bad, 0, idx)
    with np.errstate(invalid='ignore'):
        solid, label = np.asarray(density, F32) >= F32(threshold), np.asarray(nn_dist, F32) < F32(radius)
    pred = np.where(solid, id_class(pred_id, n_ids), n_ids)
    gt_ids = np.asarray(target_id, F32)[safe] if m else np.zeros(len(idx), F32)
    gt = np.where(label, id_class(gt_ids, n_ids), n_ids)
    bad |= (pred < 0) | (gt < 0)
    C = n_ids + 1
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (gt[~bad], pred[~bad]), 1)
    frame[BAD_ROWS] += bad.sum()
    frame[FRAME_HEAD:FRAME_HEAD + C * C] += conf.ravel()


def restate_points(frame, rows, ids, n_ids, side):
    rows, cls = np.asarray(rows, F32)[:, :3], id_class(ids, n_ids)
    with np.errstate(invalid='ignore'):
        inside = (np.abs(rows) <= F32(1024)).all(axis=1)                        # (NaN and +-inf fail)
    named = (cls >= 0) & (cls < n_ids)
    bad, good = (cls < 0) | (named & ~inside), named & inside
    fixed = np.rint(rows[good].astype(np.float64) * 2 ** 20).astype(np.int64)   # (np.rint: half to even)
    table = np.zeros((n_ids, POINT_WORDS), np.int64)
    np.add.at(table[:, 0], cls[good], 1)
    for d in range(3):
        np.add.at(table[:, 1 + d], cls[good], fixed[:, d])
    lo = FRAME_HEAD + (n_ids + 1) ** 2 + side * n_ids * POINT_WORDS
    frame[BAD_ROWS] += bad.sum()
    frame[lo:lo + n_ids * POINT_WORDS] += table.ravel()


def split_frame(frame, n_ids):
    C = n_ids + 1
    conf = frame[FRAME_HEAD:FRAME_HEAD + C * C].reshape(C, C)
    pts = frame[FRAME_HEAD + C * C:].reshape(2, n_ids, POINT_WORDS)
    return conf, pts[SIDE_PRED], pts[SIDE_GT]


def restate_fold(frame, n_ids, inst_group, n_groups):
    """What one frame table adds: (counts int64, sums float64) in the library's layout."""
    conf, pred, gt = split_frame(frame, n_ids)
    counts, sums = np.zeros(HEAD + n_groups * GROUP_COUNTS, np.int64), np.zeros(n_groups * GROUP_SUMS, np.float64)
    counts[BAD_ROWS] = frame[BAD_ROWS]
    for i in range(n_ids):
        gt_q, pr_q, inter = int(conf[i].sum()), int(conf[:, i].sum()), int(conf[i, i])
        union = gt_q + pr_q - inter
        annotated, predicted = gt_q >= 1, pr_q >= 1
        if not annotated and not predicted:
            continue
        g = 0 if inst_group is None else int(inst_group[i])
        if g < 0 or g >= n_groups:
            counts[BAD_ROWS] += 1
            continue
        c, s = counts[HEAD + g * GROUP_COUNTS:HEAD + (g + 1) * GROUP_COUNTS], sums[g * GROUP_SUMS:(g + 1) * GROUP_SUMS]
        c[N_GT] += annotated
        c[N_PRED] += predicted
        c[SUM_INTER] += inter
        c[SUM_UNION] += union
        if annotated:
            iou = np.float64(inter) / np.float64(union)
            s[SUM_IOU] += iou
            if 2 * inter > union:
                c[N_MATCH] += 1
                s[SUM_IOU_MATCHED] += iou
            if pred[i, 0] >= 1 and gt[i, 0] >= 1:
                delta = [np.float64(pred[i, 1 + d]) / np.float64(pred[i, 0]) / SCALE - np.float64(gt[i, 1 + d]) / np.float64(gt[i, 0]) / SCALE
                         for d in range(3)]
                d2 = delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]
                c[N_CENTROID] += 1
                s[SUM_CENTROID_D] += np.sqrt(d2)
                s[SUM_CENTROID_D2] += d2
    return counts, sums


def closed_forms(counts, sums, n_groups):
    """The figures of InstanceStats.summary() from the arrays, written out with Python scalars."""
    def div(a, b):
        return float(a) / float(b) if b else float('nan')
    res = []
    for g in range(n_groups):
        c, s = counts[HEAD + g * GROUP_COUNTS:HEAD + (g + 1) * GROUP_COUNTS], sums[g * GROUP_SUMS:(g + 1) * GROUP_SUMS]
        match = int(c[N_MATCH])
        r = dict(instance_miou=div(s[SUM_IOU], c[N_GT]), instance_iou_micro=div(c[SUM_INTER], c[SUM_UNION]),
                 rq=div(match, match + 0.5 * (int(c[N_PRED]) - match) + 0.5 * (int(c[N_GT]) - match)), sq=div(s[SUM_IOU_MATCHED], match),
                 centroid_error=div(s[SUM_CENTROID_D], c[N_CENTROID]), centroid_error_sq=div(s[SUM_CENTROID_D2], c[N_CENTROID]))
        r['pq'] = r['sq'] * r['rq']
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------------------ kernel-level cases
def _ids(rng, n, n_ids, adversarial=True):
    """n float32 ids: mostly instance ids and -1, and every adversarial value of the issue in every cloud that has room."""
    v = rng.integers(-1, n_ids, size=n).astype(F32)
    if adversarial:
        pool = np.array([-1.0, -0.0, 0.5, n_ids, n_ids - 1, np.nan, np.inf, -np.inf, -2.5, 2.0 ** 31, -(2.0 ** 31), 1e-40], F32)
        where = rng.permutation(n)[:min(n, len(pool))] if n < 4 * len(pool) else rng.permutation(n)[:max(len(pool), n // 16)]
        v[where] = pool[np.arange(len(where)) % len(pool)]
    return v


def _coords(rng, n):
    x = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(F32)
    ties = ((2 * rng.integers(-4096, 4096, size=(n, 3)) + 1) * 2.0 ** -21).astype(F32)      # odd multiples of 2^-21: rounding ties
    pick = rng.uniform(size=(n, 3)) < 0.25
    x[pick] = ties[pick]
    pool = np.array([1024.0, -1024.0, np.nextafter(F32(1024), F32(np.inf)), 1e30, np.nan, 1e-40, -1.4e-45, np.inf, -np.inf,
                     -np.nextafter(F32(1024), F32(np.inf)), 1023.9999, 2.0 ** -21, 3 * 2.0 ** -21], F32)
    flat = x.reshape(-1)
    where = rng.permutation(flat.size)[:min(flat.size, max(len(pool), flat.size // 24))]
    flat[where] = pool[np.arange(len(where)) % len(pool)]
    return x


def make_case(seed, n, m, n_ids, n_groups, grouped, strided, special=None):
    """Seeded host-made inputs of one kernel-level case: no search is involved, every decision is exact.  n queries and n
    predicted rows, m target points."""
    rng = np.random.default_rng(seed)
    density = rng.uniform(0, 1, size=n).astype(F32)
    density[::7] = THRESHOLD                                       # exactly at the threshold: solid (>=)
    density[1::7] = np.nextafter(THRESHOLD, F32(0))                # its fp32 neighbours
    density[2::7] = np.nextafter(THRESHOLD, F32(1))
    if n > 16:
        density[5] = np.nan
    nn_dist = rng.uniform(0, 0.4, size=n).astype(F32)
    nn_dist[::5] = RADIUS                                          # exactly at the radius: no label (<)
    nn_dist[1::5] = np.nextafter(RADIUS, F32(0))
    nn_dist[2::5] = np.nextafter(RADIUS, F32(1))
    nn_idx = rng.integers(0, m, size=n).astype(np.int32)
    if n >= 3:
        nn_idx[n // 2], nn_idx[n // 3] = m, -1
    c = dict(n_ids=n_ids, n_groups=n_groups, strided=strided, density=density, pred_id=_ids(rng, n, n_ids), nn_idx=nn_idx, nn_dist=nn_dist,
             target_id=_ids(rng, m, n_ids), pred_rows=_coords(rng, n), pred_ids=_ids(rng, n, n_ids), gt_rows=_coords(rng, m))
    c['inst_group'] = rng.integers(0, n_groups, size=n_ids).astype(np.int32) if grouped else None
    if special == 'one_cell':                                      # every row in the cell (n_ids - 1, 0); every point on one id
        c['density'][:], c['nn_dist'][:], c['pred_id'][:], c['target_id'][:] = 0.9, 0.1, 0.0, n_ids - 1
        c['nn_idx'] = rng.integers(0, m, size=n).astype(np.int32)
        c['pred_ids'][:] = n_ids - 1
        c['pred_rows'] = rng.uniform(-1024.0, 1024.0, size=(n, 3)).astype(F32)
    elif special == 'all_none':                                    # the common grid: nothing solid, nothing near
        c['density'][:], c['nn_dist'][:] = 0.1, 0.3
        c['nn_idx'] = rng.integers(0, m, size=n).astype(np.int32)
    elif special == 'each_cell':                                   # one row per cell: n = (n_ids + 1)^2, m = n_ids + 1
        C = n_ids + 1
        assert n == C * C and m == C
        c['target_id'] = np.append(np.arange(n_ids), -1).astype(F32)
        c['nn_idx'] = (np.arange(n) // C).astype(np.int32)
        c['pred_id'] = np.where(np.arange(n) % C == n_ids, -1, np.arange(n) % C).astype(F32)
        c['density'][:], c['nn_dist'][:] = 0.9, 0.1
    elif special == 'bad_groups':                                  # a group id of -1 and of n_groups
        c['inst_group'] = rng.integers(0, n_groups, size=n_ids).astype(np.int32)
        c['inst_group'][0], c['inst_group'][n_ids - 1] = -1, n_groups
    return c


NS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
MS, IDS, GROUPS = (1, 7, 1000), (1, 12, 64), (1, 3, 8)
LARGE_N = GRID_CAP_ROWS + 257             # 262 401: a second trip of the grid-stride loop, for 257 rows


def matrix():
    """(id, make_case arguments): every n with every n_ids, contiguous and strided; m, n_groups and with / without inst_group
    cycle so that every value meets every n.  Once LARGE_N.  Then the special clouds."""
    cases = []
    for k, ((i, n), (j, n_ids), strided) in enumerate(itertools.product(enumerate(NS), enumerate(IDS), (False, True))):
        m, ng = MS[(i + j + strided) % 3], GROUPS[(i + 2 * j + strided) % 3]
        grouped = (i + j) % 2 == 0
        cases.append(('n%d-m%d-ids%d-g%d%s%s' % (n, m, n_ids, ng, '-grouped' if grouped else '', '-strided' if strided else ''),
                      (200 + k, n, m, n_ids, ng, grouped, strided)))
    cases.append(('large', (300, LARGE_N, 1000, 12, 3, True, True)))
    for n_ids in IDS:
        C = n_ids + 1
        cases.append(('one_cell-ids%d' % n_ids, (310 + n_ids, 1025, 7, n_ids, 3, True, False, 'one_cell')))
        cases.append(('each_cell-ids%d' % n_ids, (320 + n_ids, C * C, C, n_ids, 8, True, True, 'each_cell')))
    cases.append(('all_none', (330, 4099, 1000, 12, 1, False, False, 'all_none')))
    cases.append(('bad_groups', (331, 1025, 1000, 12, 3, True, False, 'bad_groups')))
    cases.append(('bad_groups-ids64', (332, 1025, 1000, 64, 8, True, True, 'bad_groups')))
    return cases


def want_case(c):
    frame = np.zeros(frame_len(c['n_ids']), np.int64)
    restate_confusion(frame, c['density'], c['pred_id'], c['nn_idx'], c['nn_dist'], c['target_id'], c['n_ids'])
    restate_points(frame, c['pred_rows'], c['pred_ids'], c['n_ids'], SIDE_PRED)
    restate_points(frame, c['gt_rows'], c['target_id'], c['n_ids'], SIDE_GT)
    return (frame,) + restate_fold(frame, c['n_ids'], c['inst_group'], c['n_groups'])


def column(a, strided, device):
    """The (n,) array as a device tensor: contiguous, or column 0 of an (n, 1 + PAD) tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if not strided:
        return t
    wide = torch.full((t.shape[0], 1 + PAD), 777, dtype=t.dtype, device=device)
    wide[:, 0] = t
    return wide[:, 0]


def rows3(a, strided, device):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if not strided:
        return t
    wide = torch.full((t.shape[0], 3 + PAD), 777.0, dtype=t.dtype, device=device)
    wide[:, :3] = t
    return wide[:, :3]


def place_case(c, device):
    dev, s = torch.device(device), c['strided']
    t = dict(density=column(c['density'], s, dev), pred_id=column(c['pred_id'], s, dev), nn_idx=column(c['nn_idx'], False, dev),
             nn_dist=column(c['nn_dist'], False, dev), target_id=column(c['target_id'], s, dev), pred_rows=rows3(c['pred_rows'], s, dev),
             pred_ids=column(c['pred_ids'], s, dev), gt_rows=rows3(c['gt_rows'], s, dev))
    t['inst_group'] = None if c['inst_group'] is None else torch.from_numpy(c['inst_group']).to(dev)
    if s and c['density'].shape[0] > 1:
        assert t['density'].stride(0) == 1 + PAD and t['pred_rows'].stride(0) == 3 + PAD
    return t


def run_placed(c, t, device, counts=None, sums=None, frame=None):
    """The four library calls on a zero-filled frame, onto (fresh or given) counts / sums -> (frame, counts, sums) tensors."""
    n_frame, n_counts, n_sums = pk.ops.inst_layout(c['n_ids'], c['n_groups'])
    dev = torch.device(device)
    frame = torch.zeros(n_frame, dtype=torch.int64, device=dev) if frame is None else frame.zero_()
    counts = torch.zeros(n_counts, dtype=torch.int64, device=dev) if counts is None else counts
    sums = torch.zeros(n_sums, dtype=torch.float64, device=dev) if sums is None else sums
    pk.ops.inst_confusion(t['density'], t['pred_id'], t['nn_idx'], t['nn_dist'], t['target_id'], frame, n_ids=c['n_ids'],
                          density_threshold=float(THRESHOLD), radius=float(RADIUS))
    pk.ops.inst_points(t['pred_rows'], t['pred_ids'], frame, n_ids=c['n_ids'], side=SIDE_PRED)
    pk.ops.inst_points(t['gt_rows'], t['target_id'], frame, n_ids=c['n_ids'], side=SIDE_GT)
    pk.ops.inst_fold(frame, counts, sums, n_ids=c['n_ids'], n_groups=c['n_groups'], inst_group=t['inst_group'])
    return frame, counts, sums


def run_case(c, device):
    return tuple(x.cpu().numpy() for x in run_placed(c, place_case(c, device), device))


def same_stats(got, want, rel=1e-9, what=''):
    """Frame and counts equal; sums within `rel` relative (the terms are non-negative)."""
    for k in (0, 1):
        diff = np.flatnonzero(got[k] != want[k])
        assert got[k].shape == want[k].shape and diff.size == 0, (what, k, diff[:8], got[k][diff[:8]], want[k][diff[:8]])
    err = np.abs(got[2] - want[2])
    assert np.all(err <= rel * np.abs(want[2])), (what, got[2], want[2])


def check_case(args, device):
    c = make_case(*args)
    got, want = run_case(c, device), want_case(c)
    same_stats(got, want, what=str(args))
    return c, got, want


def check_matrix(device):
    """Every case of the matrix; -> the number of cases.  Also asserts that the matrix exercises what it is there for."""
    seen = dict(bad=0, conf=0, cent=0, neg=0)
    for name, args in matrix():
        c, got, want = check_case(args, device)
        seen['bad'] += int(got[0][BAD_ROWS] > 0)
        seen['conf'] += int(np.count_nonzero(got[0][FRAME_HEAD:FRAME_HEAD + (c['n_ids'] + 1) ** 2]) > 1)
        seen['cent'] += int(got[1][HEAD:].reshape(-1, GROUP_COUNTS)[:, N_CENTROID].sum() > 0)
        seen['neg'] += int((got[0] < 0).any())
        if name.startswith('one_cell'):
            conf = split_frame(got[0], c['n_ids'])[0]
            assert conf[c['n_ids'] - 1, 0] == 1025 == conf.sum(), name
            assert np.abs(split_frame(got[0], c['n_ids'])[1][:, 1:]).max() > 2 ** 32, name      # (sums beyond 32 bits)
        elif name.startswith('each_cell'):
            assert (split_frame(got[0], c['n_ids'])[0] == 1).all(), name
        elif name == 'all_none':
            conf = split_frame(got[0], c['n_ids'])[0]
            assert conf[-1, -1] == 4099 == conf.sum(), name
        elif name.startswith('bad_groups'):
            assert got[1][BAD_ROWS] >= got[0][BAD_ROWS] + 1, name
    assert min(seen.values()) > 0, seen
    return len(matrix())


def check_ties_round_to_even(device):
    """Odd multiples of 2^-21 are ties of the fixed-point rounding: half to even, in both directions."""
    k = np.array([1, 3, 5, -1, -3, -5, 2 ** 20 + 1], np.float64)
    x = (k * 2.0 ** -21).astype(F32)
    assert np.array_equal(x.astype(np.float64), k * 2.0 ** -21)
    rows = np.zeros((len(k), 3), F32)
    rows[:, 0] = x
    frame = torch.zeros(frame_len(len(k)), dtype=torch.int64, device=device)
    pk.ops.inst_points(torch.from_numpy(rows).to(device), torch.arange(len(k), dtype=torch.float32, device=device), frame, n_ids=len(k),
                       side=SIDE_GT)
    got = split_frame(frame.cpu().numpy(), len(k))[2]
    assert got[:, 0].tolist() == [1] * len(k) and got[:, 1].tolist() == [0, 2, 2, 0, -2, -2, 2 ** 19], got[:, 1]
    assert not got[:, 2:].any()


def check_thresholds(device):
    """density == threshold is solid (>=), nn_dist == radius carries no label (<): four rows decide it."""
    below_t, below_r = np.nextafter(THRESHOLD, F32(0)), np.nextafter(RADIUS, F32(0))
    c = dict(n_ids=2, n_groups=1, strided=False, inst_group=None, density=np.array([THRESHOLD, below_t, THRESHOLD, below_t], F32),
             nn_dist=np.array([RADIUS, RADIUS, below_r, below_r], F32), pred_id=np.zeros(4, F32), nn_idx=np.zeros(4, np.int32),
             target_id=np.ones(1, F32), pred_rows=np.zeros((0, 3), F32), pred_ids=np.zeros(0, F32), gt_rows=np.zeros((1, 3), F32))
    conf = split_frame(run_case(c, device)[0], 2)[0]
    assert conf.tolist() == [[0, 0, 0], [1, 0, 1], [1, 0, 1]], conf          # rows: gt 0, gt 1, none; columns: pred 0, pred 1, none


def check_repeatable(device, streams=None):
    """The same calls give the same bits: twice in a row, and (on the device) on three streams."""
    args = dict(matrix())['large']
    c = make_case(*args)
    t = place_case(c, device)
    first = [x.clone() for x in run_placed(c, t, device)]
    again = run_placed(c, t, device)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert first[2].abs().sum() > 0 and torch.equal(first[2].view(torch.int64), again[2].view(torch.int64))
    for s in (streams or []):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = run_placed(c, t, device)
        s.synchronize()
        assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(first, got))


def check_twice_doubles(device):
    """One frame folded twice onto zeros doubles every entry exactly; the fold leaves the frame as it is."""
    for name in ('large', 'bad_groups-ids64', 'each_cell-ids12'):
        args = dict(matrix())[name]
        c = make_case(*args)
        t = place_case(c, device)
        frame, counts, sums = run_placed(c, t, device)
        once = (frame.clone(), counts.clone(), sums.clone())
        pk.ops.inst_fold(frame, counts, sums, n_ids=c['n_ids'], n_groups=c['n_groups'], inst_group=t['inst_group'])
        assert torch.equal(frame, once[0]) and torch.equal(counts, 2 * once[1]) and torch.equal(sums, 2 * once[2]), name
        assert once[2].abs().sum() > 0, name


# ------------------------------------------------------------------------------------------------------------ InstanceStats
def hand_frame():
    """Three instances whose IoUs are 1, exactly 0.5 and 0, as add_frame inputs with the search given.  Target: 2 points per
    instance.  Queries: instance 0: 4 labelled, 4 predicted (IoU 1); instance 1: 3 labelled, 2 of them predicted 1, one not solid,
    and one unlabelled query predicted 1 (inter 2, union 4); instance 2: 2 labelled, none solid (IoU 0); 3 queries of nothing."""
    target = np.zeros((6, 9), F32)
    target[:, :3] = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 6, 2], [5, 5, 5], [7, 5, 5]], F32)
    target[:, 3] = [0, 0, 1, 1, 2, 2]
    #            gt id (via nn_idx)   near  solid pred id
    rows = [(0, True, True, 0)] * 4 + [(2, True, True, 1)] * 2 + [(3, True, False, 1)] + [(2, False, True, 1)] + \
           [(4, True, False, 2), (5, True, False, -1)] + [(0, False, False, 0)] * 3
    n = len(rows)
    rng = np.random.default_rng(5)
    q = np.zeros((n, 4), F32)
    q[:, :3] = rng.uniform(-2, 8, size=(n, 3)).astype(F32)
    out = np.zeros((n, 5), F32)
    out[:, 0] = [0.9 if r[2] else 0.1 for r in rows]
    out[:, 4] = [r[3] for r in rows]
    nn_idx = np.array([r[0] for r in rows], np.int32)
    nn_dist = np.array([0.05 if r[1] else 0.7 for r in rows], F32)
    solid = out[:, 0] >= 0.5
    cent_pred = {i: q[solid & (out[:, 4] == i), :3].astype(np.float64).mean(0) for i in (0, 1)}
    cent_gt = {i: target[target[:, 3] == i, :3].astype(np.float64).mean(0) for i in (0, 1, 2)}
    return dict(q=q, out=out, target=target, nn=(nn_idx, nn_dist), cent_pred=cent_pred, cent_gt=cent_gt)


def add_hand(stats, h, device, **kw):
    dev = torch.device(device)
    nn = (torch.from_numpy(h['nn'][0]).to(dev), torch.from_numpy(h['nn'][1]).to(dev))
    return stats.add_frame(torch.from_numpy(h['q']).to(dev), torch.from_numpy(h['out']).to(dev), h['target'], density_threshold=0.5,
                           point_occupancy_radius=0.2, color_mode='rgb', data_kind='greater', nn=nn, **kw)


def check_hand_summary(device):
    h = hand_frame()
    s = add_hand(pk.evaluation.InstanceStats(3, 1, device), h, device)
    r = s.summary()
    c = r['counts']
    assert (c['n_gt'][0], c['n_pred'][0], c['n_match'][0], c['sum_inter'][0], c['sum_union'][0], c['n_centroid'][0]) == (3, 2, 1, 6, 10, 2)
    assert r['bad_rows'] == 0
    d = [np.sqrt(((h['cent_pred'][i] - h['cent_gt'][i]) ** 2).sum()) for i in (0, 1)]
    want = dict(instance_miou=1.5 / 3, instance_iou_micro=0.6, rq=1 / (1 + 0.5 * 1 + 0.5 * 2), sq=1.0, pq=0.4,
                centroid_error=(d[0] + d[1]) / 2, centroid_error_sq=(d[0] ** 2 + d[1] ** 2) / 2)
    assert sorted(want) == sorted(k for k in r if k not in ('counts', 'bad_rows'))
    for k, v in want.items():
        tol = 1e-5 if k.startswith('centroid') else 1e-12       # (the table's centroids are within 2^-20 per coordinate of the means)
        assert r[k].shape == (1,) and r[k].dtype == np.float64 and abs(r[k][0] - v) <= tol, (k, r[k], v)
    ft = s.frame_tables()
    assert ft['confusion'].tolist() == [[4, 0, 0, 0], [0, 2, 0, 1], [0, 0, 0, 2], [0, 1, 0, 3]] and ft['bad_rows'] == 0
    assert ft['pred']['count'].tolist() == [4, 3, 0] and ft['gt']['count'].tolist() == [2, 2, 2]
    assert np.isnan(ft['pred']['centroid'][2]).all() and ft['pred']['centroid'].shape == (3, 3) and ft['pred']['centroid'].dtype == np.float64
    for i in (0, 1):
        assert np.abs(ft['pred']['centroid'][i] - h['cent_pred'][i]).max() <= 2.0 ** -20
    for i in (0, 1, 2):
        assert np.abs(ft['gt']['centroid'][i] - h['cent_gt'][i]).max() <= 2.0 ** -20
    # the same through the closed forms of the restatement, per group: instance 0 alone, 1 and 2 together, group 2 empty
    g = add_hand(pk.evaluation.InstanceStats(3, 3, device), h, device, inst_group=np.array([0, 1, 1]))
    st = g.state()
    got, forms = g.summary(), closed_forms(st['counts'], st['sums'], 3)
    for k in want:
        for grp in range(3):
            a, b = got[k][grp], forms[grp][k]
            assert (np.isnan(a) and np.isnan(b)) or a == b, (k, grp, a, b)
    assert got['instance_miou'].tolist()[:2] == [1.0, 0.25] and np.isnan(got['instance_miou'][2]) and np.isnan(got['sq'][1])
    assert got['rq'].tolist()[:2] == [1.0, 0.0]
    # another labelling through pred_id: everything predicted as its label, nothing else solid -> every IoU 1
    idx, dist = h['nn']
    perfect = np.where(dist < 0.2, h['target'][idx, 3], -1).astype(F32)
    out = h['out'].copy()
    out[:, 0] = np.where(perfect >= 0, 0.9, 0.1)
    p = add_hand(pk.evaluation.InstanceStats(3, 1, device), dict(h, out=out), device, pred_id=torch.from_numpy(perfect).to(device)).summary()
    assert p['instance_miou'][0] == 1.0 and p['pq'][0] == 1.0 and p['counts']['n_centroid'][0] == 3
    # no queries: a no-op
    e = pk.evaluation.InstanceStats(3, 1, device)
    e.add_frame(np.zeros((0, 4), F32), np.zeros((0, 5), F32), h['target'], density_threshold=0.5, point_occupancy_radius=0.2,
                color_mode='rgb', data_kind='greater')
    assert not e.counts.any() and not e.sums.any() and all(np.isnan(v).all() for k, v in e.summary().items() if k not in ('counts', 'bad_rows'))


def check_merge_and_state(device):
    h = hand_frame()
    new = lambda: pk.evaluation.InstanceStats(3, 3, device)
    grp = np.array([2, 0, 1])
    one = add_hand(new(), h, device, inst_group=grp)
    other = add_hand(new(), dict(h, out=other_out(h)), device, inst_group=grp)
    both = add_hand(add_hand(new(), h, device, inst_group=grp), dict(h, out=other_out(h)), device, inst_group=grp)
    merged = add_hand(new(), h, device, inst_group=grp).merge(other)
    assert torch.equal(merged.counts, both.counts) and torch.equal(merged.sums, both.sums) and not torch.equal(merged.counts, one.counts)
    inplace = add_hand(new(), h, device, inst_group=grp)
    inplace += other
    assert torch.equal(inplace.counts, merged.counts) and torch.equal(inplace.sums, merged.sums)
    twice = add_hand(add_hand(new(), h, device, inst_group=grp), h, device, inst_group=grp)
    assert torch.equal(twice.counts, 2 * one.counts) and torch.equal(twice.sums, 2 * one.sums)
    with pytest.raises(AssertionError, match='do not add'):
        merged.merge(pk.evaluation.InstanceStats(3, 2, device))
    back = pk.evaluation.InstanceStats.from_state(merged.state(), device)
    assert (back.n_ids, back.n_groups) == (3, 3) and torch.equal(back.counts, merged.counts) and torch.equal(back.sums, merged.sums)
    assert back.counts.dtype == torch.int64 and back.sums.dtype == torch.float64
    # objects of different n_ids add (the lengths of counts / sums depend on n_groups alone: ops.inst_layout), the left one's n_ids stays
    wide = pk.evaluation.InstanceStats(5, 3, device)
    wide.counts += torch.arange(1, wide.counts.numel() + 1, dtype=torch.int64, device=wide.device)
    wide.sums += 0.5 * torch.arange(1, wide.sums.numel() + 1, dtype=torch.float64, device=wide.device)
    back += wide
    assert torch.equal(back.counts, merged.counts + wide.counts) and torch.equal(back.sums, merged.sums + wide.sums)
    assert not torch.equal(back.counts, merged.counts) and not torch.equal(back.sums, merged.sums)
    assert pk.evaluation.InstanceStats.from_state(back.state(), device).n_ids == 3
    # the two scorers do not add to each other, whatever their fields say
    with pytest.raises(AssertionError, match='do not add'):
        merged.merge(pk.evaluation.EvalStats(3, 0, device))
    with pytest.raises(AssertionError, match='do not add'):
        pk.evaluation.EvalStats(3, 0, device).merge(merged)
    bad = add_hand(new(), h, device, inst_group=np.array([0, 3, 1]))
    with pytest.raises(ValueError, match='1 rows or ids'):
        bad.summary()


def other_out(h):
    """The hand frame with every query predicted as instance 1."""
    return np.where(np.arange(5) == 4, np.float32(1), h['out']).astype(F32)


def check_argument_errors(device):
    """The contracts of the three entry points, as the library on `device` states them (csrc/inst_math.hpp: one source for both
    libraries).  Every non-null pointer is a real tensor that covers the call even if it were accepted."""
    z = lambda *shape, **kw: torch.zeros(*shape, device=device, **kw)
    I32, I64, F64 = torch.int32, torch.int64, torch.float64
    frame, counts, sums = z(frame_len(2), dtype=I64), z(9, dtype=I64), z(4, dtype=F64)
    col, idx, tid, rows = z(4), z(4, dtype=I32), z(3), z(4, 3)
    with pytest.raises(AssertionError, match='n_ids'):
        pk.ops.inst_layout(0)
    with pytest.raises(AssertionError, match='n_ids'):
        pk.ops.inst_layout(65)
    with pytest.raises(AssertionError, match='n_groups'):
        pk.ops.inst_layout(2, 9)
    with pytest.raises(AssertionError, match='frame'):
        pk.ops.inst_confusion(col, col, idx, col, tid, frame[:-1], n_ids=2)
    with pytest.raises(AssertionError, match='nn_idx'):
        pk.ops.inst_confusion(col, col, idx[:3], col, tid, frame, n_ids=2)
    with pytest.raises(AssertionError, match='side = 2'):
        pk.ops.inst_points(rows, col, frame, n_ids=2, side=2)
    with pytest.raises(AssertionError, match='rows must be'):
        pk.ops.inst_points(z(4, 2), col, frame, n_ids=2, side=0)
    with pytest.raises(AssertionError, match='inst_group'):
        pk.ops.inst_fold(frame, counts, sums, n_ids=2, inst_group=z(3, dtype=I32))
    with pytest.raises(AssertionError):
        pk.ops.inst_fold(frame, counts[:-1], sums, n_ids=2)
    with pytest.raises(AssertionError):
        pk.evaluation.InstanceStats(65, 1, device)
    with pytest.raises(AssertionError):
        pk.evaluation.InstanceStats(3, 9, device)
    L, p, E = pk._lib.lib(), pk.ops._ptr, pk._lib.EINVAL                 # what no tensor can express
    assert [L.occ4d_inst_frame_len(k) for k in (0, 1, 12, 64, 65)] == [-1, frame_len(1), frame_len(12), frame_len(64), -1]
    assert [L.occ4d_inst_counts_len(k) for k in (0, 1, 8, 9)] == [-1, 9, 65, -1] and [L.occ4d_inst_sums_len(k) for k in (0, 1, 8, 9)] == [-1, 4, 32, -1]
    conf = lambda **k: L.occ4d_inst_confusion_f32(*[k.get(name, default) for name, default in (
        ('density', p(col)), ('ld_density', 1), ('pred_id', p(col)), ('ld_pred', 1), ('n', 4), ('nn_idx', p(idx)), ('nn_dist', p(col)),
        ('target_id', p(tid)), ('ld_target', 1), ('m', 3), ('n_ids', 2), ('threshold', 0.5), ('radius', 0.2), ('frame', p(frame)), ('stream', None))])
    assert conf() == pk._lib.OK
    for kw in (dict(n_ids=0), dict(n_ids=65), dict(n=-1), dict(m=-1), dict(ld_density=0), dict(ld_pred=0), dict(ld_target=0), dict(frame=None),
               dict(density=None), dict(pred_id=None), dict(nn_idx=None), dict(nn_dist=None), dict(target_id=None)):
        assert conf(**kw) == E and b'occ4d_inst_confusion_f32' in L.occ4d_last_error(), kw
    assert conf(n=0, density=None, pred_id=None, nn_idx=None, nn_dist=None, target_id=None) == pk._lib.OK
    pts = lambda **k: L.occ4d_inst_points_f32(*[k.get(name, default) for name, default in (
        ('rows', p(rows)), ('ld', 3), ('n', 4), ('id', p(col)), ('ld_id', 1), ('n_ids', 2), ('side', 1), ('frame', p(frame)), ('stream', None))])
    assert pts() == pk._lib.OK
    for kw in (dict(n_ids=0), dict(n_ids=65), dict(n=-1), dict(ld=2), dict(ld_id=0), dict(side=2), dict(side=-1), dict(frame=None), dict(rows=None),
               dict(id=None)):
        assert pts(**kw) == E and b'occ4d_inst_points_f32' in L.occ4d_last_error(), kw
    assert pts(n=0, rows=None, id=None) == pk._lib.OK
    fold = lambda **k: L.occ4d_inst_fold(*[k.get(name, default) for name, default in (
        ('frame', p(frame)), ('n_ids', 2), ('inst_group', None), ('n_groups', 1), ('counts', p(counts)), ('sums', p(sums)), ('stream', None))])
    for kw in (dict(n_ids=0), dict(n_ids=65), dict(n_groups=0), dict(n_groups=9), dict(frame=None), dict(counts=None), dict(sums=None)):
        assert fold(**kw) == E and b'occ4d_inst_fold' in L.occ4d_last_error(), kw
    # the two accepted calls counted 4 queries in the cell (gt 0, none) and 4 ground-truth points of id 0 at the origin; nothing
    # else was written
    f = frame.cpu().numpy()
    assert f[FRAME_HEAD + 2] == 4 and f[FRAME_HEAD + 9 + 2 * POINT_WORDS] == 4 and f.sum() == 8 and not counts.any() and not sums.any()


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E_IDS = 4                                # the fixture follows the ids 0, 1, 2; id 3 stays empty


def e2e_group(time_idx, frame_rows):
    """An inst_group_fn: ids 0 and 1 in a group that alternates with the frame, the others in group 1."""
    return np.array([time_idx % 2, time_idx % 2, 1, 1], np.int32)


def restate_result(res, target, nn, n_ids, inst_group, n_groups, radius, threshold=0.5, track=4):
    """(frame, counts, sums) of one perform_inference result: the restatement fed with the returned implicit_output and
    points_query, the target rows and the query -> target search `nn` = (idx, dist) as numpy."""
    out, q = res['implicit_output'], res['points_query']
    solid = out[:, 0] >= F32(threshold)
    frame = np.zeros(frame_len(n_ids), np.int64)
    restate_confusion(frame, out[:, 0], out[:, track], nn[0], nn[1], target[:, 3], n_ids, threshold=threshold, radius=radius)
    restate_points(frame, q[solid, :3], out[solid, track], n_ids, SIDE_PRED)
    restate_points(frame, target[:, :3], target[:, 3], n_ids, SIDE_GT)
    return (frame,) + restate_fold(frame, n_ids, inst_group, n_groups)


def check_end_to_end(device, monkeypatch):
    """perform_inference(track_mode='all', inst_stats=..., stats=...) on the tracking fixture (768 points, 1500 queries asked for):
    the result dict is what it is without the scorers, the host waits once, and the InstanceStats equals the restatement."""
    import track_cases as tc
    inputs = tc.nets(device)
    pcl, sem, target, inf, enc, dec = inputs
    calls = dict(wait=0)
    wait = pk.inference._HostCopies.wait

    def counted_wait(self):
        calls['wait'] += 1
        return wait(self)
    monkeypatch.setattr(pk.inference._HostCopies, 'wait', counted_wait)
    plain = tc.infer(device, inputs)
    assert calls == dict(wait=1)
    grp = e2e_group(1, target)
    inst, stats = pk.evaluation.InstanceStats(E2E_IDS, 2, device), pk.evaluation.EvalStats(1, 0, device)
    scored = tc.infer(device, inputs, inst_stats=inst, stats=stats, inst_group=grp)
    assert calls == dict(wait=2)                                   # (one more: the scorers add no host wait)
    tc.same_result(plain, scored)
    alone = pk.evaluation.EvalStats(1, 0, device)
    tc.same_result(plain, tc.infer(device, inputs, stats=alone))
    assert torch.equal(alone.counts, stats.counts) and torch.equal(alone.sums, stats.sums)      # (EvalStats is not disturbed)
    # the fixture's condition: two distinct instance ids among the predicted-solid queries, an id with a non-empty intersection
    out = scored['implicit_output']
    solid_ids = np.unique(out[out[:, 0] >= 0.5, 4])
    ft = inst.frame_tables()
    assert len(solid_ids[solid_ids >= 0]) >= 2 and np.diag(ft['confusion'])[:E2E_IDS].max() > 0, (solid_ids, ft['confusion'])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    idx, dist = pk.inference.nn_target(to(scored['points_query'][:, :3]), to(target[:, :3]))
    want = restate_result(scored, target, (idx.cpu().numpy(), dist.cpu().numpy()), E2E_IDS, grp, 2, radius=0.8)
    st = inst.state()
    same_stats((inst.frame.cpu().numpy(), st['counts'], st['sums']), want, what='end to end')
    assert st['counts'][BAD_ROWS] == 0 and want[1][HEAD:].reshape(2, GROUP_COUNTS)[:, N_GT].tolist() == [0, 3]
    summary, forms = inst.summary(), closed_forms(want[1], want[2], 2)
    for k in forms[1]:
        a, b = summary[k][1], forms[1][k]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * abs(b), (k, a, b)
    return inst


def check_clip_end_to_end(device):
    """evaluate_clip(inst_stats=..., inst_group_fn=...) over two frames = two add_frame calls on the two decodes; the clip's
    arrays are what they are without the scorer."""
    import types

    import track_cases as tc
    pcl, sem, target, inf, enc, dec = tc.nets(device)
    second = target[:257].copy()
    second[:, :3] *= np.float32(0.5)
    frames = [target, second]
    batch = dict(pcl_input=pcl, pcl_input_sem=torch.from_numpy(sem)[None], pcl_target=[torch.from_numpy(f)[None] for f in frames],
                 meta_data=dict(pcl_target_size=[torch.tensor([f.shape[0]]) for f in frames]))
    args = types.SimpleNamespace(min_z=inf['min_z'], cr_cube_bounds=inf['cube_bounds'], color_mode=inf['color_mode'],
                                 sample_implicit=True, num_sample=tc.CASE['num_sample'], point_sample_mode='grid',
                                 implicit_batch_size=tc.CASE['batch_size'], segmentation_lw=0.0, track_mode='all',
                                 point_occupancy_radius=0.8, semantic_classes=13, density_threshold=0.5, cube_mode=4)
    clip = pk.evaluation.InstanceStats(E2E_IDS, 2, device)
    pcl_all = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, inst_stats=clip, inst_group_fn=e2e_group)
    bare = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True)
    for a, b in zip(pcl_all, bare):
        assert len(a) == len(b) == 7 and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    two = pk.evaluation.InstanceStats(E2E_IDS, 2, device)
    tables = []
    for t, frame in enumerate(frames):
        res = pk.inference.perform_inference(
            pcl.clone(), sem.copy(), None, [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=tc.CASE['num_sample'], point_sample_mode='grid', batch_size=tc.CASE['batch_size'],
            predict_segmentation=False, track_mode='all', semantic_classes=13, density_threshold=0.5, data_kind='greater', cube_mode=4,
            compress_air=True, point_occupancy_radius=0.8)
        assert np.array_equal(res['points_query'], pcl_all[t][6])
        two.add_frame(res['points_query'], res['implicit_output'], frame, density_threshold=0.5, point_occupancy_radius=0.8,
                      color_mode=inf['color_mode'], data_kind='greater', inst_group=e2e_group(t, frame))
        tables.append(two.frame_tables())
    assert torch.equal(clip.counts, two.counts) and torch.equal(clip.sums, two.sums) and torch.equal(clip.frame, two.frame)
    assert clip.counts[HEAD:].sum() > 0 and clip.counts[BAD_ROWS] == 0 and not np.array_equal(tables[0]['confusion'], tables[1]['confusion'])
    assert tables[1]['gt']['count'].sum() == (frames[1][:, 3] >= 0).sum()      # every labelled target point, near a query or not
