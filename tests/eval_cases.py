"""The yardstick of the evaluation statistics (include/occ4d_eval.h): a plain numpy float64 restatement of what a frame adds
to the two arrays, the seeded case generator of the kernel-level matrix and the runner shared by tests/test_eval_host.py (the
g++ twin) and tests/test_gpu_eval.py (the HIP kernels).  The restatement never calls the code under test; the layout offsets
are written out here and compared with the header's defines by a test."""
import itertools

import numpy as np
import pytest
import torch

import occlusions4d_amd as pk

HEAD, BAD_ROWS, GROUP_COUNTS, GROUP_SUMS = 1, 0, 16, 8
(OCC_TP, OCC_FP, OCC_FN, OCC_TN, TRACK_TP, TRACK_FP, TRACK_FN, TRACK_TN, SEG_IGNORED, N_ACCURACY, N_COMPLETENESS, N_COLOR,
 N_SEG) = range(13)
SUM_ACC_D, SUM_ACC_D2, SUM_COMP_D, SUM_COMP_D2, SUM_COLOR = range(5)
FLAG_COLOR, FLAG_TRACK, FLAG_SEG = 1, 2, 4
TRACK_IDX = {'rgb': 4, 'rgb_nosigmoid': 4, 'hsv': 15, 'bins': 10}
COLUMNS = {9: dict(col_rgb=5, col_track=8, col_sem=-1), 11: dict(col_rgb=7, col_track=10, col_sem=5)}
GRID_CAP_ROWS = 1024 * 256          # rows one trip of the kernels' grid-stride loop covers (csrc/evalstats.hip: GRID_CAP * THREADS)


def restate_rows(out, label, rows, grp, d, *, n_groups, n_classes, threshold, flags, col_rgb, col_track, col_sem, out_track,
                 bad=None, comp_dist=None, comp_group=None):
    """counts (int64), sums (float64) in the library's layout from per-query arrays: out (N, G) float32, label (N,) bool, rows
    (N, Dt) = every query's nearest target row, grp (N,) its group, d (N,) its distance (None: distance sums stay 0), bad (N,)
    bool = rows the library skips.  comp_dist (M,) / comp_group (M,): the completeness distances and groups of the target
    points (None: no completeness pass)."""
    C = n_classes
    stride = GROUP_COUNTS + C * C
    counts, sums = np.zeros(HEAD + n_groups * stride, np.int64), np.zeros(n_groups * GROUP_SUMS, np.float64)
    grp = np.asarray(grp, np.int64)
    bad = np.zeros(len(out), bool) if bad is None else bad.copy()
    bad |= (grp < 0) | (grp >= n_groups)
    counts[BAD_ROWS] += bad.sum()
    pred = out[:, 0] >= np.float32(threshold)
    label = np.asarray(label, bool)
    for g in range(n_groups):
        c, s = counts[HEAD + g * stride:HEAD + (g + 1) * stride], sums[g * GROUP_SUMS:(g + 1) * GROUP_SUMS]
        sel = ~bad & (grp == g)
        tp = sel & pred & label
        c[OCC_TP], c[OCC_FP] = tp.sum(), (sel & pred & ~label).sum()
        c[OCC_FN], c[OCC_TN] = (sel & ~pred & label).sum(), (sel & ~pred & ~label).sum()
        c[N_ACCURACY] = (sel & pred).sum()
        if d is not None:
            d64 = np.asarray(d)[sel & pred].astype(np.float64)
            s[SUM_ACC_D], s[SUM_ACC_D2] = d64.sum(), (d64 * d64).sum()
        o, t = out[tp], rows[tp]
        if flags & FLAG_COLOR and col_rgb >= 0:
            diff = np.abs(o[:, 1:4].astype(np.float64) - t[:, col_rgb:col_rgb + 3].astype(np.float64))
            c[N_COLOR], s[SUM_COLOR] = tp.sum(), (diff[:, 0] + diff[:, 1] + diff[:, 2]).sum()
        if flags & FLAG_TRACK and col_track >= 0:
            p, q = o[:, out_track] >= np.float32(0.5), t[:, col_track] > np.float32(0.5)
            c[TRACK_TP], c[TRACK_FP], c[TRACK_FN], c[TRACK_TN] = (p & q).sum(), (p & ~q).sum(), (~p & q).sum(), (~p & ~q).sum()
        if flags & FLAG_SEG and col_sem >= 0 and C >= 1:
            tag = t[:, col_sem].astype(np.float64)
            valid = (tag >= 0) & (tag < C) & (tag == np.floor(tag))
            col = np.argmax(o[:, o.shape[1] - C:], axis=1)                 # (numpy's argmax is the first one)
            conf = np.zeros((C, C), np.int64)
            np.add.at(conf, (tag[valid].astype(np.int64), col[valid]), 1)
            c[GROUP_COUNTS:] = conf.ravel()
            c[N_SEG], c[SEG_IGNORED] = valid.sum(), (~valid).sum()
        if comp_dist is not None:
            mine = np.asarray(comp_group, np.int64) == g
            cd = np.asarray(comp_dist)[mine].astype(np.float64)
            c[N_COMPLETENESS], s[SUM_COMP_D], s[SUM_COMP_D2] = mine.sum(), cd.sum(), (cd * cd).sum()
    if comp_dist is not None:
        cg = np.asarray(comp_group, np.int64)
        counts[BAD_ROWS] += ((cg < 0) | (cg >= n_groups)).sum()
    return counts, sums


def restate(out, nn_idx, nn_dist, target, *, radius, target_group=None, comp_dist=None, **kw):
    """restate_rows from the search results: nn_idx (N,), nn_dist (N,) (float32, or float64 of a CPU search)."""
    M = target.shape[0]
    idx = np.asarray(nn_idx, np.int64)
    bad = (idx < 0) | (idx >= M)
    safe = np.where(bad, 0, idx)
    tg = np.zeros(M, np.int64) if target_group is None else np.asarray(target_group, np.int64)
    return restate_rows(out, np.asarray(nn_dist) < np.float32(radius), target[safe], tg[safe], nn_dist, bad=bad, comp_dist=comp_dist,
                        comp_group=tg, **kw)


def closed_forms(counts, sums, n_groups, n_classes):
    """The figures of EvalStats.summary() from the arrays, written out with Python scalars."""
    stride, res = GROUP_COUNTS + n_classes * n_classes, []

    def div(a, b):
        return float(a) / float(b) if b else float('nan')
    for g in range(n_groups):
        c, s = counts[HEAD + g * stride:HEAD + (g + 1) * stride], sums[g * GROUP_SUMS:(g + 1) * GROUP_SUMS]
        tp, fp, fn = int(c[OCC_TP]), int(c[OCC_FP]), int(c[OCC_FN])
        conf = c[GROUP_COUNTS:].reshape(n_classes, n_classes)
        ious = [div(conf[k, k], conf[k].sum() + conf[:, k].sum() - conf[k, k]) for k in range(n_classes)
                if conf[k].sum() + conf[:, k].sum() > 0]
        r = dict(precision=div(tp, tp + fp), recall=div(tp, tp + fn), f1=div(2 * tp, 2 * tp + fp + fn), iou=div(tp, tp + fp + fn),
                 chamfer_accuracy=div(s[SUM_ACC_D], c[N_ACCURACY]), chamfer_completeness=div(s[SUM_COMP_D], c[N_COMPLETENESS]),
                 chamfer_accuracy_sq=div(s[SUM_ACC_D2], c[N_ACCURACY]), chamfer_completeness_sq=div(s[SUM_COMP_D2], c[N_COMPLETENESS]),
                 seg_accuracy=div(np.trace(conf), conf.sum()), seg_miou=div(sum(ious), len(ious)),
                 track_iou=div(c[TRACK_TP], c[TRACK_TP] + c[TRACK_FP] + c[TRACK_FN]), color_l1=div(s[SUM_COLOR], c[N_COLOR]))
        r['chamfer'] = r['chamfer_accuracy'] + r['chamfer_completeness']
        r['chamfer_sq'] = r['chamfer_accuracy_sq'] + r['chamfer_completeness_sq']
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------------------ kernel-level cases
def make_case(seed, N, M, n_groups, C, wide, Dt, color_mode='rgb', special=None):
    """Seeded host-made inputs of one kernel-level case: no search is involved, every decision is exact.  The output is a
    column slice of a wider array (row stride > G).  wide: G = base + C (segmentation scored when the target has a semantic
    column), else G = base (segmentation not scored; C still sizes the layout); base = 5, or 16 for 'hsv'."""
    rng = np.random.default_rng(seed)
    base = 16 if color_mode == 'hsv' else 5
    G = base + (C if wide else 0)
    thr, radius = np.float32(0.5), np.float32(0.2)
    out = rng.uniform(0, 1, size=(N, G + 3)).astype(np.float32)[:, 1:1 + G]      # (out.base: the wider array)
    out[::7, 0] = thr                                             # exactly at the threshold: solid (>=)
    nn_dist = rng.uniform(0, 0.4, size=N).astype(np.float32)
    nn_dist[::5] = radius                                          # exactly at the radius: label 0 (<)
    nn_idx = rng.integers(0, M, size=N).astype(np.int32)
    target = rng.uniform(0, 1, size=(M, Dt)).astype(np.float32)
    cols = COLUMNS[Dt]
    target[:, cols['col_track']] = rng.integers(0, 2, size=M)
    if cols['col_sem'] >= 0:
        target[:, cols['col_sem']] = rng.integers(0, max(C, 1), size=M)
    group = rng.integers(0, n_groups, size=M).astype(np.int32) if n_groups > 1 else None
    if special == 'all_solid':
        out[:, 0] = 0.9
    elif special == 'none_solid':
        out[:, 0] = 0.1
    elif special == 'all_label0':
        nn_dist[:] = rng.uniform(0.2, 0.4, size=N).astype(np.float32)
    elif special == 'tags':                                        # -1, C and 2.5 are no class: SEG_IGNORED
        target[0::3, cols['col_sem']] = -1.0
        target[1::3, cols['col_sem']] = float(C)
        target[2::3, cols['col_sem']] = 2.5
        target[M // 2, cols['col_sem']] = 0.0
        out[:, 0], nn_dist[:] = 0.9, 0.1                           # (every query an occupancy TP: every tag is looked at)
    elif special == 'bad':
        nn_idx[N // 2] = M
        group = rng.integers(0, n_groups, size=M).astype(np.int32)
        group[M // 3] = n_groups
    flags = (FLAG_COLOR if color_mode in ('rgb', 'rgb_nosigmoid') else 0) | FLAG_TRACK | (FLAG_SEG if wide and C > 0 else 0)
    return dict(out=out, nn_idx=nn_idx, nn_dist=nn_dist, target=target, target_group=group,
                comp_dist=rng.uniform(0, 0.5, size=M).astype(np.float32),
                kw=dict(n_groups=n_groups, n_classes=C, flags=flags, out_track=TRACK_IDX[color_mode], **cols),
                threshold=float(thr), radius=float(radius))


NS = (1, 255, 256, 257, 4099, GRID_CAP_ROWS + 257)       # the last: a second trip of the grid-stride loop, for 257 rows
MS, GROUPS, CLASSES = (1, 7, 1000), (1, 3, 8), (0, 1, 13, 32)


def matrix():
    """(id, make_case arguments): every N with every C, once with G = 5 + C and an 11-column target and once with G = 5 and a
    9-column target; M and n_groups cycle so that every value meets every N."""
    cases = []
    for k, ((i, N), (j, C), wide) in enumerate(itertools.product(enumerate(NS), enumerate(CLASSES), (True, False))):
        M, ng = MS[(i + j + wide) % 3], GROUPS[(i + 2 * j + wide) % 3]
        Dt = 11 if wide else 9
        cases.append(('N%d-M%d-g%d-C%d-G%d-D%d' % (N, M, ng, C, 5 + (C if wide else 0), Dt), (100 + k, N, M, ng, C, wide, Dt)))
    for tag, N, M, ng, C, Dt in (('cross-a', 4099, 1000, 8, 32, 9), ('cross-b', 257, 1, 3, 13, 11), ('cross-c', 255, 7, 1, 1, 9)):
        cases.append((tag, (90, N, M, ng, C, False, Dt)))           # (G = 5 against the other target width)
    return cases


SPECIALS = [(s, (7, 4099, 1000, 3, 13, True, 11, 'rgb', s)) for s in ('all_solid', 'none_solid', 'all_label0', 'tags')] + \
           [('hsv', (8, 4099, 1000, 3, 13, True, 11, 'hsv', None))]
BAD_CASE = (9, 4099, 1000, 3, 13, True, 11, 'rgb', 'bad')


def run_case(case, device):
    """The two library calls on fresh arrays -> (counts, sums) as numpy."""
    dev = torch.device(device)
    t = {k: (None if case[k] is None else torch.from_numpy(case[k]).to(dev)) for k in ('nn_idx', 'nn_dist', 'target', 'target_group', 'comp_dist')}
    wide = torch.from_numpy(np.ascontiguousarray(case['out'].base)).to(dev)
    out = wide[:, 1:1 + case['out'].shape[1]]                      # the same column slice on the device: row stride > G
    assert out.stride(0) > out.shape[1] or out.shape[0] == 1
    kw = case['kw']
    n_counts, n_sums = pk.ops.eval_layout(kw['n_groups'], kw['n_classes'])
    counts, sums = torch.zeros(n_counts, dtype=torch.int64, device=dev), torch.zeros(n_sums, dtype=torch.float64, device=dev)
    pk.ops.eval_target_stats(t['comp_dist'], counts, sums, n_groups=kw['n_groups'], n_classes=kw['n_classes'],
                             target_group=t['target_group'])
    pk.ops.eval_query_stats(out, t['nn_idx'], t['nn_dist'], t['target'], counts, sums, density_threshold=case['threshold'],
                            radius=case['radius'], target_group=t['target_group'], **kw)
    return counts.cpu().numpy(), sums.cpu().numpy()


def want_case(case):
    return restate(case['out'], case['nn_idx'], case['nn_dist'], case['target'], radius=case['radius'], threshold=case['threshold'],
                   target_group=case['target_group'], comp_dist=case['comp_dist'], **case['kw'])


def same_stats(got, want, rel=1e-9, what=''):
    """Counts equal; sums within `rel` relative (the terms are non-negative: only the order of the additions differs)."""
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero(got[0] != want[0])[:8], got[0][got[0] != want[0]][:8], want[0][got[0] != want[0]][:8])
    err = np.abs(got[1] - want[1])
    assert np.all(err <= rel * np.abs(want[1])), (what, got[1], want[1])


def check_case(args, device):
    case = make_case(*args)
    got, want = run_case(case, device), want_case(case)
    same_stats(got, want, what=str(args))
    return case, got, want


# ------------------------------------------------------------------------------------------------------------ end-to-end clouds
def cloud_case(seed=3, N=4099, M=1000, radius=0.05, n_groups=3):
    """Seeded clouds in the unit cube for add_frame end to end: queries (N, 4), output (N, 5), GREATER target rows (M, 9), groups,
    and the two searches done here in float64.  Asserts while generating that no query -> target distance lies within 1e-5 of the
    radius and that every nearest / second-nearest gap exceeds 1e-6: an fp32 search cannot decide differently."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0, 1, size=(N, 4)).astype(np.float32)
    out = rng.uniform(0, 1, size=(N, 5)).astype(np.float32)
    target = rng.uniform(0, 1, size=(M, 9)).astype(np.float32)
    target[:, 8] = rng.integers(0, 2, size=M)
    group = rng.integers(0, n_groups, size=M).astype(np.int32)

    def search(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        d = np.sqrt(sum((a[:, None, k] - b[None, :, k]) ** 2 for k in range(3)))
        two = np.partition(d, 1, axis=1)[:, :2] if b.shape[0] > 1 else np.stack([d[:, 0], d[:, 0] + 1], 1)
        assert (two[:, 1] - two[:, 0] > 1e-6).all(), 'nearest / second-nearest gap'
        return d.argmin(1), d.min(1)
    nn_idx, nn_dist = search(q[:, :3], target[:, :3])
    assert (np.abs(nn_dist - np.float64(np.float32(radius))) > 1e-5).all(), 'distance near the radius'
    solid = q[out[:, 0] >= np.float32(0.5)]
    _, comp = search(target[:, :3], solid[:, :3])
    return dict(q=q, out=out, target=target, group=group, nn_idx=nn_idx, nn_dist=nn_dist, comp_dist=comp, radius=radius, n_groups=n_groups)


def want_cloud(c, track_mode='one'):
    return restate(c['out'], c['nn_idx'], c['nn_dist'], c['target'], radius=c['radius'], threshold=0.5, target_group=c['group'],
                   comp_dist=c['comp_dist'], n_groups=c['n_groups'], n_classes=0, out_track=4,
                   flags=FLAG_COLOR | (FLAG_TRACK if track_mode != 'none' else 0), **COLUMNS[9])


def add_cloud(stats, c, device, track_mode='one', **kw):
    dev = torch.device(device)
    return stats.add_frame(torch.from_numpy(c['q']).to(dev), torch.from_numpy(c['out']).to(dev), c['target'], density_threshold=0.5,
                           point_occupancy_radius=c['radius'], color_mode='rgb', predict_segmentation=False, track_mode=track_mode,
                           data_kind='greater', target_group=c['group'], **kw)


def check_argument_errors(device):
    """The contract of the query statistics, as the library on `device` states it (csrc/eval_math.hpp: one source for both
    libraries)."""
    z = lambda *shape, **kw: torch.zeros(*shape, device=device, **kw)
    counts, sums = z(17, dtype=torch.int64), z(8, dtype=torch.float64)
    out, idx, dist, tgt = z(8, 5)[2:6], z(4, dtype=torch.int32), z(4), z(3, 9)      # (out: four rows with two rows of slack each side)
    with pytest.raises(AssertionError, match='col_rgb'):
        pk.ops.eval_query_stats(out, idx, dist, tgt, counts, sums, flags=FLAG_COLOR, col_rgb=7)
    with pytest.raises(AssertionError, match='out_track'):
        pk.ops.eval_query_stats(out, idx, dist, tgt, counts, sums, flags=FLAG_TRACK, col_track=8, out_track=5)
    with pytest.raises(AssertionError, match='n_classes'):
        pk.ops.eval_query_stats(out, idx, dist, z(3, 11), z(1 + 16 + 169, dtype=torch.int64), sums,
                                flags=FLAG_SEG, col_sem=5, n_classes=13)
    with pytest.raises(AssertionError):
        pk.ops.eval_query_stats(out, idx, dist, tgt, counts[:16], sums)
    with pytest.raises(AssertionError):
        pk.evaluation.EvalStats(9, 0, device)
    assert not counts.any() and not sums.any()
