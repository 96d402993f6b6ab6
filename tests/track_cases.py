"""Shared by tests/test_track_host.py (through the g++ twin) and tests/test_gpu_track.py (on the device): the numpy restatement of
the reference's multi_track_merge (utils/utils.py:343-397) in the streaming form of include/occ4d_track.h, the case matrix of
the two merge entry points, and the end-to-end comparisons of perform_inference(track_merge='device') with 'host'.
Everything is compared EQUAL: the non-NaN elements bit for bit (so -0 is not +0), the NaN positions as positions."""
import types

import numpy as np
import pytest
import torch

import gen_track_fixture as gen
import golden_cases as gc
import occlusions4d_amd as pk
from conftest import load_golden

ROW_COUNTS = [0, 1, 255, 256, 257, 1025, 262401]      # (262401 rows: more than one trip of the grid-stride loop)
WIDTHS = [1, 5, 6, 16, 29, 32]
RUN_COUNTS = [1, 2, 3, 5, 6, 7]
PAD = 3                                               # a strided view has ld = g + PAD
SENTINEL = 777.0
# the large row count is there for the grid-stride trips, which depend on the element count alone (a workgroup loop covers
# 1024 * 256 items per trip): width 1 (a flat (n, 1) view, as the abstract cloud's is) makes two trips of the one-element
# loop, width 5 two trips of the four-element flat loop (328 001 items) and six of the one-element loop.  Two widths and two
# run counts keep it to seconds; every smaller row count takes the full cross
LARGE_WIDTHS, LARGE_RUN_COUNTS = [1, 5], [2, 7]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


def same_values(a, b):
    """np.array_equal with the NaN positions compared separately: the comparison with the REFERENCE's arrays.  numpy's mean
    starts its sum from +0, so where every rerun holds -0 the reference has +0 and the streaming form (acc = run_0) -0: equal
    values, different bits.  same_bits() is for everything that is compared with the streaming form itself."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan]))


def restate(ids, runs, track_col):
    """multi_track_merge on the list `runs` of (..., G) float32 arrays (already squashed), streaming: -> merged."""
    acc = np.array(runs[0], dtype=np.float32, copy=True)
    for r in runs[1:]:
        acc += r
    merged = acc / np.float32(len(runs))
    assert merged.dtype == np.float32
    if track_col >= 0:
        winner = np.full(acc.shape[:-1], -1.0, dtype=np.float32)
        best = np.zeros(acc.shape[:-1], dtype=np.float32)
        with np.errstate(invalid='ignore'):
            for inst_id, r in zip(ids, runs):
                score = r[..., track_col]
                winner[np.logical_and(score >= 0.5, score >= best)] = inst_id      # (a tie goes to the later rerun)
                best = np.maximum(score, best)                                      # (NaN-propagating)
        merged[..., track_col] = winner
    return merged


def track_columns(g):
    return [-1, 0] if g == 1 else sorted({-1, min(4, g - 1), g - 1})


def mixed_codes(g, shift):
    return [1] if g == 1 else [(c + shift) % 3 for c in range(g)]


def raw_runs(n, g, k_max, rng):
    """k_max reruns (k_max, n, g) of RAW outputs spanning +-100: the sigmoid saturates to 0, to subnormals and to 1."""
    raw = rng.uniform(-100.0, 100.0, size=(k_max, n, g)).astype(np.float32)
    near = rng.uniform(size=raw.shape) < 0.4
    raw[near] = rng.uniform(-3.0, 3.0, size=int(near.sum())).astype(np.float32)
    zero = rng.uniform(size=raw.shape) < 0.05                        # (sigmoid(+-0) is exactly 0.5)
    raw[zero] = np.where(rng.uniform(size=int(zero.sum())) < 0.5, 0.0, -0.0).astype(np.float32)
    tiny = rng.uniform(size=raw.shape) < 0.02                        # (subnormal raw values)
    raw[tiny] = np.where(rng.uniform(size=int(tiny.sum())) < 0.5, 1e-40, -1.4e-45).astype(np.float32)
    return raw


def place(array, strided, offset, device, fill=None):
    """`array` (n, g) as a device tensor: a contiguous tensor or columns 0 .. g - 1 of an (n, g + PAD) one, its base 16-byte
    aligned or one float behind that.  fill: the value of every element (padding included) instead of the array's."""
    n, g = array.shape
    ld = g + PAD if strided else g
    buf = torch.full((n * ld + 4,), SENTINEL, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    rows = buf[offset:offset + n * ld].view(n, ld)
    view = rows[:, :g]
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(array)))
    else:
        rows.fill_(fill)
    return buf, rows, view


def merge_on(device, ids, views, track_col, codes, strided=False, offset=0):
    """The running merge of the (n, g) tensors `views` -> (buffer, rows with padding, acc view); the accumulator, best and
    winner start from garbage."""
    n, g = views[0].shape
    buf, rows, acc = place(np.empty((n, g), np.float32), strided, offset, device, fill=float('nan'))
    if strided:
        rows[:, g:] = SENTINEL
    best = torch.full((n,), float('nan'), device=device)
    winner = torch.full((n,), 12345.0, device=device)
    for k, (inst_id, v) in enumerate(zip(ids, views)):
        assert pk.ops.track_merge_add(v, acc, best if track_col >= 0 else None, winner if track_col >= 0 else None, inst_id,
                                      track_col, codes, first=(k == 0)) is acc
    pk.ops.track_merge_finish(acc, winner if track_col >= 0 else None, len(views), track_col)
    return buf, rows, acc


def check_combo(device, raw, ids, track_col, codes, strided, offset):
    """One cell of the matrix; raw (K, n, g).  Returns nothing, asserts."""
    K, n, g = raw.shape
    tag = (n, g, K, track_col, codes, strided, offset)
    placed = [place(raw[k], strided, offset, device) for k in range(K)]
    views = [p[2] for p in placed]
    before = [p[0].clone() for p in placed]
    if codes is None:
        squashed = [raw[k] for k in range(K)]
    else:                                             # the library's own squash on a copy, then the identity-code merge
        squashed = [pk.ops.squash(v.clone(), codes).cpu().numpy() for v in views]
    want = restate(ids, squashed, track_col)
    buf, rows, acc = merge_on(device, ids, views, track_col, codes, strided, offset)
    assert same_bits(acc.cpu().numpy(), want), tag
    for p, b in zip(placed, before):                                 # `out` is read only
        assert torch.equal(p[0].view(torch.int32), b.view(torch.int32)), tag
    tail = buf.cpu().numpy()
    assert (tail[:offset] == SENTINEL).all() and (tail[offset + rows.numel():] == SENTINEL).all(), tag
    if strided and n:
        assert bool((rows[:, g:] == SENTINEL).all()), tag               # the padding columns keep their sentinel
    if codes is not None and n:                       # ... and that two-step merge through the library as well
        _, _, two_step = merge_on(device, ids, [torch.from_numpy(s).to(device) for s in squashed], track_col, None)
        assert same_bits(two_step.cpu().numpy(), want), tag


def check_matrix(n, device):
    """Every cell of the matrix at `n` rows; returns the number of cells."""
    rng = np.random.default_rng(1000 + n)
    large = n > 100000
    cells = 0
    for g in (LARGE_WIDTHS if large else WIDTHS):
        raw = raw_runs(n, g, max(RUN_COUNTS), rng)
        scores = gen.SCORE_POOL[rng.integers(0, len(gen.SCORE_POOL), size=raw.shape[:2])]
        for K in (LARGE_RUN_COUNTS if large else RUN_COUNTS):
            ids = [int(i) for i in rng.permutation(4096)[:K]]
            for track_col in track_columns(g):
                for codes in (None, mixed_codes(g, K + max(track_col, 0))):
                    runs = raw[:K]
                    if codes is None and track_col >= 0:             # identity: the adversarial scores themselves (NaN included)
                        runs = runs.copy()
                        runs[:, :, track_col] = scores[:K]
                    for strided in (False, True):
                        for offset in (0, 1):
                            check_combo(device, runs, ids, track_col, codes, strided, offset)
                            cells += 1
    return cells


def cells_of(n):
    large = n > 100000
    return sum(len(track_columns(g)) for g in (LARGE_WIDTHS if large else WIDTHS)) * len(LARGE_RUN_COUNTS if large else RUN_COUNTS) * 8


def check_golden(name, device):
    """The reference's own result of one fixture: through the restatement, and through the library."""
    z = load_golden(name)
    ids, track_col = [int(i) for i in z['ids']], int(z['track_col'])
    K = len(ids)
    want = dict(output=restate(ids, list(z['outputs']), track_col), abstract=restate(ids, list(z['abstract']), -1),
                features=restate(ids, list(z['features']), -1))
    for key in want:                                                   # restatement and reference are tied together
        assert same_values(want[key], z['merged_' + key]), key
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    _, _, out = merge_on(device, ids, [dev(z['outputs'][k]) for k in range(K)], track_col, None)
    assert same_values(out.cpu().numpy(), z['merged_output']) and same_bits(out.cpu().numpy(), want['output'])
    for key in ('abstract', 'features'):                               # as inference does: flat (n, 1) views, no track column
        _, _, flat = merge_on(device, ids, [dev(z[key][k]).view(-1, 1) for k in range(K)], -1, None)
        got = flat.cpu().numpy().reshape(z['merged_' + key].shape)
        assert same_values(got, z['merged_' + key]) and same_bits(got, want[key])


# ---------------------------------------------------------------------------------------------------------------- end to end
CASE = gc.TRACK_CASES[0]              # 768 points, 1500 queries, three tracked ids, one id below the minimum


def nets(device):
    pcl, sem, target, pa, ia, inf, esd, dsd = gc.track_inputs(CASE)
    enc = pk.model.PointCompletionNetV3(**pa).to(device).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(device).eval()
    dec.load_state_dict(dsd)
    return pcl, sem, target, inf, enc, dec


def infer(device, inputs, **kw):
    pcl, sem, target, inf, enc, dec = inputs
    return pk.inference.perform_inference(
        pcl.clone(), sem.copy(), target.copy(), [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'],
        CASE['time_idx'], None, sample_implicit=True, num_sample=CASE['num_sample'], point_sample_mode='grid',
        batch_size=CASE['batch_size'], predict_segmentation=False, track_mode='all', semantic_classes=13, density_threshold=0.5,
        data_kind='greater', cube_mode=4, compress_air=True, point_occupancy_radius=0.8, **kw)


def same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        if a[k].dtype == np.float32:
            assert same_bits(a[k], b[k]), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def check_modes_agree(device, monkeypatch):
    """'device' equals 'host' on every entry of the result dict (gt_solid / gt_air included) and in the EvalStats; the device
    mode blocks on the host ONCE and never calls multi_track_merge, the host mode blocks twice and calls it."""
    inputs = nets(device)
    calls = dict(wait=0, merge=0)
    wait, merge = pk.inference._HostCopies.wait, pk.inference.multi_track_merge

    def counted_wait(self):
        calls['wait'] += 1
        return wait(self)

    def counted_merge(*a, **k):
        calls['merge'] += 1
        return merge(*a, **k)
    monkeypatch.setattr(pk.inference._HostCopies, 'wait', counted_wait)
    monkeypatch.setattr(pk.inference, 'multi_track_merge', counted_merge)
    stats = {m: pk.evaluation.EvalStats(1, 0, device) for m in ('device', 'host')}
    res = {}
    for mode, want in (('device', dict(wait=1, merge=0)), ('host', dict(wait=3, merge=1))):
        res[mode] = infer(device, inputs, track_merge=mode, stats=stats[mode])
        assert calls == want, (mode, calls)
    assert {'gt_solid', 'gt_air', 'implicit_output', 'pcl_abstract', 'features_global'} <= set(res['host'])
    same_result(res['device'], res['host'])
    ids = np.unique(res['host']['implicit_output'][:, 4])
    assert set(ids) <= {-1.0, 0.0, 1.0, 2.0} and len(ids) >= 2           # (the id with 5 points is never followed)
    a, b = stats['device'].state(), stats['host'].state()
    assert a['counts'].sum() > 0 and np.array_equal(a['counts'], b['counts']) and np.array_equal(a['sums'], b['sums'])
    return res


def check_clip_reuses_the_encodes(device, monkeypatch):
    """evaluate_clip over two frames in 'all' mode: one encode per tracked instance with reuse_encode (K, not 2 K), same arrays."""
    pcl, sem, target, inf, enc, dec = nets(device)
    frames = [target, target[:257] * np.float32(0.5)]
    batch = dict(pcl_input=pcl, pcl_input_sem=torch.from_numpy(sem)[None], pcl_target=[torch.from_numpy(f)[None] for f in frames],
                 meta_data=dict(pcl_target_size=[torch.tensor([f.shape[0]]) for f in frames]))
    args = types.SimpleNamespace(min_z=inf['min_z'], cr_cube_bounds=inf['cube_bounds'], color_mode=inf['color_mode'],
                                 sample_implicit=True, num_sample=CASE['num_sample'], point_sample_mode='grid',
                                 implicit_batch_size=CASE['batch_size'], segmentation_lw=0.0, track_mode='all',
                                 point_occupancy_radius=0.8, semantic_classes=13, density_threshold=0.5, cube_mode=4)
    encodes = []
    forward = type(enc).forward

    def counted(self, *a, **k):
        encodes.append(1)
        return forward(self, *a, **k)
    monkeypatch.setattr(type(enc), 'forward', counted)
    K = 3
    shared = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, reuse_encode=True)
    assert len(encodes) == K
    separate = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, reuse_encode=False)
    assert len(encodes) == K + 2 * K
    assert len(shared) == len(separate) == 2
    for a, b in zip(shared, separate):
        assert len(a) == len(b) == 7
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
    assert not np.array_equal(shared[0][2], shared[1][2])               # (two different output frames)


def check_argument_errors(device):
    """The contract of the two entry points, as the library on `device` states it (csrc/track_math.hpp: one source for both
    libraries).  Every non-null pointer is a real tensor that covers the call even if it were accepted."""
    z = lambda *shape: torch.zeros(*shape, device=device)
    o, acc, col = z(10, 5), z(10, 5), z(10)
    add, fin = pk.ops.track_merge_add, pk.ops.track_merge_finish
    with pytest.raises(AssertionError, match='track_col'):
        add(o, acc, col, col.clone(), 1, 5)
    with pytest.raises(AssertionError, match='track_col'):
        add(o, acc, col, col.clone(), 1, -2)
    with pytest.raises(AssertionError, match='op code'):
        add(o, acc, col, col.clone(), 1, 4, [0, 1, 2, 3, 0])
    with pytest.raises(AssertionError, match='op code'):
        add(o, acc, col, col.clone(), 1, 4, [0, 1, -1, 0, 0])
    with pytest.raises(AssertionError, match='null best / winner'):
        add(o, acc, None, None, 1, 4)
    with pytest.raises(AssertionError, match='null best / winner'):
        add(o, acc, col, None, 1, 4)
    with pytest.raises(AssertionError, match='g = 33'):
        add(z(4, 33), z(4, 33), None, None, 1, -1)
    with pytest.raises(AssertionError, match='inst_id'):
        add(o, acc, col, col.clone(), 2.5, 4)
    with pytest.raises(AssertionError, match='inst_id'):
        add(o, acc, col, col.clone(), 2 ** 24 + 1, 4)
    with pytest.raises(AssertionError, match='acc must be'):
        add(o, z(10, 6), col, col.clone(), 1, 4)
    with pytest.raises(AssertionError, match='n_runs'):
        fin(acc, col, 0, 4)
    with pytest.raises(AssertionError, match='track_col'):
        fin(acc, col, 2, 5)
    with pytest.raises(AssertionError, match='null winner'):
        fin(acc, None, 2, 4)
    with pytest.raises(AssertionError, match='g = 33'):
        fin(z(4, 33), None, 2, -1)
    L, p = pk._lib.lib(), pk.ops._ptr                                 # what no tensor can express: short strides, null arrays
    assert L.occ4d_track_merge_add_f32(p(o), 4, 10, 5, None, -1, 1.0, 1, p(acc), 5, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_add_f32(p(o), 5, 10, 5, None, -1, 1.0, 1, p(acc), 4, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_add_f32(None, 5, 10, 5, None, -1, 1.0, 1, p(acc), 5, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_add_f32(p(o), 5, 10, 5, None, -1, 1.0, 1, None, 5, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_add_f32(p(o), 5, 10, 5, None, -1, 1.0, 2, p(acc), 5, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_add_f32(p(o), 5, -1, 5, None, -1, 1.0, 1, p(acc), 5, None, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_finish_f32(p(acc), 4, 10, 5, 2, -1, None, None) == pk._lib.EINVAL
    assert L.occ4d_track_merge_finish_f32(None, 5, 10, 5, 2, -1, None, None) == pk._lib.EINVAL
    assert b'occ4d_track_merge_finish_f32' in L.occ4d_last_error()
    assert L.occ4d_track_merge_add_f32(None, 5, 0, 5, None, 4, 1.0, 1, None, 5, None, None, None) == pk._lib.OK      # n = 0
    assert L.occ4d_track_merge_finish_f32(None, 5, 0, 5, 1, 4, None, None) == pk._lib.OK
    assert float(acc.abs().sum()) == 0.0 and float(o.abs().sum()) == 0.0
