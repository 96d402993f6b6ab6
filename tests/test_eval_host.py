"""The evaluation statistics (include/occ4d_eval.h, occlusions4d_amd.evaluation.EvalStats) through the g++ twin, without a GPU:
the binding, the kernel-level case matrix against the numpy restatement of tests/eval_cases.py (counts equal, sums within
1e-9 relative: every term is exact in double and non-negative, so only the order of at most 2^20 additions differs, bounded by
n 2^-53 = 1.2e-10) and the EvalStats arithmetic.  The twin and the HIP kernels share the per-row source (csrc/eval_math.hpp);
tests/test_gpu_eval.py runs the same matrix on the device."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import eval_cases as ec
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_eval_signatures_match_the_header():
    lib = pk._lib
    with open(lib.EVAL_HEADER_PATH) as f:
        text = f.read()
    assert lib.EVAL_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.EVAL_SIGNATURES) == ['occ4d_eval_counts_len', 'occ4d_eval_query_stats_f32', 'occ4d_eval_sums_len',
                                           'occ4d_eval_target_stats_f32', 'occ4d_eval_workspace_bytes']
    assert not any(n in lib.SIGNATURES or n in lib.FRONTEND_SIGNATURES for n in lib.EVAL_SIGNATURES)
    assert not any(n in lib.SIGNATURES for n in lib.FRONTEND_SIGNATURES)
    res, args = lib.EVAL_SIGNATURES['occ4d_eval_query_stats_f32']
    assert res is ctypes.c_int and len(args) == 24 and args[1] is ctypes.c_int64 and args[17] is ctypes.c_float
    assert lib.EVAL_SIGNATURES['occ4d_eval_counts_len'][0] is ctypes.c_int64


def test_layout_constants_are_the_restatement_s():
    c = pk._lib.EVAL_CONSTANTS
    for name in ('HEAD', 'BAD_ROWS', 'GROUP_COUNTS', 'GROUP_SUMS', 'OCC_TP', 'OCC_FP', 'OCC_FN', 'OCC_TN', 'TRACK_TP', 'TRACK_FP',
                 'TRACK_FN', 'TRACK_TN', 'SEG_IGNORED', 'N_ACCURACY', 'N_COMPLETENESS', 'N_COLOR', 'N_SEG', 'FLAG_COLOR',
                 'FLAG_TRACK', 'FLAG_SEG'):
        assert c[name] == getattr(ec, name), name
    assert (c['SUM_ACCURACY_D'], c['SUM_ACCURACY_D2'], c['SUM_COMPLETENESS_D'], c['SUM_COMPLETENESS_D2'], c['SUM_COLOR_L1']) == \
        (ec.SUM_ACC_D, ec.SUM_ACC_D2, ec.SUM_COMP_D, ec.SUM_COMP_D2, ec.SUM_COLOR)
    assert (c['MAX_GROUPS'], c['MAX_CLASSES']) == (8, 32)
    assert pk.evaluation.TARGET_COLUMNS == {'greater': ec.COLUMNS[9], 'carla': ec.COLUMNS[11]}


def test_hip_library_exports_the_eval_symbols():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.EVAL_SIGNATURES:
        assert hasattr(handle, name), name


def test_twin_binds_the_eval_prototypes_and_sizes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.EVAL_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name
    assert pk.ops.eval_layout(1, 0) == (1 + 16, 8) and pk.ops.eval_layout(8, 32) == (1 + 8 * (16 + 1024), 64)
    assert lib.occ4d_eval_counts_len(0, 0) == -1 and lib.occ4d_eval_counts_len(9, 0) == -1 and lib.occ4d_eval_counts_len(1, 33) == -1
    assert lib.occ4d_eval_sums_len(0) == -1 and lib.occ4d_eval_workspace_bytes(-1) == -1 and lib.occ4d_eval_workspace_bytes(5) % 8 == 0


@pytest.mark.parametrize('name,args', ec.matrix(), ids=[c[0] for c in ec.matrix()])
def test_matrix_against_the_restatement(twin, name, args):
    ec.check_case(args, CPU)


@pytest.mark.parametrize('name,args', ec.SPECIALS, ids=[c[0] for c in ec.SPECIALS])
def test_special_cases(twin, name, args):
    case, got, want = ec.check_case(args, CPU)
    kw = case['kw']
    stride = ec.GROUP_COUNTS + kw['n_classes'] ** 2
    per = got[0][ec.HEAD:].reshape(kw['n_groups'], stride).sum(0)
    n = case['out'].shape[0]
    if name == 'all_solid':
        assert per[ec.OCC_FN] == per[ec.OCC_TN] == 0 and per[ec.N_ACCURACY] == n
    elif name == 'none_solid':
        assert per[ec.OCC_TP] == per[ec.OCC_FP] == per[ec.N_ACCURACY] == per[ec.N_COLOR] == 0 and not got[1].reshape(-1, 8)[:, [0, 1, 4]].any()
    elif name == 'all_label0':
        assert per[ec.OCC_TP] == per[ec.OCC_FN] == 0 and per[ec.N_COLOR] == 0
    elif name == 'tags':
        assert per[ec.OCC_TP] == n and per[ec.SEG_IGNORED] > 0 and per[ec.N_SEG] + per[ec.SEG_IGNORED] == n
        assert per[ec.GROUP_COUNTS:].sum() == per[ec.N_SEG] > 0                 # (only the one integer tag is a class)
    elif name == 'hsv':
        assert per[ec.N_COLOR] == 0 and not got[1].reshape(-1, 8)[:, ec.SUM_COLOR].any() and per[ec.TRACK_TP] > 0


def test_threshold_and_radius_are_compared_as_the_split_and_the_label_do(twin):
    """out[0] == threshold is solid (>=), nn_dist == radius is label 0 (<): two rows decide it."""
    out = torch.tensor([[0.5, 0, 0, 0, 0], [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0, 0, 0]], dtype=torch.float32)
    tgt = torch.zeros((1, 9))
    for dist, want in (([0.2, 0.2], {ec.OCC_FP: 1, ec.OCC_TN: 1}), ([float(np.nextafter(np.float32(0.2), np.float32(0)))] * 2, {ec.OCC_TP: 1, ec.OCC_FN: 1})):
        counts, sums = torch.zeros(17, dtype=torch.int64), torch.zeros(8, dtype=torch.float64)
        pk.ops.eval_query_stats(out, torch.zeros(2, dtype=torch.int32), torch.tensor(dist, dtype=torch.float32), tgt, counts, sums,
                                density_threshold=0.5, radius=0.2)
        got = {k: int(v) for k, v in enumerate(counts[1:5].tolist()) if v}
        assert got == want, (dist, got)


def test_bad_rows_are_skipped_and_summary_raises(twin):
    case, got, want = ec.check_case(ec.BAD_CASE, CPU)
    # the query with nn_idx = M, the target point with group id = n_groups, and the queries nearest to that point
    nearest = int((case['nn_idx'] == 1000 // 3).sum())
    assert nearest > 0 and got[0][ec.BAD_ROWS] == 2 + nearest
    s = pk.evaluation.EvalStats.from_state(dict(n_groups=3, semantic_classes=13, counts=got[0], sums=got[1]), CPU)
    with pytest.raises(ValueError, match=str(int(got[0][ec.BAD_ROWS]))):
        s.summary()


def test_argument_errors(twin):
    ec.check_argument_errors(CPU)


# ------------------------------------------------------------------------------------------------------------------- EvalStats
@pytest.fixture(scope='module')
def cloud():
    return ec.cloud_case()


def _stats(c, **kw):
    return ec.add_cloud(pk.evaluation.EvalStats(c['n_groups'], 0, CPU), c, CPU, **kw)


def test_add_frame_end_to_end(twin, cloud):
    """Both searches, the split and the two passes on seeded clouds whose decisions an fp32 search cannot change: counts equal, the
    distance sums within 1e-5 relative (the fp32 distance is within a few ulp, 4e-7, of the float64 one)."""
    s = _stats(cloud)
    st = s.state()
    want = ec.want_cloud(cloud)
    ec.same_stats((st['counts'], st['sums']), want, rel=1e-5)
    assert st['counts'][ec.BAD_ROWS] == 0 and st['counts'][ec.HEAD:].reshape(3, 16)[:, ec.N_COMPLETENESS].sum() == 1000
    # the caller's own search results and solid rows give the same arrays
    dev_q = torch.from_numpy(cloud['q'])
    idx, dist = pk.ops.knn(dev_q[:, :3].contiguous(), torch.from_numpy(cloud['target'][:, :3].copy()), 1, metric=1, return_dist=True)
    solid = dev_q[torch.from_numpy(cloud['out'][:, 0] >= 0.5)]
    t = _stats(cloud, nn=(idx[:, 0], dist[:, 0]), solid=solid).state()
    assert np.array_equal(t['counts'], st['counts']) and np.array_equal(t['sums'], st['sums'])
    # numpy inputs, 3-column queries
    u = pk.evaluation.EvalStats(3, 0, CPU).add_frame(cloud['q'][:, :3], cloud['out'], cloud['target'], density_threshold=0.5,
                                                     point_occupancy_radius=cloud['radius'], color_mode='rgb', predict_segmentation=False,
                                                     track_mode='one', data_kind='greater', target_group=cloud['group']).state()
    assert np.array_equal(u['counts'], st['counts']) and np.array_equal(u['sums'], st['sums'])


def test_no_solid_prediction_skips_completeness(twin, cloud):
    c = dict(cloud, out=np.minimum(cloud['out'], np.float32(0.4)))
    st = _stats(c).state()
    per = st['counts'][ec.HEAD:].reshape(3, 16)
    assert per[:, ec.N_COMPLETENESS].sum() == 0 and per[:, ec.N_ACCURACY].sum() == 0 and per[:, [ec.OCC_FN, ec.OCC_TN]].sum() == 4099
    summary = pk.evaluation.EvalStats.from_state(st, CPU).summary()
    assert np.isnan(summary['chamfer']).all() and np.isnan(summary['precision']).all() and (summary['recall'] == 0).all()


def test_same_frame_twice_doubles_and_merge_adds(twin, cloud):
    once = _stats(cloud)
    twice = _stats(cloud)
    ec.add_cloud(twice, cloud, CPU)
    a, b = once.state(), twice.state()
    assert np.array_equal(b['counts'], 2 * a['counts']) and np.array_equal(b['sums'], 2 * a['sums'])       # (x + x is exact)
    other = ec.cloud_case(seed=5, N=257, M=7, radius=0.2)
    both = _stats(cloud)
    ec.add_cloud(both, other, CPU)
    merged = _stats(cloud).merge(_stats(other))
    assert torch.equal(merged.counts, both.counts) and torch.equal(merged.sums, both.sums)       # (a call adds its own total)
    inplace = _stats(cloud)
    inplace += _stats(other)
    assert torch.equal(inplace.counts, merged.counts) and torch.equal(inplace.sums, merged.sums)
    with pytest.raises(AssertionError, match='do not add'):
        merged.merge(pk.evaluation.EvalStats(2, 0, CPU))
    with pytest.raises(AssertionError, match='do not add'):
        merged.merge(pk.evaluation.InstanceStats(3, merged.n_groups, CPU))
    with pytest.raises(AssertionError, match='do not add'):
        pk.evaluation.InstanceStats(3, merged.n_groups, CPU).merge(merged)


def test_state_round_trips(twin, cloud):
    s = _stats(cloud)
    back = pk.evaluation.EvalStats.from_state(s.state(), CPU)
    assert (back.n_groups, back.semantic_classes) == (3, 0) and torch.equal(back.counts, s.counts) and torch.equal(back.sums, s.sums)
    assert back.counts.dtype == torch.int64 and back.sums.dtype == torch.float64


def test_summary_of_an_empty_object_is_nan_with_zero_counts(twin):
    s = pk.evaluation.EvalStats(3, 13, CPU).summary()
    for k, v in s.items():
        if k == 'counts':
            assert all(a.shape == (3,) and not a.any() for a in v.values())
        elif k == 'confusion':
            assert v.shape == (3, 13, 13) and not v.any()
        elif k == 'bad_rows':
            assert v == 0
        else:
            assert v.shape == (3,) and np.isnan(v).all(), k


@pytest.mark.parametrize('name,args', [ec.matrix()[38], ec.SPECIALS[3], ec.SPECIALS[4]])
def test_summary_equals_the_closed_forms(twin, name, args):
    case = ec.make_case(*args)
    counts, sums = ec.want_case(case)
    kw = case['kw']
    got = ec.run_case(case, CPU)
    s = pk.evaluation.EvalStats.from_state(dict(n_groups=kw['n_groups'], semantic_classes=kw['n_classes'], counts=got[0], sums=got[1]), CPU)
    summary = s.summary()
    want = ec.closed_forms(counts, sums, kw['n_groups'], kw['n_classes'])
    keys = sorted(want[0])
    assert sorted(k for k in summary if k not in ('counts', 'confusion', 'bad_rows')) == keys
    for g in range(kw['n_groups']):
        for k in keys:
            a, b = summary[k][g], want[g][k]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * abs(b), (g, k, a, b)
    stride = ec.GROUP_COUNTS + kw['n_classes'] ** 2
    per = counts[ec.HEAD:].reshape(kw['n_groups'], stride)
    assert np.array_equal(summary['counts']['occ_tp'], per[:, ec.OCC_TP]) and np.array_equal(summary['confusion'].reshape(kw['n_groups'], -1), per[:, 16:])


# ------------------------------------------------------------------------------------------------------------------- all_reduce
def _reduce_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        with pk.cpu_twin.loaded():
            c = ec.cloud_case(seed=11 + rank, N=257, M=7, radius=0.2)
            s = ec.add_cloud(pk.evaluation.EvalStats(3, 0, CPU), c, CPU)
            own = s.state()
            s.all_reduce()
            ret[rank] = (own, s.state())
    finally:
        dist.destroy_process_group()


def test_all_reduce_on_two_gloo_ranks_gives_the_sum():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        out = {r: ret[r] for r in range(2)}
    counts = out[0][0]['counts'] + out[1][0]['counts']
    sums = out[0][0]['sums'] + out[1][0]['sums']
    assert counts[ec.HEAD:].sum() > 0
    for r in range(2):
        assert np.array_equal(out[r][1]['counts'], counts) and np.array_equal(out[r][1]['sums'], sums)


def test_evaluate_clip_passes_the_frames_through(monkeypatch):
    """evaluate_clip(stats=...) hands perform_inference the object, each frame (cut to its size) and its groups; without `stats` the
    call carries none of the three keywords."""
    import types
    seen = []

    def fake(pcl_input, sem, target, networks, device, mode, *a, return_encoded=False, **kw):
        seen.append({k: kw[k] for k in ('stats', 'stats_target', 'stats_group') if k in kw})
        return dict(pcl_abstract=np.zeros((2, 4), np.float32), output_solid=np.zeros((1, 9), np.float32),
                    output_air=np.zeros((1, 5), np.float32), points_query=np.zeros((2, 4), np.float32), _encoded=(None, None))
    monkeypatch.setattr(pk.inference, 'perform_inference', fake)
    args = types.SimpleNamespace(track_mode='none', min_z=-1.0, cr_cube_bounds=5.0, color_mode='rgb', sample_implicit=True,
                                 num_sample=8, point_sample_mode='grid', implicit_batch_size=8, segmentation_lw=0.0,
                                 point_occupancy_radius=0.2, semantic_classes=13, density_threshold=0.5, cube_mode=4)
    frames = [torch.arange(27, dtype=torch.float32).reshape(1, 3, 9) + t for t in range(2)]
    batch = dict(pcl_input=torch.zeros((1, 4, 8)), pcl_input_sem=torch.zeros((1, 4, 1)), pcl_target=frames,
                 meta_data=dict(pcl_target_size=[3, 2]))
    enc = torch.nn.Module()
    pk.evaluation.evaluate_clip(batch, [enc, None], 'cpu', args, 'greater')
    assert seen == [{}, {}]
    del seen[:]
    marker = object()
    pk.evaluation.evaluate_clip(batch, [enc, None], 'cpu', args, 'greater', stats=marker, stats_group_fn=lambda rows: (rows[:, 4] != 4).astype(np.int32))
    assert [s['stats'] for s in seen] == [marker, marker]
    assert np.array_equal(seen[0]['stats_target'], frames[0][0].numpy()) and np.array_equal(seen[1]['stats_target'], frames[1][0, :2].numpy())
    assert seen[0]['stats_group'].tolist() == [0, 1, 1] and seen[1]['stats_group'].tolist() == [1, 1]
