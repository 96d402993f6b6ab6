"""The instance statistics (include/occ4d_inst.h, occlusions4d_amd.evaluation.InstanceStats) through the g++ twin, without a GPU:
the binding, the kernel-level case matrix against the numpy restatement of tests/inst_cases.py (frame tables and counts equal,
sums within 1e-9 relative), the InstanceStats arithmetic, the argument contracts, occlusion_groups and a 2-rank gloo all_reduce.
The twin and the HIP kernels share the per-row and per-id source (csrc/inst_math.hpp); tests/test_gpu_inst.py runs the same checks
on the device."""
import ctypes
import os
import socket
import types

import numpy as np
import pytest
import torch

import inst_cases as ic
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_inst_signatures_match_the_header():
    lib = pk._lib
    assert lib.FEATURE_HEADERS['INST'] == 'occ4d_inst.h'
    with open(lib.INST_HEADER_PATH) as f:
        text = f.read()
    assert lib.INST_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.INST_SIGNATURES) == ['occ4d_inst_confusion_f32', 'occ4d_inst_counts_len', 'occ4d_inst_fold', 'occ4d_inst_frame_len',
                                           'occ4d_inst_points_f32', 'occ4d_inst_sums_len']
    res, args = lib.INST_SIGNATURES['occ4d_inst_confusion_f32']
    assert res is ctypes.c_int and len(args) == 15 and args[1] is ctypes.c_int64 and args[11] is ctypes.c_float
    assert lib.INST_SIGNATURES['occ4d_inst_frame_len'][0] is ctypes.c_int64


def test_layout_constants_are_the_restatement_s():
    c = pk._lib.INST_CONSTANTS
    for name in ('MAX_IDS', 'MAX_GROUPS', 'BAD_ROWS', 'FRAME_HEAD', 'POINT_WORDS', 'HEAD', 'GROUP_COUNTS', 'GROUP_SUMS', 'N_GT', 'N_PRED',
                 'N_MATCH', 'SUM_INTER', 'SUM_UNION', 'N_CENTROID', 'SUM_IOU', 'SUM_IOU_MATCHED', 'SUM_CENTROID_D', 'SUM_CENTROID_D2',
                 'SIDE_PRED', 'SIDE_GT'):
        assert c[name] == getattr(ic, name), name
    assert (c['POINT_COUNT'], c['POINT_SX'], c['POINT_SY'], c['POINT_SZ'], c['FRACTION_BITS']) == (0, 1, 2, 3, 20)
    assert pk.evaluation.INSTANCE_COLUMNS == {'greater': 3, 'carla': 4}
    assert all('col_inst' not in d for d in pk.evaluation.TARGET_COLUMNS.values())


def test_hip_library_exports_the_inst_symbols():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.INST_SIGNATURES:
        assert hasattr(handle, name), name


def test_twin_binds_the_inst_prototypes_and_sizes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.INST_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name
    assert pk.ops.inst_layout(1) == (1 + 4 + 8, 9, 4) and pk.ops.inst_layout(64, 8) == (1 + 65 * 65 + 512, 65, 32)
    assert pk.ops.inst_layout(12, 3) == (ic.frame_len(12), 25, 12)


def test_matrix_against_the_restatement(twin):
    assert ic.check_matrix(CPU) == len(ic.matrix()) >= 9 * 3 * 2 + 1


def test_rounding_ties_go_to_even(twin):
    ic.check_ties_round_to_even(CPU)


def test_threshold_and_radius_are_compared_as_the_split_and_the_label_do(twin):
    ic.check_thresholds(CPU)


def test_identical_calls_give_identical_bits(twin):
    ic.check_repeatable(CPU)


def test_a_frame_folded_twice_doubles_every_entry(twin):
    ic.check_twice_doubles(CPU)


def test_summary_and_frame_tables_of_the_hand_made_frame(twin):
    ic.check_hand_summary(CPU)


def test_merge_state_and_bad_groups(twin):
    ic.check_merge_and_state(CPU)


def test_argument_errors(twin):
    ic.check_argument_errors(CPU)


def test_add_frame_searches_and_splits_like_the_caller(twin):
    """Without nn / solid, add_frame makes the search and the split itself: the same arrays as with the caller's."""
    rng = np.random.default_rng(3)
    q = rng.uniform(0, 1, size=(777, 4)).astype(np.float32)
    out = rng.uniform(0, 1, size=(777, 5)).astype(np.float32)
    out[:, 4] = rng.integers(-1, 3, size=777)
    target = rng.uniform(0, 1, size=(100, 9)).astype(np.float32)
    target[:, 3] = rng.integers(-1, 3, size=100)
    kw = dict(density_threshold=0.5, point_occupancy_radius=0.1, color_mode='rgb', data_kind='greater')
    own = pk.evaluation.InstanceStats(3, 1, CPU).add_frame(q[:, :3], out, target, **kw)
    tq, tt = torch.from_numpy(q), torch.from_numpy(target)
    idx, dist = pk.ops.knn(tq[:, :3].contiguous(), tt[:, :3].contiguous(), 1, metric=1, return_dist=True)
    solid = pk.ops.split_solid_air(tq, torch.from_numpy(out), 0.5)[0]
    given = pk.evaluation.InstanceStats(3, 1, CPU).add_frame(tq, torch.from_numpy(out), tt, nn=(idx[:, 0], dist[:, 0]), solid=solid, **kw)
    assert torch.equal(own.frame, given.frame) and torch.equal(own.counts, given.counts) and torch.equal(own.sums, given.sums)
    frame = np.zeros(ic.frame_len(3), np.int64)
    ic.restate_confusion(frame, out[:, 0], out[:, 4], idx[:, 0].numpy(), dist[:, 0].numpy(), target[:, 3], 3, radius=0.1)
    ic.restate_points(frame, q[out[:, 0] >= 0.5, :3], out[out[:, 0] >= 0.5, 4], 3, ic.SIDE_PRED)
    ic.restate_points(frame, target[:, :3], target[:, 3], 3, ic.SIDE_GT)
    ic.same_stats((own.frame.numpy(), own.counts.numpy(), own.sums.numpy()), (frame,) + ic.restate_fold(frame, 3, None, 1))
    assert own.summary()['counts']['n_gt'][0] == 3
    # a CARLA-width target reads column 4
    wide = np.zeros((100, 11), np.float32)
    wide[:, :3], wide[:, 4] = target[:, :3], target[:, 3]
    carla = pk.evaluation.InstanceStats(3, 1, CPU).add_frame(q, out, wide, **dict(kw, data_kind='carla'))
    assert torch.equal(carla.frame, own.frame)
    with pytest.raises(AssertionError, match='no instance column'):
        pk.evaluation.InstanceStats(3, 1, CPU).add_frame(q, out, target, **dict(kw, data_kind='other'))


def test_occlusion_groups():
    live = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.9, 0.1])
    valo = np.array([3, 0, 5, 1, 7, 9, -1], np.int32)                  # (id 9 is beyond n_ids, the last entry is padding)
    g = pk.evaluation.occlusion_groups(live, valo, 6, 8)
    assert g.dtype == np.int32 and g.shape == (8,)
    assert g.tolist() == [1, 2, 3, 0, 3, 1, 3, 2]                      # ids 2, 4, 6: no valo id -> the last group, len(edges) + 1
    for i, f in zip(valo[:5], live[:5]):
        assert g[i] == np.searchsorted((0.25, 0.75), f, side='right')
    assert pk.evaluation.occlusion_groups(live, valo, 0, 3).tolist() == [3, 3, 3]
    assert pk.evaluation.occlusion_groups(live, valo, 6, 4, edges=(0.5,)).tolist() == [0, 1, 2, 0]
    with pytest.raises(AssertionError, match='ascend'):
        pk.evaluation.occlusion_groups(live, valo, 6, 8, edges=(0.75, 0.25))


# ------------------------------------------------------------------------------------------------------------------- all_reduce
def _reduce_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        with pk.cpu_twin.loaded():
            h = ic.hand_frame()
            if rank == 1:
                h = dict(h, out=ic.other_out(h))
            s = ic.add_hand(pk.evaluation.InstanceStats(3, 2, CPU), h, CPU, inst_group=np.array([0, 1, 1]))
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
    assert counts[ic.HEAD:].sum() > 0 and not np.array_equal(out[0][0]['counts'], out[1][0]['counts'])
    for r in range(2):
        assert np.array_equal(out[r][1]['counts'], counts) and np.array_equal(out[r][1]['sums'], sums)


def test_evaluate_clip_passes_the_frames_through(monkeypatch):
    """evaluate_clip(inst_stats=...) hands perform_inference the object, each frame (cut to its size) and its instance groups;
    without it the call carries none of the keywords."""
    seen = []

    def fake(pcl_input, sem, target, networks, device, mode, *a, return_encoded=False, **kw):
        seen.append({k: kw[k] for k in ('stats', 'stats_target', 'stats_group', 'inst_stats', 'inst_group') if k in kw})
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
    pk.evaluation.evaluate_clip(batch, [enc, None], 'cpu', args, 'greater', inst_stats=marker,
                                inst_group_fn=lambda t, rows: np.full(4, t + len(rows), np.int32))
    assert [sorted(s) for s in seen] == [['inst_group', 'inst_stats', 'stats_target']] * 2 and [s['inst_stats'] for s in seen] == [marker, marker]
    assert np.array_equal(seen[0]['stats_target'], frames[0][0].numpy()) and np.array_equal(seen[1]['stats_target'], frames[1][0, :2].numpy())
    assert seen[0]['inst_group'].tolist() == [3] * 4 and seen[1]['inst_group'].tolist() == [3] * 4
    del seen[:]
    pk.evaluation.evaluate_clip(batch, [enc, None], 'cpu', args, 'greater', stats=marker, inst_stats=marker)
    assert [sorted(s) for s in seen] == [['inst_group', 'inst_stats', 'stats', 'stats_group', 'stats_target']] * 2
    assert seen[0]['inst_group'] is None and seen[0]['stats_group'] is None


def test_track_mode_all_is_scored_end_to_end(twin, monkeypatch):
    ic.check_end_to_end(CPU, monkeypatch)
