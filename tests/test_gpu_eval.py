"""The evaluation statistics on the HIP kernels (csrc/evalstats.hip): the kernel-level matrix of tests/eval_cases.py against the
numpy restatement (counts equal, sums within 1e-9 relative), bit-reproducibility of the sums, EvalStats.add_frame end to end and
the `stats` keywords of perform_inference / evaluate_clip.  tests/test_eval_host.py runs the same matrix through the g++ twin."""
import types

import numpy as np
import pytest
import torch

import eval_cases as ec
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('name,args', ec.matrix(), ids=[c[0] for c in ec.matrix()])
def test_matrix_against_the_restatement(name, args):
    """N = 262 401 = 1024 workgroups x 256 rows + 257: the grid is capped at 1024 workgroups (GRID_CAP), so 257 rows are reached
    only by a second trip of the grid-stride loop."""
    ec.check_case(args, DEV)


@pytest.mark.parametrize('name,args', ec.SPECIALS + [('bad', ec.BAD_CASE)], ids=[c[0] for c in ec.SPECIALS] + ['bad'])
def test_special_cases(name, args):
    case, got, want = ec.check_case(args, DEV)
    if name == 'bad':
        s = pk.evaluation.EvalStats.from_state(dict(n_groups=3, semantic_classes=13, counts=got[0], sums=got[1]), DEV)
        with pytest.raises(ValueError, match=str(int(got[0][ec.BAD_ROWS]))):
            s.summary()


def test_argument_errors():
    ec.check_argument_errors(DEV)


@pytest.mark.parametrize('idx', [42, 44])                # N = 262 401 (two trips, 1024 partials) with 8 and 3 groups
def test_two_identical_calls_give_bit_identical_sums(idx):
    case = ec.make_case(*ec.matrix()[idx][1])
    assert case['out'].shape[0] > ec.GRID_CAP_ROWS
    a, b = ec.run_case(case, DEV), ec.run_case(case, DEV)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[1].any()


@pytest.fixture(scope='module')
def cloud():
    return ec.cloud_case()


def test_add_frame_end_to_end(cloud):
    """Seeded clouds (N = 4099 queries, M = 1000 target points, unit cube) whose decisions an fp32 search cannot change: counts
    equal, sums within 1e-5 relative (the kernel's fp32 distance is within a few ulp, 4e-7, of the float64 one)."""
    s = ec.add_cloud(pk.evaluation.EvalStats(3, 0, DEV), cloud, DEV)
    assert s.counts.is_cuda and s.sums.is_cuda
    st = s.state()
    ec.same_stats((st['counts'], st['sums']), ec.want_cloud(cloud), rel=1e-5)
    assert st['counts'][ec.BAD_ROWS] == 0
    summary = s.summary()
    want = ec.closed_forms(st['counts'], st['sums'], 3, 0)
    for g in range(3):
        assert summary['iou'][g] == want[g]['iou'] and summary['chamfer'][g] == want[g]['chamfer'] and np.isnan(summary['seg_miou'][g])
    twice = ec.add_cloud(ec.add_cloud(pk.evaluation.EvalStats(3, 0, DEV), cloud, DEV), cloud, DEV).state()
    assert np.array_equal(twice['counts'], 2 * st['counts']) and np.array_equal(twice['sums'], 2 * st['sums'])


def _nets(seed=31):
    pa, ia, inf = pk.configs.model_args('greater', 768)
    esd, dsd = pk.configs.synthetic_weights(pa, ia, seed=seed)
    enc = pk.model.PointCompletionNetV3(**pa).to(DEV).eval()
    dec = pk.implicit.LocalPclResnetFC(**ia).to(DEV).eval()
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    return inf, enc, dec


def _target(rng, m, lo=-5.0, hi=5.0):
    t = rng.uniform(0, 1, size=(m, 9)).astype(np.float32)
    t[:, :3] = rng.uniform(lo, hi, size=(m, 3))
    t[:, 4] = rng.integers(0, 3, size=m)                         # view_idx
    t[:, 8] = rng.integers(0, 2, size=m)
    return t


def test_perform_inference_with_stats():
    """perform_inference(..., stats=s) on the smoke-size networks: s equals the restatement evaluated on the arrays the same call
    returns (implicit_output, and the label / nearest target row of every query in gt_solid / gt_air); every other key is
    bit-identical to a call without `stats`."""
    inf, enc, dec = _nets()
    pcl = pk.configs.synthetic_pcl('greater', 768, 4, seed=32)
    target = _target(np.random.default_rng(33), 300)
    kw = dict(num_sample=1024, point_sample_mode='grid', batch_size=512, predict_segmentation=False, track_mode='one',
              semantic_classes=13, density_threshold=0.5, data_kind='greater', cube_mode=4, compress_air=False,
              point_occupancy_radius=1.0)

    def run(**extra):
        return pk.inference.perform_inference(pcl.clone(), None, target, [enc, dec], DEV, 'if', inf['min_z'], inf['cube_bounds'],
                                              inf['color_mode'], 1, None, **kw, **extra)
    s = pk.evaluation.EvalStats(1, 0, DEV)
    plain, scored = run(), run(stats=s)
    assert sorted(plain) == sorted(scored)
    for k in plain:
        assert plain[k].dtype == scored[k].dtype and np.array_equal(plain[k], scored[k]), k
    out = scored['implicit_output']
    solid = out[:, 0] >= np.float32(0.5)
    nngt = np.empty((out.shape[0], 1 + 9), scored['gt_solid'].dtype)
    nngt[solid], nngt[~solid] = scored['gt_solid'], scored['gt_air']
    assert 0 < solid.sum() < out.shape[0] and 0 < nngt[:, 0].sum() < out.shape[0]      # (the inputs put rows on both sides of both)
    want = ec.restate_rows(out, nngt[:, 0] > 0, nngt[:, 1:].astype(np.float32), np.zeros(out.shape[0], np.int64), None, n_groups=1,
                           n_classes=0, threshold=0.5, flags=ec.FLAG_COLOR | ec.FLAG_TRACK, out_track=4, comp_dist=np.zeros(300),
                           comp_group=np.zeros(300, np.int64), **ec.COLUMNS[9])
    st = s.state()
    assert np.array_equal(st['counts'], want[0])
    per = st['sums'].reshape(1, 8)[0]
    assert abs(per[ec.SUM_COLOR] - want[1][ec.SUM_COLOR]) <= 1e-9 * want[1][ec.SUM_COLOR] and per[ec.SUM_ACC_D] > 0 and per[ec.SUM_COMP_D] > 0
    # without the gt branch: the target comes through stats_target, the result has no gt keys
    s2 = pk.evaluation.EvalStats(1, 0, DEV)
    res = pk.inference.perform_inference(pcl.clone(), None, None, [enc, dec], DEV, 'if', inf['min_z'], inf['cube_bounds'],
                                         inf['color_mode'], 1, None, **kw, stats=s2, stats_target=target)
    assert 'gt_solid' not in res and torch.equal(s2.counts, s.counts) and torch.equal(s2.sums, s.sums)


def test_evaluate_clip_with_stats_is_the_merge_of_its_frames():
    inf, enc, dec = _nets(seed=41)
    rng = np.random.default_rng(42)
    pcl = pk.configs.synthetic_pcl('greater', 768, 4, 43)
    frames = [_target(rng, 300), _target(rng, 257)]
    batch = dict(pcl_input=pcl, pcl_input_sem=torch.zeros((1, 768, 1)), pcl_target=[torch.from_numpy(f)[None] for f in frames],
                 meta_data=dict(pcl_target_size=[torch.tensor([300]), torch.tensor([200])]))
    args = types.SimpleNamespace(min_z=inf['min_z'], cr_cube_bounds=inf['cube_bounds'], color_mode=inf['color_mode'],
                                 sample_implicit=True, num_sample=1024, point_sample_mode='grid', implicit_batch_size=512,
                                 segmentation_lw=0.0, track_mode='none', point_occupancy_radius=1.0, semantic_classes=13,
                                 density_threshold=0.5, cube_mode=4)

    def group_fn(rows):
        return (rows[:, 4] != 0).astype(np.int32)
    plain = pk.evaluation.evaluate_clip(batch, [enc, dec], DEV, args, 'greater')
    clip = pk.evaluation.EvalStats(2, 0, DEV)
    scored = pk.evaluation.evaluate_clip(batch, [enc, dec], DEV, args, 'greater', stats=clip, stats_group_fn=group_fn)
    assert all(np.array_equal(x, y) for a, b in zip(plain, scored) for x, y in zip(a, b))
    merged = pk.evaluation.EvalStats(2, 0, DEV)
    for t, (frame, size) in enumerate(zip(frames, (300, 200))):
        one = pk.evaluation.EvalStats(2, 0, DEV)
        pk.inference.perform_inference(pcl.clone(), None, None, [enc, dec], DEV, 'if', args.min_z, args.cr_cube_bounds, args.color_mode,
                                       t, None, num_sample=1024, point_sample_mode='grid', batch_size=512, track_mode='none',
                                       point_occupancy_radius=1.0, density_threshold=0.5, data_kind='greater', cube_mode=4,
                                       compress_air=True, stats=one, stats_target=frame[:size], stats_group=group_fn(frame[:size]))
        assert one.state()['counts'][ec.HEAD:].sum() > 0
        merged += one
    assert torch.equal(clip.counts, merged.counts) and torch.equal(clip.sums, merged.sums)
    per = clip.state()['counts'][ec.HEAD:].reshape(2, 16)
    assert per[:, :4].sum() == sum(item[2].shape[0] + item[4].shape[0] for item in plain) and per.min(axis=1)[0] >= 0 and per[:, :4].sum(axis=1).all()
