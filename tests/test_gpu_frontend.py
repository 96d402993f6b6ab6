"""The clip front end on the HIP path (csrc/frontend.hip): the reference's fixtures bit for bit (the kernels and the g++
twin of tests/test_frontend_host.py share their per-element source), synthetic clips at working sizes against a torch count
and an fp64 evaluation, and frames -> greater_clip -> perform_inference without a host round trip."""
import numpy as np
import pytest
import torch

import frontend_cases as fc
import gen_frontend_fixture as gen
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def test_greater_every_stage_bit_for_bit():
    fc.check_greater_stages(DEV)


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_greater_clip_bit_for_bit(name):
    got, g, _ = fc.run_greater(name, DEV)
    assert got[0].is_cuda and got[1].is_cuda and all(f.is_cuda for f in got[2])
    fc.check_tail(got, g, 'greater ' + name)


@pytest.mark.parametrize('mode,ref_frame', gen.CARLA_STAGE_CASES)
def test_carla_transform_and_filter_bit_for_bit(mode, ref_frame):
    fc.check_carla_stages(DEV, mode, ref_frame)


@pytest.mark.parametrize('name', [c[0] for c in gen.CARLA_CASES])
def test_carla_clip_bit_for_bit(name):
    got, g = fc.run_carla(name, DEV)
    assert got[0].is_cuda
    fc.check_tail(got, g, 'carla ' + name)


def _chain64(a, cols):
    """The kernel's fused chain emulated through float64: the product of two float32 is exact in float64, the sum is rounded
    to float64 and then to float32 -- a double rounding that differs from the fused result rarely, and then by 1 ulp."""
    acc = (a[0].astype(np.float64) * cols[0].astype(np.float64)).astype(np.float32)
    for k in (1, 2, 3):
        acc = (a[k].astype(np.float64) * cols[k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_error_conventions():
    fc.check_argument_errors(DEV)


@pytest.mark.parametrize('T,H,W', [(12, 240, 320), (3, 37, 53)])
def test_synthetic_clip_counts_order_and_coordinates(T, H, W):
    rng = np.random.default_rng(H * W)
    depth = rng.uniform(2.0, 14.0, size=(T, H, W)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
    rgb = rng.uniform(size=(T, H, W, 3)).astype(np.float32)
    cam_RT = np.stack([gen._look_at([7.0 * np.cos(0.1 * t), 7.0 * np.sin(0.1 * t), 3.5], [0.0, 0.0, 0.5]) for t in range(T)])
    cam_K = np.zeros((T, 3, 3), dtype=np.float32)
    cam_K[:, 0, 0] = cam_K[:, 1, 1] = 1.1 * W
    cam_K[:, 0, 2], cam_K[:, 1, 2], cam_K[:, 2, 2] = W / 2.0, H / 2.0, 1.0
    k_inv, rt_inv = pk.frontend.inverse_4x4(cam_K), pk.frontend.inverse_4x4(cam_RT)
    bounds = (-5.0, 5.0, -5.0, 5.0, -1.0, 5.0)
    d_dev = torch.from_numpy(depth).to(DEV)
    rows, _, key = pk.frontend.rgbd_rows(d_dev, torch.from_numpy(rgb).to(DEV), None, torch.from_numpy(k_inv).to(DEV),
                                         torch.from_numpy(rt_inv).to(DEV), None, bounds, floor_fix=True)
    # the row count = a torch-on-device count of depth > 0 and the filter on the kernel's own coordinates
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    keep = (d_dev.reshape(-1) > 0) & (x >= -5) & (x <= 5) & (y >= -5) & (y <= 5) & (z >= -1) & (z <= 5) & \
        (z > (torch.maximum(x.abs(), y.abs()) - 4.5) / 3.5)
    assert torch.equal(keep, key > 0.5)
    kept, _ = pk.ops.compact_rows(rows, key, 0.5, strict=True)
    assert kept.shape[0] == int(keep.sum().item()) and 0 < kept.shape[0] < int((d_dev > 0).sum().item())
    assert torch.equal(kept, rows[keep])                                   # pixel order: frame-major, row-major
    assert bool((rows[:, 3] == -1).all()) and torch.equal(rows[:, 4:7], torch.from_numpy(rgb).to(DEV).reshape(-1, 3))
    assert torch.equal(rows[:, 7], torch.arange(T, device=DEV).repeat_interleave(H * W).float())
    # coordinates: the fp32 fused chain evaluated through float64, within 1 ulp
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    got = rows[:, :3].cpu().numpy().reshape(T, H * W, 3)
    worst = 0
    for t in range(T):
        one = np.ones(H * W, dtype=np.float32)
        src = [_chain64(k_inv[t, i], [px.reshape(-1), py.reshape(-1), one, one]) for i in range(4)]
        zt = depth[t].reshape(-1)
        src = [src[0] * zt, src[1] * zt, src[2] * zt, src[3]]
        for i in range(3):
            worst = max(worst, int(_ulps(_chain64(rt_inv[t, i], src), got[t][:, i]).max()))
    print('max ulp distance to the float64 evaluation: %d' % worst)
    assert worst <= 1


def test_frames_to_inference_without_a_host_round_trip():
    """frames -> greater_clip -> perform_inference on the config-1 networks = perform_inference on the fixture's host-built
    cloud, bit for bit."""
    n = 1024
    pa, ia, inf = pk.configs.model_args('greater', n)
    esd, dsd = pk.configs.synthetic_weights(pa, ia, seed=1830)
    enc = pk.model.PointCompletionNetV3(**pa).cuda().eval()
    dec = pk.implicit.LocalPclResnetFC(**ia).cuda().eval()
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    kw = dict(num_sample=4096, point_sample_mode='grid', batch_size=2048, predict_segmentation=False, track_mode='none',
              semantic_classes=13, density_threshold=0.5, data_kind='greater', cube_mode=4, compress_air=True)

    def infer(pcl):
        return pk.inference.perform_inference(pcl, None, None, [enc, dec], DEV, 'if', inf['min_z'], inf['cube_bounds'],
                                              inf['color_mode'], 1, None, **kw)
    (pcl_input, _, _, _), g, _ = fc.run_greater('a', DEV)
    assert pcl_input.is_cuda and tuple(pcl_input.shape) == (n, 8)
    got = infer(pcl_input[None])
    want = infer(torch.from_numpy(g['pcl_input'])[None])
    assert np.array_equal(got['implicit_output'], want['implicit_output'])
    assert np.array_equal(got['pcl_abstract'], want['pcl_abstract'])
