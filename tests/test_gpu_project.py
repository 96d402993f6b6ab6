"""Clouds into camera views on the HIP path (csrc/project.hip): the reference's fixtures, the case matrix, the one-pixel and
foreign-key cases, the round trip with the front end and the evaluate_clip comparison of tests/test_project_host.py on the device
(the kernels and the g++ twin share their per-element source), a z-buffer that does not depend on the stream or the run, and
render_views without a device -> host copy.  Everything EQUAL.

If a z-buffer ever differs from the restatement, compare ops.project_points with project_cases.chain_restate on those rows
first: the splat repeats that projection, and the minimum itself has no order to depend on."""
import numpy as np
import pytest
import torch

import gen_project_fixture as gen
import project_cases as pc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('name', gen.NAMES)
def test_projection_equals_the_reference(name):
    pc.check_golden(name, DEV)


@pytest.mark.parametrize('n', pc.ROW_COUNTS)
def test_case_matrix(n):
    assert pc.check_matrix(n, DEV) == pc.cells_of(n)


def test_all_rows_on_one_pixel():
    assert pc.check_one_pixel(DEV)


def test_key_image_with_foreign_indices():
    pc.check_foreign_keys(DEV)


def test_round_trip_with_the_front_end():
    pc.check_roundtrip(DEV)


def test_argument_errors():
    pc.check_argument_errors(DEV)


def test_zbuffer_does_not_depend_on_the_stream_or_the_run():
    """Three streams at once and a repeated call: equal bits (the minimum of a set has no order)."""
    n, V, H, W, radius = 110000, 3, 240, 320, 1
    rows = pc.cloud(n, np.random.default_rng(23))
    rt_np, k_np = pc.cameras(V, H, W)
    dev_rows, rt, k = (torch.from_numpy(a).to(DEV) for a in (rows, rt_np, k_np))
    uvz = pk.ops.project_points(dev_rows, rt, k).cpu().numpy()
    zdepth, zindex = pc.restate_zbuffer(uvz, H, W, radius)
    want = pc.restate_resolve(zdepth, zindex, rows, n, [3, 5], 0.0, 0.0)
    assert (zindex >= 0).mean() > 0.5
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                keys = pk.ops.zbuffer_splat(dev_rows, rt, k, H, W, radius)
                outs.append((keys, pk.ops.zbuffer_resolve(keys, dev_rows, [3, 5])))
    torch.cuda.synchronize()
    for keys, images in outs:
        pc.same(keys.cpu().numpy().view(np.uint64), pc.restate_keys(zdepth, zindex), 'keys')
        for got, w in zip(images, want):
            pc.same(got, w, 'images')


def test_render_views_makes_no_device_to_host_copy(monkeypatch):
    rows = torch.from_numpy(pc.cloud(4099, np.random.default_rng(29))).to(DEV)
    rt_np, k_np = pc.cameras(3, 37, 53)
    cam_RT, cam_K = torch.from_numpy(rt_np[:, :3]).to(DEV), torch.from_numpy(k_np[:, :3, :3]).to(DEV)
    depth0 = pk.projection.render_views(rows, cam_RT, cam_K, 37, 53)['depth']
    torch.cuda.synchronize()
    seen = []

    def forbid(name, fn):
        def wrapper(self, *a, **kw):
            if self.is_cuda:
                seen.append(name)
            return fn(self, *a, **kw)
        return wrapper
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__int__', '__float__', '__index__'):
        monkeypatch.setattr(torch.Tensor, name, forbid(name, getattr(torch.Tensor, name)))
    torch.cuda.set_sync_debug_mode('error')                                # a blocking copy or a synchronising call raises
    try:
        img = pk.projection.render_views(rows, cam_RT, cam_K, 37, 53, channels=(3, 5), radius=1)
        codes = pk.projection.visibility(rows, depth0, cam_RT, cam_K, 0.05)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    monkeypatch.undo()
    assert seen == []
    assert all(img[key].is_cuda for key in ('depth', 'index', 'features')) and codes.is_cuda
    assert tuple(img['features'].shape) == (3, 37, 53, 2) and tuple(codes.shape) == (3, 4099)
    assert int((img['index'] >= 0).sum()) > 1000 and sorted(set(codes.reshape(-1).tolist())) == [0, 1, 2]


def test_evaluate_clip_groups_by_visibility():
    pc.check_evaluate_clip(DEV)
