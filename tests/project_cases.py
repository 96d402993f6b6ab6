"""Shared by tests/test_project_host.py (through the g++ twin) and tests/test_gpu_project.py (on the device): a numpy restatement of
the z-buffer and visibility DECISIONS of include/occ4d_project.h, given (u, v, depth) -- per pixel the first row of
np.lexsort((index, depth)), the clipped footprint, the background rule, the three codes --, the case matrix of the four entry
points, the comparison with the reference's own pixel_coords_from_point_cloud (tests/golden/project_*.npz) and the round trip
with the front end's unprojection.  Everything is compared EQUAL: floats by their bits."""
import ctypes
import ctypes.util
import types

import numpy as np
import pytest
import torch

import gen_project_fixture as gen
import frontend_cases as fc
import occlusions4d_amd as pk
from conftest import load_golden

ROW_COUNTS = [0, 1, 2, 255, 256, 257, 1025, 262401]   # (262401 rows: more than one trip of the grid-stride loop)
VIEW_COUNTS = [1, 3]
IMAGES = [(1, 1), (3, 5), (37, 53), (240, 320)]
RADII = [0, 1, 4]
CHANNEL_COUNTS = [0, 1, 5, 32]
D = 6                                                 # row width of the matrix clouds; a strided view has ld = D + PAD
PAD = 3
SENTINEL = 777.0
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# the large row count is there for the trips of the grid-stride loop, which depend on the item count alone (a trip covers
# 1024 * 256 items): (views, image, radii, strided) -- three views make four trips, one view two; every pixel of the 1 x 1 image
# takes 262 401 atomics.  Every smaller row count takes the full cross.
LARGE_CELLS = [(3, (240, 320), [0], False), (1, (1, 1), [1], True)]
LARGE_CHANNEL_COUNTS = [0, 5]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), '%s: %d elements differ' % (what, int((bits(got) != bits(want)).sum()))


# ---------------------------------------------------------------------------------------------------------------- restatement
def on_image(uvz, H, W):
    """-> (mask (n,), px, py of the rows under the mask): the pixel rule on one view's (n, 3) float32 (u, v, depth)."""
    u, v, z = uvz[:, 0], uvz[:, 1], uvz[:, 2]
    with np.errstate(invalid='ignore'):
        ru, rv = np.round(u), np.round(v)                                     # (half to even, on float32)
        on = (z > 0) & np.isfinite(z) & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
    return on, ru[on].astype(np.int64), rv[on].astype(np.int64)


def restate_zbuffer(uvz, H, W, radius):
    """uvz (V, n, 3) -> (depth (V, H, W) float32 with 0 where empty, index (V, H, W) int64 with -1 where empty)."""
    V, n, _ = uvz.shape
    depth, index = np.zeros((V, H * W), np.float32), np.full((V, H * W), -1, np.int64)
    for v in range(V):
        on, px, py = on_image(uvz[v], H, W)
        rows = np.flatnonzero(on)
        pix, dep, ind = [], [], []
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                x, y = px + dx, py + dy
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)                  # the footprint is clipped to the image
                pix.append((y * W + x)[ok])
                dep.append(uvz[v, rows[ok], 2])
                ind.append(rows[ok])
        pix, dep, ind = np.concatenate(pix), np.concatenate(dep), np.concatenate(ind)
        order = np.lexsort((ind, dep, pix))                                   # per pixel: nearest first, lowest row on a tie
        first = np.ones(len(order), bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win = order[first]
        depth[v, pix[win]], index[v, pix[win]] = dep[win], ind[win]
    return depth.reshape(V, H, W), index.reshape(V, H, W)


def restate_keys(depth, index):
    keys = (bits(depth).astype(np.uint64) << np.uint64(32)) | (index & 0xFFFFFFFF).astype(np.uint64)
    return np.where(index >= 0, keys, EMPTY)


def restate_resolve(depth, index, rows, n, cols, background, feature_background):
    """The images of the first n rows of `rows`: a pixel whose index is >= n is background."""
    keep = (index >= 0) & (index < n)
    d = np.where(keep, depth, np.float32(background)).astype(np.float32)
    i = np.where(keep, index, -1).astype(np.int32)
    feat = np.full(index.shape + (len(cols),), feature_background, np.float32)
    if len(cols):
        feat[keep] = rows[index[keep]][:, cols]
    return d, i, feat


def restate_visibility(uvz, depth_images, margin):
    V, n, _ = uvz.shape
    H, W = depth_images.shape[1:]
    code = np.full((V, n), 2, np.int32)
    for v in range(V):
        on, px, py = on_image(uvz[v], H, W)
        z, d = uvz[v, on, 2], depth_images[v, py, px]
        with np.errstate(invalid='ignore'):
            code[v, on] = ((d > 0) & ((z - d) > np.float32(margin))).astype(np.int32)          # (float32 throughout)
    return code


_fmaf = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6').fmaf
_fmaf.restype, _fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3


def chain_restate(rows, rt, k):
    """The chain of include/occ4d_project.h written out with libm's fmaf, one scalar at a time: (V, n, 3) float32.  For the row
    counts the reference's numpy path cannot pin (a one-row cloud) and as a second opinion on small ones."""
    f32 = np.float32
    fma = lambda a, b, c: _fmaf(float(a), float(b), float(c))
    row = lambda a, b: f32(fma(a[3], b[3], fma(a[2], b[2], fma(a[1], b[1], f32(a[0]) * f32(b[0])))))
    out = np.zeros((rt.shape[0], rows.shape[0], 3), f32)
    with np.errstate(all='ignore'):
        for v in range(rt.shape[0]):
            for i in range(rows.shape[0]):
                p = (rows[i, 0], rows[i, 1], rows[i, 2], f32(1))
                c = [row(rt[v, j], p) for j in range(4)]
                q = (f32(c[0] / c[2]), f32(c[1] / c[2]), f32(1), c[3])
                out[v, i] = (row(k[v, 0], q), row(k[v, 1], q), c[2])
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def expand(cam_RT, cam_K):
    """numpy (V, 3, 4), (V, 3, 3) -> the expanded (V, 4, 4) pair."""
    V = cam_RT.shape[0]
    rt, k = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    rt[:, :3], k[:, :3, :3] = cam_RT, cam_K
    return rt, k


def cameras(V, H, W, focal=None):
    """View 0: the identity pose (depth = z, exactly) with a plain K; further views look at the cloud from the side."""
    f = 0.5 * W if focal is None else focal
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f * 1.25, (H - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32)
    RT = [np.eye(4, dtype=np.float32)[:3]] + [gen.fgen._look_at(eye, [0.0, 0.0, 6.0]) for eye in ([5.0, 1.0, 2.0], [-4.0, -3.0, 9.0])]
    return expand(np.stack(RT[:V]), np.stack([K] * V))


def adversarial_rows():
    """Rows that view 0 (identity pose) sees at exactly these depths: ties, 0, -0, a subnormal, +inf, NaN, u = +-1e30 z."""
    z = [2.0, 2.0, 2.0, 0.0, -0.0, 1e-40, np.inf, np.nan, 3.0, 3.0, 1.0, 1.0, -np.inf, 5.0, 5.0]
    x = [0.1, 0.1, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 3e30, -3e30, np.nan, np.inf, 0.0, -0.2, -0.2]
    rows = np.zeros((len(z), 3), np.float32)
    rows[:, 0], rows[:, 2] = x, z
    rows[:, 1] = rows[:, 0] * np.float32(0.5)
    return rows


def cloud(n, rng):
    """(n, D) rows: in front of view 0 at depths 1 .. 12 within and around its frustum, some behind it, the adversarial pool and
    exact duplicates of earlier rows spread through it."""
    z = rng.uniform(1.0, 12.0, size=n)
    z[rng.uniform(size=n) < 0.1] *= -1.0
    xy = rng.uniform(-1.2, 1.2, size=(n, 2)) * z[:, None] * np.array([1.0, 0.8])
    rows = np.concatenate([xy, z[:, None], rng.normal(size=(n, D - 3))], axis=1).astype(np.float32)
    if n >= 2:
        dup = rng.integers(0, n, size=max(1, n // 8))
        rows[dup, :3] = rows[rng.integers(0, n, size=len(dup)), :3]             # exact depth ties on one pixel
    pool = adversarial_rows()
    if n >= 2 * len(pool):
        at = rng.permutation(n)[:len(pool)]
        rows[at, :3] = pool
    rows[:, D - 1] = np.arange(n) % 1000                                       # (a feature that names the row)
    return rows


def place(array, strided, device):
    """`array` (n, d) as a device tensor: contiguous, or columns 0 .. d - 1 of an (n, d + PAD) buffer full of SENTINEL."""
    n, d = array.shape
    buf = torch.full((n, d + PAD if strided else d), SENTINEL, dtype=torch.float32, device=device)
    view = buf[:, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(array)))
    return buf, view


def depth_images(zdepth, rng):
    """Depth images for the visibility test out of a z-buffer's: shifted both ways, with holes, negative values, inf and NaN."""
    d = zdepth + rng.choice(np.array([-0.5, -0.01, 0.0, 0.01, 0.5, 2.0], np.float32), size=zdepth.shape)
    empty = zdepth == 0
    d[empty] = rng.uniform(0.5, 13.0, size=int(empty.sum())).astype(np.float32)
    special = rng.uniform(size=d.shape) < 0.15
    d[special] = rng.choice(np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1e-40], np.float32), size=int(special.sum()))
    return d.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the matrix
def columns(C):
    return [(3 * c + 1) % D for c in range(C)]


def check_cell(device, rows, V, H, W, radii, channel_counts, strided, rng, focal=None):
    """One (rows, views, image, stride) cell: projection, visibility, and for every radius the splat and for every channel count
    the resolve.  Returns the number of resolve comparisons made."""
    n = rows.shape[0]
    tag = (n, V, H, W, strided)
    rt_np, k_np = cameras(V, H, W, focal)
    rt, k = torch.from_numpy(rt_np).to(device), torch.from_numpy(k_np).to(device)
    buf, view = place(rows, strided, device)
    before = buf.clone()
    uvz_t = pk.ops.project_points(view, rt, k)
    uvz = uvz_t.cpu().numpy()
    assert uvz.shape == (V, n, 3) and uvz.dtype == np.float32
    if n <= 257:
        same(uvz, chain_restate(rows, rt_np, k_np), 'uvz %s' % (tag,))
        same(pk.ops.project_points(view, rt, k, flip_xy=True), uvz[:, :, [1, 0, 2]], 'uvz flipped %s' % (tag,))
    done = 0
    zdepth = None
    for radius in radii:
        zdepth, zindex = restate_zbuffer(uvz, H, W, radius)
        keys = pk.ops.zbuffer_splat(view, rt, k, H, W, radius)
        assert keys.dtype == torch.int64 and tuple(keys.shape) == (V, H, W)
        same(keys.cpu().numpy().view(np.uint64), restate_keys(zdepth, zindex), 'keys %s r=%d' % (tag, radius))
        for C in channel_counts:
            cols = columns(C)
            for n_known in sorted({n, n // 2}):                                # n // 2: the key image holds indices >= n
                known_buf, known = place(rows[:n_known], strided, device)
                depth, index, feat = pk.ops.zbuffer_resolve(keys, known, cols, background=-7.5, feature_background=9.25)
                want = restate_resolve(zdepth, zindex, rows, n_known, cols, -7.5, 9.25)
                what = '%s r=%d C=%d n_known=%d' % (tag, radius, C, n_known)
                same(depth, want[0], 'depth ' + what)
                same(index, want[1], 'index ' + what)
                same(feat, want[2], 'features ' + what)
                done += 1
    dimg = depth_images(zdepth, rng)
    dbuf = torch.full((V, H, W + PAD if strided else W), SENTINEL, dtype=torch.float32, device=device)
    dview = dbuf[:, :, :W]
    dview.copy_(torch.from_numpy(dimg))
    for margin in (0.0, 0.05):
        code = pk.ops.visibility(view, rt, k, dview, margin)
        same(code, restate_visibility(uvz, dimg, margin), 'codes %s margin=%g' % (tag, margin))
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), tag      # the rows are read only, the padding untouched
    assert not strided or bool((dbuf[:, :, W:] == SENTINEL).all()), tag
    return done


def check_matrix(n, device):
    rng = np.random.default_rng(2000 + n)
    rows = cloud(n, rng)
    done = 0
    if n > 100000:
        for V, (H, W), radii, strided in LARGE_CELLS:
            done += check_cell(device, rows, V, H, W, radii, LARGE_CHANNEL_COUNTS, strided, rng)
        return done
    for V in VIEW_COUNTS:
        for H, W in IMAGES:
            for strided in (False, True):
                done += check_cell(device, rows, V, H, W, RADII, CHANNEL_COUNTS, strided, rng)
    return done


def cells_of(n):
    known = len({n, n // 2})
    if n > 100000:
        return sum(len(radii) for _, _, radii, _ in LARGE_CELLS) * len(LARGE_CHANNEL_COUNTS) * known
    return len(VIEW_COUNTS) * len(IMAGES) * 2 * len(RADII) * len(CHANNEL_COUNTS) * known


def check_one_pixel(device, n=4099):
    """All n rows onto the ONE pixel of a 1 x 1 image (focal length 0): every atomic on one address; the nearest row wins."""
    rng = np.random.default_rng(77)
    rows = cloud(n, rng)
    rows = rows[np.isfinite(rows[:, :3]).all(axis=1)]
    rt_np, k_np = cameras(1, 1, 1, focal=0.0)
    rt, k = torch.from_numpy(rt_np).to(device), torch.from_numpy(k_np).to(device)
    dev_rows = torch.from_numpy(rows).to(device)
    uvz = pk.ops.project_points(dev_rows, rt, k).cpu().numpy()
    front = uvz[0, :, 2] > 0
    assert front.sum() > 3000 and (uvz[0, front, :2] == 0).all()
    keys = pk.ops.zbuffer_splat(dev_rows, rt, k, 1, 1, 4)
    depth, index, feat = pk.ops.zbuffer_resolve(keys, dev_rows, [D - 1])
    z = np.where(front, uvz[0, :, 2], np.inf)
    winner = int(np.flatnonzero(z == z.min())[0])
    assert int(index[0, 0, 0]) == winner and float(depth[0, 0, 0]) == float(z.min()) and float(feat[0, 0, 0, 0]) == rows[winner, D - 1]
    return done_keys(keys, z.min(), winner)


def done_keys(keys, depth, winner):
    want = (np.uint64(np.float32(depth).view(np.uint32)) << np.uint64(32)) | np.uint64(winner)
    assert keys.cpu().numpy().view(np.uint64).reshape(-1).tolist() == [int(want)]
    return True


def check_foreign_keys(device):
    """A key image that was not made from these rows: indices n, n + 1 and 0xFFFFFFF0 are background, n - 1 is gathered."""
    n = 10
    rows = cloud(n, np.random.default_rng(5))
    dev_rows = torch.from_numpy(rows).to(device)
    one = np.uint64(np.float32(1.5).view(np.uint32)) << np.uint64(32)
    keys = np.array([one | np.uint64(i) for i in (n - 1, n, n + 1, 0xFFFFFFF0, 0)] + [EMPTY], np.uint64).reshape(1, 2, 3)
    depth, index, feat = pk.ops.zbuffer_resolve(torch.from_numpy(keys.view(np.int64)).to(device), dev_rows, [0, D - 1], background=0.0,
                                                feature_background=-1.0)
    assert index.cpu().numpy().reshape(-1).tolist() == [n - 1, -1, -1, -1, 0, -1]
    assert depth.cpu().numpy().reshape(-1).tolist() == [1.5, 0.0, 0.0, 0.0, 1.5, 0.0]
    want = np.full((6, 2), -1.0, np.float32)
    want[0], want[4] = rows[n - 1][[0, D - 1]], rows[0][[0, D - 1]]
    same(feat.reshape(6, 2), want, 'foreign keys')


# ---------------------------------------------------------------------------------------------------------------- fixtures
def check_golden(name, device):
    """One fixture of the reference's pixel_coords_from_point_cloud: the wrapper (numpy in and tensor in, both flips), and
    the z-buffer and visibility decisions on the reference's own (u, v, depth)."""
    z = load_golden(name)
    pcl, cam_RT, cam_K, H, W = z['pcl'], z['cam_RT'], z['cam_K'], int(z['height']), int(z['width'])
    fn = pk.projection.pixel_coords_from_point_cloud
    got = fn(pcl, cam_RT, cam_K)
    assert isinstance(got, np.ndarray)
    same(got, z['out'], name + ' out')
    same(fn(pcl, cam_RT, cam_K, flip_xy=True), z['out_flip'], name + ' out_flip')
    as_tensor = fn(torch.from_numpy(pcl).to(device), torch.from_numpy(cam_RT), cam_K, flip_xy=False)
    assert isinstance(as_tensor, torch.Tensor) and as_tensor.device.type == device.type
    same(as_tensor, z['out'], name + ' out (tensor)')
    uvz = z['out'][None, :, :3]
    channels = list(range(3, pcl.shape[1]))
    for radius in (0, 1):
        img = pk.projection.render_views(torch.from_numpy(pcl).to(device), cam_RT[None], cam_K, H, W, channels=channels, radius=radius)
        zdepth, zindex = restate_zbuffer(uvz, H, W, radius)
        want = restate_resolve(zdepth, zindex, pcl, pcl.shape[0], channels, 0.0, 0.0)
        for key, w in zip(('depth', 'index', 'features'), want):
            same(img[key], w, '%s %s r=%d' % (name, key, radius))
    margin = float(z['margin'])
    code = pk.projection.visibility(pcl, z['depth_image'], cam_RT, cam_K, margin)
    want = restate_visibility(uvz, z['depth_image'][None], margin)
    same(code, want, name + ' codes')
    return want


def check_roundtrip(device):
    """The rows the library unprojects from a fixture RGB-D frame, rendered under the same camera at radius 0: the index image is
    the identity over the valid pixels and -1 elsewhere, the depth image holds the reference function's depth for those rows."""
    z = load_golden(gen.ROUNDTRIP)
    v, t = int(z['view']), int(z['frame'])
    inp = fc.greater_inputs()
    depth, rgb, flat = (torch.from_numpy(np.ascontiguousarray(inp[k][v, t][None])).to(device) for k in ('depth', 'rgb', 'flat'))
    H, W = depth.shape[1:]
    inv = lambda m: torch.from_numpy(pk.frontend.inverse_4x4(m[v, t][None])).to(device)
    big = 1e30
    rows, _, key = pk.frontend.rgbd_rows(depth, rgb, flat, inv(inp['cam_K']), inv(inp['cam_RT']), torch.from_numpy(inp['hue_clusters']).to(device),
                                         (-big, big, -big, big, -big, big), floor_fix=False)
    valid = inp['depth'][v, t].reshape(-1) > 0
    assert np.array_equal(key.cpu().numpy() > 0.5, valid)
    cloud_rows = rows[torch.from_numpy(valid).to(device)]
    assert cloud_rows.shape[0] == len(z['depth']) and 0 < valid.sum() < H * W
    img = pk.projection.render_views(cloud_rows, inp['cam_RT'][v, t][None], inp['cam_K'][v, t], H, W, channels=(4, 5, 6))
    want_index = np.full(H * W, -1, np.int32)
    want_index[valid] = np.arange(valid.sum())
    want_depth = np.zeros(H * W, np.float32)
    want_depth[valid] = z['depth']
    same(img['index'], want_index.reshape(1, H, W), 'round trip index')
    same(img['depth'], want_depth.reshape(1, H, W), 'round trip depth')
    want_rgb = np.where(valid[:, None], inp['rgb'][v, t].reshape(-1, 3), np.float32(0)).astype(np.float32)
    same(img['features'], want_rgb.reshape(1, H, W, 3), 'round trip colours')


# ---------------------------------------------------------------------------------------------------------------- evaluate_clip
def check_evaluate_clip(device):
    """evaluate_clip(stats_occlusion=...) against evaluate_clip(stats_group_fn=...) fed with codes that numpy makes of the chain
    restatement: equal EvalStats states, equal clip results; the depth images are z-buffers of the INPUT cloud (what a data set
    without depth frames would use).  Both keywords together raise."""
    import track_cases as tc
    pcl, sem, target, inf, enc, dec = tc.nets(device)
    frames = [target, target[:257] * np.float32(0.5)]
    batch = dict(pcl_input=pcl, pcl_input_sem=torch.from_numpy(sem)[None], pcl_target=[torch.from_numpy(f)[None] for f in frames],
                 meta_data=dict(pcl_target_size=[torch.tensor([f.shape[0]]) for f in frames]))
    args = types.SimpleNamespace(min_z=inf['min_z'], cr_cube_bounds=inf['cube_bounds'], color_mode=inf['color_mode'],
                                 sample_implicit=True, num_sample=tc.CASE['num_sample'], point_sample_mode='grid',
                                 implicit_batch_size=tc.CASE['batch_size'], segmentation_lw=0.0, track_mode='none',
                                 point_occupancy_radius=0.8, semantic_classes=13, density_threshold=0.5, cube_mode=4)
    H, W, margin = 37, 53, 0.05
    centre = target[:, :3].mean(axis=0).astype(np.float64)
    cam_RT = np.stack([gen.fgen._look_at(centre + eye, centre) for eye in ([6.0, 1.0, 2.5], [-2.0, 5.0, 1.0])])
    cam_K = np.array([[40.0, 0.0, W / 2.0], [0.0, 40.0, H / 2.0], [0.0, 0.0, 1.0]], np.float32)
    depth = pk.projection.render_views(pcl[0].to(device), cam_RT, cam_K, H, W, radius=1)['depth']
    assert 0 < int((depth > 0).sum()) < depth.numel()
    rt_np, k_np = expand(cam_RT, np.stack([cam_K] * 2))
    depth_np = depth.cpu().numpy()
    codes = {f.shape[0]: restate_visibility(chain_restate(f[:, :3], rt_np[t:t + 1], k_np[t:t + 1]), depth_np[t:t + 1], margin)[0]
             for t, f in enumerate(frames)}
    assert all(set(np.unique(c)) == {0, 1, 2} for c in codes.values()), [np.bincount(c) for c in codes.values()]
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', **kw)
    by_fn, by_occlusion, plain = (pk.evaluation.EvalStats(3, 0, device) for _ in range(3))
    occlusion = dict(depth=depth, cam_RT=cam_RT, cam_K=cam_K, margin=margin)
    res_fn = run(stats=by_fn, stats_group_fn=lambda rows: codes[rows.shape[0]])
    res_occlusion = run(stats=by_occlusion, stats_occlusion=occlusion)
    res_plain = run(stats=plain)
    a, b, c = by_fn.state(), by_occlusion.state(), plain.state()
    assert a['counts'].sum() > 0 and np.array_equal(a['counts'], b['counts']) and np.array_equal(a['sums'], b['sums'])
    head = pk._lib.EVAL_CONSTANTS['HEAD']
    per = lambda s: s['counts'][head:].reshape(3, -1)
    assert (per(a).sum(axis=1) > 0).all()                                  # every group scored something
    assert np.array_equal(per(a).sum(axis=0), per(c)[0]) and not per(c)[1:].any()      # the default call: one group, the same totals
    for other in (res_occlusion, res_plain):
        assert len(other) == len(res_fn) == 2
        for x, y in zip(res_fn, other):
            assert len(x) == len(y) and all(p.dtype == q.dtype and np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))
    try:
        run(stats=by_fn, stats_group_fn=lambda rows: codes[rows.shape[0]], stats_occlusion=occlusion)
    except AssertionError as e:
        assert 'exclude' in str(e)
    else:
        raise RuntimeError('both keywords were accepted')
    try:
        run(stats=pk.evaluation.EvalStats(2, 0, device), stats_occlusion=occlusion)
    except AssertionError as e:
        assert 'n_groups' in str(e)
    else:
        raise RuntimeError('two groups were accepted')
    assert np.array_equal(by_fn.state()['counts'], a['counts'])            # (the rejected calls added nothing)


def check_argument_errors(device):
    """The contract of the four entry points, as the library on `device` states it (csrc/project_math.hpp: one source for both
    libraries).  Every non-null pointer is a real tensor that covers the call even if it were accepted."""
    z = lambda *shape, **kw: torch.zeros(*shape, device=device, **kw)
    rows, rt, k = z(10, 6), torch.eye(4, device=device).reshape(1, 16), torch.eye(4, device=device).reshape(1, 16)
    ops = pk.ops
    with pytest.raises(AssertionError, match='radius'):
        ops.zbuffer_splat(rows, rt, k, 4, 4, radius=5)
    with pytest.raises(AssertionError, match='radius'):
        ops.zbuffer_splat(rows, rt, k, 4, 4, radius=-1)
    with pytest.raises(AssertionError, match='H = 0'):
        ops.zbuffer_splat(rows, rt, k, 0, 4)
    with pytest.raises(AssertionError, match='W = 40000'):
        ops.zbuffer_splat(rows, rt, k, 4, 40000)
    with pytest.raises(AssertionError, match='keys must be'):
        ops.zbuffer_splat(rows, rt, k, 4, 4, keys=z(1, 4, 5, dtype=torch.int64))
    with pytest.raises(AssertionError, match='x, y, z'):
        ops.project_points(z(10, 2), rt, k)
    with pytest.raises(AssertionError, match='rt / k'):
        ops.project_points(rows, rt, z(2, 16))
    keys = ops.zbuffer_splat(rows, rt, k, 4, 4)
    with pytest.raises(AssertionError, match='column 6'):
        ops.zbuffer_resolve(keys, rows, [0, 6])
    with pytest.raises(AssertionError, match='column -1'):
        ops.zbuffer_resolve(keys, rows, [-1])
    with pytest.raises(AssertionError, match='C = 33'):
        ops.zbuffer_resolve(keys, rows, [0] * 33)
    with pytest.raises(AssertionError, match='depth must be'):
        ops.visibility(rows, rt, k, z(2, 4, 4), 0.0)
    L, p = pk._lib.lib(), pk.ops._ptr                                 # what no tensor can express: short strides, null arrays
    code = z(10, dtype=torch.int32)
    img = z(1, 4, 4)
    rt3, k3, uvz = rt.repeat(3, 1), k.repeat(3, 1), z(30)
    assert L.occ4d_project_points_f32(p(rows), 2, 10, p(rt), p(k), 1, 0, p(uvz), None) == pk._lib.EINVAL
    assert L.occ4d_project_points_f32(None, 6, 10, p(rt), p(k), 1, 0, p(uvz), None) == pk._lib.EINVAL
    assert L.occ4d_project_points_f32(p(rows), 6, 10, p(rt), p(k), 1, 0, None, None) == pk._lib.EINVAL
    assert L.occ4d_project_points_f32(p(rows), 6, -1, p(rt), p(k), 1, 0, None, None) == pk._lib.EINVAL
    assert L.occ4d_zbuffer_splat_f32(p(rows), 6, 10, p(rt), p(k), 1, 4, 4, 0, None, None) == pk._lib.EINVAL
    assert L.occ4d_zbuffer_splat_f32(p(rows), 6, 10, p(rt3), p(k3), 3, 32768, 32768, 0, p(keys), None) == pk._lib.EINVAL
    assert L.occ4d_zbuffer_resolve_f32(None, 1, 4, 4, p(rows), 6, 10, 6, 0.0, p(img), None, None, 0, 0.0, None, None) == pk._lib.EINVAL
    assert L.occ4d_zbuffer_resolve_f32(p(keys), 1, 4, 4, p(rows), 5, 10, 6, 0.0, p(img), None, (ctypes.c_int32 * 1)(0), 1, 0.0, p(img),
                                       None) == pk._lib.EINVAL
    assert L.occ4d_visibility_f32(p(rows), 6, 10, p(rt), p(k), 1, p(img), 3, 4, 4, 0.0, p(code), None) == pk._lib.EINVAL
    assert L.occ4d_visibility_f32(p(rows), 6, 10, p(rt), p(k), 1, None, 4, 4, 4, 0.0, p(code), None) == pk._lib.EINVAL
    assert b'occ4d_visibility_f32' in L.occ4d_last_error()
    assert L.occ4d_project_points_f32(None, 6, 0, None, None, 1, 0, None, None) == pk._lib.OK                    # n = 0, V = 0
    assert L.occ4d_zbuffer_splat_f32(None, 6, 10, None, None, 0, 4, 4, 0, None, None) == pk._lib.OK
    assert L.occ4d_zbuffer_resolve_f32(None, 0, 4, 4, None, 6, 10, 6, 0.0, None, None, None, 0, 0.0, None, None) == pk._lib.OK
    assert L.occ4d_visibility_f32(None, 6, 0, None, None, 1, None, 4, 4, 4, 0.0, None, None) == pk._lib.OK
    assert bool((keys == -1).all()) and float(rows.abs().sum()) == 0.0            # (rows at the camera centre: depth 0, no splat)
