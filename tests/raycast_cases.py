"""Shared by tests/test_raycast_host.py (through the g++ twin) and tests/test_gpu_raycast.py (on the device): the numpy float32
restatement of the ray-cast rules (include/ext/occ4d_raycast.h) in the stated operation order, the case matrix of the entry point, the
checks that do not use the restatement (the round trip through the projection, the analytic depth of a linear field) and the
end-to-end comparisons of perform_inference(views=...) on the tracking fixture.
Everything but the two independent checks is compared EQUAL: the non-NaN elements bit for bit, the NaN positions as positions.

The ray setup goes through libm's fmaf, one scalar at a time (as tests/project_cases.py does); the sample loop is vectorised over
the rays with masks."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk
from track_cases import same_bits, same_result

F32 = np.float32
GRIDS = [(2, 2, 2), (3, 2, 5), (17, 9, 33)]
IMAGES = [(1, 1), (5, 7), (16, 16), (20, 33)]         # (H, W): 7 x 5, 16 x 16, 33 x 20 pixels: ragged tiles, wave borders
VIEW_COUNTS = [1, 3]
STEP_COUNTS = [1, 2, 64]
CHANNEL_COUNTS = [0, 1, 5, 32]
PLACEMENTS = ['outside', 'inside', 'miss', 'behind', 'side']
D = 6                                 # width of the attribute array; a strided array has ld = D + PAD
PAD = 3
SENTINEL = 777.0
LEVEL = F32(0.46)
POOL = np.array([LEVEL, np.nextafter(LEVEL, F32(-1)), np.nextafter(LEVEL, F32(2)), 0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0],
                dtype=F32)
MINS, SPACINGS = (-1.25, 0.5, 3.0), (0.3, 0.7, 0.11)
# the frame of the exact cases: point i of an axis lies at i / 4, an exact float
EXACT_MINS, EXACT_SPACINGS = (-0.125, -0.125, -0.125), (0.25, 0.25, 0.25)

_fmaf = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6').fmaf
_fmaf.restype, _fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3


# ---------------------------------------------------------------------------------------------------------------- restatement
def _row(a, b):
    fma = lambda x, y, z: _fmaf(float(x), float(y), float(z))
    return F32(fma(a[3], b[3], fma(a[2], b[2], fma(a[1], b[1], F32(a[0]) * F32(b[0])))))


def ray_point(k_inv, rt_inv, px, py, d):
    """P(d) of the header for one pixel: three float32."""
    px, py, d = F32(px), F32(py), F32(d)
    q = (px * d, py * d, d, F32(1))
    s = [_row(k_inv[j], q) for j in range(4)]
    return [_row(rt_inv[a], s) for a in range(3)]


def rays(k_inv, rt_inv, H, W):
    """(P0, dir), both (V, H, W, 3) float32, of cameras k_inv, rt_inv (V, 4, 4) float32."""
    V = k_inv.shape[0]
    P0, P1 = np.zeros((V, H, W, 3), F32), np.zeros((V, H, W, 3), F32)
    with np.errstate(all='ignore'):
        for v in range(V):
            for py in range(H):
                for px in range(W):
                    P0[v, py, px] = ray_point(k_inv[v], rt_inv[v], px, py, 0.0)
                    P1[v, py, px] = ray_point(k_inv[v], rt_inv[v], px, py, 1.0)
        return P0, P1 - P0


def grid_coords(p, mins, spacings):
    """(R, 3) positions -> (R, 3) grid coordinates: (p - origin) / spacing - 0.5, each operation rounded to float32."""
    return (p - np.asarray(mins, F32)) / np.asarray(spacings, F32) - F32(0.5)


def lerp(a, b, w):
    return a + w * (b - a)


def trilinear(column, counts, c, w):
    """column (n,) float32; c (R, 3) cells, w (R, 3) float32 weights: z first, then y, then x."""
    nx, ny, nz = counts
    flat = (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]
    at = lambda ox, oy, oz: column[flat + (ox * ny + oy) * nz + oz]
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    v00, v01 = lerp(at(0, 0, 0), at(0, 0, 1), wz), lerp(at(0, 1, 0), at(0, 1, 1), wz)
    v10, v11 = lerp(at(1, 0, 0), at(1, 0, 1), wz), lerp(at(1, 1, 0), at(1, 1, 1), wz)
    return lerp(lerp(v00, v01, wy), lerp(v10, v11, wy), wx)


def cells_of(g, counts):
    top = np.asarray(counts, np.int64) - 2
    c = np.minimum(np.floor(g).astype(np.int64), top)
    return c, (g - c.astype(F32)).astype(F32)


def restate(field, counts, mins, spacings, level, k_inv, rt_inv, H, W, near, step, n_steps, attrs=None, cols=(), background=0.0,
            feature_background=None):
    """dict(depth (V, H, W) float32, cell (V, H, W) int32, features (V, H, W, C) float32, hit (V, H, W) bool, position
    (V, H, W, 3) float32: P0 + depth * dir of the hit rays)."""
    field = np.asarray(field, F32)
    k_inv, rt_inv = np.asarray(k_inv, F32).reshape(-1, 4, 4), np.asarray(rt_inv, F32).reshape(-1, 4, 4)
    V = k_inv.shape[0]
    level, near, step = F32(level), F32(near), F32(step)
    top = np.asarray(counts, F32) - F32(1)
    P0, direction = rays(k_inv, rt_inv, H, W)
    P0, direction = P0.reshape(-1, 3), direction.reshape(-1, 3)
    R = P0.shape[0]
    depth = np.zeros(R, F32)
    hit = np.zeros(R, bool)
    prev_in = np.zeros(R, bool)
    prev_v = np.zeros(R, F32)
    with np.errstate(all='ignore'):
        for i in range(n_steps):
            live = np.flatnonzero(~hit)
            if live.size == 0:
                break
            d = near + F32(i) * step
            g = grid_coords(P0[live] + d * direction[live], mins, spacings)
            inside = ((F32(0) <= g) & (g <= top)).all(axis=1)
            v = np.zeros(live.size, F32)
            c, w = cells_of(g[inside], counts)
            v[inside] = trilinear(field, counts, c, w)
            now = inside & (v >= level)
            refine = now & prev_in[live] & (prev_v[live] < level) & (i >= 1)
            t = (level - prev_v[live]) / (v - prev_v[live])
            t = np.where((t >= F32(0)) & (t <= F32(1)), t, F32(0.5)).astype(F32)
            d0 = near + F32(i - 1) * step
            depth[live[now]] = np.where(refine, d0 + t * (d - d0), d).astype(F32)[now]
            hit[live[now]] = True
            prev_in[live], prev_v[live] = inside, v
        position = P0 + depth[:, None] * direction
        g = np.fmin(np.fmax(grid_coords(position, mins, spacings), F32(0)), top)
        c, w = cells_of(g, counts)
        cell = np.where(hit, (c[:, 0] * counts[1] + c[:, 1]) * counts[2] + c[:, 2], -1).astype(np.int32)
        fbg = background if feature_background is None else feature_background
        feat = np.full((R, len(cols)), fbg, F32)
        for j, col in enumerate(cols):
            feat[hit, j] = trilinear(np.ascontiguousarray(attrs[:, col]), counts, c[hit], w[hit])
    depth = np.where(hit, depth, F32(background)).astype(F32)
    return dict(depth=depth.reshape(V, H, W), cell=cell.reshape(V, H, W), features=feat.reshape(V, H, W, len(cols)),
                hit=hit.reshape(V, H, W), position=position.reshape(V, H, W, 3))


def same_images(got, want):
    """got: (depth, cell, features) arrays or None each."""
    depth, cell, feat = got
    return ((depth is None or same_bits(depth, want['depth'])) and
            (cell is None or (cell.dtype == np.int32 and np.array_equal(cell, want['cell']))) and
            (feat is None or same_bits(feat, want['features'])))


# ---------------------------------------------------------------------------------------------------------------- inputs
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """(3, 4) float64 world -> camera, the camera's z axis from eye to target."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(z, np.array([0.0, 1.0, 0.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    return np.concatenate([Rm, (-Rm @ eye)[:, None]], axis=1)


def hull(counts, mins=MINS, spacings=SPACINGS):
    lo = np.array([m + 0.5 * s for m, s in zip(mins, spacings)])
    hi = np.array([m + (c - 0.5) * s for m, s, c in zip(mins, spacings, counts)])
    return lo, hi


def camera(placement, counts, H, W):
    """(cam_RT (3, 4), cam_K (3, 3)) float32 of one placement round the grid `counts` in the frame MINS / SPACINGS."""
    lo, hi = hull(counts)
    centre, ext = 0.5 * (lo + hi), hi - lo
    reach = float(np.linalg.norm(ext))
    f = 0.9 * max(H, W)
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f * 1.1, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    if placement == 'outside':                            # looking in from outside, obliquely
        RT = look_at(centre + np.array([-0.9, -0.7, 0.6]) * reach, centre)
    elif placement == 'inside':                           # inside the grid: the first sample may already be solid
        RT = look_at(centre + 0.05 * ext, centre + np.array([1.0, 0.3, 0.2]))
    elif placement == 'miss':                             # outside, the grid off to the side of every ray
        eye = centre + np.array([0.0, -3.0, 0.0]) * reach
        RT = look_at(eye, eye + np.array([1.0, 0.0, 0.0]))
    elif placement == 'behind':                           # outside, looking away from the grid
        eye = centre + np.array([-0.8, 0.0, 0.0]) * reach
        RT = look_at(eye, eye + np.array([-1.0, 0.1, 0.0]))
    elif placement == 'side':                             # along +y, half of the image beside the grid
        eye = centre + np.array([0.5 * ext[0], -0.8 * reach, 0.0])
        RT = look_at(eye, eye + np.array([0.0, 1.0, 0.0]))
    else:
        raise ValueError(placement)
    return RT.astype(F32), K.astype(F32)


def cameras(placements, counts, H, W):
    pairs = [camera(p, counts, H, W) for p in placements]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def march_of(counts, n_steps):
    """(near, step) such that n_steps = 64 samples reach through the grid from the outside placements; fewer steps stay near."""
    lo, hi = hull(counts)
    reach = float(np.linalg.norm(hi - lo))
    step = 2.6 * reach / 64.0
    return F32(step), F32(step)


def fields(scenario, n, rng):
    if scenario == 'pool':
        d = POOL[rng.integers(0, len(POOL), size=n)]
        mix = rng.uniform(size=n) < 0.6
        d[mix] = rng.uniform(-0.5, 1.2, size=int(mix.sum())).astype(F32)
        return d
    if scenario == 'all_above':
        return np.full(n, 0.9, F32)
    if scenario == 'all_below':
        return np.full(n, -2.0, F32)
    raise ValueError(scenario)


def blob(counts, rng, mins=MINS, spacings=SPACINGS):
    """A smooth field over the grid: high in a ball round the centre, low outside, plus a little noise."""
    lo, hi = hull(counts, mins, spacings)
    axes = [np.linspace(l, h, c) for l, h, c in zip(lo, hi, counts)]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    r = np.sqrt(sum(((A - 0.5 * (l + h)) / max(h - l, 1e-9)) ** 2 for A, l, h in zip((X, Y, Z), lo, hi)))
    return (0.9 - 1.6 * r + rng.uniform(-0.02, 0.02, size=r.shape)).astype(F32).reshape(-1)


def attributes(n, rng):
    return rng.uniform(-2.0, 2.0, size=(n, D)).astype(F32)


def columns(C, rng):
    return [int(c) for c in rng.integers(0, D, size=C)]


def padded(device, values, strided):
    """(buffer (rows, width + PAD) with the sentinel in the padding, or the dense array; its (rows, width) view)."""
    values = np.asarray(values, F32)
    rows, width = values.shape
    buf = torch.full((rows, width + PAD if strided else width), SENTINEL, dtype=torch.float32)
    buf[:, :width] = torch.from_numpy(values)
    buf = buf.to(device)
    return buf, buf[:, :width]


def inverses(cam_RT, cam_K):
    rt_inv, k_inv, rt64 = pk.projection.invert_cameras(cam_RT, cam_K)
    return rt_inv, k_inv


def raw_call(device, field_view, ld, counts, mins, spacings, level, k_inv, rt_inv, H, W, near, step, n_steps, attrs_view=None, ld_attr=0,
             d=0, cols=(), background=0.0, feature_background=0.0, want=(True, True, True), guard=3):
    """The entry point as it is, each output null where `want` says so, sentinel guards round every output.  -> three numpy arrays
    (or None)."""
    L, p = pk._lib.lib(), pk.ops._ptr
    V, C = k_inv.shape[0], len(cols)
    pixels = V * H * W
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32)).to(device)
    depth = torch.full((pixels + 2 * guard,), SENTINEL, dtype=torch.float32, device=device)
    cell = torch.full((pixels + 2 * guard,), -7, dtype=torch.int32, device=device)
    feat = torch.full((pixels * C + 2 * guard,), SENTINEL, dtype=torch.float32, device=device)
    k_t, rt_t = dev(k_inv), dev(rt_inv)
    arr = (ctypes.c_int32 * C)(*cols) if C else None
    status = L.occ4d_raycast_grid_f32(
        p(field_view), ld, *counts, mins[0], spacings[0], mins[1], spacings[1], mins[2], spacings[2], float(level), p(k_t), p(rt_t), V,
        H, W, float(near), float(step), n_steps, p(attrs_view), ld_attr, d, arr, C, float(background), float(feature_background),
        p(depth[guard:]) if want[0] else None, p(cell[guard:]) if want[1] else None, p(feat[guard:]) if want[2] and C else None,
        pk.ops._stream())
    assert status == pk._lib.OK, L.occ4d_last_error()
    out = []
    for t, fill, shape, wanted in ((depth, SENTINEL, (V, H, W), want[0]), (cell, -7, (V, H, W), want[1]),
                                   (feat, SENTINEL, (V, H, W, C), want[2])):
        a = t.cpu().numpy()
        assert (a[:guard] == fill).all() and (a[-guard:] == fill).all()
        if not wanted:
            assert (a == fill).all()
        out.append(a[guard:len(a) - guard].reshape(shape) if wanted else None)
    return out


# ---------------------------------------------------------------------------------------------------------------- the matrix
def check_cell(device, counts, image, placements, n_steps, C, strided, scenario, rng, want_outputs=(True, True, True)):
    """One cell: the raw entry point with padded strides when `strided`, ops.raycast_grid otherwise.  -> the restatement."""
    tag = (counts, image, placements, n_steps, C, strided, scenario, want_outputs)
    H, W = image
    n = counts[0] * counts[1] * counts[2]
    field = blob(counts, rng) if scenario == 'blob' else fields(scenario, n, rng)
    attrs, cols = attributes(n, rng), columns(C, rng)
    cam_RT, cam_K = cameras(placements, counts, H, W)
    rt_inv, k_inv = inverses(cam_RT, cam_K)
    near, step = march_of(counts, n_steps)
    want = restate(field, counts, MINS, SPACINGS, LEVEL, k_inv, rt_inv, H, W, near, step, n_steps, attrs, cols, background=-1.5,
                   feature_background=-2.5)
    field_buf, field_view = padded(device, field[:, None], strided)
    attr_buf, attr_view = padded(device, attrs, strided)
    if strided or want_outputs != (True, True, True):
        got = raw_call(device, field_view, field_buf.stride(0), counts, MINS, SPACINGS, LEVEL, k_inv, rt_inv, H, W, near, step, n_steps,
                       attr_view if C else None, attr_buf.stride(0) if C else 0, D if C else 0, cols, -1.5, -2.5, want_outputs)
    else:
        to = lambda a: torch.from_numpy(a).to(device)
        got = pk.ops.raycast_grid(field_view[:, 0], counts, MINS, SPACINGS, float(LEVEL), to(rt_inv), to(k_inv), H, W, float(near),
                                  float(step), n_steps, attrs=attr_view if C else None, channels=cols, background=-1.5,
                                  feature_background=-2.5)
        assert got[0].shape == (len(placements), H, W) and got[1].dtype == torch.int32 and got[2].shape == (len(placements), H, W, C), tag
        got = [g.cpu().numpy() for g in got]
    assert same_images(got, want), tag
    for a in got:                                         # no sentinel from the padding in any output
        assert a is None or not (a == SENTINEL).any(), tag
    assert (field_buf.cpu().numpy()[:, 1:] == SENTINEL).all() and (attr_buf.cpu().numpy()[:, D:] == SENTINEL).all(), tag
    if scenario == 'all_below':
        assert not want['hit'].any(), tag
    return want


def matrix_cells(counts):
    """The cells of one grid: every image x every view count, the other factors cycled so that each of their values occurs."""
    cells = []
    k = 0
    for image in IMAGES:
        for V in VIEW_COUNTS:
            placements = [PLACEMENTS[(k + j) % len(PLACEMENTS)] for j in range(V)]
            cells.append((image, placements, STEP_COUNTS[k % 3] if image != (20, 33) else 64, CHANNEL_COUNTS[k % 4], k % 2 == 1,
                          ('pool', 'blob')[(k // 2) % 2]))
            k += 1
    # the remaining step counts and channel counts with every placement at once, both field strides
    for n_steps in STEP_COUNTS:
        for strided in (False, True):
            cells.append(((5, 7), PLACEMENTS, n_steps, CHANNEL_COUNTS[(k + 1) % 4], strided, 'pool'))
            k += 1
    cells.append(((5, 7), PLACEMENTS[:3], 64, 32, True, 'blob'))
    cells.append(((16, 16), ['outside', 'inside', 'side'], 64, 5, False, 'all_above'))
    cells.append(((5, 7), ['outside', 'inside'], 64, 1, True, 'all_below'))
    return cells


def check_matrix(counts, device):
    rng = np.random.default_rng(7000 + counts[0] * 10000 + counts[1] * 100 + counts[2])
    hits = 0
    cells = matrix_cells(counts)
    for cell in cells:
        hits += int(check_cell(device, counts, *cell, rng)['hit'].sum())
    assert hits > 0, counts
    return len(cells)


def check_placements(device):
    """What each placement is there for, on the blob: outside and side hit and miss, inside hits on its first sample, miss and
    behind hit nothing."""
    counts, (H, W) = (17, 9, 33), (16, 16)
    rng = np.random.default_rng(5)
    seen = {}
    for placement in PLACEMENTS:
        want = check_cell(device, counts, (H, W), [placement], 64, 1, False, 'blob' if placement != 'inside' else 'all_above', rng)
        seen[placement] = want
    near, _ = march_of(counts, 64)
    assert seen['outside']['hit'].any() and not seen['outside']['hit'].all()
    assert seen['side']['hit'].any() and not seen['side']['hit'].all()
    assert seen['inside']['hit'].all() and (seen['inside']['depth'] == near).all()          # the first sample is already solid
    assert not seen['miss']['hit'].any() and not seen['behind']['hit'].any()


def check_null_outputs(device):
    """Each output pointer null in turn, and all of them."""
    rng = np.random.default_rng(11)
    for want_outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False), (True, False, False)):
        check_cell(device, (3, 2, 5), (5, 7), ['outside', 'inside', 'side'], 64, 5, True, 'blob', rng, want_outputs)


def exact_case(counts, rng, eye_z):
    """The frame whose points are exact floats, the identity camera at (0, 0, eye_z): pixel (px, py) has the direction (px, py, 1)
    and every sample lies ON a grid point (integer g on all axes, g = n - 1 included)."""
    n = counts[0] * counts[1] * counts[2]
    field = fields('pool', n, rng)
    RT = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [-eye_z]])], axis=1).astype(F32)
    return field, RT[None], np.eye(3, dtype=F32)[None]


def check_exact_grid_points(device):
    """An axis-aligned camera whose rays pass exactly through grid points: the value of a sample is the field's own value there,
    the hit cell is limited to n - 2 at g = n - 1."""
    rng = np.random.default_rng(3)
    for counts in GRIDS:
        for eye_z in (0.0, -0.5):
            field, cam_RT, cam_K = exact_case(counts, rng, eye_z)
            rt_inv, k_inv = inverses(cam_RT, cam_K)
            assert np.array_equal(rt_inv[0, :3, :3], np.eye(3)) and np.array_equal(k_inv[0], np.eye(4))
            H, W = counts[1], counts[0]                    # pixel (px, py) at depth 0.25 j from the eye: grid point (j px, j py, .)
            n_steps = 4 * counts[2] + 8
            want = restate(field, counts, EXACT_MINS, EXACT_SPACINGS, LEVEL, k_inv, rt_inv, H, W, 0.25, 0.25, n_steps)
            to = lambda a: torch.from_numpy(a).to(device)
            got = pk.ops.raycast_grid(to(field), counts, EXACT_MINS, EXACT_SPACINGS, float(LEVEL), to(rt_inv), to(k_inv), H, W, 0.25,
                                      0.25, n_steps)
            assert same_images([g.cpu().numpy() for g in got[:2]] + [None], want), (counts, eye_z)
            assert want['cell'].max() <= (counts[0] - 2) * counts[1] * counts[2] + (counts[1] - 2) * counts[2] + counts[2] - 2


def check_first_point_is_solid(device):
    """The exact frame again, finite values, the camera half a unit in front of grid point (0, 0, 0), which is solid: the ray of pixel
    (0, 0) runs along the points (0, 0, iz); its samples at depths 0.25 are outside the grid, the one at 0.5 is ON that point, whose
    own value it takes: depth 0.5 exactly, cell 0."""
    rng = np.random.default_rng(4)
    for counts in GRIDS:
        field, cam_RT, cam_K = exact_case(counts, rng, -0.5)
        field = rng.uniform(-0.5, 0.4, size=field.shape).astype(F32)
        field[0] = LEVEL                                    # value == level is inside
        rt_inv, k_inv = inverses(cam_RT, cam_K)
        to = lambda a: torch.from_numpy(a).to(device)
        depth, cell, feat = pk.ops.raycast_grid(to(field), counts, EXACT_MINS, EXACT_SPACINGS, float(LEVEL), to(rt_inv), to(k_inv), 1, 1,
                                                0.25, 0.25, 8, attrs=to(field[:, None]), channels=[0])
        assert depth.item() == 0.5 and cell.item() == 0 and feat.item() == float(LEVEL), counts
        field[0] = np.nextafter(LEVEL, F32(-1))             # one ulp below: not inside there
        depth, cell, _ = pk.ops.raycast_grid(to(field), counts, EXACT_MINS, EXACT_SPACINGS, float(LEVEL), to(rt_inv), to(k_inv), 1, 1,
                                             0.25, 0.25, 3)
        assert depth.item() == 0.0 and cell.item() == -1, counts


def check_argument_errors(device):
    """ops.raycast_grid: rejected arguments raise AssertionError with the library's text (the table of both libraries' texts is
    tests/test_gpu_raycast_contract_texts.py); V = 0 and H W = 0 are no-ops."""
    counts = (3, 2, 5)
    n = 30
    z = lambda *s: torch.zeros(*s, device=device)
    cams = z(1, 16)
    call = lambda **k: pk.ops.raycast_grid(**dict(dict(values=z(n), counts=counts, mins=MINS, spacings=SPACINGS, level=0.5, rt_inv=cams,
                                                       k_inv=cams, height=4, width=4, near=0.1, step=0.1, n_steps=4), **k))
    for kw, text in ((dict(counts=(30, 1, 1)), 'must be >= 2'), (dict(step=0.0), 'step = 0 must be finite and > 0'),
                     (dict(step=float('nan')), 'step = nan'), (dict(near=float('inf')), 'near = inf must be finite'),
                     (dict(n_steps=0), 'n_steps = 0 must be in 1 .. 65536'), (dict(n_steps=65537), 'n_steps = 65537'),
                     (dict(attrs=z(n, 2), channels=[2]), 'column 2 must be in 0 .. d - 1 = 1'),
                     (dict(attrs=z(n, 2), channels=[0] * 33), 'C = 33 must be in 0 .. 32')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for kw in (dict(rt_inv=z(0, 16), k_inv=z(0, 16)), dict(height=0), dict(width=0)):
        depth, cell, feat = call(**kw)
        assert depth.numel() == 0 and cell.numel() == 0
    depth, cell, feat = call(n_steps=65536, step=1e-6)
    assert (cell.cpu().numpy() == -1).all()


# ---------------------------------------------------------------------------------------------------------------- independent checks
# Worst absolute differences seen on the g++ twin (printed by the two checks below), and the tolerances taken from them: 4 x.
ROUND_TRIP_WORST, ROUND_TRIP_TOL = 2.55e-7, 1.02e-6
ANALYTIC_WORST, ANALYTIC_TOL = 2.29e-8, 9.16e-8


def check_round_trip(device):
    """(a) pixel_coords_from_point_cloud of every hit position returns the ray's own pixel after rint, and the ray's depth.  The
    hit position is P0 + depth * dir in float64 from the float32 matrices the library was given; the depth is compared with the
    projection's float32 depth and with a float64 evaluation of the same camera chain (row 2 of RT (x, y, z, 1)).
    On the g++ twin (799 hits, depths 2 to 8) the float64 comparison shows a worst difference of 2.55e-7 (the float32 projection:
    1.49e-7); the tolerance is 4 x that, ROUND_TRIP_TOL = 1.02e-6, for both comparisons, on the twin and on the device."""
    counts, (H, W) = (17, 9, 33), (20, 33)
    rng = np.random.default_rng(21)
    field = blob(counts, rng)
    cam_RT, cam_K = cameras(['outside', 'side', 'inside'], counts, H, W)
    rt_inv, k_inv = inverses(cam_RT, cam_K)
    near, step = march_of(counts, 64)
    to = lambda a: torch.from_numpy(a).to(device)
    depth, cell, _ = (t.cpu().numpy() for t in pk.ops.raycast_grid(to(field), counts, MINS, SPACINGS, float(LEVEL), to(rt_inv), to(k_inv),
                                                                   H, W, float(near), float(step), 64))
    worst32 = worst64 = 0.0
    total = 0
    for v in range(3):
        py, px = np.nonzero(cell[v] >= 0)
        total += py.size
        d = depth[v, py, px].astype(np.float64)
        q = np.stack([px * d, py * d, d, np.ones_like(d)])
        world = (rt_inv[v].astype(np.float64) @ (k_inv[v].astype(np.float64) @ q))[:3].T
        uvz = pk.projection.pixel_coords_from_point_cloud(np.ascontiguousarray(world, F32), cam_RT[v], cam_K[v])
        assert np.array_equal(np.rint(uvz[:, 0]), px) and np.array_equal(np.rint(uvz[:, 1]), py), v
        z64 = np.concatenate([world.astype(F32).astype(np.float64), np.ones((len(d), 1))], axis=1) @ cam_RT[v].astype(np.float64)[2]
        worst32 = max(worst32, float(np.abs(uvz[:, 2].astype(np.float64) - d).max()))
        worst64 = max(worst64, float(np.abs(z64 - d).max()))
    print('round trip: %d hits, worst |projected depth - ray depth| = %.3e (float32 chain), %.3e (float64 chain)' % (total, worst32, worst64))
    assert total > 300
    assert worst32 <= ROUND_TRIP_TOL and worst64 <= ROUND_TRIP_TOL, (worst32, worst64, ROUND_TRIP_TOL)


def check_analytic_depth(device):
    """(b) A field linear in x, seen by a camera that looks along +x: every ray crosses the level at the same camera depth,
    x* - eye_x = 2.776, whatever its pixel.  On the g++ twin the worst error over the 256 pixels is 2.29e-8 (a tenth of the depth's
    float32 spacing: every pixel gives the same float); the tolerance is 4 x that, ANALYTIC_TOL = 9.16e-8, on the twin and on the device."""
    counts, (H, W) = (17, 9, 33), (16, 16)
    lo, hi = hull(counts)
    x = np.linspace(lo[0], hi[0], counts[0])
    slope, x_star = 0.8, lo[0] + 0.37 * (hi[0] - lo[0])
    field = np.broadcast_to((float(LEVEL) + slope * (x - x_star))[:, None, None], counts).astype(F32).reshape(-1)
    centre = 0.5 * (lo + hi)
    eye = np.array([lo[0] - 1.0, centre[1], centre[2]])
    Rm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])          # camera z = world x
    cam_RT = np.concatenate([Rm, (-Rm @ eye)[:, None]], axis=1).astype(F32)[None]
    f = 40.0                                                                      # narrow: every ray crosses inside the hull
    cam_K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]], F32)[None]
    rt_inv, k_inv = inverses(cam_RT, cam_K)
    to = lambda a: torch.from_numpy(a).to(device)
    depth, cell, _ = (t.cpu().numpy() for t in pk.ops.raycast_grid(to(field), counts, MINS, SPACINGS, float(LEVEL), to(rt_inv), to(k_inv),
                                                                   H, W, 0.05, 0.05, 200))
    assert (cell >= 0).all()
    worst = float(np.abs(depth.astype(np.float64) - (x_star - eye[0])).max())
    print('analytic depth: expected %.6f, worst error %.3e' % (x_star - eye[0], worst))
    assert worst <= ANALYTIC_TOL, (worst, ANALYTIC_TOL)


# ---------------------------------------------------------------------------------------------------------------- end to end
COUNTS = rc.COUNTS
IMAGE = (12, 16)


def frame_of(shared):
    inf = shared.inputs[3]
    counts, mins, spacings = pk.geometry.grid_frame(rc.CASE['num_sample'], inf['min_z'], inf['cube_bounds'], 'greater', 4)
    assert tuple(counts) == COUNTS
    return mins, spacings


def fixture_cameras(shared):
    """(cam_RT (2, 3, 4), cam_K (3, 3)) round the fixture's query grid: one outside looking in, one from above."""
    mins, spacings = frame_of(shared)
    lo, hi = hull(COUNTS, mins, spacings)
    centre, reach = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    H, W = IMAGE
    K = np.array([[0.8 * W, 0.0, (W - 1) / 2.0], [0.0, 0.8 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]], F32)
    RT = np.stack([look_at(centre + np.array([-0.8, -0.5, 0.4]) * reach, centre),
                   look_at(centre + np.array([0.05, 0.0, 0.9]) * reach, centre)]).astype(F32)
    return RT, K


def fixture_views(shared, **kw):
    return pk.projection.FieldViews(*fixture_cameras(shared), *IMAGE, **kw)


def restate_views(shared, views, output, level=0.5):
    mins, spacings = frame_of(shared)
    field = output[:, 0]
    if views.select is not None:
        field = np.where(output[:, views.select[0]] >= F32(views.select[1]), field, F32(0))
    near, step, n_steps = pk.projection.march_range(COUNTS, mins, spacings, views.rt64, step=views.step)
    return restate(field, COUNTS, mins, spacings, level, views.k_inv, views.rt_inv, views.height, views.width, near, step, n_steps,
                   output, views.channels)


def check_against_restatement(shared, views, got, level=0.5):
    images = got['views']
    assert sorted(images) == ['cell', 'depth', 'features'] and all(isinstance(a, np.ndarray) for a in images.values())
    want = restate_views(shared, views, got['implicit_output'], level)
    assert same_images((images['depth'], images['cell'], images['features']), want)
    return want


def without_views(result):
    return {k: v for k, v in result.items() if k != 'views'}


def check_single_run(shared):
    views = fixture_views(shared, channels=(0, 1, 2, 3, 4))
    got = rc.infer(shared.device, shared.inputs, views=views)
    want = check_against_restatement(shared, views, got)
    assert want['hit'].any() and not want['hit'].all()                       # the fixture's condition: there is something to see
    same_result(without_views(got), shared.dense)
    views = fixture_views(shared, level=0.47, step=0.05)
    got = rc.infer(shared.device, shared.inputs, views=views)
    assert check_against_restatement(shared, views, got, level=0.47)['hit'].any()
    same_result(without_views(got), shared.dense)


def check_select(shared):
    """select = (track column, 0.5): the mask of the tracked object alone is a subset of the unselected render's hit mask."""
    track = pk.inference.get_track_idx(shared.inputs[3]['color_mode'])
    plain = rc.infer(shared.device, shared.inputs, views=fixture_views(shared))
    views = fixture_views(shared, select=(track, 0.5), channels=(track,))
    got = rc.infer(shared.device, shared.inputs, views=views)
    check_against_restatement(shared, views, got)
    mask, full = got['views']['cell'] >= 0, plain['views']['cell'] >= 0
    assert not (mask & ~full).any()
    same_result(without_views(got), shared.dense)
    # render_field on the array itself gives the same images
    mins, spacings = frame_of(shared)
    out = torch.from_numpy(got['implicit_output']).to(shared.device)
    again = pk.projection.render_field(out, COUNTS, mins, spacings, *fixture_cameras(shared), *IMAGE, 0.5, channels=(track,),
                                       select=(track, 0.5))
    assert same_images([again[k].cpu().numpy() for k in ('depth', 'cell', 'features')], got['views'])


def check_refine(shared):
    refine = pk.inference.GridRefine(2, 0.46, 1)
    views = fixture_views(shared, channels=(0, 4))
    plain = rc.infer(shared.device, shared.inputs, refine=refine)
    got = rc.infer(shared.device, shared.inputs, refine=refine, views=views)
    check_against_restatement(shared, views, got)
    same_result({k: v for k, v in without_views(got).items() if k != 'refine'}, {k: v for k, v in plain.items() if k != 'refine'})
    assert got['refine'] == plain['refine']


def check_track_all(shared):
    views = fixture_views(shared, channels=(0, 4))
    on_device = rc.infer(shared.device, shared.inputs, track_mode='all', views=views, track_merge='device')
    on_host = rc.infer(shared.device, shared.inputs, track_mode='all', views=views, track_merge='host')
    for got in (on_device, on_host):
        assert check_against_restatement(shared, views, got)['hit'].any()
        same_result(without_views(got), shared.dense_all)
    for k in ('depth', 'cell', 'features'):
        assert np.array_equal(on_device['views'][k], on_host['views'][k], equal_nan=True)


def check_clip(shared):
    """evaluate_clip(views=..., images=[]) over two frames: one dict per frame, that of the perform_inference call."""
    device = shared.device
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    views = fixture_views(shared, channels=(0, 1))
    images = []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, views=views, images=images)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(images) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        res = pk.inference.perform_inference(
            pcl.clone(), None, frames[t], [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=rc.CASE['num_sample'], point_sample_mode='grid', batch_size=rc.CASE['batch_size'],
            predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater',
            cube_mode=4, compress_air=True, point_occupancy_radius=0.8, views=views)
        assert same_images((images[t]['depth'], images[t]['cell'], images[t]['features']), res['views'])
        assert (images[t]['cell'] >= 0).any()
    with pytest.raises(ValueError, match='images'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', views=views)


def check_none_is_untouched(shared, monkeypatch):
    """views=None: no new key, the one host wait, the entry point is not called, implicit_output bit-identical; with views still
    one wait."""
    calls = rc.count_waits(monkeypatch)

    def forbidden(*a, **k):
        raise AssertionError('views=None must not reach the ray cast')
    monkeypatch.setattr(pk.ops, 'raycast_grid', forbidden)
    L = pk._lib.lib()
    for name in pk._lib.RAYCAST_SIGNATURES:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, views=None)
    assert calls == dict(wait=1)
    assert sorted(res) == ['features_global', 'gt_air', 'gt_solid', 'implicit_output', 'output_air', 'output_solid', 'pcl_abstract',
                           'points_query']
    same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, views=fixture_views(shared))
    assert calls['wait'] == 1


def check_value_errors(shared):
    views = fixture_views(shared)
    with pytest.raises(ValueError, match='grid'):
        rc.infer(shared.device, shared.inputs, views=views, point_sample_mode='random')
    with pytest.raises(ValueError):
        rc.infer(shared.device, shared.inputs, views=0.5)
    with pytest.raises(ValueError, match='NaN'):
        fixture_views(shared, level=float('nan'))
    with pytest.raises(ValueError, match='n_steps'):
        rc.infer(shared.device, shared.inputs, views=fixture_views(shared, step=1e-7))
    mins, spacings = frame_of(shared)
    with pytest.raises(ValueError, match='step'):
        pk.projection.march_range(COUNTS, mins, spacings, views.rt64, step=0.0)
    near, step, n_steps = pk.projection.march_range(COUNTS, mins, spacings, views.rt64)
    lo, hi = hull(COUNTS, mins, spacings)
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    depths = corners @ views.rt64[:, 2, :].T
    assert step == 0.5 * min(spacings) and near == max(depths.min(), step) and n_steps == int(np.ceil((depths.max() - near) / step)) + 1
