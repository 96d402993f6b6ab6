"""Writes tests/golden/project_*.npz: the REFERENCE's own pixel_coords_from_point_cloud (utils/geometry.py:67-115) on small
clouds -- inputs and outputs.  Container-only, like tests/gen_frontend_fixture.py: it imports the real reference through
oracle.ref_import.load() (unchanged).

    python tests/gen_project_fixture.py [OUT_DIR]

A case file holds pcl (N, D), cam_RT (3, 4), cam_K (3, 3), the image size, the reference's result `out` (N, D) and `out_flip`
(flip_xy=True), and for the visibility test a depth image (H, W) with holes and a margin.  The cameras are those of the synthetic
GREATER clip (gen_frontend_fixture.greater_cameras), a forward camera on the synthetic CARLA clip's first sensor pose, and two
random rigid cameras with a skewed K.  About an eighth of the points lie behind their camera and another eighth beside the image.
project_roundtrip.npz holds the reference's depth column for the rows the reference unprojects from one fixture RGB-D frame
(tests/golden/frontend_greater_a.npz: unprojected_v0_t0) under that frame's camera.

Margin condition, asserted at generation time: no u or v within 1e-3 px of a half-integer (a rounding boundary, the image's
borders -0.5, W - 0.5, H - 0.5 among them); no depth within 1e-4 of 0; no |depth - d - margin| < 1e-4 against the depth image's pixel.  Points that violate it are re-drawn until it holds: no decision hangs on a last bit and NO ROW
IS LEFT OUT of any comparison.  The round-trip rows are not drawn but derived: the generator asserts the condition on them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_frontend_fixture as fgen      # noqa: E402

PIXEL_MARGIN, DEPTH_MARGIN = 1e-3, 1e-4
# (name, camera, N, D, H, W, visibility margin, seed)
CASES = [
    ('project_greater_n2', ('greater', 0, 0), 2, 3, 48, 64, 0.05, 501),
    ('project_greater_n7', ('greater', 1, 2), 7, 8, 48, 64, 0.0, 502),
    ('project_greater_n1000', ('greater', 0, 1), 1000, 8, 48, 64, 0.05, 503),
    ('project_carla_n2000', ('carla', 0, 0), 2000, 11, 37, 53, 0.25, 504),
    ('project_skew_n257', ('skew', 0, 0), 257, 5, 3, 5, 0.1, 505),
    ('project_skew_n1025', ('skew', 1, 0), 1025, 4, 240, 320, 0.02, 506),
]
NAMES = [c[0] for c in CASES]
ROUNDTRIP = 'project_roundtrip'
ROUNDTRIP_FRAME = (0, 0)                   # (view, frame) of the synthetic GREATER clip


def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.concatenate([q, rng.uniform(-3.0, 3.0, size=(3, 1))], axis=1).astype(np.float32)


def camera(kind, a, b, H, W, rng):
    """-> cam_RT (3, 4), cam_K (3, 3), float32."""
    if kind == 'greater':
        cam_RT, cam_K = fgen.greater_cameras()
        return cam_RT[a, b], cam_K[a, b]
    if kind == 'carla':                    # a camera at the first sensor pose, looking along the sensor's +x (z forward, y down)
        crng = np.random.default_rng(fgen.CARLA['seed'])
        pose = fgen._rigid(crng, 0.3, [40.0, -12.0, 1.0]).astype(np.float64)
        axes = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
        cam_RT = (axes @ np.linalg.inv(pose))[:3].astype(np.float32)
        cam_K = np.array([[30.0, 0.0, W / 2.0], [0.0, 30.0, H / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)
        return cam_RT, cam_K
    cam_RT = _rigid(rng)
    f = 0.9 * W + 3.0 * a
    cam_K = np.array([[f, 0.37 * f / 10.0, W / 2.0 + 0.3], [0.0, 1.1 * f, H / 2.0 - 0.2], [0.0, 0.0, 1.0]], dtype=np.float32)
    return cam_RT, cam_K


def draw_points(rng, n, cam_RT, cam_K, H, W):
    """World points whose image lies on or around the (H, W) image at depths 1 .. 12, an eighth behind the camera."""
    uv = np.stack([rng.uniform(-0.15 * W - 2.0, 1.15 * W + 2.0, size=n), rng.uniform(-0.15 * H - 2.0, 1.15 * H + 2.0, size=n)], axis=1)
    z = rng.uniform(1.0, 12.0, size=n)
    z[rng.uniform(size=n) < 0.125] *= -1.0
    K, RT = cam_K.astype(np.float64), np.eye(4)
    RT[:3] = cam_RT
    cam = np.linalg.solve(K, np.concatenate([uv, np.ones((n, 1))], axis=1).T) * z
    world = np.linalg.solve(RT, np.concatenate([cam, np.ones((1, n))], axis=0))[:3].T
    return world.astype(np.float32)


def pixel_violations(out, H, W):
    """Rows of a reference result (x, y, depth first) that break the margin condition of the pixel rule."""
    u, v, z = (out[:, i].astype(np.float64) for i in range(3))
    bad = np.abs(z) < DEPTH_MARGIN
    for c, side in ((u, W), (v, H)):
        frac = c - np.floor(c)
        bad |= np.abs(frac - 0.5) < PIXEL_MARGIN                   # (the borders -0.5 and side - 0.5 are half-integers too)
    return bad


def visibility_violations(out, depth_image, margin):
    H, W = depth_image.shape
    z = out[:, 2]
    with np.errstate(invalid='ignore'):
        px, py = np.round(out[:, 0]), np.round(out[:, 1])
        on = (z > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    d = np.zeros(len(z))
    d[on] = depth_image[py[on].astype(np.int64), px[on].astype(np.int64)]
    return on & (d > 0) & (np.abs(z.astype(np.float64) - d - margin) < DEPTH_MARGIN)


def make_case(fn, name, cam, N, D, H, W, margin, seed):
    rng = np.random.default_rng(seed)
    cam_RT, cam_K = camera(cam[0], cam[1], cam[2], H, W, rng)
    depth_image = (np.round(rng.uniform(0.5, 13.0, size=(H, W)) * 64.0) / 64.0).astype(np.float32)      # (64ths: the file stays small)
    depth_image[rng.uniform(size=(H, W)) < 0.2] = 0.0                             # holes: they hide nothing
    pcl = np.concatenate([draw_points(rng, N, cam_RT, cam_K, H, W), rng.normal(size=(N, D - 3)).astype(np.float32)], axis=1)
    for attempt in range(100):
        out = fn(pcl.copy(), cam_RT.copy(), cam_K.copy())
        bad = pixel_violations(out, H, W) | visibility_violations(out, depth_image, margin)
        if not bad.any():
            break
        pcl[bad, :3] = draw_points(rng, int(bad.sum()), cam_RT, cam_K, H, W)
    else:
        raise RuntimeError('the margin condition could not be met')
    out_flip = fn(pcl.copy(), cam_RT.copy(), cam_K.copy(), flip_xy=True)
    assert out.dtype == np.float32 and out.shape == (N, D) and out_flip.dtype == np.float32
    assert (out[:, 2] < 0).any() or N < 7
    return dict(pcl=pcl, cam_RT=cam_RT, cam_K=cam_K, height=np.int64(H), width=np.int64(W), out=out, out_flip=out_flip,
                depth_image=depth_image, margin=np.float64(margin))


def make_roundtrip(fn):
    import conftest
    v, t = ROUNDTRIP_FRAME
    inp = conftest.load_golden('frontend_greater_inputs')
    rows = conftest.load_golden('frontend_greater_a')['unprojected_v%d_t%d' % (v, t)]
    H, W = inp['depth_u16'].shape[2:]
    out = fn(rows.copy(), inp['cam_RT'][v, t].copy(), inp['cam_K'][v, t].copy())
    assert out.dtype == np.float32 and not pixel_violations(out, H, W).any()
    ys, xs = np.where(inp['depth_u16'][v, t] > 0)
    assert np.array_equal(np.round(out[:, 0]), xs) and np.array_equal(np.round(out[:, 1]), ys) and (out[:, 2] > 0).all()
    return dict(view=np.int64(v), frame=np.int64(t), depth=out[:, 2].copy())


def write(out_dir):
    from oracle import ref_import
    fn = ref_import.load().geometry.pixel_coords_from_point_cloud
    os.makedirs(out_dir, exist_ok=True)
    files = {c[0]: make_case(fn, *c) for c in CASES}
    files[ROUNDTRIP] = make_roundtrip(fn)
    paths = []
    for name, arrays in files.items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < 480 * 1024, (path, size)
        paths.append((path, size))
    return paths


if __name__ == '__main__':
    for path, size in write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'golden')):
        print('%8d  %s' % (size, path))
