"""Shared by tests/test_occl_host.py (g++ twin) and tests/test_gpu_occl.py (HIP): a numpy restatement of the segmented id
histogram (include/occ4d_occl.h) -- plain `==` / `<` per bin, int64 --, the case matrix, and the comparisons of
occlusions4d_amd.occlusion against the reference's own results (tests/golden/occl_*.npz, written by tests/gen_occl_fixture.py).
Counts must be EQUAL: there is no tolerance anywhere."""
import itertools

import numpy as np
import pytest
import torch

import frontend_cases as fc
import gen_occl_fixture as gen
import occlusions4d_amd as pk
from conftest import load_golden

# one beyond a single trip of the kernel's grid (GRID_CAP = 1024 workgroups x 256 rows = 262 144 rows, + one tile + 1 row):
# workgroups then walk more than one tile
ROW_COUNTS = [0, 1, 255, 256, 257, 1000, 262401]
SEGMENTS = [1, 3, 48]
N_IDS = [1, 12, 4096]
D, LD, COL, PRED_COL = 6, 9, 3, 5                                  # rows (n, 6) inside a (n, 9) buffer: ld > d
PREDICATES = [(), (4.0,), (4.0, 10.0)]


def restate(rows, col, offsets, n_ids, key=None, pred_col=-1, pred_values=()):
    """(S, n_ids + 2) int64.  Bin i: counted rows with value == i; n_ids: value < 0; n_ids + 1: the rest."""
    rows = np.asarray(rows)
    S = len(offsets) - 1
    out = np.zeros((S, n_ids + 2), dtype=np.int64)
    counted = np.ones(rows.shape[0], dtype=bool)
    if key is not None:
        counted &= np.asarray(key) > np.float32(0.5)
    if pred_values:
        p = rows[:, pred_col]
        counted &= np.logical_or.reduce([p == np.float32(v) for v in pred_values])
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        v = rows[lo:hi, col][counted[lo:hi]]
        with np.errstate(invalid='ignore'):
            present = np.unique(v[(v >= 0) & (v < n_ids)])         # (a bin no value compares equal to is zero: skip its scan)
            for i in present[present == np.floor(present)].astype(np.int64):
                out[s, i] = (v == np.float32(i)).sum()
            out[s, n_ids] = (v < 0).sum()
        out[s, n_ids + 1] = v.shape[0] - out[s].sum()
    return out


def offsets_for(n, S, rng):
    """S + 1 ascending offsets from 0 to n: the first segment shorter than a wave, some segments empty, no boundary chosen
    as a multiple of 256."""
    if S == 1:
        return np.array([0, n], dtype=np.int64)
    cuts = np.sort(rng.integers(0, n + 1, size=S - 1))
    cuts[0] = min(n, 37)
    if S > 3:
        cuts[3] = cuts[2]                                            # an empty segment in the middle
        cuts[-1] = n                                                 # and an empty last one
    return np.concatenate([[0], np.sort(cuts), [n]]).astype(np.int64)


def make_rows(n, n_ids, kind, rng):
    """-> (view (n, D) of a (n, LD) buffer, key (n)).  'mixed': a few ids of the range with n_ids - 1, n_ids, -1, -0.0, 2.5, NaN
    and +inf among them; 'same': every row the id n_ids - 1 (the most contention on one bin)."""
    buf = rng.uniform(-1, 1, size=(n, LD)).astype(np.float32)
    if kind == 'same':
        ids = np.full(n, n_ids - 1, dtype=np.float32)
    else:
        pool = np.concatenate([rng.integers(0, n_ids, size=6), [0, n_ids - 1, n_ids, n_ids + 3]]).astype(np.float32)
        pool = np.concatenate([pool, np.array([-1.0, -0.0, 2.5, np.nan, np.inf, -np.inf, -3.0], dtype=np.float32)])
        ids = pool[rng.integers(0, len(pool), size=n)]
        runs = rng.uniform(size=n) < 0.5                             # runs of one value, as image rows have them
        ids[runs] = np.float32(-1.0) if n_ids == 1 else pool[0]
    buf[:, COL] = ids
    buf[:, PRED_COL] = np.array([0.0, 4.0, 10.0, 7.0], dtype=np.float32)[rng.integers(0, 4, size=n)]
    key = np.array([0.0, 1.0, 1.0, 0.5], dtype=np.float32)[rng.integers(0, 4, size=n)]       # (0.5 is NOT > 0.5)
    return buf[:, :D], key


def matrix(n):
    """Every (S, n_ids, key, predicate, kind) combination for n rows."""
    for S, n_ids, with_key, pred in itertools.product(SEGMENTS, N_IDS, (False, True), PREDICATES):
        kinds = ('mixed', 'same') if (not with_key and not pred) else ('mixed',)
        for kind in kinds:
            yield S, n_ids, with_key, pred, kind


def check_matrix(n, device):
    """The whole matrix for one row count on one device, and that a second call doubles every entry."""
    checked = 0
    for S, n_ids, with_key, pred, kind in matrix(n):
        rng = np.random.default_rng(1000 * S + n_ids + 7 * len(pred) + with_key)
        rows, key = make_rows(n, n_ids, kind, rng)
        off = offsets_for(n, S, rng)
        want = restate(rows, COL, off, n_ids, key if with_key else None, PRED_COL, pred)
        assert want.sum() <= n and (with_key or pred or want.sum() == n)
        r = torch.from_numpy(np.ascontiguousarray(rows.base)).to(device)[:, :D]
        k = torch.from_numpy(key).to(device) if with_key else None
        kw = dict(key=k, pred_col=PRED_COL if pred else -1, pred_values=pred)
        got = pk.ops.id_histogram(r, COL, off, n_ids, **kw)
        what = 'n=%d S=%d n_ids=%d key=%s pred=%s %s' % (n, S, n_ids, with_key, pred, kind)
        assert got.dtype == torch.int32 and tuple(got.shape) == (S, n_ids + 2), what
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), what
        if checked % 9 == 0:                                         # ADDS onto its output; offsets as a device tensor
            again = pk.ops.id_histogram(r, COL, torch.from_numpy(off).to(device), n_ids, out=got, **kw)
            assert again is got and np.array_equal(got.cpu().numpy().astype(np.int64), 2 * want), what + ' (second call)'
        checked += 1
    return checked


# ------------------------------------------------------------------------------------------------------------ the goldens
GOLDEN_NAMES = [c[0] for c in gen.GREATER_CASES] + [c[0] for c in gen.CARLA_CASES]


def golden_arguments(name, device):
    """The arguments of occlusion.valo_ids for one fixture, rebuilt from its integer columns: clouds that are zero but for the
    instance id (and semantic tag) columns."""
    g = load_golden('occl_' + name)
    carla = name.startswith('carla')
    kw = (gen.CARLA_BY_NAME if carla else gen.GREATER_BY_NAME)[name][1]
    width, cols, sem_width, sem_cols = (9, [4, 5], 3, [1, 2]) if carla else (7, [3], 1, [0])
    V = len({k.split('_')[1] for k in g if k.startswith('cloud_')})
    T = len([k for k in g if k.startswith('cloud_v0_')])

    def cloud(a, w, c):
        out = np.zeros((a.shape[0], w), dtype=np.float32)
        out[:, c] = a
        return torch.from_numpy(out).to(device)
    all_pcl = [[cloud(g['cloud_v%d_t%d' % (v, t)], width, cols) for t in range(T)] for v in range(V)]
    sem = cloud(g['input_sem'], sem_width, sem_cols)
    merged = [cloud(g['merged_%d' % t][:, None], width + 1, cols[:1]) for t in range(T)]
    args = dict(live_occl_mode=str(g['live_occl_mode']), filter_vehped=carla, sem_inst_col=1 if carla else 0,
                sem_cat_col=2 if carla else None, merged_inst_col=4 if carla else 3, pcl_input_frames=kw['pcl_input_frames'],
                video_length=T, src_view=0 if carla else kw['src_view'], num_views=V,
                max_valo_ids=gen.MAX_VALO_CARLA if carla else gen.MAX_VALO_GREATER, all_pcl=all_pcl, pcl_input_sem=sem,
                pcl_merged_frames=merged)
    return args, g


def same_valo(got, g, what):
    live_occl, ids, num, mask = got
    assert live_occl.dtype == np.float64 and live_occl.shape == g['live_occl'].shape, what
    assert np.array_equal(live_occl, g['live_occl']), what + ': live_occl'
    assert ids.dtype == np.int32 and np.array_equal(ids, g['valo_ids']), what + ': valo_ids'
    assert num == int(g['num_valo_ids']), what + ': num_valo_ids'
    if 'vehped_mask' in g:
        assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), g['vehped_mask']), what + ': vehped_mask'
    else:
        assert mask is None


def check_valo_golden(name, device, **override):
    args, g = golden_arguments(name, device)
    args.update(override)
    same_valo(pk.occlusion.valo_ids(**args), g, name)
    if not str(g['live_occl_mode']).startswith('unfilt'):          # merged frames not given: the sum over the views
        same_valo(pk.occlusion.valo_ids(**dict(args, pcl_merged_frames=None)), g, name + ' (views summed)')


def check_track_golden(name, device, **override):
    """choose_track_id from the generator state the reference's choice started from: the id and the state afterwards."""
    g = load_golden('occl_' + name)
    sem = torch.from_numpy(g['input_sem'].astype(np.float32)).to(device)
    pcl_input = torch.zeros((sem.shape[0], 7), dtype=torch.float32)
    pcl_input[:, 6] = torch.from_numpy(g['input_t'].astype(np.float32))
    np.random.seed(0)
    state = list(np.random.get_state())
    state[1], state[2] = g['np_state_before'], int(g['np_pos_before'])
    np.random.set_state(tuple(state))
    got = pk.occlusion.choose_track_id(pcl_input.to(device), sem, str(g['track_mode']), **override)
    after = np.random.get_state()
    assert got == int(g['track_id']), name
    assert np.array_equal(after[1], g['np_state']) and after[2] == int(g['np_pos']), name + ': numpy generator state'
    return got


# ------------------------------------------------------------------------------------------------------------ the clips
def greater_clip(name, device, **extra):
    _, kw, mode, track_mode, _ = gen.GREATER_BY_NAME[name]
    g = load_golden('occl_' + name)
    fc.seed(g['seed'])
    return pk.frontend.greater_clip(device=device, **fc.greater_inputs(), **kw, **extra), g, mode, track_mode


def carla_clip(name, device, **extra):
    _, kw, mode, _ = gen.CARLA_BY_NAME[name]
    g = load_golden('occl_' + name)
    lidar, inp = fc.carla_inputs()
    assert int(g['id_mod']) == gen.CARLA_ID_MOD
    fc.seed(g['seed'])
    got = pk.frontend.carla_clip(gen.carla_variant(lidar), inp['sensor_RT'], min_z=float(inp['min_z']),
                                 other_bounds=float(inp['other_bounds']), target_bounds=float(inp['target_bounds']), device=device,
                                 **kw, **extra)
    return got, g, mode


def generator_state():
    s = np.random.get_state()
    return s[1].copy(), s[2], torch.get_rng_state().numpy().copy()


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def same_clouds(a, b):
    assert torch.equal(a[0][:, :7], b[0][:, :7]) and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2])
    assert all(torch.equal(x[:, :-1], y[:, :-1]) for x, y in zip(a[2], b[2]))


def check_clip_meta(meta, g, what):
    same_valo((meta['live_occl'], meta['valo_ids'], meta['num_valo_ids'], None), {k: v for k, v in g.items() if k != 'vehped_mask'}, what)


def check_greater_clip(name, device):
    """The clip with the new arguments against the fixture (fractions, ids, track id, marks, generator state), and against
    the clip without them (clouds bit-identical, meta keys, generator consumption)."""
    plain, g, mode, track_mode = greater_clip(name, device)
    state_plain = generator_state()
    assert sorted(plain[3]) == sorted(['cuboid_filter_ratios', 'pcl_sizes', 'sample_input_ratios', 'sample_target_ratios',
                                       'pcl_input_size', 'pcl_target_size'])
    occl, _, _, _ = greater_clip(name, device, live_occl_mode=mode)
    assert same_state(generator_state(), state_plain)
    same_clouds(plain, occl)
    assert torch.equal(plain[0], occl[0])                            # (track_id = -1 in both)
    assert sorted(set(occl[3]) - set(plain[3])) == ['live_occl', 'num_valo_ids', 'valo_ids']
    check_clip_meta(occl[3], g, name)
    both, _, _, _ = greater_clip(name, device, live_occl_mode=mode, track_mode=track_mode, track_id=7)
    state_both = generator_state()
    same_clouds(plain, both)
    check_clip_meta(both[3], g, name + ' + track_mode')
    assert both[3]['track_id'] == int(g['track_id'])
    assert np.array_equal(state_both[0], g['np_state']) and state_both[1] == int(g['np_pos']), name + ': numpy generator state'
    assert np.array_equal(state_both[2], g['torch_state'])
    if track_mode != 'random' or int(g['np_pos']) == int(g['np_pos_before']):
        assert same_state(state_both, state_plain)
    assert np.array_equal(both[0][:, 7].cpu().numpy(), g['input_mark'].astype(np.float32)), name + ': input mark'
    for i, frame in enumerate(both[2]):
        assert np.array_equal(frame[:, 8].cpu().numpy(), g['target_mark_%d' % i].astype(np.float32)), name + ': target mark'
    only, _, _, _ = greater_clip(name, device, track_mode='snitch')
    assert sorted(set(only[3]) - set(plain[3])) == ['track_id'] and same_state(generator_state(), state_plain)
    return both


def check_carla_clip(name, device):
    plain, g, mode = carla_clip(name, device)
    state_plain = generator_state()
    occl, _, _ = carla_clip(name, device, live_occl_mode=mode)
    assert same_state(generator_state(), state_plain)
    assert np.array_equal(state_plain[0], g['np_state']) and state_plain[1] == int(g['np_pos'])
    assert torch.equal(plain[0], occl[0]) and torch.equal(plain[1], occl[1])
    assert all(torch.equal(x, y) for x, y in zip(plain[2], occl[2]))
    assert sorted(set(occl[3]) - set(plain[3])) == ['live_occl', 'num_valo_ids', 'valo_ids'] and set(plain[3]) <= set(occl[3])
    check_clip_meta(occl[3], g, name)
    assert np.array_equal(occl[1].cpu().numpy()[:, 1:], g['input_sem'].astype(np.float32))
    return occl


class TransferCount:
    """Counts torch.Tensor.cpu() / .item() / .tolist() calls on device tensors while it is active."""

    def __enter__(self):
        self.n, self.saved = 0, {}
        for name in ('cpu', 'item', 'tolist'):
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.n += 1
                return _orig(t, *a, **k)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


class _Log:
    def warning(self, *a, **k):
        pass


def through_the_sampler(got, kind, bias, cube_bounds):
    """valo_ids / num_valo_ids of a clip are what GuidedImplicitPointSampler takes (a batch of one; the sampler's kernels
    are not part of the g++ twin, so this runs on the device only)."""
    _, _, targets, meta = got
    sampler = pk.geometry.GuidedImplicitPointSampler(_Log(), min_z=-1.0, cube_bounds=cube_bounds, point_occupancy_radius=0.2,
                                                     num_solid=64, num_air=64, data_kind=kind, point_sample_bias=bias)
    res = sampler([f[None] for f in targets], [torch.tensor([f.shape[0]]) for f in targets],
                  torch.from_numpy(meta['valo_ids'])[None], torch.tensor([meta['num_valo_ids']]), 0)
    assert tuple(res[0].shape) == (1, 64, 4) and tuple(res[1].shape) == (1, 64, 4)


def check_argument_errors(device):
    """The contract of the histogram, as the library on `device` states it (csrc/occl_math.hpp: one source for both libraries).
    Offsets handed over as a TENSOR that break the contract are not here: only a library that has them in host memory can
    reject them (tests/test_occl_host.py)."""
    rows = torch.zeros(10, 4, device=device)
    with pytest.raises(AssertionError, match='n_ids'):
        pk.ops.id_histogram(rows, 0, [0, 10], 0)
    with pytest.raises(AssertionError, match='n_ids'):
        pk.ops.id_histogram(rows, 0, [0, 10], 4097)
    with pytest.raises(AssertionError, match='col'):
        pk.ops.id_histogram(rows, 4, [0, 10], 4)
    with pytest.raises(AssertionError, match='pred_col'):
        pk.ops.id_histogram(rows, 0, [0, 10], 4, pred_col=4, pred_values=(1.0,))
    with pytest.raises(AssertionError, match='seg_offsets'):
        pk.ops.id_histogram(rows, 0, [0, 7, 3, 10], 4)
    with pytest.raises(AssertionError, match='seg_offsets'):
        pk.ops.id_histogram(rows, 0, [0, 9], 4)
    assert pk.ops.id_histogram(rows[:0], 0, [0], 4).shape == (0, 6)
    assert int(pk.ops.id_histogram(rows[:0], 0, [0, 0, 0], 4).sum()) == 0
