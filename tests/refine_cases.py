"""Shared by tests/test_refine_host.py (through the g++ twin) and tests/test_gpu_refine.py (on the device): the numpy restatement
of the coarse-to-fine decode's rules (include/occ4d_refine.h) -- the block of a point, the representative of a block, hot, the
clipped neighbourhood, selected, the expansion --, the case matrix of the two entry points, the expansion's guard, and the
end-to-end comparisons of perform_inference(refine=...) with the dense call on the tracking fixture.
Everything is compared EQUAL: the non-NaN elements bit for bit, the NaN positions as positions."""
import types

import numpy as np
import pytest
import torch

import inst_cases as ic
import track_cases as tc
import occlusions4d_amd as pk
from track_cases import same_bits, same_result

F32 = np.float32
GRIDS = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (9, 7, 5), (16, 16, 16), (17, 9, 33)]
LARGE_GRID = (65, 65, 65)             # 274 625 points = 1073 tiles of 256 rows: a second trip of the expansion's tile loop
BLOCKS = [2, 3, 4, 8]
DILATES = [0, 1, 2]
OPS = [0, 1, 2]
WIDTHS = [1, 5, 32]
PAD = 3                               # a strided array has ld = g + PAD
SENTINEL = 777.0
LOW = F32(0.46)
# the representatives' densities are drawn from this pool (raw values: under op 1 the +-100 saturate the sigmoid, +-0 give 0.5)
POOL = np.array([LOW, np.nextafter(LOW, F32(-1)), np.nextafter(LOW, F32(2)), 0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0,
                 -0.17, 0.3, 0.7, -3.0], dtype=F32)


# ---------------------------------------------------------------------------------------------------------------- restatement
def n_blocks(counts, b):
    return tuple(-(-n // b) for n in counts)


def representative_index(counts, b):
    """(nbx, nby, nbz) int64: the flat grid index of every block's representative."""
    nx, ny, nz = counts
    nbx, nby, nbz = n_blocks(counts, b)
    rep = np.zeros((nbx, nby, nbz), np.int64)
    for bx in range(nbx):
        for by in range(nby):
            for bz in range(nbz):
                ix, iy, iz = min(bx * b + b // 2, nx - 1), min(by * b + b // 2, ny - 1), min(bz * b + b // 2, nz - 1)
                rep[bx, by, bz] = (ix * ny + iy) * nz + iz
    return rep


def block_of_points(counts, b):
    """(nx * ny * nz,) int64: the flat block index of every grid point, x slowest, z fastest."""
    nbx, nby, nbz = n_blocks(counts, b)
    ix, iy, iz = np.indices(counts).reshape(3, -1)
    return ((ix // b) * nby + iy // b) * nbz + iz // b


def restate_mark(density, counts, b, dilate, low):
    """density (blocks,) float32, ALREADY squashed -> (active (blocks,) int32, key (n,) float32)."""
    nb = n_blocks(counts, b)
    with np.errstate(invalid='ignore'):
        hot = ~(np.asarray(density, F32).reshape(nb) < F32(low))
    active = np.zeros(nb, np.int32)
    for bx in range(nb[0]):
        for by in range(nb[1]):
            for bz in range(nb[2]):
                active[bx, by, bz] = hot[max(bx - dilate, 0):bx + dilate + 1, max(by - dilate, 0):by + dilate + 1,
                                         max(bz - dilate, 0):bz + dilate + 1].any()
    active = active.reshape(-1)
    selected = active[block_of_points(counts, b)] != 0
    selected[representative_index(counts, b).reshape(-1)] = False
    return active, selected.astype(F32)


def restate_expand(key, counts, b, rep_out, fine_out):
    """The dense (n, g) array: a selected row takes the next row of fine_out, every other row its block's row of rep_out."""
    selected = np.asarray(key) > 0.5
    out = np.array(rep_out[block_of_points(counts, b)], dtype=F32, copy=True)
    assert fine_out.shape[0] == int(selected.sum())
    out[selected] = fine_out
    return out


def restate_refine(dense, counts, b, dilate, low):
    """The contract on a dense call's (already squashed) implicit_output -> (expanded array, active, selected as bool)."""
    rep = representative_index(counts, b).reshape(-1)
    active, key = restate_mark(dense[rep, 0], counts, b, dilate, low)
    selected = key > 0.5
    return restate_expand(key, counts, b, dense[rep], dense[selected]), active, selected


# ---------------------------------------------------------------------------------------------------------------- entry points
def squashed(raw, op, device):
    """The library's own squash (occ4d_squash_f32) of a column: the yardstick compares what the mark's `op` must equal."""
    col = torch.from_numpy(np.ascontiguousarray(raw, dtype=F32)).to(device).view(-1, 1).clone()
    return pk.ops.squash(col, [op]).cpu().numpy().reshape(-1)


def densities(scenario, blocks, rng):
    if scenario == 'pool':
        d = POOL[rng.integers(0, len(POOL), size=blocks)]
        mix = rng.uniform(size=blocks) < 0.3
        d[mix] = rng.uniform(-1.0, 1.0, size=int(mix.sum())).astype(F32)
        return d
    if scenario == 'all_hot':
        return np.full(blocks, 0.9, F32)
    d = np.full(blocks, -2.0, F32)                      # 'no_hot': below LOW under every op
    if scenario == 'corner':
        d[blocks - 1] = 3.0                             # one hot block, the last corner (sigmoid(3) = 0.95, clamp 1)
    return d


def rows_on(device, n, g, strided, value_of_row):
    """(buffer, (n, ld) rows, (n, g) view) with row r, column c = value_of_row(r) * 32 + c and the padding a sentinel."""
    ld = g + PAD if strided else g
    rows = torch.full((n, ld), SENTINEL, dtype=torch.float32)
    rows[:, :g] = torch.from_numpy(np.asarray(value_of_row(np.arange(n, dtype=np.float64))[:, None] * 32
                                              + np.arange(g, dtype=np.float64)[None, :], dtype=F32))
    rows = rows.to(device)
    return rows, rows[:, :g]


def check_cell(device, counts, b, dilate, op, g, strided, scenario, rng):
    """One cell: mark, compaction, expansion against the restatement."""
    tag = (counts, b, dilate, op, g, strided, scenario)
    n = counts[0] * counts[1] * counts[2]
    blocks = int(np.prod(n_blocks(counts, b)))
    raw = densities(scenario, blocks, rng)
    # the mark reads a strided column when `strided`: the density column of (blocks, 3) rows
    holder = torch.full((blocks, 3 if strided else 1), SENTINEL, dtype=torch.float32)
    holder[:, 0] = torch.from_numpy(raw)
    holder = holder.to(device)
    key, active = pk.ops.refine_mark(holder[:, 0], counts, b, dilate, float(LOW), op=op)
    want_active, want_key = restate_mark(squashed(raw, op, device), counts, b, dilate, LOW)
    assert active.dtype == torch.int32 and np.array_equal(active.cpu().numpy(), want_active), tag
    assert same_bits(key.cpu().numpy(), want_key), tag
    if scenario == 'all_hot':
        assert want_active.all() and int(want_key.sum()) == n - blocks, tag
    elif scenario == 'no_hot':
        assert not want_active.any() and not want_key.any(), tag
    elif scenario == 'corner':
        assert want_active[-1] == 1 and 1 <= want_active.sum() <= (dilate + 1) ** 3, tag
    # the compaction of the grid's rows (here: the row number) with that key, and its offsets
    index_rows = torch.arange(n, dtype=torch.float32, device=device).view(n, 1)
    kept, n_fine, offsets = pk.ops.compact_rows_with_offsets(index_rows, key, 0.5)
    assert n_fine == int(want_key.sum()) and np.array_equal(kept.cpu().numpy()[:, 0], np.flatnonzero(want_key > 0.5)), tag
    # distinct sentinel rows: representative rows >= 0, decoded rows < 0
    rep_rows, rep_out = rows_on(device, blocks, g, strided, lambda r: r)
    fine_rows, fine_out = rows_on(device, n_fine, g, strided, lambda r: -(r + 1))
    out_rows = torch.full((n + 2, g + PAD if strided else g), SENTINEL, dtype=torch.float32, device=device)
    out = out_rows[1:n + 1, :g]                                       # a guard row in front and behind
    assert pk.ops.refine_expand(key, offsets, rep_out, fine_out if n_fine else None, counts, b, out=out) is out
    want = restate_expand(want_key, counts, b, rep_out.cpu().numpy(), fine_out.cpu().numpy())
    assert same_bits(np.ascontiguousarray(out.cpu().numpy()), want), tag
    host = out_rows.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[n + 1] == SENTINEL).all() and (host[:, g:] == SENTINEL).all(), tag
    assert (rep_rows.cpu().numpy()[:, g:] == SENTINEL).all() and (fine_rows.cpu().numpy()[:, g:] == SENTINEL).all(), tag


def cells_of(counts):
    return len(BLOCKS) * len(DILATES) * (len(OPS) * len(WIDTHS) * 2 + 3)


def check_matrix(counts, device):
    """Every cell of the matrix on one grid; returns the number of cells."""
    rng = np.random.default_rng(7000 + counts[0] * 10000 + counts[1] * 100 + counts[2])
    cells = 0
    for b in BLOCKS:
        for dilate in DILATES:
            for op in OPS:
                for g in WIDTHS:
                    for strided in (False, True):
                        check_cell(device, counts, b, dilate, op, g, strided, 'pool', rng)
                        cells += 1
            for scenario in ('all_hot', 'no_hot', 'corner'):
                check_cell(device, counts, b, dilate, (b + dilate) % 3, 5, bool(dilate % 2), scenario, rng)
                cells += 1
    return cells


def check_large(device):
    rng = np.random.default_rng(65)
    check_cell(device, LARGE_GRID, 3, 1, 1, 5, True, 'pool', rng)
    assert (LARGE_GRID[0] ** 3 + 255) // 256 > 1024


def check_expand_guard(device):
    """Offsets that point past n_fine, and n_fine = 0 with a null fine_out: the affected rows hold their representative's row,
    and no row outside `out` changes.  Nothing is provoked: fine_out is a window of a larger tensor whose other rows carry
    their own marker, so a read outside the window would show as a value."""
    counts, b, g = (9, 7, 5), 2, 5
    n = 9 * 7 * 5
    blocks = int(np.prod(n_blocks(counts, b)))
    key, active = pk.ops.refine_mark(torch.full((blocks,), 1.0, device=device), counts, b, 0, float(LOW))
    want_key = restate_mark(np.full(blocks, 1.0, F32), counts, b, 0, LOW)[1]
    n_sel = int(want_key.sum())
    assert n_sel == n - blocks and same_bits(key.cpu().numpy(), want_key)
    _, n_fine, offsets = pk.ops.compact_rows_with_offsets(torch.zeros((n, 1), device=device), key, 0.5)
    assert n_fine == n_sel and offsets.shape == (2,)
    _, rep_out = rows_on(device, blocks, g, False, lambda r: r)
    backing = torch.full((n_sel + 64, g), -5.0, dtype=torch.float32, device=device)       # -5: "read outside the window"
    window = backing[32:32 + n_sel]
    window.copy_(rows_on(device, n_sel, g, False, lambda r: -(r + 100))[1])
    rep_np, fine_np = rep_out.cpu().numpy(), window.cpu().numpy()
    blk = block_of_points(counts, b)
    selected = want_key > 0.5
    rank = np.cumsum(selected) - selected

    def expand(offs, n_given, fine):
        out_rows = torch.full((n + 2, g), SENTINEL, dtype=torch.float32, device=device)
        L = pk._lib.lib()
        rc = L.occ4d_refine_expand_f32(pk.ops._ptr(key), pk.ops._ptr(offs), pk.ops._ptr(rep_out), g, pk.ops._ptr(fine), g, n_given,
                                       counts[0], counts[1], counts[2], b, g, pk.ops._ptr(out_rows[1:]), g, pk.ops._stream())
        assert rc == pk._lib.OK, L.occ4d_last_error()
        host = out_rows.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[n + 1] == SENTINEL).all()
        return host[1:n + 1]

    first_of_tile = np.where(np.arange(n) < 256, 0, rank[256] if n > 256 else 0)

    def expected(offs, n_given):
        pos = np.asarray(offs, np.int64)[np.arange(n) // 256] + (rank - first_of_tile)
        ok = selected & (pos >= 0) & (pos < n_given)
        want = rep_np[blk].copy()
        want[ok] = fine_np[pos[ok]]
        return want, int(ok.sum())

    # (a) the true offsets, but only the first 100 decoded rows are declared: the rest take their representative
    want, inside = expected(offsets.cpu().numpy(), 100)
    got = expand(offsets, 100, window)
    assert inside == 100 and same_bits(got, want) and (got != -5.0).all()
    # (b) offsets past n_fine, negative, at the ends of int32, and shifted: a position outside [0, n_fine) is never read
    for pair, n_inside in (((n_sel, 10 ** 6), 0), ((-10 ** 6, -256), 0), ((2 ** 31 - 1, -2 ** 31), 0), ((n_sel - 7, -3), None)):
        offs = torch.tensor(pair, dtype=torch.int32, device=device)
        want, inside = expected(pair, n_sel)
        assert n_inside is None or inside == n_inside
        got = expand(offs, n_sel, window)
        assert same_bits(got, want) and (got != -5.0).all(), pair
        if n_inside == 0:
            assert same_bits(got, rep_np[blk])
    # (c) n_fine = 0 with a null fine_out, whatever the key says
    got = expand(offsets, 0, None)
    assert same_bits(got, rep_np[blk])
    assert (backing[:32] == -5.0).all() and (backing[32 + n_sel:] == -5.0).all()


def check_argument_errors(device):
    """The two contracts through the Python layer and the raw entry points, as the library on `device` states them."""
    z = lambda *shape, **k: torch.zeros(*shape, device=device, **k)
    mark, expand = pk.ops.refine_mark, pk.ops.refine_expand
    counts = (4, 4, 4)
    for b in (1, 9):
        with pytest.raises(AssertionError, match='b = %d' % b):
            mark(z(-(-4 // b) ** 3), counts, b, 0, 0.5)
    with pytest.raises(AssertionError, match='dilate = 3'):
        mark(z(8), counts, 2, 3, 0.5)
    with pytest.raises(AssertionError, match='op code 3'):
        mark(z(8), counts, 2, 1, 0.5, op=3)
    with pytest.raises(AssertionError, match='rep_density must be'):
        mark(z(7), counts, 2, 1, 0.5)
    key, offs = z(64), z(1, dtype=torch.int32)
    with pytest.raises(AssertionError, match='g = 33'):
        expand(key, offs, z(8, 33), None, counts, 2)
    with pytest.raises(AssertionError, match='rep_out must hold'):
        expand(key, offs, z(9, 5), None, counts, 2)
    with pytest.raises(AssertionError, match='out must be'):
        expand(key, offs, z(8, 5), None, counts, 2, out=z(64, 6))
    L, p = pk._lib.lib(), pk.ops._ptr
    EINVAL = pk._lib.EINVAL
    assert L.occ4d_refine_mark_f32(p(z(8)), 1, -1, 4, 4, 2, 0, 0, 0.5, p(z(8, dtype=torch.int32)), p(z(64)), None) == EINVAL
    assert L.occ4d_refine_mark_f32(None, 1, 4, 4, 4, 2, 0, 0, 0.5, p(z(8, dtype=torch.int32)), p(z(64)), None) == EINVAL
    assert L.occ4d_refine_mark_f32(p(z(8)), 0, 4, 4, 4, 2, 0, 0, 0.5, p(z(8, dtype=torch.int32)), p(z(64)), None) == EINVAL
    assert L.occ4d_refine_mark_f32(p(z(8)), 1, 65536, 65536, 1, 2, 0, 0, 0.5, p(z(8, dtype=torch.int32)), p(z(64)), None) == EINVAL
    assert b'INT32_MAX' in L.occ4d_last_error()
    assert L.occ4d_refine_expand_f32(p(key), p(offs), p(z(8, 5)), 4, None, 5, 0, 4, 4, 4, 2, 5, p(z(64, 5)), 5, None) == EINVAL
    assert L.occ4d_refine_expand_f32(p(key), p(offs), p(z(8, 5)), 5, None, 5, 3, 4, 4, 4, 2, 5, p(z(64, 5)), 5, None) == EINVAL
    assert b'null fine_out' in L.occ4d_last_error()
    assert L.occ4d_refine_expand_f32(p(key), p(offs), p(z(8, 5)), 5, None, 5, 0, 4, 4, 4, 2, 0, p(z(64, 5)), 5, None) == EINVAL
    assert L.occ4d_refine_mark_f32(None, 1, 0, 4, 4, 2, 0, 0, 0.5, None, None, None) == pk._lib.OK            # an empty grid
    assert L.occ4d_refine_expand_f32(None, None, None, 5, None, 5, 0, 4, 0, 4, 2, 5, None, 5, None) == pk._lib.OK


# ---------------------------------------------------------------------------------------------------------------- end to end
CASE = tc.CASE                        # 768 points; the grid is 14 x 14 x 9 = 1764 queries, 7 x 7 x 5 = 245 blocks of edge 2
COUNTS, N_QUERIES, N_BLOCKS = (14, 14, 9), 1764, 245


def infer(device, inputs, track_mode='none', **kw):
    pcl, sem, target, inf, enc, dec = inputs
    kw.setdefault('point_sample_mode', 'grid')
    return pk.inference.perform_inference(
        pcl.clone(), sem.copy() if track_mode != 'none' else None, target.copy(), [enc, dec], device, 'if', inf['min_z'],
        inf['cube_bounds'], inf['color_mode'], CASE['time_idx'], None, sample_implicit=True, num_sample=CASE['num_sample'],
        batch_size=CASE['batch_size'], predict_segmentation=False, track_mode=track_mode, semantic_classes=13,
        density_threshold=0.5, data_kind='greater', cube_mode=4, compress_air=True, point_occupancy_radius=0.8, **kw)


class Shared:
    """The inputs and the dense calls of one device: computed once per module, never changed."""

    def __init__(self, device):
        self.device = device
        self.inputs = tc.nets(device)
        pcl, sem, target, inf, enc, dec = self.inputs
        assert pk.geometry.grid_counts(CASE['num_sample'], inf['min_z'], inf['cube_bounds'], 'greater', 4) == COUNTS
        self.dense = infer(device, self.inputs)
        self.dense_all = infer(device, self.inputs, track_mode='all')


def clip_inputs(shared, n_frames=2):
    """The clip the check_clip of every cases module runs evaluate_clip over -> (frames, batch, args): the target frame, its first
    257 rows scaled by a half and, as a third frame, the target again."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames = [target, target[:257] * F32(0.5), target][:n_frames]
    batch = dict(pcl_input=pcl, pcl_input_sem=torch.from_numpy(sem)[None], pcl_target=[torch.from_numpy(f)[None] for f in frames],
                 meta_data=dict(pcl_target_size=[torch.tensor([f.shape[0]]) for f in frames]))
    args = types.SimpleNamespace(min_z=inf['min_z'], cr_cube_bounds=inf['cube_bounds'], color_mode=inf['color_mode'],
                                 sample_implicit=True, num_sample=CASE['num_sample'], point_sample_mode='grid',
                                 implicit_batch_size=CASE['batch_size'], segmentation_lw=0.0, track_mode='none',
                                 point_occupancy_radius=0.8, semantic_classes=13, density_threshold=0.5, cube_mode=4)
    return frames, batch, args


def count_waits(monkeypatch):
    """Counts the host waits of the calls that follow -> the dict whose 'wait' counts them (monkeypatch.undo() ends the count)."""
    calls = dict(wait=0)
    wait = pk.inference._HostCopies.wait

    def counted_wait(self):
        calls['wait'] += 1
        return wait(self)
    monkeypatch.setattr(pk.inference._HostCopies, 'wait', counted_wait)
    return calls


def check_single_run(shared, dilate):
    """track_mode 'none' with GridRefine(2, 0.46, dilate) against the restatement applied to the dense call's output."""
    dense = shared.dense
    assert dense['implicit_output'].shape == (N_QUERIES, 5) and 'refine' not in dense
    want, active, selected = restate_refine(dense['implicit_output'], COUNTS, 2, dilate, 0.46)
    assert 0 < active.sum() < N_BLOCKS, active.sum()                 # the fixture's condition
    got = infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, dilate))
    assert got['refine'] == dict(n_queries=N_QUERIES, n_decoded=N_BLOCKS + int(selected.sum()))
    assert got['refine']['n_decoded'] < N_QUERIES and all(type(v) is int for v in got['refine'].values())
    assert same_bits(got['implicit_output'], want)
    assert sorted(got) == sorted(list(dense) + ['refine'])
    for k in ('points_query', 'pcl_abstract', 'features_global'):
        assert same_bits(got[k], dense[k]), k
    # the solid rows: the restatement's, and a subset of the dense call's in the same order
    solid = want[:, 0] >= F32(0.5)
    assert same_bits(got['output_solid'], np.concatenate([dense['points_query'], want], axis=1)[solid])
    dense_solid = dense['implicit_output'][:, 0] >= F32(0.5)
    assert not (solid & ~dense_solid).any()
    keep = solid[dense_solid]
    assert same_bits(got['output_solid'], dense['output_solid'][keep])
    assert got['output_air'].shape[0] == N_QUERIES - int(solid.sum()) and got['gt_solid'].shape[0] == int(solid.sum())
    return active


def check_low_extremes(shared):
    """low = 0: every block is active and the result is the dense one bit for bit; low = 2: no block is, 245 rows are decoded
    and every row is its representative's copy."""
    dense = shared.dense
    got = infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.0, 0))
    assert got.pop('refine') == dict(n_queries=N_QUERIES, n_decoded=N_QUERIES)
    same_result(got, dense)
    got = infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 2.0, 2))
    assert got['refine'] == dict(n_queries=N_QUERIES, n_decoded=N_BLOCKS)
    rep = representative_index(COUNTS, 2).reshape(-1)
    assert same_bits(got['implicit_output'], dense['implicit_output'][rep][block_of_points(COUNTS, 2)])
    want, active, selected = restate_refine(dense['implicit_output'], COUNTS, 2, 2, 2.0)
    assert not active.any() and not selected.any() and same_bits(got['implicit_output'], want)


def check_track_all(shared):
    """track_mode 'all': the device merge equals the host merge under the same refine, and low = 0 equals the dense 'all' call."""
    refine = pk.inference.GridRefine(2, 0.46, 1)
    on_device = infer(shared.device, shared.inputs, track_mode='all', refine=refine, track_merge='device')
    on_host = infer(shared.device, shared.inputs, track_mode='all', refine=refine, track_merge='host')
    assert on_device['refine'] == on_host['refine'] and on_device['refine']['n_queries'] == 3 * N_QUERIES
    assert 3 * N_BLOCKS < on_device['refine']['n_decoded'] < 3 * N_QUERIES
    for r in (on_device, on_host):
        r.pop('refine')
    same_result(on_device, on_host)
    full = infer(shared.device, shared.inputs, track_mode='all', refine=pk.inference.GridRefine(2, 0.0, 1))
    assert full.pop('refine') == dict(n_queries=3 * N_QUERIES, n_decoded=3 * N_QUERIES)
    same_result(full, shared.dense_all)


def check_scorers(shared):
    """stats= / inst_stats= with refine: the scorers see the expanded array -- they equal the same scorers fed with the returned
    arrays."""
    device = shared.device
    target = shared.inputs[2]
    inf = shared.inputs[3]
    refine = pk.inference.GridRefine(2, 0.46, 1)
    stats, inst = pk.evaluation.EvalStats(1, 0, device), pk.evaluation.InstanceStats(ic.E2E_IDS, 1, device)
    res = infer(device, shared.inputs, track_mode='all', refine=refine, stats=stats, inst_stats=inst)
    assert not same_bits(res['implicit_output'], shared.dense_all['implicit_output'])      # (the scorers are fed something else)
    stats2, inst2 = pk.evaluation.EvalStats(1, 0, device), pk.evaluation.InstanceStats(ic.E2E_IDS, 1, device)
    stats2.add_frame(res['points_query'], res['implicit_output'], target, density_threshold=0.5, point_occupancy_radius=0.8,
                     color_mode=inf['color_mode'], predict_segmentation=False, track_mode='all', data_kind='greater')
    inst2.add_frame(res['points_query'], res['implicit_output'], target, density_threshold=0.5, point_occupancy_radius=0.8,
                    color_mode=inf['color_mode'], data_kind='greater')
    assert stats.counts.sum() > 0 and torch.equal(stats.counts, stats2.counts) and torch.equal(stats.sums, stats2.sums)
    assert torch.equal(inst.counts, inst2.counts) and torch.equal(inst.sums, inst2.sums) and torch.equal(inst.frame, inst2.frame)


def check_clip(shared):
    """evaluate_clip(refine=...) over two frames = two perform_inference calls."""
    device = shared.device
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = clip_inputs(shared)
    refine = pk.inference.GridRefine(2, 0.46, 1)
    clip =pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, refine=refine)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == 2
    for t, frame in enumerate(frames):
        res = pk.inference.perform_inference(
            pcl.clone(), None, frame, [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=CASE['num_sample'], point_sample_mode='grid', batch_size=CASE['batch_size'],
            predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater',
            cube_mode=4, compress_air=True, point_occupancy_radius=0.8, refine=refine)
        assert len(clip[t]) == 7
        for got, want in zip(clip[t], (pcl[0].numpy(), res['pcl_abstract'], res['output_solid'], frame, res['output_air'], sem,
                                       res['points_query'])):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert clip[t][2].shape[0] <= dense[t][2].shape[0] and res['refine']['n_decoded'] < N_QUERIES


def check_none_is_untouched(shared, monkeypatch):
    """refine=None: the result keys and the one host wait are what they were; the refinement's entry points are never called."""
    calls = count_waits(monkeypatch)
    calls['refine'] = 0

    def counted(*a, **k):
        calls['refine'] += 1
        raise AssertionError('refine=None must not reach the refinement')
    for name in ('refine_mark', 'refine_expand', 'compact_rows_with_offsets'):
        monkeypatch.setattr(pk.ops, name, counted)
    res = infer(shared.device, shared.inputs, refine=None)
    assert calls == dict(wait=1, refine=0)
    assert sorted(res) == ['features_global', 'gt_air', 'gt_solid', 'implicit_output', 'output_air', 'output_solid', 'pcl_abstract',
                           'points_query']
    same_result(res, shared.dense)
    monkeypatch.undo()
    calls = count_waits(monkeypatch)
    infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1))
    assert calls['wait'] == 1                                          # (the refinement adds a count read, not a wait on the copies)


def check_value_errors(shared):
    refine = pk.inference.GridRefine(2, 0.46, 1)
    with pytest.raises(ValueError, match='grid'):
        infer(shared.device, shared.inputs, refine=refine, point_sample_mode='random')
    lists = (np.zeros((N_QUERIES, 8), np.int64), None)
    with pytest.raises(ValueError, match='neighbour_lists'):
        infer(shared.device, shared.inputs, refine=refine, neighbour_lists=lists)
    with pytest.raises(ValueError):
        infer(shared.device, shared.inputs, refine=(2, 0.46, 1))
