"""Shortest free-space paths over the decoded occupancy on the dense query grid, on the device (include/ext/occ4d_geodesic.h): how
far it is from here to there WITHOUT passing through a predicted solid, and by which way -- from ONE decode, on the clearance of
distance.py.

perform_inference(clearance=Clearance(), route=Route(seeds, goals)) adds result['route'] = dict(cost (N,) int32, status (2,)
int32[, parent (N,) int32][, paths (G, cap) int32, path_len (G,) int32]): per query the least total step cost of a path from any
seed over queries whose clearance is >= min_clear (2^31 - 1: not passable, or no path), and for every goal the path back to a seed.

    route = Route(seeds=[[0.1, 0.2, 0.0]], goals=[[2.0, -1.5, 0.4]], min_clear=4)      # a robot of radius 2 grid steps
    res = perform_inference(..., point_sample_mode='grid', clearance=Clearance(), route=route)
    r = res['route']
    assert r['status'][0] == 1                                                          # converged: the costs are THE shortest
    way = paths_to_world(r['paths'], r['path_len'], mins, spacings, counts)[0]         # (L, 3), goal first

STEPS.  A move to a face, edge or corner neighbour costs an integer; the default (3, 4, 5) at connectivity 26 is the 3-4-5
chamfer metric (metric(cost, unit, 3) overestimates the Euclidean length of a free straight line by at most 8 %), (1, ., .) at
connectivity 6 counts steps.  Integers only: a converged result is the same bit for bit under any scheduling.

ROUNDS.  The kernel relaxes tile by tile, one launch per round; information crosses one tile border per round, so the rounds needed
are about the number of tile borders the longest shortest path crosses.  The default (ops.geodesic_default_rounds) is twice the sum
of the tile counts of the three axes, a heuristic; status[0] says whether it was enough, and solve(rounds=None) goes on in batches
until it is (one 8-byte read per batch).  Inside perform_inference nothing is read: check status[0] in the result.

WAYPOINTS.  A traced path is a staircase of face, edge and corner moves.  Route(..., pull=True) / solve(..., pull=True) / pull()
add waypoints (G, cap) int32 and waypoint_len (G,) int32 (include/ext/occ4d_pull.h): a subsequence of each path, goal first, whose
legs are straight segments over passable queries only -- the exact supercover walk of sight.py over the set dist2 < min_clear --
or single moves of the path; one more launch pair inside the same call, no host read.  One greedy pass from the goal, NOT the
Euclidean shortest path.  straight(clear, counts, a, b) is the pair test on its own; polyline_length measures either polyline."""
import numpy as np
import torch

from . import _lib, ops, products

NONE = _lib.GEODESIC_CONSTANTS['NONE']


def _steps(steps, who):
    try:
        s = tuple(steps)
    except TypeError:
        s = ()
    if len(s) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= 2 ** 31 - 1 for x in s):
        raise ValueError('%s: steps = %r must be three integers >= 1' % (who, steps))
    return tuple(int(x) for x in s)


def _connectivity(connectivity, who):
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError('%s: connectivity = %r must be 6, 18 or 26' % (who, connectivity))
    return int(connectivity)


def grid_index(points, mins, spacings, counts):
    """World points (S, 3) -> (S,) int64 flat indices of the cell-centred grid of geometry.grid_frame (query (ix, iy, iz) lies at
    mins + (i + 0.5) * spacings): the cell that contains the point, floor((p - mins) / spacings) in float64, x slowest and z
    fastest.  A point outside the grid (or not finite) raises ValueError."""
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError('grid_index: points must be (S, 3), got %s' % (p.shape,))
    counts = np.asarray([int(c) for c in counts], np.int64)
    g = np.floor((p - np.asarray(mins, np.float64)) / np.asarray(spacings, np.float64))
    bad = ~(np.isfinite(g).all(1) & (g >= 0).all(1) & (g < counts).all(1))
    if bad.any():
        raise ValueError('grid_index: point %d = %r lies outside the grid' % (int(np.flatnonzero(bad)[0]), p[np.flatnonzero(bad)[0]].tolist()))
    i = g.astype(np.int64)
    return (i[:, 0] * counts[1] + i[:, 1]) * counts[2] + i[:, 2]


def _indices(what, name):
    """seeds / goals as given -> ('flat', (S,) int32 numpy) or ('world', (S, 3) float64 numpy)."""
    a = np.asarray(what)
    if a.ndim == 2 and a.shape[1] == 3 and a.dtype.kind in 'fiu':
        return 'world', a.astype(np.float64)
    if a.ndim == 1 and (a.dtype.kind in 'iu' or a.size == 0):
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ValueError('Route: %s holds a value outside int32' % name)
        return 'flat', a.astype(np.int32)
    raise ValueError('Route: %s must be (S,) integer flat indices or (S, 3) world points, got shape %s of %s' % (name, a.shape, a.dtype))


class Route(products.GridProduct):
    """The option object of perform_inference(route=...) / evaluate_clip(route=..., routes=[]); needs `clearance`.  seeds, goals: (S,)
    integer flat indices of the query grid or (S, 3) world points (turned into indices on the host with grid_index before the decode;
    one outside the grid raises ValueError), goals None = no paths; min_clear: a query is passable when its clearance's dist2 >=
    min_clear; connectivity 6 / 18 / 26 and steps = (face, edge, corner) integer costs; rounds None = ops.geodesic_default_rounds;
    parent: also return each query's predecessor (goals imply it on the device); path_cap: the most points of a path, None = four
    times the longest axis; pull: also the paths pulled straight into waypoints (needs goals).  The product: dict(cost (N,) int32,
    status (2,) int32[, parent (N,) int32][, paths (G, cap) int32, path_len (G,) int32[, waypoints (G, cap) int32, waypoint_len
    (G,) int32]]) over that call's clearance dist2 (solve with rounds given): a fixed number of launches and no device value
    read, so status[0] == 1 -- the costs are converged, i.e. THE shortest -- has to be looked at."""
    keyword, clip_list = 'route', ('routes', 'one dict of costs and paths')
    needs = ('clearance', 'route needs clearance=<a distance.Clearance>: a query is passable when its dist2 >= route.min_clear')

    def __init__(self, seeds, goals=None, min_clear=1, connectivity=26, steps=(3, 4, 5), rounds=None, parent=False, path_cap=None,
                 pull=False):
        self.seeds = _indices(seeds, 'seeds')
        self.goals = None if goals is None else _indices(goals, 'goals')
        if isinstance(min_clear, bool) or not isinstance(min_clear, (int, np.integer)) or not -2 ** 31 <= min_clear <= 2 ** 31 - 1:
            raise ValueError('Route: min_clear = %r must be an int32' % (min_clear,))
        self.min_clear = int(min_clear)
        self.connectivity, self.steps = _connectivity(connectivity, 'Route'), _steps(steps, 'Route')
        if rounds is not None and (isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer))
                                   or not 0 <= rounds <= _lib.GEODESIC_CONSTANTS['MAX_ROUNDS']):
            raise ValueError('Route: rounds = %r must be None or an integer in [0, %d]' % (rounds, _lib.GEODESIC_CONSTANTS['MAX_ROUNDS']))
        self.rounds = None if rounds is None else int(rounds)
        if path_cap is not None and (isinstance(path_cap, bool) or not isinstance(path_cap, (int, np.integer)) or path_cap < 1):
            raise ValueError('Route: path_cap = %r must be None or an integer >= 1' % (path_cap,))
        self.parent, self.path_cap = bool(parent), None if path_cap is None else int(path_cap)
        if pull and goals is None:
            raise ValueError('Route: pull=True needs goals: the waypoints are those of the goals\' paths')
        self.pull = bool(pull)

    def resolve(self, counts, mins, spacings):
        """-> (seeds (S,) int32 numpy, goals (G,) int32 numpy or None, path cap) on this grid; ValueError for a world point outside."""
        def flat(which):
            kind, a = which
            return a if kind == 'flat' else grid_index(a, mins, spacings, counts).astype(np.int32)
        cap = self.path_cap if self.path_cap is not None else 4 * max(int(c) for c in counts)
        return flat(self.seeds), None if self.goals is None else flat(self.goals), cap

    def prepare(self, grid):
        return self.resolve(grid.counts, grid.mins, grid.spacings)

    def run(self, grid, on_grid, made):
        seeds, goals = (None if a is None else torch.from_numpy(a).to(grid.device) for a in on_grid[:2])
        rounds = ops.geodesic_default_rounds(grid.counts) if self.rounds is None else self.rounds
        return solve(made['clearance']['dist2'], grid.counts, seeds, goals, self.min_clear, self.connectivity, self.steps, rounds,
                     self.parent, on_grid[2], self.pull)

    def __repr__(self):
        return 'Route(seeds=<%s %s>, goals=%s, min_clear=%r, connectivity=%r, steps=%r, rounds=%r, parent=%r, path_cap=%r, pull=%r)' % (
            self.seeds[0], self.seeds[1].shape, None if self.goals is None else '<%s %s>' % (self.goals[0], self.goals[1].shape),
            self.min_clear, self.connectivity, self.steps, self.rounds, self.parent, self.path_cap, self.pull)


def solve(clear, counts, seeds, goals=None, min_clear=1, connectivity=26, steps=(3, 4, 5), rounds=None, parent=False, path_cap=None,
          pull=False):
    """The stand-alone piece.  clear (n,) int32 on the device (distance.transform's dist2), seeds / goals (S,) int32 flat indices on
    the device.  -> dict(cost, status[, parent][, paths, path_len[, waypoints, waypoint_len]]) on the device; pull=True (needs goals)
    adds the last two, pull() of the paths over the same clear and min_clear.
    rounds=None: batches of ops.geodesic_default_rounds(counts) rounds, the 8-byte status read after each, until a round changes
    nothing (at most one batch per tile: RuntimeError beyond); status[1] then counts the changing rounds of all batches.  rounds
    given: one call, NO host read -- look at status[0]."""
    connectivity, steps = _connectivity(connectivity, 'geodesic.solve'), _steps(steps, 'geodesic.solve')
    if pull and goals is None:
        raise ValueError('geodesic.solve: pull=True needs goals')
    want_parent = bool(parent) or goals is not None
    if rounds is not None:
        cost, status, up = ops.grid_geodesic(clear, counts, seeds, min_clear, connectivity, steps, rounds, want_parent)
    else:
        k = _lib.GEODESIC_CONSTANTS
        tiles = 1
        for c, t in zip(counts, ('TILE_X', 'TILE_Y', 'TILE_Z')):
            tiles *= max(1, -(-int(c) // k[t]))
        batch = max(1, ops.geodesic_default_rounds(counts))
        cost, changed = None, 0
        for _ in range(tiles + 1):
            cost, status, up = ops.grid_geodesic(clear, counts, seeds, min_clear, connectivity, steps, batch, want_parent, resume=cost)
            done, more = (int(v) for v in status.cpu())
            changed += more
            if done or cost.shape[0] == 0:
                break
        else:
            raise RuntimeError('geodesic.solve: not converged after %d batches of %d rounds' % (tiles + 1, batch))
        status = torch.tensor([1, changed], dtype=torch.int32, device=cost.device)
    result = dict(cost=cost, status=status)
    if parent:
        result['parent'] = up
    if goals is not None:
        cap = path_cap if path_cap is not None else 4 * max([int(c) for c in counts] + [1])
        result['paths'], result['path_len'] = ops.geodesic_trace(cost, up, goals, cap)
        if pull:
            result['waypoints'], result['waypoint_len'] = _pull_paths(clear, counts, result['paths'], result['path_len'], min_clear)
    return result


def straight(clear, counts, a, b, min_clear=1):
    """The stand-alone pair test.  clear (n,) int32 on the device, a, b (P,) int32 flat indices on the device, any values -> hit (P,)
    int32 on the device (HIT of include/ext/occ4d_pull.h): -1 where both ends are passable (clear >= min_clear) and the straight
    segment between their centres passes over passable queries only, -2 where an index is outside the grid, else the flat index of
    the first blocked query met from a (a or b itself when blocked).  hit == -1 is symmetric in a and b, the blocker is not.  Two
    launches, no host read."""
    return ops.grid_segments(ops.grid_blocked_bits(clear, min_clear), counts, a, b)


def pull(clear, counts, paths, path_len, min_clear=1):
    """paths (G, cap), path_len (G,) int32 on the device as solve(goals=...) returns them, over the same clear (n,) int32 and
    min_clear -> (waypoints (G, cap) int32, waypoint_len (G,) int32) on the device (PULL of include/ext/occ4d_pull.h): from the goal,
    always the farthest point of the path that the straight segment reaches over passable queries, or the next point of the path
    when there is none; -1 behind the waypoints; waypoint_len = path_len where that is <= 0.  One greedy pass, not the Euclidean
    shortest path.  Two launches, no host read."""
    return ops.geodesic_pull(ops.grid_blocked_bits(clear, min_clear), counts, paths, path_len)


_pull_paths = pull          # (solve's keyword `pull` hides the function's name there)


def metric(cost, unit=1.0, step=3):
    """cost * unit / step as float32 on cost's device (in float64, rounded once): the path length in world units when a face move
    of cost `step` is `unit` long; inf where cost is NONE."""
    assert cost.dtype == torch.int32, 'cost must be torch.int32, got %s' % (cost.dtype,)
    d = cost.to(torch.float64) * (float(unit) / float(step))
    return torch.where(cost == NONE, torch.full_like(d, float('inf')), d).to(torch.float32)


def paths_to_world(paths, path_len, mins, spacings, counts):
    """paths (G, cap), path_len (G,) as numpy arrays or tensors -> a list of G float64 (L, 3) arrays on the host: the centres of the
    path's queries, mins + (i + 0.5) * spacings, goal first; L = min(|path_len|, cap), 0 for an unreached goal."""
    paths = np.asarray(paths.cpu() if isinstance(paths, torch.Tensor) else paths)
    path_len = np.asarray(path_len.cpu() if isinstance(path_len, torch.Tensor) else path_len)
    nx, ny, nz = (int(c) for c in counts)
    mins, spacings = np.asarray(mins, np.float64), np.asarray(spacings, np.float64)
    out = []
    for row, length in zip(paths, path_len):
        p = row[:min(abs(int(length)), paths.shape[1])].astype(np.int64)
        i = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], -1) if len(p) else np.zeros((0, 3), np.int64)
        out.append(mins + (i + 0.5) * spacings)
    return out


def polyline_length(paths, path_len, spacings, counts):
    """paths (G, cap), path_len (G,) -- or waypoints, waypoint_len -- as numpy arrays or tensors -> (G,) float64 on the host: the
    Euclidean length in world units of the polyline through the centres of the row's path_len queries; 0 for a single point, nan
    for a row with path_len <= 0 (an unreached goal, a path longer than cap)."""
    paths = np.asarray(paths.cpu() if isinstance(paths, torch.Tensor) else paths)
    path_len = np.asarray(path_len.cpu() if isinstance(path_len, torch.Tensor) else path_len)
    out = np.full((len(path_len),), np.nan, np.float64)
    for g, way in enumerate(paths_to_world(paths, path_len, np.zeros(3), spacings, counts)):
        if int(path_len[g]) > 0:
            out[g] = np.sqrt((np.diff(way, axis=0) ** 2).sum(1)).sum()
    return out
