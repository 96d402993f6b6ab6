"""Measured returns carved into the query grid, on the device (include/ext/occ4d_evidence.h, ops.grid_carve, ops.grid_evidence):
what the sensors actually established about the scene, and how the completed field stands against it.

A measured return proves two things: the cells between the sensor and the return were empty, and the cell at the return was not.
Everything else is unknown -- and that is where the model completes amodally.  So, per cell of a point_sample_mode='grid' call:

    UNKNOWN_FREE 0     predicted air that no ray reached          COMPLETED 3         predicted solid that no ray reached
    CONFIRMED_FREE 1   predicted air a ray passed through         CONTRADICTED 4      predicted solid in measured free space
    MISSED 2           a return in predicted air                  CONFIRMED_SOLID 5   predicted solid with a return in it

code = STATE + 3 * SOLID with STATE = UNKNOWN 0 / FREE 1 / HIT 2 (a hit wins over grazing rays) and SOLID = density >= level (and
the optional select column): sight's member test.  The three counts an occlusion model is judged by -- hallucinations
(CONTRADICTED), misses (MISSED) and completions (COMPLETED) -- need no ground truth, per scene (totals, rates) and per object
(by_label), for CARLA as well as GREATER.

    carve      returns + sensor cells -> the passed bits, hits[, passes], status
    classify   a dense (N, G) array + those -> code (N,), totals (6,)
    observe    the stand-alone piece that runs both
    by_label   (K, 6) counts per component or segment
    rates      contradicted / missed / completed shares of totals, on the host
    Evidence   the option object of perform_inference(evidence=...) / evaluate_clip(evidence=..., evidences=[])

    res = perform_inference(..., point_sample_mode='grid', components=Components(), evidence=Evidence(points, lidar_positions, sensor=sweep_of_point))
    e = res['evidence']
    share = evidence.rates(e['totals'])                                # scene: contradicted, missed, completed
    per_object = evidence.by_label(labels, k, code)                    # (K, 6): row[COMPLETED] filled in, row[CONTRADICTED] refuted

The cell of a return is floorf((p - mins) / spacings) in float32 on the device, the cell that contains it; a sensor becomes its
cell on the host in float64 (sight.grid_origin): the same one approximation as sight's.  The walk from the return's cell to the
sensor's is sight's stepping without its solid test: a cell the segment touches only at an edge or a corner is not carved -- the
side the rule errs on is "unknown".  Integer marks, sums and ORs only: the same bits under any scheduling and any order of the
returns.

What it is NOT.  The returns are taken as given and are TIMELESS: in a moving scene the caller selects the rows of the frames that
bear on the output time, with torch, before the call; evaluate_clip applies one option to every output frame.  There is no sensor
noise model and no beam width.  Rays without a return (maximum range) are not carved.  A return outside the grid is dropped, even
when its ray crosses the grid (the header says why).  NOT MEASURED: how a trained model's shares come out.  There is no
checkpoint."""
import numpy as np
import torch

from . import _lib, ops, products, sight
from .projection import _device, _tensor

MAX_SENSORS = _lib.EVIDENCE_CONSTANTS['MAX_SENSORS']
MAX_COORD = _lib.EVIDENCE_CONSTANTS['MAX_COORD']
UNKNOWN, FREE, HIT = (_lib.EVIDENCE_CONSTANTS[k] for k in ('UNKNOWN', 'FREE', 'HIT'))
UNKNOWN_FREE, CONFIRMED_FREE, MISSED, COMPLETED, CONTRADICTED, CONFIRMED_SOLID = range(6)
CODES = ('UNKNOWN_FREE', 'CONFIRMED_FREE', 'MISSED', 'COMPLETED', 'CONTRADICTED', 'CONFIRMED_SOLID')
STATUS = ('carved', 'dropped_sensor', 'dropped_far', 'dropped_outside')


def _sensors(origins_ijk, who):
    """(V, 3) int32 numpy of integer lattice origins; ValueError unless 1 <= V <= 4096 and every coordinate is within 2^20."""
    o = np.asarray(origins_ijk)
    if o.ndim != 2 or o.shape[1] != 3 or o.dtype.kind not in 'iu':
        raise ValueError('%s: origins must be (V, 3) integers, got %s %s' % (who, o.dtype, o.shape))
    _count(o.shape[0], who)
    if np.abs(o.astype(np.int64)).max() > MAX_COORD:
        raise ValueError('%s: an origin lies beyond 2^20 cells' % who)
    return np.ascontiguousarray(o, dtype=np.int32)


def _count(V, who):
    if not 1 <= V <= MAX_SENSORS:
        raise ValueError('%s: V = %d sensors, must be in [1, %d]' % (who, V, MAX_SENSORS))


def _min_pass(min_pass, counts_too, who):
    if int(min_pass) != min_pass or int(min_pass) < 1:
        raise ValueError('%s: min_pass = %r must be an integer >= 1' % (who, min_pass))
    if int(min_pass) > 1 and not counts_too:
        raise ValueError('%s: min_pass = %d needs counts=True: the bits say only whether a ray passed' % (who, min_pass))
    return int(min_pass)


def carve(returns, origins_ijk, counts, mins, spacings, sensor=None, counts_too=False):
    """Measured returns carved into the (nx, ny, nz) = `counts` grid whose points ops.grid_points made from `mins` / `spacings`
    (geometry.grid_frame).  returns: (R, >= 3) float32 world points, a tensor on the device (a numpy array is uploaded); origins_ijk:
    (V, 3) integer lattice cells of the sensors on the host (sight.grid_origin), 1 <= V <= 4096, within 2^20 cells (ValueError) -- or
    an int32 (V, 3) tensor that is on the device already, taken as it is: the kernel checks its values, a return of a sensor out of
    range is dropped; sensor: (R,) integers, the sensor of every return, or None = sensor 0; counts_too: also count the walks per
    cell.  -> dict(passed (ceil(N / 32),) int32, hits (N,) int32[, passes (N,) int32], status (4,) int32 = [returns carved,
    dropped for the sensor, dropped as not finite / too far, dropped outside the grid]) on the device.  Nothing is read back."""
    device = _device(returns)
    ret = _tensor(returns, device, 'returns')
    if ret.dim() != 2 or ret.shape[1] < 3:
        raise ValueError('evidence.carve: returns must be (R, >= 3), got %s' % (tuple(ret.shape),))
    if isinstance(origins_ijk, torch.Tensor):
        org = origins_ijk
        if org.dim() != 2 or org.shape[1] != 3 or org.dtype != torch.int32:
            raise ValueError('evidence.carve: an origins tensor must be (V, 3) int32, got %s %s' % (org.dtype, tuple(org.shape)))
        _count(org.shape[0], 'evidence.carve')
        org = org.to(ret.device)
    else:
        org = torch.from_numpy(_sensors(origins_ijk, 'evidence.carve')).to(ret.device)
    sen = None
    if sensor is not None:
        sen = sensor if isinstance(sensor, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sensor, dtype=np.int32))
        if sen.dim() != 1 or sen.shape[0] != ret.shape[0] or sen.dtype.is_floating_point:
            raise ValueError('evidence.carve: sensor must be (%d,) integers, got %s %s' % (ret.shape[0], sen.dtype, tuple(sen.shape)))
        sen = sen.to(device=ret.device, dtype=torch.int32)
    passed, hits, passes, status = ops.grid_carve(ret, org, counts, mins, spacings, sen, counts_too)
    out = dict(passed=passed, hits=hits)
    if passes is not None:
        out['passes'] = passes
    out['status'] = status
    return out


def classify(implicit_output, level, carved, select=None, min_pass=1, channel=0):
    """implicit_output (N, G) dense on the grid `carved` was made for; its solid set column `channel` >= level (select = (column,
    threshold): the mask column), as sight.look; carved: carve()'s dict -- with 'passes' a cell is FREE from min_pass walks on, else
    from its bit of 'passed' (min_pass > 1 then: ValueError).  -> (code (N,) int32, totals (6,) int64 = the histogram of code) on
    the device.  Nothing is read back."""
    level = float(level)
    if level != level:
        raise ValueError('evidence.classify: level is NaN')
    min_pass = _min_pass(min_pass, 'passes' in carved, 'evidence.classify')
    values, mask, mask_level = products.columns(implicit_output, channel, sight._select(select, 'evidence.classify'))
    if 'passes' in carved:
        return ops.grid_evidence(values, level, carved['hits'], passes=carved['passes'], min_pass=min_pass, mask=mask, mask_level=mask_level)
    return ops.grid_evidence(values, level, carved['hits'], passed=carved['passed'], mask=mask, mask_level=mask_level)


def observe(implicit_output, counts, mins, spacings, returns, origins, sensor=None, level=0.5, select=None, counts_too=False, min_pass=1,
            channel=0):
    """The stand-alone piece: carve() then classify().  origins: (V, 3) WORLD points of the sensors, snapped to their cells by
    sight.grid_origin (ValueError beyond 2^20 cells).  -> dict(code (N,) int32, hits (N,) int32[, passes (N,) int32 with
    counts_too], totals (6,) int64, status (4,) int32) on the device: the product of Evidence.  Four launches, whatever the data;
    nothing is read back."""
    _min_pass(min_pass, counts_too, 'evidence.observe')
    origins_ijk = _sensors(sight.grid_origin(origins, mins, spacings), 'evidence.observe')
    device = _device(implicit_output)
    out = _tensor(implicit_output, device, 'implicit_output')
    return _product(out, counts, mins, spacings, returns, origins_ijk, sensor, level, select, counts_too, min_pass, channel)


def _product(out, counts, mins, spacings, returns, origins_ijk, sensor, level, select, counts_too, min_pass, channel=0):
    carved = carve(returns if isinstance(returns, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(returns, dtype=np.float32)).to(out.device),
                   origins_ijk, counts, mins, spacings, sensor, counts_too)
    code, totals = classify(out, level, carved, select, min_pass, channel)
    made = dict(code=code, hits=carved['hits'])
    if counts_too:
        made['passes'] = carved['passes']
    made['totals'], made['status'] = totals, carved['status']
    return made


def by_label(labels, k, code):
    """Per predicted object what the sensors say about it.  labels (N,) integers on the device: per query the number in [0, k) of
    its component or segment (components.label, watershed.split; anything else, like -1 = air, is left out); code (N,) of classify
    -> (k, 6) int64 on the device: per number the cells of each code.  row[COMPLETED] / row[3:].sum() is the share of the object
    that was filled in, row[CONTRADICTED] / row[3:].sum() the share the sensors refute.  torch operations only; nothing is read
    back."""
    k = int(k)
    lab = labels.to(torch.int64)
    slot = torch.where((lab >= 0) & (lab < k), lab * 6 + code.to(torch.int64), torch.full_like(lab, 6 * k))
    table = torch.zeros((6 * k + 1,), dtype=torch.int64, device=code.device)
    table.scatter_add_(0, slot, torch.ones_like(slot))
    return table[:6 * k].view(k, 6)


def rates(totals):
    """totals (6,) (or (..., 6): by_label's rows) -> dict(contradicted, missed, completed) of float64 on the host: contradicted =
    CONTRADICTED / predicted solid, missed = MISSED / cells with a hit, completed = COMPLETED / predicted solid; NaN where the
    denominator is 0."""
    t = totals.detach().cpu().numpy() if isinstance(totals, torch.Tensor) else np.asarray(totals)
    t = t.astype(np.float64)
    if t.shape[-1:] != (6,):
        raise ValueError('evidence.rates: totals must be (..., 6), got %s' % (t.shape,))
    solid, hit = t[..., 3:].sum(-1), t[..., MISSED] + t[..., CONFIRMED_SOLID]
    with np.errstate(all='ignore'):
        div = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
        return dict(contradicted=div(t[..., CONTRADICTED], solid), missed=div(t[..., MISSED], hit), completed=div(t[..., COMPLETED], solid))


class Evidence(products.LevelProduct):
    """The option object of perform_inference(evidence=...) / evaluate_clip(evidence=..., evidences=[]).  returns: (R, >= 3) world
    points of the measured returns, a float32 tensor (used where it is when it is on the call's device already) or numpy; origins:
    (V, 3) world points, the sensors' positions, one per sweep and view, 1 <= V <= 4096; sensor: (R,) integers, the sensor of every
    return, or None = sensor 0.  level: the density from which a query is solid (density >= level), None = the call's
    density_threshold; select = (column, threshold) or None: solid queries also need implicit_output[:, column] >= threshold;
    counts: also count the walks per cell; min_pass: a cell is FREE from that many walks on (> 1 needs counts=True: ValueError).
    The product: dict(code (N,) int32, hits (N,) int32[, passes (N,) int32], totals (6,) int64, status (4,) int32) (the module's
    doc-string); no device value is read.  All host work happens in prepare(), before the encode: the origins snapped to cells of
    the call's grid, ValueError for V or for an origin beyond 2^20 cells.  In track_mode 'all' the solid set is that of the merged
    array, under `refine` that of the expanded one.  THE RETURNS ARE TIMELESS: select the rows of the frames that bear on the
    output time before the call; evaluate_clip applies this one option to every output frame."""
    keyword, clip_list = 'evidence', ('evidences', 'one dict of code, hits[, passes], totals, status')

    def __init__(self, returns, origins, sensor=None, level=None, select=None, counts=False, min_pass=1):
        self.level, self.select, self.counts = self._level(level), sight._select(select, 'Evidence'), bool(counts)
        self.min_pass = _min_pass(min_pass, self.counts, 'Evidence')
        self.returns = returns if isinstance(returns, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(returns, dtype=np.float32))
        if self.returns.dim() != 2 or self.returns.shape[1] < 3 or self.returns.dtype != torch.float32:
            raise ValueError('Evidence: returns must be (R, >= 3) float32, got %s %s' % (self.returns.dtype, tuple(self.returns.shape)))
        self.origins = np.array(origins, np.float64)
        if self.origins.ndim != 2 or self.origins.shape[1] != 3:
            raise ValueError('Evidence: origins must be (V, 3) world points, got %s' % (self.origins.shape,))
        _count(self.origins.shape[0], 'Evidence')
        self.sensor = None
        if sensor is not None:
            s = sensor if isinstance(sensor, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sensor))
            if s.dim() != 1 or s.shape[0] != self.returns.shape[0] or s.dtype.is_floating_point:
                raise ValueError('Evidence: sensor must be (%d,) integers, got %s %s' % (self.returns.shape[0], s.dtype, tuple(s.shape)))
            self.sensor = s.to(torch.int32)

    def prepare(self, grid):
        return self.resolve(grid.density_threshold), _sensors(sight.grid_origin(self.origins, grid.mins, grid.spacings), 'Evidence')

    def run(self, grid, prepared, made):
        level, origins_ijk = prepared
        out = grid.output
        sensor = None if self.sensor is None else self.sensor.to(out.device)
        return _product(out, grid.counts, grid.mins, grid.spacings, self.returns.to(out.device), origins_ijk, sensor, level, self.select,
                        self.counts, self.min_pass)

    def __repr__(self):
        return 'Evidence(R=%d, V=%d, sensor=%s, level=%r, select=%r, counts=%r, min_pass=%r)' % (
            self.returns.shape[0], self.origins.shape[0], 'None' if self.sensor is None else '(R,)', self.level, self.select, self.counts,
            self.min_pass)
