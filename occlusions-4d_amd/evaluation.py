"""Per-clip evaluation loop and its on-disk contract.

Interface mirror of the body of the reference's eval/test.py:test (:31-135): for one data-loader batch (one clip),
every output frame is decoded by ``inference.perform_inference`` with the reference's arguments and the results are
collected as the list the downstream visualisation reads (utils/utils.py:400-479):

    pcl_all[time_idx] = (pcl_input (N,8), pcl_abstract (M,3+E), output_solid (S,4+G), pcl_target_frame (T,9-11),
                         output_air (A,5))                                  [+ (pcl_input_sem, points_query) with save_gt]

written as ``<log_dir>/test_<tag>/pcl_io_s<step>.p`` with ``pickle.dump`` (utils/logvis.py:222-234), next to
``metadata_s<step>.p`` = (meta_data, cam_RT, cam_K).  The published eval/test.py reads ``args.save_gt``, which no
parser defines; here it is an explicit argument, default False.

One difference that does not change results: the reference re-encodes the same input cloud for every output frame
(:67-86); the encode is deterministic, so it is done once per clip and shared (``reuse_encode=False`` restores the
per-frame encode; it is also what happens, automatically, for an encoder built with fps_random_start=True).
"""
import os
import pickle

import numpy as np
import torch

from . import _lib
from . import components as components_mod
from . import distance as distance_mod
from . import geodesic as geodesic_mod
from . import watershed as watershed_mod
from . import sight as sight_mod
from . import inference
from . import ops
from . import products
from . import projection
from . import surface as surface_mod
from . import sweep as sweep_mod
from . import evidence as evidence_mod

_EC = _lib.EVAL_CONSTANTS
# target columns (R; G, B follow / mark_track / semantic tag, -1 = absent) of the two data kinds (eval/inference.py:96):
# GREATER rows are (x, y, z, instance, view, R, G, B, mark_track), CARLA rows (x, y, z, cosine, instance, semantic, view,
# R, G, B, mark_track)
TARGET_COLUMNS = {'greater': dict(col_rgb=5, col_track=8, col_sem=-1), 'carla': dict(col_rgb=7, col_track=10, col_sem=5)}
# target column of the instance id of the two data kinds (the rows above).  A table of its own: the dicts of TARGET_COLUMNS are
# splatted into ops.eval_query_stats
INSTANCE_COLUMNS = {'greater': 3, 'carla': 4}
_IC = _lib.INST_CONSTANTS
_INST_COUNT_NAMES = ('N_GT', 'N_PRED', 'N_MATCH', 'SUM_INTER', 'SUM_UNION', 'N_CENTROID')
_COUNT_NAMES = ('OCC_TP', 'OCC_FP', 'OCC_FN', 'OCC_TN', 'TRACK_TP', 'TRACK_FP', 'TRACK_FN', 'TRACK_TN', 'SEG_IGNORED',
                'N_ACCURACY', 'N_COMPLETENESS', 'N_COLOR', 'N_SEG')


def _ratio(num, den):
    """num / den element-wise in float64, nan where den == 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den != 0)


class _AdditiveStats:
    """What EvalStats and InstanceStats share: two device accumulators, `counts` (int64) and `sums` (float64), that sum across
    frames, clips and ranks, their numpy state, their one-transfer read and the inputs of an `add_frame`.  A subclass names its
    constructor arguments in order (_FIELDS: the state's keys) and those that size the two arrays (_LAYOUT_FIELDS: objects of
    one class that agree on these add)."""
    _FIELDS = _LAYOUT_FIELDS = ()

    def _allocate(self, device, n_counts, n_sums):
        self.device = torch.device('cpu' if _lib.is_twin() else 'cuda') if device is None else torch.device(device)
        self.counts = torch.zeros((n_counts,), dtype=torch.int64, device=self.device)
        self.sums = torch.zeros((n_sums,), dtype=torch.float64, device=self.device)

    def _tensor(self, a, dtype=torch.float32):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=self.device, dtype=dtype)

    def _frame_inputs(self, points_query, implicit_output, target_rows):
        """The three arrays of an add_frame on the device, checked: q (N, 3 or 4), out (N, G), tgt (M, Dt)."""
        q, out, tgt = self._tensor(points_query), self._tensor(implicit_output), self._tensor(target_rows)
        assert q.dim() == 2 and q.shape[1] in (3, 4) and out.dim() == 2 and out.shape[0] == q.shape[0], 'points_query (N, 3 or 4), implicit_output (N, G)'
        assert tgt.dim() == 2 and tgt.shape[0] >= 1 and tgt.shape[1] >= 3, 'target_rows must be (M >= 1, Dt >= 3)'
        return q, out, tgt

    def _frame_search(self, q, tgt, nn, group):
        """(idx (N,) int32, dist (N,), grp) on the device: the query -> target 1-NN (searched unless the caller has it as `nn`)
        and the group ids, or None when there is no query: nothing to add, and nothing is searched."""
        grp = None if group is None else self._tensor(np.asarray(group) if not torch.is_tensor(group) else group,
                                                      torch.int32).contiguous()
        if q.shape[0] == 0:
            return None
        if nn is None:
            idx, dist = ops.knn(q[:, :3], tgt[:, :3], 1, metric=1, return_dist=True)
            nn = (idx[:, 0], dist[:, 0])
        return self._tensor(nn[0], torch.int32), self._tensor(nn[1]), grp

    @staticmethod
    def _split_solid(q, values, density_threshold):
        """The predicted-solid rows (xyz, t, then `values`' columns) when the caller has not split them."""
        q4 = q if q.shape[1] == 4 else torch.nn.functional.pad(q, (0, 1))
        return ops.split_solid_air(q4.contiguous(), values, density_threshold)[0]

    def _same_layout(self, other):
        assert type(other) is type(self) and all(getattr(other, f) == getattr(self, f) for f in self._LAYOUT_FIELDS), \
            '%s of different %s do not add' % (type(self).__name__, ' / '.join(self._LAYOUT_FIELDS))

    def merge(self, other):
        self._same_layout(other)
        self.counts += other.counts.to(self.device)
        self.sums += other.sums.to(self.device)
        return self

    __iadd__ = merge

    def all_reduce(self, group=None):
        """torch.distributed SUM over both arrays (the same layout on every rank)."""
        import torch.distributed as dist
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)
        return self

    def state(self):
        """The object as numpy (copies: a later add does not change them); from_state() is the way back."""
        return dict({f: getattr(self, f) for f in self._FIELDS}, counts=self.counts.cpu().numpy().copy(),
                    sums=self.sums.cpu().numpy().copy())

    @classmethod
    def from_state(cls, state, device=None):
        self = cls(*(int(state[f]) for f in cls._FIELDS), device)
        counts, sums = np.asarray(state['counts'], np.int64), np.asarray(state['sums'], np.float64)
        assert counts.shape == tuple(self.counts.shape) and sums.shape == tuple(self.sums.shape)
        self.counts.copy_(torch.from_numpy(counts))
        self.sums.copy_(torch.from_numpy(sums))
        return self

    def _read(self):
        """(counts, sums) as numpy from ONE transfer (the int64 words travel reinterpreted as float64 bits)."""
        both = torch.cat([self.counts.view(torch.float64), self.sums]).cpu()
        return both[:self.counts.numel()].view(torch.int64).numpy(), both[self.counts.numel():].numpy()


class EvalStats(_AdditiveStats):
    """Additive evaluation statistics of decoded frames against their ground-truth frames (include/occ4d_eval.h): two device
    arrays, `counts` (int64) and `sums` (float64), that `add_frame` accumulates onto with no host read of their contents,
    that sum across frames, clips and ranks (`merge`, `+=`, `all_reduce`) and that `summary()` turns into the usual figures
    with ONE host read.  Every statistic is kept per group (n_groups <= 8: the caller's partition of the target points,
    e.g. visible / occluded); semantic_classes (<= 32) sizes the segmentation confusion matrix, 0 = none.
    In track_mode 'all' the TRACK_* counts compare a winner id with 0.5 and mean nothing: InstanceStats is the scorer for that
    mode."""

    _FIELDS = _LAYOUT_FIELDS = ('n_groups', 'semantic_classes')

    def __init__(self, n_groups=1, semantic_classes=0, device=None):
        self.n_groups, self.semantic_classes = int(n_groups), int(semantic_classes)
        self._allocate(device, *ops.eval_layout(self.n_groups, self.semantic_classes))

    def add_frame(self, points_query, implicit_output, target_rows, *, density_threshold, point_occupancy_radius, color_mode,
                  predict_segmentation, track_mode, data_kind, target_group=None, nn=None, solid=None, col_rgb=None,
                  col_track=None, col_sem=None):
        """Adds one output frame: points_query (N, 3 or 4), implicit_output (N, G) (squashed, as perform_inference returns it),
        target_rows (M, Dt) (device tensors or numpy, uploaded once).  target_group: (M,) integer group id per target point.
        nn = (idx (N,), dist (N,)): the query -> target 1-NN if the caller has it; solid: the predicted-solid rows
        (xyz first) if the caller has split them.  The target columns default from data_kind (TARGET_COLUMNS).  Colour is
        scored for color_mode 'rgb' / 'rgb_nosigmoid', tracking for track_mode != 'none', segmentation for
        predict_segmentation with semantic_classes > 0 and a semantic column."""
        q, out, tgt = self._frame_inputs(points_query, implicit_output, target_rows)
        cols = dict(TARGET_COLUMNS.get(data_kind, dict(col_rgb=-1, col_track=-1, col_sem=-1)))
        cols.update({k: int(v) for k, v in dict(col_rgb=col_rgb, col_track=col_track, col_sem=col_sem).items() if v is not None})
        flags = 0
        if color_mode in ('rgb', 'rgb_nosigmoid'):
            flags |= _EC['FLAG_COLOR']
        if track_mode != 'none':
            flags |= _EC['FLAG_TRACK']
        if predict_segmentation and self.semantic_classes > 0:
            flags |= _EC['FLAG_SEG']
        found = self._frame_search(q, tgt, nn, target_group)
        if found is None:
            return self
        idx, dist, grp = found
        kw = dict(n_groups=self.n_groups, n_classes=self.semantic_classes, target_group=grp)
        solid = self._tensor(self._split_solid(q, out, density_threshold) if solid is None else solid)
        if solid.shape[0] > 0:               # completeness: every target point to its nearest predicted-solid query
            _, back = ops.knn(tgt[:, :3], solid[:, :3], 1, metric=1, return_dist=True)
            ops.eval_target_stats(back[:, 0], self.counts, self.sums, **kw)
        ops.eval_query_stats(out, idx, dist, tgt, self.counts, self.sums, density_threshold=density_threshold,
                             radius=point_occupancy_radius, flags=flags, out_track=inference.get_track_idx(color_mode), **cols, **kw)
        return self

    def summary(self):
        """The figures per group, as float64 arrays of shape (n_groups,) (nan where the denominator is 0), from one host read:
        precision, recall, f1, iou (occupancy, prediction against the 1-NN label); chamfer_accuracy (mean nn distance of
        the predicted-solid queries), chamfer_completeness (mean distance of the target points to the nearest predicted-
        solid query), chamfer (their sum) and chamfer_*_sq / chamfer_sq on squared distances; seg_accuracy, seg_miou (over
        the classes that occur as a row or a column of the confusion matrix); track_iou; color_l1 (mean |dR| + |dG| + |dB|).
        'counts': the raw counts by name ((n_groups,) int64 each), 'confusion' (n_groups, C, C), 'bad_rows'.  Raises
        ValueError when rows were skipped (bad_rows > 0)."""
        G, C, K = self.n_groups, self.semantic_classes, _EC['GROUP_COUNTS']
        counts, sums = self._read()
        bad = int(counts[_EC['BAD_ROWS']])
        if bad > 0:
            raise ValueError('EvalStats: %d rows were skipped (nn_idx outside the target, or a group id outside [0, %d))' % (bad, G))
        per = counts[_EC['HEAD']:].reshape(G, K + C * C)
        c = {name.lower(): per[:, _EC[name]].copy() for name in _COUNT_NAMES}
        conf = per[:, K:].reshape(G, C, C).copy()
        s = sums.reshape(G, _EC['GROUP_SUMS'])
        tp, fp, fn = c['occ_tp'], c['occ_fp'], c['occ_fn']
        res = dict(precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), f1=_ratio(2 * tp, 2 * tp + fp + fn),
                   iou=_ratio(tp, tp + fp + fn))
        res['chamfer_accuracy'] = _ratio(s[:, _EC['SUM_ACCURACY_D']], c['n_accuracy'])
        res['chamfer_completeness'] = _ratio(s[:, _EC['SUM_COMPLETENESS_D']], c['n_completeness'])
        res['chamfer'] = res['chamfer_accuracy'] + res['chamfer_completeness']
        res['chamfer_accuracy_sq'] = _ratio(s[:, _EC['SUM_ACCURACY_D2']], c['n_accuracy'])
        res['chamfer_completeness_sq'] = _ratio(s[:, _EC['SUM_COMPLETENESS_D2']], c['n_completeness'])
        res['chamfer_sq'] = res['chamfer_accuracy_sq'] + res['chamfer_completeness_sq']
        diag = np.einsum('gcc->gc', conf)
        union = conf.sum(axis=2) + conf.sum(axis=1) - diag
        res['seg_accuracy'] = _ratio(diag.sum(axis=1), conf.sum(axis=(1, 2)))
        res['seg_miou'] = _ratio(np.where(union > 0, _ratio(diag, union), 0.0).sum(axis=1), (union > 0).sum(axis=1))
        res['track_iou'] = _ratio(c['track_tp'], c['track_tp'] + c['track_fp'] + c['track_fn'])
        res['color_l1'] = _ratio(s[:, _EC['SUM_COLOR_L1']], c['n_color'])
        res.update(counts=c, confusion=conf, bad_rows=bad)
        return res


class InstanceStats(_AdditiveStats):
    """Additive instance-level statistics of a dense instance labelling (perform_inference with track_mode 'all': the merged
    mark_track channel holds the id of the most confident rerun, or -1) against ground-truth frames (include/occ4d_inst.h): per
    frame a device table -- the (n_ids + 1)^2 confusion of ALL queries, class n_ids = none, and per id the count and the
    fixed-point coordinate sums of the predicted-solid rows and of the target points -- that `add_frame` fills and folds onto
    `counts` (int64) and `sums` (float64) with no host read.  The two arrays sum across frames, clips and ranks (`merge`, `+=`,
    `all_reduce`); `summary()` turns them into instance IoU, panoptic quality and the centroid error with ONE host read, and
    `frame_tables()` reads the latest frame's table: where every tracked object is.  Every figure is kept per group
    (n_groups <= 8: the caller's partition of the ids, e.g. `occlusion_groups`); n_ids <= 64.  A sibling of EvalStats, whose
    TRACK_* counts mean nothing for a winner id.  The frame table is not part of `state()`; the lengths of `counts` and `sums`
    depend on n_groups alone (ops.inst_layout), so objects of different n_ids add."""
    _FIELDS, _LAYOUT_FIELDS = ('n_ids', 'n_groups'), ('n_groups',)

    def __init__(self, n_ids, n_groups=1, device=None):
        self.n_ids, self.n_groups = int(n_ids), int(n_groups)
        n_frame, n_counts, n_sums = ops.inst_layout(self.n_ids, self.n_groups)
        self._allocate(device, n_counts, n_sums)
        self.frame = torch.zeros((n_frame,), dtype=torch.int64, device=self.device)

    def add_frame(self, points_query, implicit_output, target_rows, *, density_threshold, point_occupancy_radius, color_mode,
                  data_kind, inst_group=None, nn=None, solid=None, col_inst=None, pred_id=None):
        """Adds one output frame: points_query (N, 3 or 4), implicit_output (N, G) (squashed and merged, as perform_inference
        returns it), target_rows (M, Dt) (device tensors or numpy, uploaded once).  inst_group: (n_ids,) integer group id per
        instance id.  nn = (idx (N,), dist (N,)): the query -> target 1-NN if the caller has it; solid: the predicted-solid rows
        of ops.split_solid_air (xyz, t, then the G channels) if the caller has split them.  The target's instance column
        defaults from data_kind (INSTANCE_COLUMNS).  pred_id (N,): another labelling of the queries to score instead of the
        mark_track channel.  The frame table is zero-filled, filled by the confusion pass and the two point passes and folded;
        no host read."""
        q, out, tgt = self._frame_inputs(points_query, implicit_output, target_rows)
        col = INSTANCE_COLUMNS.get(data_kind) if col_inst is None else int(col_inst)
        assert col is not None and 0 <= col < tgt.shape[1], 'no instance column: data_kind = %r, col_inst = %r, Dt = %d' % (data_kind, col_inst, tgt.shape[1])
        track = inference.get_track_idx(color_mode)
        if pred_id is None:
            assert track < out.shape[1], 'implicit_output has no mark_track channel %d (G = %d)' % (track, out.shape[1])
        else:
            pred_id = self._tensor(pred_id)
            assert pred_id.shape == (q.shape[0],), 'pred_id must be (N,)'
        found = self._frame_search(q, tgt, nn, inst_group)
        if found is None:
            return self
        idx, dist, grp = found
        if pred_id is not None:               # the solid rows carry the track channel, not this labelling: split it alongside
            solid = self._split_solid(q, torch.cat([out[:, :1], pred_id[:, None]], dim=1), density_threshold)
            solid_ids, pred_col = solid[:, 5], pred_id
        else:
            solid = self._tensor(self._split_solid(q, out, density_threshold) if solid is None else solid)
            solid_ids, pred_col = solid[:, 4 + track], out[:, track]
        self.frame.zero_()
        ops.inst_confusion(out[:, 0], pred_col, idx, dist, tgt[:, col], self.frame, n_ids=self.n_ids,
                           density_threshold=density_threshold, radius=point_occupancy_radius)
        ops.inst_points(solid, solid_ids, self.frame, n_ids=self.n_ids, side=_IC['SIDE_PRED'])
        ops.inst_points(tgt, tgt[:, col], self.frame, n_ids=self.n_ids, side=_IC['SIDE_GT'])
        ops.inst_fold(self.frame, self.counts, self.sums, n_ids=self.n_ids, n_groups=self.n_groups, inst_group=grp)
        return self

    def frame_tables(self):
        """The latest frame's table, from one host read: 'confusion' (n_ids + 1, n_ids + 1) int64 (row = ground truth, column
        = prediction, the last class = none), 'bad_rows', and per side 'pred' / 'gt' a dict of 'count' (n_ids,) int64 and
        'centroid' (n_ids, 3) float64, nan where the count is 0: the position of every object in this frame (its trajectory,
        when read once per output frame)."""
        K, C, W = self.n_ids, self.n_ids + 1, _IC['POINT_WORDS']
        f = self.frame.cpu().numpy()
        head = _IC['FRAME_HEAD']
        res = dict(confusion=f[head:head + C * C].reshape(C, C).copy(), bad_rows=int(f[_IC['BAD_ROWS']]))
        for name, side in (('pred', _IC['SIDE_PRED']), ('gt', _IC['SIDE_GT'])):
            t = f[head + C * C + side * K * W:head + C * C + (side + 1) * K * W].reshape(K, W)
            count = t[:, _IC['POINT_COUNT']].copy()
            s = t[:, _IC['POINT_SX']:_IC['POINT_SX'] + 3].astype(np.float64)
            res[name] = dict(count=count, centroid=_ratio(s, count[:, None]) / float(1 << _IC['FRACTION_BITS']))
        return res

    def summary(self):
        """The figures per group, as float64 arrays of shape (n_groups,) (nan where the denominator is 0), from one host read:
        instance_miou (mean IoU over the annotated instances), instance_iou_micro (summed intersections over summed unions),
        rq, sq, pq (recognition, segmentation and panoptic quality: an annotated instance is matched when its IoU > 0.5),
        centroid_error / centroid_error_sq (mean distance / squared distance between the centroid of an instance's predicted-
        solid queries and that of its target points).  'counts': the raw counts by name ((n_groups,) int64 each), 'bad_rows'.
        Raises ValueError when rows or ids were skipped (bad_rows > 0)."""
        G = self.n_groups
        counts, sums = self._read()
        bad = int(counts[_IC['BAD_ROWS']])
        if bad > 0:
            raise ValueError('InstanceStats: %d rows or ids were skipped (nn_idx outside the target, an id that is no integer in '
                             '[0, %d) and not negative, a coordinate beyond 1024, or a group id outside [0, %d))' % (bad, self.n_ids, G))
        per = counts[_IC['HEAD']:].reshape(G, _IC['GROUP_COUNTS'])
        c = {name.lower(): per[:, _IC[name]].copy() for name in _INST_COUNT_NAMES}
        s = sums.reshape(G, _IC['GROUP_SUMS'])
        match = c['n_match']
        res = dict(instance_miou=_ratio(s[:, _IC['SUM_IOU']], c['n_gt']), instance_iou_micro=_ratio(c['sum_inter'], c['sum_union']),
                   rq=_ratio(match, match + 0.5 * (c['n_pred'] - match) + 0.5 * (c['n_gt'] - match)),
                   sq=_ratio(s[:, _IC['SUM_IOU_MATCHED']], match),
                   centroid_error=_ratio(s[:, _IC['SUM_CENTROID_D']], c['n_centroid']),
                   centroid_error_sq=_ratio(s[:, _IC['SUM_CENTROID_D2']], c['n_centroid']))
        res['pq'] = res['sq'] * res['rq']
        res.update(counts=c, bad_rows=bad)
        return res


def occlusion_groups(live_occl_row, valo_ids_pad, num_valo_ids, n_ids, edges=(0.25, 0.75)):
    """(n_ids,) int32 group of every instance id for InstanceStats, from the outputs of occlusion.live_occlusion (host
    arithmetic): live_occl_row (max_valo_ids,) = the occlusion fractions of one input frame, valo_ids_pad / num_valo_ids = the
    ids they belong to.  A valo id with fraction f gets group np.searchsorted(edges, f, side='right') (0 .. len(edges)); every
    other id the last group, len(edges) + 1: an InstanceStats for it needs n_groups = len(edges) + 2."""
    edges = np.asarray(edges, np.float64)
    assert edges.ndim == 1 and bool((np.diff(edges) > 0).all()), 'edges must ascend'
    group = np.full((int(n_ids),), len(edges) + 1, dtype=np.int32)
    ids = np.asarray(valo_ids_pad)[:int(num_valo_ids)].astype(np.int64)
    frac = np.asarray(live_occl_row, np.float64)[:int(num_valo_ids)]
    keep = (ids >= 0) & (ids < int(n_ids))
    group[ids[keep]] = np.searchsorted(edges, frac[keep], side='right').astype(np.int32)
    return group


def evaluate_clip(batch, networks, device, args, data_kind, logger=None, save_gt=False, reuse_encode=True, stats=None,
                  stats_group_fn=None, stats_occlusion=None, inst_stats=None, inst_group_fn=None, refine=None, surface=None,
                  meshes=None, views=None, images=None, components=None, objects=None, tracker=None, clearance=None,
                  clearances=None, evidence=None, evidences=None, sweep=None, sweeps=None, layers=None, layer_images=None, boxes=None, next_view=None, next_views=None, sight=None, sights=None, segments=None, parts=None, route=None, routes=None):
    """batch: dict with 'pcl_input' (1,N,8), 'pcl_input_sem' (1,N,1-3), 'pcl_target' list of (1,T,9-11) tensors and
    batch['meta_data']['pcl_target_size'] (list of (1,) tensors), as the reference's test data loader yields them
    (data/data_greater.py:593-606, data/data_carla.py:651-661).  args: namespace with the test_args fields used
    below (args.py:311-410).  Returns pcl_all (list over output frames of tuples of numpy arrays).
    stats: an EvalStats that every output frame is added to, scored against its target frame (on the device, beside the
    decode); stats_group_fn(frame_rows) -> (T,) integer array: the group of every target point.  None: nothing is scored.
    stats_occlusion: instead of stats_group_fn, a dict 'depth' (T_out, H, W), 'cam_RT' (T_out, 3, 4), 'cam_K' ((3, 3) or
    (T_out, 3, 3)), 'margin': the group of a target point of output frame t is its projection.visibility code against depth[t]
    under camera t (VISIBLE 0 / OCCLUDED 1 / OUTSIDE 2; `stats` needs n_groups >= 3), computed on the device.
    inst_stats: an InstanceStats that every output frame is added to in the same way (track_mode 'all': the instance
    labelling); inst_group_fn(time_idx, frame_rows) -> (n_ids,) integer array: the group of every instance id, None: group 0.
    refine: an inference.GridRefine handed to every perform_inference call (the coarse-to-fine decode of the query grid), or None.
    surface / meshes, views / images, components / objects, clearance / clearances, segments / parts, sight / sights, next_view / next_views, route / routes: a grid product's
    option object (surface.Surface, projection.FieldViews, components.Components, distance.Clearance, watershed.Segments,
    sight.Sight, sight.NextView, geodesic.Route; `route` needs `clearance`, `next_view` needs `sight`)
    handed to every perform_inference call, or None, and the list every output frame's result[keyword] dict is appended to (the
    tuples of pcl_all keep their contract).  An option without such a list is a ValueError; all options are checked before the
    first frame.
    tracker: a components.Tracker, or None (needs `components`): reset here, then handed to every perform_inference call, so that
    every dict of `objects` gains 'link' (K, 4), the frame's components linked to those of the output frame before
    (components.tracks turns the list into trajectories).
    boxes: a components.Boxes, or None (needs the product its `of` names, `components` or `segments`): handed to every
    perform_inference call, so that every dict of `objects` (or `parts`) gains 'box' (K, 8) and 'dirs' (A, 4), the upright
    oriented box of every object; it takes no list of its own, as `tracker`.  components.tracks then also gives obox_centre,
    obox_size and obox_yaw per trajectory.
    layers / layer_images: a projection.ObjectLayers, or None (needs the product its `of` names, `components` or `segments`), and
    the list every output frame's result['layers'] dict is appended to: that product's objects as depth layers in the option's
    camera views -- amodal and visible masks, occlusion rates and order (projection.amodal_mask, visible_mask, occlusion_rate,
    occlusion_pairs, layer_depth work on the dict's arrays).
    sweep / sweeps: a sweep.FieldSweep, or None (with of= it needs that product, `components` or `segments`), and the list every
    output frame's result['sweep'] dict is appended to: the decoded field scanned by a virtual lidar -- ranges, incidence cosines,
    class and object per ray, and with rows= the returns in the lidar loader's row format (sweep.rows_of).
    evidence / evidences: an evidence.Evidence, or None, and the list every output frame's result['evidence'] dict is appended to:
    the option's measured returns carved into the grid and crossed with the predicted solid set -- code, hits[, passes], totals,
    status (evidence.rates, evidence.by_label).  ONE option for every output frame: the returns are timeless, the caller selects
    the rows that bear on the clip."""
    chosen = products.check_clip((
        (geodesic_mod.Route, route, routes), (sight_mod.NextView, next_view, next_views), (sight_mod.Sight, sight, sights),
        (evidence_mod.Evidence, evidence, evidences), (sweep_mod.FieldSweep, sweep, sweeps), (projection.ObjectLayers, layers, layer_images), (components_mod.Boxes, boxes, None),
        (watershed_mod.Segments, segments, parts), (distance_mod.Clearance, clearance, clearances),
        (components_mod.Tracker, tracker, None),
        (components_mod.Components, components, objects), (projection.FieldViews, views, images), (surface_mod.Surface, surface, meshes)))
    if tracker is not None:
        tracker.reset()
    assert stats_group_fn is None or stats_occlusion is None, 'stats_group_fn and stats_occlusion exclude each other'
    if stats_occlusion is not None and stats is not None:
        assert stats.n_groups >= 3, 'stats_occlusion needs an EvalStats with n_groups >= 3, got %d' % stats.n_groups
        occ_rt, occ_k = stats_occlusion['cam_RT'], stats_occlusion['cam_K']
    # One encode per clip is only equivalent to the reference's encode per output frame when the encode is
    # deterministic: a network built with fps_random_start=True (the constructor default; the reference's test path
    # builds its networks with False, eval/inference.py:59) draws a new FPS start per call, so it is re-encoded per frame.
    if reuse_encode and any(getattr(m, 'fps_random_start', False) for m in networks[0].modules()):
        reuse_encode = False
    pcl_input = batch['pcl_input']
    pcl_input_numpy = pcl_input[0].detach().cpu().numpy()
    pcl_input_sem_numpy = batch['pcl_input_sem'][0].detach().cpu().numpy()
    sem_inference = pcl_input_sem_numpy if args.track_mode != 'none' else None
    pcl_target = batch['pcl_target']
    sizes = batch['meta_data']['pcl_target_size']
    pcl_all = []
    encoded = None
    for time_idx in range(len(pcl_target)):
        frame = pcl_target[time_idx][0].detach().cpu().numpy()
        frame = frame[:int(sizes[time_idx].item() if torch.is_tensor(sizes[time_idx]) else sizes[time_idx])]
        stats_kw = {}
        if stats is not None:
            group = None if stats_group_fn is None else stats_group_fn(frame)
            if stats_occlusion is not None:
                group = projection.visibility(torch.from_numpy(np.ascontiguousarray(frame[:, :3])).to(stats.device),
                                              stats_occlusion['depth'][time_idx], occ_rt[time_idx],
                                              occ_k if np.ndim(occ_k) == 2 else occ_k[time_idx], stats_occlusion['margin'])[0]
            stats_kw = dict(stats=stats, stats_target=frame, stats_group=group)
        if inst_stats is not None:
            stats_kw.update(inst_stats=inst_stats, stats_target=frame,
                            inst_group=None if inst_group_fn is None else inst_group_fn(time_idx, frame))
        res = inference.perform_inference(
            pcl_input.clone(), sem_inference, frame if save_gt else None, networks, device, 'if', args.min_z,
            args.cr_cube_bounds, args.color_mode, time_idx, logger, sample_implicit=args.sample_implicit,
            num_sample=args.num_sample, point_sample_mode=args.point_sample_mode, batch_size=args.implicit_batch_size,
            predict_segmentation=args.segmentation_lw > 0.0, track_mode=args.track_mode,
            point_occupancy_radius=args.point_occupancy_radius, semantic_classes=args.semantic_classes,
            density_threshold=args.density_threshold, data_kind=data_kind, cube_mode=args.cube_mode, compress_air=True,
            encoded=encoded if reuse_encode else None, return_encoded=reuse_encode, refine=refine,
            **{option.keyword: option for option, _ in chosen}, **stats_kw)
        if reuse_encode:                  # (track_mode 'all': a dict with one encode per tracked instance)
            encoded = res.pop('_encoded')
        else:
            res.pop('_encoded', None)
        for option, into in chosen:
            if into is not None:
                into.append(res[option.keyword])
        item =(pcl_input_numpy, res['pcl_abstract'], res['output_solid'], frame, res['output_air'])
        if save_gt:
            item = item + (pcl_input_sem_numpy, res['points_query'])
        pcl_all.append(item)
    return pcl_all


def store_clip(pcl_all, log_dir, test_tag, cur_step, meta=None):
    """Writes pcl_io_s{step}.p (and metadata_s{step}.p when `meta` = (meta_data, cam_RT, cam_K) is given) under
    <log_dir>/test_<tag>/ exactly as eval/test.py:120-135 does through logvis.save_pickle.  Returns the path."""
    folder = os.path.join(log_dir, 'test_' + test_tag)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, 'pcl_io_s%d.p' % cur_step)
    with open(path, 'wb') as f:
        pickle.dump(pcl_all, f)
    if meta is not None:
        with open(os.path.join(folder, 'metadata_s%d.p' % cur_step), 'wb') as f:
            pickle.dump(meta, f)
    return path


def load_clip(path):
    """Reads a pcl_io_s{step}.p back; checks the tuple contract."""
    with open(path, 'rb') as f:
        pcl_all = pickle.load(f)
    assert isinstance(pcl_all, list)
    for item in pcl_all:
        assert isinstance(item, tuple) and len(item) in (5, 7)
        assert all(isinstance(a, np.ndarray) for a in item)
    return pcl_all
