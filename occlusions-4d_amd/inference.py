"""Inference driver on the HIP library.

Interface mirror of the reference's eval/inference.py: ``load_models`` (:23-80) and
``perform_inference`` (:83-325, same positional/keyword arguments and result dict).
Differences that do not change results: the query grid is uploaded once and every
mini-batch, the post-ops (sigmoid / clamp, :218-243) and the concatenation stay on the
device; one device-to-host copy happens at the end instead of one per batch (:206,245).
The optional ground-truth 1-NN labelling branch (:270-276, sklearn KDTree on targets)
is provided on the streaming k = 1 kernel; track_mode 'all' reruns the path once per instance id.
"""
import functools
import os

import numpy as np
import torch

from . import geometry
from . import implicit
from . import kernels
from . import model
from . import ops
from . import products
from . import projection
from . import surface as surface_nets
from . import components as components_mod
from . import distance as distance_mod
from . import geodesic as geodesic_mod
from . import watershed as watershed_mod
from . import sight as sight_mod
from . import sweep as sweep_mod
from . import evidence as evidence_mod


def get_track_idx(color_mode):
    """Channel of mark_track in the implicit output (utils/utils.py:204-224)."""
    table = {'rgb': 4, 'rgb_nosigmoid': 4, 'hsv': 15, 'bins': 10}
    if color_mode not in table:
        raise ValueError()
    return table[color_mode]


def load_models(checkpoint_path, device, epoch=-1, logger=None):
    """Builds [pcl_net, implicit_net] from a reference checkpoint (keys args, dset_args,
    pcl_args, implicit_args, pcl_net, implicit_net, epoch -- train.py:339-350)."""
    print_fn = logger.info if logger is not None else print
    assert os.path.exists(checkpoint_path)
    if os.path.isdir(checkpoint_path):
        checkpoint_path = os.path.join(checkpoint_path, f'model_{epoch}.pth' if epoch >= 0 else 'checkpoint.pth')
    print_fn('Loading weights from: ' + checkpoint_path)
    ckpt = torch.load(checkpoint_path, map_location='cpu', weights_only=False)
    train_args, dset_args = ckpt['args'], ckpt['dset_args']
    pcl_args, implicit_args = dict(ckpt['pcl_args']), dict(ckpt['implicit_args'])
    pcl_args['fps_random_start'] = False          # deterministic at test time (:59)
    dec_sd = {(('pt_blocks.0.' + k[len('pt_block.'):]) if k.startswith('pt_block.') else k): v
              for k, v in ckpt['implicit_net'].items()}   # legacy key rename (:62-63)
    pcl_net = model.PointCompletionNetV3(**pcl_args).to(device)
    pcl_net.load_state_dict(ckpt['pcl_net'])
    implicit_net = implicit.LocalPclResnetFC(**implicit_args).to(device)
    implicit_net.load_state_dict(dec_sd)
    epoch = ckpt['epoch']
    print_fn('=> Loaded epoch (1-based): ' + str(epoch + 1))
    return ([pcl_net, implicit_net], train_args, dset_args, pcl_args, implicit_args, epoch)


def squash_codes(d_out, color_mode, predict_segmentation, track_mode, semantic_classes):
    """Per-channel post-op codes for occ4d_squash_f32 (0 identity, 1 sigmoid, 2 clamp[0,1]),
    equivalent to the in-place sequence of eval/inference.py:218-243 (a later sigmoid on a
    channel composes with an earlier op exactly as the reference's sequential writes do
    only when ranges do not overlap; overlapping ranges are rejected)."""
    codes = [0] * d_out
    applied = [0] * d_out

    def put(lo, hi, code):
        for c in range(lo, hi):
            c = c % d_out
            codes[c] = code
            applied[c] += 1
    put(0, 1, 1)
    if color_mode == 'rgb':
        put(1, 4, 1)
    elif color_mode == 'rgb_nosigmoid':
        put(1, 4, 2)
    elif color_mode == 'hsv':
        put(1, 13, 1)
        put(13, 15, 2)
    elif color_mode == 'bins':
        put(1, 10, 1)
    if predict_segmentation:
        put(d_out - semantic_classes, d_out, 1)
    if track_mode != 'none':
        ti = get_track_idx(color_mode)
        put(ti, ti + 1, 1)
    assert max(applied) <= 1, 'overlapping post-op channel ranges'
    return codes


PINNED_HOST_IO = os.environ.get('OCC4D_PINNED_HOST_IO', '1') == '1'

# Side streams live as long as the process, one set per device.  torch's caching allocator keeps a block pool PER STREAM:
# with fresh `torch.cuda.Stream()` objects in every call the decode workspaces (465 MB at the BASELINE grid) and the
# result buffers were allocated again by every perform_inference call until torch's 32-stream pool had gone round
# (profiles/host_boundary_probe.py: +8 ms per call).
_STREAMS = {}


def side_streams(device, role, count=1):
    """`count` persistent HIP streams of `device` for `role` ('decode' / 'copy')."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, role)
    have = _STREAMS.setdefault(key, [])
    while len(have) < count:
        have.append(torch.cuda.Stream(device=torch.device('cuda', index)))
    return have[:count]


class _HostCopies:
    """Device -> host result copies of perform_inference: every array goes into a page-locked buffer from torch's caching
    host allocator with a non-blocking copy on a side stream that waits for the producing stream, so that the copies
    overlap each other and the remaining device work, and the host blocks ONCE, at the end.  (The reference moves each
    array with a blocking `.cpu()` through pageable memory: eval/inference.py:218-246; at 0.53 M queries that was 24 ms
    of a 144 ms call.)  The numpy arrays handed out own their buffers (views of the pinned tensors, kept alive by numpy's
    base reference); the allocator reuses a block only after the caller has dropped the array."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.on = PINNED_HOST_IO and self.device.type == 'cuda'
        self.stream = side_streams(self.device, 'copy')[0] if self.on else None
        self.pending = []

    def fetch(self, t, dtype=None):
        """Schedules the copy of device tensor `t` (optionally converted to `dtype` on the device) and returns a handle;
        `result(handle)` after `wait()` gives the numpy array."""
        if t is None:
            return None
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if not self.on:
            return t.cpu().numpy()
        t = t.contiguous()
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        self.stream.wait_stream(torch.cuda.current_stream(t.device))
        with torch.cuda.stream(self.stream):
            host.copy_(t, non_blocking=True)
        t.record_stream(self.stream)
        self.pending.append(host)
        return host

    def wait(self):
        if self.on:
            self.stream.synchronize()

    @staticmethod
    def result(h):
        return h.numpy() if torch.is_tensor(h) else h


_REQUIRED = object()


class GridRefine:
    """One-level coarse-to-fine decode of the dense query grid (perform_inference(refine=...), include/occ4d_refine.h).  The
    grid is cut into blocks of `block` points per axis (2 .. 8; edge blocks are clipped).  Pass 1 decodes one representative
    per block, the grid point at min(block index * block + block // 2, n_axis - 1) per axis.  A block is hot when its
    representative's squashed density d satisfies not (d < low); it is active when a block within Chebyshev distance `dilate`
    (0 .. 2) is hot.  Pass 2 decodes the other points of the active blocks; every point that was not decoded takes its
    block's representative row.  `low` has no default: the value that loses no solid query depends on the trained density
    field."""

    def __init__(self, block=2, low=_REQUIRED, dilate=1):
        if low is _REQUIRED:
            raise TypeError("GridRefine needs `low`: the density below which a block's representative counts as air")
        for name, v, lo, hi in (('block', block, 2, 8), ('dilate', dilate, 0, 2)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError('GridRefine: %s = %r must be an integer in %d .. %d' % (name, v, lo, hi))
        low = float(low)
        if low != low:
            raise ValueError('GridRefine: low is NaN')
        self.block, self.low, self.dilate = int(block), low, int(dilate)

    def __repr__(self):
        return 'GridRefine(block=%d, low=%r, dilate=%d)' % (self.block, self.low, self.dilate)


def perform_inference(pcl_input, pcl_input_sem, pcl_target_frame, networks, device, task, min_z,
                      cube_bounds, color_mode, time_idx, logger,
                      sample_implicit=True, num_sample=16384, point_sample_mode='random',
                      batch_size=1024, predict_segmentation=False, track_mode='none',
                      point_occupancy_radius=0.2, semantic_classes=13,
                      density_threshold=0.5, data_kind='', cube_mode=4, compress_air=False,
                      encoded=None, return_encoded=False, neighbour_lists=None, stats=None, stats_target=None,
                      stats_group=None, track_merge='device', inst_stats=None, inst_group=None, refine=None, surface=None,
                      views=None, components=None, route=None, evidence=None, sweep=None, layers=None, boxes=None, next_view=None, sight=None, segments=None, tracker=None, clearance=None):
    """One encode of the input point-cloud video + decode of all query points of one output frame.  Returns
    dict(output_solid, output_air, pcl_abstract, features_global, implicit_output, points_query) of float32 numpy arrays, and
    gt_solid / gt_air when `pcl_target_frame` is given.  The keywords from `encoded` on are extensions whose defaults give the
    reference's behaviour.  The host blocks once, at the end; the scorers and `refine` add no wait.

    Encode reuse.  `encoded` = the (pcl_abstract, features_global) device tensors of an earlier call on the same input cloud
    (the reference re-encodes the clip for every output frame, eval/test.py:67-86); `return_encoded` adds them to the result as
    '_encoded'.  In track_mode 'all' both are dicts {instance id: (pcl_abstract, features_global)}, one entry per rerun.

    Neighbour lists.  `neighbour_lists` = (knn_local (N_q, 8), knn_cross (N_q, 14)) integer arrays, either may be None: the
    decoder's neighbour lists of a particular run of the reference for these queries (LocalPclResnetFC.forward's extension).

    Scoring.  `stats` = an evaluation.EvalStats this frame is added to, scored on the device against `pcl_target_frame` (or
    `stats_target` when that is None: no gt_solid / gt_air then), `stats_group` = the group id per target point.  `inst_stats`
    = an evaluation.InstanceStats added to in the same way (the scorer of track_mode 'all': the merged mark_track channel as an
    instance labelling), `inst_group` = the group id per instance id.  The scorers and the gt branch share one upload of the
    target rows, one query -> target search and the solid split; they change neither the result dict nor the one host wait.

    Track merge.  `track_merge`: where the reruns of track_mode 'all' are merged.  'device': a running merge in the library
    (ops.track_merge_add / track_merge_finish: squash, sums and the winner / best update in one pass per rerun); the merged
    tensor stays on the device for the split and the scoring.  'host': every rerun is copied to the host (a second host wait),
    multi_track_merge runs in numpy and the merged array is uploaded again.  Same bits.

    Refine.  `refine`: a GridRefine (its two passes per run are described there), or None = every query is decoded.
    point_sample_mode 'grid' only, and not with `neighbour_lists` (ValueError).  The dense (N, G) output is rebuilt on the
    device: the split, compress_air, the scorers, the track merge and the result dict work on it as on a dense decode.  THE
    CONTRACT, and nothing stronger: every decoded row equals the dense call's row bit for bit; every other row is a copy of
    its block's representative row, whose density is below `low`.  With refine.low <= density_threshold, output_solid is
    therefore a subset of the dense call's, in the same order, and the same set exactly when no solid query lies in an
    inactive block.  One device->host read per run (two counts, 8 bytes) sizes the second pass.  The result gains 'refine' =
    dict(n_queries, n_decoded): host ints, summed over the reruns.  (Bit for bit under the default kernel selection, whose one
    dependence of a row on its place in the mini-batch decode_refined reproduces; under another kernels.Selection only within
    the mini-batch-split bound, 1e-5.)

    Grid products.  `surface`, `views`, `components`, `tracker`, `clearance`, `segments`, `boxes`, `layers`, `sweep`, `evidence`, `sight`, `next_view`, `route`: option objects (products.GridProduct), or
    None = nothing is called and no key is added.  point_sample_mode 'grid' only (ValueError).  Each turns the same squashed (N, G)
    array -- in track_mode 'all' merged, under `refine` expanded -- into more arrays on the device, which come back with the others,
    under the one host wait; the option class describes its arguments and its arrays.  They are checked, and run, in this order:
    `surface`: a surface.Surface -> result['surface'] = dict(vertices, faces), the quad mesh of density == level.  Under `refine`
    with refine.low <= level the mesh exists only where blocks were decoded (surface.py).
    `views`: a projection.FieldViews -> result['views'] = dict(depth, cell, features), the array ray-cast into the cameras.
    `components`: a components.Components -> result['components'] = dict(labels, table), the connected components of density >=
    level; by_class needs predict_segmentation (ValueError).
    `tracker`: a components.Tracker; needs `components` (ValueError) -> result['components'] gains 'link': the components linked
    to those of the tracker's previous frame.  The tracker then holds this frame.
    `clearance`: a distance.Clearance -> result['clearance'] = dict(dist2[, nearest][, inside2]), the exact distance transform of
    density >= level.
    `segments` (in the signature in front of `tracker` as well): a watershed.Segments -> result['segments'] = dict(labels, table,
    peaks), the solid set split at its necks: the watershed segments of its own inside2, with the tolerance h (required).
    `sight` (in the signature in front of `segments`): a sight.Sight -> result['sight'] = dict(seen[, framed][, blocker]), line of
    sight through density >= level: per query a bit per sensor origin, set where the segment between them meets no solid cell;
    with cameras also which of them frame the query, with blocker=True the cell that hides it.  Needs no other product.
    `boxes` (in the signature in front of `next_view`: the suite pins the names that follow): a components.Boxes; needs the product
    its `of` names, `components` or `segments` (ValueError) -> that product's dict gains box (K, 8) int32 and dirs (A, 4) int32,
    with extents=True also extent (K, A, 4) int32: per object the upright oriented box of least footprint area over a table of
    headings (components.oriented_boxes turns the rows into centre, length, width, height and yaw).  Runs after `segments`.
    `layers` (in the signature in front of `boxes`): a projection.ObjectLayers; needs the product its `of` names, `components` or
    `segments` (ValueError) -> result['layers'] = dict(<the chosen of label, first, samples, point (V, H, W, L), count (V, H, W)>,
    table (V, K, 7), status (2,), march (2,)): that product's objects as depth layers in the option's camera views -- per pixel the
    objects its ray passes through in the order of first entry, per view and object the amodal and the visible pixel counts, the
    nearest sample and the amodal 2-D box (include/ext/occ4d_layers.h).  status[0] == 0 says that no pixel dropped an object and
    the table is exact.  A layer's depth is quantised to the march's step; it is not the refined crossing of `views`.  Runs after
    `boxes`.
    `sweep` (in the signature in front of `layers`): a sweep.FieldSweep -> result['sweep'] = dict(range, point, cell, owner, cos[, sem]
    [, inst], features[, rows, n_rows], march (2,)): the array scanned by a virtual lidar -- per ray of the option's poses and
    directions the range of the first crossing of density == level, the incidence cosine, the grid point on the solid side with
    its class (predict_segmentation) and its object (the option's `of` names the label product, `components` or `segments`, which
    has to be given: ValueError), and with rows= the returns as rows in the lidar loader's format (include/ext/occ4d_sweep.h;
    sweep.rows_of trims them).  Uniform samples with the refinement of `views`, not an exact intersection.  Runs after `layers`.
    `evidence` (in the signature in front of `sweep`): an evidence.Evidence -> result['evidence'] = dict(code, hits[, passes], totals,
    status): the option's measured returns carved into the grid -- the cells between a sensor and its return are measured free, the
    return's cell is hit, the rest is unknown -- crossed with density >= level into six codes per query: a predicted solid in
    measured free space is CONTRADICTED, a return in predicted air MISSED, a predicted solid no ray reached COMPLETED
    (include/ext/occ4d_evidence.h; evidence.rates, evidence.by_label).  The returns are taken as given and are timeless.  Needs no
    other product.  Runs after `sweep`.
    `next_view` (in the signature in front of `sight`: the suite pins the last four names): a sight.NextView; needs `sight`
    (ValueError) -> result['next_view'] = dict(gain, picks, pick_gain, status): of the queries that call's sensors do not see, how
    many each candidate viewpoint would see, and a greedy choice of up to k of them that together see the most.
    `route` (in the signature it stands in front of `tracker`: the suite pins the last two names): a geodesic.Route; needs
    `clearance` (ValueError) -> result['route'] = dict(cost, status[, parent][, paths, path_len]), the shortest free-space paths over
    that call's dist2.  World-point seeds and goals become grid indices on the host before the decode (ValueError outside the
    grid); status[0] == 1 says that the costs are converged and has to be looked at."""
    assert task == 'if'
    assert sample_implicit
    assert track_merge in ('device', 'host'), track_merge
    slots = ((surface_nets.Surface, surface), (projection.FieldViews, views), (components_mod.Components, components),
             (components_mod.Tracker, tracker), (distance_mod.Clearance, clearance), (watershed_mod.Segments, segments),
             (components_mod.Boxes, boxes), (projection.ObjectLayers, layers), (sweep_mod.FieldSweep, sweep), (evidence_mod.Evidence, evidence), (sight_mod.Sight, sight), (sight_mod.NextView, next_view), (geodesic_mod.Route, route))
    grid = None                               # the very floats the query grid is generated from
    if point_sample_mode == 'grid' and (refine is not None or any(option is not None for _, option in slots)):
        grid = products.Grid(geometry.grid_frame(num_sample, min_z, cube_bounds, data_kind, cube_mode), density_threshold,
                             predict_segmentation, semantic_classes, device)
    if refine is not None:
        if not isinstance(refine, GridRefine):
            raise ValueError('refine must be a GridRefine or None, got %r' % (refine,))
        if point_sample_mode != 'grid':
            raise ValueError("refine needs point_sample_mode 'grid', got %r" % (point_sample_mode,))
        if neighbour_lists is not None:
            raise ValueError('refine decodes gathered queries: neighbour_lists cannot be given with it')
    plan = products.prepare(slots, grid, point_sample_mode)
    refine_stats = dict(n_queries=0, n_decoded=0)
    output_track_idx = get_track_idx(color_mode)
    input_inst_idx = 0 if data_kind == 'greater' else 1
    pcl_net, implicit_net = networks
    if isinstance(pcl_input, np.ndarray):
        pcl_input = torch.from_numpy(pcl_input).unsqueeze(0)
    pcl_input = pcl_input.to(device)

    # One rerun per tracked instance (track_mode 'all', :144-161), otherwise a single run.
    if track_mode in ('none', 'one'):
        track_instance_ids = [-1]
    else:
        assert data_kind == 'greater'
        assert pcl_input_sem.shape[-1] == 1
        if isinstance(pcl_input_sem, np.ndarray):
            sem_numpy = pcl_input_sem
            pcl_input_sem = torch.from_numpy(pcl_input_sem).unsqueeze(0).to(device)
        else:
            sem_numpy = pcl_input_sem[0].detach().cpu().numpy()
            pcl_input_sem = pcl_input_sem.to(device)
        ids, counts = np.unique(sem_numpy, return_counts=True)
        track_instance_ids = [int(i) for i, c in zip(ids, counts) if i >= 0 and c >= 16]

    queries_dev = geometry.sample_implicit_points_blind_device(
        num_sample, min_z, cube_bounds, time_idx, data_kind, cube_mode, point_sample_mode, device)
    copies = _HostCopies(device)
    # (an empty id list goes to the host merge and fails inside multi_track_merge)
    kind = _SingleRun if track_instance_ids == [-1] else _DeviceMerge if track_merge == 'device' and track_instance_ids else _HostMerge
    collector = kind(copies, track_instance_ids, output_track_idx, (color_mode, predict_segmentation, track_mode, semantic_classes))
    points_query = copies.fetch(queries_dev)              # (under the encode / decode that follows)
    encoded_out = {}
    with torch.no_grad():
        for inst_id in track_instance_ids:
            if inst_id >= 0:                  # mark the instance to follow in the input cloud (:190-193)
                pcl_input[..., -1] = (pcl_input_sem[..., input_inst_idx] == inst_id)
            res = infer_device(pcl_input, queries_dev, pcl_net, implicit_net, batch_size, color_mode,
                               predict_segmentation, track_mode, semantic_classes,
                               encoded=_encoded_for(encoded, inst_id), neighbour_lists=neighbour_lists,
                               squash=collector.squash, refine=refine, grid_counts=None if refine is None else grid.counts)
            encoded_out[inst_id] = (res['pcl_abstract'], res['features_global'])
            if refine is not None:
                for k in refine_stats:
                    refine_stats[k] += res['refine'][k]
            collector.add(res, inst_id)
        output_dev = collector.finish()            # (N, G), squashed and merged

        gt_available = pcl_target_frame is not None
        target_dev, nn_dev, labels = _target_frame(queries_dev[:, :3], pcl_target_frame, point_occupancy_radius, device,
                                                  stats_target, scored=stats is not None or inst_stats is not None)
        if gt_available:                      # nearest ground-truth point of every query (:270-276)
            points_nngt = np.concatenate([labels[0][:, None], pcl_target_frame[labels[1]]], axis=-1)

        # density-threshold split + compress_air on the device (:279-305): order-preserving compaction
        solid, air = ops.split_solid_air(queries_dev, output_dev, density_threshold, compress_air, semantic_classes)
        if stats is not None:
            assert not predict_segmentation or stats.semantic_classes in (0, semantic_classes), \
                'stats.semantic_classes = %d, semantic_classes = %d' % (stats.semantic_classes, semantic_classes)
            stats.add_frame(queries_dev, output_dev, target_dev, density_threshold=density_threshold,
                            point_occupancy_radius=point_occupancy_radius, color_mode=color_mode,
                            predict_segmentation=predict_segmentation, track_mode=track_mode, data_kind=data_kind,
                            target_group=stats_group, nn=nn_dev, solid=solid)
        if inst_stats is not None:
            inst_stats.add_frame(queries_dev, output_dev, target_dev, density_threshold=density_threshold,
                                 point_occupancy_radius=point_occupancy_radius, color_mode=color_mode, data_kind=data_kind,
                                 inst_group=inst_group, nn=nn_dev, solid=solid)
        # (the reference's concatenate with the int64 argmax promotes the compressed air rows to float64: converted on
        # the device, not by a host pass over the array)
        solid_h = copies.fetch(solid)
        air_h = copies.fetch(air, torch.float64 if compress_air else None)
        if grid is not None:
            grid.output, grid.points = output_dev, queries_dev[:, :3]
        made, fetched = {}, []                # per product its device tensors; (result key, the handles of their copies)
        for product, prepared in plan:
            made[product.keyword] = product.run(grid, prepared, made)
            fetched.append((product.into or product.keyword, {k: copies.fetch(t) for k, t in made[product.keyword].items()}))
        copies.wait()
        solid, air = copies.result(solid_h), copies.result(air_h)
        points_query = copies.result(points_query)
        (pcl_abstract, features_global, implicit_output) = collector.host()
    ops.check_pending()                      # cooperative-FPS status words (everything above has completed)
    result = dict(output_solid=solid, output_air=air, pcl_abstract=pcl_abstract,
                  features_global=features_global, implicit_output=implicit_output, points_query=points_query)
    if refine is not None:
        result['refine'] = refine_stats
    for key, handles in fetched:
        result.setdefault(key, {}).update((k, copies.result(h)) for k, h in handles.items())
    if return_encoded:
        result['_encoded'] = encoded_out[-1] if -1 in encoded_out else encoded_out     # (a tuple for the one unmarked run)
    if gt_available:
        solid_mask = implicit_output[..., 0] >= density_threshold
        gt_solid, gt_air = points_nngt[solid_mask], points_nngt[~solid_mask]
        if compress_air:
            gt_air = np.concatenate([gt_air[..., :1], gt_air[..., 4:5]], axis=-1)
        result['gt_solid'], result['gt_air'] = gt_solid, gt_air
    return result


def _encoded_for(encoded, inst_id):
    """The caller's encode of the run that follows `inst_id` (-1: the unmarked run), or None: encode it now."""
    if inst_id < 0:
        return None if isinstance(encoded, dict) else encoded
    return encoded.get(inst_id) if isinstance(encoded, dict) else None


class _Runs:
    """The decode runs of one perform_inference call on their way to one result; three collectors fill this in.  `squash`: whether
    infer_device squashes a run's output; add(res, inst_id) per run; finish() -> the squashed and merged (N, G) device tensor;
    host(), after the call's last copies.wait() -> the numpy (pcl_abstract, features_global, implicit_output)."""
    squash = True

    def __init__(self, copies, track_instance_ids, track_col, post_ops):
        self.copies, self.ids, self.track_col, self.post_ops = copies, track_instance_ids, track_col, post_ops

    def host(self):
        return tuple(self.copies.result(h) for h in self.handles)


class _SingleRun(_Runs):
    """The one unmarked run (track_mode 'none' / 'one'): its tensors are the result."""

    def add(self, res, inst_id):
        self.output = res['implicit_output']
        output_h = self.copies.fetch(self.output)
        self.handles = (self.copies.fetch(res['pcl_abstract']), self.copies.fetch(res['features_global']), output_h)

    def finish(self):
        return self.output


class _DeviceMerge(_Runs):
    """multi_track_merge as a running merge on the device: one accumulator each for the RAW implicit output (squashed by the
    add, with the winner / best columns of its track channel), the abstract cloud and the global feature.  The latter two go
    through the same entry point as flat contiguous (n, 1) views without squash or track column; an abstract of None stays None."""
    squash = False
    runs = 0

    def add(self, res, inst_id):
        raw, pcl_abstract, features_global = res['implicit_output'], res['pcl_abstract'], res['features_global']
        first = self.runs == 0
        if first:
            new = lambda like, shape: torch.empty(shape, dtype=torch.float32, device=like.device)
            self.output, self.best, self.winner = new(raw, tuple(raw.shape)), new(raw, raw.shape[:1]), new(raw, raw.shape[:1])
            self.abstract = None if pcl_abstract is None else new(pcl_abstract, pcl_abstract.shape)
            self.features = new(features_global, features_global.shape)
            self.codes = squash_codes(raw.shape[1], *self.post_ops)
        ops.track_merge_add(raw, self.output, self.best, self.winner, inst_id, self.track_col, self.codes, first=first)
        for part, acc in ((pcl_abstract, self.abstract), (features_global, self.features)):
            if acc is not None:
                ops.track_merge_add(part.contiguous().view(-1, 1), acc.view(-1, 1), None, None, inst_id, -1, None, first=first)
        self.runs += 1

    def finish(self):
        ops.track_merge_finish(self.output, self.winner, self.runs, self.track_col)
        for acc in (self.abstract, self.features):
            if acc is not None:
                ops.track_merge_finish(acc.view(-1, 1), None, self.runs, -1)
        self.handles = tuple(self.copies.fetch(t) for t in (self.abstract, self.features, self.output))
        return self.output


class _HostMerge(_Runs):
    """The merge of the reruns as host arithmetic: every run is copied to the host; finish() waits for the copies, merges
    them with multi_track_merge (the arrays host() hands out) and uploads the merged output for the split and the scoring."""

    def __init__(self, *args):
        super().__init__(*args)
        self.output, self.abstract, self.features = [], [], []

    def add(self, res, inst_id):
        self.output.append(self.copies.fetch(res['implicit_output']))
        self.abstract.append(self.copies.fetch(res['pcl_abstract']))
        self.features.append(self.copies.fetch(res['features_global']))

    def finish(self):
        self.copies.wait()
        self.handles = multi_track_merge(self.ids, *([self.copies.result(h) for h in part]
                                                     for part in (self.abstract, self.features, self.output)), self.track_col)
        return torch.from_numpy(self.handles[2]).to(self.copies.device)


def _target_frame(points_query_xyz, pcl_target_frame, thresh, device, stats_target=None, scored=False):
    """The target frame (`pcl_target_frame`, else `stats_target`) for the scorers and the gt branch -> (target_dev, nn, labels),
    each None when nobody asks for it.  target_dev: the full-width rows, uploaded only when the frame is `scored` (otherwise the
    xyz columns alone go up); nn: the ONE query -> target search; labels: get_1nn_label's, when pcl_target_frame is given."""
    rows = pcl_target_frame if pcl_target_frame is not None else stats_target
    if not scored and pcl_target_frame is None:
        return None, None, None
    target_dev = None
    if scored:
        assert rows is not None, 'stats / inst_stats need a target frame: pcl_target_frame or stats_target'
        target_dev = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float32) if isinstance(rows, np.ndarray)
                                     else rows).to(device=device, dtype=torch.float32)
    nn = nn_target(points_query_xyz, target_dev[:, :3] if scored else
                   torch.from_numpy(np.ascontiguousarray(rows[..., :3], dtype=np.float32)).to(device))
    return target_dev, nn, None if pcl_target_frame is None else nn_labels(*nn, thresh)


def nn_target(points_query_xyz, target_xyz):
    """(idx (N,) int32, dist (N,)) on the device: the nearest target point of every query.  Streaming k = 1 kernel."""
    idx, dist = ops.knn(points_query_xyz, target_xyz, 1, metric=1, return_dist=True)
    return idx[:, 0], dist[:, 0]


def nn_labels(idx, dist, thresh):
    """The host arrays of get_1nn_label from a search's device results."""
    return (dist < thresh).cpu().numpy() * 1, idx.cpu().numpy().astype(np.int64)


def get_1nn_label(points_query_xyz, pcl_target_frame, thresh, device):
    """Pseudo label of every query from its nearest target point (utils/geometry.py:444-455, an sklearn
    KDTree there): label = (distance < thresh), plus the neighbour's index.  Streaming k = 1 kernel."""
    return _target_frame(points_query_xyz, pcl_target_frame, thresh, device)[2]


def multi_track_merge(track_instance_ids, pcl_abstract, features_global, implicit_output, output_track_idx):
    """Merge the per-instance reruns (utils/utils.py:343-397): features and outputs are averaged, the
    mark_track channel becomes the id of the most confident run (>= 0.5), else -1."""
    assert len(pcl_abstract) == len(features_global) == len(implicit_output)
    if len(pcl_abstract) == 1 and track_instance_ids[0] == -1:
        return (pcl_abstract[0], features_global[0], implicit_output[0])
    merged_abstract = np.mean(pcl_abstract, axis=0) if pcl_abstract[0] is not None else None
    merged_global = np.mean(features_global, axis=0)
    merged_output = np.mean(implicit_output, axis=0)
    winner = -np.ones_like(merged_output[..., 0])
    best = np.zeros_like(merged_output[..., 0])
    for inst_id, out in zip(track_instance_ids, implicit_output):
        score = out[..., output_track_idx]
        winner[np.logical_and(score >= 0.5, score >= best)] = inst_id
        best = np.maximum(score, best)
    merged_output[..., output_track_idx] = winner
    return (merged_abstract, merged_global, merged_output)


def infer_device(pcl_input, points_query, pcl_net, implicit_net, batch_size, color_mode,
                 predict_segmentation=False, track_mode='none', semantic_classes=13, encoded=None,
                 neighbour_lists=None, squash=True, refine=None, grid_counts=None):
    """Device-resident core of perform_inference: encode once, decode every mini-batch, squash.
    All tensors are CUDA; returns CUDA tensors (implicit_output (N,G), pcl_abstract (M,3+E),
    features_global (D)).  squash=False: implicit_output holds the network's RAW outputs (the caller squashes).
    refine: a GridRefine for points_query = the (nx, ny, nz) = `grid_counts` grid: two decode passes and the expansion stand
    in for the dense decode (decode_refined), and the result gains 'refine' = dict(n_queries, n_decoded)."""
    n = points_query.shape[0]
    prelude = None
    if encoded is not None:
        (pcl_abstract, features_global) = encoded
    else:
        if neighbour_lists is None and refine is None:
            prelude = QueryPrelude.start(pcl_input, points_query, 0, n, pcl_net, implicit_net)
        (pcl_abstract, features_global, _) = pcl_net(pcl_input, False)
        if pcl_abstract is not None:
            pcl_abstract = pcl_abstract.squeeze(0)
        features_global = features_global.squeeze(0)
    out = torch.empty((n, implicit_net.d_out), dtype=torch.float32, device=points_query.device)
    lists = None
    if neighbour_lists is not None:
        lists = tuple(None if a is None else torch.as_tensor(a).to(points_query.device) for a in neighbour_lists)
        assert len(lists) == 2 and all(a is None or a.shape[0] == n for a in lists)
    codes = squash_codes(implicit_net.d_out, color_mode, predict_segmentation, track_mode, semantic_classes)
    res = dict(implicit_output=out, pcl_abstract=pcl_abstract, features_global=features_global)
    if refine is None:
        decode_batches(implicit_net, points_query, 0, n, batch_size, pcl_abstract, features_global, out, lists=lists,
                       prelude=prelude)
    else:
        assert lists is None and grid_counts is not None, 'refine: no neighbour_lists, and the grid counts of points_query'
        res['refine'] = decode_refined(implicit_net, points_query, grid_counts, refine, batch_size, pcl_abstract,
                                       features_global, out, codes[0])
    if squash:                           # (on copied rows too: the squash of a copy is the copy of the squashed row)
        ops.squash(out, codes)
    return res


# A decoded row's bits depend on ONE thing beside the query itself: its slot in the mini-batch.  The fused attention kernel packs
# 9 consecutive queries of a mini-batch per workgroup (DECODE_ALIGN below), and the ninth of them (position % 9 == 8) takes
# another reduction order than the first eight: the two kinds of slot differ in the last bits (4.8e-7 at most on the tracking
# fixture), rows within a kind do not, and neither the batch's length nor a shift by a multiple of 9 changes anything.  The
# gathered passes of the coarse-to-fine decode therefore give every query a slot of the kind it has in the dense decode.
SLOT_PERIOD = 9
ODD_SLOT = 8


def _dense_slot_is_odd(grid_index, chunk):
    """Whether the dense decode (mini-batches of `chunk` rows from row 0) puts grid row `grid_index` into a ninth slot."""
    return (grid_index % chunk) % SLOT_PERIOD == ODD_SLOT


def _like_slots(odd):
    """odd (m,) bool, in batch order -> slot (m,) int64: a position of its own for every row, whose kind is the row's -- the
    ninth slots 8, 17, 26, ... for the odd rows, the other positions 0 .. 7, 9 .. 16, ... for the rest, each kind in the rows'
    order.  The batch that holds them has `_slots_len(rows of the other kind, odd rows)` rows; the positions no row takes are
    padding."""
    odd = odd.to(torch.int64)
    odd_rank = torch.cumsum(odd, 0) - odd
    other_rank = torch.arange(odd.shape[0], dtype=torch.int64, device=odd.device) - odd_rank
    return torch.where(odd.bool(), odd_rank * SLOT_PERIOD + ODD_SLOT, other_rank + other_rank // (SLOT_PERIOD - 1))


def _slots_len(n_other, n_odd):
    last_other = (n_other - 1) + (n_other - 1) // (SLOT_PERIOD - 1) if n_other > 0 else -1
    last_odd = (n_odd - 1) * SLOT_PERIOD + ODD_SLOT if n_odd > 0 else -1
    return max(last_other, last_odd) + 1


def _slot_batch(batch_size):
    """(the dense decode's mini-batch length, the batch_size of a gathered pass: the largest one below it that keeps a row's
    position in its mini-batch congruent to its position in the pass modulo 9)."""
    chunk = decode_chunk(batch_size)
    gathered = chunk - chunk % SLOT_PERIOD if chunk >= SLOT_PERIOD else chunk
    assert decode_chunk(gathered) % SLOT_PERIOD == 0 or gathered < SLOT_PERIOD, 'OCC4D_DECODE_ALIGN must be a multiple of 9'
    return chunk, gathered


def _decode_in_slots(implicit_net, rows, slot, length, filler, batch_size, pcl_abstract, features_global, g):
    """Decodes rows (m, 4) at the positions `slot` (m,) of a batch of `length` rows (the rest: copies of the query `filler`)
    -> their (m, g) raw outputs."""
    batch = filler.expand(length, rows.shape[1]).contiguous()
    batch.index_copy_(0, slot, rows)
    out = torch.empty((length, g), dtype=torch.float32, device=rows.device)
    decode_batches(implicit_net, batch, 0, length, batch_size, pcl_abstract, features_global, out)
    return ops.gather_rows(out, slot.to(torch.int32))


@functools.lru_cache(maxsize=8)
def _grid_plan(counts, block, chunk, device):
    """What depends on the grid alone: (flat grid index of every block's representative, in flat block order, (blocks,) int32;
    the representatives' slots (blocks,) int64 and the length of their batch; (n,) float32: 1.0 where the dense decode puts the
    grid row into a ninth slot), on `device`."""
    axes = []
    for n in counts:
        first = torch.arange((n + block - 1) // block, dtype=torch.int64) * block + block // 2
        axes.append(torch.clamp(first, max=n - 1))
    nx, ny, nz = counts
    rep = ((axes[0][:, None, None] * ny + axes[1][None, :, None]) * nz + axes[2][None, None, :]).reshape(-1)
    rep_odd = _dense_slot_is_odd(rep, chunk)
    n_odd = int(rep_odd.sum())
    grid_odd = _dense_slot_is_odd(torch.arange(nx * ny * nz, dtype=torch.int64), chunk).to(torch.float32)
    return (rep.to(torch.int32).to(device), _like_slots(rep_odd).to(device), _slots_len(rep.shape[0] - n_odd, n_odd),
            grid_odd.to(device))


def decode_refined(implicit_net, points_query, counts, refine, batch_size, pcl_abstract, features_global, out, density_op):
    """The coarse-to-fine decode of the (nx, ny, nz) = `counts` grid `points_query` into the dense `out` (N, G), RAW outputs:
    the representatives' OWN rows of the grid tensor are gathered and decoded, the mark selects (on the raw density with its
    squash code `density_op`), the order-preserving compaction gathers the selected rows, they are decoded, and one pass
    expands.  Mini-batches are independent and every gathered query is decoded in a mini-batch slot of the kind the dense
    decode gives it (SLOT_PERIOD above; a few padding rows fill the slots no query takes), so every decoded row has the
    dense decode's bits.  One device->host read per call: the selected count and, with it, the count of ninth-slot rows
    among them.  -> dict(n_queries, n_decoded): n_decoded counts the representatives and the selected rows, not the padding."""
    counts = tuple(int(c) for c in counts)
    n, g = out.shape
    assert points_query.shape[0] == n == counts[0] * counts[1] * counts[2], \
        'points_query holds %d rows, the grid %s' % (points_query.shape[0], counts)
    chunk, gathered = _slot_batch(batch_size)
    rep_rows, rep_slot, rep_len, grid_odd = _grid_plan(counts, refine.block, chunk, points_query.device)
    filler = points_query[:1]
    rep_out = _decode_in_slots(implicit_net, ops.gather_rows(points_query, rep_rows), rep_slot, rep_len, filler, gathered,
                               pcl_abstract, features_global, g)
    key, _ = ops.refine_mark(rep_out[:, 0], counts, refine.block, refine.dilate, refine.low, op=density_op)
    # the selected rows with their kind of slot as a fifth column; the two counts in one read
    tagged = torch.cat([points_query, grid_odd[:, None]], dim=1)
    fine_rows, count, offsets = ops.compact_rows_with_offsets(tagged, key, 0.5, sync=False)
    n_fine, n_odd = (int(v) for v in torch.stack([count[0].to(torch.int64), (key * grid_odd).sum(dtype=torch.float64).to(torch.int64)]).tolist())
    fine_out = None
    if n_fine > 0:
        fine_rows = fine_rows[:n_fine]
        fine_out = _decode_in_slots(implicit_net, fine_rows[:, :4].contiguous(), _like_slots(fine_rows[:, 4] > 0.5),
                                    _slots_len(n_fine - n_odd, n_odd), filler, gathered, pcl_abstract, features_global, g)
    ops.refine_expand(key, offsets, rep_out, fine_out, counts, refine.block, out=out)
    return dict(n_queries=n, n_decoded=rep_rows.shape[0] + n_fine)


# decode streams: kernels.Selection.decode_streams (default 2, OCC4D_DECODE_STREAMS; 1 = the reference's strictly serial loop)
# The fused attention kernel packs 9 queries per workgroup and one workgroup occupies a CU (129 KB LDS): a mini-batch
# of 9 * 256 * r queries is exactly r full rounds of the 256 CUs.  The caller's batch_size (a memory knob in the
# reference) is rounded DOWN to such a multiple (32768 -> 32256: 14 full rounds instead of 14.2 -> 15); every query
# is still decoded, results do not depend on the split (tests).  0 disables.
DECODE_ALIGN = int(os.environ.get('OCC4D_DECODE_ALIGN', str(9 * 256)))


def decode_chunk(batch_size):
    if DECODE_ALIGN > 0 and batch_size >= DECODE_ALIGN:
        return batch_size - batch_size % DECODE_ALIGN
    return batch_size


def _decode_into(implicit_net, q, pcl_abstract, features_global, out_rows, lists=None, prelude=None):
    """One mini-batch: the network's raw outputs written into `out_rows`.  The library-backed decoder writes them in
    place and skips the penultimate activation perform_inference discards (eval/inference.py:211); any other module
    with the reference's forward signature is called as the reference calls it.  `prelude`: (buffers, first row, end row)
    of a QueryPrelude for these very queries."""
    direct = getattr(implicit_net, 'forward_output_only', None)
    kw = {} if lists is None else dict(knn_local=lists[0], knn_cross=lists[1])
    if direct is not None and getattr(implicit_net, 'num_local_features', 0) > 0 and q.dim() == 2 and q.shape[0] > 0:
        if prelude is not None:
            kw['prelude'] = prelude
        direct(q, pcl_abstract, features_global, None, out_rows, **kw)
        return
    assert prelude is None
    (o, _) = implicit_net(q, pcl_abstract, features_global, None, **kw)
    out_rows.copy_(o)


class QueryPrelude:
    """The decode's query front end issued BEFORE the encoder: the searches, the interpolation
    weights and lin_in of points_query[lo:hi] need the abstract cloud's coordinates only, and those exist a few hundred
    microseconds into the encoder's sampling chain (PointCompletionNetV3.abstract_xyz_early) -- so one native pass over all
    rows (LocalPclResnetFC.query_prelude) runs on a side stream while the rest of that single-workgroup chain would leave
    the device empty.  Order of issue: start() (early coordinates + the pass, both on the side stream), then the encoder,
    then decode_batches(prelude=...), whose mini-batches wait for `done`.  Ordering is by stream events only.
    start() returns None wherever the path does not apply (kernels.Selection.query_prelude off, host tensors or the CPU
    twin, a decoder without the library path, an encoder whose sampling is not the deterministic nested chain); the
    decode then runs its front end per mini-batch as before."""

    def __init__(self, buffers, lo, hi, done):
        self.buffers, self.lo, self.hi, self.done = buffers, lo, hi, done

    @classmethod
    def start(cls, pcl_input, points_query, lo, hi, pcl_net, implicit_net):
        if not (kernels.scope().query_prelude and hi > lo and torch.is_tensor(pcl_input) and pcl_input.is_cuda
                and points_query.is_cuda and points_query.dim() == 2 and hasattr(pcl_net, 'abstract_xyz_early')
                and hasattr(implicit_net, 'query_prelude') and getattr(implicit_net, 'num_local_features', 0) > 0
                and implicit_net._library_path_ok() and not ops._lib.is_twin()
                and not implicit.needs_grad(implicit_net) and not implicit.needs_grad(pcl_net, pcl_input)):
            return None
        # (the second decode stream: idle until the second mini-batch, and no further hardware queue)
        side = side_streams(points_query.device, 'decode', 2)[1]
        early = pcl_net.abstract_xyz_early(pcl_input, stream=side)      # (waits for the work queued on the current stream:
        if early is None:                                               #  the last decode that read the buffers is among it)
            return None
        xyz, _ = early
        with torch.cuda.stream(side):
            buffers = implicit_net.query_prelude(points_query[lo:hi], xyz)
            done = torch.cuda.Event()
            done.record(side)
        return cls(buffers, lo, hi, done)


def decode_batches(implicit_net, points_query, lo, hi, batch_size, pcl_abstract, features_global, out, out_offset=0,
                   lists=None, prelude=None):
    """Runs implicit_net on points_query[lo:hi] in mini-batches of `batch_size` (the reference's
    loop, eval/inference.py:204-246) and writes rows into out[out_offset:].  Mini-batches are
    independent, so consecutive ones alternate between `decode_streams` (kernels.Selection) HIP streams: a 32768-query
    batch is exactly one wave of 256 workgroups for the row-tiled kernels, and the next batch's
    kernels fill the tail of the previous one's instead of waiting behind it.  The first batch runs
    on the caller's stream so the per-scene tables are built (and cached) before the side streams
    start.  `prelude`: the QueryPrelude started for exactly these rows, or None."""
    batch_size = decode_chunk(batch_size)
    starts = list(range(lo, hi, batch_size))
    n_streams = kernels.scope().decode_streams if points_query.is_cuda else 1      # (host tensors: the explicit CPU twin)
    main = torch.cuda.current_stream() if points_query.is_cuda else None
    side = side_streams(points_query.device, 'decode', n_streams) if n_streams > 1 and len(starts) > 2 else []
    if prelude is not None:
        assert lists is None and (prelude.lo, prelude.hi) == (lo, hi)
        main.wait_event(prelude.done)                    # (the side streams wait for `main` behind the first mini-batch)

    def rows(b, e):           # the caller's neighbour lists of these queries (rows are indexed like points_query)
        return None if lists is None else tuple(None if a is None else a[b:e] for a in lists)

    def pre(b, e):
        return None if prelude is None else (prelude.buffers, b - lo, e - lo)

    for bi, b in enumerate(starts):
        e = min(hi, b + batch_size)
        if bi == 0 or not side:
            _decode_into(implicit_net, points_query[b:e], pcl_abstract, features_global, out[out_offset + b - lo:out_offset + e - lo],
                         rows(b, e), pre(b, e))
            if bi == 0:
                for st in side:
                    st.wait_stream(main)
            continue
        st = side[bi % len(side)]
        with torch.cuda.stream(st):
            _decode_into(implicit_net, points_query[b:e], pcl_abstract, features_global, out[out_offset + b - lo:out_offset + e - lo],
                         rows(b, e), pre(b, e))
    for st in side:
        main.wait_stream(st)
    if prelude is not None:
        prelude.buffers['released'] = main.record_event()        # (the next prelude overwrites the buffers behind this)
    return out
