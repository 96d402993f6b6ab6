"""The clip front end: RGB-D frames (GREATER) / lidar sweeps (CARLA) -> the clouds the networks and the training step take,
built on the device (the rest of the per-clip dataloader geometry).

``greater_clip`` restates data/data_greater.py:386-516 and :528-567 of the reference, ``carla_clip`` data/data_carla.py:443-623:
unprojection / lidar transform, instance ids from the flat render's hue, cuboid filters, per-frame random subsampling, time
accumulation, view merge, shuffles, farthest-point subsampling.  The element-wise steps are the two kernels of
include/occ4d_frontend.h, selections are the order-preserving compaction, shuffles and subsamples are row gathers, the
final reduction is geometry.subsample_pad_pcl_torch.  The frames, every intermediate cloud and the results stay on the
device; the host reads one vector of frame counts per view (carla_clip: one more for the kept counts of all target frames
after the output cuboid).

Every random number comes from numpy's or torch's GLOBAL CPU generator in the reference's call order (the per-frame
np.random.choice draws, the shuffles -- drawn as np.random.shuffle of arange(n), which consumes the generator exactly as
shuffling the (n, D) array does --, the torch.randint start of the farthest-point sampling), so equal seeds give the
reference's clouds bit for bit (tests/golden/frontend_*.npz).

With ``live_occl_mode`` ('unfilt' / 'normal') the clip functions also give the loader's ``valo_ids``, ``num_valo_ids`` and
``live_occl`` (get_valo_ids, data/data_utils.py:12-100), with ``track_mode`` greater_clip chooses ``track_id`` as data/
data_greater.py:534-552 does (occlusion.py): the id histograms run on buffers the clip holds anyway ('unfilt': the raw rows and
their keep key, no compacted copy) and all tables are fetched in ONE further device -> host read.

Out of scope: file I/O and image decoding, the dataset classes, the occlusion-biased clip choice (sample_bias='occl' reads
occl.txt from the dataset).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, geometry, occlusion, ops


def _device_f32(a, device, name, shape_tail=None):
    """`a` (numpy array or tensor) as a contiguous fp32 tensor on `device`."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    assert isinstance(t, torch.Tensor), '%s must be a numpy array or a tensor' % name
    assert shape_tail is None or tuple(t.shape[-len(shape_tail):]) == tuple(shape_tail), \
        '%s must end in %s, got %s' % (name, tuple(shape_tail), tuple(t.shape))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _host_f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


def inverse_4x4(m):
    """np.linalg.inv of float32 (3, 3) intrinsics / (3, 4) extrinsics / (4, 4) matrices embedded in eye(4), one matrix at a
    time as the reference inverts them (utils/geometry.py:42-59): (..., 4, 4) float32."""
    m = _host_f32(m)
    lead = m.shape[:-2]
    out = np.empty(lead + (4, 4), dtype=np.float32)
    for i in np.ndindex(*lead):
        full = np.eye(4, dtype=np.float32)
        full[:m.shape[-2], :m.shape[-1]] = m[i]
        out[i] = np.linalg.inv(full)
    return out


def rgbd_rows(depth, rgb, flat, k_inv, rt_inv, hue_clusters, bounds, floor_fix=True, view_idx=0, want_target=False):
    """occ4d_rgbd_rows_f32 for the T frames of one view (device tensors; k_inv / rt_inv (T, 4, 4)): -> rows (T H W, 8) =
    (x, y, z, instance, R, G, B, t), target rows (T H W, 8) = (x, y, z, instance, view, R, G, B) or None, keep key (T H W)."""
    depth = ops._dev(depth, name='depth')
    assert depth.dim() == 3, 'depth must be (T, H, W), got %s' % (tuple(depth.shape),)
    T, H, W = depth.shape
    assert tuple(rgb.shape) == (T, H, W, 3), 'rgb must be (T, H, W, 3) = %s, got %s' % ((T, H, W, 3), tuple(rgb.shape))
    assert flat is None or tuple(flat.shape) == (T, H, W, 3), 'flat must be (T, H, W, 3), got %s' % (tuple(flat.shape),)
    assert tuple(k_inv.shape) == (T, 4, 4) and tuple(rt_inv.shape) == (T, 4, 4), 'k_inv / rt_inv must be (T, 4, 4)'
    assert len(bounds) == 6
    tensors = [ops._dev(t.contiguous(), name=n) for t, n in ((depth, 'depth'), (rgb, 'rgb'), (k_inv, 'k_inv'), (rt_inv, 'rt_inv'))]
    flat = None if flat is None else ops._dev(flat.contiguous(), name='flat')
    clusters = None
    if flat is not None:
        clusters = ops._dev(hue_clusters.contiguous(), name='hue_clusters')
        assert clusters.dim() == 1
    n = T * H * W
    rows = torch.empty((n, 8), dtype=torch.float32, device=depth.device)
    target = torch.empty((n, 8), dtype=torch.float32, device=depth.device) if want_target else None
    key = torch.empty((n,), dtype=torch.float32, device=depth.device)
    _lib.check(_lib.lib().occ4d_rgbd_rows_f32(
        ops._ptr(tensors[0]), ops._ptr(tensors[1]), ops._ptr(flat), ops._ptr(tensors[2]), ops._ptr(tensors[3]),
        ops._ptr(clusters), 0 if clusters is None else clusters.numel(), T, H, W, *[float(b) for b in bounds],
        int(bool(floor_fix)), int(view_idx), ops._ptr(rows), ops._ptr(target), ops._ptr(key), ops._stream()))
    return rows, target, key


def lidar_rows(rows, source_matrix=None, inv_target_matrix=None, z_offset=0.0, cube_mode=0, min_z=-0.5, other_bounds=20.0,
               out=None, out_key=None):
    """occ4d_lidar_rows_f32 for one sweep (N, D) on the device: -> (rows (N, D) with xyz transformed / offset, keep key (N)).
    The two (4, 4) matrices are host float32 arrays (inv_target_matrix already inverted) or both None; `out`: a row-strided
    (N, >= D) destination (the caller's wider buffer), `out_key`: a contiguous (N) destination for the key."""
    r, ld = ops._rows(ops._dev(rows, name='rows'), 'rows')
    n, d = r.shape
    assert d >= 3, 'lidar rows must start with x, y, z, got %d columns' % d
    assert (source_matrix is None) == (inv_target_matrix is None)
    assert cube_mode in (0, 1, 2, 3, 4), 'cube_mode must be 0 (no filter) or 1 .. 4, got %r' % (cube_mode,)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=r.device)
    o, ldo = ops._rows(ops._dev(out, name='out'), 'out')
    assert o is out and o.shape[0] == n and o.shape[1] >= d
    key = torch.empty((n,), dtype=torch.float32, device=r.device) if out_key is None else ops._dev(out_key, name='out_key')
    assert tuple(key.shape) == (n,) and key.is_contiguous(), 'out_key must be a contiguous (N) tensor'
    mats = [None, None]
    if source_matrix is not None:
        mats = [np.ascontiguousarray(m, dtype=np.float32) for m in (source_matrix, inv_target_matrix)]
        assert mats[0].shape == (4, 4) and mats[1].shape == (4, 4), 'lidar transforms must be (4, 4)'
    ptrs = [C.c_void_p(m.ctypes.data) if m is not None else C.c_void_p(0) for m in mats]
    _lib.check(_lib.lib().occ4d_lidar_rows_f32(ops._ptr(r), ld, n, d, ptrs[0], ptrs[1], float(z_offset), int(cube_mode),
                                               float(min_z), float(other_bounds), ops._ptr(o), ldo, ops._ptr(key), ops._stream()))
    return out[:, :d] if out.shape[1] != d else out, key


class _Segments:
    """Order-preserving compaction of consecutive row segments (frames) by one key vector: the counts stay on the device
    until read() fetches all of them in ONE transfer; rows() then compacts any row tensor that shares the key."""

    def __init__(self, key, bounds):
        self.key, self.bounds = key, bounds                           # bounds: [(lo, hi)] row ranges
        self.scratch, st = [], ops._stream()
        for lo, hi in bounds:
            n = hi - lo
            nb = (n + 255) // 256
            s = torch.zeros(nb + 1, dtype=torch.int32, device=key.device)
            if n:
                _lib.check(_lib.lib().occ4d_compact_count_f32(ops._ptr(key[lo:hi]), 1, n, 0.5, 1, ops._ptr(s), ops._ptr(s[nb:]), st))
            self.scratch.append(s)

    def totals(self):
        return torch.cat([s[-1:] for s in self.scratch])              # (segments,) int32 on the device

    def rows(self, src, seg, kept):
        """Segment `seg` of the row tensor `src` compacted: (kept, D); `kept` = its count as read from totals()."""
        lo, hi = self.bounds[seg]
        d = src.shape[1]
        out = torch.empty((kept, d), dtype=torch.float32, device=src.device)
        if kept:
            _lib.check(_lib.lib().occ4d_compact_rows_f32(ops._ptr(src[lo:hi]), src.stride(0), hi - lo, d, ops._ptr(self.key[lo:hi]), 1,
                                                         0.5, 1, ops._ptr(self.scratch[seg]), ops._ptr(out), None, ops._stream()))
        return out


def _take(rows, inds):
    """rows[inds] for a host integer index array, on the gather kernel."""
    if len(inds) == 0:
        return rows[:0]
    return ops.gather_rows(rows, torch.from_numpy(np.ascontiguousarray(inds, dtype=np.int32)).to(rows.device))


def _subsample_frame(n, n_points_rnd):
    """subsample_pad_pcl_numpy's draw for a frame of n rows: ascending indices, or None when the frame is kept whole."""
    if n_points_rnd > 0 and n > n_points_rnd:
        inds = np.random.choice(n, n_points_rnd, replace=False)
        inds.sort()
        return inds
    return None


def _shuffled(rows):
    """np.random.shuffle(rows) without the rows on the host: the same permutation drawn on arange(n), as a gather."""
    perm = np.arange(rows.shape[0])
    np.random.shuffle(perm)
    return _take(rows, perm) if rows.shape[0] else rows


def _cat(parts, d, device):
    parts = [p for p in parts if p.shape[0]]
    return torch.cat(parts, dim=0) if parts else torch.empty((0, d), dtype=torch.float32, device=device)


def _finish(all_input, all_target, n_fps_input, n_fps_target, pcl_input_frames, pcl_target_frames, n_sem, track_id,
            target_inst_col, target_filter=None, retain_vehped=False, segm_idx=None, occl=None):
    """The common tail of both loaders.  all_input: list-T of the source view's rows (x, y, z, sem..., R, G, B, t);
    all_target: list-T of list-V of rows (x, y, z, sem..., view, R, G, B); target_filter(frame) -> keep key (m) on the device:
    an order-preserving selection of every shuffled target frame, the kept counts of all frames read in ONE transfer.
    occl: the clip's occlusion.ClipCounts or None; its one read comes after every random draw of the clip, and a track id it
    chooses replaces `track_id`."""
    device = all_input[0].device
    meta = dict(sample_input_ratios=[], sample_target_ratios=[])
    pcl_input = _shuffled(_cat(all_input[:pcl_input_frames], all_input[0].shape[1], device))
    pre = pcl_input.shape[0]
    pcl_input = geometry.subsample_pad_pcl_torch(pcl_input, n_fps_input, sample_mode='farthest_point', subsample_only=False)
    post = pcl_input.shape[0]
    meta['sample_input_ratios'].append(post / max(pre, 1))
    meta['pcl_input_size'] = min(pre, post)

    T = len(all_target)
    pcl_target, counts = [], []
    for t in range(pcl_target_frames):
        views = all_target[T - pcl_target_frames + t]
        frame = _shuffled(_cat(views, views[0].shape[1], device))
        if target_filter is not None:
            frame, count = ops.compact_rows_nosync(frame, target_filter(frame), 0.5, strict=True)
            counts.append(count)
        pcl_target.append(frame)
    if counts:
        counts = torch.cat(counts).cpu().numpy()                                       # ONE device -> host read
        pcl_target = [frame[:int(n)] for frame, n in zip(pcl_target, counts)]
    sizes = [frame.shape[0] for frame in pcl_target]
    if n_fps_target != 0:
        mode = 'farthest_point' if n_fps_target > 0 else 'random'
        for i in range(pcl_target_frames):
            pre = pcl_target[i].shape[0]
            pcl_target[i] = geometry.subsample_pad_pcl_torch(pcl_target[i], abs(n_fps_target), sample_mode=mode,
                                                             subsample_only=False, retain_vehped=retain_vehped, segm_idx=segm_idx)
            post = pcl_target[i].shape[0]
            meta['sample_target_ratios'].append(post / max(pre, 1))
            sizes[i] = min(pre, post)
    meta['pcl_target_size'] = sizes

    if occl is not None:
        extra = occl.finish(pcl_input)
        track_id = extra.get('track_id', track_id)
        meta.update(extra)
    pcl_input_sem = pcl_input[:, 3:3 + n_sem]
    track_in = torch.zeros_like(pcl_input[:, 0:1])
    track_tg = [torch.zeros_like(f[:, 0:1]) for f in pcl_target]
    if track_id is not None and track_id >= 0:                  # (first input frame in time, every target frame)
        track_in = torch.logical_and(pcl_input_sem[:, 0] == track_id, pcl_input[:, -1] == 0).to(torch.float32)[:, None]
        track_tg = [(f[:, target_inst_col] == track_id).to(torch.float32)[:, None] for f in pcl_target]
    pcl_input = torch.cat([pcl_input[:, :3], pcl_input[:, -4:], track_in], dim=-1)
    pcl_target = [torch.cat([f, m], dim=-1) for f, m in zip(pcl_target, track_tg)]
    return pcl_input, pcl_input_sem.contiguous(), pcl_target, meta


def greater_clip(rgb, flat, depth, cam_RT, cam_K, hue_clusters, other_bounds=5.0, min_z=-1.0, n_points_rnd=0,
                 n_fps_input=14336, n_fps_target=14336, pcl_input_frames=12, pcl_target_frames=12, src_view=0, track_id=-1,
                 device=None, live_occl_mode=None, track_mode=None, max_valo_ids=32, occl_n_ids=None):
    """RGB-D frames of V views and T times -> (pcl_input (n, 8) = (x, y, z, R, G, B, t, mark_track), pcl_input_sem (n, 1) =
    (instance_id), pcl_target list of (m, 9) = (x, y, z, instance_id, view_idx, R, G, B, mark_track), meta_data) on the device.
    rgb, flat (V, T, H, W, 3), depth (V, T, H, W), cam_RT (V, T, 3, 4), cam_K (V, T, 3, 3): numpy arrays or tensors (tensors on
    the device are used in place).  meta_data: pcl_sizes (V, T), cuboid_filter_ratios, sample_input_ratios,
    sample_target_ratios, pcl_input_size, pcl_target_size.
    live_occl_mode 'unfilt' (counts over the un-subsampled clouds; needs pcl_input_frames == T) or 'normal' (over the subsampled
    ones): meta_data gains valo_ids (max_valo_ids, int32, padded with -1), num_valo_ids, live_occl (pcl_input_frames,
    max_valo_ids) and track_id (occlusion.valo_ids).  track_mode 'none' / 'snitch' / 'random': `track_id` is ignored, the id is
    chosen as the reference's loader does (occlusion.choose_track_id; 'random' draws np.random.choice AFTER every other draw of
    the clip) and stands in meta_data['track_id'].  occl_n_ids: bins of the id histogram (default: len(hue_clusters)).  Either
    argument costs the clip ONE more device -> host read; with both None nothing changes."""
    return _greater_clip(rgb, flat, depth, cam_RT, cam_K, hue_clusters, other_bounds, min_z, n_points_rnd, n_fps_input,
                         n_fps_target, pcl_input_frames, pcl_target_frames, src_view, track_id, device, None,
                         live_occl_mode, track_mode, max_valo_ids, occl_n_ids)


def _greater_clip(rgb, flat, depth, cam_RT, cam_K, hue_clusters, other_bounds, min_z, n_points_rnd, n_fps_input, n_fps_target,
                  pcl_input_frames, pcl_target_frames, src_view, track_id, device, stages, live_occl_mode=None, track_mode=None,
                  max_valo_ids=32, occl_n_ids=None):
    """greater_clip; `stages` (private, the stage-by-stage tests): a dict that receives references to the intermediate
    clouds the function builds anyway -- it never changes the work done."""
    if device is None:
        device = depth.device if isinstance(depth, torch.Tensor) else torch.device('cpu' if _lib.is_twin() else 'cuda')
    depth = _device_f32(depth, device, 'depth')
    assert depth.dim() == 4, 'depth must be (V, T, H, W), got %s' % (tuple(depth.shape),)
    V, T, H, W = depth.shape
    rgb = _device_f32(rgb, device, 'rgb', (T, H, W, 3))
    flat = None if flat is None else _device_f32(flat, device, 'flat', (T, H, W, 3))
    assert rgb.shape[0] == V and (flat is None or flat.shape[0] == V), 'rgb / flat must have V = %d views' % V
    cam_RT, cam_K = _host_f32(cam_RT), _host_f32(cam_K)
    assert cam_RT.shape == (V, T, 3, 4), 'cam_RT must be (V, T, 3, 4), got %s' % (cam_RT.shape,)
    assert cam_K.shape == (V, T, 3, 3), 'cam_K must be (V, T, 3, 3), got %s' % (cam_K.shape,)
    assert 1 <= pcl_input_frames <= T and 1 <= pcl_target_frames <= T and 0 <= src_view < V
    clusters = None if flat is None else _device_f32(np.asarray(hue_clusters, dtype=np.float32), device, 'hue_clusters')
    k_inv = torch.from_numpy(inverse_4x4(cam_K)).to(device)
    rt_inv = torch.from_numpy(inverse_4x4(cam_RT)).to(device)
    ob = float(other_bounds)
    bounds = (-ob, ob, -ob, ob, float(min_z), ob)

    occl = None
    if live_occl_mode is not None or track_mode is not None:
        n_ids = occl_n_ids if occl_n_ids is not None else (1 if clusters is None else max(1, clusters.numel()))
        occl = occlusion.ClipCounts(live_occl_mode, track_mode, V, T, pcl_input_frames, src_view, False, 0, None, 3, max_valo_ids,
                                    n_ids, device)
    keep_frames = occl is not None and live_occl_mode is not None and not occl.unfilt      # ('normal': every subsampled frame)
    meta = dict(cuboid_filter_ratios=[])
    pcl_sizes = np.zeros((V, T), dtype=np.int64)
    all_input, all_target = None, [[None] * V for _ in range(T)]
    first_target = T - pcl_target_frames
    for v in range(V):
        rows, target, key = rgbd_rows(depth[v], rgb[v], None if flat is None else flat[v], k_inv[v], rt_inv[v], clusters, bounds,
                                      floor_fix=True, view_idx=v, want_target=True)
        seg = _Segments(key, [(t * H * W, (t + 1) * H * W) for t in range(T)])
        if occl is not None and occl.unfilt:                      # the kept rows where they lie: frame segments known on the host
            occl.add_view(v, rows, [t * H * W for t in range(T + 1)], key=key)
        view_frames = []
        valid = (depth[v] > 0).reshape(T, -1).sum(dim=1).to(torch.int32)
        counts = torch.cat([seg.totals(), valid]).cpu().numpy()                        # the view's ONE device -> host read
        kept, pre_filter = counts[:T], counts[T:]
        view_input = []
        for t in range(T):
            meta['cuboid_filter_ratios'].append(int(kept[t]) / max(int(pre_filter[t]), 1))
            inds = _subsample_frame(int(kept[t]), n_points_rnd)
            frame_in = frame_tg = None
            if v == src_view and t < pcl_input_frames:
                frame_in = seg.rows(rows, t, int(kept[t]))
                frame_in = frame_in if inds is None else _take(frame_in, inds)
                view_input.append(frame_in)
            if t >= first_target:
                frame_tg = seg.rows(target, t, int(kept[t]))
                all_target[t][v] = frame_tg if inds is None else _take(frame_tg, inds)
            pcl_sizes[v, t] = int(kept[t]) if inds is None else len(inds)
            if keep_frames:
                if frame_in is None:
                    frame_in = seg.rows(rows, t, int(kept[t]))
                    frame_in = frame_in if inds is None else _take(frame_in, inds)
                view_frames.append(frame_in)
            if stages is not None:
                stages[('kept', v, t)] = int(kept[t])
                stages[('subsample', v, t)] = inds
                stages[('frame', v, t)] = frame_in
                stages[('frame_target', v, t)] = all_target[t][v]
        if stages is not None:
            stages[('rows', v)], stages[('key', v)] = rows, key
        if keep_frames:
            occl.add_view(v, *occlusion._frames(view_frames))
        if v == src_view:
            all_input = view_input
    meta['pcl_sizes'] = pcl_sizes
    pcl_input, sem, pcl_target, tail = _finish(all_input, all_target[first_target:], n_fps_input, n_fps_target, pcl_input_frames,
                                               pcl_target_frames, 1, track_id, 3, occl=occl)
    meta.update(tail)
    return pcl_input, sem, pcl_target, meta


def carla_clip(lidar, sensor_RT, reference_frame=None, correct_origin_ground=True, min_z=-1.0, other_bounds=20.0,
               target_bounds=16.0, cube_mode=4, n_points_rnd=0, n_fps_input=14336, n_fps_target=14336, pcl_input_frames=12,
               pcl_target_frames=12, oversample_vehped_target=False, track_id=-1, device=None, live_occl_mode=None,
               max_valo_ids=256, occl_n_ids=None):
    """Lidar sweeps -> the CARLA clouds on the device.  lidar: list-V of list-T of (N, 9) rows (x, y, z, cosine_angle,
    instance_id, semantic_tag, R, G, B) (numpy or tensors); sensor_RT (T, V, 4, 4): sensor-to-world matrices of the clip's
    frames; reference_frame: index of the clip frame whose forward (view 0) sensor is the common frame, None = every frame's
    own.  Returns (pcl_input (n, 8) = (x, y, z, R, G, B, t, mark_track), pcl_input_sem (n, 3) = (cosine_angle, instance_id,
    semantic_tag), pcl_target list of (m, 11) = (x, y, z, cosine_angle, instance_id, semantic_tag, view_idx, R, G, B,
    mark_track), meta_data as greater_clip).  The input is view 0 (data/data_carla.py:523-529).  Host reads: the T frame
    counts once per view, and the kept counts of all target frames after the output cuboid once.
    live_occl_mode 'unfilt' / 'normal': meta_data gains valo_ids, num_valo_ids and live_occl over the vehicle / pedestrian
    instances (occlusion.valo_ids; occl_n_ids: bins of the id histogram, default OCC4D_OCCL_MAX_IDS) for ONE more read."""
    V, T = len(lidar), len(lidar[0])
    sensor_RT = _host_f32(sensor_RT)
    assert sensor_RT.shape == (T, V, 4, 4), 'sensor_RT must be (T, V, 4, 4) = %s, got %s' % ((T, V, 4, 4), sensor_RT.shape)
    assert all(len(view) == T for view in lidar), 'every view needs T = %d sweeps' % T
    assert 1 <= pcl_input_frames <= T and 1 <= pcl_target_frames <= T
    assert reference_frame is None or -T <= reference_frame < T
    if device is None:
        first = lidar[0][0]
        device = first.device if isinstance(first, torch.Tensor) else torch.device('cpu' if _lib.is_twin() else 'cuda')
    z_offset = 1.0 if correct_origin_ground else 0.0            # (the hard-coded sensor height, data/data_carla.py:461-463)
    filter_mode = cube_mode if cube_mode in (1, 2, 3, 4) else 0

    occl = None
    if live_occl_mode is not None:
        occl = occlusion.ClipCounts(live_occl_mode, None, V, T, pcl_input_frames, 0, True, 1, 2, 4, max_valo_ids,
                                    occlusion.MAX_IDS if occl_n_ids is None else occl_n_ids, device)
    keep_frames = occl is not None and not occl.unfilt
    meta = dict(cuboid_filter_ratios=[])
    pcl_sizes = np.zeros((V, T), dtype=np.int64)
    first_target = T - pcl_target_frames
    all_input, all_target = [], [[None] * V for _ in range(T)]
    for v in range(V):
        sweeps = [_device_f32(lidar[v][t], device, 'lidar[%d][%d]' % (v, t)) for t in range(T)]
        assert all(s.dim() == 2 and s.shape[1] == sweeps[0].shape[1] and s.shape[1] >= 3 for s in sweeps), \
            'lidar sweeps must be (N, D >= 3) with one D'
        d = sweeps[0].shape[1]
        offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in sweeps])])
        buf = torch.empty((int(offsets[-1]), d + 1), dtype=torch.float32, device=device)      # (..., t): accumulate_pcl_time
        key = torch.empty((int(offsets[-1]),), dtype=torch.float32, device=device)
        for t in range(T):
            ref_t = t if reference_frame is None else range(T)[reference_frame]
            src = inv = None
            if t != ref_t or v != 0:
                src = sensor_RT[t, v]
                inv = np.linalg.inv(sensor_RT[ref_t, 0])
            lo, hi = int(offsets[t]), int(offsets[t + 1])
            if hi > lo:
                lidar_rows(sweeps[t], src, inv, z_offset, filter_mode, min_z, other_bounds, out=buf[lo:hi], out_key=key[lo:hi])
                ops.fill_rows(buf[lo:hi, d:], float(t))
        seg = _Segments(key, [(int(offsets[t]), int(offsets[t + 1])) for t in range(T)])
        if occl is not None and occl.unfilt:
            occl.add_view(v, buf, offsets, key=key)
        view_frames = []
        kept = seg.totals().cpu().numpy()                                              # the view's ONE device -> host read
        for t in range(T):
            n_t = int(offsets[t + 1] - offsets[t])
            meta['cuboid_filter_ratios'].append(int(kept[t]) / max(n_t, 1))
            inds = _subsample_frame(int(kept[t]), n_points_rnd)
            pcl_sizes[v, t] = int(kept[t]) if inds is None else len(inds)
            need_in, need_tg = v == 0 and t < pcl_input_frames, t >= first_target
            frame = None
            if need_in or need_tg or keep_frames:
                frame = seg.rows(buf, t, int(kept[t]))
                frame = frame if inds is None else _take(frame, inds)
            if keep_frames:
                view_frames.append(frame)
            if need_in:
                all_input.append(frame)
            if need_tg:                                                                # merge_pcl_views_numpy(insert_view_idx)
                all_target[t][v] = torch.cat([frame[:, :d - 3], torch.full_like(frame[:, :1], float(v)), frame[:, d - 3:d]], dim=1)
        if keep_frames:
            occl.add_view(v, *occlusion._frames(view_frames))
    meta['pcl_sizes'] = pcl_sizes

    def output_cuboid(frame):              # filter_pcl_bounds_carla_output_torch(padding = 2) as a keep key for the compaction
        sx, sy, sz = geometry._CARLA_OUTPUT_SCALE[cube_mode]
        ob, pad = target_bounds, 2.0
        keep = torch.ones(frame.shape[0], dtype=torch.bool, device=frame.device)
        for col, lo, hi in ((0, 0.0 - pad, ob * sx + pad), (1, -ob * sy - pad, ob * sy + pad), (2, min_z, ob * sz)):
            keep = keep & (lo <= frame[:, col]) & (frame[:, col] <= hi)
        return keep.to(torch.float32)

    n_sem = all_input[0].shape[1] - 3 - 4                       # (what stands between xyz and R, G, B, t)
    pcl_input, sem, pcl_target, tail = _finish(all_input, all_target[first_target:], n_fps_input, n_fps_target, pcl_input_frames,
                                               pcl_target_frames, n_sem, track_id, 4,
                                               target_filter=output_cuboid if cube_mode in geometry._CARLA_OUTPUT_SCALE else None,
                                               retain_vehped=oversample_vehped_target, segm_idx=5, occl=occl)
    meta.update(tail)
    return pcl_input, sem, pcl_target, meta
