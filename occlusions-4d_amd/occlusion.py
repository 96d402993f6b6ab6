"""Per-instance visibility on the device: the ids that are visible at least once ("valo ids"), the live occlusion fraction
of every instance in every input frame, and the choice of the instance to track.

``valo_ids`` restates data/data_utils.py:12-100 of the reference (get_valo_ids), ``choose_track_id`` data/data_greater.py:534-552.
Where the reference scans every frame once per id with ``(column == id).sum()``, one pass of the segmented id histogram
(ops.id_histogram, include/occ4d_occl.h) counts every id of every frame; all tables of a call sit in ONE device buffer that is
read with ONE device -> host transfer, and the fractions are formed on the host in float64 from the integer tables, in the
reference's operation order.  Counts are integers: there is no tolerance anywhere.

The histogram has bins for the ids 0 .. n_ids - 1.  When a counted input row holds anything else that is not negative (an id
>= n_ids, a non-integral value), the call takes the STEP-BY-STEP path (``_stepwise_*`` below): torch.unique on the device, then
one mask per id, as the reference does it.  It gives the same results and is allowed to be slow; the sampler's "ids outside
0 .. 63" path in geometry.py works the same way.
"""
import numpy as np
import torch

from . import _lib, ops

MAX_IDS = _lib.OCCL_CONSTANTS['MAX_IDS']
_EXTRA = _lib.OCCL_CONSTANTS['EXTRA_BINS']
_OTHER = _lib.OCCL_CONSTANTS['OTHER']
VEHPED_TAGS = (4.0, 10.0)                          # 4 = pedestrian, 10 = vehicles (data/data_utils.py:65)
TRACK_MIN_POINTS = 16                              # data/data_greater.py:540-542


class Tables:
    """The histograms of one call: every add() launches one ops.id_histogram into the next rows of one device buffer;
    read() fetches what was filled in ONE device -> host transfer and hands out the tables by name as int64 arrays."""

    def __init__(self, n_ids, capacity, device):
        self.n_ids = int(n_ids)
        self.buf = torch.zeros((int(capacity), self.n_ids + _EXTRA), dtype=torch.int32, device=device)
        self.used, self.where = 0, {}

    def add(self, name, rows, col, seg_offsets, key=None, pred_col=-1, pred_values=()):
        S = len(seg_offsets) - 1
        assert self.used + S <= self.buf.shape[0] and name not in self.where
        ops.id_histogram(rows, col, seg_offsets, self.n_ids, key=key, pred_col=pred_col, pred_values=pred_values,
                         out=self.buf[self.used:self.used + S])
        self.where[name] = (self.used, self.used + S)
        self.used += S

    def read(self):
        host = self.buf[:self.used].cpu().numpy().astype(np.int64)                     # the call's ONE device -> host read
        return {name: host[lo:hi] for name, (lo, hi) in self.where.items()}


def _frames(frames):
    """list of (N_t, D) device tensors -> (their concatenation, the host row offsets)."""
    offsets = np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int64)
    return (frames[0] if len(frames) == 1 else torch.cat(list(frames), dim=0)), offsets


def _min_points(live_occl_mode):
    if 'unfilt' in live_occl_mode:
        return 16
    if 'normal' in live_occl_mode:
        return 8
    raise ValueError(live_occl_mode)


def live_occlusion(input_counts, src_counts, merged_counts, min_points, pcl_input_frames, video_length, num_views, max_valo_ids):
    """The host part of get_valo_ids from the integer tables.  input_counts (bins): the (vehicle / pedestrian) input rows per
    id; src_counts (T, bins): the source view's frames; merged_counts (T, bins): the merged frames.  The tables may be arrays or
    dicts id -> count (the step-by-step path).  -> (live_occl, valo_ids_pad, num_valo_ids)."""
    if isinstance(input_counts, dict):
        ids = sorted(i for i, c in input_counts.items() if i >= 0 and c >= min_points)
        count = lambda table, t, i: int(table[t].get(i, 0))
    else:
        n_ids = len(input_counts) - _EXTRA
        ids = [i for i in range(n_ids) if input_counts[i] >= min_points]
        count = lambda table, t, i: int(table[t][i])
    # An id is a valo id when it is >= 0 and its count in the (vehicle / pedestrian) input rows reaches the minimum.  The
    # reference draws its candidates from unique() of the int32-cast column and keeps those whose `== id` count reaches the
    # minimum (>= 8): every id with such a count is among the candidates, and a candidate that only arose from the cast
    # (2 from 2.5) has to pass the same count.  unique() adds nothing to the rule; it only makes the ids ascend.
    num = len(ids)
    if num > max_valo_ids:
        raise IndexError('%d valo ids do not fit max_valo_ids = %d (the reference fails here with an IndexError on live_occl)'
                         % (num, max_valo_ids))
    live_occl = np.zeros((pcl_input_frames, max_valo_ids))
    for i, vis_id in enumerate(ids):
        c_max = -1
        for t in range(video_length):
            c_max = max(count(merged_counts, t, vis_id), c_max)
        for t in range(pcl_input_frames):
            c_in = count(src_counts, t, vis_id)
            live_occl[t, i] = max(1.0 - c_in * num_views / (c_max + 1e-6), 0.0)
    valo_ids_pad = -np.ones(max_valo_ids, dtype=np.int32)
    valo_ids_pad[:num] = ids
    return live_occl, valo_ids_pad, num


def _vehped_mask(sem, sem_cat_col):
    return torch.logical_or(sem[..., sem_cat_col] == VEHPED_TAGS[0], sem[..., sem_cat_col] == VEHPED_TAGS[1])


def valo_ids(live_occl_mode, filter_vehped, sem_inst_col, sem_cat_col, merged_inst_col, pcl_input_frames, video_length, src_view,
             num_views, max_valo_ids, all_pcl, pcl_input_sem, pcl_merged_frames, n_ids=None):
    """get_valo_ids (data/data_utils.py:12-100) on device tensors.
      all_pcl: list-V of list-T of (N, D) clouds, (x, y, z, instance_id, R, G, B) for GREATER, (x, y, z, cosine_angle,
        instance_id, semantic_tag, R, G, B) for CARLA -- the un-subsampled clouds for 'unfilt', the subsampled ones for 'normal';
      pcl_input_sem (n, 1 / 3): the input cloud's semantic columns ('normal' counts over it AS GIVEN, with the zero rows that
        padding added: they count for id 0, as in the reference; 'unfilt' does not read it);
      pcl_merged_frames: list-T of the merged frames or None ('normal': the merged count of frame t is then the sum over the
        views of all_pcl, which is what merging is; 'unfilt' always counts over all_pcl, as the reference does);
      filter_vehped, sem_inst_col, sem_cat_col, merged_inst_col: False, 0, None, 3 for GREATER; True, 1, 2, 4 for CARLA;
      n_ids: bins of the histogram (default OCC4D_OCCL_MAX_IDS = 4096).
    -> (live_occl float64 (pcl_input_frames, max_valo_ids), valo_ids_pad int32 (max_valo_ids) padded with -1, num_valo_ids,
    vehped_mask: device bool tensor over the input rows, or None).  'unfilt' takes at least 16 input points per id and
    pcl_input_frames == video_length, 'normal' 8; any other mode raises ValueError; more than max_valo_ids valo ids raise
    IndexError.  One device -> host read.  Ids the histogram has no bin for send the call down the step-by-step path
    (_stepwise_valo_ids: torch.unique and one mask per id on the device; same results, slow)."""
    min_points = _min_points(live_occl_mode)
    unfilt = 'unfilt' in live_occl_mode
    V, T = len(all_pcl), video_length
    assert all(len(view) == T for view in all_pcl), 'every view of all_pcl needs video_length = %d frames' % T
    assert 0 <= src_view < V and 1 <= pcl_input_frames <= T
    n_ids = MAX_IDS if n_ids is None else int(n_ids)
    device = all_pcl[0][0].device
    if unfilt:
        assert pcl_input_frames == video_length
        src_rows, src_off = _frames(all_pcl[src_view])
        input_rows, input_off, input_col = src_rows, src_off, 3 + sem_inst_col          # nss_input[..., 3:-4]
        cat_col = None if not filter_vehped else 3 + sem_cat_col
        used_input_sem = src_rows[:, 3:]
    else:
        input_rows, input_off, input_col = pcl_input_sem, np.array([0, pcl_input_sem.shape[0]]), sem_inst_col
        cat_col = None if not filter_vehped else sem_cat_col
        used_input_sem = pcl_input_sem
    mask = _vehped_mask(used_input_sem, sem_cat_col) if filter_vehped else None

    merged_given = (not unfilt) and pcl_merged_frames is not None
    assert not merged_given or len(pcl_merged_frames) == T
    views = [src_view] if merged_given else list(range(V))
    shared = unfilt and cat_col is None and input_col == merged_inst_col      # (GREATER: the input table IS the source view's)
    tables = Tables(n_ids, len(input_off) - 1 + len(views) * T + (T if merged_given else 0), device)
    if not shared:
        tables.add('input', input_rows, input_col, input_off, pred_col=-1 if cat_col is None else cat_col,
                   pred_values=() if cat_col is None else VEHPED_TAGS)
    for v in views:
        rows, off = (src_rows, src_off) if unfilt and v == src_view else _frames(all_pcl[v])
        tables.add(('view', v), rows, merged_inst_col, off)
    if merged_given:
        rows, off = _frames(pcl_merged_frames)
        tables.add('merged', rows, merged_inst_col, off)
    host = tables.read()
    input_counts = host[('view', src_view) if shared else 'input'].sum(axis=0)
    if input_counts[n_ids + _OTHER] != 0:                        # an id without a bin among the counted input rows
        return _stepwise_valo_ids(min_points, input_rows[:, input_col], mask, all_pcl, pcl_merged_frames if merged_given else None,
                                  merged_inst_col, pcl_input_frames, video_length, src_view, num_views, max_valo_ids) + (mask,)
    merged = host['merged'] if merged_given else sum(host[('view', v)] for v in views)
    return live_occlusion(input_counts, host[('view', src_view)], merged, min_points, pcl_input_frames, video_length, num_views,
                          max_valo_ids) + (mask,)


def _stepwise_ids(column):
    """The ids >= 0 of a device column with their `== id` counts, the reference's way: {id: count}.  Candidates are the
    integral, finite values >= 0 (another value equals no integer); one device -> host read."""
    c = column.reshape(-1)
    c = c[torch.isfinite(c) & (c >= 0) & (c == torch.floor(c))]
    ids, counts = torch.unique(c.to(torch.float64), return_counts=True)
    both = torch.stack([ids, counts.to(torch.float64)]).cpu().numpy()
    return {int(i): int(n) for i, n in zip(both[0], both[1])}


def _stepwise_valo_ids(min_points, input_column, mask, all_pcl, merged_frames, inst_col, pcl_input_frames, video_length, src_view,
                       num_views, max_valo_ids):
    """The step-by-step path of valo_ids: unique ids of the input rows, then one mask per id and frame, on the device."""
    input_counts = _stepwise_ids(input_column if mask is None else input_column[mask])
    ids = sorted(i for i, c in input_counts.items() if c >= min_points)
    src, merged = [dict() for _ in range(video_length)], [dict() for _ in range(video_length)]
    if ids:
        sums = []
        for vis_id in ids:
            for t in range(video_length):
                if merged_frames is not None:
                    per_view = [(merged_frames[t][:, inst_col] == vis_id).sum()]
                else:
                    per_view = [(view[t][:, inst_col] == vis_id).sum() for view in all_pcl]
                sums += [torch.stack(per_view).sum(), (all_pcl[src_view][t][:, inst_col] == vis_id).sum()]
        sums = torch.stack(sums).cpu().numpy().reshape(len(ids), video_length, 2)
        for k, vis_id in enumerate(ids):
            for t in range(video_length):
                merged[t][vis_id], src[t][vis_id] = int(sums[k, t, 0]), int(sums[k, t, 1])
    return live_occlusion(input_counts, src, merged, min_points, pcl_input_frames, video_length, num_views, max_valo_ids)


def track_id_from_counts(first_counts, track_mode):
    """The choice of data/data_greater.py:534-552 from the id counts of the first input frame (an array over the bins, or a
    dict id -> count).  'random' makes exactly one np.random.choice draw on numpy's global generator, and only when an id
    qualifies."""
    if track_mode not in ('none', 'snitch', 'random'):
        raise ValueError(track_mode)
    if track_mode == 'none':
        return -1
    if isinstance(first_counts, dict):
        vis_ids = sorted(i for i, c in first_counts.items() if i >= 0 and c >= TRACK_MIN_POINTS)
    else:
        vis_ids = [i for i in range(len(first_counts) - _EXTRA) if first_counts[i] >= TRACK_MIN_POINTS]
    if not vis_ids:
        return -1
    if track_mode == 'snitch':
        return 0
    return int(np.random.choice(np.asarray(vis_ids, dtype=np.int32)))


def choose_track_id(pcl_input, pcl_input_sem, track_mode, n_ids=None):
    """The instance to track (data/data_greater.py:534-552): pcl_input (n, 7) = (x, y, z, R, G, B, t) -- the time is the LAST
    column --, pcl_input_sem (n, 1) = (instance_id), on the device.  The candidates are the ids >= 0 with at least 16 points in
    the first input frame (t == 0): 'none' -> -1; 'snitch' -> 0 if any id qualifies, else -1; 'random' -> np.random.choice of
    them (one draw on numpy's global generator, none when the list is empty); anything else raises ValueError.  One histogram
    call with the t == 0 predicate, one device -> host read (ids without a bin: the step-by-step path, _stepwise_ids)."""
    if track_mode not in ('none', 'snitch', 'random'):
        raise ValueError(track_mode)
    if track_mode == 'none':
        return -1
    n_ids = MAX_IDS if n_ids is None else int(n_ids)
    pair = torch.stack([pcl_input_sem[:, 0], pcl_input[:, -1]], dim=1)                  # (instance_id, t)
    counts = ops.id_histogram(pair, 0, [0, pair.shape[0]], n_ids, pred_col=1, pred_values=(0.0,)).cpu().numpy()[0]
    if counts[n_ids + _OTHER] != 0:
        counts = _stepwise_ids(pair[:, 0][pair[:, 1] == 0])
    return track_id_from_counts(counts, track_mode)


class ClipCounts:
    """What frontend.greater_clip / carla_clip collect for the live occlusion fractions and the track choice: the per-view
    tables are launched while the clip is built (no count is read), finish() adds the tables over the finished input cloud
    and fetches everything in the clip's ONE extra device -> host read."""

    def __init__(self, live_occl_mode, track_mode, V, T, pcl_input_frames, src_view, filter_vehped, sem_inst_col, sem_cat_col,
                 inst_col, max_valo_ids, n_ids, device):
        if track_mode is not None and track_mode not in ('none', 'snitch', 'random'):
            raise ValueError(track_mode)
        self.mode, self.track_mode = live_occl_mode, track_mode
        self.min_points = None if live_occl_mode is None else _min_points(live_occl_mode)
        self.unfilt = live_occl_mode is not None and 'unfilt' in live_occl_mode
        assert not self.unfilt or pcl_input_frames == T, "live_occl_mode 'unfilt' needs pcl_input_frames == video_length"
        self.V, self.T, self.frames, self.src_view = V, T, pcl_input_frames, src_view
        self.vehped, self.sem_inst_col, self.sem_cat_col, self.inst_col = filter_vehped, sem_inst_col, sem_cat_col, inst_col
        self.max_valo_ids, self.n_ids = max_valo_ids, int(n_ids)
        self.tables = Tables(n_ids, (V + 1) * T + 2, device)
        self.sources = [None] * V

    def add_view(self, v, rows, offsets, key=None):
        """View v's clouds as one row array (x, y, z, sem..., ...) with the frames' row offsets; `key`: the keep key of raw
        rows ('unfilt' counts the kept rows where they lie: no compacted copy) or None for frames already selected."""
        if self.mode is None:
            return
        offsets = np.asarray(offsets, dtype=np.int64)
        self.sources[v] = (rows, offsets, key)
        self.tables.add(('view', v), rows, self.inst_col, offsets, key=key)
        if self.unfilt and v == self.src_view and self.vehped:
            self.tables.add('input', rows, self.inst_col, offsets, key=key, pred_col=3 + self.sem_cat_col, pred_values=VEHPED_TAGS)

    def _source_frames(self, v):
        rows, off, key = self.sources[v]
        out = []
        for t in range(self.T):
            f = rows[int(off[t]):int(off[t + 1])]
            out.append(f if key is None else f[key[int(off[t]):int(off[t + 1])] > 0.5])
        return out

    def finish(self, pcl_input):
        """pcl_input (n, 3 + n_sem + 4) = (x, y, z, sem..., R, G, B, t), the finished input cloud -> the meta entries
        (valo_ids, num_valo_ids, live_occl; track_id when a track mode was given)."""
        n, t_col = pcl_input.shape[0], pcl_input.shape[1] - 1
        inst = 3 + self.sem_inst_col
        if self.mode is not None and not self.unfilt:
            cat = () if not self.vehped else VEHPED_TAGS
            self.tables.add('input', pcl_input, inst, [0, n], pred_col=3 + self.sem_cat_col if self.vehped else -1, pred_values=cat)
        choose = self.track_mode is not None and self.track_mode != 'none'
        if choose:
            self.tables.add('first', pcl_input, inst, [0, n], pred_col=t_col, pred_values=(0.0,))
        host = self.tables.read() if self.tables.used else {}
        other = self.n_ids + _OTHER
        meta = {}
        if self.mode is not None:
            shared = 'input' not in host
            input_counts = host[('view', self.src_view) if shared else 'input'].sum(axis=0)
            if input_counts[other] != 0:                         # ids without a bin: the step-by-step path
                all_pcl = [self._source_frames(v) for v in range(self.V)]
                if self.unfilt:
                    sem = torch.cat(all_pcl[self.src_view], dim=0)[:, 3:]
                else:
                    sem = pcl_input[:, 3:]
                mask = _vehped_mask(sem, self.sem_cat_col) if self.vehped else None
                res = _stepwise_valo_ids(self.min_points, sem[:, self.sem_inst_col], mask, all_pcl, None, self.inst_col, self.frames,
                                         self.T, self.src_view, self.V, self.max_valo_ids)
            else:
                merged = sum(host[('view', v)] for v in range(self.V))
                res = live_occlusion(input_counts, host[('view', self.src_view)], merged, self.min_points, self.frames, self.T, self.V,
                                     self.max_valo_ids)
            meta['live_occl'], meta['valo_ids'], meta['num_valo_ids'] = res
        if self.track_mode is not None:
            counts = None
            if choose:
                counts = host['first'][0]
                if counts[other] != 0:
                    counts = _stepwise_ids(pcl_input[:, inst][pcl_input[:, t_col] == 0])
            meta['track_id'] = track_id_from_counts(counts, self.track_mode)
        return meta
