"""Training step on the HIP library (BASELINE config 5).

The reference's train loop (train.py:38-159) wraps a pipeline whose call arity does not match the
published models, so the step is restated against model/ signatures: encode the
point-cloud video, decode supervision query points of every target frame, sum the implicit
losses of loss.py (density BCE :50-64, colour :66-154 (L1 on RGB, or the hsv / bins classification forms), segmentation CE :156-173, tracking
BCE :175-194), backward through occlusions4d_amd.autograd, all-reduce gradients across ranks
(one process per GPU, RCCL) instead of nn.DataParallel, clip, AdamW step.

torch supplies the tape, the loss reductions, the optimiser and torch.distributed; every network
forward and backward kernel is libocc4d.so.  Query points and their targets are inputs of the step;
the training-time point sampler that draws them (utils/geometry.py:578-1105, rank 2 of 8(f)) is
geometry.GuidedImplicitPointSampler (bench_train.py --sampler runs it inside the step).
"""
import copy
import math
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import autograd, kernels, ops
from .point_transformer_layer import invalidate_weight_caches


FUSED_LOSS = os.environ.get('OCC4D_FUSED_LOSS', '1') == '1'      # the loss terms, value and gradient, as one library call (csrc/loss.hip)


def _masked_mean(values, mask):
    """mean of values[mask] without data-dependent shapes (capturable in a hipGraph); same value up to fp32
    summation order."""
    m = mask.to(values.dtype)
    while m.dim() < values.dim():
        m = m[..., None]
    return (values * m).sum() / (m.sum() * (values.numel() // mask.numel()))


def squash_for_loss(implicit_output, color_mode):
    """The pre-loss squashing of the training pipeline (pipeline.py:198-212): density stays a logit (BCE with
    logits follows); 'rgb' -> sigmoid of channels 1:4, 'rgb_nosigmoid' -> clamp to [0, 1] (so no gradient
    flows through colours outside [0, 1]), 'hsv' -> clamp of (S, V), 'bins' -> nothing.  Out of place."""
    if color_mode == 'rgb':
        mid = torch.sigmoid(implicit_output[..., 1:4])
    elif color_mode == 'rgb_nosigmoid':
        mid = torch.clamp(implicit_output[..., 1:4], min=0.0, max=1.0)
    elif color_mode == 'hsv':
        return torch.cat([implicit_output[..., :13], torch.clamp(implicit_output[..., 13:15], min=0.0, max=1.0),
                          implicit_output[..., 15:]], dim=-1)
    elif color_mode == 'bins':
        return implicit_output
    else:
        raise ValueError('Unknown color_mode: ' + str(color_mode))
    return torch.cat([implicit_output[..., :1], mid, implicit_output[..., 4:]], dim=-1)


TRACK_IDX = {'rgb': 4, 'rgb_nosigmoid': 4, 'hsv': 15, 'bins': 10}      # utils.get_track_idx (utils/utils.py:204-224)


def rgb_to_hsv(rgb, epsilon=1e-10):
    """(N, 3) -> (N, 3) hue in degrees, saturation, value: the reference's own arithmetic (utils/utils.py:169-191)."""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    max_rgb = rgb.max(1)[0]
    min_rgb, argmin = rgb.min(1)
    max_min = max_rgb - min_rgb + epsilon
    h1 = 60.0 * (g - r) / max_min + 60.0
    h2 = 60.0 * (b - g) / max_min + 180.0
    h3 = 60.0 * (r - b) / max_min + 300.0
    h = torch.stack((h2, h3, h1), dim=0).gather(0, argmin[None])[0]
    return torch.stack((h, max_min / (max_rgb + epsilon), max_rgb), dim=1)


def _color_term(o, y, keep, color_mode, static_shapes):
    """implicit_color_loss (loss.py:66-154) of one (example, frame): o (N, G) squashed outputs, y (N, 6) targets, keep
    (N) = solid AND colour available.  static_shapes: masked means instead of boolean indexing (capturable)."""
    if color_mode in ('rgb', 'rgb_nosigmoid'):                                   # :78-83: L1 on (R, G, B)
        if static_shapes:
            return _masked_mean((o[:, 1:4] - y[:, 1:4]).abs(), keep)
        return F.l1_loss(o[keep, 1:4], y[keep, 1:4])
    if not static_shapes:
        o, y = o[keep], y[keep]
        keep = torch.ones(o.shape[0], dtype=torch.bool, device=o.device)
    hsv = rgb_to_hsv(y[:, 1:4])                      # (rows outside `keep` carry -1 colours: finite junk, masked out)
    sat, val = hsv[:, 1], hsv[:, 2]

    def bins(n):                                                                 # :93-97 / :121-125
        hue = torch.round(hsv[:, 0] / 360.0 * n).to(torch.int64)
        hue = torch.where(hue == n, torch.zeros_like(hue), hue)
        return hue.clamp(0, n - 1) if static_shapes else hue

    def mean(values, mask):
        if static_shapes:
            m = mask.to(values.dtype)
            return (values * m).sum() / m.sum().clamp(min=1.0)
        return values[mask].mean()
    if color_mode == 'hsv':                                                      # :85-114
        hue = bins(12)
        hm = keep & (sat >= 0.2) & (val >= 0.2)        # hue is not supervised where it is too bland / too dark
        ce = F.cross_entropy(o[:, 1:13], hue, reduction='none')
        if static_shapes:
            loss_hue = torch.where(hm.sum() >= 16, mean(ce, hm) / 2.0, ce.new_zeros(()))
        else:
            loss_hue = ce[hm].mean() / 2.0 if int(hm.sum()) >= 16 else 0.0
        return (loss_hue + mean((o[:, 13] - sat).abs(), keep) + mean((o[:, 14] - val).abs(), keep)) / 3.0
    assert color_mode == 'bins'                                                  # :116-149
    target = bins(6)
    bland = (sat < 0.3) | (val < 0.3)
    target = torch.where((val < 0.2) & bland, torch.full_like(target, 6), target)
    target = torch.where((0.2 <= val) & (val < 0.6) & bland, torch.full_like(target, 7), target)
    target = torch.where((0.6 <= val) & bland, torch.full_like(target, 8), target)
    return mean(F.cross_entropy(o[:, 1:10], target, reduction='none'), keep) / 3.0


def _fused_loss_layout(g, color_mode, semantic_classes, density_lw, color_lw, segmentation_lw, tracking_lw):
    """Whether occ4d_implicit_loss_terms_f32 takes this channel layout (its argument contract, include/occ4d.h): the weighted
    terms' channels exist and the segmentation classes sit behind them.  Anything else stays on the torch path below."""
    if min(density_lw, color_lw, segmentation_lw, tracking_lw) < 0.0:
        return False
    used = 1
    if color_lw > 0.0:
        used = TRACK_IDX[color_mode]              # (one past the last colour channel)
    if tracking_lw > 0.0:
        used = TRACK_IDX[color_mode] + 1
    if g < used:
        return False
    return segmentation_lw <= 0.0 or 1 <= semantic_classes <= g - used


def implicit_loss(implicit_output, implicit_target, density_lw=1.0, color_lw=0.0, segmentation_lw=0.0,
                  tracking_lw=0.0, color_mode='rgb', semantic_classes=13, static_shapes=False, squashed=False,
                  return_terms=False):
    """loss.MyLosses.per_example + entire_batch (loss.py:200-294) on the RAW decoder outputs.

    implicit_output (T,N,G) or (T,B,N,G) logits (density, R, G, B, mark_track, segm?); implicit_target
    (T,[B,]N,6) with (density, R, G, B, mark_track, segm).  As the reference: the outputs are squashed first
    (squash_for_loss, pipeline.py:198-212; skipped when `squashed`), every term is the mean over its supervised
    points of ONE (example, frame) -- density BCE on all points (:50-64); colour L1 where density >= 0.1 AND
    colour available, target[..., 1] >= 0 (:72-83); segmentation CE where label >= 0 (:156-173); tracking BCE
    where density >= 0.1 AND mark_track >= 0 (:175-194) -- the per-(example, frame) values are averaged
    (:243-250) and summed with their weights (:276-277).
    static_shapes=True computes the masked means by weighting instead of boolean indexing (no host sync, no
    data-dependent shapes): the form a captured step needs, and the one the eager step uses to avoid its host reads.
    return_terms=True: (total, terms) with terms a detached (4,) tensor on the outputs' device -- the unweighted colour /
    density / segmentation / tracking means the reference logs every step (:255-294), 0 for a term without weight; no
    host read is added for it."""
    if implicit_output.dim() == 3:
        implicit_output, implicit_target = implicit_output[:, None], implicit_target[:, None]
    if color_mode not in TRACK_IDX:
        raise ValueError('Unknown color_mode: ' + str(color_mode))
    track_idx = TRACK_IDX[color_mode]    # the tracking logit sits behind the colour channels (utils.get_track_idx)
    if (FUSED_LOSS and implicit_output.is_cuda and not ops._lib.is_twin() and not (squashed and color_lw > 0.0)
            and implicit_output.dtype == torch.float32 and implicit_target.dtype == torch.float32
            and implicit_target.shape[-1] == 6
            and _fused_loss_layout(implicit_output.shape[-1], color_mode, semantic_classes, density_lw, color_lw,
                                   segmentation_lw, tracking_lw)):
        # every weighted term, the squash included, value and gradient, as one library call of two launches (csrc/loss.hip;
        # the two-term form of round 6 replaced ~60 element-wise launches and 6.6 ms of host time per step); same means over
        # the same points as the eager form below (an empty selection gives a non-finite total in both)
        (nf, nb, n, g) = implicit_output.shape
        total, terms = autograd.ImplicitLossTermsFn.apply(
            implicit_output.reshape(nf * nb, n, g).contiguous(), implicit_target.reshape(nf * nb, n, 6).contiguous(),
            color_mode, int(semantic_classes), float(density_lw), float(color_lw), float(segmentation_lw), float(tracking_lw))
        return (total, terms) if return_terms else total
    if not squashed and color_lw > 0.0:
        implicit_output = squash_for_loss(implicit_output, color_mode)
    total = implicit_output.new_zeros(())
    sums = [0.0, 0.0, 0.0, 0.0]          # (colour, density, segmentation, tracking) over the cells, for return_terms
    (nf, nb) = implicit_output.shape[:2]
    cells = nf * nb
    for t in range(nf):
        for b in range(nb):
            o, y = implicit_output[t, b], implicit_target[t, b]
            solid = y[:, 0] >= 0.1
            if density_lw > 0.0:
                term = F.binary_cross_entropy_with_logits(o[:, 0], y[:, 0])
                sums[1] = sums[1] + term.detach()
                total = total + density_lw * term / cells
            if color_lw > 0.0:
                term = _color_term(o, y, solid & (y[:, 1] >= 0.0), color_mode, static_shapes)
                sums[0] = sums[0] + term.detach()
                total = total + color_lw * term / cells
            if segmentation_lw > 0.0:
                lab = y[:, -1].to(torch.int64)
                keep = lab >= 0
                if static_shapes:
                    ce = F.cross_entropy(o[:, -semantic_classes:], lab.clamp(min=0), reduction='none')
                    term = _masked_mean(ce, keep)
                else:
                    term = F.cross_entropy(o[keep][:, -semantic_classes:], lab[keep])
                sums[2] = sums[2] + term.detach()
                total = total + segmentation_lw * term / cells
            if tracking_lw > 0.0:
                keep = solid & (y[:, 4] >= 0.0)
                if static_shapes:
                    bce = F.binary_cross_entropy_with_logits(o[:, track_idx], y[:, 4].clamp(min=0.0),
                                                             reduction='none')
                    term = _masked_mean(bce, keep)
                else:
                    term = F.binary_cross_entropy_with_logits(o[keep, track_idx], y[keep, 4])
                sums[3] = sums[3] + term.detach()
                total = total + tracking_lw * term / cells
    if not return_terms:
        return total
    zero = total.new_zeros(())
    return total, torch.stack([s if torch.is_tensor(s) else zero for s in sums]).detach() / cells


class Participation:
    """Which parameters some rank produced a gradient for, as agreed in the last eager step of ONE training-step object
    (the mask lives on the TrainStep, not in a module-level table keyed by id(): ids are recycled after a model is
    freed).  `used` is None until an eager agreement exists."""

    def __init__(self):
        self.used = None

    def clear(self):
        """Forget the agreement: the next eager step of EVERY rank agrees again (call it on all ranks at the same point
        of the program -- an epoch boundary, after freezing / unfreezing parameters)."""
        self.used = None


def allreduce_gradients(params, world=None, participation=None):
    """Average gradients over ranks with ONE flat all-reduce (28.8 MB for the 7.21 M parameters:
    latency/bandwidth of a single bucket; xGMI is point to point, so few large messages).  `participation`: the
    caller's Participation record; a captured step REQUIRES one that an eager step has filled."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    world = world or dist.get_world_size()
    params = [p for p in params if p.requires_grad]
    if not params:
        return
    # Which parameters take part is agreed first (one small MAX all-reduce of a has-gradient mask): a parameter
    # without a gradient on THIS rank must still be reduced (as zeros) when another rank produced one -- every rank
    # reduces the same flat layout -- but one that NO rank used keeps grad = None, so that the optimiser skips it
    # (no weight decay, no moment update), exactly as in a single-process run and as under the reference's
    # nn.DataParallel (train.py:305).
    # The agreement needs one host read (a stall of the launching thread, and forbidden inside a stream capture), so it is
    # made ONCE per Participation record -- the first eager step -- and reused by every later step, eager or captured,
    # until the caller clears it (round 5; round 4 agreed again in every eager step).  All ranks run the same program, so
    # they agree / reuse at the same steps.  The set of parameters that receive gradients is a property of the model
    # graph (which heads and losses are switched on), not of the data; a parameter that turns up with a gradient after
    # the agreement excluded it is a program error and raises instead of silently skipping its reduction.
    capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    if participation is not None and participation.used is not None and len(participation.used) == len(params):
        used = participation.used
        late = [i for i, (p, u) in enumerate(zip(params, used)) if p.grad is not None and not u]
        if late:
            raise RuntimeError('allreduce_gradients: %d parameter(s) received a gradient after the ranks agreed that nobody '
                               'uses them; call Participation.clear() on every rank when the set of trained parameters '
                               'changes' % len(late))
    elif capturing:
        raise AssertionError('a captured step needs the participation mask of a preceding eager step '
                             '(run one eager step before capturing)')
    else:
        has = torch.tensor([0.0 if p.grad is None else 1.0 for p in params], device=params[0].device)
        dist.all_reduce(has, op=dist.ReduceOp.MAX)
        used = [bool(v) for v in has.tolist()]
        if participation is not None:
            participation.used = used
    grads = []
    for p, u in zip(params, used):
        if u:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad)
    if not grads:
        return
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat /= world
    off = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[off:off + n].view_as(g))
        off += n


class SideStreamSampler:
    """Draws the supervision points of the NEXT training step on a side stream while the current step runs.

    The reference samples inside the step on the training stream (pipeline.py:118-161 calls
    GuidedImplicitPointSampler per target frame before the forward pass); the points depend on the target frames and on
    the random generators only, so they can be drawn one step ahead like any dataloader work.  The sampling stream
    never waits for the main stream (the step queued there runs beside it); `take()` makes the main stream wait for the
    draw's completion event and hands the tensors over (record_stream: the allocator must not recycle them under the
    consumer).  The random stream is the one a serial loop would consume: same points, same losses."""

    def __init__(self, sampler, n_frames):
        self.sampler, self.n_frames = sampler, n_frames
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())     # (inputs uploaded so far on the main stream)
        self._pending = None

    def draw(self, frames, sizes, valo_ids, num_valo_ids, ready=None):
        """Queues one step's draw: (queries (T, N, 4), targets (T, N, 6)) of batch element 0, as the bench consumes them.
        The inputs must be COMPLETE on the device before the side stream reads them: either they were uploaded before
        this object was built, or the caller passes `ready` -- an event recorded on the producing stream right after the
        upload (as PointCompletionNetV3.prefetch_geometry takes it): the side stream waits for that event only, not for
        the step queued behind it.  Without `ready` the side stream waits for everything queued on the current stream
        so far (safe, but it then also waits for a step already queued there)."""
        if ready is not None:
            self.stream.wait_event(ready)
        else:
            self.stream.wait_stream(torch.cuda.current_stream())
        for t_ in list(frames) + list(sizes) + [valo_ids, num_valo_ids]:
            if torch.is_tensor(t_) and t_.is_cuda:
                t_.record_stream(self.stream)      # the allocator must not recycle an input under the side stream
        with torch.cuda.stream(self.stream):
            qs, ts = [], []
            for t in range(self.n_frames):
                (si, ai, st, at, _, _) = self.sampler(frames, sizes, valo_ids, num_valo_ids, t)
                qs.append(torch.cat([si, ai], dim=1)[0])
                ts.append(torch.cat([st, at], dim=1)[0])
            q, tgt = torch.stack(qs), torch.stack(ts)
            done = torch.cuda.Event()
            done.record()
        self._pending = (q, tgt, done)

    def take(self):
        """The pending draw, ordered before everything queued on the current stream from here on."""
        assert self._pending is not None, 'draw() first'
        (q, tgt, done), self._pending = self._pending, None
        cur = torch.cuda.current_stream()
        cur.wait_event(done)
        q.record_stream(cur)
        tgt.record_stream(cur)
        return q, tgt


_UNSET = object()


class FusedClipAdamW(torch.optim.Optimizer):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW.step() for all parameters as ONE library call of three launches and no
    host read (occ4d_adamw_clip_groups_f32, csrc/optim.hip; train.py:107-109, 287-293).

    The parameters become views of one flat fp32 buffer (`p.data` is re-pointed once, here; values unchanged) and the two
    moment buffers are flat beside it; gradients stay wherever the backward pass left them -- a table of their addresses
    and per-tensor hyper-parameters (pinned host array -> one small asynchronous upload) is the only per-step host work:
    ~0.3 ms against ~15 ms for the ~150-tensor foreach path of torch (profiles/r05_train_phases.txt).  A parameter whose
    .grad is None is skipped entirely (no decay, no moment update), as torch does.  The gradients are NOT scaled in
    memory: the clip coefficient is applied inside the update (`last_norm` / `last_coef` stay on the device for whoever
    wants to log them).

    It is a torch.optim.Optimizer: `params` is an iterable of tensors or a list of group dicts with their own lr / betas /
    eps / weight_decay, read from `param_groups` at EVERY step (an lr scheduler's change acts on the next step; tensors
    of all groups are updated by the same launch).  `max_norm` (None = no clip) is a group default too, so that a bare
    `step()` -- what `GradScaler(enabled=False).step(optimizer)` calls -- clips.  `state[p]` holds torch's entries for every
    parameter that has had a gradient: `exp_avg` / `exp_avg_sq` are VIEWS of the flat moment buffers, `step` is a host
    integer here and the float32 scalar tensor torch writes in `state_dict()`, whose layout is torch.optim.AdamW's (the
    moments there are copies).  `load_state_dict()` takes that layout from torch.optim.AdamW or from this class (any
    device) and copies into the flat buffers; the flat layout this class wrote earlier ('exp_avg' without 'state') still
    loads.  Refused: amsgrad, maximize, capturable, differentiable, Adam's coupled weight decay, a device-tensor lr (a
    host read per step), add_param_group() after construction (the flat layout is fixed), and a step after the module
    was moved or cast (`net.half()`, `net.to(device)`: the modules then read other storage than the step updates)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, max_norm=None):
        # the group keys of THIS torch's AdamW (they differ between releases), so that state_dict() is its layout
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        capturable=capturable, differentiable=differentiable, max_norm=max_norm)
        self._layout_fixed = False
        super().__init__(params, defaults)
        self._layout_fixed = True                                           # (add_param_group raises from here on)
        for k, group in enumerate(self.param_groups):
            self._hyper(k, group)
        self.params = [p for group in self.param_groups for p in group['params']]
        assert all(p.is_cuda and p.dtype == torch.float32 for p in self.params), 'CUDA fp32 parameters'
        self.steps = 0
        dev = self.params[0].device
        assert all(p.device == dev for p in self.params), 'parameters on one device'
        T = len(self.params)
        numels = [p.numel() for p in self.params]
        offsets, total = [], 0
        for n in numels:
            offsets.append(total)
            total += (n + 3) // 4 * 4                                   # (16-byte aligned views)
        self.flat = torch.zeros((total,), dtype=torch.float32, device=dev)
        for p, off, n in zip(self.params, offsets, numels):
            view = self.flat[off:off + n].view(p.shape)
            view.copy_(p.data)
            p.data = view
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self._moments = [(self.exp_avg[off:off + n].view(p.shape), self.exp_avg_sq[off:off + n].view(p.shape))
                         for p, off, n in zip(self.params, offsets, numels)]
        self._entries = [None] * T                                          # state[p] of parameter i once it has had a gradient
        self._where = [(self.flat.data_ptr() + 4 * off, n) for off, n in zip(offsets, numels)]
        chunk = int(ops._lib.lib().occ4d_adamw_chunk())
        ct, cs = [], []
        for t, n in enumerate(numels):
            for lo in range(0, n, chunk):
                ct.append(t)
                cs.append(lo)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)      # noqa: E731
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
        self._offsets, self._numels, self._chunk_tensor, self._chunk_start = i64(offsets), i64(numels), i32(ct), i32(cs)
        self._n_chunks = len(ct)
        # the table ([0, T): gradient addresses; behind them 8 floats per tensor: bias1, sqrt(bias2), lr, beta1, beta2, eps,
        # weight_decay, unused) is uploaded asynchronously: a ring of pinned staging arrays, each reused only after the
        # upload that read it has run (the host may be several steps ahead of the device)
        self._staging = [[torch.zeros((5 * T,), dtype=torch.int64, pin_memory=True), None] for _ in range(4)]
        self._grad_ptrs = torch.zeros((5 * T,), dtype=torch.int64, device=dev)
        self._ws = torch.zeros((self._n_chunks + 2,), dtype=torch.float32, device=dev)

    @staticmethod
    def _hyper(k, group):
        """(lr, beta1, beta2, eps, weight_decay) of param_groups[k] as floats; ValueError for what the step does not do."""
        for flag in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
            if group.get(flag):
                raise ValueError('FusedClipAdamW: param_groups[%d] sets %s=True, which the fused step does not implement'
                                 % (k, flag))
        if group.get('decoupled_weight_decay', True) is False:
            raise ValueError('FusedClipAdamW: param_groups[%d] asks for Adam\'s coupled weight decay (AdamW only)' % k)
        lr = group['lr']
        if torch.is_tensor(lr) and lr.is_cuda:
            raise ValueError('FusedClipAdamW: param_groups[%d]: lr is a device tensor (a host read in every step)' % k)
        lr, b1, b2 = float(lr), float(group['betas'][0]), float(group['betas'][1])
        eps, wd = float(group['eps']), float(group['weight_decay'])
        if not (lr >= 0.0 and eps >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and wd >= 0.0):
            raise ValueError('FusedClipAdamW: param_groups[%d]: lr=%r, betas=(%r, %r), eps=%r, weight_decay=%r (need lr, eps, '
                             'weight_decay >= 0 and betas in [0, 1))' % (k, lr, b1, b2, eps, wd))
        return lr, b1, b2, eps, wd

    def add_param_group(self, param_group):
        if getattr(self, '_layout_fixed', False):
            raise RuntimeError('FusedClipAdamW: the flat parameter layout is fixed at construction; build a new optimizer '
                               'over all parameter groups instead of adding one')
        super().add_param_group(param_group)

    @property
    def last_norm(self):
        return self._ws[self._n_chunks]

    @property
    def last_coef(self):
        return self._ws[self._n_chunks + 1]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _set_count(self, i, k):
        """Parameter i has had k updates; k = 0: no state entry (torch's state of a parameter that never had a gradient)."""
        if k == 0:
            self.state.pop(self.params[i], None)
            self._entries[i] = None
            return
        st = self._entries[i]
        if st is None:
            st = self._entries[i] = self.state[self.params[i]]
            st.update(step=0, exp_avg=self._moments[i][0], exp_avg_sq=self._moments[i][1])
        st['step'] = k

    def step(self, closure=None, max_norm=_UNSET, grad_scale=1.0):
        """`max_norm` unset: the groups' default (None / 0 = no clip).  `grad_scale`: every gradient is read as
        g * grad_scale, in the norm and in the update (1 / world after a SUM all-reduce, or an un-scale factor)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        if max_norm is _UNSET:
            max_norm = groups[0]['max_norm']
            if any(g['max_norm'] != max_norm for g in groups[1:]):
                raise ValueError('FusedClipAdamW: the clip is over the gradients of ALL groups; they need one max_norm')
        T = len(self.params)
        if sum(len(g['params']) for g in groups) != T:
            raise RuntimeError('FusedClipAdamW: param_groups were changed after construction (the flat layout is fixed)')
        for i, (p, (ptr, n)) in enumerate(zip(self.params, self._where)):
            if p.data_ptr() != ptr or p.dtype != torch.float32 or p.numel() != n:
                raise RuntimeError('FusedClipAdamW: parameter %d no longer lives in the optimizer\'s flat buffer: the module '
                                   'was moved or cast (.to / .half / .cpu) after the optimizer was built; build the '
                                   'optimizer after that' % i)
        hyper = [self._hyper(k, g) for k, g in enumerate(groups)]           # (all checked before any count moves)
        self.steps += 1
        slot = self._staging[self.steps % len(self._staging)]
        if slot[1] is not None:
            slot[1].synchronize()
        table = slot[0].numpy()
        rows = table[T:].view(np.float32).reshape(T, 8)
        keep = []                                                           # (non-contiguous gradients: packed copies, kept alive)
        i = 0
        for group, (lr, b1, b2, eps, wd) in zip(groups, hyper):
            members = group['params']
            rows[i:i + len(members), 2:7] = (lr, b1, b2, eps, wd)
            for p in members:
                g = p.grad
                if g is None:
                    table[i] = 0
                    i += 1
                    continue
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                assert g.dtype == torch.float32 and g.is_cuda
                table[i] = g.data_ptr()
                st = self._entries[i]
                k = 1 if st is None else st['step'] + 1
                self._set_count(i, k)
                rows[i, 0] = 1.0 - b1 ** k
                rows[i, 1] = math.sqrt(1.0 - b2 ** k)
                i += 1
        self._grad_ptrs.copy_(slot[0], non_blocking=True)
        L = ops._lib
        L.check(L.lib().occ4d_adamw_clip_groups_f32(
            ops._ptr(self.flat), ops._ptr(self.exp_avg), ops._ptr(self.exp_avg_sq), ops._ptr(self._grad_ptrs),
            ops._ptr(self._offsets), ops._ptr(self._numels), T, ops._ptr(self._chunk_tensor),
            ops._ptr(self._chunk_start), self._n_chunks, float(max_norm) if max_norm else 0.0, float(grad_scale),
            ops._ptr(self._ws), ops._stream()))
        slot[1] = torch.cuda.Event()
        slot[1].record()
        del keep
        return loss

    def state_dict(self):
        """torch.optim.AdamW's layout (loadable by it for the same parameter list); the moments are copies."""
        sd = super().state_dict()
        for group in sd['param_groups']:
            group.pop('max_norm', None)                                     # (not a key of torch's groups)
        sd['state'] = {i: dict(step=torch.tensor(float(st['step']), dtype=torch.float32), exp_avg=st['exp_avg'].clone(),
                               exp_avg_sq=st['exp_avg_sq'].clone()) for i, st in sd['state'].items()}
        return sd

    def load_state_dict(self, sd):
        T = len(self.params)
        if 'state' not in sd and 'exp_avg' in sd:                           # the flat layout this class wrote earlier
            counts = [int(k) for k in sd.get('counts', [int(sd['step'])] * T)]
            assert len(counts) == T
            self.exp_avg.copy_(sd['exp_avg'])
            self.exp_avg_sq.copy_(sd['exp_avg_sq'])
            self.steps = int(sd['step'])
            for i, k in enumerate(counts):
                self._set_count(i, k)
            return
        groups, saved = self.param_groups, sd['param_groups']
        if len(groups) != len(saved):
            raise ValueError('loaded state dict has a different number of parameter groups')
        if any(len(g['params']) != len(s['params']) for g, s in zip(groups, saved)):
            raise ValueError('loaded state dict contains a parameter group that doesn\'t match the size of optimizer\'s group')
        merged = [dict(g, **{k: copy.deepcopy(v) for k, v in s.items() if k != 'params'}) for g, s in zip(groups, saved)]
        for k, group in enumerate(merged):
            self._hyper(k, group)                                           # (refused before anything is changed)
        index = {pid: i for i, pid in enumerate(pid for s in saved for pid in s['params'])}
        entries = {}
        for pid, st in sd['state'].items():
            if pid not in index:
                raise ValueError('loaded state dict has state for a parameter (%r) that no group lists' % (pid,))
            i = index[pid]
            if any(tuple(st[name].shape) != tuple(self.params[i].shape) for name in ('exp_avg', 'exp_avg_sq')):
                raise ValueError('loaded state of parameter %d does not have its shape %s' % (i, tuple(self.params[i].shape)))
            entries[i] = st
        for i, (m, v) in enumerate(self._moments):
            st = entries.get(i)
            if st is None:
                m.zero_()
                v.zero_()
                self._set_count(i, 0)
            else:
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                self._set_count(i, int(round(float(st['step']))))
        for group, new in zip(groups, merged):
            group.update(new)                                               # (in place: a scheduler may hold the dicts)


class TrainStep:
    """One optimisation step: forward (encoder + decoder per target frame), losses, backward,
    gradient all-reduce, clip (train.py:107-109, max norm 0.2), optimiser step."""

    def __init__(self, pcl_net, implicit_net, lr=1e-3, weight_decay=1e-2, grad_clip=0.2, loss_kwargs=None,
                 kernel_selection=None, fused_optimizer=True, param_groups=None):
        """`kernel_selection`: dict of kernels.Selection fields this step's forward runs under (e.g.
        dict(train_precision='bf16x6', logit_precision='bf16x6', checkpoint_attention=False)); the backward pass follows
        it through the autograd Functions.  None = the calling thread's scope.
        `param_groups`: a list of optimizer group dicts, or a callable (pcl_net, implicit_net) -> such a list, in place
        of the single group of all parameters (`lr` / `weight_decay` are the defaults of keys a group leaves out)."""
        self.kernel_selection = dict(kernel_selection or {})
        self.pcl_net, self.implicit_net = pcl_net, implicit_net
        self.params = list(pcl_net.parameters()) + list(implicit_net.parameters())
        # clip + AdamW as one library call over flat buffers (round 6); fused_optimizer=False: torch's own two calls
        self.fused = bool(fused_optimizer) and all(p.is_cuda for p in self.params)
        groups = self.params
        if param_groups is not None:
            groups = param_groups(pcl_net, implicit_net) if callable(param_groups) else param_groups
            groups = [dict(g, params=list(g['params'])) for g in groups]
            if sorted(id(p) for g in groups for p in g['params']) != sorted(id(p) for p in self.params):
                raise ValueError('param_groups must list every parameter of the two networks exactly once')
        if self.fused:
            self.optimizer = FusedClipAdamW(groups, lr=lr, weight_decay=weight_decay)
        else:
            self.optimizer = torch.optim.AdamW(groups, lr=lr, weight_decay=weight_decay)
        self.grad_clip = grad_clip
        self.loss_kwargs = loss_kwargs or {}
        self.participation = Participation()
        # the last step's unweighted (colour, density, segmentation, tracking) terms, what the reference logs every step
        # (loss.py:255-294): a (4,) device tensor, not read by the step itself
        self.last_loss_terms = None

    batch_frames = True

    def forward_loss(self, pcl_input, points_query, implicit_target):
        """pcl_input (1,N,8); points_query (T,Nq,4); implicit_target (T,Nq,6) -> scalar loss.
        The reference decodes the T target frames one after the other (pipeline.py:170-212); the decoder is pointwise
        in the queries (the frame is their 4th coordinate), so batch_frames runs all T * Nq of them through ONE decoder
        call: same outputs, GEMMs of 68 812 instead of 17 203 rows (269 instead of 135 row tiles for 256 CUs) and a
        quarter of the launches."""
        with kernels.use(**self.kernel_selection):
            return self._forward_loss(pcl_input, points_query, implicit_target)

    def _forward_loss(self, pcl_input, points_query, implicit_target):
        (pcl_abstract, features_global, _) = self.pcl_net(pcl_input, False)
        T_, Nq = points_query.shape[:2]
        if self.batch_frames:
            out = self.implicit_net(points_query.reshape(T_ * Nq, points_query.shape[-1]), pcl_abstract[0],
                                    features_global[0], None)[0].reshape(T_, Nq, -1)
        else:
            out = torch.stack([self.implicit_net(points_query[t], pcl_abstract[0], features_global[0], None)[0]
                               for t in range(T_)])
        loss, self.last_loss_terms = implicit_loss(out, implicit_target, return_terms=True, **self.loss_kwargs)
        return loss

    def __call__(self, pcl_input, points_query, implicit_target, next_pcl_input=None):
        """`next_pcl_input` (optional): the NEXT step's point cloud, already resident.  Its farthest-point chain and
        kNNs (coordinates only, no weights) are issued on the encoder's geometry stream as soon as this step's forward
        is launched, so they run under this step's backward (PointCompletionNetV3.prefetch_geometry)."""
        ops.check_pending(wait=False)          # status of earlier steps' cooperative FPS launches (no stall)
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.forward_loss(pcl_input, points_query, implicit_target)
        if next_pcl_input is not None:
            self.pcl_net.prefetch_geometry(next_pcl_input)
        with autograd.gradient_overlap():      # parameter gradients beside the data-gradient chain, joined on exit
            loss.backward()
        allreduce_gradients(self.params, participation=self.participation)
        if self.fused:
            self.optimizer.step(max_norm=self.grad_clip)
        else:
            if self.grad_clip:
                torch.nn.utils.clip_grad_norm_(self.params, self.grad_clip)
            self.optimizer.step()
        invalidate_weight_caches()             # merged inference matrices / per-scene tables are stale now
        return loss.detach()


def checkpoint_dict(step, lr_scheduler, epoch, args, pcl_args, dset_args, implicit_args):
    """The reference's checkpoint dict (train.py:339-350) of a TrainStep: optimizer and scheduler state in torch's layout,
    'scaler' as a disabled GradScaler writes it; torch.save() it and inference.load_models reads the file."""
    nets = {name: {k: v.detach().cpu() for k, v in net.state_dict().items()}
            for name, net in (('pcl_net', step.pcl_net), ('implicit_net', step.implicit_net))}
    return {'optimizer': step.optimizer.state_dict(), 'lr_scheduler': lr_scheduler.state_dict(), 'scaler': {},
            'epoch': epoch, 'args': args, 'pcl_args': pcl_args, 'dset_args': dset_args, 'implicit_args': implicit_args,
            'pcl_net': nets['pcl_net'], 'implicit_net': nets['implicit_net']}


def resume(step, lr_scheduler, checkpoint):
    """train.py:323-331 for a TrainStep: networks (copied in place, so the optimizer's flat views stay), optimizer and
    scheduler from a checkpoint dict; returns the epoch to start with."""
    step.pcl_net.load_state_dict(checkpoint['pcl_net'])
    step.implicit_net.load_state_dict({(('pt_blocks.0.' + k[len('pt_block.'):]) if k.startswith('pt_block.') else k): v
                                       for k, v in checkpoint['implicit_net'].items()})      # (legacy key rename)
    step.optimizer.load_state_dict(checkpoint['optimizer'])
    lr_scheduler.load_state_dict(checkpoint['lr_scheduler'])
    invalidate_weight_caches()
    return checkpoint['epoch'] + 1
