"""Differentiable wrappers (torch.autograd.Function) over the HIP kernels: the training path.

SURVEY.md 8(f) rank 1.  The reference trains through torch autograd over ATen ops
(train.py:101-118); here every forward AND backward computation runs in libocc4d.so.  torch
supplies the tape, tensor glue (cat / slicing) and the optimiser only.  The training forward
uses the as-written op order of model/*.py (no weight merging), built from the unfused kernels;
kNN / FPS carry no gradient (they depend on coordinates only).
"""
import contextlib
import os

import torch
from torch.autograd import Function

from . import kernels
from . import ops

# Training-path Linear layers with a 416-wide operand (the decoder trunk, the 416 -> 832 / 832 <- 416 layers of the
# attention MLP and their data gradients) run on the row-resident kernel of the inference trunk (occ4d_rowlin_f32:
# 0.72-0.79 of the fp32 MFMA peak against 0.46-0.65 for the generic kernel at these shapes, profiles/train_shapes.py).
# The stage-packed copy of a weight (and of its transpose, for the data gradient) is rebuilt when the weight changes.
ROWLIN_IN_TRAINING = True
# ... in its half-CU re-cut (csrc/trunk4.hip: 64-row workgroups, two per CU).  The training row counts are not whole
# dispatch rounds of the 8-wave kernel (68812 query rows = 2.1 rounds of 256 x 128 rows: the third round runs 26
# workgroups); a half-CU workgroup that has its CU to itself in the last round runs faster, and at whole rounds the two
# are level: 232 vs 301 us at 68812 rows, 276 vs 302 us at 98304 (profiles/time_rowlin_tail.py).
ROWLIN_HALF_CU = os.environ.get('OCC4D_TRAIN_ROWLIN_HALF_CU', '1') == '1'
# Opt-in (round 5), fp32-class: the 416-input Linear layers of the training path -- forward, and the data gradients whose
# reduction side is 416 wide -- on the split-precision row kernel (csrc/trunk_bf16x6.hip: bf16 x 3 pieces, 6 partial
# products, fp32 accumulate).  Weight gradients stay on the fp32 MFMA kernels.  Same strict gradient tests.
# Selected per call: kernels.Selection.train_precision (`with kernels.use(train_precision='bf16x6')`, default from
# OCC4D_TRAIN_PRECISION); the Functions below carry the selection of their forward into their backward.


def _x6():
    return kernels.scope().train_precision == 'bf16x6'


_PACKS = {}           # stage-packed copies of nn.Parameters only (small LRU); transient leaves are packed uncached
_PACKS_MAX = 128
_ZEROS = {}           # zero bias vectors, kept apart from the packs and created eagerly (never inside a capture)


# ---- parameter gradients beside the data-gradient chain ---------------------------------------------------------------
# A backward pass is one dependency chain of DATA gradients (each layer's dx feeds the layer below) with a PARAMETER
# gradient hanging off every link (dW = g^T x, db, the scatter onto the key / value tables, ...) that nothing reads until
# the optimiser.  Issued on one stream they serialise: every partial dispatch round of a GEMM, every split-M partial sum
# and every 5 us reduction is waited for.  Inside `gradient_overlap()` (training.TrainStep wraps loss.backward() in it)
# the parameter-gradient launches go to a second stream that is ordered behind the producer of their operands (an event
# per submission) and joined at the end of the pass: they fill the tails and small-kernel gaps of the chain
# (88.7 -> 83.7 ms per config-5 step when first measured; same kernels, same operands, same sums).
#   * results are never handed to the autograd engine from the side stream (its accumulation would run on the main
#     stream, unordered): gradients of nn.Parameters collect in private buffers that `gradient_overlap()` adds to .grad
#     on exit, after the join; gradients of the transient leaves of a recompute pass collect in `gradient_sinks()`;
#   * every operand a side-stream kernel reads is HELD (a reference, released once an event behind that kernel has
#     completed): the allocator cannot recycle it underneath, and -- the hazard a record_stream would not cover -- the
#     autograd engine cannot accumulate into it in place (it adds a later gradient contribution INTO a buffer it holds
#     the only reference to: `dy` handed on as the residual's gradient is such a buffer while the side stream still
#     reads it as the `g` of a weight gradient);
#   * while a stream is being captured nothing is moved (one stream).  A captured step with the same two branches was
#     measured in round 5 and is gone with the captured step itself (profiles/r05_train_graph_vs_eager.txt).
#   * the side stream may fall behind (the chain's kernels are submitted first and fill the machine); the operands held
#     for it are bounded: beyond GRADIENT_OVERLAP_BYTES the main stream waits for the oldest submission before it goes on.
GRADIENT_OVERLAP = os.environ.get('OCC4D_GRADIENT_OVERLAP', '1') == '1'
GRADIENT_OVERLAP_BYTES = int(float(os.environ.get('OCC4D_GRADIENT_OVERLAP_GB', '6')) * 2 ** 30)


class _Overlap:
    stream = None
    device = None        # the device the side stream lives on (asserted: one device per process)
    depth = 0
    params = {}          # id(parameter) -> [parameter, sum]      (filled on the side stream)
    sinks = {}           # id(leaf) -> [leaf, sum or None]        (gradient_sinks)
    held = []            # (event behind a side-stream submission, the operands it reads, their bytes), oldest first
    held_bytes = 0


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _release_held(everything=False, room_for=None):
    held = _Overlap.held
    while held and (everything or held[0][0].query()):
        _Overlap.held_bytes -= held.pop(0)[2]
    if room_for is not None:
        # over the budget: the current stream waits for the oldest submissions (a stream-side wait, the host goes on);
        # what is queued here afterwards is ordered behind their reads
        while held and _Overlap.held_bytes + room_for > GRADIENT_OVERLAP_BYTES:
            torch.cuda.current_stream().wait_event(held[0][0])
            _Overlap.held_bytes -= held.pop(0)[2]


def _overlap_on():
    return _Overlap.depth > 0 and GRADIENT_OVERLAP and torch.cuda.is_available() and not _capturing()


def join_gradients():
    """The current stream waits for every parameter-gradient launch submitted so far."""
    if _Overlap.stream is not None and not _capturing():
        torch.cuda.current_stream().wait_stream(_Overlap.stream)
        # (operands still held are read by kernels the current stream now waits for: anything queued here from now on is
        # ordered behind those reads, so the references can go)
        _release_held(everything=True)


@contextlib.contextmanager
def gradient_overlap():
    """Scope of one backward pass whose parameter gradients may run beside the data-gradient chain (see above).  On exit
    the current stream waits for them and the collected sums are added to the parameters' .grad.
    NOT compatible with hook-based reducers: inside the scope the Functions of this module report the
    gradients of nn.Parameters to autograd as None and write .grad here, on exit -- AccumulateGrad never runs for them, so
    parameter hooks / post-accumulate-grad hooks (DDP- or FSDP-style bucket reducers) do not fire and
    torch.autograd.grad(loss, params) inside the scope returns None for them.  This package reduces gradients AFTER the
    scope (training.allreduce_gradients).  The scope is process-wide state with one side stream on the device that was
    current at its first use: one training thread, one device per process (the launch model of bench_train.py)."""
    _Overlap.depth += 1
    try:
        yield
    finally:
        _Overlap.depth -= 1
        if _Overlap.depth == 0:
            join_gradients()
            collected, _Overlap.params = _Overlap.params, {}
            for p, g in collected.values():
                p.grad = g if p.grad is None else p.grad + g


class gradient_sinks:
    """`with gradient_sinks(leaves) as sink:` -- inside, the Functions of this module do not return the gradients of these
    leaf tensors to autograd (they return None: ask autograd.grad with allow_unused=True) but add them up here, on the
    stream the parameter gradients run on; `sink.sums()` joins that stream and returns one tensor per leaf (zeros for a leaf
    nothing reached)."""

    def __init__(self, leaves):
        self.leaves = list(leaves)

    def __enter__(self):
        for t in self.leaves:
            assert id(t) not in _Overlap.sinks
            _Overlap.sinks[id(t)] = [t, None]
        return self

    def sums(self):
        join_gradients()
        return [torch.zeros_like(t) if _Overlap.sinks[id(t)][1] is None else _Overlap.sinks[id(t)][1] for t in self.leaves]

    def __exit__(self, *exc):
        for t in self.leaves:
            _Overlap.sinks.pop(id(t), None)
        return False


def _deposit(targets, compute, *operands):
    """`compute()` returns one gradient per entry of `targets` (the tensors they are gradients OF; None = not wanted).
    Gradients of sink leaves and -- inside gradient_overlap() -- of nn.Parameters are added to their private sums on the
    side stream and reported to autograd as None; everything else is computed on the current stream and returned."""
    modes = []
    for t in targets:
        if t is None:
            modes.append(None)
        elif id(t) in _Overlap.sinks:
            modes.append('sink')
        elif _overlap_on() and isinstance(t, torch.nn.Parameter):
            modes.append('param')
        else:
            modes.append('plain')
    if not any(m in ('sink', 'param') for m in modes):
        return compute()
    side = _overlap_on() and 'plain' not in modes

    def run():
        out = []
        for t, m, g in zip(targets, modes, compute()):
            if m in ('sink', 'param') and g is not None:
                slot = _Overlap.sinks[id(t)] if m == 'sink' else _Overlap.params.setdefault(id(t), [t, None])
                slot[1] = g if slot[1] is None else slot[1].add_(g)
                g = None
            out.append(g)
        return tuple(out)

    if not side:
        join_gradients()                       # (earlier deposits into the same sums ran on the side stream)
        return run()
    if _Overlap.stream is None:
        _Overlap.stream = torch.cuda.Stream()
        _Overlap.device = torch.cuda.current_device()
    assert torch.cuda.current_device() == _Overlap.device, \
        'gradient_overlap(): one device per process (side stream on cuda:%d, called on cuda:%d)' % (
            _Overlap.device, torch.cuda.current_device())
    ready = torch.cuda.Event()
    ready.record()
    _Overlap.stream.wait_event(ready)
    with torch.cuda.stream(_Overlap.stream):
        res = run()
        done = torch.cuda.Event()
        done.record()
    nbytes = sum(t.numel() * t.element_size() for t in operands if torch.is_tensor(t))
    _release_held(room_for=nbytes)
    _Overlap.held.append((done, operands, nbytes))
    _Overlap.held_bytes += nbytes
    return res


def _packed(w, transposed, x6=False):
    from . import point_transformer_layer as ptl
    src = w.detach().t().contiguous() if transposed else w.detach()
    pack = ops.pack_rowlin_bf16x6 if x6 else (ops.pack_trunk4_rows if ROWLIN_HALF_CU else ops.pack_trunk_rows)
    if not isinstance(w, torch.nn.Parameter):
        # a transient leaf (the merged matrices rebuilt by every _CheckpointedAttention.backward): caching it would only
        # pin the leaf and its packed copy (a few MB each) until the table is cleared -- it can never hit again
        return pack(src)
    key = (id(w), bool(transposed), bool(x6))
    tag = (w.data_ptr(), w._version, tuple(w.shape), ptl.weights_epoch(), ROWLIN_HALF_CU)
    hit = _PACKS.get(key)
    if hit is not None and hit[0] is w and hit[1] == tag:
        _PACKS[key] = _PACKS.pop(key)              # most recently used last
        return hit[2]
    packed = pack(src)
    _PACKS.pop(key, None)
    while len(_PACKS) >= _PACKS_MAX:
        _PACKS.pop(next(iter(_PACKS)))             # least recently used first
    _PACKS[key] = (w, tag, packed)                 # (w kept alive: its id cannot be recycled under this key)
    return packed


def _zeros(n, device):
    key = (n, str(device))
    z = _ZEROS.get(key)
    if z is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # a buffer first created inside a capture would be a captured memset that has not run yet: an eager use
            # before the first replay would read garbage as the bias.  Capture warm-up steps create every size eagerly.
            raise RuntimeError('zero-bias buffer of %d floats requested for the first time inside a stream capture; '
                               'run one eager step before capturing' % n)
        z = _ZEROS[key] = torch.zeros((n,), dtype=torch.float32, device=device)
    return z


def _linear_fwd(x, w, b, relu_in=False, relu_out=False, residual=None, transposed=False, mask=None, skip=None):
    """[relu]([relu](x) W'^T + b) + residual with W' = w (or w^T when `transposed`: the data gradient); `mask`: the
    result is zeroed where mask <= 0 (the ReLU of a relu_in layer applied to its data gradient); `skip` is added AFTER the
    mask (the gradient of a skip connection around the layer: one launch on the half-CU row kernel)."""
    n_out, k = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    if (_x6() and k == ops.TRUNK_WIDTH and n_out in ops.X6_ROWLIN_WIDTHS and not relu_out
            and x.shape[0] >= 1024 and x.is_contiguous() and not (residual is not None and skip is not None)):
        res = residual if residual is not None else skip
        return ops.rowlin_bf16x6(x, None, b, relu_in=relu_in, res=res, packed=_packed(w, transposed, x6=True), mask=mask,
                                 res_after_mask=skip is not None, n_out=n_out)
    if (ROWLIN_IN_TRAINING and k == ops.TRUNK_WIDTH and n_out % 32 == 0 and not relu_out and x.shape[0] >= 1024
            and x.is_contiguous() and (residual is None or residual.is_contiguous())):
        bias = b if b is not None else _zeros(n_out, x.device)
        if mask is not None and not mask.is_contiguous():
            mask = mask.contiguous()
        if skip is not None and not (ROWLIN_HALF_CU and mask is not None and residual is None and skip.is_contiguous()):
            return ops.rowlin(x, _packed(w, transposed), bias, n_out, relu_in=relu_in, residual=residual, mask=mask) + skip
        return ops.rowlin(x, _packed(w, transposed), bias, n_out, relu_in=relu_in, residual=residual, mask=mask, skip=skip)
    y = ops.linear(x, w.t().contiguous() if transposed else w, b, relu_in=relu_in, relu_out=relu_out,
                   residual=residual)
    y = y if mask is None else ops.relu_mask(y, mask)
    return y if skip is None else y + skip


class MatmulF64Fn(Function):
    """c = a @ b in fp64 on the library (the merged weights of DESIGN.md 4 (i) and, in training, their gradients back
    to the original parameters); b may be a vector."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.vec = b.dim() == 1
        b2 = b[:, None] if ctx.vec else b
        ctx.save_for_backward(a, b2)
        c = ops.matmul_f64(a, b2)
        return c[:, 0] if ctx.vec else c

    @staticmethod
    def backward(ctx, dc):
        a, b2 = ctx.saved_tensors
        dc2 = dc[:, None] if ctx.vec else dc
        da = ops.matmul_f64(dc2, b2.t()) if ctx.needs_input_grad[0] else None
        db = ops.matmul_f64(a.t(), dc2) if ctx.needs_input_grad[1] else None
        if db is not None and ctx.vec:
            db = db[:, 0]
        return da, db


def matmul64(a, b):
    """fp64 product of the merged-weight algebra.  CUDA tensors: the library kernel.  CPU tensors only occur when the
    algebra itself is checked on the host (tests/test_host.py builds a module on the CPU and compares the merged
    matrices with the as-written expression); such a module cannot run a forward pass -- every op rejects CPU tensors."""
    if not a.is_cuda:
        return a @ b
    return MatmulF64Fn.apply(a, b)


class FanOut:
    """Shared by the `uses` LinearFn calls that consume the SAME input tensor (the decoder's per-query latent feeds one
    lin_z layer per block): each call's data gradient is a GEMM whose epilogue adds the running sum of the calls before it,
    and only the last one reports the total to autograd (the others report None) -- instead of `uses` separate gradients
    that the engine adds up in `uses - 1` element-wise passes over an (n, K) tensor.
    CONTRACT: every one of the `uses` nodes must run in the SAME backward pass, i.e. the whole decoder forward
    is differentiated at once (what TrainStep and the tests do).  Differentiating a sub-graph that holds only some of them
    (autograd.grad of an intermediate block output w.r.t. the shared latent) leaves the running sum unreported: the
    object then says so -- `pending()` is True -- and the next pass through it raises instead of adding to a stale sum.
    One object serves ONE forward pass (LocalPclResnetFC._forward_train builds a fresh one per call)."""

    def __init__(self, uses):
        self.uses, self.left, self.total = uses, uses, None

    def pending(self):
        """True between the first and the last of the sharing nodes' backward calls (a partial pass stays pending)."""
        return 0 < self.left < self.uses

    def take(self, dx):
        """One sharing node's data gradient (already holding the running sum): returns the total for the last node, None
        (not reported yet) for the others."""
        assert self.left > 0, 'FanOut: more backward calls than the %d nodes that share the input' % self.uses
        self.left -= 1
        if self.left > 0:
            self.total = dx
            return None
        self.total, self.left = None, self.uses          # complete: ready for a second pass over a retained graph
        return dx


@kernels.carries_selection
class LinearFn(Function):
    """y = [relu]( [relu](x) W^T + b ) + residual   (never relu_out together with residual)."""

    @staticmethod
    def forward(ctx, x, w, b, relu_in, relu_out, residual, fan=None):
        assert not (relu_out and residual is not None)
        y = _linear_fwd(x, w, b, relu_in=relu_in, relu_out=relu_out, residual=residual)
        ctx.fan = fan
        ctx.flags = (relu_in, relu_out, b is not None, residual is not None)
        ctx.save_for_backward(x, w, y if relu_out else None)
        ctx.params = (w, b)        # (the objects themselves: saved_tensors hands back new tensor objects, and the
        return y                   #  gradient sums of _deposit are keyed on the parameter / leaf object)

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        relu_in, relu_out, has_b, has_res = ctx.flags
        dy = dy.contiguous()
        g = ops.relu_mask(dy, y) if relu_out else dy
        dx = dw = db = dres = None
        if ctx.needs_input_grad[0]:
            fan = ctx.fan
            if fan is not None and not relu_in:
                dx = fan.take(_linear_fwd(g, w, None, transposed=True, residual=fan.total))   # (reported by the last of the
                                                                                              #  calls that share the input)
            else:
                dx = _linear_fwd(g, w, None, transposed=True, mask=x if relu_in else None)
        want_db = has_b and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            # one kernel: dW = g^T [relu](x) on the MFMA, db = column sums of the g tiles it stages
            def wgrad():
                res = ops.linear_wgrad(g, x, bias=want_db, relu_x=relu_in)
                return res if want_db else (res, None)
            dw, db = _deposit((ctx.params[0], ctx.params[1] if want_db else None), wgrad, g, x)
        elif want_db:
            (db,) = _deposit((ctx.params[1],), lambda: (ops.colsum(g),), g)
        if has_res and ctx.needs_input_grad[5]:
            dres = dy
        return (dx, dw, db, None, None, dres, None)[:len(ctx.needs_input_grad)]     # (`fan` may be left out)


def linear(x, lin, relu_in=False, relu_out=False, residual=None, fan=None):
    """x (n,K) through an nn.Linear's parameters.  `fan`: a FanOut shared by every call that consumes this same x."""
    return LinearFn.apply(x, lin.weight, lin.bias, relu_in, relu_out, residual, fan)


@kernels.carries_selection
class ResBlockFn(Function):
    """y = x + W1 relu(W0 relu(x) + b0) + b1  (model/implicit.py:66-85 without shortcut, ReLU): the two Linear layers of a
    residual block as ONE autograd node, so that the skip connection's gradient is added in the epilogue of the last
    data-gradient GEMM (dx = dy + relu'(x) (dh W0)) instead of by the engine in a separate pass over (n, d)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1):
        h = _linear_fwd(x, w0, b0, relu_in=True)
        y = _linear_fwd(h, w1, b1, relu_in=True, residual=x)
        ctx.save_for_backward(x, h, w0, w1)
        ctx.params = (w0, b0, w1, b1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, w0, w1 = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = dy.contiguous()
        dx = dw0 = db0 = dw1 = db1 = None

        def wgrad(gg, xx, want_w, want_b):
            if not want_w:
                return (None, ops.colsum(gg))
            res = ops.linear_wgrad(gg, xx, bias=bool(want_b), relu_x=True)
            return res if want_b else (res, None)

        (t0, tb0, t1, tb1) = ctx.params
        if need[3] or need[4]:
            dw1, db1 = _deposit((t1 if need[3] else None, tb1 if need[4] else None),
                                lambda: wgrad(g, h, need[3], need[4]), g, h)
        if need[0] or need[1] or need[2]:
            dh = _linear_fwd(g, w1, None, transposed=True, mask=h)
            if need[1] or need[2]:
                dw0, db0 = _deposit((t0 if need[1] else None, tb0 if need[2] else None),
                                    lambda: wgrad(dh, x, need[1], need[2]), dh, x)
            if need[0]:
                dx = _linear_fwd(dh, w0, None, transposed=True, mask=x, skip=g)
        return dx, dw0, db0, dw1, db1


def resblock(x, fc_0, fc_1):
    """The residual block above through two nn.Linear modules' parameters (both with bias)."""
    return ResBlockFn.apply(x, fc_0.weight, fc_0.bias, fc_1.weight, fc_1.bias)


class ImplicitLossFn(Function):
    """training.implicit_loss's density + segmentation terms as one library call (ops.implicit_loss_fused): the gradient
    is formed with the value and scaled by the incoming scalar in backward."""

    @staticmethod
    def forward(ctx, out, target, semantic_classes, density_lw, segmentation_lw):
        loss, grad = ops.implicit_loss_fused(out, target, semantic_classes, density_lw, segmentation_lw,
                                             want_grad=out.requires_grad)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


class ImplicitLossTermsFn(Function):
    """training.implicit_loss's four terms as one library call (ops.implicit_loss_terms_fused) on the RAW decoder outputs ->
    (total, terms (4,)): the gradient is formed with the value and scaled by the incoming scalar in backward; the per-term
    values are for logging and carry no gradient."""

    @staticmethod
    def forward(ctx, out, target, color_mode, semantic_classes, density_lw, color_lw, segmentation_lw, tracking_lw):
        loss, terms, grad = ops.implicit_loss_terms_fused(out, target, color_mode, semantic_classes, density_lw, color_lw,
                                                          segmentation_lw, tracking_lw, want_grad=out.requires_grad)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms)
        return loss.reshape(()), terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None, None, None


class PosHiddenFn(Function):
    """r = relu(P1 (pos_i - pos2_j) + c1); gradients to P1, c1 only (coordinates are data)."""

    @staticmethod
    def forward(ctx, pos, pos2, idx, P1, c1):
        r = ops.pt_pos_hidden(pos, pos2, idx, P1, c1)
        ctx.save_for_backward(pos, pos2, idx, r)
        ctx.params = (P1, c1)
        return r

    @staticmethod
    def backward(ctx, gr):
        pos, pos2, idx, r = ctx.saved_tensors
        gr = gr.contiguous()
        dP1, dc1 = _deposit(ctx.params, lambda: ops.pt_pos_hidden_bwd(pos, pos2, idx, r, gr), pos, pos2, idx, r, gr)
        return None, None, None, dP1, dc1


class AttnInFn(Function):
    """a[p] = q[i] - kf[idx[p]] + pe[p]."""

    @staticmethod
    def forward(ctx, q, kf, pe, idx):
        ctx.save_for_backward(idx)
        ctx.m = kf.shape[0]
        return ops.pt_attn_in(q, kf, pe, idx)

    @staticmethod
    def backward(ctx, da):
        (idx,) = ctx.saved_tensors
        da = da.contiguous()
        k = idx.shape[1]
        return ops.segment_sum(da, k), ops.scatter_add_rows(da, idx, ctx.m, scale=-1.0), da, None


class AttnInLinearFn(Function):
    """a[p] = q[i] - kf[idx[p]] + r[p] Wp^T  (p = i k + j): AttnInFn fused with the K = 32 Linear that feeds it -- the
    (N k, 2D) product Wp r is never written on its own and the gather / subtract pass over it disappears (the generic
    Linear kernel adds the gathered rows in its epilogue)."""

    @staticmethod
    def forward(ctx, q, kf, r, wp, idx):
        k = idx.shape[1]
        a = ops.linear(r, wp, add_rows=q, add_div=k, sub_rows=kf, sub_idx=idx.reshape(-1))
        ctx.save_for_backward(r, wp, idx)
        ctx.m = kf.shape[0]
        ctx.params = (kf, wp)
        return a

    @staticmethod
    def backward(ctx, da):
        r, wp, idx = ctx.saved_tensors
        da = da.contiguous()
        k, m = idx.shape[1], ctx.m
        dq = ops.segment_sum(da, k) if ctx.needs_input_grad[0] else None
        dkf = dwp = None
        if ctx.needs_input_grad[1]:
            (dkf,) = _deposit(ctx.params[:1], lambda: (ops.scatter_add_rows(da, idx, m, scale=-1.0),), da, idx)
        dr = _linear_fwd(da, wp, None, transposed=True) if ctx.needs_input_grad[2] else None
        if ctx.needs_input_grad[3]:
            (dwp,) = _deposit(ctx.params[1:], lambda: (ops.linear_wgrad(da, r),), da, r)
        return dq, dkf, dr, dwp, None


PAIR_MLP_FUSED = os.environ.get('OCC4D_PAIR_MLP', '1') == '1'


def pair_mlp_fused_ok(aq, r, idx):
    """The fused pair-tensor kernel is built for d = 416 and 32 positional hidden units, with 32-bit row offsets."""
    d = ops.TRUNK_WIDTH
    return (PAIR_MLP_FUSED and aq.shape[1] == 2 * d and r.shape[1] == 32
            and idx.numel() * 2 * d * 4 < 2 ** 32 and aq.shape[0] * aq.stride(0) * 4 < 2 ** 32)


@kernels.carries_selection
class PairMlpFn(Function):
    """(logits, pe) of the merged-form layer from ONE kernel (ops.pt_pair_mlp), for the chain
        a = aq_i - kt_j + Wp r;  logits = W2 relu(a) [+ b2];  pe = P2 r + c2
    (AttnInLinearFn -> LinearFn(relu_in) -> LinearFn in separate launches otherwise).  b2 is not added: the logits only
    feed the softmax over the neighbour axis, where a per-channel constant cancels; its gradient (the column sums of
    dlogits, zero up to rounding) is still returned.  backward = the backward passes of those three Functions."""

    _stream = None       # (W2, wp, P2, their versions, packed stream) of the last call: the recompute walks the queries
                         # in chunks with the SAME weight tensors (identity + version: held here, so no address is recycled)

    @staticmethod
    def _packed_stream(W2, b2, wp, P2, c2, x6=None):
        x6 = _x6() if x6 is None else x6
        hit = PairMlpFn._stream
        if (hit is not None and hit[0] is W2 and hit[1] is wp and hit[2] is P2
                and hit[3] == (W2._version, wp._version, P2._version, x6)):
            return hit[4]
        stream = ops.pack_attn_bf16x6_stream(W2, wp, P2) if x6 else ops.pack_attn16p_stream(W2, b2, wp, P2, c2)
        PairMlpFn._stream = (W2, wp, P2, (W2._version, wp._version, P2._version, x6), stream)
        return stream

    @staticmethod
    def forward(ctx, aq, kt, r, wp, W2, b2, P2, c2, idx, kept=None):
        """`kept` = (a | None, logits, pe | None): what the training forward's fused kernel stored for these rows
        (Selection.store_pairs).  All three: no launch at all.  Logits only: the launch recomputes a and pe (fp32 kernel,
        memory-bound: the split scheme has nothing to gain there)."""
        if kept is not None and kept[0] is not None:
            a, logits, pe = (t.detach() for t in kept)    # (fresh tensor objects on the same rows: outputs, not the inputs)
        elif kept is not None:
            stream = PairMlpFn._packed_stream(W2, b2, wp, P2, c2, x6=False)
            a, logits, pe = ops.pt_pair_mlp(aq, kt, r, idx, c2, stream, logits=kept[1])
            logits = logits.detach()
        elif _x6():
            stream = PairMlpFn._packed_stream(W2, b2, wp, P2, c2)
            a, logits, pe = ops.pt_pair_mlp_bf16x6(aq, kt, r, idx, c2, stream)
        else:
            stream = PairMlpFn._packed_stream(W2, b2, wp, P2, c2)
            a, logits, pe = ops.pt_pair_mlp(aq, kt, r, idx, c2, stream)
        ctx.save_for_backward(a, r, wp, W2, P2, idx)
        ctx.m = kt.shape[0]
        ctx.params = (kt, wp, W2, b2, P2, c2)
        return logits, pe

    @staticmethod
    def backward(ctx, dlogits, dpe):
        a, r, wp, W2, P2, idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        k = idx.shape[1]
        dlogits, dpe = dlogits.contiguous(), dpe.contiguous()
        dW2 = db2 = dP2 = dc2 = dwp = daq = dkt = dr = None
        (t_kt, t_wp, t_W2, t_b2, t_P2, t_c2), m = ctx.params, ctx.m

        def wgrad_bias(g, x, want_w, want_b, relu_x):
            if not want_w:
                return (None, ops.colsum(g))
            res = ops.linear_wgrad(g, x, bias=bool(want_b), relu_x=relu_x)
            return res if want_b else (res, None)

        if need[4] or need[5]:
            dW2, db2 = _deposit((t_W2 if need[4] else None, t_b2 if need[5] else None),
                                lambda: wgrad_bias(dlogits, a, need[4], need[5], True), dlogits, a)
        da = _linear_fwd(dlogits, W2, None, transposed=True, mask=a)          # (x > 0) . (g W2)
        if need[0]:
            daq = ops.segment_sum(da, k)
        if need[1]:
            (dkt,) = _deposit((t_kt,), lambda: (ops.scatter_add_rows(da, idx, m, scale=-1.0),), da, idx)
        if need[3]:
            (dwp,) = _deposit((t_wp,), lambda: (ops.linear_wgrad(da, r),), da, r)
        if need[6] or need[7]:
            dP2, dc2 = _deposit((t_P2 if need[6] else None, t_c2 if need[7] else None),
                                lambda: wgrad_bias(dpe, r, need[6], need[7], False), dpe, r)
        if need[2]:
            dr = _linear_fwd(da, wp, None, transposed=True)
            dr += _linear_fwd(dpe, P2, None, transposed=True)
        return daq, dkt, dr, dwp, dW2, db2, dP2, dc2, None, None


class SoftmaxAggFn(Function):
    """agg[i] = sum_j softmax_j(logits / sqrt(d)) * (v[idx] + pe)."""

    @staticmethod
    def forward(ctx, logits, v, pe, idx):
        ctx.save_for_backward(logits, v, pe, idx)
        ctx.params = (v,)
        return ops.pt_softmax_agg(logits, v, pe, idx)

    @staticmethod
    def backward(ctx, dagg):
        logits, v, pe, idx = ctx.saved_tensors
        dlogits, dpe, dv = ops.pt_softmax_agg_bwd(logits, v, pe, idx, dagg.contiguous(), reduce_dv=False)
        if not torch.is_tensor(dv):
            # the kernel left the per-pair value gradients (dv = (dval, idx32, m)): their sum per abstract point is a
            # parameter-side reduction nothing below reads
            dval, idx32, m = dv
            (dv,) = _deposit(ctx.params, lambda: (ops.scatter_add_rows(dval, idx32, m),), dval, idx32)
        else:
            done = dv
            (dv,) = _deposit(ctx.params, lambda: (done,), done)
        return dlogits, dv, dpe, None


class SoftmaxAggGradOnlyFn(Function):
    """SoftmaxAggFn for a caller that only differentiates: the recompute-in-backward path rebuilds the pair tensors to
    back-propagate a GIVEN output gradient and never looks at the output value (the forward pass already produced it
    with the fused kernel), so forward returns an uninitialised tensor of the right shape and launches nothing."""

    @staticmethod
    def forward(ctx, logits, v, pe, idx):
        ctx.save_for_backward(logits, v, pe, idx)
        ctx.params = (v,)
        return logits.new_empty((idx.shape[0], v.shape[1]))

    backward = SoftmaxAggFn.backward


class MaxPoolGatherFn(Function):
    @staticmethod
    def forward(ctx, y, idx):
        ctx.save_for_backward(y, idx)
        return ops.maxpool_gather(y, idx)

    @staticmethod
    def backward(ctx, dz):
        y, idx = ctx.saved_tensors
        return ops.maxpool_gather_bwd(y, idx, dz.contiguous()), None


class LayerNormReluFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y = ops.layernorm(x, gamma, beta, eps=eps, relu=True)
        ctx.eps = eps
        ctx.save_for_backward(x, gamma, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, y = ctx.saved_tensors
        g = ops.relu_mask(dy.contiguous(), y)
        dx, dgamma, dbeta = ops.layernorm_bwd(x, gamma, g, ctx.eps)
        return dx, dgamma, dbeta, None


class BatchNormReluFn(Function):
    """BatchNorm1d in training mode + ReLU (model/modules.py:98-102,152).  Returns (out, batch mean, biased batch
    variance); the statistics are outputs without gradient (the module updates its running statistics from them)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, eps):
        out, mean, var = ops.bn_train_fwd(y, gamma, beta, eps)
        ctx.eps = eps
        ctx.save_for_backward(y, gamma, out, mean, var)
        ctx.mark_non_differentiable(mean, var)
        return out, mean, var

    @staticmethod
    def backward(ctx, g, _gm, _gv):
        y, gamma, out, mean, var = ctx.saved_tensors
        dx, dgamma, dbeta = ops.bn_train_bwd(y, g.contiguous(), out, mean, var, gamma, ctx.eps)
        return dx, dgamma, dbeta, None


class SwishFn(Function):
    """x sigmoid(x) (model/implicit.py:46-64, the reference's other activation) with its analytic backward."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.swish(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.swish_bwd(g.contiguous(), x)


def act_linear(x, lin, activation, residual=None):
    """lin(activation(x)) [+ residual] for the training path: 'relu' folds into the Linear kernels (relu_in), 'swish' is an
    element-wise pass in front of a plain Linear."""
    if activation == 'relu':
        return linear(x, lin, relu_in=True, residual=residual)
    if activation == 'swish':
        return linear(SwishFn.apply(x), lin, residual=residual)
    raise ValueError('Unknown activation: ' + str(activation))


class MeanRowsFn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.n = x.shape[0]
        return ops.mean_rows(x)

    @staticmethod
    def backward(ctx, dout):
        return ops.broadcast_rows(dout.contiguous(), ctx.n, 1.0 / ctx.n)


class ExpandRowsFn(Function):
    """v (d) -> (n, d), every row = v: `v[None].expand(n, d)` with a backward on the library's column-sum kernels.
    torch's own backward of expand is a multi-block reduction whose completion counters are cleared by a cudaMemsetAsync:
    inside a captured step that is a MEMSET NODE, and on this HIP runtime memset nodes are not ordered reliably against
    the kernel nodes around them (profiles/r04_graph_replay_probe.txt: the replayed step computed a wrong gradient for the
    global embedding whenever an eager kernel had run since the last device-wide synchronisation)."""

    @staticmethod
    def forward(ctx, v, n):
        return ops.broadcast_rows(v, n, 1.0)

    @staticmethod
    def backward(ctx, dout):
        return ops.colsum(dout), None


class InterpFn(Function):
    """y[i] = sum_j w[i,j] table[idx[i,j]]  (inverse-distance feature interpolation)."""

    @staticmethod
    def forward(ctx, table, idx, w):
        ctx.save_for_backward(idx, w)
        ctx.m = table.shape[0]
        y = torch.zeros((idx.shape[0], table.shape[1]), dtype=torch.float32, device=table.device)
        return ops.interp_add(y, None, table, idx, w)

    @staticmethod
    def backward(ctx, dy):
        idx, w = ctx.saved_tensors
        return ops.interp_bwd(dy.contiguous(), idx, w, ctx.m), None, None
