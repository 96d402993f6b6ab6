"""Cross-attention local-implicit decoder on the HIP library.

Interface mirror of the reference's model/implicit.py: ``positional_encode`` (:20-43),
``ResnetBlockFC`` (:68-101), ``ResnetFC`` (:104-208) and ``LocalPclResnetFC`` (:211-445)
with the reference's constructor kwargs (the checkpoint's ``implicit_args``), parameter
names (lin_in, lin_out, lin_z.N, blocks.N.fc_{0,1}, pt_blocks.N.*) and
``forward(points_query, points_abstract, features_global, features_abstract)
-> (output, penult)``.

Exact-in-R refactorings used: (ii) lin_z[i](features_query) splits into a
per-scene constant (global half + bias) plus the inverse-distance interpolation of the
per-abstract-point table W_z^local f_j, because the interpolation is linear; per-scene
tables are computed once per abstract cloud, not once per call.
"""
import os

import torch

from . import geometry  # noqa: F401  (same module graph as the reference)
from . import kernels
from . import modules
from . import ops
from . import autograd
from . import point_transformer_layer as ptl
from .point_transformer_layer import needs_grad, weights_epoch



def positional_encode(points, base_frequency, num_powers):
    """(..., C) -> (..., C*(2F+1)): [p, sin(p w_0), cos(p w_0), ..., sin(p w_{F-1}), cos(p w_{F-1})],
    w_i = 2 pi base 2^i."""
    flat = points.reshape(-1, points.shape[-1])
    enc = ops.posenc(flat, num_powers, base_frequency)
    return enc.reshape(*points.shape[:-1], enc.shape[-1])


ACTIVATIONS = {'relu': 1, 'swish': 2}       # act_in codes of occ4d_linear_f32 (0 = none); swish = x * sigmoid(x) (:46-64)

# LocalPclResnetFC.query_prelude keeps lin_in's output of ALL queries (n * d_hidden * 4 bytes) only up to this many bytes;
# above, the prelude leaves the lists and weights and every mini-batch embeds its own rows.  4 GiB: the 2.1 M-query grid (3.5 GB)
PRELUDE_X0_MAX = int(os.environ.get('OCC4D_PRELUDE_X0_MAX', str(4 << 30)))


def _check_activation(name):
    if name not in ACTIVATIONS:
        raise ValueError('Unknown activation: ' + str(name))


def _trunk_pack(weight, kind):
    """Stage-packed copy of a (416, 416) weight for the fused residual-block kernel (ops.pack_trunk_rows / _cols =
    the library's packers), cached on the tensor object while (storage, version, weights epoch, variant) are unchanged."""
    if tuple(weight.shape) != (ops.TRUNK_WIDTH, ops.TRUNK_WIDTH) or not weight.is_cuda:
        return None
    trunk4 = kernels.scope().trunk4
    key = (weights_epoch(), weight.data_ptr(), weight._version, kind, trunk4)
    hit = getattr(weight, '_occ4d_trunk_pack', None)
    if hit is not None and hit[0] == key:
        return hit[1]
    if trunk4:
        packed = ops.pack_trunk4_rows(weight) if kind == 'rows' else ops.pack_trunk4_cols(weight)
    else:
        packed = ops.pack_trunk_rows(weight) if kind == 'rows' else ops.pack_trunk_cols(weight)
    weight._occ4d_trunk_pack = (key, packed)
    return packed


class ResnetBlockFC(torch.nn.Module):
    """x + fc_1(act(fc_0(act(x)))) (pre-activation residual block, DVR style)."""

    def __init__(self, d_in=64, d_hidden=256, d_out=64, activation='relu'):
        super().__init__()
        _check_activation(activation)
        self.activation = activation
        self.d_in, self.d_hidden, self.d_out = d_in, d_hidden, d_out
        self.fc_0 = torch.nn.Linear(d_in, d_hidden, bias=True)
        self.fc_1 = torch.nn.Linear(d_hidden, d_out, bias=True)
        self.shortcut = None if d_in == d_out else torch.nn.Linear(d_in, d_out, bias=False)

    def forward(self, x):
        flat = x.reshape(-1, x.shape[-1])
        if needs_grad(self, x):
            return self._run_train(flat).reshape(*x.shape[:-1], self.d_out)
        return self._run(flat).reshape(*x.shape[:-1], self.d_out)

    def _run_train(self, x):
        if (self.shortcut is None and self.activation == 'relu' and self.fc_0.bias is not None
                and self.fc_1.bias is not None):
            return autograd.resblock(x, self.fc_0, self.fc_1)          # one autograd node: skip gradient in the GEMM epilogue
        h = autograd.act_linear(x, self.fc_0, self.activation)
        xs = x if self.shortcut is None else autograd.linear(x, self.shortcut)
        return autograd.act_linear(h, self.fc_1, self.activation, residual=xs)

    def _run(self, x, inplace=False):
        act = ACTIVATIONS[self.activation]
        if (self.shortcut is None and kernels.scope().trunk_kernels and self.d_in == self.d_hidden == self.d_out
                and self.activation == 'relu'):
            # both layers in one kernel, the (n, d_hidden) intermediate never leaves the registers (csrc/trunk.hip)
            w0p, w1p = _trunk_pack(self.fc_0.weight, 'rows'), _trunk_pack(self.fc_1.weight, 'cols')
            if w0p is not None and w1p is not None:
                return ops.resblock(x, w0p, self.fc_0.bias, w1p, self.fc_1.bias, out=x if inplace else None)
        h = ops.linear(x, self.fc_0.weight, self.fc_0.bias, relu_in=act)
        if self.shortcut is None:
            return ops.linear(h, self.fc_1.weight, self.fc_1.bias, relu_in=act, residual=x,
                              out=x if inplace else None)
        xs = ops.linear(x, self.shortcut.weight)
        return ops.linear(h, self.fc_1.weight, self.fc_1.bias, relu_in=act, residual=xs, out=xs)


class ResnetFC(torch.nn.Module):
    """pixelNeRF-style conditioned residual MLP (global or per-point latent)."""

    def __init__(self, mixed_precision=False, d_in=4, d_hidden=256, d_out=64, d_latent=256,
                 n_blocks=5, pos_encoding_freqs=0, activation='relu'):
        super().__init__()
        _check_activation(activation)
        if mixed_precision:
            raise NotImplementedError('fp32 only (the reference default, args.py:55)')
        self.mixed_precision = mixed_precision
        self.activation = activation
        self.d_in, self.d_hidden, self.d_out, self.d_latent = d_in, d_hidden, d_out, d_latent
        self.n_blocks = n_blocks
        self.pos_encoding_freqs = pos_encoding_freqs
        self.actual_d_in = d_in * (pos_encoding_freqs * 2 + 1) if pos_encoding_freqs > 0 else d_in
        if self.actual_d_in > 0:
            self.lin_in = torch.nn.Linear(self.actual_d_in, d_hidden, bias=True)
        self.lin_out = torch.nn.Linear(d_hidden, d_out, bias=True)
        self.blocks = torch.nn.ModuleList(
            [ResnetBlockFC(d_hidden, d_hidden, d_hidden, activation=activation) for _ in range(n_blocks)])
        if d_latent > 0:
            self.lin_z = torch.nn.ModuleList(
                [torch.nn.Linear(d_latent, d_hidden, bias=True) for _ in range(n_blocks)])

    def forward(self, points, features):
        return self.do_forward(points, features)

    def _embed(self, pts):
        """(n, d_in) -> (n, H): Fourier features + lin_in."""
        if self.pos_encoding_freqs > 0:
            pts = ops.posenc(pts, self.pos_encoding_freqs, 0.1)
        return ops.linear(pts, self.lin_in.weight, self.lin_in.bias)

    def do_forward(self, points, features):
        """points (B,N,d_in) or (N,d_in); features (B,D) or (B,N,D) -> (output (B,N,G), penult (B,N,H))."""
        if needs_grad(self, points, features):
            raise NotImplementedError('training is implemented for the published configuration '
                                      "(local_mode='attention'); ResnetFC.do_forward is inference-only")
        no_batch = points.dim() == 2
        if no_batch:
            points, features = points[None], features[None]
        assert points.shape[0] == features.shape[0]
        assert points.shape[-1] == self.d_in and features.shape[-1] == self.d_latent
        assert self.d_in > 0
        outs, pens = [], []
        for b in range(points.shape[0]):
            x = self._embed(points[b])
            f = features[b]
            for i in range(self.n_blocks):
                if self.d_latent > 0:
                    lz = self.lin_z[i]
                    if f.dim() == 1:
                        # one global embedding steers every point: x += (W f + b), a row constant
                        z = ops.linear(f[None].contiguous(), lz.weight, lz.bias)[0]
                        n = x.shape[0]
                        ops.interp_add(x, z, x.new_zeros((1, self.d_hidden)),
                                       torch.zeros((n, 1), dtype=torch.int32, device=x.device),
                                       x.new_zeros((n, 1)))
                    else:
                        assert f.shape[0] == x.shape[0]
                        x = ops.linear(f, lz.weight, lz.bias, residual=x, out=x)
                x = self.blocks[i]._run(x, inplace=True)
            pens.append(x)
            outs.append(ops.linear(x, self.lin_out.weight, self.lin_out.bias, relu_in=ACTIVATIONS[self.activation]))
        output, penult = ops.stack_batch(outs), ops.stack_batch(pens)
        if no_batch:
            output, penult = output[0], penult[0]
        return (output, penult)


class LocalPclResnetFC(ResnetFC, kernels.HasKernelSelection):
    """ResnetFC + local feature interpolation + query-to-abstract vector cross-attention."""

    def __init__(self, num_local_features=0, local_mode='attention', d_latent_local=64,
                 cross_attn_neighbors=12, cross_attn_layers=1, cr_attn_type='cccccccccc', **kwargs):
        self.num_local_features = num_local_features
        self.local_mode = local_mode
        self.d_latent_local = d_latent_local
        self.cross_attn_neighbors = cross_attn_neighbors
        self.cross_attn_layers = cross_attn_layers
        self.cr_attn_type = cr_attn_type
        super().__init__(**kwargs)
        if local_mode == 'attention':
            blocks, use_at = [], []
            for i in range(cross_attn_layers):
                if cr_attn_type[i] == 'c':
                    blocks.append(modules.PointTransformerBlock(
                        self.d_latent, self.d_latent, self.d_latent, num_neighbors=cross_attn_neighbors,
                        d_hidden_abstract=d_latent_local))
                elif cr_attn_type[i] == 's':
                    raise NotImplementedError()
                else:
                    raise ValueError()
                use_at.append(int((i + 1) * self.n_blocks / (cross_attn_layers + 1)))
            self.pt_blocks = torch.nn.ModuleList(blocks)
            self.use_pt_inds = {j: i for i, j in enumerate(use_at)}
        self._scene = {}              # per flag value: the last abstract cloud's tables

    # -- the library's view of this module ------------------------------------------------
    def path_weights(self):
        """occ4d_decoder_weights over this module's parameters in the reference's layout and the library's prepared
        buffer for them (occ4d_decoder_prepare_f32: stage-packed residual blocks, merged + packed cross-attention
        layers).  Cached while the parameters (storage, version, weights epoch) and the kernel flags are unchanged."""
        flags = ptl.path_flags(self)
        # use_pt_inds {block: layer} is the reference's map (model/implicit.py:264-268) and, as there, what decides which
        # layer runs where: two layers the constructor's formula puts behind ONE block share a key, the later one
        # shadows the earlier (whose parameters stay in the state dict and are never run)
        live = tuple(sorted(self.use_pt_inds.items())) if self.local_mode == 'attention' else ()
        key = (flags, weights_epoch(), live) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        cache = self.__dict__.setdefault('_path', {})       # one entry per flag value (threads under different selections)
        hit = cache.get(flags)
        if hit is not None and hit[0] == key:
            return hit[1], hit[2], flags
        L = ops._lib
        assert self.n_blocks <= L.MAX_BLOCKS and len(live) <= L.MAX_CROSS
        assert all(0 <= i < self.n_blocks and 0 <= j < len(self.pt_blocks) for i, j in live), live
        keep = []

        def dp(t):
            t = t.detach()
            if not t.is_contiguous():
                t = t.contiguous()
            ops._dev(t, name='parameter')                  # (RuntimeError for CPU tensors: there is no fallback path)
            keep.append(t)
            return t.data_ptr()
        p_in = self.actual_d_in
        w_in = self.lin_in.weight.detach()
        if p_in % 4:                                   # rows zero-padded to a multiple of 4 floats (vector loads)
            w_in = torch.nn.functional.pad(w_in, (0, 4 - p_in % 4))
        w = L.DecoderWeights(d_in=self.d_in, n_freq=self.pos_encoding_freqs, d_hidden=self.d_hidden, d_out=self.d_out,
                             d_latent=self.d_latent, d_latent_local=self.d_latent_local, n_blocks=self.n_blocks,
                             n_cross=len(live),
                             k_local=self.num_local_features, k_cross=self.cross_attn_neighbors,
                             activation=ACTIVATIONS[self.activation] - 1, lin_in_ld=w_in.shape[1], base_frequency=0.1)
        w.lin_in_w, w.lin_in_b = dp(w_in), dp(self.lin_in.bias)
        w.lin_out_w, w.lin_out_b = dp(self.lin_out.weight), dp(self.lin_out.bias)
        for i in range(self.n_blocks):
            w.lin_z_w[i], w.lin_z_b[i] = dp(self.lin_z[i].weight), dp(self.lin_z[i].bias)
            w.fc0_w[i], w.fc0_b[i] = dp(self.blocks[i].fc_0.weight), dp(self.blocks[i].fc_0.bias)
            w.fc1_w[i], w.fc1_b[i] = dp(self.blocks[i].fc_1.weight), dp(self.blocks[i].fc_1.bias)
        for j, (after, layer) in enumerate(live):          # cross[j]: the layer that runs behind the j-th position, ascending
            blk = self.pt_blocks[layer]
            lw, _, _ = blk.layer2.path_weights(cross=True, pre=blk.layer1, post=blk.layer3, flags=flags)
            w.cross[j] = lw
            keep.append(lw)
            w.cross_after[j] = after
        w._keep = keep
        prepared = ops.decoder_prepare(w, flags, self.lin_out.weight.device)
        cache[flags] = (key, w, prepared)
        return w, prepared, flags

    def _library_path_ok(self):
        return (self.num_local_features > 0 and self.local_mode in ('feature', 'attention') and self.d_latent > 0
                and self.d_latent_local > 0 and all(b.shortcut is None and b.d_hidden == self.d_hidden for b in self.blocks)
                and self.d_hidden % 4 == 0 and self.d_latent_local % 4 == 0 and (self.d_latent - self.d_latent_local) % 4 == 0)

    # -- per-scene precompute ---------------------------------------------------------
    def prepare_scene(self, points_abstract, features_global, features_abstract=None):
        """Per-scene tables of the library (occ4d_decoder_prepare_scene_f32): abstract xyz packed, Z = F [Wz_0^loc; ..]^T
        (M, n_blocks*H), c = [Wz_i^glob g + b_i] (n_blocks*H), and per cross layer (W1 Wk) F, Wv F, Wv F + c2 -- the
        reference recomputes to_k / to_v per forward call.  Cached on the identity (+version) of the
        tensors the caller passes, which are kept alive here so their storage cannot be recycled."""
        w, prepared, flags = self.path_weights()
        key = (id(points_abstract), points_abstract._version, id(features_global), features_global._version,
               id(features_abstract), None if features_abstract is None else features_abstract._version,
               id(prepared), flags)
        sc = self._scene.get(flags)
        if sc is not None and sc['key'] == key and sc['owners'][0] is points_abstract \
                and sc['owners'][1] is features_global and sc['owners'][2] is features_abstract:
            return sc
        pa, fa, fg = points_abstract, features_abstract, features_global
        if fa is None:
            fa = pa[..., 3:]
            pa = pa[..., :3]
        if pa.dim() == 3:
            assert pa.shape[0] == 1, 'LocalPclResnetFC supports B == 1 only (model/implicit.py:317)'
            pa, fa = pa[0], fa[0]
        if fg.dim() == 2:
            assert fg.shape[0] == 1
            fg = fg[0]
        assert pa.shape[0] == fa.shape[0]
        assert fa.shape[-1] == self.d_latent_local
        assert fg.shape[-1] == self.d_latent - self.d_latent_local
        sc = dict(key=key, owners=(points_abstract, features_global, features_abstract), m=pa.shape[0], prepared=prepared,
                  scene=ops.decoder_prepare_scene(w, prepared, pa, fa, fg, flags))
        self._scene[flags] = sc
        return sc

    # -- forward ----------------------------------------------------------------------
    def forward(self, points_query, points_abstract, features_global, features_abstract, knn_local=None, knn_cross=None):
        """points_query (B,N,4) or (N,4); points_abstract (B,M,3) (or (B,M,3+E) with
        features_abstract None); features_global (B,D); features_abstract (B,M,E).
        B must be 1.  Returns (output (B,N,G), penult (B,N,H)) (no batch dim if none came in).
        Inference: ONE library call per mini-batch (occ4d_decoder_query_fwd_f32) on per-scene tables built once per
        abstract cloud (occ4d_decoder_prepare_scene_f32).
        Extension (keyword only in spirit; the reference's four positionals are unchanged): knn_local (N, 8) /
        knn_cross (N, 14) integer tensors = the caller's own neighbour lists of the abstract cloud -- what
        geometry.my_knn_torch (model/implicit.py:328) and kNN_torch (model/point_transformer_layer.py:167) returned in
        the run to be reproduced.  The reference orders equidistant points with an unstable sort; CARLA's two-level
        abstract cloud holds every coarse point twice (model/model.py:202-228), so there its choice at the k-th rank is
        implementation-defined and only the run's own lists pin it.  None = searched here, lowest index first.
        Kernel variants / precision: the calling thread's `kernels.use(...)` scope with this module's `kernel_selection`
        on top (kernels.py); the nested layers run under the same selection."""
        with kernels.use(kernels.current(self)):
            return self._forward(points_query, points_abstract, features_global, features_abstract, knn_local, knn_cross)

    def _forward(self, points_query, points_abstract, features_global, features_abstract, knn_local=None, knn_cross=None):
        if needs_grad(self, points_abstract, features_global, features_abstract):
            return self._forward_train(points_query, points_abstract, features_global, features_abstract,
                                       knn_local=knn_local, knn_cross=knn_cross)
        if self.num_local_features <= 0:
            return super().do_forward(points_query, features_global)
        if self.local_mode == 'function':
            raise NotImplementedError()
        if self.local_mode not in ('feature', 'attention'):
            raise ValueError()
        no_batch = points_query.dim() == 2
        if not no_batch:
            assert points_query.shape[0] == 1, 'LocalPclResnetFC supports B == 1 only'
            assert points_abstract.shape[0] == 1 and features_global.shape[0] == 1
        q = points_query if no_batch else points_query[0]
        assert q.shape[-1] == self.d_in
        assert self._library_path_ok(), 'unsupported LocalPclResnetFC configuration for the HIP library'
        sc = self.prepare_scene(points_abstract, features_global, features_abstract)
        w, prepared, flags = self.path_weights()
        if knn_local is not None and knn_local.dim() == 3:
            knn_local = knn_local[0]
        if knn_cross is not None and knn_cross.dim() == 3:
            knn_cross = knn_cross[0]
        output, penult = ops.decoder_query_fwd(w, prepared, sc['scene'], sc['m'], q, flags, knn_local=knn_local,
                                               knn_cross=knn_cross)
        if not no_batch:
            output, penult = output[None], penult[None]
        return (output, penult)

    def forward_output_only(self, points_query, points_abstract, features_global, features_abstract, out,
                            knn_local=None, knn_cross=None, prelude=None):
        """Extension for the device-resident driver (inference.decode_batches): the raw outputs of one mini-batch
        written straight into `out` (a row slice of the caller's result tensor); the penultimate activation, which
        perform_inference discards (eval/inference.py:211), is not materialised for the caller.  `prelude`: (buffers of
        query_prelude over a query tensor, first row, end row) -- points_query is that tensor's [first:end] slice and the
        searches, the weights and the embedding of these rows are taken from the buffers (x0's rows are consumed)."""
        assert not needs_grad(self, points_abstract, features_global, features_abstract)
        assert self.num_local_features > 0 and self._library_path_ok() and points_query.dim() == 2
        with kernels.use(kernels.current(self)):
            sc = self.prepare_scene(points_abstract, features_global, features_abstract)
            w, prepared, flags = self.path_weights()
            if prelude is not None:
                assert knn_local is None and knn_cross is None
                buf, b, e = prelude
                assert buf['m'] == sc['m'] and e - b == points_query.shape[0]
                ops.decoder_query_fwd_prelude(w, prepared, sc['scene'], sc['m'], points_query, buf['idx_local'][b:e],
                                              buf['w_local'][b:e], None if buf['idx_cross'] is None else buf['idx_cross'][b:e],
                                              None if buf['x0'] is None else buf['x0'][b:e], flags, out=out, want_penult=False)
                return out
            ops.decoder_query_fwd(w, prepared, sc['scene'], sc['m'], points_query, flags, out=out, want_penult=False,
                                  knn_local=knn_local, knn_cross=knn_cross)
        return out

    def query_prelude(self, points_query, xyz_abstract):
        """The query front end of a whole decode in one pass (occ4d_decoder_query_prelude_f32): the two neighbour lists and
        the interpolation weights of points_query (n, d_in) over the abstract coordinates xyz_abstract (m, 3), and lin_in's
        output x0 while n * d_hidden * 4 bytes <= PRELUDE_X0_MAX.  Needs no encoder feature, so inference.QueryPrelude
        issues it beside the encoder.  The buffers are this module's, one set per device (replaced when n changes), rewritten
        by the next call, which waits for buffers['released'] when the reader has left an event there (decode_batches does)."""
        assert points_query.dim() == 2 and points_query.shape[1] == self.d_in and self._library_path_ok()
        n, dev = points_query.shape[0], points_query.device
        with kernels.use(kernels.current(self)):
            w, _, _ = self.path_weights()
            cache = self.__dict__.setdefault('_prelude_buffers', {})
            want_x0 = n * self.d_hidden * 4 <= PRELUDE_X0_MAX
            buf = cache.get(dev)
            if buf is not None and buf.get('released') is not None:
                # (the last decode that read the buffers may have run on another stream than this call's)
                torch.cuda.current_stream().wait_event(buf['released'])
            if buf is None or buf['n'] != n or (buf['x0'] is not None) != want_x0:
                cache.pop(dev, None)          # (dropped first: the old set's blocks are free for the new one)
                del buf
                buf = cache[dev] = dict(
                    n=n,
                    idx_local=torch.empty((n, w.k_local), dtype=torch.int32, device=dev),
                    w_local=torch.empty((n, w.k_local), dtype=torch.float32, device=dev),
                    idx_cross=torch.empty((n, w.k_cross), dtype=torch.int32, device=dev) if w.n_cross else None,
                    x0=torch.empty((n, self.d_hidden), dtype=torch.float32, device=dev) if want_x0 else None,
                    workspace=torch.empty((ops.decoder_query_prelude_workspace(w, n),), dtype=torch.float32, device=dev)
                    if want_x0 else None)
            buf['m'] = xyz_abstract.shape[0]
            ops.decoder_query_prelude(w, xyz_abstract, points_query, buf['idx_local'], buf['w_local'], buf['idx_cross'],
                                      buf['x0'], buf['workspace'])
        return buf

    # -- training path (as-written op order, differentiable kernels) ------------------------
    def _forward_train(self, points_query, points_abstract, features_global, features_abstract, knn_local=None,
                       knn_cross=None):
        """Same contract as forward(); every op is a occlusions4d_amd.autograd Function, so gradients
        reach this module's parameters and, through features_abstract / features_global, the encoder."""
        assert self.local_mode == 'attention' and self.num_local_features > 0, \
            "training is implemented for the published configuration (local_mode='attention')"
        no_batch = points_query.dim() == 2
        q = points_query if no_batch else points_query[0]
        pa, fa, fg = points_abstract, features_abstract, features_global
        if fa is None:
            fa, pa = pa[..., 3:], pa[..., :3]
        if pa.dim() == 3:
            assert pa.shape[0] == 1, 'LocalPclResnetFC supports B == 1 only (model/implicit.py:317)'
            pa, fa = pa[0], fa[0]
        if fg.dim() == 2:
            fg = fg[0]
        pa = pa.detach().contiguous()
        fa = fa.contiguous()
        n = q.shape[0]
        dg = self.d_latent - self.d_latent_local
        m_abs = pa.shape[0]
        if knn_local is not None:            # (shape-checked and clamped into [0, m): the gathers below are unchecked -- ADVICE r5)
            idx8 = ops._neighbour_list(knn_local[0] if knn_local.dim() == 3 else knn_local, n, self.num_local_features,
                                       'knn_local', m=m_abs)
            dist = ops.knn_dists(q, pa, idx8, metric=1)
        else:
            idx8, dist = ops.knn(q, pa, self.num_local_features, metric=1, return_dist=True)
        w8 = ops.interp_weights(dist)
        f_local = autograd.InterpFn.apply(fa, idx8, w8)                                   # (n, E)
        f_query = torch.cat([autograd.ExpandRowsFn.apply(fg, n), f_local], dim=-1)         # (n, D)
        x = autograd.linear(ops.posenc(q, self.pos_encoding_freqs, 0.1), self.lin_in)
        qxyz = q[:, :3].detach()
        idx_att = None
        if knn_cross is not None:
            idx_att = ops._neighbour_list(knn_cross[0] if knn_cross.dim() == 3 else knn_cross, n, self.cross_attn_neighbors,
                                          'knn_cross', m=m_abs)
        fan = autograd.FanOut(self.n_blocks)       # f_query feeds one lin_z layer per block: one running gradient sum
        for i in range(self.n_blocks):
            x = autograd.linear(f_query, self.lin_z[i], residual=x, fan=fan)
            x = self.blocks[i]._run_train(x)
            if i in self.use_pt_inds:
                blk = self.pt_blocks[self.use_pt_inds[i]]
                y = autograd.linear(x, blk.layer1)
                if idx_att is None:       # one kNN_torch for all cross-attention layers (same xyz on both sides, same K)
                    idx_att = ops.knn(qxyz, pa, self.cross_attn_neighbors, metric=0)
                agg = blk.layer2._forward(y[None], qxyz[None], fa[None], pa[None], pre=None,
                                          knn_idx=idx_att[None])[0]
                x = autograd.linear(agg, blk.layer3, residual=x)
        output = autograd.act_linear(x, self.lin_out, self.activation)
        penult = x
        if not no_batch:
            output, penult = output[None], penult[None]
        return (output, penult)
