"""Point-transformer encoder on the HIP library.

Interface mirror of the reference's model/model.py ``PointCompletionNetV3``
(:12-233): constructor kwargs (the checkpoint's ``pcl_args``), parameter names
(pre_mlp, blocks.N, global_mlp, abstract_skip_mlps) and
``forward(pcl, return_intermediate) -> (pcl_out, x_global, layer_coords)``.
Only the published inference configuration is built: enable_decoder=False,
skip_connections=False (train.py:216-224); the UpTransition branch is out of scope.
"""
import contextlib

import torch

from . import modules
from . import ops
from . import autograd
from .point_transformer_layer import needs_grad


class PointCompletionNetV3(torch.nn.Module):

    def __init__(self, mixed_precision=False, n_input=4096, n_output=1024, d_in=6, d_out=6,
                 d_feat=32, down_blocks=3, up_blocks=2, transition_factor=4,
                 pt_num_neighbors=16, pt_norm_type='none', down_neighbors=8, abstract_levels=1,
                 skip_connections=False, enable_decoder=False, output_featurized=True,
                 output_global_emb=True, global_dim=512, fps_random_start=True):
        super().__init__()
        if enable_decoder or skip_connections:
            raise NotImplementedError('the UpTransition decoder branch is unused by every published '
                                      'configuration (train.py:223) and is out of scope')
        if mixed_precision:
            raise NotImplementedError('fp32 only (the reference default, args.py:55)')
        for k, v in dict(locals()).items():
            if k not in ('self', '__class__'):
                setattr(self, k, v)
        dim = d_feat
        self.pre_mlp = torch.nn.Sequential(torch.nn.Linear(d_in, dim), torch.nn.ReLU(),
                                           torch.nn.Linear(dim, dim))
        blocks = []
        for _ in range(down_blocks):
            blocks.append(modules.PointTransformerBlock(dim, dim, dim, num_neighbors=pt_num_neighbors))
            blocks.append(modules.DownTransition(dim, dim * 2, factor=transition_factor, knn_k=down_neighbors,
                                                 norm_type=pt_norm_type, fps_random_start=fps_random_start))
            dim *= 2
        blocks.append(modules.PointTransformerBlock(dim, dim, dim, num_neighbors=pt_num_neighbors))
        self.center_block_idx = len(blocks) - 1
        if output_global_emb:
            self.global_mlp = torch.nn.Sequential(torch.nn.Linear(dim, global_dim), torch.nn.ReLU(),
                                                  torch.nn.Linear(global_dim, global_dim))
        if abstract_levels > 1:
            self.abstract_skip_mlps = torch.nn.ModuleList(
                [torch.nn.Linear(dim // int(2 ** (abstract_levels - 1 - lv)), dim)
                 for lv in range(abstract_levels - 1)])
        self.blocks = torch.nn.ModuleList(blocks)

    def _geometry_chain(self, pos, full=False, ready=None):
        """The coordinate-only work of the encoder on a side stream: FPS -> sub-cloud of every DownTransition (the FPS
        steps are a multi-ms single-CU dependent chain that would otherwise serialise the whole encode) and the kNNs of
        the levels that only exist once the FPS has run.  Returns {block index: (per-batch geometry, clouds, event)}; the
        main stream waits on the event right before the block needs it.
          DownTransition i   -> [(inds, p_sub[, nn_idx])]: the pooling neighbours are included when they can be derived
                                here -- a row gather of the preceding block's self-kNN lists
                                (modules.pool_neighbours_from_self_knn: no kNN launch) -- or, full=True, computed here.
          PointTransformerBlock i -> [self-kNN (N_l, K) int32] for every level BELOW the first (their clouds come out of
                                the FPS; with the nested levels of DESIGN.md 4 (iv) all of them right after level 0's
                                launch, so these kNNs run beside the feature chain instead of inside it), and for the
                                first level too when full=True (prefetch_geometry: nothing of it is left to forward()).
        `ready`: an event after which `pos` is complete; without it the side stream waits for everything queued on the
        current stream."""
        on_device = pos.is_cuda                 # (host tensors: the explicit CPU twin -- the same chain, in line)
        out = {}
        if on_device:
            main = torch.cuda.current_stream()
            if self._geom_stream is None:
                self._geom_stream = torch.cuda.Stream()
            side = self._geom_stream
            if ready is not None:
                side.wait_event(ready)
            else:
                side.wait_stream(main)

        def publish(i, payload, clouds):
            if not on_device:
                out[i] = (payload, clouds, None)
                return
            for item in payload:                # produced on `side`, consumed on `main`
                for t in (item if isinstance(item, tuple) else (item,)):
                    t.record_stream(main)
            ev = torch.cuda.Event()
            ev.record(side)
            out[i] = (payload, clouds, ev)
        with (torch.cuda.stream(side) if on_device else contextlib.nullcontext()):
            cur = [ops.copy_rows(pos[b]) for b in range(pos.shape[0])]     # (the stride-8 xyz view, packed)
            nested = [modules.NestedFps() for _ in cur]      # (the levels' farthest-point subsets are prefixes of level 0's)
            for c in cur:
                # allocated on the side stream, read by kernels on the main stream: without this the block could be
                # recycled by a later side-stream allocation while such a kernel is still queued
                if on_device:
                    c.record_stream(main)
            self_idx = None                     # self-kNN lists of `cur` when they were computed on this stream
            deferred = []                       # (block index, clouds) of the levels' self-kNNs: issued after ALL sampling
            for i, block in enumerate(self.blocks):
                if isinstance(block, modules.DownTransition):
                    g = [block.sample(c, nested=nf) for c, nf in zip(cur, nested)]
                    if modules.POOL_FROM_SELF_KNN and self_idx is not None and self_idx[0].shape[1] >= block.knn_k:
                        g = [(inds, p_sub, modules.pool_neighbours_from_self_knn(sx, inds, block.knn_k))
                             for (inds, p_sub), sx in zip(g, self_idx)]
                    elif full:
                        g = [(inds, p_sub, block.neighbours(p_sub, c)) for (inds, p_sub), c in zip(g, cur)]
                    publish(i, g, cur)
                    cur = [t[1] for t in g]
                    self_idx = None
                elif full:
                    self_idx = [ops.knn(c, c, block.num_neighbors, metric=0) for c in cur]
                    publish(i, self_idx, cur)
                elif i > 0:
                    if all(nf.order is not None for nf in nested):
                        # nested levels: no FPS launch is left behind this point (the further subsets are index arithmetic),
                        # and this level's lists are what the feature chain waits for next
                        publish(i, [ops.knn(c, c, block.num_neighbors, metric=0) for c in cur], cur)
                    else:
                        deferred.append((i, block, cur))
            # forward() path with one FPS launch per level: the sampling chain first (nothing may delay an FPS), then the
            # self-kNNs of the lower levels
            for i, block, clouds in deferred:
                publish(i, [ops.knn(c, c, block.num_neighbors, metric=0) for c in clouds], clouds)
        return out

    def prefetch_geometry(self, pcl, ready=None):
        """Issues the coordinate-only part of forward(pcl) -- the FPS chain and every kNN of the encoder -- NOW, on the
        geometry stream; the next forward() called with this very tensor (same storage, same version) picks the
        results up instead of computing them.  A training loop calls it for batch i + 1 once batch i's forward is
        launched (training.TrainStep does, given `next_pcl_input`): the 23 ms FPS chain of a 28672-point cloud then runs
        under batch i's backward instead of in front of batch i + 1's forward -- the reference hides the same work in
        its dataloader workers (utils/geometry.py:353-364).  With fps_random_start the start indices are drawn from
        torch's CPU generator at this call rather than inside forward().  `ready` (optional torch.cuda.Event): `pcl` is
        complete once it has fired; by default the geometry stream waits for all work queued on the current stream.
        Returns the geometry (also kept for the next forward)."""
        pos = pcl[..., :3].detach()
        geom = self._geometry_chain(pos, full=True, ready=ready)
        # the tensor OBJECT is kept (alive, so its address cannot be recycled by another cloud) next to the
        # (storage, version, shape) key; forward() requires both to match
        self._prefetched = (self.geometry_key(pcl), geom, pcl)
        return geom

    def abstract_level_sizes(self, n_points):
        """Point counts of the levels that enter the abstract cloud, in pcl_abstract's row order (largest first)."""
        sizes = [n_points]
        for _ in range(self.down_blocks):
            sizes.append(-(-sizes[-1] // self.transition_factor))
        return sizes[len(sizes) - self.abstract_levels:]

    def abstract_xyz_early(self, pcl, stream=None):
        """The coordinates forward(pcl) will return in pcl_abstract[..., :3], as an (M, 3) tensor, after a SHORT sampling
        launch instead of the whole chain: -> (xyz, event recorded behind it), or None when they cannot be had early.
        With the nested levels of DESIGN.md 4 (iv) every level's subset is a prefix of level 0's selection order, so the
        largest abstract level (531 of 4779 picks for GREATER, 1593 for CARLA's two levels) is what the SAME sampling
        kernel with the same start index selects when asked for that many samples; the smaller levels follow by
        modules.NestedFps' index arithmetic and the rows by the library's gather kernel: the chain's own expressions,
        bit for bit (as long as the picks are distinct points, which the chain's prefix property presumes too).  The
        launches go to `stream` (default: a stream of this module's own) behind the work queued on the current stream;
        forward() is not changed and still runs the full chain."""
        downs = [b for b in self.blocks if isinstance(b, modules.DownTransition)]
        if (not pcl.is_cuda or pcl.dim() != 3 or pcl.shape[0] != 1 or not modules.NESTED_FPS or not self.output_featurized
                or any(b.fps_random_start for b in downs) or pcl.shape[1] >= ops.FPS_COOP_MIN_POINTS or pcl.requires_grad
                or not 1 <= self.abstract_levels <= len(downs)):
            return None          # (above the single-workgroup sampler's range a second cooperative launch is not worth its spin)
        sizes = self.abstract_level_sizes(pcl.shape[1])
        if self._early_stream is None and stream is None:
            self._early_stream = torch.cuda.Stream()
        side = stream if stream is not None else self._early_stream
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            pos = pcl[0, :, :3].detach()
            orig, order = ops.fps_auto(pos, sizes[0], start=0, return_order=True)
            xyz = torch.empty((sum(sizes), 3), dtype=torch.float32, device=pcl.device)
            at = 0
            for lv, m in enumerate(sizes):
                if lv > 0:
                    _, orig = ops.nested_fps_level(order, orig, m)
                ops.gather_rows(pos, orig, out=xyz[at:at + m])
                at += m
            ev = torch.cuda.Event()
            ev.record(side)
        xyz.record_stream(main)
        return xyz, ev

    _early_stream = None

    @staticmethod
    def geometry_key(pcl):
        return (pcl.data_ptr(), pcl._version, tuple(pcl.shape))

    _prefetched = None

    _geom_stream = None

    def forward(self, pcl, return_intermediate):
        """pcl (B,N,d_in) rows (x,y,z,...) -> (pcl_out (B,M,3+D) | None, x_global (B,F) | None,
        layer_coords list | None)."""
        train = needs_grad(self, pcl)
        B = pcl.shape[0]
        pos = pcl[..., :3].detach()
        layer_coords = [pos, pos] if return_intermediate else None
        l0, l2 = self.pre_mlp[0], self.pre_mlp[2]
        if train:
            x = ops.stack_batch([autograd.linear(autograd.linear(pcl[b], l0, relu_out=True), l2) for b in range(B)])
        else:
            x = ops.stack_batch([ops.linear(ops.linear(pcl[b], l0.weight, l0.bias, relu_out=True), l2.weight, l2.bias)
                             for b in range(B)])
        skips = []
        x_global = None
        pre, self._prefetched = self._prefetched, None
        if pre is not None and pre[2] is pcl and pre[0] == self.geometry_key(pcl):
            geom = pre[1]
        else:
            geom = self._geometry_chain(pos)
        self_idx = None          # self-kNN lists of the current level (the next DownTransition's pooling lists are a prefix)
        for i, block in enumerate(self.blocks):
            if isinstance(block, modules.DownTransition):
                g, clouds, ev = geom[i]
                if ev is not None:
                    torch.cuda.current_stream().wait_event(ev)
                if len(g[0]) == 2:
                    if modules.POOL_FROM_SELF_KNN and self_idx is not None and self_idx[0].shape[1] >= block.knn_k:
                        g = [(inds, p_sub, modules.pool_neighbours_from_self_knn(sx, inds, block.knn_k))
                             for (inds, p_sub), sx in zip(g, self_idx)]
                    else:
                        g = [(inds, p_sub, block.neighbours(p_sub, c)) for (inds, p_sub), c in zip(g, clouds)]
                (x, pos) = block(x, pos, geometry=g)
                self_idx = None
            else:
                if i in geom:
                    self_idx, _, ev = geom[i]
                    if ev is not None:
                        torch.cuda.current_stream().wait_event(ev)
                else:
                    # (the first level's lists: on the main stream, beside the FPS of the geometry stream)
                    self_idx = [ops.knn(pos[b], pos[b], block.num_neighbors, metric=0) for b in range(B)]
                (x, pos) = block(x, pos, knn_idx=self_idx)
            if self.output_global_emb and i == self.center_block_idx:
                g0, g2 = self.global_mlp[0], self.global_mlp[2]
                if train:
                    x_global = ops.stack_batch([
                        autograd.linear(autograd.linear(autograd.MeanRowsFn.apply(x[b])[None], g0, relu_out=True),
                                        g2)[0] for b in range(B)])
                else:
                    x_global = ops.stack_batch([
                        ops.linear(ops.linear(ops.mean_rows(x[b])[None], g0.weight, g0.bias, relu_out=True),
                                   g2.weight, g2.bias)[0] for b in range(B)])
            if return_intermediate:
                layer_coords.append(pos)
            if self.abstract_levels > 1 and isinstance(block, modules.DownTransition):
                for j, skip in enumerate(self.abstract_skip_mlps):
                    if skip.in_features == x.shape[-1]:
                        if train:
                            y = ops.stack_batch([autograd.linear(x[b], skip) for b in range(B)])
                            y = torch.cat([y[..., :-1], torch.full_like(y[..., :1], j + 1.0)], dim=-1)
                            skips.append(torch.cat([pos, y], dim=-1))
                        else:     # (kept as parts: written in place into the output below)
                            skips.append((pos, [ops.linear(x[b], skip.weight, skip.bias) for b in range(B)], j + 1.0))
        if self.output_featurized and not train:
            # pos | features of every level written IN PLACE into one (B, M, 3 + D) tensor by the library's row-copy /
            # fill kernels (model/model.py:217-228: cat([pos, x]), level id in the last channel, cat of the levels)
            parts = skips + [(pos, [x[b] for b in range(B)], float(self.abstract_levels))]
            assert len(parts) == self.abstract_levels
            total = sum(p.shape[1] for p, _, _ in parts)
            D = x.shape[-1]
            pcl_out = torch.empty((B, total, 3 + D), dtype=torch.float32, device=x.device)
            at = 0
            for p, feats, level in parts:
                n = p.shape[1]
                for b in range(B):
                    rows = pcl_out[b, at:at + n]
                    ops.copy_rows(p[b], out=rows[:, :3])
                    ops.copy_rows(feats[b], out=rows[:, 3:])
                    if self.abstract_levels > 1:
                        ops.fill_rows(rows[:, -1:], level)
                at += n
        elif self.output_featurized:
            pcl_out = torch.cat([pos, x], dim=-1)
            if self.abstract_levels > 1:
                # (no in-place write on a taped tensor)
                pcl_out = torch.cat([pcl_out[..., :-1],
                                     torch.full_like(pcl_out[..., :1], float(self.abstract_levels))], dim=-1)
                assert len(skips) == self.abstract_levels - 1
                pcl_out = torch.cat([torch.cat(skips, dim=1), pcl_out], dim=1)
        else:
            pcl_out = None
        return (pcl_out, x_global, layer_coords)
