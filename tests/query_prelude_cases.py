"""Shared by tests/test_query_prelude_host.py (g++ twin) and tests/test_gpu_query_prelude.py (HIP library): one decoder over a small
random abstract cloud, and the forward computed both ways."""
import torch

import occlusions4d_amd as pk

ROWS = 300            # neither a multiple of 128 nor of 9


def scene_of(kind, device, seed=5):
    """(decoder, abstract xyz (m, 3), features (m, E), global embedding, queries (ROWS, 4)) at the smallest cloud the pruned
    sampler serves: model_args(kind, 1536), whose abstract cloud has 57 (GREATER) / 171 + 57 (CARLA) points."""
    pa, ia, _ = pk.configs.model_args(kind, 1536)
    _, dsd = pk.configs.synthetic_weights(pa, ia, seed)
    dec = pk.implicit.LocalPclResnetFC(**ia).eval()
    dec.load_state_dict(dsd)
    m = 57 if kind == 'greater' else 171 + 57
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand((m, 3), generator=g) * 4 - 2
    feats = torch.randn((m, ia['d_latent_local']), generator=g) * 0.5
    fglobal = torch.randn((ia['d_latent'] - ia['d_latent_local'],), generator=g) * 0.5
    q = torch.cat([torch.rand((ROWS, 3), generator=g) * 5 - 2.5, torch.randint(0, 4, (ROWS, 1), generator=g).float()], dim=1)
    return dec.to(device), xyz.to(device), feats.to(device), fglobal.to(device), q.to(device)


def prelude_buffers(w, n, device, with_x0):
    return dict(idx_local=torch.empty((n, w.k_local), dtype=torch.int32, device=device),
                w_local=torch.empty((n, w.k_local), dtype=torch.float32, device=device),
                idx_cross=torch.empty((n, w.k_cross), dtype=torch.int32, device=device),
                x0=torch.empty((n, w.d_hidden), dtype=torch.float32, device=device) if with_x0 else None,
                workspace=torch.empty((pk.ops.decoder_query_prelude_workspace(w, n),), dtype=torch.float32, device=device)
                if with_x0 else None)


def forward_both_ways(dec, xyz, feats, fglobal, q, with_x0):
    """((out, penult) of the entry that searches itself, (out, penult) of the entry on the prelude's rows, the buffers)."""
    sc = dec.prepare_scene(xyz, fglobal, feats)
    w, prepared, flags = dec.path_weights()
    ref = pk.ops.decoder_query_fwd(w, prepared, sc['scene'], sc['m'], q, flags)
    buf = prelude_buffers(w, q.shape[0], q.device, with_x0)
    pk.ops.decoder_query_prelude(w, xyz, q, buf['idx_local'], buf['w_local'], buf['idx_cross'], buf['x0'], buf['workspace'])
    kept = {k: None if v is None else v.clone() for k, v in buf.items()}
    got = pk.ops.decoder_query_fwd_prelude(w, prepared, sc['scene'], sc['m'], q, buf['idx_local'], buf['w_local'],
                                           buf['idx_cross'], buf['x0'], flags)
    return ref, got, kept
