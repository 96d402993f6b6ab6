"""The reference's own caller driving this package's modules on the g++ twin (container-only, like gen_golden).

TEST INFRASTRUCTURE.  Run from the repo root where the reference is mounted (oracle/ref_import.py):

    python -m oracle.check_reference_caller

INTEGRATION.md section A, executed: the reference's eval/inference.py with `model` / `implicit` bound to this package.
ITS load_models (:23-80) builds the PRODUCT's networks from a reference-format checkpoint (constructor kwargs, state_dict
keys, legacy rename, fps_random_start override) and ITS perform_inference (:83-325) -- grid sampling, batch loop,
post-ops, threshold split -- calls the product's forwards.  The results must equal what the same code returned with the
reference's own modules (fixtures G17, G10).  Not part of tests/: it runs the reference's code, which the repository
does not contain; the suite pins the same outputs through the product's own load_models / perform_inference
(tests/test_checkpoint.py, tests/test_cpu_twin.py).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import golden_cases as gc  # noqa: E402
import occlusions4d_amd as pk  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def check_checkpoint_case(ref, case):
    inf_mod = ref.inference
    saved = (inf_mod.model, inf_mod.implicit)
    inf_mod.model, inf_mod.implicit = pk.model, pk.implicit        # sys.modules['model'] / ['implicit'] of section A
    real_load = torch.load
    torch.load = lambda *a, **k: real_load(*a, **dict(k, weights_only=False))     # (torch >= 2.6 default; the reference predates it)
    try:
        (nets, _, _, pcl_args, _, epoch) = inf_mod.load_models(os.path.join(GOLDEN, gc.CKPT_DIR), torch.device('cpu'),
                                                               epoch=case['epoch_arg'])
    finally:
        torch.load = real_load
        inf_mod.model, inf_mod.implicit = saved
    assert isinstance(nets[0], pk.model.PointCompletionNetV3) and isinstance(nets[1], pk.implicit.LocalPclResnetFC)
    assert epoch == case['epoch'] and pcl_args['fps_random_start'] is False
    for net in nets:
        net.eval()
    _, _, inf = gc.ckpt_model_args(case)
    pcl = pk.configs.synthetic_pcl(gc.CKPT_INFER['kind'], gc.CKPT_INFER['n'], gc.CKPT_INFER['video_len'], gc.CKPT_INFER['seed'])
    with torch.no_grad():                                            # (eval/test.py:32-34)
        res = inf_mod.perform_inference(
            pcl.clone(), None, None, nets, torch.device('cpu'), 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'],
            gc.CKPT_INFER['time_idx'], None, sample_implicit=True, num_sample=gc.CKPT_INFER['num_sample'],
            point_sample_mode='grid', batch_size=gc.CKPT_INFER['batch_size'], predict_segmentation=False,
            track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind=inf['data_kind'], cube_mode=4,
            compress_air=True)
    g = load_golden('g17_ckpt_' + case['name'])
    assert np.array_equal(res['pcl_abstract'][:, :3], g['pcl_abstract'][:, :3])
    assert np.abs(res['pcl_abstract'] - g['pcl_abstract']).max() < 1e-4
    assert np.abs(res['implicit_output'] - g['implicit_output']).max() < 1e-4
    assert res['output_solid'].shape[0] == int(g['n_solid'][0])


def check_config1(ref):
    """The same at BASELINE configs[0]: the reference's perform_inference over the product's networks = G10."""
    case = gc.INFER_CASES[0]
    g = load_golden('g10_infer_' + case['name'])
    pcl, pa, ia, inf, esd, dsd = gc.infer_inputs(case)
    enc = pk.model.PointCompletionNetV3(**pa).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).eval()
    dec.load_state_dict(dsd)
    kw = dict(sample_implicit=True, num_sample=case['num_sample'], point_sample_mode='grid', batch_size=case['batch_size'],
              predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13,
              density_threshold=0.5, data_kind=inf['data_kind'], cube_mode=4, compress_air=True)
    with torch.no_grad():
        res = ref.inference.perform_inference(pcl.clone(), None, None, [enc, dec], torch.device('cpu'), 'if', inf['min_z'],
                                              inf['cube_bounds'], inf['color_mode'], case['time_idx'], None, **kw)
    assert np.array_equal(res['pcl_abstract'][:, :3], g['pcl_abstract'][:, :3])
    assert np.abs(res['implicit_output'] - g['implicit_output']).max() < 1e-4
    assert res['output_solid'].shape[0] == int(g['n_solid'][0]) and res['output_air'].shape == (8640 - res['output_solid'].shape[0], 5)


def main():
    if not ref_import.available():
        print('check_reference_caller: the reference is not mounted here', file=sys.stderr)
        return 2
    ref = ref_import.load()
    with pk.cpu_twin.loaded():
        for case in gc.CKPT_CASES:
            check_checkpoint_case(ref, case)
            print('reference load_models + perform_inference over the product modules, checkpoint %s: ok' % case['name'])
        check_config1(ref)
        print('reference perform_inference over the product modules, %s: ok' % gc.INFER_CASES[0]['name'])
    return 0


if __name__ == '__main__':
    sys.exit(main())
