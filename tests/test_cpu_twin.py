"""The g++ twin of the C ABI (occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp -> libocc4d_cpu.so; SURVEY.md 8(b): "each with a
CPU twin compiled by g++ for config 1"; BASELINE configs[0]: "runs without a GPU").  Explicit opt-in only
(occlusions4d_amd.cpu_twin.enable()); the product stays loud without the HIP library (test_abi.py).

BASELINE configs[0] through the PRODUCT modules (PointCompletionNetV3, LocalPclResnetFC, perform_inference) on the twin =
the reference's golden run G10.  (The REFERENCE's own eval/inference.py driving the product modules, INTEGRATION.md
section A, needs the reference's code and runs where it is mounted: oracle/check_reference_caller.py.)"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import occlusions4d_amd as pk
from conftest import load_golden


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def _kw(case, inf):
    return dict(sample_implicit=True, num_sample=case['num_sample'], point_sample_mode='grid', batch_size=case['batch_size'],
                predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13,
                density_threshold=0.5, data_kind=inf['data_kind'], cube_mode=4, compress_air=True)


def test_the_twin_is_never_loaded_unasked():
    assert not pk.cpu_twin.enabled() and not pk._lib.is_twin()
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        pk.ops.knn(torch.zeros(4, 3), torch.zeros(4, 3), 2)            # CPU tensors: rejected, no fallback
    with pk.cpu_twin.loaded():
        assert pk._lib.lib().occ4d_is_cpu_twin() == 1
        idx = pk.ops.knn(torch.tensor([[0., 0, 0]]), torch.tensor([[1., 0, 0], [0.5, 0, 0], [3, 0, 0]]), 2)
        assert idx.tolist() == [[1, 0]]
        with pytest.raises(NotImplementedError, match='not part of the CPU twin'):
            pk._lib.lib().occ4d_pack_trunk_rows_f32(None, 0, 0, None, None)
    assert not pk.cpu_twin.enabled()
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        pk.ops.knn(torch.zeros(4, 3), torch.zeros(4, 3), 2)


def test_twin_exports_the_header_prototypes_of_the_minimum_set(twin):
    lib = pk._lib.lib()
    for name in ('occ4d_knn_f32', 'occ4d_fps_f32', 'occ4d_fps_start_f32', 'occ4d_linear_f32', 'occ4d_pt_layer_prepare_f32',
                 'occ4d_pt_layer_fwd_f32', 'occ4d_down_pool_fwd_f32', 'occ4d_decoder_prepare_f32',
                 'occ4d_decoder_prepare_scene_f32', 'occ4d_decoder_query_fwd_f32', 'occ4d_squash_f32',
                 'occ4d_grid_points_f32', 'occ4d_split_count_f32', 'occ4d_split_write_f32', 'occ4d_posenc_f32'):
        fn = getattr(lib, name)
        assert fn.argtypes == pk._lib.SIGNATURES[name][1] and fn.restype == pk._lib.SIGNATURES[name][0], name
    assert lib.occ4d_abi_version() == pk._lib.ABI_VERSION


@pytest.mark.parametrize('case', gc.INFER_CASES, ids=lambda c: c['name'])
def test_config1_through_the_product_modules_on_the_twin(twin, case):
    """BASELINE configs[0] (n_points 2048, video_len 4, 8640 grid queries) and the small CARLA case: the product's
    perform_inference on CPU tensors = the reference's run (G10) at 1e-4; FPS subsets bit-exact."""
    g = load_golden('g10_infer_' + case['name'])
    pcl, pa, ia, inf, esd, dsd = gc.infer_inputs(case)
    enc = pk.model.PointCompletionNetV3(**pa).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).eval()
    dec.load_state_dict(dsd)
    lists = (g['knn_local'], g['knn_cross']) if 'knn_local' in g else None      # (CARLA: the reference run's own tie order)
    res = pk.inference.perform_inference(pcl.clone(), None, None, [enc, dec], torch.device('cpu'), 'if', inf['min_z'],
                                         inf['cube_bounds'], inf['color_mode'], case['time_idx'], None,
                                         neighbour_lists=lists, **_kw(case, inf))
    assert np.array_equal(res['pcl_abstract'][:, :3], g['pcl_abstract'][:, :3])
    assert np.abs(res['pcl_abstract'] - g['pcl_abstract']).max() < 1e-4
    assert np.abs(res['features_global'] - g['features_global']).max() < 1e-4
    assert res['implicit_output'].shape == g['implicit_output'].shape
    assert np.abs(res['implicit_output'] - g['implicit_output']).max() < 1e-4
    near = int((np.abs(g['implicit_output'][:, 0] - 0.5) < 1e-4).sum())
    assert abs(res['output_solid'].shape[0] - int(g['n_solid'][0])) <= near
    assert res['output_air'].dtype == np.float64 and res['output_air'].shape[1] == 5


def test_twin_nested_level_rule_for_repeated_picks(twin):
    """The rule the HIP kernel is tested against (tests/test_gpu_fps_pruned.py): distinct positions first, ascending, the
    last one repeated behind them."""
    orig = torch.tensor([2, 5, 7, 11, 13, 20, 21, 40], dtype=torch.int32)
    order = torch.tensor([13, 2, 13, 40, 2, 2, 7, 13], dtype=torch.int32)
    pos, nxt = pk.ops.nested_fps_level(order, orig, 6)
    assert pos.tolist() == [0, 4, 7, 7, 7, 7] and nxt.tolist() == [2, 13, 40, 40, 40, 40]
    pos, nxt = pk.ops.nested_fps_level(order, orig, 8)
    assert pos.tolist() == [0, 2, 4, 7, 7, 7, 7, 7] and nxt.tolist() == [2, 7, 13, 40, 40, 40, 40, 40]
