"""The watershed segments on the HIP path (csrc/watershed.hip): the case matrix of tests/watershed_cases.py through libocc4d.so,
EQUAL to the restatement of the header's rules and to the g++ twin bit for bit (the twin loaded as a second plain handle: the kernels
and the twin share ORDER, the ascent choice, the MERGE test and the item bodies; the kernel stages tiles of 8 x 8 x 8 points in LDS and
runs under any scheduling, the twin goes over the whole grid in order), every call twice with equal bits, one full-size grid against
the twin, and the end-to-end comparisons of tests/test_watershed_host.py on the device.  Integers only, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import refine_cases as rc
import watershed_cases as wc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


@pytest.fixture(scope='module')
def twin_handle():
    handle = pk._lib.bind(ctypes.CDLL(pk.cpu_twin.build()), missing=lambda name: None)      # a second handle: enable() is not called
    assert not pk.cpu_twin.enabled() and handle.occ4d_is_cpu_twin() == 1
    return handle


def test_hip_library_exports_the_symbols():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in wc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['WATERSHED'] == 'ext/occ4d_watershed.h'


@pytest.mark.parametrize('name', wc.NAMES)
def test_case_equals_the_restatement_and_the_twin_twice(twin_handle, name):
    wc.check(name, DEV, twin_handle)


def test_two_touching_balls_flip_where_the_restatement_says(twin_handle):
    wc.check_balls(DEV, twin_handle)


def test_caps_and_untouched_rows(twin_handle):
    wc.check_caps(DEV, pk._lib.lib())
    wc.check_caps('cpu', twin_handle, loaded=False)


def test_full_size_grid_equals_the_twin(twin_handle):
    """96 x 96 x 58, the depth of a thresholded smooth synthetic field (six blobs that touch, as the field of the timings does): the
    kernels against the twin, once -- 2088 numbering tiles, 1152 ascent tiles, 7 jump rounds."""
    counts = (96, 96, 58)
    x, y, z = np.meshgrid(*(np.arange(c, dtype=np.float32) for c in counts), indexing='ij')
    field = np.zeros(counts, np.float32)
    for cx, cy, cz, r in ((30, 30, 20, 14), (48, 34, 24, 12), (62, 50, 30, 15), (40, 62, 36, 11), (70, 70, 22, 13), (24, 70, 40, 10)):
        field += np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / np.float32(r * r))
    values = torch.from_numpy(field.reshape(-1)).to(DEV)
    inside2 = pk.ops.grid_distance(values, counts, 0.5, target=1)[0]
    assert pk.ops.grid_components(values, counts, 0.5, 26)[1].cpu().tolist()[0] < 6              # blobs that touch
    height = inside2.cpu().numpy()
    for h, connectivity in ((0, 26), (8, 6)):
        got = wc.run_ops(DEV, height, counts, connectivity, h)
        assert got['totals'][0] >= 4 and got['totals'][3] >= got['totals'][0] and got['totals'][1] == (height >= 1).sum()
        wc.same(wc.run_raw(twin_handle, 'cpu', height, counts, connectivity, h), got, 'full size h%d' % h)


def test_argument_errors():
    wc.check_argument_errors(DEV)


def test_compositions_with_components_distance_and_tracker():
    wc.check_compositions(DEV)


def test_perform_inference_with_segments(shared):
    wc.check_end_to_end(shared)


def test_evaluate_clip_passes_segments_through(shared):
    wc.check_clip(shared)


def test_segments_none_is_untouched(shared, monkeypatch):
    wc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    wc.check_value_errors(shared)
