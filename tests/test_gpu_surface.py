"""The occupancy surface as a quad mesh on the HIP path (csrc/surface.hip): the case matrix, the guard, the mesh properties and
the end-to-end comparisons of tests/test_surface_host.py on the device (the kernels and the g++ twin share their per-element
source), and results that do not depend on the stream or the run.  Everything but the properties EQUAL.

If a mesh ever differs from the restatement end to end, compare result['implicit_output'] with the call without `surface` first:
the two entry points are pinned by the matrix."""
import ctypes

import numpy as np
import pytest
import torch

import refine_cases as rc
import surface_cases as sc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_hip_library_exports_the_symbols():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.SURFACE_SIGNATURES:
        assert hasattr(handle, name), name
    assert sorted(pk._lib.SURFACE_SIGNATURES) == ['occ4d_surface_count_f32', 'occ4d_surface_write_f32']
    assert pk._lib.FEATURE_HEADERS['SURFACE'] == 'occ4d_surface.h'


@pytest.mark.parametrize('counts', sc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(counts):
    assert sc.check_matrix(counts, DEV) == sc.cells_of()


def test_entry_points_on_more_than_1024_tiles():
    sc.check_large(DEV)


def test_one_inside_point():
    sc.check_one_inside_point(DEV)


def test_guard():
    sc.check_guard(DEV)


def test_sphere_is_closed_oriented_and_of_genus_0():
    sc.check_sphere(DEV)


def test_plane_at_the_exact_crossing():
    sc.check_plane(DEV)


def test_argument_errors():
    sc.check_argument_errors(DEV)


def test_does_not_depend_on_the_stream_or_the_run():
    """Two calls on each of three streams: equal bits (no atomics, every element has one owner)."""
    counts, n_attr = sc.LARGE_GRID, 5
    n = 65 ** 3
    rng = np.random.default_rng(29)
    dens, attrs = sc.densities('pool', n, rng), sc.attributes(n, n_attr, rng)
    want = sc.restate(dens, counts, sc.LEVEL, sc.MINS, sc.SPACINGS, attrs)
    dens_t, attrs_t = torch.from_numpy(dens).to(DEV), torch.from_numpy(attrs).to(DEV)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    results = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                results.append(pk.ops.surface_nets(dens_t, counts, float(sc.LEVEL), sc.MINS, sc.SPACINGS, attrs=attrs_t))
    torch.cuda.synchronize()
    for v, f in results:
        assert sc.same_mesh(v.cpu().numpy(), f.cpu().numpy(), want)


def test_single_run_equals_the_restatement(shared):
    sc.check_single_run(shared)


def test_under_refine_the_mesh_is_that_of_the_expanded_array(shared):
    sc.check_refine(shared)


def test_track_mode_all_meshes_the_merged_array(shared):
    sc.check_track_all(shared)


def test_evaluate_clip_passes_surface_through(shared):
    sc.check_clip(shared)


def test_surface_none_is_untouched(shared, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    sc.check_value_errors(shared)
