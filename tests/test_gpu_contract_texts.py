"""libocc4d.so and the g++ twin take the argument contracts of the five feature headers from one source (the check_* functions of
csrc/*_math.hpp over csrc/contract.hpp).  Here both are loaded in one process -- the twin as a second plain handle, never
enabled -- and handed the same rejected calls, device tensors for the one and same-shaped host tensors for the other: the same
status and the same occ4d_last_error() bytes.  The one contract line only libocc4d.so has, the 16-byte alignment of the RGB-D
rows, must differ: the twin accepts that call."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL, OK = pk._lib.EINVAL, pk._lib.OK


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads; host arrays are host in both.
# The flags of the two evaluation calls are OCC4D_EVAL_FLAG_COLOR = 1 and OCC4D_EVAL_FLAG_TRACK = 2.
I32, I64, F64 = torch.int32, torch.int64, torch.float64
HOST_EYE = torch.eye(4)
REJECTED = [
    ('ld = 2 must be >= 3', lambda L, z: L.occ4d_project_points_f32(p(z(10, 6)), 2, 10, p(z(16)), p(z(16)), 1, 0, p(z(30)), None)),
    ('null rows / rt / k', lambda L, z: L.occ4d_project_points_f32(None, 6, 10, p(z(16)), p(z(16)), 1, 0, p(z(30)), None)),
    ('null uvz', lambda L, z: L.occ4d_project_points_f32(p(z(10, 6)), 6, 10, p(z(16)), p(z(16)), 1, 0, None, None)),
    ('n = -1', lambda L, z: L.occ4d_project_points_f32(p(z(10, 6)), 6, -1, p(z(16)), p(z(16)), 1, 0, None, None)),
    ('null keys', lambda L, z: L.occ4d_zbuffer_splat_f32(p(z(10, 6)), 6, 10, p(z(16)), p(z(16)), 1, 4, 4, 0, None, None)),
    ('must be < 2^31', lambda L, z: L.occ4d_zbuffer_splat_f32(p(z(10, 6)), 6, 10, p(z(48)), p(z(48)), 3, 32768, 32768, 0,
                                                              p(z(16, dtype=I64)), None)),
    ('radius = 5', lambda L, z: L.occ4d_zbuffer_splat_f32(p(z(10, 6)), 6, 10, p(z(16)), p(z(16)), 1, 4, 4, 5, p(z(16, dtype=I64)), None)),
    ('null keys', lambda L, z: L.occ4d_zbuffer_resolve_f32(None, 1, 4, 4, p(z(10, 6)), 6, 10, 6, 0.0, p(z(16)), None, None, 0, 0.0, None,
                                                           None)),
    ('need 1 <= d <= ld', lambda L, z: L.occ4d_zbuffer_resolve_f32(p(z(16, dtype=I64)), 1, 4, 4, p(z(10, 6)), 5, 10, 6, 0.0, p(z(16)), None,
                                                                   (ctypes.c_int32 * 1)(0), 1, 0.0, p(z(16)), None)),
    ('column 6', lambda L, z: L.occ4d_zbuffer_resolve_f32(p(z(16, dtype=I64)), 1, 4, 4, p(z(10, 6)), 6, 10, 6, 0.0, p(z(16)), None,
                                                          (ctypes.c_int32 * 2)(0, 6), 2, 0.0, p(z(32)), None)),
    ('ld_depth = 3', lambda L, z: L.occ4d_visibility_f32(p(z(10, 6)), 6, 10, p(z(16)), p(z(16)), 1, p(z(16)), 3, 4, 4, 0.0,
                                                         p(z(10, dtype=I32)), None)),
    ('null depth / code', lambda L, z: L.occ4d_visibility_f32(p(z(10, 6)), 6, 10, p(z(16)), p(z(16)), 1, None, 4, 4, 4, 0.0,
                                                              p(z(10, dtype=I32)), None)),
    ('ld_out = 4', lambda L, z: L.occ4d_track_merge_add_f32(p(z(10, 5)), 4, 10, 5, None, -1, 1.0, 1, p(z(10, 5)), 5, None, None, None)),
    ('null out / acc', lambda L, z: L.occ4d_track_merge_add_f32(None, 5, 10, 5, None, -1, 1.0, 1, p(z(10, 5)), 5, None, None, None)),
    ('first = 2', lambda L, z: L.occ4d_track_merge_add_f32(p(z(10, 5)), 5, 10, 5, None, -1, 1.0, 2, p(z(10, 5)), 5, None, None, None)),
    ('op code 3', lambda L, z: L.occ4d_track_merge_add_f32(p(z(10, 5)), 5, 10, 5, (ctypes.c_int32 * 5)(0, 1, 2, 3, 0), -1, 1.0, 1,
                                                           p(z(10, 5)), 5, None, None, None)),
    ('null best / winner', lambda L, z: L.occ4d_track_merge_add_f32(p(z(10, 5)), 5, 10, 5, None, 4, 1.0, 1, p(z(10, 5)), 5, p(z(10)), None,
                                                                    None)),
    ('ld_acc = 4', lambda L, z: L.occ4d_track_merge_finish_f32(p(z(10, 5)), 4, 10, 5, 2, -1, None, None)),
    ('n_runs = 0', lambda L, z: L.occ4d_track_merge_finish_f32(p(z(10, 5)), 5, 10, 5, 0, 4, p(z(10)), None)),
    ('null winner', lambda L, z: L.occ4d_track_merge_finish_f32(p(z(10, 5)), 5, 10, 5, 2, 4, None, None)),
    ('go together', lambda L, z: L.occ4d_lidar_rows_f32(p(z(4, 4)), 4, 4, 4, p(HOST_EYE), None, 0.0, 0, 0.0, 1.0, p(z(4, 4)), 4, p(z(4)),
                                                        None)),
    ('cube_mode 9', lambda L, z: L.occ4d_lidar_rows_f32(p(z(4, 4)), 4, 4, 4, None, None, 0.0, 9, 0.0, 1.0, p(z(4, 4)), 4, p(z(4)), None)),
    ('n_clusters = 65', lambda L, z: L.occ4d_rgbd_rows_f32(p(z(4)), p(z(12)), p(z(12)), p(z(16)), p(z(16)), p(z(65)), 65, 1, 2, 2, -1.0, 1.0,
                                                           -1.0, 1.0, -1.0, 1.0, 0, 0, p(z(32)), None, p(z(4)), None)),
    ('n_ids = 0', lambda L, z: L.occ4d_id_histogram_f32(p(z(10, 4)), 4, 10, 0, p(z(2, dtype=I64)), 1, 0, None, -1, 0.0, 0.0,
                                                        p(z(6, dtype=I32)), None)),
    ('col = 4', lambda L, z: L.occ4d_id_histogram_f32(p(z(10, 4)), 4, 10, 4, p(z(2, dtype=I64)), 1, 4, None, -1, 0.0, 0.0,
                                                      p(z(6, dtype=I32)), None)),
    ('pred_col = 4', lambda L, z: L.occ4d_id_histogram_f32(p(z(10, 4)), 4, 10, 0, p(z(2, dtype=I64)), 1, 4, None, 4, 1.0, 1.0,
                                                           p(z(6, dtype=I32)), None)),
    ('colour needs', lambda L, z: L.occ4d_eval_query_stats_f32(p(z(5, 5)), 5, 4, 5, p(z(4, dtype=I32)), p(z(4)), p(z(3, 9)), 9, 3, 9, 7, -1,
                                                               -1, 4, None, 1, 0, 0.5, 0.2, 1, p(z(17, dtype=I64)), p(z(8, dtype=F64)),
                                                               p(z(24, dtype=F64)), None)),
    ('tracking needs', lambda L, z: L.occ4d_eval_query_stats_f32(p(z(5, 5)), 5, 4, 5, p(z(4, dtype=I32)), p(z(4)), p(z(3, 9)), 9, 3, 9, -1,
                                                                 8, -1, 5, None, 1, 0, 0.5, 0.2, 2, p(z(17, dtype=I64)), p(z(8, dtype=F64)),
                                                                 p(z(24, dtype=F64)), None)),
    ('n_groups = 9', lambda L, z: L.occ4d_eval_target_stats_f32(p(z(4)), 4, None, 9, 0, p(z(17, dtype=I64)), p(z(8, dtype=F64)),
                                                                p(z(24, dtype=F64)), None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_only_the_hip_library_asks_for_aligned_rgbd_rows(libraries):
    """The call's only fault: out_rows one float off a 16-byte boundary."""
    hip, twin = libraries

    def call(L, z):
        out = z(36)[1:33]
        assert out.data_ptr() % 16 == 4
        return L.occ4d_rgbd_rows_f32(p(z(4)), p(z(12)), None, p(z(16)), p(z(16)), None, 0, 1, 2, 2, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 0, 0,
                                     p(out), None, p(z(4)), None)
    on_device, on_host = zeros_on(DEV), zeros_on('cpu')
    assert call(hip, on_device) == EINVAL and b'16-byte aligned' in hip.occ4d_last_error()
    assert call(twin, on_host) == OK
