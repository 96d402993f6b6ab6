/* occ4d_frontend.h -- the per-clip geometry in front of the point cloud: RGB-D frames / lidar sweeps -> cloud rows.
 *
 * A second header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned): the same conventions -- extern "C",
 * int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers,
 * explicit sizes, the stream as void*, no allocation, no hidden synchronisation.  The symbols live in libocc4d.so and in
 * the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * Both entry points are element-wise: one output row and one keep key per input element, in input order.  The rows the
 * reference keeps, in the reference's order, are what occ4d_compact_count_f32 / occ4d_compact_rows_f32 (occ4d.h) select
 * with the key, threshold 0.5, per frame segment.
 *
 * Arithmetic (bit-pinned to the reference's numpy results, tests/golden/frontend_*.npz): every 4 x 4 product is the
 * fused chain fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 * b0))) -- what np.matmul / np.dot of a (4, 4) with a (4, N)
 * float32 operand computes --, every stage rounded on its own; divisions are correctly rounded; comparisons are fp32
 * with inclusive bounds. */
#ifndef OCC4D_FRONTEND_H
#define OCC4D_FRONTEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* point_cloud_from_rgbd (utils/geometry.py:19-64, :118-146) + the instance id from the hue of the "flat" render
 * (data/data_greater.py:394-399) + filter_pcl_bounds_numpy (:149-172) for the T frames of ONE view, one thread per pixel.
 *   depth (T, H, W), rgb (T, H, W, 3), flat (T, H, W, 3) or null (instance id -1), contiguous;
 *   k_inv, rt_inv (T, 4, 4): the host's np.linalg.inv of the 4 x 4 intrinsics / extrinsics (the kernel only multiplies);
 *   hue_clusters (n_clusters <= 64): hue centres in degrees; the id is the first argmin of |round(360 h) - cluster|,
 *     round = half to even, h = matplotlib.colors.rgb_to_hsv's hue; saturation < 0.9 -> -1;
 *   the cuboid, floor_fix != 0: also z > (max(|x|, |y|) - 4.5) / 3.5 (greater_floor_fix);
 *   out_rows (T H W, 8): (x, y, z, instance, R, G, B, t), t = the frame index;
 *   out_target (T H W, 8) or null: (x, y, z, instance, view_idx, R, G, B) (merge_pcl_views_numpy's row, utils/utils.py:64-101);
 *   out_key (T H W): 1 when depth > 0 and the point passes the filter, else 0.
 * Pixels are in frame-major, row-major order: np.where(depth > 0)'s order inside a frame.  T H W < 2^31. */
int occ4d_rgbd_rows_f32(const float* depth, const float* rgb, const float* flat, const float* k_inv, const float* rt_inv,
                        const float* hue_clusters, int n_clusters, int T, int H, int W, float x_min, float x_max,
                        float y_min, float y_max, float z_min, float z_max, int floor_fix, int view_idx, float* out_rows,
                        float* out_target, float* out_key, void* stream);

/* transform_lidar_frame (utils/geometry.py:1286-1306) + the ground offset (data/data_carla.py:461-463) +
 * filter_pcl_bounds_carla_input_numpy (:191-221) for one sweep.
 *   rows (n, d >= 3), row stride ld: xyz first;
 *   source, inv_target (4, 4) or both null (source frame = target frame: no transform): points -> source ->
 *     inv(target), each stage rounded on its own (the matrices are never pre-multiplied); the host inverts.  These two
 *     are HOST pointers, read before the call returns (64 bytes each, passed to the kernel by value);
 *   z_offset: added to z after the transform (0 = none);
 *   cube_mode 1 .. 4: the input cuboid of that mode from min_z / other_bounds (bounds formed in double, compared in
 *     fp32); 0: no filter (every key 1);
 *   out_rows (n, d), row stride ldo >= d: xyz transformed, the other columns copied; out_key (n). */
int occ4d_lidar_rows_f32(const float* rows, int64_t ld, int n, int d, const float* source, const float* inv_target,
                         float z_offset, int cube_mode, double min_z, double other_bounds, float* out_rows, int64_t ldo,
                         float* out_key, void* stream);

#ifdef __cplusplus
}
#endif

#endif
