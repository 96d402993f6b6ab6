/* occ4d_project.h -- clouds into camera views, on the device: the projection of pixel_coords_from_point_cloud
 * (utils/geometry.py:67-115), a z-buffer over it and the per-point visibility test against a depth image.
 *
 * A sixth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned), occ4d_frontend.h, occ4d_eval.h,
 * occ4d_occl.h and occ4d_track.h: the same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of
 * occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation,
 * no hidden synchronisation.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * Cameras are V pairs of the reference's EXPANDED matrices, rt (V, 16) and k (V, 16), row-major 4 x 4: eye(4) with the (3, 4)
 * extrinsics in its first three rows / the (3, 3) intrinsics in its upper left corner.  The arithmetic of a row (x, y, z) under
 * one camera is the inverse of occ4d_rgbd_rows_f32's, with the same fused chain
 *     row(a, b) = fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 * b0)))
 *     c_j = row(rt row j, (x, y, z, 1)), j = 0 .. 3;   u' = c0 / c2, v' = c1 / c2 (correctly rounded fp32 divisions);
 *     u = row(k row 0, (u', v', 1, c3)), v = row(k row 1, (u', v', 1, c3)), depth = c2
 * which equals the reference's two np.matmul products bit for bit (tests/golden/project_*.npz).
 *
 * The pixel rule of the z-buffer and of the visibility test: a row TAKES PART in a view when its depth is finite and > 0 and
 * its centre pixel (rintf(u), rintf(v)) -- half to even, as np.round -- lies in [0, W) x [0, H).  The comparisons are made on
 * the floats (a NaN fails them) and only then is a value converted to an integer: no value in any array can move an access
 * outside an image.  The ONE access indexed by data is the feature gather of occ4d_zbuffer_resolve_f32, which is guarded. */
#ifndef OCC4D_PROJECT_H
#define OCC4D_PROJECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* uvz[v][i] = (u, v, depth) of row i under camera v; flip_xy != 0: (v, u, depth).
 *   rows (n, >= 3), row stride ld >= 3: xyz first, read only;  rt, k (V, 16);  uvz (V, n, 3), contiguous.
 * No filtering: points behind the camera, NaN and inf pass through as numpy passes them.  n = 0 or V = 0 is a no-op. */
int occ4d_project_points_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int flip_xy,
                             float* uvz, void* stream);

/* The z-buffer, pass one: every row that takes part in view v writes
 *     key = (uint64)bits(depth) << 32 | i
 * with a 64-bit unsigned atomic MIN into the (2 radius + 1)^2 square of pixels around its centre pixel, clipped to the image
 * (the centre itself must lie inside).  Positive finite floats order as their bit patterns: the nearest row wins a pixel, among
 * exactly equal depths the lowest row index; the result does not depend on scheduling.
 *   keys (V, H, W), contiguous: the CALLER fills it with all-ones (= empty) before the first splat; several splats of the SAME
 *     rows array may share it.  0 <= radius <= 4;  1 <= H, W <= 32768;  V H W < 2^31.
 * n = 0 or V = 0 is a no-op. */
int occ4d_zbuffer_splat_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int H, int W,
                            int radius, unsigned long long* keys, void* stream);

/* The z-buffer, pass two: key image -> images.  A pixel whose key is all-ones, or whose index (the key's low word) is >= n, is
 * BACKGROUND: depth_background / -1 / feat_background.  Every other pixel gets
 *     depth[p] = the float of the key's high word;  index[p] = the key's low word;
 *     feat[p][c] = rows[index][cols_host[c]], c = 0 .. C - 1  -- the only access indexed by data, reached only with index < n.
 *   depth (V, H, W) float or null, index (V, H, W) int32 or null, feat (V, H, W, C) or null (only with C = 0), all contiguous;
 *   rows (n, d), row stride ld >= d: needed for C > 0 only (null otherwise);  cols_host: C column numbers in [0, d) on the HOST,
 *   read before the call returns;  0 <= C <= 32.
 * V = 0 is a no-op. */
int occ4d_zbuffer_resolve_f32(const unsigned long long* keys, int V, int H, int W, const float* rows, int64_t ld, int n, int d,
                              float depth_background, float* depth, int32_t* index, const int32_t* cols_host, int C,
                              float feat_background, float* feat, void* stream);

/* code[v][i] of row i against the depth image of view v, projection and test fused (uvz is never stored):
 *     2 = outside:  the row does not take part in the view (depth not finite or <= 0, or centre pixel off the image);
 *     1 = occluded: the image holds a valid depth d > 0 at the centre pixel and depth - d > margin (fp32 subtraction, fp32
 *                   comparison);
 *     0 = visible:  everything else -- a pixel without a valid depth hides nothing.
 *   depth (V, H, W), image-row stride ld_depth >= W (view stride H ld_depth), read only;  code (V, n) int32, contiguous.
 * n = 0 or V = 0 is a no-op. */
int occ4d_visibility_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* depth,
                         int64_t ld_depth, int H, int W, float margin, int32_t* code, void* stream);

#ifdef __cplusplus
}
#endif

#endif
