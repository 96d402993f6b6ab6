/* occ4d_raycast.h -- the decoded occupancy field ray-cast into camera views, on the device (projection.render_field,
 * inference.perform_inference(views=...)): per pixel the first crossing of field == level along the pixel's ray, with columns of
 * the dense (N, G) array sampled there.  No atomics, one owner per output element, and the orders below fix every output bit.
 *
 * A tenth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned) and the eight feature headers of include/, whose
 * list is closed; this one is the first of include/ext/ (_lib.EXTENSION_HEADERS; include it as "ext/occ4d_raycast.h").  The same
 * conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation, nothing read back.  The symbol lives in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers,
 * synchronous).
 *
 * THE RULES.  All arithmetic is fp32.  row(a, b) = fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 * b0))) is the fused chain of
 * occ4d_frontend.h / occ4d_project.h; it is used for the ray's two end points and NOWHERE else: every other expression below is
 * evaluated as written, each operation rounded on its own (the builds have -ffp-contract=off).
 *   GRID.  The flat one of occ4d_grid_points_f32: (nx, ny, nz) points, x slowest, z fastest, flat index (ix * ny + iy) * nz + iz.
 *     Point i of axis a lies at ((float)i + 0.5f) * spacing_a + origin_a.  f(p) = field[p * ld].
 *   CAMERAS.  V pairs k_inv, rt_inv (V, 16), row-major 4 x 4: the INVERSES of the expanded matrices, exactly what
 *     occ4d_rgbd_rows_f32 takes.  The kernel only multiplies.
 *   RAY of pixel (px, py) (column, row; as floats) of view v.  For a depth d:
 *       q = (px * d, py * d, d, 1);   s_j = row(k_inv row j, q), j = 0 .. 3;   P(d)_a = row(rt_inv row a, s), a = 0, 1, 2.
 *     P0 = P(0.0f), P1 = P(1.0f), dir_a = P1_a - P0_a.
 *   SAMPLES i = 0 .. n_steps - 1:   d_i = near + (float)i * step;   p_a = P0_a + d_i * dir_a.
 *   GRID COORDINATE per axis:   g_a = (p_a - origin_a) / spacing_a - 0.5f   (a correctly rounded division).
 *     A sample is IN the grid when 0.0f <= g_a && g_a <= (float)(n_a - 1) on all three axes: float comparisons, a NaN fails.
 *     Only then c_a = min((int)floorf(g_a), n_a - 2) and w_a = g_a - (float)c_a.
 *   VALUE of a sample in the grid: trilinear over the eight corners of cell (cx, cy, cz), lerp(a, b, w) = a + w * (b - a),
 *     along z first (four lerps with wz, in the order (x, y) = (0,0), (0,1), (1,0), (1,1)), then y (two with wy), then x.
 *   HIT.  The first i whose sample is in the grid with value >= level (a NaN value is no hit: the comparison of the solid split).
 *     If i >= 1 and sample i - 1 is in the grid with a value v0 < level (a NaN v0 fails), with v1 the value of sample i:
 *         t = (level - v0) / (v1 - v0);  if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;       (the fallback of occ4d_surface.h)
 *         depth = d_{i-1} + t * (d_i - d_{i-1})
 *     otherwise depth = d_i.
 *   HIT POSITION.  h_a = P0_a + depth * dir_a, its grid coordinate g_a as above, then CLAMPED:
 *         g_a = fminf(fmaxf(g_a, 0.0f), (float)(n_a - 1))
 *     before c_a and w_a are taken as above: only rounding can have moved the position out, and a NaN lands on 0.
 *   OUTPUTS, each may be null:
 *     depth (V, H, W): the hit's depth, or depth_background where the ray has no hit;
 *     cell (V, H, W) int32: (cx * ny + cy) * nz + cz of the hit position's cell (its low corner's flat index), or -1;
 *     feat (V, H, W, C): for each of the C columns cols_host[c] of attrs (n, d) the trilinear value (the same order) at the hit
 *       position, or feat_background.
 *
 * ACCESS SAFETY.  The only accesses indexed by data are the corner reads of `field` and `attrs`.  Every cell index is converted
 * to an integer from a float that has just passed 0 <= g <= n - 1 (the samples) or been clamped to that range (the hit
 * position), and is then limited to n - 2, so c and c + 1 are grid points: no value in any array, matrix or scalar argument can
 * move an access outside field[0 .. (n - 1) * ld] / attrs' n rows.  Columns are checked on the host. */
#ifndef OCC4D_RAYCAST_H
#define OCC4D_RAYCAST_H

#include <stdint.h>

#define OCC4D_RAYCAST_MAX_STEPS 65536      /* the most samples per ray */
#define OCC4D_RAYCAST_MAX_CHANNELS 32      /* the most columns sampled at the hit */

#ifdef __cplusplus
extern "C" {
#endif

/* field: one value per grid point, element stride ld >= 1 (a column of the dense array, the pointer already at that column);
 *   nx, ny, nz >= 2 with nx * ny * nz <= INT32_MAX;  x0, sx, y0, sy, z0, sz: origin and spacing per axis, the floats of
 *   occ4d_grid_points_f32;  level: a NaN level hits nothing.
 * k_inv, rt_inv (V, 16);  V >= 0;  1 <= H, W <= 32768 (or H * W == 0: a no-op);  V * H * W < 2^31.
 * near finite, step finite and > 0, 1 <= n_steps <= OCC4D_RAYCAST_MAX_STEPS.
 * attrs (n, d), row stride ld_attr >= d, and cols_host: C column numbers in [0, d) on the HOST, read before the call returns;
 *   0 <= C <= OCC4D_RAYCAST_MAX_CHANNELS; with C == 0 attrs, cols_host and feat are not looked at (they may be null).
 * depth, cell, feat: contiguous, each may be null (feat only matters with C > 0).
 * V == 0 or H * W == 0 is a no-op that touches no pointer.  One launch. */
int occ4d_raycast_grid_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                           float sz, float level, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth,
                           float step, int n_steps, const float* attrs, int64_t ld_attr, int d, const int32_t* cols_host, int C,
                           float depth_background, float feat_background, float* depth, int32_t* cell, float* feat, void* stream);

#ifdef __cplusplus
}
#endif

#endif
