/* occ4d_sweep.h -- the decoded occupancy field scanned by a virtual lidar, on the device (sweep.py, ops.sweep_rays,
 * inference.perform_inference(sweep=...)): an arbitrary bundle of rays -- per view a sensor pose and a table of directions --
 * marched through the dense (N, G) array; per ray the range of the first crossing of field == level, the cosine of the incidence
 * angle there, the grid point on the solid side of the crossing with its class and object, and columns of the array sampled at
 * the hit.  No atomics, one owner per output element, and the orders below fix every output bit.
 *
 * One more header of include/ext/ (_lib.ADDON_HEADERS, whose list is open; include it as "ext/occ4d_sweep.h") beside occ4d.h,
 * whose symbol set and OCC4D_ABI_VERSION are pinned.  The same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL /
 * OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and strides, the stream as
 * void*, no allocation, no hidden synchronisation, nothing read back.  The symbol lives in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.  All arithmetic is fp32, every expression is evaluated as written, each operation rounded on its own (the builds
 * have -ffp-contract=off); the one fused chain is that of RAYS.
 *   GRID, SAMPLES, IN, VALUE, HIT, HIT POSITION.  Those of ext/occ4d_raycast.h, word for word, with P0 and dir from RAYS below
 *     and `range` for its `depth` (the implementation calls that header's functions: march, sample, grid_coord, in_axis, cell_of,
 *     trilinear, clamped_coord, depth_of).  In short: point i of axis a lies at ((float)i + 0.5f) * spacing_a + origin_a, flat
 *     index (ix * ny + iy) * nz + iz, f(p) = field[p * ld];  samples i = 0 .. n_steps - 1 at d_i = near + (float)i * step,
 *     p_a = P0_a + d_i * dir_a, g_a = (p_a - origin_a) / spacing_a - 0.5f, IN the grid when 0.0f <= g_a && g_a <= (float)(n_a - 1)
 *     on all axes (a NaN fails), then c_a = min((int)floorf(g_a), n_a - 2), w_a = g_a - (float)c_a and the trilinear VALUE (z, then
 *     y, then x);  the HIT is the first i whose sample is in the grid with value >= level (a NaN value, a NaN level: no hit),
 *     refined against sample i - 1 when that is in the grid with a value < level: t = (level - v0) / (v1 - v0), 0.5f unless
 *     0 <= t <= 1, range = d_{i-1} + t * (d_i - d_{i-1}), else range = d_i;  the HIT POSITION h_a = P0_a + range * dir_a, its grid
 *     coordinate CLAMPED to [0, n_a - 1] (a NaN lands on 0) before the cell (cx, cy, cz) and the weights (wx, wy, wz) are taken.
 *     near, step, n_steps and level keep that header's limits.
 *   RAYS.  The rays of view v, 0 <= v < V:  pose (V, 12): row-major [Rm | t] (three rows of four), sensor to the grid's world;
 *     dirs (D, 3): directions in the sensor frame;  R = B * A rays per view.  per_view == 0: D = R, all views share the table, ray
 *     r of every view takes row r.  per_view == 1: D = V * R, ray r of view v takes row v * R + r.  With (d0, d1, d2) that row:
 *         P0_a = t_a = pose[v][4 a + 3];    dir_a = fmaf(Rm_a2, d2, fmaf(Rm_a1, d1, Rm_a0 * d0)),  Rm_aj = pose[v][4 a + j].
 *     Directions are NOT normalised: the parameter d of P0 + d * dir, and so `range`, is in units of |dir| (sweep.py supplies unit
 *     vectors rounded from float64).  A zero or NaN direction is no error: every sample of a zero direction is the origin itself
 *     (a hit at d_0 = near if the origin's sample is solid, else none), a NaN direction has no sample in the grid.
 *   GRADIENT of the trilinear interpolant at the hit position.  f_xyz = f at corner (cx + x, cy + y, cz + z) of the hit cell,
 *     lerp(a, b, w) = a + w * (b - a):
 *         gx = lerp(lerp(f100 - f000, f101 - f001, wz), lerp(f110 - f010, f111 - f011, wz), wy) / spacing_x
 *         gy = lerp(lerp(f010 - f000, f011 - f001, wz), lerp(f110 - f100, f111 - f101, wz), wx) / spacing_y
 *         gz = lerp(lerp(f001 - f000, f011 - f010, wy), lerp(f101 - f100, f111 - f110, wy), wx) / spacing_z
 *   COS.  nd = gx * dir_x + gy * dir_y + gz * dir_z,  nn = gx * gx + gy * gy + gz * gz,  dd = dir_x * dir_x + dir_y * dir_y +
 *     dir_z * dir_z, each summed left to right;  den = sqrtf(nn * dd) (correctly rounded, as the divisions);
 *         cos = den > 0.0f ? fminf(fabsf(nd) / den, 1.0f) : 0.0f
 *     the non-negative cosine of the incidence angle (the cosine_angle column of a lidar row).  A NaN or zero den gives 0; a NaN
 *     quotient under a positive den gives 1 (fminf returns its other operand).
 *   OWNER.  The corner of the hit cell with the greatest field value, the first of them in the order (x, y, z) = (0,0,0), (0,0,1),
 *     (0,1,0), (0,1,1), (1,0,0), ..., (1,1,1):  best = -INFINITY, k = 0;  for each corner j in that order: if (f_j > best)
 *     { best = f_j; k = j; }.  A NaN never wins; all corners NaN (or -INFINITY) give corner 0.  owner = the flat index of corner k.
 *     It is the solid side of the crossing: the grid point nearest to the hit may be an air point, whose colour and class mean
 *     nothing.
 *       sem = the argmax of columns sem_first .. sem_first + n_sem - 1 of attrs at row `owner`: m = column sem_first, sem = 0;
 *         for j = 1 .. n_sem - 1: if (column sem_first + j > m) { m = it; sem = j; }  (the first maximum wins).
 *       inst = labels[owner] if 0 <= labels[owner] < K, else -1.
 *     inst == -1 CAN OCCUR AT A HIT: the refined crossing is rounded, so the cell's greatest corner may lie below the level the
 *     label product cut at; and a label product with min_size or select leaves solid points unlabelled.
 *   OUTPUTS, contiguous, ray index v * R + r, each may be null and only those given are written:
 *     range (V, R): the hit's range, or range_background;
 *     point (V, R, 3): the hit position h -- the very floats the cell is clamped from --, or range_background in all three;
 *     cell (V, R) int32: (cx * ny + cy) * nz + cz of the hit cell (its low corner's flat index), or -1;
 *     owner (V, R) int32: the OWNER's flat index, or -1;
 *     cos (V, R): COS, or 0 with no hit;
 *     sem (V, R) int32: or -1 with no hit; not written with n_sem == 0;
 *     inst (V, R) int32: or -1 with no hit; not written with labels null;
 *     feat (V, R, C): for each of the C columns cols_host[c] of attrs the trilinear value at the hit position (the function and
 *       the order of ext/occ4d_raycast.h's feat), or feat_background; not written with C == 0.
 *
 * ACCESS SAFETY.  The accesses indexed by data are the corner reads of `field` and `attrs` (the samples, the gradient, the owner
 * scan, feat), the row `owner` of attrs (sem) and labels[owner].  Every cell index is converted to an integer from a float that
 * has just passed 0 <= g <= n - 1 (the samples) or been clamped to that range (the hit position), and is then limited to n - 2,
 * so c and c + 1 are grid points and owner is one of them: no value in any array, pose, direction or scalar argument -- a zero,
 * infinite or NaN direction or pose included -- can move an access outside field[0 .. (n - 1) * ld], attrs' n rows or labels' n
 * elements.  pose and dirs are indexed by v and r alone.  A label is compared, never used as an index.  Columns are checked on the
 * host. */
#ifndef OCC4D_SWEEP_H
#define OCC4D_SWEEP_H

#include <stdint.h>

#define OCC4D_SWEEP_MAX_STEPS 65536      /* the most samples per ray (OCC4D_RAYCAST_MAX_STEPS) */
#define OCC4D_SWEEP_MAX_CHANNELS 32      /* the most columns sampled at the hit (OCC4D_RAYCAST_MAX_CHANNELS) */

#ifdef __cplusplus
extern "C" {
#endif

/* field: one value per grid point, element stride ld >= 1 (a column of the dense array, the pointer already at that column);
 *   nx, ny, nz >= 2 with nx * ny * nz <= INT32_MAX;  x0, sx, y0, sy, z0, sz: origin and spacing per axis, the floats of
 *   occ4d_grid_points_f32;  level: a NaN level hits nothing.
 * pose (V, 12), dirs (D, 3) contiguous;  V, B, A >= 0, R = B * A with V * R < 2^31;  per_view 0 or 1.
 * near_range finite, step finite and > 0, 1 <= n_steps <= OCC4D_SWEEP_MAX_STEPS.
 * attrs (n, d), row stride ld_attr >= d: looked at with C > 0 or n_sem > 0 only.  cols_host: C column numbers in [0, d) on the
 *   HOST, read before the call returns; 0 <= C <= OCC4D_SWEEP_MAX_CHANNELS.  n_sem >= 0, and with n_sem > 0: 0 <= sem_first and
 *   sem_first + n_sem <= d.
 * labels (n) int32 contiguous, any values, or null;  K >= 0.
 * range, point, cell, owner, cosine, sem, inst, feat: each may be null.
 * V == 0 or R == 0 is a no-op that touches no pointer.  One launch. */
int occ4d_sweep_rays_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                         float sz, float level, const float* pose, const float* dirs, int V, int B, int A, int per_view,
                         float near_range, float step, int n_steps, const float* attrs, int64_t ld_attr, int d,
                         const int32_t* cols_host, int C, int sem_first, int n_sem, const int32_t* labels, int K,
                         float range_background, float feat_background, float* range, float* point, int32_t* cell, int32_t* owner,
                         float* cosine, int32_t* sem, int32_t* inst, float* feat, void* stream);

#ifdef __cplusplus
}
#endif

#endif
