/* occ4d_distance.h -- the exact Euclidean distance transform of the solid set of the query grid, on the device (distance.transform,
 * inference.perform_inference(clearance=...)): per grid point the squared distance to the nearest predicted solid -- or, with
 * target 1, to the nearest free point: its depth inside the solid -- and which point that is.  Integers only: the float operations
 * are the >= comparisons of the member test, and the rules below fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_components.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and
 * strides, the stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbol lives in libocc4d.so and in
 * the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_components.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal.  Every axis is <= OCC4D_DISTANCE_MAX_AXIS.
 *   MEMBER.  The member test of occ4d_components.h: member(p) = field[p * ld] >= level, an fp32 comparison, a NaN value or a NaN
 *     level is no member; with `mask` not null also mask[p * ld_mask] >= mask_level (the same comparison).
 *   SITE.  target 0: the members are the sites;  target 1: the non-members are.  (A point's distance to the nearest non-member is
 *     its depth inside the solid.)
 *   COST.  For the integer weights wx, wy, wz >= 1:  cost(p, q) = wx * (ix - jx)^2 + wy * (iy - jy)^2 + wz * (iz - jz)^2.  The call is
 *     rejected unless wx * (nx - 1)^2 + wy * (ny - 1)^2 + wz * (nz - 1)^2 <= INT32_MAX - 1, tested in 64 bits at entry: every sum a
 *     kernel forms is the cost between two grid points or a term of one, so int32 never overflows.
 *   dist2 (n) int32:  dist2[p] = the minimum of cost(p, q) over the sites q, OCC4D_DISTANCE_NONE where there is no site.  A minimum
 *     of integers: the same bits under any scheduling.
 *   nearest (n) int32, or null (not computed):  the flat index of a site with cost(p, nearest[p]) == dist2[p], -1 where there is no
 *     site.  WHICH of several is fixed by the stages a separable algorithm goes through:
 *       STAGE Z.  Per point, the site of its own z-line with the least wz * dz^2; of two, the one at the lower iz.  c1 = that cost.
 *       STAGE Y.  Per point (ix, iy, iz): among the stage-Z results of the points (ix, j, iz) of its y-line that have a site, the
 *         one with the least c1 + wy * (j - iy)^2; of two, the one at the lower j.  The point's site is that entry's site.
 *       STAGE X.  The same over the stage-Y results (j, iy, iz) of its x-line, with wx; of two, the lower j.
 *     The stage-X cost is dist2[p] (the minimum over x of the minimum over y of the minimum over z).
 *
 * LAUNCHES.  Three, whatever the data, one per stage (csrc/distance.hip): a workgroup stages whole lines in LDS, takes each point's
 *   minimum over the candidates of its line and writes the result in place into dist2 / nearest.  No work array, no atomics, no
 *   workgroup waits for another one.
 *
 * ACCESS SAFETY.  field and mask are read at p in [0, n) only, with p from the thread's own index.  Every other index -- into
 * dist2, nearest and the LDS tile -- is made of axis indices that a loop bound produced.  No value of field, mask, level, a weight,
 * or a site stored in nearest reaches an address. */
#ifndef OCC4D_DISTANCE_H
#define OCC4D_DISTANCE_H

#include <stdint.h>

#define OCC4D_DISTANCE_NONE 2147483647     /* dist2 where there is no site: INT32_MAX */
#define OCC4D_DISTANCE_MAX_AXIS 512        /* the longest axis */
#define OCC4D_DISTANCE_TILE_POINTS 4096    /* points of a workgroup's tile of lines: two int32 each, 32 KiB of LDS */
#define OCC4D_DISTANCE_TILE_WIDTH 16       /* lines of a tile of the y and x stages: halved until length * width <= TILE_POINTS */
#define OCC4D_DISTANCE_RUN_POINTS 1024     /* points of a tile of the z stage: max(1, RUN_POINTS / nz) consecutive lines */

#ifdef __cplusplus
extern "C" {
#endif

/* field: one value per grid point, element stride ld >= 1 (a column of the dense array, the pointer already at that column);
 * mask: null, or a second such column with stride ld_mask >= 1;  target 0 or 1;  0 <= nx, ny, nz <= OCC4D_DISTANCE_MAX_AXIS;
 * wx, wy, wz >= 1 within the bound of COST;  dist2 (n) int32;  nearest (n) int32 or null.
 * n == 0 is a no-op that touches no pointer. */
int occ4d_distance_grid_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                            int target, int nx, int ny, int nz, int wx, int wy, int wz,
                            int32_t* dist2, int32_t* nearest, void* stream);

#ifdef __cplusplus
}
#endif

#endif
