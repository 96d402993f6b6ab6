/* occ4d_components.h -- the connected components of the solid set of the query grid, labelled on the device (components.label,
 * inference.perform_inference(components=...)): how many separate objects the decoded occupancy holds, and per object its size,
 * its box and its coordinate sums.  Integers only: the float operations are the >= comparisons of the member test, and the rules
 * below fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_raycast.h and occ4d_prelude.h; it is a row of _lib.ADDON_HEADERS, the table that is open by
 * design (the next header is a row there as well).  The same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL /
 * OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*,
 * no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  The flat one of occ4d_grid_points_f32: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz.
 *     n = nx * ny * nz.  An axis of length 1 is legal.
 *   MEMBER.  member(p) = field[p * ld] >= level: an fp32 comparison, a NaN value or a NaN level is no member (the comparison of the
 *     solid split).  With `mask` not null also mask[p * ld_mask] >= mask_level (the same comparison); with `klass` not null also
 *     klass[p] >= 0.
 *   ADJACENCY.  Two members p, q are adjacent when their coordinates differ by at most 1 on every axis, on at least one axis and on
 *     at most 1 / 2 / 3 axes for connectivity 6 / 18 / 26, and, with `klass` not null, klass[p] == klass[q].
 *   COMPONENT.  An equivalence class of members under the transitive closure of adjacency.  Its ROOT is its lowest flat index, its
 *     SIZE its number of points.
 *   KEPT.  The components with size >= min_size are kept and numbered 0, 1, ... in increasing order of root.
 *   labels (n) int32: the number of the point's component, or -1 for a non-member and for a point of a component that is not kept.
 *   totals int32[3]: kept components, points of kept components, all components (the dropped ones included).
 *   table (cap, OCC4D_COMPONENTS_COLS) int64, row k for the kept component number k, written for 0 <= k < min(cap, totals[0]) and
 *     for no other k: a row outside [0, cap) is never written (the guard of occ4d_surface_write_f32), nor is a row past the last
 *     kept component.  Columns: 0 size; 1 root; 2 the component's class, -1 without `klass`; 3 .. 5 the sums of ix, iy, iz over its
 *     points; 6 .. 8 the minima of ix, iy, iz; 9 .. 11 the maxima.  Sums of integers: any order of addition gives the same bits.
 *
 * WORK.  occ4d_components_label_f32 takes `work`, int32, of
 *         3 * n + 3 * ((n + OCC4D_COMPONENTS_TILE - 1) / OCC4D_COMPONENTS_TILE)
 *   elements (parent, root and size per point; three counts per numbering tile of OCC4D_COMPONENTS_TILE points).  Uninitialised on
 *   entry, garbage on return.
 *
 * LAUNCHES.  Seven for the labels, two for the table, whatever the data: no pass is repeated "until nothing changes", no workgroup
 *   waits for another one.  The device algorithm is label-equivalence union-find (csrc/components.hip): a root is only ever linked
 *   to a lower flat index of its own component, so every parent chain strictly decreases and ends at the component's lowest index.
 *
 * ACCESS SAFETY.  field, mask and klass are read at p in [0, n) only, with p from the thread's own index; a neighbour's index is
 * formed only after its three coordinates have passed 0 <= c < n_a.  parent[], root[] and size[] are indexed by p and by values read
 * from parent[] / root[], which are -1 (tested before use) or flat indices the kernels themselves stored: no value of field, mask,
 * klass, level or min_size reaches an index.  The table kernels index rows by labels[p], which the CALLER provides: every row
 * number is tested 0 <= k < min(cap, totals[0]) before the row is touched, so foreign labels cannot move a write out of the table. */
#ifndef OCC4D_COMPONENTS_H
#define OCC4D_COMPONENTS_H

#include <stdint.h>

#define OCC4D_COMPONENTS_COLS 12           /* columns of the table */
#define OCC4D_COMPONENTS_TILE 256          /* points per numbering tile: the O(n / 256) term of the work array */
#define OCC4D_COMPONENTS_TILE_X 6          /* the tile of the local labelling pass, points per axis (252 points) */
#define OCC4D_COMPONENTS_TILE_Y 7
#define OCC4D_COMPONENTS_TILE_Z 6

#ifdef __cplusplus
extern "C" {
#endif

/* field: one value per grid point, element stride ld >= 1 (a column of the dense array, the pointer already at that column);
 * mask: null, or a second such column with stride ld_mask >= 1;  klass: null, or (n) int32 contiguous.
 * nx, ny, nz >= 0 with nx * ny * nz <= INT32_MAX;  connectivity 6, 18 or 26;  min_size >= 1.
 * work: see WORK;  labels (n) int32;  totals int32[3].
 * n == 0 is a no-op that touches no pointer. */
int occ4d_components_label_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                               const int32_t* klass, int nx, int ny, int nz, int connectivity, int min_size, int32_t* work,
                               int32_t* labels, int32_t* totals, void* stream);

/* labels, klass, totals: what occ4d_components_label_f32 took and wrote for this grid (klass null as there);  table (cap, 12) int64
 * contiguous, cap >= 0.  n == 0 or cap == 0 is a no-op that touches no pointer. */
int occ4d_components_table_i64(const int32_t* labels, const int32_t* klass, int nx, int ny, int nz, const int32_t* totals,
                               int64_t* table, int cap, void* stream);

#ifdef __cplusplus
}
#endif

#endif
