/* occ4d_watershed.h -- touching objects of the decoded occupancy split at their necks, on the device (watershed.split,
 * inference.perform_inference(segments=...)): a watershed of an integer height map -- the product feeds inside2, the exact squared
 * depth of every solid query (occ4d_distance.h, target 1) --: one segment per thick part, with the caller's tolerance `h` for how
 * shallow a neck must be.  Integers only: the rules below fix every output bit whatever the scheduling and the tiling.
 *
 * A header of include/ext/, a row of _lib.ADDON_HEADERS.  The conventions of its siblings -- extern "C", int status (OCC4D_OK /
 * OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the stream as
 * void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_components.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal.
 *   HEIGHT.  height (n) int32 contiguous.  member(p) = height[p] >= 1; any other value, negatives included, is no member.
 *   ADJACENCY.  Two members p, q are adjacent when their coordinates differ by at most 1 on every axis, on at least one axis and on
 *     at most 1 / 2 / 3 axes for connectivity 6 / 18 / 26.
 *   ORDER.  q is above p when height[q] > height[p], or when the heights are equal and q < p: a strict total order of the members.
 *   ASCENT.  up(p) is the highest member under ORDER among p and its adjacent members.  A member with up(p) == p is a MAXIMUM.
 *     Following up strictly rises in ORDER and ends at a maximum: basin(p) is the flat index of that maximum, peak(B) = height[B].
 *     Basins are connected.  Plateaus are not special-cased: the index tie-break may cut a plateau into several basins, and MERGE
 *     reunites them for every h >= 0.
 *   MERGE.  Two basins A != B are related when some adjacent pair p in A, q in B has
 *         min(peak(A), peak(B)) - min(height[p], height[q]) <= h,          0 <= h <= INT32_MAX
 *     (the left side is >= 0 and fits int32): the highest saddle between A and B lies within h of the lower peak.  The peaks are
 *     those of the original basins; the relation is not evaluated again after a merge.
 *   SEGMENT.  An equivalence class of basins under the transitive closure of MERGE (the closure of a fixed relation: no order
 *     dependence).  Its ROOT is the lowest flat index of its points, its SIZE its number of points.
 *   KEPT.  The segments with size >= min_size are kept and numbered 0, 1, ... in increasing order of root.
 *   labels (n) int32: the number of the point's segment, or -1 for a non-member and for a point of a segment that is not kept.
 *   totals int32[4]: kept segments, points of kept segments, all segments, basins.  The first three words have the meaning of
 *     occ4d_components_label_f32's totals: the (K, 12) int64 table of the segments is occ4d_components_table_i64(labels, null, nx,
 *     ny, nz, totals, table, cap), unchanged.
 *   peaks (cap, 2) int32: row k holds the flat index and the height of the highest point, under ORDER, of kept segment k.  Rows are
 *     written for 0 <= k < min(cap, totals[0]) and for no other k.  (A row whose label no member of `labels` carries -- foreign
 *     labels only -- reads (-1, 0).)
 *
 * CONSEQUENCES.  With h >= the largest height and min_size 1 the labels are those of occ4d_components_label_f32 for the same member
 *   set and connectivity, numbering included; every segment is connected; the segments at h1 <= h2 nest; no segment spans two
 *   components.
 *
 * WORK.  occ4d_watershed_label_i32 takes `work`, int32, of
 *         4 * n + 4 * ((n + OCC4D_WATERSHED_TILE - 1) / OCC4D_WATERSHED_TILE) + OCC4D_WATERSHED_ROUND_WORDS
 *   elements (basin, parent, low and size per point; four counts per numbering tile; one word per jump round and one in front).
 *   Uninitialised on entry, garbage on return.
 *
 * LAUNCHES.  occ4d_watershed_label_i32: 7 + R with R = ceil(log8 n) <= 11, whatever the data (14 at 96 x 96 x 58):
 *     1 ascent   a workgroup owns a tile of OCC4D_WATERSHED_TILE_X x _Y x _Z points, stages the heights with a halo of one point in
 *                LDS and writes up(p) for its own points;
 *     R jumps    pointer doubling with OCC4D_WATERSHED_HOPS hops a round: up[p] = the pointer followed HOPS times (or to a maximum),
 *                in place, so a pointer's reach grows eightfold a round.  A chain can be O(n) long (a serpentine plateau), R rounds
 *                resolve any; round k returns at once when round k - 1 changed nothing (one word per round in `work`).  Every
 *                stored value is an ancestor of p, so the relaxed loads and stores of one launch may meet in any order;
 *     1 merge    label-equivalence union-find over the maxima (find / unite of csrc/components_math.hpp: a root is only ever linked,
 *                by an atomic minimum, to a lower index), one pass over the forward half of the neighbour offsets, MERGE evaluated
 *                per point pair;
 *     1 flatten  the point's segment representative; its size and its lowest index by integer atomics;
 *     3 count, scan, number   per tile of OCC4D_WATERSHED_TILE points, the scheme of csrc/components.hip;
 *     1 label.
 *   occ4d_watershed_peaks_i32: 3 (clear, one 64-bit atomic maximum per contribution on a packed (height, inverted index) key,
 *   gathered per workgroup and label in LDS first; unpack in place).
 *   Every loop is a `for` with a bound fixed before it starts, or ends because an integer strictly decreases; no workgroup waits for
 *   another one.
 *
 * ACCESS SAFETY.  height is read at flat indices made of coordinates that passed 0 <= c < n_axis, or at basin[] values, which are
 *   -1 (tested before use) or flat indices the kernels themselves stored; so are parent[], low[] and size[].  No height, h or
 *   min_size reaches an index.  The labels given to occ4d_watershed_peaks_i32 are CALLER data: every row number is tested
 *   0 <= k < min(cap, totals[0]) before the row is touched, and a height is used as a value only. */
#ifndef OCC4D_WATERSHED_H
#define OCC4D_WATERSHED_H

#include <stdint.h>

#define OCC4D_WATERSHED_TILE 256           /* points per numbering tile: the O(n / 256) term of the work array */
#define OCC4D_WATERSHED_TILE_X 8           /* the ascent's tile of grid points: one thread per point */
#define OCC4D_WATERSHED_TILE_Y 8
#define OCC4D_WATERSHED_TILE_Z 8
#define OCC4D_WATERSHED_HOPS 8             /* pointers a thread follows in one jump round */
#define OCC4D_WATERSHED_ROUND_WORDS 12     /* words of the jump rounds' flags: R + 1 <= 12 */
#define OCC4D_WATERSHED_TOTALS 4           /* words of totals */

#ifdef __cplusplus
extern "C" {
#endif

/* height (n) int32 contiguous;  nx, ny, nz >= 0 with nx * ny * nz <= INT32_MAX;  connectivity 6, 18 or 26;  h >= 0;  min_size >= 1;
 * work: see WORK;  labels (n) int32;  totals int32[4].
 * n == 0 is a no-op that touches no pointer. */
int occ4d_watershed_label_i32(const int32_t* height, int nx, int ny, int nz, int connectivity, int h, int min_size, int32_t* work,
                              int32_t* labels, int32_t* totals, void* stream);

/* height, labels (n) int32, totals: what occ4d_watershed_label_i32 took and wrote, n >= 0;  peaks (cap, 2) int32 contiguous and
 * aligned to 8 bytes, cap >= 0.  n == 0 or cap == 0 is a no-op that touches no pointer. */
int occ4d_watershed_peaks_i32(const int32_t* height, const int32_t* labels, int n, const int32_t* totals, int32_t* peaks, int cap,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif
