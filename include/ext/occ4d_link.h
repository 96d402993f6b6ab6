/* occ4d_link.h -- the components of two output frames linked on the device (components.Tracker, inference.perform_inference(
 * components=..., tracker=...)): which component of frame t + 1 continues which component of frame t.  Two label volumes of
 * occ4d_components.h on the same grid are intersected into a sparse table of (a, b) overlaps, the overlaps are compared by their
 * intersection over union in exact integers, and track ids are handed from frame to frame.  Integers only: the rules below fix
 * every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_components.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the
 * stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++
 * twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES OF THE OVERLAP (occ4d_link_overlap_i32).
 *   MEMBER.  Point p of the n points counts when 0 <= labels_a[p] < k_a and 0 <= labels_b[p] < k_b.  Every other value, the usual
 *     -1 included, is no member.
 *   PAIR.  A distinct (a, b) = (labels_a[p], labels_b[p]) of at least one member point.  Its COUNT is the number of its member
 *     points, its ROOT their lowest flat index.  A point has one pair, so roots are distinct.
 *   Pairs are numbered 0, 1, ... in increasing order of root (the convention of the components).
 *   pairs (cap, OCC4D_LINK_PAIR_COLS) int64: row i = a, b, count, root of pair i, written for 0 <= i < min(cap, totals[0]) and for
 *     no other row.
 *   totals int32[3]: [0] the number of distinct pairs, which may exceed cap; [1] the number of member points; [2] 1 when the
 *     work table could not hold the pairs, else 0.  When [2] is 1 the other outputs are unspecified (every access stayed in
 *     bounds).  The table holds `slots` pairs (WORK): [2] is 0 exactly when the number of pairs is <= slots, and then [0] is the
 *     true number of pairs -- also for cap < pairs <= slots.  slots >= cap, so [2] cannot be 1 when the number of pairs is <= cap.
 *   n == 0, k_a == 0 or k_b == 0: no pairs.  The label pointers may be null then; with n > 0 totals is still written (0, 0, 0).
 *
 * WORK.  occ4d_link_overlap_i32 takes `work`, int32, 8-byte aligned, of
 *         4 * slots + n + 2 * ((n + OCC4D_LINK_TILE - 1) / OCC4D_LINK_TILE)
 *   elements, where slots is the smallest power of two >= max(2 * min(cap, n), OCC4D_LINK_MIN_SLOTS), and 2^31 where that would be
 *   more (an open-addressing table of 64-bit keys with a count and a root per slot; the slot of the pair rooted at each point; two
 *   counts per numbering tile of OCC4D_LINK_TILE points).  A point has one pair, so there are never more than n pairs.
 *   Uninitialised on entry, garbage on return.  n == 0 needs no work array.
 *
 * THE RULES OF THE MATCH (occ4d_link_match_i32), over the rows 0 <= i < min(cap, totals[0]) of `pairs` with 0 <= a < k_a and
 * 0 <= b < k_b (any other row is ignored; with totals[2] != 0 no row is read).
 *   UNION.  union = size_a[a] + size_b[b] - count, the sizes from column 0 of the two component tables.
 *   BEATS.  For a fixed b, candidate i beats candidate j when count_i * union_j > count_j * union_i; when the two products are
 *     equal the lower a wins.  The products are unsigned 64-bit: with count < 2^31 and union < 2^32 they are exact.  For a fixed a
 *     it is the same with the lower b winning a tie.  best(b) / best(a) is the pair that beats all others, if there is any.
 *   LINKED.  b continues a when best(b) and best(a) are the same pair and count * iou_den >= iou_num * union, with
 *     0 <= iou_num <= iou_den and 1 <= iou_den <= OCC4D_LINK_MAX_DEN.
 *   link (k_b, 4) int32, row b: the track id; the linked a or -1; the a of best(b) or -1, linked or not; that pair's count or 0.
 *   best_a (k_a, 2) int32, row a: the b of best(a) or -1; that pair's count or 0.
 *   The track id of a linked b is track_a[a]; that of an unlinked b is next_in[0] + the number of unlinked b' < b;
 *   next_out[0] = next_in[0] + the number of unlinked b.  (next_in and next_out may be the same address.)
 *   k_a == 0: every b is new, in order.  k_b == 0: link is not touched, next_out[0] = next_in[0].
 *   Sizes are caller data: for 0 <= count <= size < 2^31 the result is as above; for anything else the VALUES are unspecified.
 *
 * LAUNCHES.  Six for the overlap (clear, insert, mark, count, scan, number), five for the match (init, best, resolve, finish,
 *   rank), whatever the data.  No workgroup waits for another one: every probe sequence and every compare-and-swap loop is a `for`
 *   with a bound fixed before it starts.
 *
 * ACCESS SAFETY.  The labels are read at p in [0, n) only, p from the thread's own index, and tested 0 <= label < k before they
 * become part of a key; a key is hashed into [0, slots) with a mask and indexes nothing else.  A slot's root is a flat index the
 * kernels themselves stored and is tested 0 <= root < n before it indexes.  A row of `pairs` is written only for i < min(cap,
 * totals[0]).  The match takes a and b out of `pairs`, which the CALLER provides: both are tested 0 <= a < k_a, 0 <= b < k_b before
 * a row of a table, of track_a, of link or of best_a is touched; a stored pair index is tested against min(cap, totals[0]) before
 * it is followed.  No size, count, track id or threshold ever reaches an index. */
#ifndef OCC4D_LINK_H
#define OCC4D_LINK_H

#include <stdint.h>

#define OCC4D_LINK_PAIR_COLS 4             /* columns of a pair row: a, b, count, root */
#define OCC4D_LINK_TILE 256                /* points per numbering tile: the O(n / 256) term of the work array */
#define OCC4D_LINK_MIN_SLOTS 64            /* the smallest work table */
#define OCC4D_LINK_MAX_DEN 1048576         /* the largest iou_den: 2^20 */

#ifdef __cplusplus
extern "C" {
#endif

/* labels_a, labels_b (n) int32 contiguous, the same grid;  k_a, k_b >= 0;  0 <= n <= INT32_MAX;  work: see WORK;
 * pairs (cap, 4) int64 contiguous, cap >= 0 (null with cap == 0);  totals int32[3].  n == 0 is a no-op that touches no pointer. */
int occ4d_link_overlap_i32(const int32_t* labels_a, const int32_t* labels_b, int k_a, int k_b, int64_t n, int32_t* work,
                           int64_t* pairs, int cap, int32_t* totals, void* stream);

/* pairs, totals, cap: what occ4d_link_overlap_i32 took and wrote;  table_a (k_a rows), table_b (k_b rows) int64 with row strides
 * ld_a, ld_b >= 1 elements, read at column 0;  track_a (k_a) int32;  next_in, next_out int32[1];  link (k_b, 4), best_a (k_a, 2)
 * int32 contiguous.  pairs, totals, the tables and track_a may be null when k_a == 0, k_b == 0 or cap == 0;  link with k_b == 0;
 * best_a with k_a == 0. */
int occ4d_link_match_i32(const int64_t* pairs, const int32_t* totals, int cap, const int64_t* table_a, int64_t ld_a,
                         const int64_t* table_b, int64_t ld_b, int k_a, int k_b, const int32_t* track_a, int iou_num, int iou_den,
                         const int32_t* next_in, int32_t* link, int32_t* best_a, int32_t* next_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
