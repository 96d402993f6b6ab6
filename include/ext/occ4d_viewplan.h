/* occ4d_viewplan.h -- the next best view over the query grid, on the device (sight.plan, inference.perform_inference(next_view=...)):
 * for C candidate viewpoints, which of the TARGET points -- the part of the predicted scene no sensor sees yet -- each of them would
 * see, and a greedy choice of up to k candidates that together see the most.  Integers only, no floats anywhere: the rules below
 * fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_sight.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the
 * stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_sight.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal.  Every axis is <= OCC4D_SIGHT_MAX_AXIS.
 *   BITS.  The layout of occ4d_sight.h: an array of W = ceil(n / 32) uint32 words, bit p % 32 of word p / 32 is point p; the unused
 *     bits of the last word are 0.  `solid` is the array occ4d_sight_bits_f32 makes.  `targets` is a second array of that layout: the
 *     points that count.  It is any such array, however it was made (occ4d_pull_bits_i32 over `seen` with min_clear = 1 gives the
 *     points no sensor sees; word operations may AND it with `solid` or any mask).
 *   CANDIDATES.  C lattice points c = (cx, cy, cz), (C, 3) int32 ON THE DEVICE, 1 <= C <= OCC4D_VIEWPLAN_MAX_CANDIDATES and
 *     C * W < 2^31.  They may lie outside the grid.  A candidate is DEAD when a coordinate lies outside [-OCC4D_SIGHT_MAX_COORD,
 *     OCC4D_SIGHT_MAX_COORD], or when it stands in a solid cell of the grid (a sensor cannot stand inside an object).
 *     A DEAD CANDIDATE SEES NOTHING.  The values are device data: the kernel makes the range test, before any coordinate is used.
 *   RANGE.  (wx, wy, wz): integer weights in [1, OCC4D_VIEWPLAN_MAX_WEIGHT]; max_dist2: int64, negative = no limit.  A point p is IN
 *     RANGE of c when  wx * dx^2 + wy * dy^2 + wz * dz^2 <= max_dist2  with d = c - p, in 64-bit integers (every term is below 2^51).
 *     The units are those of dist2 in occ4d_distance.h.
 *   VIS.  vis (C, W) uint32: bit p of row c is set iff all four hold:
 *       targets(p);
 *       c is not DEAD;
 *       p is in range of c;
 *       walk(q = p, o = c) == -1: THE WALK of occ4d_sight.h, word for word, from the query p to the origin c over `solid`.  p itself
 *       and c itself are never tested, the cells outside the grid are free, the SQUEEZE is included.
 *     Every word has one owner, there are no atomics.  The unused bits of a row's last word are 0 (even where those of `targets`
 *     are not).
 *   GREEDY.  From vis, targets and k in [0, OCC4D_VIEWPLAN_MAX_PICKS]:  remaining = targets.  In round r = 0 .. k - 1:
 *       count[c] = sum over w of popcount(vis[c, w] & remaining[w]);
 *       best = THE LOWEST c that attains the largest count;
 *       if that count is 0:  picks[r] = -1, pick_gain[r] = 0, and the same for every later round;
 *       otherwise  picks[r] = best, pick_gain[r] = count[best], remaining &= ~vis[best].
 *     gain (C) int32 = the count of round 0: each candidate's score on its own; written for k = 0 too.
 *     status (2) int32 = [popcount(targets), popcount(remaining after the last round)].
 *     It follows that no candidate is picked twice, that pick_gain never increases and that status[0] - status[1] is the sum of
 *     pick_gain.  ONE GREEDY PASS: the k picks are not the best set of k candidates, which is a covering problem; the greedy set
 *     reveals at least 1 - 1/e of what the best one does.
 *
 * LAUNCHES.  A fixed number, whatever the data (csrc/viewplan.hip).
 *   occ4d_viewplan_visible_u32: ONE.  A wave owns 64 consecutive flat indices -- two words of a row -- and OCC4D_VIEWPLAN_CHUNK
 *     consecutive candidates, which it takes one after the other: a ballot per candidate, stored by lanes 0 and 32.  A wave whose two
 *     words of `targets` are 0 stores zeros and walks nothing; a lane without a target bit, or out of range, votes 0 without walking.
 *     `solid` is read where it is, in global memory.
 *   occ4d_viewplan_greedy_u32: 1 + 2 * max(k, 1).  One launch copies targets to `remaining` and clears the counts and sets the
 *     flag word; then per round one launch counts -- a workgroup takes OCC4D_VIEWPLAN_SLICE words of one row, reduces its popcounts
 *     over the wave and through LDS and adds them to count[c] with one integer atomic add, whose order cannot matter -- and one
 *     launch of ONE workgroup picks: the largest (count, lowest c) key over the candidates, `remaining` updated and counted, the
 *     counts cleared for the next round.  Round 0 also counts `remaining` itself (status[0]) and writes gain; with k = 0 it does only
 *     that.  Behind a -1 pick the flag word is 0 and both launches of every later round return at once.
 *   No workgroup waits for another one.  Every loop is a `for` whose bound is fixed before it starts.  Barriers stand in uniform
 *   control flow only.
 *   work: the caller's int32 array of W + C + 2 elements: remaining (W), count (C + 1: the last one counts `remaining` itself), the
 *   flag word.
 *
 * ACCESS SAFETY.  No value read from memory reaches an address without a range test.  targets, vis and remaining are indexed by the
 * thread's own word, tested against W, and by the launch's own candidate, below C.  A candidate's coordinates are range-tested in
 * the kernel and only then become cell coordinates, which pass the grid test of solid_at (csrc/sight_math.hpp) before a word of
 * `solid` is read: its index is < ceil(n / 32).  A pick is tested against [0, C) before it indexes vis.  No value of vis, targets
 * or solid is ever an index. */
#ifndef OCC4D_VIEWPLAN_H
#define OCC4D_VIEWPLAN_H

#include <stdint.h>

#include "occ4d_sight.h"                   /* OCC4D_SIGHT_MAX_AXIS, OCC4D_SIGHT_MAX_COORD */

#define OCC4D_VIEWPLAN_MAX_CANDIDATES 4096 /* C */
#define OCC4D_VIEWPLAN_MAX_PICKS 32        /* k */
#define OCC4D_VIEWPLAN_MAX_WEIGHT 1024     /* wx, wy, wz */
#define OCC4D_VIEWPLAN_CHUNK 8             /* the consecutive candidates one wave takes */
#define OCC4D_VIEWPLAN_SLICE 4096          /* the words of a row one counting workgroup takes */

#ifdef __cplusplus
extern "C" {
#endif

/* solid, targets: (ceil(n / 32)) uint32 for n = nx * ny * nz;  0 <= nx, ny, nz <= OCC4D_SIGHT_MAX_AXIS;  candidates (C, 3) int32, any
 * values;  0 <= C <= OCC4D_VIEWPLAN_MAX_CANDIDATES;  wx, wy, wz in [1, OCC4D_VIEWPLAN_MAX_WEIGHT];  max_dist2 < 0: no limit;
 * vis (C, ceil(n / 32)) uint32.  n == 0 or C == 0 is a no-op that touches no pointer. */
int occ4d_viewplan_visible_u32(const uint32_t* solid, int nx, int ny, int nz, const uint32_t* targets,
                               const int32_t* candidates, int C, int wx, int wy, int wz, int64_t max_dist2,
                               uint32_t* vis, void* stream);

/* vis (C, W) uint32, targets (W) uint32 as above;  0 <= C <= OCC4D_VIEWPLAN_MAX_CANDIDATES, W >= 0, C * W < 2^31;  0 <= k <=
 * OCC4D_VIEWPLAN_MAX_PICKS;  work (W + C + 2) int32;  gain (C) int32;  picks, pick_gain (k) int32, null with k == 0;  status (2)
 * int32.  W == 0 or C == 0 is a no-op that touches no pointer. */
int occ4d_viewplan_greedy_u32(const uint32_t* vis, int C, int64_t W, const uint32_t* targets, int k, int32_t* work,
                              int32_t* gain, int32_t* picks, int32_t* pick_gain, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif
