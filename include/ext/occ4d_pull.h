/* occ4d_pull.h -- straight free legs over the query grid, on the device (geodesic.straight, geodesic.pull, inference.perform_inference(
 * route=Route(..., pull=True))): whether the straight segment between two ARBITRARY grid points stays on passable points, over an
 * ARBITRARY blocked set, and the traced paths of occ4d_geodesic.h pulled straight into a few waypoints joined by such segments.
 * Integers only, no floats anywhere: the rules below fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_sight.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the
 * stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_sight.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal.  Every axis is <= OCC4D_SIGHT_MAX_AXIS.
 *   BLOCKED.  blocked(p) = !(clear[p] >= min_clear), an int32 comparison: the complement of PASSABLE in occ4d_geodesic.h.  `clear`
 *     is any (n) int32 array; with dist2 of occ4d_distance.h, min_clear = 1 is "solid" and min_clear = r^2 "no ball of radius r fits".
 *   BITS.  The layout of occ4d_sight.h: `blocked` is an array of ceil(n / 32) uint32 words, bit p % 32 of word p / 32 is blocked(p);
 *     the unused bits of the last word are 0.  occ4d_pull_bits_i32 makes it; the other two entry points read nothing else of `clear`,
 *     and take any such array, however it was made.
 *   FREE(a, b), for flat indices a, b.  It holds iff all three of these hold:
 *       both lie in [0, n);
 *       neither is blocked;
 *       walk(a -> b) over the blocked bits returns -1.
 *     The walk is THE WALK of occ4d_sight.h, word for word, from the query a to the origin b, with "solid" read as "blocked": the
 *     supercover of the segment between the two cell centres in 64-bit integers, the SQUEEZE at edges and corners.  It tests neither
 *     a nor b, which is why the second condition stands beside it.  a == b is free when a is passable.  Both ends lie in the grid,
 *     so every visited cell and every side cell of a SQUEEZE lies in the ends' bounding box: THE "OUTSIDE THE GRID" RULE OF THE WALK
 *     (its step 7) NEVER FIRES HERE.
 *     FREE is symmetric: FREE(a, b) == FREE(b, a).  The walk from b visits the same cells in the opposite order and meets the same
 *     edges and corners with the same side cells.
 *   HIT(a, b) int32.  THE VALUE DEPENDS ON THE DIRECTION a -> b (the first blocker met from a), while FREE does not.  The first
 *     that applies:
 *       -2   when an index is outside [0, n);
 *       a    when a is blocked;
 *       b    when b is blocked;
 *       the walk's blocker -- the flat index of a blocked cell -- when the walk is stopped;
 *       -1   when FREE(a, b).
 *   PULL.  Per goal g the input is the chain p_0 .. p_{L-1}: row g of paths (n_goals, cap) with L = path_len[g], as
 *     occ4d_geodesic_trace_i32 leaves them (goal first, the seed last).
 *       With L <= 0, or L > cap (which the trace never leaves): waypoint_len[g] = path_len[g] and row g of waypoints is all -1.
 *       Otherwise k_0 = 0, and while k_i < L - 1:  k_{i+1} is the largest j in (k_i + 1, L - 1] with FREE(p_{k_i}, p_j); if there is
 *       no such j, k_{i+1} = k_i + 1 -- THE ORIGINAL MOVE IS KEPT UNTESTED.  The fallback is needed: a legal edge or corner move of
 *       occ4d_geodesic.h between two blocked side cells is not FREE under the SQUEEZE.
 *       waypoints[g] holds p_{k_0}, p_{k_1}, .. and -1 behind them; waypoint_len[g] is their number.  The first is the goal, the
 *       last is p_{L-1}, and the waypoints are a subsequence of the chain.
 *     "The largest j" is the rule, not "the j before the first failure": visibility along a chain is not monotone.  A chain value
 *     outside [0, n), or a blocked one, is never FREE with anything: it is reached by the fallback and left by it.
 *     ONE GREEDY PASS FROM THE GOAL.  THE RESULT IS NOT THE EUCLIDEAN SHORTEST PATH, nor the fewest waypoints: every leg is FREE or
 *     one original move, and by the triangle inequality the polyline through the waypoints is no longer than the one through the
 *     chain.  Nothing more is promised.
 *
 * LAUNCHES.  One per entry point, whatever the data (csrc/pull.hip).  occ4d_pull_bits_i32: a wave makes two words with a ballot
 *   each.  occ4d_pull_pairs_u32: one thread per pair, one store per pair.  occ4d_pull_paths_i32: one workgroup of OCC4D_PULL_ROUND
 *   threads per goal; per anchor it scans the candidates j from the far end, OCC4D_PULL_ROUND at a time (thread t of a round tests
 *   j = top - t), reduces the largest free j over the workgroup (a ballot per wave, then one word per wave through LDS) and stops at
 *   the first round with a hit -- the same result as testing every j, with less work.  Thread 0 stores the waypoints.  Every loop is
 *   a `for` whose bound is fixed before it starts: anchors <= cap, rounds <= ceil(cap / OCC4D_PULL_ROUND), the walk's nx + ny + nz.
 *   Where ceil(n / 32) <= OCC4D_PULL_LDS_WORDS each workgroup first copies `blocked` into LDS and walks its copy (measured faster than
 *   reading global memory in every comparison: the kernel waits on one word after another); a larger grid is read where it is.  The
 *   results are the same bits either way.  No atomics, no work array, no workgroup waits for another one.
 *
 * ACCESS SAFETY.  No value read from memory reaches an address without a range test.  clear is read at p in [0, n) only, with p from
 * the thread's own index; a, b, hit, path_len and waypoint_len are indexed by the thread's or the workgroup's own pair or goal;
 * paths and waypoints at g * cap + k with 0 <= k < cap, and a chain position only after L <= cap.  A value of a, b or paths becomes
 * coordinates only after 0 <= v < n.  A word of `blocked` is read only for a cell whose three coordinates were tested against
 * [0, nx) x [0, ny) x [0, nz) immediately before (solid_at of csrc/sight_math.hpp), so its index is < ceil(n / 32).  No value of
 * blocked or paths is an index otherwise. */
#ifndef OCC4D_PULL_H
#define OCC4D_PULL_H

#include <stdint.h>

#include "occ4d_sight.h"                   /* OCC4D_SIGHT_MAX_AXIS: the longest axis */

#define OCC4D_PULL_ROUND 256               /* the candidates of one round = the threads of a goal's workgroup */
#define OCC4D_PULL_LDS_WORDS 32768         /* the most words of `blocked` a workgroup stages in LDS: 128 KiB, 2^20 grid points */

#ifdef __cplusplus
extern "C" {
#endif

/* clear (n) int32;  0 <= n <= INT32_MAX;  blocked (ceil(n / 32)) uint32.  n == 0 is a no-op that touches no pointer. */
int occ4d_pull_bits_i32(const int32_t* clear, int min_clear, int64_t n, uint32_t* blocked, void* stream);

/* blocked: as above, for n = nx * ny * nz (not read when n == 0: every index is then outside);  0 <= nx, ny, nz <=
 * OCC4D_SIGHT_MAX_AXIS;  a, b (n_pairs) int32 flat indices, any values;  hit (n_pairs) int32 = HIT(a, b).
 * n_pairs == 0 is a no-op that touches no pointer. */
int occ4d_pull_pairs_u32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* a, const int32_t* b, int n_pairs,
                         int32_t* hit, void* stream);

/* blocked, nx, ny, nz: as above;  paths (n_goals, cap) int32 and path_len (n_goals) int32 as occ4d_geodesic_trace_i32 left them,
 * any values;  cap >= 0, n_goals * cap <= INT32_MAX;  waypoints (n_goals, cap) int32;  waypoint_len (n_goals) int32.
 * n_goals == 0 or n == 0 is a no-op that touches no pointer. */
int occ4d_pull_paths_i32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* paths, const int32_t* path_len, int n_goals,
                         int cap, int32_t* waypoints, int32_t* waypoint_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif
