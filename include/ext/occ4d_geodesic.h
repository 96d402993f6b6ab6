/* occ4d_geodesic.h -- shortest free-space paths over the query grid, on the device (geodesic.solve, inference.perform_inference(
 * route=...)): per grid point the least total step cost of a path from any seed that never leaves the passable set, which neighbour
 * that path comes from, and the paths themselves from chosen goals back to a seed.  Integers only, no floats anywhere; the rules
 * below fix every output bit of a converged call whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_distance.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the
 * stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_components.h / occ4d_distance.h: (nx, ny, nz) points, x slowest, z fastest, flat index
 *     p = (ix * ny + iy) * nz + iz, n = nx * ny * nz.  An axis of length 1 is legal.  Every axis is <= OCC4D_GEODESIC_MAX_AXIS.
 *   PASSABLE.  passable(p) = clear[p] >= min_clear, an int32 comparison.  `clear` is any (n) int32 array; with dist2 of
 *     occ4d_distance.h, min_clear = 1 is "not solid" and min_clear = r^2 "a ball of radius r fits".
 *   MOVES.  The neighbours of a point differ from it by at most 1 on every axis and on 1 (face), 2 (edge) or 3 (corner) axes;
 *     connectivity 6 has the face moves, 18 also the edge moves, 26 all.  A move costs step_face, step_edge or step_corner, integers
 *     >= 1.  It is legal when BOTH its end points are passable; there is no further corner-cutting rule (inflate with min_clear).
 *     The call is rejected unless (n - 1) * max(step_face, step_edge, step_corner) <= INT32_MAX - 1, tested in 64 bits at entry: a
 *     stored cost is that of a path without a repeated point, so it is within that bound, and a kernel forms the sum v + w only after
 *     v < best - w, so no sum it forms overflows int32.
 *   NEIGHBOUR ORDER.  Neighbour c = 0 .. 26 without 13 has the offset (dx, dy, dz) = (c / 9 - 1, (c / 3) % 3 - 1, c % 3 - 1): raster
 *     order, the lower flat index first.  Those the connectivity leaves out are skipped.
 *   SEEDS.  seeds (n_seeds) int32 flat indices.  A seed outside [0, n) or not passable is no source; the test is made on the device
 *     and precedes every use of the value.
 *   cost (n) int32:  the least total cost of a legal path from any seed; 0 at a seed; OCC4D_GEODESIC_NONE where the point is not
 *     passable or no path reaches it.
 *   status (2) int32:  status[0] = 1 iff one of the `rounds` relaxation rounds changed no value: cost is then the fixed point.
 *     status[1] = the number of rounds that changed one.
 *       status[0] == 1:  cost is the shortest-path cost, every bit fixed whatever the scheduling and the tiling.
 *       status[0] == 0:  every value is >= the shortest-path cost and the seeds are 0; nothing else is promised, equality between
 *         two runs included.  A further call with resume = 1 goes on from there.
 *   parent (n) int32, or null (not computed):  filled from the finished cost.  For a point with 0 < cost < NONE the first
 *     neighbour q in the NEIGHBOUR ORDER with cost[q] + w(q, p) == cost[p]; -1 at seeds (cost 0), at points without a cost, and
 *     where no neighbour qualifies (which a converged call never shows).  Deterministic when cost is; meaningful with status[0] == 1.
 *   TRACE.  Per goal one serial chain: goal, parent[goal], ... until a point whose parent is outside [0, n) -- a seed.  paths
 *     (n_goals, cap) int32 holds the chain's first min(length, cap) points and -1 behind them; path_len (n_goals) int32 the length,
 *     0 for a goal outside [0, n) or with cost NONE (or below 0), and -needed when the chain has needed > cap points.
 *
 * ALGORITHM (csrc/geodesic.hip): a block relaxation.  A workgroup owns a tile of OCC4D_GEODESIC_TILE_X x _Y x _Z points, loads
 * them and a halo of one point into LDS, relaxes its own points there until none changes (a `for` bounded by the tile's points, left
 * on a workgroup vote) and writes back what it lowered; the halo is read only.  One launch per round; round k returns at once when
 * round k - 1 lowered nothing (one word per round in `work`).  Launches: 1 (seeding) + rounds + 1 (status) + 1 with parent, whatever
 * the data.  No workgroup waits for another one.  Words that another workgroup may write in the same launch are read and written
 * with relaxed device-scope atomics: either value is an upper bound of the true cost, and only a point's owner writes it.
 *
 * ACCESS SAFETY.  clear, cost and parent are indexed by flat indices made of coordinates that passed 0 <= c < n_axis, or by a seed /
 * goal / parent value that passed 0 <= v < n just before.  No value of clear or cost reaches an address. */
#ifndef OCC4D_GEODESIC_H
#define OCC4D_GEODESIC_H

#include <stdint.h>

#define OCC4D_GEODESIC_NONE 2147483647     /* cost of a point no path reaches: INT32_MAX */
#define OCC4D_GEODESIC_MAX_AXIS 512        /* the longest axis */
#define OCC4D_GEODESIC_TILE_X 8            /* a workgroup's tile of grid points: one thread per point */
#define OCC4D_GEODESIC_TILE_Y 8
#define OCC4D_GEODESIC_TILE_Z 8
#define OCC4D_GEODESIC_MAX_ROUNDS 65536    /* the most rounds (launches) of one call */

#ifdef __cplusplus
extern "C" {
#endif

/* clear (n) int32;  seeds (n_seeds) int32, null with n_seeds == 0;  connectivity 6, 18 or 26;  steps >= 1 within the bound of MOVES;
 * 0 <= rounds <= OCC4D_GEODESIC_MAX_ROUNDS;  resume 0: cost is made from the seeds;  1: cost is what an earlier call with the same
 * other arguments left, and the rounds go on from it (seeds is not read);  work: rounds + 1 int32 (no contents expected);
 * cost (n) int32;  parent (n) int32 or null;  status (2) int32.
 * n == 0 is a no-op that touches no pointer. */
int occ4d_geodesic_grid_i32(const int32_t* clear, int min_clear, int nx, int ny, int nz, const int32_t* seeds, int n_seeds,
                            int connectivity, int step_face, int step_edge, int step_corner, int rounds, int resume,
                            int32_t* work, int32_t* cost, int32_t* parent, int32_t* status, void* stream);

/* cost, parent (n) int32 as the call above left them, 0 <= n;  goals (n_goals) int32;  cap >= 0;  paths (n_goals, cap) int32;
 * path_len (n_goals) int32.  n_goals == 0 is a no-op that touches no pointer. */
int occ4d_geodesic_trace_i32(const int32_t* cost, const int32_t* parent, int n, const int32_t* goals, int n_goals, int cap,
                             int32_t* paths, int32_t* path_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif
