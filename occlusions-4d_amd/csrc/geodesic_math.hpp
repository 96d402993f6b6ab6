// Shortest free-space paths over the grid (include/ext/occ4d_geodesic.h), shared WORD FOR WORD by the HIP kernels
// (csrc/geodesic.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the neighbour table and its order, the relax step, the parent
// rule, the seed test, the tiling, the trace and the two argument contracts (host only).  Integers only.
//
// ONE FACT carries the rest: a point that is not passable keeps the cost NONE for ever -- it is never seeded and never relaxed --,
// so "the neighbour's cost is a cost" (0 <= v < NONE) already says that the neighbour is passable, and only a point's OWN
// passability is ever looked up in `clear`.
#pragma once
#include <stdint.h>

#include "ext/occ4d_geodesic.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_geodesic {

constexpr int32_t NONE = OCC4D_GEODESIC_NONE;
constexpr int MAX_AXIS = OCC4D_GEODESIC_MAX_AXIS, MAX_ROUNDS = OCC4D_GEODESIC_MAX_ROUNDS;
constexpr int TX = OCC4D_GEODESIC_TILE_X, TY = OCC4D_GEODESIC_TILE_Y, TZ = OCC4D_GEODESIC_TILE_Z;
constexpr int TILE_POINTS = TX * TY * TZ;                         // one thread per point
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;              // the tile and its halo of one point
constexpr int HALO_POINTS = HX * HY * HZ;
constexpr int NEIGHBOURS = 27;                                    // offsets c = 0 .. 26; c = 13 is the point itself
static_assert(NONE == INT32_MAX && TILE_POINTS <= 1024, "a tile is one workgroup");

struct Args {
  const int32_t* clear;
  const int32_t* seeds;
  int32_t *cost, *parent, *status;
  int32_t* flags;                                                 // work: flags[0] = 1, flags[k] = round k lowered a value, k = 1 .. rounds
  int n[3], tiles[3];
  int64_t points, n_tiles;
  int step[3];                                                    // face, edge, corner
  int min_clear, n_seeds, rank, rounds, resume;                   // rank 1, 2, 3: the most axes a move changes
};

struct TraceArgs {
  const int32_t *cost, *parent, *goals;
  int32_t *paths, *path_len;
  int n, n_goals, cap;
};

// ---- the rules
OCC4D_HD bool is_cost(int32_t v) { return (uint32_t)v < (uint32_t)NONE; }                      // 0 <= v < NONE

// THE RELAX STEP.  best: the point's value so far, 0 <= best <= NONE;  v: a neighbour's value;  w >= 1: the move's cost.  The sum
// v + w is formed only when it is below best, hence below 2^31: no overflow (best - w >= -INT32_MAX).
OCC4D_HD int32_t relax(int32_t best, int32_t v, int32_t w) { return is_cost(v) && v < best - w ? v + w : best; }

// neighbour c: its offset, and the number of axes it changes (0: the point itself); the NEIGHBOUR ORDER of the header is ascending c
OCC4D_HD int offset_of(int c, int* d) {
  d[0] = c / 9 - 1;
  d[1] = (c / 3) % 3 - 1;
  d[2] = c % 3 - 1;
  return (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
}

// The least of `own` and every neighbour's value plus its move, over the moves of this connectivity.  at(dx, dy, dz): the value
// at that offset, NONE outside the grid.  Called for passable points only.
template <class F>
OCC4D_HD int32_t relax_point(int rank, const int* step, int32_t own, F&& at) {
  int32_t best = own;
#pragma unroll
  for (int c = 0; c < NEIGHBOURS; ++c) {
    int d[3];
    const int kind = offset_of(c, d);
    if (kind == 0 || kind > rank) continue;
    best = relax(best, at(d[0], d[1], d[2]), step[kind - 1]);
  }
  return best;
}

// THE PARENT RULE: the first neighbour c in order with value + move == own, for 0 < own < NONE; -1 otherwise
template <class F>
OCC4D_HD int parent_choice(int rank, const int* step, int32_t own, F&& at) {
  if (!is_cost(own) || own == 0) return -1;
  for (int c = 0; c < NEIGHBOURS; ++c) {
    int d[3];
    const int kind = offset_of(c, d);
    if (kind == 0 || kind > rank) continue;
    const int32_t v = at(d[0], d[1], d[2]);
    if (is_cost(v) && v == own - step[kind - 1]) return c;          // (own - step > -2^31; a negative one equals no cost)
  }
  return -1;
}

OCC4D_HD void coords_of(const Args& a, int64_t p, int* i) {
  i[2] = (int)(p % a.n[2]);
  i[1] = (int)((p / a.n[2]) % a.n[1]);
  i[0] = (int)(p / ((int64_t)a.n[1] * a.n[2]));
}

// the flat index of the coordinates, -1 outside the grid
OCC4D_HD int64_t flat_of(const Args& a, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0 || x >= a.n[0] || y >= a.n[1] || z >= a.n[2]) return -1;
  return ((int64_t)x * a.n[1] + y) * a.n[2] + z;
}

OCC4D_HD bool passable(const Args& a, int64_t p) { return a.clear[p] >= a.min_clear; }

// seed k as a source: its flat index, or -1 (outside [0, n) -- tested before any use --, or not passable)
OCC4D_HD int64_t seed_point(const Args& a, int k) {
  const int32_t s = a.seeds[k];
  if (s < 0 || (int64_t)s >= a.points) return -1;
  return passable(a, s) ? (int64_t)s : -1;
}

// the neighbour values of point (i) straight from cost[]: the parent pass, and the twin's relaxation of the whole grid in place
struct GridAt {
  const Args& a;
  const int* i;
  OCC4D_HD int32_t operator()(int dx, int dy, int dz) const {
    const int64_t q = flat_of(a, i[0] + dx, i[1] + dy, i[2] + dz);
    return q < 0 ? NONE : a.cost[q];
  }
};

// the parent pass, point p: from the FINISHED cost
OCC4D_HD void parent_item(const Args& a, int64_t p) {
  int i[3], d[3];
  coords_of(a, p, i);
  const int c = parent_choice(a.rank, a.step, a.cost[p], GridAt{a, i});
  if (c >= 0) offset_of(c, d);
  a.parent[p] = c < 0 ? -1 : (int32_t)flat_of(a, i[0] + d[0], i[1] + d[1], i[2] + d[2]);     // (in the grid: its value was a cost)
}

// the status pass: `changed` = the number of k in 1 .. rounds with flags[k] != 0.  A round that lowered nothing is followed by
// rounds that return at once, so changed < rounds says that one of them changed no value.
OCC4D_HD void status_item(const Args& a, int changed) {
  a.status[0] = changed < a.rounds ? 1 : 0;
  a.status[1] = changed;
}

// ---- the tiling of csrc/geodesic.hip: tile b of tiles[0] x tiles[1] x tiles[2], z fastest; thread t owns the point (lx, ly, lz) =
// (t / (TY TZ), (t / TZ) % TY, t % TZ) of the tile; LDS slot of a point of the tile-with-halo box (hx, hy, hz) = (hx HY + hy) HZ + hz
OCC4D_HD void tile_origin(const Args& a, int64_t b, int* o) {
  o[2] = (int)(b % a.tiles[2]) * TZ;
  o[1] = (int)((b / a.tiles[2]) % a.tiles[1]) * TY;
  o[0] = (int)(b / ((int64_t)a.tiles[1] * a.tiles[2])) * TX;
}

OCC4D_HD int64_t halo_point(const Args& a, const int* o, int h) {     // h in [0, HALO_POINTS) -> flat index, -1 outside the grid
  return flat_of(a, o[0] + h / (HY * HZ) - 1, o[1] + (h / HZ) % HY - 1, o[2] + h % HZ - 1);
}

OCC4D_HD int own_slot(int t) { return ((t / (TY * TZ) + 1) * HY + (t / TZ) % TY + 1) * HZ + t % TZ + 1; }
OCC4D_HD int64_t own_point(const Args& a, const int* o, int t) { return flat_of(a, o[0] + t / (TY * TZ), o[1] + (t / TZ) % TY, o[2] + t % TZ); }

// the index in the tile (thread t) of flat index p, -1 when p lies in another tile
OCC4D_HD int tile_index(const Args& a, const int* o, int64_t p) {
  int i[3];
  coords_of(a, p, i);
  const int lx = i[0] - o[0], ly = i[1] - o[1], lz = i[2] - o[2];
  if (lx < 0 || ly < 0 || lz < 0 || lx >= TX || ly >= TY || lz >= TZ) return -1;
  return (lx * TY + ly) * TZ + lz;
}

// ---- the trace of goal g: one serial chain.  Every index -- the goal, each parent -- passes 0 <= v < n before it is used.  The
// writing loop is a `for` bounded by cap; the count behind it (only when the chain is longer than cap) a `for` bounded by n: a
// chain of a converged call repeats no point, and a foreign array with a cycle ends there too.
OCC4D_HD void trace_item(const TraceArgs& a, int g) {
  int32_t* row = a.paths + (int64_t)g * a.cap;
  int32_t cur = a.goals[g];
  if (cur < 0 || cur >= a.n || !is_cost(a.cost[cur])) cur = -1;
  int len = 0;
  for (int k = 0; k < a.cap; ++k) {
    row[k] = cur;
    if (cur < 0) continue;
    ++len;
    const int32_t up = a.parent[cur];
    cur = up < 0 || up >= a.n ? -1 : up;
  }
  int needed = len;
  for (int k = a.cap; k < a.n && cur >= 0; ++k) {
    ++needed;
    const int32_t up = a.parent[cur];
    cur = up < 0 || up >= a.n ? -1 : up;
  }
  a.path_len[g] = needed > len || cur >= 0 ? -(needed > len ? needed : len + 1) : len;
}

// ---- the argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_geodesic(const int32_t* clear, int min_clear, int nx, int ny, int nz, const int32_t* seeds, int n_seeds, int connectivity,
                          int step_face, int step_edge, int step_corner, int rounds, int resume, int32_t* work, int32_t* cost,
                          int32_t* parent, int32_t* status, bool& empty, Args& a) {
  const char* who = "occ4d_geodesic_grid_i32";
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  OCC4D_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity = %d must be 6, 18 or 26", who,
                connectivity);
  OCC4D_REQUIRE(step_face >= 1 && step_edge >= 1 && step_corner >= 1, "%s: step_face = %d, step_edge = %d, step_corner = %d must be >= 1",
                who, step_face, step_edge, step_corner);
  const int64_t n = (int64_t)nx * ny * nz;                                                       // <= 2^27
  const int64_t top = step_face > step_edge ? (step_face > step_corner ? step_face : step_corner)
                                             : (step_edge > step_corner ? step_edge : step_corner);
  const int64_t longest = (n > 0 ? n - 1 : 0) * top;                                             // < 2^27 * 2^31
  OCC4D_REQUIRE(longest <= (int64_t)INT32_MAX - 1, "%s: the longest path %lld = (%lld - 1) * %lld exceeds INT32_MAX - 1", who,
                (long long)longest, (long long)n, (long long)top);
  OCC4D_REQUIRE(n_seeds >= 0, "%s: n_seeds = %d must be >= 0", who, n_seeds);
  OCC4D_REQUIRE(rounds >= 0 && rounds <= MAX_ROUNDS, "%s: rounds = %d must be in [0, %d]", who, rounds, MAX_ROUNDS);
  OCC4D_REQUIRE(resume == 0 || resume == 1, "%s: resume = %d must be 0 or 1", who, resume);
  empty = n == 0;
  OCC4D_REQUIRE(empty || clear, "%s: null clear with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(empty || resume || n_seeds == 0 || seeds, "%s: null seeds with n_seeds = %d", who, n_seeds);
  OCC4D_REQUIRE(empty || (work && cost && status), "%s: null work / cost / status with n = %lld", who, (long long)n);
  a.clear = clear; a.seeds = seeds; a.cost = cost; a.parent = parent; a.status = status; a.flags = work;
  a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
  a.tiles[0] = (nx + TX - 1) / TX; a.tiles[1] = (ny + TY - 1) / TY; a.tiles[2] = (nz + TZ - 1) / TZ;
  a.points = n;
  a.n_tiles = (int64_t)a.tiles[0] * a.tiles[1] * a.tiles[2];
  a.step[0] = step_face; a.step[1] = step_edge; a.step[2] = step_corner;
  a.min_clear = min_clear; a.n_seeds = n_seeds; a.rank = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  a.rounds = rounds; a.resume = resume;
  return OCC4D_OK;
}

inline int check_trace(const int32_t* cost, const int32_t* parent, int n, const int32_t* goals, int n_goals, int cap, int32_t* paths,
                       int32_t* path_len, bool& empty, TraceArgs& a) {
  const char* who = "occ4d_geodesic_trace_i32";
  OCC4D_REQUIRE(n >= 0, "%s: n = %d must be >= 0", who, n);
  OCC4D_REQUIRE(n_goals >= 0, "%s: n_goals = %d must be >= 0", who, n_goals);
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  OCC4D_REQUIRE((int64_t)n_goals * cap <= INT32_MAX, "%s: n_goals * cap = %d * %d exceeds INT32_MAX", who, n_goals, cap);
  empty = n_goals == 0;
  OCC4D_REQUIRE(empty || goals, "%s: null goals with n_goals = %d", who, n_goals);
  OCC4D_REQUIRE(empty || n == 0 || (cost && parent), "%s: null cost / parent with n = %d", who, n);
  OCC4D_REQUIRE(empty || path_len, "%s: null path_len with n_goals = %d", who, n_goals);
  OCC4D_REQUIRE(empty || cap == 0 || paths, "%s: null paths with n_goals = %d, cap = %d", who, n_goals, cap);
  a = TraceArgs{cost, parent, goals, paths, path_len, n, n_goals, cap};
  return OCC4D_OK;
}

}  // namespace occ4d_geodesic
