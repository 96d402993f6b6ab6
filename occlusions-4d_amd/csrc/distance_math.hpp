// The distance transform of the grid's solid set (include/ext/occ4d_distance.h), shared WORD FOR WORD by the HIP kernel
// (csrc/distance.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the site test, the order relation of the candidates, a line's
// minimum, the tiling of a stage, the two item bodies of a tile and the argument contract (host only).  Integers only; the float
// operations are the >= comparisons of is_site().
#pragma once
#include <stdint.h>

#include "ext/occ4d_distance.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_distance {

constexpr int32_t NONE = OCC4D_DISTANCE_NONE;
constexpr int MAX_AXIS = OCC4D_DISTANCE_MAX_AXIS;
constexpr int TILE_POINTS = OCC4D_DISTANCE_TILE_POINTS;
constexpr int TILE_WIDTH = OCC4D_DISTANCE_TILE_WIDTH;
constexpr int RUN_POINTS = OCC4D_DISTANCE_RUN_POINTS;
static_assert(NONE == INT32_MAX && MAX_AXIS * (TILE_WIDTH / 2) <= TILE_POINTS && MAX_AXIS <= RUN_POINTS && RUN_POINTS <= TILE_POINTS,
              "the longest line fits a tile at half the width, and a run");

struct Args {
  const float* field; int64_t ld;
  const float* mask; int64_t ld_mask;
  int32_t *dist2, *nearest;                                       // nearest: null = not computed
  int n[3], w[3];                                                 // nx, ny, nz;  wx, wy, wz
  int64_t points;
  float level, mask_level;
  int target;
};

// ---- the rules
OCC4D_HD bool is_site(const Args& a, int64_t p) {
  bool member = a.field[p * a.ld] >= a.level;
  if (member && a.mask) member = a.mask[p * a.ld_mask] >= a.mask_level;
  return member != (a.target != 0);
}

// THE ORDER RELATION.  A candidate is the entry at axis index `at` of the point's line: its own cost c (NONE: it has no site) plus
// step = w * (at - l)^2 for the steps between them.  The lower cost wins, then the lower axis index.  line_min visits the
// candidates in ASCENDING index, so "strictly lower cost" alone is that relation: a later candidate of equal cost has the higher
// index and loses.  No candidate's cost is NONE (the bound of the header leaves INT32_MAX free), so {NONE, -1} is "none so far" and
// needs no test of its own.  Two selects, no branch.
struct Best {
  int32_t cost, at;
};

OCC4D_HD void consider(Best& b, int32_t c, int32_t step, int at) {
  const int32_t cand = c == NONE ? NONE : c + step;               // the cost between the point and the entry's site
  const bool take = cand < b.cost;
  b.cost = take ? cand : b.cost;
  b.at = take ? at : b.at;
}

// The minimum over the L entries cost[0], cost[stride], ... of a line, for its point l.  step runs through w * (at - l)^2 by its
// differences, w * (2 (at - l) + 1), which grow by 2 w: two additions per candidate, no product.  For at < L it is a term of a legal
// cost; the value formed behind the last candidate is never used and may not be one, so the two run modulo 2^32 (unsigned).
OCC4D_HD Best line_min(const int32_t* cost, int stride, int L, int l, int w) {
  Best b{NONE, -1};
  uint32_t step = (uint32_t)w * (uint32_t)(l * l), grow = (uint32_t)w * (uint32_t)(1 - 2 * l);
#pragma unroll 4
  for (int at = 0; at < L; ++at) {
    consider(b, cost[at * stride], (int32_t)step, at);
    step += grow;
    grow += 2u * (uint32_t)w;
  }
  return b;
}

// ---- a stage: the array viewed as (outer, L, inner), the point (o, l, i) at flat index (o * L + l) * inner + i; its lines run
// along l.  Stage 0 (z): (nx * ny, nz, 1);  1 (y): (nx, ny, nz);  2 (x): (1, nx, ny * nz).
// A TILE is `width` whole lines.  Stage 0: consecutive o (a contiguous run of the array), slot s = j * L + l for line j;  stages
// 1 and 2: consecutive i of one o, slot s = l * width + j.  Either way neighbouring slots are neighbouring addresses.
struct Pass {
  int64_t outer, inner, per_outer, tiles;                         // per_outer: tiles of one o (stages 1, 2)
  int L, w, width, stage;
};

OCC4D_HD int run_width(int L) { return RUN_POINTS / L > 1 ? RUN_POINTS / L : 1; }             // lines of a tile of stage 0

OCC4D_HD int tile_width(int L) {                                                                // ... of stages 1 and 2
  int width = TILE_WIDTH;
  while (width > 1 && (int64_t)width * L > TILE_POINTS) width /= 2;
  return width;
}

// width 0: the launcher's (run_width / tile_width);  the twin passes 1: line by line
OCC4D_HD Pass pass_of(const Args& a, int stage, int width) {
  Pass ps;
  const int64_t nx = a.n[0], ny = a.n[1], nz = a.n[2];
  ps.stage = stage;
  ps.outer = stage == 0 ? nx * ny : stage == 1 ? nx : 1;
  ps.inner = stage == 0 ? 1 : stage == 1 ? nz : ny * nz;
  ps.L = a.n[2 - stage];
  ps.w = a.w[2 - stage];
  ps.width = width > 0 ? width : stage == 0 ? run_width(ps.L) : tile_width(ps.L);
  ps.per_outer = (ps.inner + ps.width - 1) / ps.width;
  ps.tiles = stage == 0 ? (ps.outer + ps.width - 1) / ps.width : ps.outer * ps.per_outer;
  return ps;
}

OCC4D_HD int tile_slots(const Pass& ps) { return ps.L * ps.width; }

struct Tile {
  int64_t o, first;                                               // stage 0: lines o = first ..;  else: lines i = first .. of this o
  int lines;                                                      // <= width: the last tile may hold fewer
};

OCC4D_HD Tile tile_of(const Pass& ps, int64_t b) {
  Tile t;
  t.o = ps.stage == 0 ? 0 : b / ps.per_outer;
  t.first = ps.stage == 0 ? b * ps.width : (b % ps.per_outer) * ps.width;
  const int64_t left = (ps.stage == 0 ? ps.outer : ps.inner) - t.first;
  t.lines = left < ps.width ? (int)left : ps.width;
  return t;
}

// slot s in [0, tile_slots) -> its line j of the tile and its axis index l; whether the tile has that line
OCC4D_HD bool slot_point(const Pass& ps, const Tile& t, int s, int& j, int& l, int64_t& p) {
  if (ps.stage == 0) {
    j = s / ps.L;
    l = s - j * ps.L;
    p = (t.first + j) * ps.L + l;
  } else {
    l = s / ps.width;
    j = s - l * ps.width;
    p = (t.o * ps.L + l) * ps.inner + t.first + j;
  }
  return j < t.lines;
}

// step 1 (then a barrier): the (cost, site) pair of slot s into the tile.  Stage 0 makes it from the site test, the others read what
// the stage before wrote.  s_site: null without `nearest`.
OCC4D_HD void stage_item(const Args& a, const Pass& ps, const Tile& t, int s, int32_t* s_cost, int32_t* s_site) {
  int j, l;
  int64_t p;
  if (!slot_point(ps, t, s, j, l, p)) return;
  if (ps.stage == 0) {
    const bool site = is_site(a, p);
    s_cost[s] = site ? 0 : NONE;
    if (s_site) s_site[s] = site ? (int32_t)p : -1;
  } else {
    s_cost[s] = a.dist2[p];
    if (s_site) s_site[s] = a.nearest[p];
  }
}

// step 2: the minimum over the line of slot s, written IN PLACE: the tile holds every line it writes, whole, since step 1
OCC4D_HD void min_item(const Args& a, const Pass& ps, const Tile& t, int s, const int32_t* s_cost, const int32_t* s_site) {
  int j, l;
  int64_t p;
  if (!slot_point(ps, t, s, j, l, p)) return;
  const int base = ps.stage == 0 ? j * ps.L : j, stride = ps.stage == 0 ? 1 : ps.width;
  const Best b = line_min(s_cost + base, stride, ps.L, l, ps.w);
  a.dist2[p] = b.cost;
  if (s_site) a.nearest[p] = b.at >= 0 ? s_site[base + b.at * stride] : -1;
}

// ---- the argument contract (host): the status, `empty` = nothing to do, the arguments filled
inline int check_distance(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level, int target,
                          int nx, int ny, int nz, int wx, int wy, int wz, int32_t* dist2, int32_t* nearest, bool& empty, Args& a) {
  const char* who = "occ4d_distance_grid_f32";
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX",
                who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  OCC4D_REQUIRE(target == 0 || target == 1, "%s: target = %d must be 0 or 1", who, target);
  OCC4D_REQUIRE(wx >= 1 && wy >= 1 && wz >= 1, "%s: wx = %d, wy = %d, wz = %d must be >= 1", who, wx, wy, wz);
  const int64_t dx = nx > 0 ? nx - 1 : 0, dy = ny > 0 ? ny - 1 : 0, dz = nz > 0 ? nz - 1 : 0;
  const int64_t largest = wx * dx * dx + wy * dy * dy + wz * dz * dz;     // (< 2^31 * 2^18 * 3)
  OCC4D_REQUIRE(largest <= (int64_t)INT32_MAX - 1, "%s: the largest cost %lld = %d * %lld^2 + %d * %lld^2 + %d * %lld^2 exceeds INT32_MAX - 1",
                who, (long long)largest, wx, (long long)dx, wy, (long long)dy, wz, (long long)dz);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(!mask || ld_mask >= 1, "%s: ld_mask = %lld must be >= 1", who, (long long)ld_mask);
  const int64_t n = (int64_t)nx * ny * nz;
  empty = n == 0;
  OCC4D_REQUIRE(empty || field, "%s: null field with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(empty || dist2, "%s: null dist2 with n = %lld", who, (long long)n);
  a = Args{field, ld, mask, ld_mask, dist2, nearest, {nx, ny, nz}, {wx, wy, wz}, n, level, mask_level, target};
  return OCC4D_OK;
}

}  // namespace occ4d_distance
