// Measured returns carved into the query grid (include/ext/occ4d_evidence.h), shared WORD FOR WORD by the HIP kernels
// (csrc/evidence.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the snap, the walk, the body of a return, the code of a cell and the
// two argument contracts (host only).  Where a mark lands -- an atomic in global memory, an atomic in LDS, a plain store in the twin
// -- is the caller's `Marks`: hit(flat), pass(flat) and arrive(flat) = the pass of the sensor's own cell.  The solid test is csrc/sight_math.hpp's member(), CALLED here.  The floats
// are the snap's subtraction, division and floorf and member()'s comparisons; both builds compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ext/occ4d_evidence.h"
#include "sight_math.hpp"         // sm::member, sm::BitsArgs, MAX_AXIS; OCC4D_HD; contract.hpp

namespace occ4d_evidence {

namespace sm = occ4d_sight;

constexpr int MAX_AXIS = sm::MAX_AXIS;
constexpr int MAX_SENSORS = OCC4D_EVIDENCE_MAX_SENSORS;
constexpr int MAX_COORD = OCC4D_EVIDENCE_MAX_COORD;
static_assert(MAX_COORD == sm::MAX_COORD, "the walk's terms stay below 2^43 as occ4d_sight.h's do");
enum { CARVED = 0, DROP_SENSOR = 1, DROP_FAR = 2, DROP_OUTSIDE = 3 };           // the slots of status

struct CarveArgs {
  const float* returns; int64_t ld, R;
  const int32_t* sensor;                                          // null: sensor 0
  const int32_t* origins; int V;
  int n[3];
  float min[3], spacing[3];
  uint32_t* passed; int32_t *hits, *passes, *status;              // passes: null = not counted
  int64_t points, words;
};

struct ClassifyArgs {
  sm::BitsArgs solid;                                             // field, ld, mask, ld_mask, level, mask_level, n of member()
  const uint32_t* passed; const int32_t *passes, *hits;
  int32_t* code; int64_t* totals;
  int min_pass;
};

// ---- the rules
// SNAP of one axis -> false: DROPPED 2.  The float is compared with 2^20 before it becomes an integer; a NaN fails.
OCC4D_HD bool snap(float p, float min, float spacing, int& cell) {
  const float g = floorf((p - min) / spacing);
  if (!(fabsf(g) <= (float)MAX_COORD)) return false;
  cell = (int)g;
  return true;
}

OCC4D_HD bool coord_ok(int32_t c) { return c >= -MAX_COORD && c <= MAX_COORD; }

// THE WALK from the return's cell e (in the grid) towards the origin o: sight_math.hpp's stepping -- the six 64-bit terms that grow
// by additions, T = the live axes that no axis beats -- without the SQUEEZE and the solid test.  Every cell stepped into is passed
// while it lies in the grid, o included.
template <class Marks>
OCC4D_HD void walk(const int* n, const Marks& marks, int ex, int ey, int ez, int ox, int oy, int oz) {
  int cx = ex, cy = ey, cz = ez;
  const int sx = ox > ex ? 1 : -1, sy = oy > ey ? 1 : -1, sz = oz > ez ? 1 : -1;      // (the sign of a dead axis is never used)
  const int64_t mx = ox > ex ? (int64_t)ox - ex : (int64_t)ex - ox, my = oy > ey ? (int64_t)oy - ey : (int64_t)ey - oy,
                mz = oz > ez ? (int64_t)oz - ez : (int64_t)ez - oz;
  int64_t pxy = my, pyx = mx, pxz = mz, pzx = mx, pyz = mz, pzy = my;                 // j = 0: (2 j + 1) = 1
  const int bound = n[0] + n[1] + n[2];
  for (int step = 0; step < bound; ++step) {
    const bool tx = cx != ox && !(pyx < pxy) && !(pzx < pxz);
    const bool ty = cy != oy && !(pxy < pyx) && !(pzy < pyz);
    const bool tz = cz != oz && !(pxz < pzx) && !(pyz < pzy);
    if (!(tx || ty || tz)) return;                                                    // c == o
    if (tx) { cx += sx; pxy += 2 * my; pxz += 2 * mz; }
    if (ty) { cy += sy; pyx += 2 * mx; pyz += 2 * mz; }
    if (tz) { cz += sz; pzx += 2 * mx; pzy += 2 * my; }
    if (!((unsigned)cx < (unsigned)n[0] && (unsigned)cy < (unsigned)n[1] && (unsigned)cz < (unsigned)n[2])) return;   // the grid is convex
    const int32_t flat = (cx * n[1] + cy) * n[2] + cz;
    if (cx == ox && cy == oy && cz == oz) { marks.arrive(flat); return; }              // o is passed as any other cell: a call site of its own
    marks.pass(flat);
  }
}

// the body of return r -> its slot of status
template <class Marks>
OCC4D_HD int return_item(const CarveArgs& a, int64_t r, const Marks& marks) {
  const int32_t v = a.sensor ? a.sensor[r] : 0;
  if (v < 0 || v >= a.V) return DROP_SENSOR;
  const int32_t* o = a.origins + 3 * (int64_t)v;
  const int32_t ox = o[0], oy = o[1], oz = o[2];
  if (!(coord_ok(ox) && coord_ok(oy) && coord_ok(oz))) return DROP_SENSOR;
  const float* p = a.returns + r * a.ld;
  int ex = 0, ey = 0, ez = 0;
  const bool in_reach = snap(p[0], a.min[0], a.spacing[0], ex) & snap(p[1], a.min[1], a.spacing[1], ey) & snap(p[2], a.min[2], a.spacing[2], ez);
  if (!in_reach) return DROP_FAR;
  if (!((unsigned)ex < (unsigned)a.n[0] && (unsigned)ey < (unsigned)a.n[1] && (unsigned)ez < (unsigned)a.n[2])) return DROP_OUTSIDE;
  marks.hit((ex * a.n[1] + ey) * a.n[2] + ez);
  walk(a.n, marks, ex, ey, ez, ox, oy, oz);
  return CARVED;
}

// STATE and CODE of cell p
OCC4D_HD int state_of(const ClassifyArgs& a, int64_t p) {
  if (a.hits[p] > 0) return OCC4D_EVIDENCE_HIT;
  const bool is_free = a.passes ? a.passes[p] >= a.min_pass : (a.passed[p >> 5] >> (p & 31)) & 1u;
  return is_free ? OCC4D_EVIDENCE_FREE : OCC4D_EVIDENCE_UNKNOWN;
}

OCC4D_HD int code_of(const ClassifyArgs& a, int64_t p) { return state_of(a, p) + 3 * (int)sm::member(a.solid, p); }

// ---- the argument contracts (host): the status, the arguments filled
inline int check_carve(const float* returns, int64_t ld_returns, int64_t R, const int32_t* sensor, const int32_t* origins, int V, int nx,
                       int ny, int nz, float x0, float sx, float y0, float sy, float z0, float sz, uint32_t* passed, int32_t* hits,
                       int32_t* passes, int32_t* status, CarveArgs& a) {
  const char* who = "occ4d_evidence_carve_f32";
  OCC4D_REQUIRE(R >= 0 && R <= INT32_MAX, "%s: R = %lld must be in [0, INT32_MAX]", who, (long long)R);
  OCC4D_REQUIRE(ld_returns >= 3, "%s: ld_returns = %lld must be >= 3", who, (long long)ld_returns);
  OCC4D_REQUIRE(V >= 1 && V <= MAX_SENSORS, "%s: V = %d must be in [1, %d]", who, V, MAX_SENSORS);
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  OCC4D_REQUIRE(fabsf(x0) < INFINITY && fabsf(y0) < INFINITY && fabsf(z0) < INFINITY, "%s: min = (%g, %g, %g) must be finite", who,
                (double)x0, (double)y0, (double)z0);
  OCC4D_REQUIRE(sx > 0.0f && sx < INFINITY && sy > 0.0f && sy < INFINITY && sz > 0.0f && sz < INFINITY,
                "%s: spacing = (%g, %g, %g) must be finite and > 0", who, (double)sx, (double)sy, (double)sz);
  const int64_t n = (int64_t)nx * ny * nz;                        // <= 2^27
  OCC4D_REQUIRE(status, "%s: null status", who);
  OCC4D_REQUIRE(n == 0 || (passed && hits), "%s: null passed / hits with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(R == 0 || returns, "%s: null returns with R = %lld", who, (long long)R);
  OCC4D_REQUIRE(R == 0 || origins, "%s: null origins with V = %d", who, V);
  a = CarveArgs{returns, ld_returns, R, sensor, origins, V, {nx, ny, nz}, {x0, y0, z0}, {sx, sy, sz}, passed, hits, passes, status, n,
                (n + 31) / 32};
  return OCC4D_OK;
}

inline int check_classify(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level, int64_t n,
                          const uint32_t* passed, const int32_t* passes, int min_pass, const int32_t* hits, int32_t* code,
                          int64_t* totals, ClassifyArgs& a) {
  const char* who = "occ4d_evidence_classify_f32";
  OCC4D_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld must be in [0, INT32_MAX]", who, (long long)n);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(!mask || ld_mask >= 1, "%s: ld_mask = %lld must be >= 1", who, (long long)ld_mask);
  OCC4D_REQUIRE(min_pass >= 1, "%s: min_pass = %d must be >= 1", who, min_pass);
  OCC4D_REQUIRE(passes || min_pass == 1, "%s: min_pass = %d needs passes: the bits say only whether a ray passed", who, min_pass);
  OCC4D_REQUIRE(totals, "%s: null totals", who);
  OCC4D_REQUIRE(n == 0 || field, "%s: null field with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(n == 0 || passes || passed, "%s: null passed and null passes with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(n == 0 || (hits && code), "%s: null hits / code with n = %lld", who, (long long)n);
  a = ClassifyArgs{sm::BitsArgs{field, ld, mask, ld_mask, nullptr, n, (n + 31) / 32, level, mask_level}, passed, passes, hits, code, totals,
                   min_pass};
  return OCC4D_OK;
}

}  // namespace occ4d_evidence
