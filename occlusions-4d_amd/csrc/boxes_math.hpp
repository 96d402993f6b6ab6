// Oriented boxes of the labelled objects (include/ext/occ4d_boxes.h), shared WORD FOR WORD by the HIP kernels (csrc/boxes.hip) and
// the g++ twin (csrc_cpu/occ4d_twin.cpp): the DEAD test, the two projections, the EMPTY rows, the qualification test and the
// (area, a) order of CHOICE, the row a choice writes, and the two argument contracts (host only).  Integers only.
#pragma once
#include <stdint.h>

#include "ext/occ4d_boxes.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_boxes {

constexpr int MAX_AXIS = OCC4D_BOXES_MAX_AXIS;
constexpr int MAX_DIRS = OCC4D_BOXES_MAX_DIRS;
constexpr int MAX_COEF = OCC4D_BOXES_MAX_COEF;
constexpr int COLS = OCC4D_BOXES_COLS;
constexpr int TILE = OCC4D_BOXES_TILE;
constexpr int SLOTS = OCC4D_BOXES_GATHER_SLOTS;
constexpr int PROBES = OCC4D_BOXES_GATHER_PROBES;
constexpr int64_t MAX_WIDTH = (int64_t)1 << 30;                   // a qualifying extent has 0 <= max - min < MAX_WIDTH
static_assert(2ll * MAX_COEF * (MAX_AXIS - 1) < (1ll << 28), "|u|, |v| < 2^28");
static_assert(PROBES <= SLOTS, "a probe sequence visits no slot twice");

struct ExtentArgs {
  const int32_t *labels, *dirs;
  int32_t *extent, *zr;
  int n[3];
  int K, A;
};

struct ChooseArgs {
  const int32_t *extent, *zr, *dirs;
  int32_t* box;
  int K, A;
};

// ---- DIRECTIONS
struct Dir {
  int32_t ax, ay, bx, by;
  bool live;
};

OCC4D_HD bool coef_ok(int32_t c) { return c >= -MAX_COEF && c <= MAX_COEF; }

// Row a of the table: DEAD when a coefficient lies outside [-MAX_COEF, MAX_COEF] -- tested before any of them is used; a DEAD
// row's coefficients are 0 from here on.
OCC4D_HD Dir dir_at(const int32_t* dirs, int a) {
  const int32_t ax = dirs[4 * a], ay = dirs[4 * a + 1], bx = dirs[4 * a + 2], by = dirs[4 * a + 3];
  if (coef_ok(ax) && coef_ok(ay) && coef_ok(bx) && coef_ok(by)) return Dir{ax, ay, bx, by, true};
  return Dir{0, 0, 0, 0, false};
}

OCC4D_HD int32_t along(const Dir& d, int ix, int iy) { return d.ax * ix + d.ay * iy; }
OCC4D_HD int32_t across(const Dir& d, int ix, int iy) { return d.bx * ix + d.by * iy; }

// ---- EXTENTS and RANGE.  Word c of an EMPTY row of extent: [INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN]; of zr: [.., .., 0]
OCC4D_HD int32_t empty_extent(int c) { return (c & 1) ? INT32_MIN : INT32_MAX; }
OCC4D_HD int32_t empty_zr(int c) { return c == 0 ? INT32_MAX : c == 1 ? INT32_MIN : 0; }

// ... whether a label names an object
OCC4D_HD bool object_of(int32_t label, int K) { return label >= 0 && label < K; }

// ---- CHOICE
// ... whether the row [min u, max u, min v, max v] of a live direction takes part: 0 <= max - min < 2^30 on both axes
OCC4D_HD bool qualifies(const int32_t* e) {
  const int64_t du = (int64_t)e[1] - e[0], dv = (int64_t)e[3] - e[2];
  return du >= 0 && du < MAX_WIDTH && dv >= 0 && dv < MAX_WIDTH;
}

OCC4D_HD int64_t abs64(int32_t c) { return c < 0 ? -(int64_t)c : (int64_t)c; }

// the area of a qualifying row's rectangle: each side covers the cells, not just their centres
OCC4D_HD int64_t area_of(const Dir& d, const int32_t* e) {
  const int64_t w1 = (int64_t)e[1] - e[0] + abs64(d.ax) + abs64(d.ay), w2 = (int64_t)e[3] - e[2] + abs64(d.bx) + abs64(d.by);
  return w1 * w2;
}

constexpr int64_t NO_AREA = INT64_MAX;                            // the key of a direction that does not qualify; a = -1 with it
struct Key {
  int64_t area;
  int a;
};

// direction a's key for object k: (area, a), or (NO_AREA, -1)
OCC4D_HD Key key_of(const ChooseArgs& c, int k, int a) {
  const Dir d = dir_at(c.dirs, a);
  const int32_t* e = c.extent + ((int64_t)k * c.A + a) * 4;
  if (!d.live || !qualifies(e)) return Key{NO_AREA, -1};
  return Key{area_of(d, e), a};
}

// the (area, a) order: the least area, among equal areas THE LOWEST a; a key that does not qualify loses to every one that does
OCC4D_HD Key better(const Key& x, const Key& y) {
  const bool take = y.a >= 0 && (x.a < 0 || y.area < x.area || (y.area == x.area && y.a < x.a));
  return Key{take ? y.area : x.area, take ? y.a : x.a};
}

// row k of box from the best key over the directions
OCC4D_HD void write_box(const ChooseArgs& c, int k, const Key& best) {
  int32_t* row = c.box + (int64_t)k * COLS;
  const int32_t* z = c.zr + (int64_t)k * 3;
  const int32_t points = z[2];
  if (points <= 0) {
    row[0] = -1;
    for (int i = 1; i < COLS; ++i) row[i] = 0;
    return;
  }
  const bool found = best.a >= 0 && best.a < c.A;
  const int32_t* e = c.extent + ((int64_t)k * c.A + (found ? best.a : 0)) * 4;
  row[0] = found ? best.a : -1;
  for (int i = 0; i < 4; ++i) row[1 + i] = found ? e[i] : 0;
  row[5] = z[0], row[6] = z[1], row[7] = points;
}

// ---- the argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_sizes(const char* who, int K, int A) {
  OCC4D_REQUIRE(K >= 0, "%s: K = %d must be >= 0", who, K);
  OCC4D_REQUIRE(A >= 1 && A <= MAX_DIRS, "%s: A = %d must be in [1, %d]", who, A, MAX_DIRS);
  OCC4D_REQUIRE((int64_t)K * A * 4 <= INT32_MAX, "%s: K * A * 4 = %d * %d * 4 exceeds INT32_MAX", who, K, A);
  return OCC4D_OK;
}

inline int check_extents(const int32_t* labels, int nx, int ny, int nz, int K, const int32_t* dirs, int A, int32_t* extent,
                         int32_t* zr, bool& empty, ExtentArgs& a) {
  const char* who = "occ4d_boxes_extents_i32";
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  const int64_t n = (int64_t)nx * ny * nz;                        // <= 2^33
  OCC4D_REQUIRE(n <= INT32_MAX, "%s: nx * ny * nz = %lld exceeds INT32_MAX", who, (long long)n);
  OCC4D_TRY(check_sizes(who, K, A));
  empty = K == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(labels || n == 0, "%s: null labels with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(dirs, "%s: null dirs with A = %d", who, A);
  OCC4D_REQUIRE(extent, "%s: null extent with K = %d, A = %d", who, K, A);
  OCC4D_REQUIRE(zr, "%s: null zr with K = %d", who, K);
  a = ExtentArgs{labels, dirs, extent, zr, {nx, ny, nz}, K, A};
  return OCC4D_OK;
}

inline int check_choose(const int32_t* extent, const int32_t* zr, const int32_t* dirs, int K, int A, int32_t* box, bool& empty,
                        ChooseArgs& a) {
  const char* who = "occ4d_boxes_choose_i32";
  OCC4D_TRY(check_sizes(who, K, A));
  empty = K == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(extent, "%s: null extent with K = %d, A = %d", who, K, A);
  OCC4D_REQUIRE(zr, "%s: null zr with K = %d", who, K);
  OCC4D_REQUIRE(dirs, "%s: null dirs with A = %d", who, A);
  OCC4D_REQUIRE(box, "%s: null box with K = %d", who, K);
  a = ChooseArgs{extent, zr, dirs, box, K, A};
  return OCC4D_OK;
}

}  // namespace occ4d_boxes
