// Line of sight through the grid's solid set (include/ext/occ4d_sight.h), shared WORD FOR WORD by the HIP kernels (csrc/sight.hip)
// and the g++ twin (csrc_cpu/occ4d_twin.cpp): the member test, the bit test with its in-grid guard, the choice of T, the SQUEEZE, the
// walk, the body of a query, the blocks of queries and the two argument contracts (host only).  Integers only; the float operations
// are the >= comparisons of member().
#pragma once
#include <stdint.h>

#include "ext/occ4d_sight.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_sight {

constexpr int MAX_AXIS = OCC4D_SIGHT_MAX_AXIS;
constexpr int MAX_ORIGINS = OCC4D_SIGHT_MAX_ORIGINS;
constexpr int MAX_COORD = OCC4D_SIGHT_MAX_COORD;
constexpr int BX = OCC4D_SIGHT_BLOCK_X, BY = OCC4D_SIGHT_BLOCK_Y, BZ = OCC4D_SIGHT_BLOCK_Z;
static_assert(BX * BY * BZ == 64, "a wave owns one block of queries");
static_assert(MAX_ORIGINS <= 31, "one bit of an int32 per origin, the sign bit free");
// the walk's terms: (2 j + 1) * m with j < m <= MAX_COORD + MAX_AXIS stays below 2^43

struct BitsArgs {
  const float* field; int64_t ld;
  const float* mask; int64_t ld_mask;
  uint32_t* bits;
  int64_t n, words;
  float level, mask_level;
};

struct Args {
  const uint32_t* bits;
  const int32_t* framed;                                          // null: every origin frames every query
  int32_t *seen, *blocker;                                        // blocker: null = not computed
  int n[3], b[3];                                                 // nx, ny, nz;  blocks of queries along each axis
  int V;
  int64_t points, blocks;
  int32_t origin[MAX_ORIGINS][3];                                 // by value: range-checked on the host
};

// ---- the rules
OCC4D_HD bool member(const BitsArgs& a, int64_t p) {
  bool m = a.field[p * a.ld] >= a.level;
  if (m && a.mask) m = a.mask[p * a.ld_mask] >= a.mask_level;
  return m;
}

// The bit test.  words(i) -> word i of bits.  A cell outside the grid is free and reads nothing:
// the index is formed only after the three range tests.  flat: the cell's flat index where it is inside.
template <class Words>
OCC4D_HD bool solid_at(const int* n, const Words& words, int x, int y, int z, bool& inside, int32_t& flat) {
  inside = (unsigned)x < (unsigned)n[0] && (unsigned)y < (unsigned)n[1] && (unsigned)z < (unsigned)n[2];
  if (!inside) return false;
  flat = (x * n[1] + y) * n[2] + z;
  return (words(flat >> 5) >> (flat & 31)) & 1u;
}

// ... of a side cell of the SQUEEZE: whether it is solid; `low` becomes the lowest flat index of the solid ones so far
template <class Words>
OCC4D_HD bool squeeze_cell(const int* n, const Words& words, int x, int y, int z, int32_t& low) {
  bool inside;
  int32_t flat = 0;
  const bool solid = solid_at(n, words, x, y, z, inside, flat);
  if (solid && flat < low) low = flat;
  return solid;
}

// THE WALK from the query (qx, qy, qz) to the origin (ox, oy, oz) -> -1: seen;  else the blocker's flat index.
// The comparison t_a < t_b of the header is pab < pba with pab = (2 j_a + 1) * m_b, pba = (2 j_b + 1) * m_a: six 64-bit terms
// that GROW BY ADDITIONS, pab by 2 m_b with every step of axis a; no product in the loop.  An axis that is not live never attains
// the minimum: with m_a = 0 its pab is 0 against pba = m_b > 0 from the start; one that has arrived has t_a > 1, every live t < 1.
// So T is the live axes that no axis beats, and live is c_a != o_a: no counters.
template <class Words>
OCC4D_HD int32_t walk(const int* n, const Words& words, int qx, int qy, int qz, int ox, int oy, int oz) {
  int cx = qx, cy = qy, cz = qz;
  const int sx = ox > qx ? 1 : -1, sy = oy > qy ? 1 : -1, sz = oz > qz ? 1 : -1;      // (the sign of a dead axis is never used)
  const int64_t mx = ox > qx ? (int64_t)ox - qx : (int64_t)qx - ox, my = oy > qy ? (int64_t)oy - qy : (int64_t)qy - oy,
                mz = oz > qz ? (int64_t)oz - qz : (int64_t)qz - oz;
  int64_t pxy = my, pyx = mx, pxz = mz, pzx = mx, pyz = mz, pzy = my;                 // j = 0: (2 j + 1) = 1
  const int bound = n[0] + n[1] + n[2];
  for (int step = 0; step < bound; ++step) {
    const bool tx = cx != ox && !(pyx < pxy) && !(pzx < pxz);
    const bool ty = cy != oy && !(pxy < pyx) && !(pzy < pyz);
    const bool tz = cz != oz && !(pxz < pzx) && !(pyz < pzy);
    if (!(tx || ty || tz)) return -1;                                                 // c == o: q == o
    const int ax = cx + sx, ay = cy + sy, az = cz + sz;
    if (tx && ty && tz) {                                                             // SQUEEZE through a corner
      int32_t low = INT32_MAX;
      const bool X = squeeze_cell(n, words, ax, cy, cz, low), Y = squeeze_cell(n, words, cx, ay, cz, low),
                 Z = squeeze_cell(n, words, cx, cy, az, low), XY = squeeze_cell(n, words, ax, ay, cz, low),
                 XZ = squeeze_cell(n, words, ax, cy, az, low), YZ = squeeze_cell(n, words, cx, ay, az, low);
      const bool pass = (!X && (!XY || !XZ)) || (!Y && (!XY || !YZ)) || (!Z && (!XZ || !YZ));
      if (!pass) return low;
    } else if ((int)tx + (int)ty + (int)tz == 2) {                                    // ... an edge: the two side cells
      int32_t low = INT32_MAX;
      const bool A = tx ? squeeze_cell(n, words, ax, cy, cz, low) : squeeze_cell(n, words, cx, ay, cz, low);
      const bool B = tz ? squeeze_cell(n, words, cx, cy, az, low) : squeeze_cell(n, words, cx, ay, cz, low);
      if (A && B) return low;
    }
    if (tx) { cx = ax; pxy += 2 * my; pxz += 2 * mz; }
    if (ty) { cy = ay; pyx += 2 * mx; pyz += 2 * mz; }
    if (tz) { cz = az; pzx += 2 * mx; pzy += 2 * my; }
    if (cx == ox && cy == oy && cz == oz) return -1;                                  // o itself is never tested
    bool inside;
    int32_t flat = 0;
    const bool solid = solid_at(n, words, cx, cy, cz, inside, flat);
    if (!inside) return -1;                                                           // the grid is convex
    if (solid) return flat;
  }
  return -1;                                                                          // (not reached: the header's bound)
}

// ---- the blocks of queries: block k of b[0] * b[1] * b[2], z fastest; the query of lane l of its wave, whether the grid has it
OCC4D_HD bool block_query(const Args& a, int64_t k, int lane, int& x, int& y, int& z) {
  const int kz = (int)(k % a.b[2]), ky = (int)(k / a.b[2] % a.b[1]), kx = (int)(k / ((int64_t)a.b[2] * a.b[1]));
  x = kx * BX + lane / (BY * BZ);
  y = ky * BY + lane / BZ % BY;
  z = kz * BZ + lane % BZ;
  return x < a.n[0] && y < a.n[1] && z < a.n[2];
}

// the body of the query (x, y, z) of the grid: its bits gathered in a register, one store per output
template <class Words>
OCC4D_HD void query_item(const Args& a, const Words& words, int x, int y, int z) {
  const int64_t p = ((int64_t)x * a.n[1] + y) * a.n[2] + z;
  const int32_t framed = a.framed ? a.framed[p] : -1;
  int32_t seen = 0;
  for (int v = 0; v < a.V; ++v) {
    int32_t blocker = -1;
    if ((framed >> v) & 1) {
      blocker = walk(a.n, words, x, y, z, a.origin[v][0], a.origin[v][1], a.origin[v][2]);
      if (blocker < 0) seen |= (int32_t)1 << v;
    }
    if (a.blocker) a.blocker[(int64_t)v * a.points + p] = blocker;
  }
  a.seen[p] = seen;
}

struct GlobalWords {
  const uint32_t* bits;
  OCC4D_HD uint32_t operator()(int32_t i) const { return bits[i]; }
};

// ---- the argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_bits(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level, int64_t n,
                      uint32_t* bits, bool& empty, BitsArgs& a) {
  const char* who = "occ4d_sight_bits_f32";
  OCC4D_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld must be in [0, INT32_MAX]", who, (long long)n);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(!mask || ld_mask >= 1, "%s: ld_mask = %lld must be >= 1", who, (long long)ld_mask);
  empty = n == 0;
  OCC4D_REQUIRE(empty || field, "%s: null field with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(empty || bits, "%s: null bits with n = %lld", who, (long long)n);
  a = BitsArgs{field, ld, mask, ld_mask, bits, n, (n + 31) / 32, level, mask_level};
  return OCC4D_OK;
}

inline int check_grid(const uint32_t* bits, int nx, int ny, int nz, const int32_t* origins_host, int V, const int32_t* framed,
                      int32_t* seen, int32_t* blocker, int flags, bool& empty, Args& a) {
  const char* who = "occ4d_sight_grid_u32";
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  OCC4D_REQUIRE(V >= 1 && V <= MAX_ORIGINS, "%s: V = %d must be in [1, %d]", who, V, MAX_ORIGINS);
  OCC4D_REQUIRE(flags == 0, "%s: flags = %d must be 0: no flag bit exists", who, flags);
  const int64_t n = (int64_t)nx * ny * nz;                        // <= 2^27
  empty = n == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(bits, "%s: null bits with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(seen, "%s: null seen with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(origins_host, "%s: null origins_host with V = %d", who, V);
  a = Args{};
  a.bits = bits, a.framed = framed, a.seen = seen, a.blocker = blocker;
  a.n[0] = nx, a.n[1] = ny, a.n[2] = nz;
  a.b[0] = (nx + BX - 1) / BX, a.b[1] = (ny + BY - 1) / BY, a.b[2] = (nz + BZ - 1) / BZ;
  a.V = V, a.points = n, a.blocks = (int64_t)a.b[0] * a.b[1] * a.b[2];
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k) {
      const int32_t c = origins_host[v * 3 + k];
      OCC4D_REQUIRE(c >= -MAX_COORD && c <= MAX_COORD, "%s: origin %d = (%d, %d, %d) has a coordinate outside [-%d, %d]", who, v,
                    origins_host[v * 3], origins_host[v * 3 + 1], origins_host[v * 3 + 2], MAX_COORD, MAX_COORD);
      a.origin[v][k] = c;
    }
  return OCC4D_OK;
}

}  // namespace occ4d_sight
