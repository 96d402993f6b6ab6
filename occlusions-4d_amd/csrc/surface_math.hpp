// The occupancy surface of the query grid as a quad mesh (include/occ4d_surface.h: naive surface nets), shared WORD FOR WORD by
// the HIP kernels (csrc/surface.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): inside, the corner mask of a cell, the quads a
// point's three edges emit, the edge parameter, the vertex accumulation, the quad of an edge, the guarded writes, and the two
// entry points' argument contracts (host only).  Both builds compile with -ffp-contract=off: no expression in here fuses.
#pragma once
#include <stdint.h>

#include "contract.hpp"

#if defined(__HIPCC__)
#define OCC4D_SURFACE_HD __host__ __device__ __forceinline__
#else
#define OCC4D_SURFACE_HD inline
#endif

namespace occ4d_surface {

constexpr int TILE = 256;                 // points per entry of cell_offsets / face_offsets
constexpr int MAX_ATTR = 32;

// the flat grid: n[a] points on axis a, x slowest, z fastest; step[a] = the flat index distance of p and p + e_a
struct Grid {
  int n[3];
  int64_t step[3];
  int64_t points;
};

OCC4D_SURFACE_HD Grid make_grid(int nx, int ny, int nz) {
  Grid g;
  g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  g.step[0] = (int64_t)ny * nz; g.step[1] = nz; g.step[2] = 1;
  g.points = (int64_t)nx * ny * nz;
  return g;
}

struct Point { int c[3]; };

OCC4D_SURFACE_HD Point point_of(const Grid& g, int64_t i) {
  return Point{{(int)(i / g.step[0]), (int)((i / g.n[2]) % g.n[1]), (int)(i % g.n[2])}};
}

struct Field {
  const float* density; int64_t ld;
  Grid grid;
  float level;
};

// inside: a NaN density (and a NaN level) is outside
OCC4D_SURFACE_HD bool inside(float f, float level) { return f >= level; }

// the cell of a point: the one whose low corner it is
OCC4D_SURFACE_HD bool has_cell(const Grid& g, const Point& p) {
  return p.c[0] <= g.n[0] - 2 && p.c[1] <= g.n[1] - 2 && p.c[2] <= g.n[2] - 2;
}

// corner number of a cell: offset o on axis a is bit 2 - a (x = 4, y = 2, z = 1)
OCC4D_SURFACE_HD int corner_bit(int axis) { return 1 << (2 - axis); }
OCC4D_SURFACE_HD int64_t corner_step(const Grid& g, int corner) {
  return (int64_t)((corner >> 2) & 1) * g.step[0] + (int64_t)((corner >> 1) & 1) * g.step[1] + (int64_t)(corner & 1);
}

// the eight corner values of the cell at point i (which has one) and their inside bits
OCC4D_SURFACE_HD unsigned load_corners(const Field& f, int64_t i, float v[8]) {
  unsigned mask = 0;
  for (int corner = 0; corner < 8; ++corner) {
    v[corner] = f.density[(i + corner_step(f.grid, corner)) * f.ld];
    mask |= (inside(v[corner], f.level) ? 1u : 0u) << corner;
  }
  return mask;
}

OCC4D_SURFACE_HD bool crossed(unsigned mask) { return mask != 0u && mask != 0xffu; }

// bit a: the edge p -> p + e_a emits a quad.  Its endpoints differ in `inside` and four cells share it: 1 <= p_b, p_c <= n - 2;
// with p_a <= n_a - 2 that is a point that has a cell, whose mask holds both endpoints.
OCC4D_SURFACE_HD unsigned quad_axes(const Grid& g, const Point& p, unsigned mask) {
  unsigned axes = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    if (((mask ^ (mask >> corner_bit(a))) & 1u) && p.c[b] >= 1 && p.c[c] >= 1) axes |= 1u << a;
  }
  return axes;
}

// what one grid point owns: its cell (mask; 0 when it has none) and the quads of its three edges
struct Item {
  unsigned mask, axes;
};

OCC4D_SURFACE_HD Item item_of(const Field& f, int64_t i, float v[8]) {
  const Point p = point_of(f.grid, i);
  if (!has_cell(f.grid, p)) return Item{0u, 0u};
  const unsigned mask = load_corners(f, i, v);
  return Item{mask, quad_axes(f.grid, p, mask)};
}

OCC4D_SURFACE_HD int quads_of(unsigned axes) { return (int)((axes & 1u) + ((axes >> 1) & 1u) + ((axes >> 2) & 1u)); }

// the edge parameter from the lower-index endpoint (value fl) to the upper one (fu); the fallback takes NaN and +-inf
OCC4D_SURFACE_HD float edge_t(float fl, float fu, float level) {
  float t = (level - fl) / (fu - fl);
  if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
  return t;
}

// the crossed edges of a cell in the header's order (edge e = a * 4 + j * 2 + k), their parameters, their number and the mean
// crossing position in cell units
struct Crossing {
  unsigned edges;
  int k;
  float t[12];
  float u[3];
};

OCC4D_SURFACE_HD void cell_crossing(const float v[8], unsigned mask, float level, Crossing& x) {
  float s[3] = {0.0f, 0.0f, 0.0f};
  x.edges = 0u;
  x.k = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k) {
        const int e = a * 4 + j * 2 + k;
        const int lo = j * corner_bit(b) + k * corner_bit(c), hi = lo + corner_bit(a);
        x.t[e] = 0.5f;
        if (((mask >> lo) ^ (mask >> hi)) & 1u) {
          const float t = edge_t(v[lo], v[hi], level);
          x.t[e] = t;
          x.edges |= 1u << e;
          x.k += 1;
          s[a] += t;
          s[b] += (float)j;
          s[c] += (float)k;
        }
      }
  }
  for (int a = 0; a < 3; ++a) x.u[a] = s[a] / (float)x.k;
}

// one attribute column on the vertex of the cell at point i: `column` = attrs + i * ld_attr + the column
OCC4D_SURFACE_HD float cell_attr(const Crossing& x, const Grid& g, const float* column, int64_t ld_attr) {
  float sum = 0.0f;
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k) {
        const int e = a * 4 + j * 2 + k;
        if (!((x.edges >> e) & 1u)) continue;
        const int lo = j * corner_bit(b) + k * corner_bit(c), hi = lo + corner_bit(a);
        const float al = column[corner_step(g, lo) * ld_attr], au = column[corner_step(g, hi) * ld_attr];
        sum += al + x.t[e] * (au - al);
      }
  }
  return sum / (float)x.k;
}

// the grid's own expression (occ4d_grid_points_f32) with the offset added
OCC4D_SURFACE_HD float world(int c, float u, float spacing, float origin) { return (((float)c + 0.5f) + u) * spacing + origin; }

struct CountArgs {
  Field f;
  int32_t* cell_offsets;
  int32_t* face_offsets;
  int32_t* totals;
  int64_t tiles;
};

struct WriteArgs {
  Field f;
  const float* attrs; int64_t ld_attr;
  int n_attr;
  float origin[3], spacing[3];
  const int32_t* cell_offsets;
  const int32_t* face_offsets;
  int32_t* work;
  float* vertices; int64_t ld_v;
  int64_t vertex_cap;
  int32_t* faces;
  int64_t face_cap;
  int64_t tiles;
};

// the vertex pass at point i: its cell's vertex number into work (-1: none), and the vertex row when the number lies inside
// the array -- `number` (the tile's offset + the rank in the tile) is the only value that depends on the offsets
OCC4D_SURFACE_HD void vertex_item(const WriteArgs& w, int64_t i, const Item& it, const float v[8], int64_t number) {
  if (!crossed(it.mask)) {
    w.work[i] = -1;
    return;
  }
  w.work[i] = (int32_t)number;
  if (number < 0 || number >= w.vertex_cap) return;
  const Point p = point_of(w.f.grid, i);
  Crossing x;
  cell_crossing(v, it.mask, w.f.level, x);
  float* row = w.vertices + number * w.ld_v;
  for (int a = 0; a < 3; ++a) row[a] = world(p.c[a], x.u[a], w.spacing[a], w.origin[a]);
  for (int col = 0; col < w.n_attr; ++col) row[3 + col] = cell_attr(x, w.f.grid, w.attrs + i * w.ld_attr + col, w.ld_attr);
}

// the quad of the edge i -> i + e_a (quad_axes has bit a): the cells p + (db, dc), (-1,-1), (0,-1), (0,0), (-1,0), reversed when
// p is outside, written only inside the array
OCC4D_SURFACE_HD void quad_item(const WriteArgs& w, int64_t i, int a, bool p_inside, int64_t number) {
  if (number < 0 || number >= w.face_cap) return;
  const int64_t sb = w.f.grid.step[(a + 1) % 3], sc = w.f.grid.step[(a + 2) % 3];
  const int32_t q0 = w.work[i - sb - sc], q1 = w.work[i - sc], q2 = w.work[i], q3 = w.work[i - sb];
  int32_t* face = w.faces + number * 4;
  if (p_inside) {
    face[0] = q0; face[1] = q1; face[2] = q2; face[3] = q3;
  } else {
    face[0] = q3; face[1] = q2; face[2] = q1; face[3] = q0;
  }
}

// the face pass at point i: its up to three quads from `number` on, axis order
OCC4D_SURFACE_HD void face_item(const WriteArgs& w, int64_t i, const Item& it, int64_t number) {
  for (int a = 0; a < 3; ++a)
    if ((it.axes >> a) & 1u) quad_item(w, i, a, (it.mask & 1u) != 0u, number++);
}

// ---- argument contracts (host): the status, `empty` = nothing to do, the pass's arguments filled
inline int check_field(const char* who, const float* density, int64_t ld, int nx, int ny, int nz, float level, Field& f) {
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  const int64_t plane = (int64_t)nx * ny, limit = INT32_MAX / 3;
  OCC4D_REQUIRE(nz == 0 || plane == 0 || (plane <= limit && plane * nz <= limit),
                "%s: 3 * nx * ny * nz = 3 * %d * %d * %d exceeds INT32_MAX", who, nx, ny, nz);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  f = Field{density, ld, make_grid(nx, ny, nz), level};
  return OCC4D_OK;
}

inline int check_count(const float* density, int64_t ld, int nx, int ny, int nz, float level, int32_t* cell_offsets,
                       int32_t* face_offsets, int32_t* totals, bool& empty, CountArgs& a) {
  const char* who = "occ4d_surface_count_f32";
  Field f;
  OCC4D_TRY(check_field(who, density, ld, nx, ny, nz, level, f));
  empty = f.grid.points == 0;
  OCC4D_REQUIRE(empty || (density && cell_offsets && face_offsets && totals), "%s: null density / cell_offsets / face_offsets / totals",
                who);
  a = CountArgs{f, cell_offsets, face_offsets, totals, (f.grid.points + TILE - 1) / TILE};
  return OCC4D_OK;
}

inline int check_write(const float* density, int64_t ld, const float* attrs, int64_t ld_attr, int n_attr, int nx, int ny, int nz,
                       float level, float x0, float sx, float y0, float sy, float z0, float sz, const int32_t* cell_offsets,
                       const int32_t* face_offsets, int32_t* work, float* vertices, int64_t ld_v, int vertex_cap, int32_t* faces,
                       int face_cap, bool& empty, WriteArgs& w) {
  const char* who = "occ4d_surface_write_f32";
  Field f;
  OCC4D_TRY(check_field(who, density, ld, nx, ny, nz, level, f));
  OCC4D_REQUIRE(n_attr >= 0 && n_attr <= MAX_ATTR, "%s: n_attr = %d: need 0 <= n_attr <= %d", who, n_attr, MAX_ATTR);
  OCC4D_REQUIRE(ld_attr >= n_attr && ld_v >= 3 + n_attr, "%s: ld_attr = %lld must be >= n_attr = %d and ld_v = %lld >= 3 + n_attr", who,
                (long long)ld_attr, n_attr, (long long)ld_v);
  OCC4D_REQUIRE(vertex_cap >= 0 && face_cap >= 0, "%s: vertex_cap = %d, face_cap = %d must be >= 0", who, vertex_cap, face_cap);
  empty = f.grid.points == 0;
  OCC4D_REQUIRE(empty || (density && cell_offsets && face_offsets && work), "%s: null density / cell_offsets / face_offsets / work", who);
  OCC4D_REQUIRE(empty || n_attr == 0 || attrs, "%s: null attrs with n_attr = %d", who, n_attr);
  OCC4D_REQUIRE(empty || ((vertex_cap == 0 || vertices) && (face_cap == 0 || faces)), "%s: null vertices / faces with vertex_cap = %d, face_cap = %d",
                who, vertex_cap, face_cap);
  w = WriteArgs{f, attrs, ld_attr, n_attr, {x0, y0, z0}, {sx, sy, sz}, cell_offsets, face_offsets, work, vertices, ld_v,
                (int64_t)vertex_cap, faces, (int64_t)face_cap, (f.grid.points + TILE - 1) / TILE};
  return OCC4D_OK;
}

}  // namespace occ4d_surface
