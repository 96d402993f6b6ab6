// The coarse-to-fine decode of the query grid (include/occ4d_refine.h), shared WORD FOR WORD by the HIP kernels
// (csrc/refine.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the block of a point, the representative of a block, hot, the
// clipped neighbourhood, selected, the source row of an expanded row, and the two entry points' argument contracts (host only).
// The squash is track_math.hpp's, the expression of occ4d_squash_f32.
#pragma once
#include <stdint.h>

#include "contract.hpp"
#include "track_math.hpp"

#if defined(__HIPCC__)
#define OCC4D_REFINE_HD __host__ __device__ __forceinline__
#else
#define OCC4D_REFINE_HD inline
#endif

namespace occ4d_refine {

constexpr int TILE = 256;                 // rows per entry of block_offsets: the compaction's tile (csrc/postops.hip)

// the flat grid (x slowest, z fastest) and its blocks of edge b
struct Grid {
  int nx, ny, nz, b;
  int nbx, nby, nbz;
  int64_t n, blocks;
};

OCC4D_REFINE_HD Grid make_grid(int nx, int ny, int nz, int b) {
  Grid g;
  g.nx = nx; g.ny = ny; g.nz = nz; g.b = b;
  g.nbx = (nx + b - 1) / b; g.nby = (ny + b - 1) / b; g.nbz = (nz + b - 1) / b;
  g.n = (int64_t)nx * ny * nz;
  g.blocks = (int64_t)g.nbx * g.nby * g.nbz;
  return g;
}

struct Cell { int x, y, z; };

OCC4D_REFINE_HD Cell point_cell(const Grid& g, int64_t i) {
  return Cell{(int)(i / ((int64_t)g.nz * g.ny)), (int)((i / g.nz) % g.ny), (int)(i % g.nz)};
}
OCC4D_REFINE_HD Cell block_cell(const Grid& g, int64_t blk) {
  return Cell{(int)(blk / ((int64_t)g.nbz * g.nby)), (int)((blk / g.nbz) % g.nby), (int)(blk % g.nbz)};
}
OCC4D_REFINE_HD int64_t block_index(const Grid& g, Cell bc) { return ((int64_t)bc.x * g.nby + bc.y) * g.nbz + bc.z; }

// the block of a point
OCC4D_REFINE_HD Cell block_of(const Grid& g, Cell p) { return Cell{p.x / g.b, p.y / g.b, p.z / g.b}; }

// the representative of a block: per axis min(block * b + b / 2, n_axis - 1)
OCC4D_REFINE_HD int rep_axis(int block, int b, int n_axis) {
  const int c = block * b + b / 2;
  return c < n_axis - 1 ? c : n_axis - 1;
}
OCC4D_REFINE_HD bool is_representative(const Grid& g, Cell p, Cell bc) {
  return p.x == rep_axis(bc.x, g.b, g.nx) && p.y == rep_axis(bc.y, g.b, g.ny) && p.z == rep_axis(bc.z, g.b, g.nz);
}

// hot: NOT (squashed density < low), so a NaN density (and a NaN low) is hot
OCC4D_REFINE_HD bool hot(float raw, int op, float low) { return !(occ4d_track::squash(raw, op) < low); }

OCC4D_REFINE_HD int clip_lo(int c, int d) { return c - d > 0 ? c - d : 0; }
OCC4D_REFINE_HD int clip_hi(int c, int d, int n) { return c + d < n - 1 ? c + d : n - 1; }

struct MarkArgs {
  const float* rep_density; int64_t ld_rep;
  Grid grid;
  int dilate, op;
  float low;
  int32_t* active;
  float* key;
};

// active: any block within Chebyshev distance `dilate`, clipped at the faces, is hot
OCC4D_REFINE_HD int32_t active_of(const MarkArgs& a, int64_t blk) {
  const Grid& g = a.grid;
  const Cell c = block_cell(g, blk);
  for (int x = clip_lo(c.x, a.dilate); x <= clip_hi(c.x, a.dilate, g.nbx); ++x)
    for (int y = clip_lo(c.y, a.dilate); y <= clip_hi(c.y, a.dilate, g.nby); ++y)
      for (int z = clip_lo(c.z, a.dilate); z <= clip_hi(c.z, a.dilate, g.nbz); ++z)
        if (hot(a.rep_density[block_index(g, Cell{x, y, z}) * a.ld_rep], a.op, a.low)) return 1;
  return 0;
}

// selected: the point's block is active and the point is not its representative -> the compaction's keep key
OCC4D_REFINE_HD float key_of(const MarkArgs& a, int64_t i) {
  const Cell p = point_cell(a.grid, i);
  const Cell bc = block_of(a.grid, p);
  return (a.active[block_index(a.grid, bc)] != 0 && !is_representative(a.grid, p, bc)) ? 1.0f : 0.0f;
}

// the compaction's predicate on that key (threshold 0.5, strict)
OCC4D_REFINE_HD bool kept(float key) { return key > 0.5f; }

struct ExpandArgs {
  const float* key;
  const int32_t* block_offsets;
  const float* rep_out; int64_t ld_rep;
  const float* fine_out; int64_t ld_fine;
  int64_t n_fine;
  Grid grid;
  int g;
  float* out; int64_t ld_out;
  int64_t tiles;
};

// the row that grid row i copies: its decoded row when it is selected and its position lies in fine_out, else the row of its
// block's representative.  `pos` is the only value that depends on data, and it is used only inside [0, n_fine).
OCC4D_REFINE_HD const float* source_row(const ExpandArgs& e, int64_t i, bool selected, int64_t pos) {
  if (selected && pos >= 0 && pos < e.n_fine) return e.fine_out + pos * e.ld_fine;
  return e.rep_out + block_index(e.grid, block_of(e.grid, point_cell(e.grid, i))) * e.ld_rep;
}

// ---- argument contracts (host): the status, `empty` = nothing to do, the pass's arguments filled
inline int check_grid(const char* who, int nx, int ny, int nz, int b, Grid& grid) {
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(b >= 2 && b <= 8, "%s: b = %d must be in 2 .. 8", who, b);
  const int64_t plane = (int64_t)nx * ny;
  OCC4D_REQUIRE(nz == 0 || plane == 0 || (plane <= INT32_MAX && plane * nz <= INT32_MAX),
                "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX", who, nx, ny, nz);
  grid = make_grid(nx, ny, nz, b);
  return OCC4D_OK;
}

inline int check_mark(const float* rep_density, int64_t ld_rep, int nx, int ny, int nz, int b, int dilate, int op, float low,
                      int32_t* active, float* key, bool& empty, MarkArgs& a) {
  const char* who = "occ4d_refine_mark_f32";
  Grid grid;
  OCC4D_TRY(check_grid(who, nx, ny, nz, b, grid));
  OCC4D_REQUIRE(dilate >= 0 && dilate <= 2, "%s: dilate = %d must be in 0 .. 2", who, dilate);
  OCC4D_REQUIRE(op >= 0 && op <= 2, "%s: op code %d", who, op);
  OCC4D_REQUIRE(ld_rep >= 1, "%s: ld_rep = %lld must be >= 1", who, (long long)ld_rep);
  empty = grid.n == 0;
  OCC4D_REQUIRE(empty || (rep_density && active && key), "%s: null rep_density / active / key", who);
  a = MarkArgs{rep_density, ld_rep, grid, dilate, op, low, active, key};
  return OCC4D_OK;
}

inline int check_expand(const float* key, const int32_t* block_offsets, const float* rep_out, int64_t ld_rep, const float* fine_out,
                        int64_t ld_fine, int n_fine, int nx, int ny, int nz, int b, int g, float* out, int64_t ld_out, bool& empty,
                        ExpandArgs& e) {
  const char* who = "occ4d_refine_expand_f32";
  Grid grid;
  OCC4D_TRY(check_grid(who, nx, ny, nz, b, grid));
  OCC4D_REQUIRE(g >= 1 && g <= 32, "%s: g = %d: need 1 <= g <= 32", who, g);
  OCC4D_REQUIRE(n_fine >= 0, "%s: n_fine = %d must be >= 0", who, n_fine);
  OCC4D_REQUIRE(ld_rep >= g && ld_fine >= g && ld_out >= g, "%s: ld_rep = %lld, ld_fine = %lld, ld_out = %lld must be >= g = %d", who,
                (long long)ld_rep, (long long)ld_fine, (long long)ld_out, g);
  empty = grid.n == 0;
  OCC4D_REQUIRE(empty || (key && block_offsets && rep_out && out), "%s: null key / block_offsets / rep_out / out", who);
  OCC4D_REQUIRE(empty || n_fine == 0 || fine_out, "%s: null fine_out with n_fine = %d", who, n_fine);
  e = ExpandArgs{key, block_offsets, rep_out, ld_rep, fine_out, ld_fine, (int64_t)n_fine, grid, g, out, ld_out,
                 (grid.n + TILE - 1) / TILE};
  return OCC4D_OK;
}

}  // namespace occ4d_refine
