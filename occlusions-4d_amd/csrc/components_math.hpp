// The connected components of the grid's solid set (include/ext/occ4d_components.h), shared WORD FOR WORD by the HIP kernels
// (csrc/components.hip), the g++ twin (csrc_cpu/occ4d_twin.cpp) and the threaded host check (profiles/micro/components_threads.cpp):
// the member test, the neighbour enumeration, find and unite, the item bodies of the passes and the two argument contracts (host
// only).  Integers only; the float operations are the >= comparisons of member().
//
// find and unite are templates over A, HOW THE ATOMIC IS SPELLED: A::load(ptr) is a relaxed atomic load and A::fetch_min(ptr, v) a
// relaxed atomic minimum that returns the value before it -- agent scope in the border pass, workgroup scope on LDS in the local
// pass, plain memory in the twin, std::atomic_ref in the threaded host check.
#pragma once
#include <stdint.h>

#include "ext/occ4d_components.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_components {

constexpr int COLS = OCC4D_COMPONENTS_COLS;
constexpr int TILE = OCC4D_COMPONENTS_TILE;                       // numbering tile: consecutive flat indices
constexpr int TX = OCC4D_COMPONENTS_TILE_X, TY = OCC4D_COMPONENTS_TILE_Y, TZ = OCC4D_COMPONENTS_TILE_Z;
constexpr int TILE_POINTS = TX * TY * TZ;                         // the local pass: one thread per point of a TX x TY x TZ tile
constexpr int BACKWARD = 13;                                      // neighbours with a lower flat index
static_assert(TILE_POINTS <= 256, "the local pass runs one 256-thread workgroup per tile");

struct Grid {
  int n[3];                                                       // nx, ny, nz
  int tiles[3];                                                   // local tiles per axis
  int64_t points, local_tiles, number_tiles;
};

struct LabelArgs {
  const float* field; int64_t ld;
  const float* mask; int64_t ld_mask;
  const int32_t* klass;
  int32_t *parent, *root, *size;                                  // work: n each
  int32_t *kept_roots, *kept_points, *all_roots;                  // work: number_tiles each
  int32_t *labels, *totals;
  Grid grid;
  float level, mask_level;
  int rank;                                                       // 1, 2, 3: the most axes two neighbours differ on
  int min_size;
};

struct TableArgs {
  const int32_t* labels; const int32_t* klass; const int32_t* totals;
  int64_t* table;
  Grid grid;
  int cap;
};

// ---- the rules
OCC4D_HD bool member(const LabelArgs& a, int64_t p) {
  if (!(a.field[p * a.ld] >= a.level)) return false;
  if (a.mask && !(a.mask[p * a.ld_mask] >= a.mask_level)) return false;
  return !a.klass || a.klass[p] >= 0;
}

// what two adjacent members must share: the class, 0 without classes; -1 for a non-member
OCC4D_HD int key_of(const LabelArgs& a, int64_t p, bool is_member) { return !is_member ? -1 : a.klass ? a.klass[p] : 0; }

// backward neighbour c = 0 .. 12: the offsets (dx, dy, dz) in {-1, 0, 1}^3 in front of (0, 0, 0) in raster order, which are
// exactly those towards a lower flat index; whether it counts at this connectivity
OCC4D_HD bool backward_offset(int c, int rank, int* d) {
  d[0] = c / 9 - 1;
  d[1] = (c / 3) % 3 - 1;
  d[2] = c % 3 - 1;
  return (d[0] != 0) + (d[1] != 0) + (d[2] != 0) <= rank;
}

OCC4D_HD void coords_of(const Grid& g, int64_t p, int* i) {
  i[2] = (int)(p % g.n[2]);
  i[1] = (int)((p / g.n[2]) % g.n[1]);
  i[0] = (int)(p / ((int64_t)g.n[1] * g.n[2]));
}

OCC4D_HD int64_t flat_of(const Grid& g, const int* i) { return ((int64_t)i[0] * g.n[1] + i[1]) * g.n[2] + i[2]; }

// ---- union-find.  INVARIANT: parent[x] <= x, and parent[x] is a point of x's component; a root has parent[x] == x.
// The loop ends because x strictly decreases: a loaded parent is x itself (return) or lower, and x >= 0.  A stale load returns an
// earlier parent of x, which is an ancestor-or-self of x just the same: find then returns SOME ancestor, never a foreign point.
template <class A>
OCC4D_HD int find(int32_t* parent, int x) {
  for (;;) {
    const int up = A::load(parent + x);
    if (up >= x || up < 0) return x;                              // (== x: a root.  > x or < 0 is never stored for a member; it ends
                                                                  //  the loop too, so no value can carry an index out of the array)
    x = up;
  }
}

// Joins the components of x and y.  Each round takes the two ancestors hi > lo and links hi to lo with an atomic minimum; THE
// VALUE THE ATOMIC RETURNS decides: == hi means hi was a root at that instant and now hangs under lo (done); anything else is the
// parent another thread gave hi in the meantime (lower than hi), and since the minimum may have replaced that link by lo, the round
// is repeated for (that parent, lo), which restores it.
// The loop ends because hi + lo strictly decreases: find never raises either, and a round that does not return replaces hi by a
// value below it; both stay >= 0.
template <class A>
OCC4D_HD void unite(int32_t* parent, int x, int y) {
  for (;;) {
    x = find<A>(parent, x);
    y = find<A>(parent, y);
    if (x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    const int before = A::fetch_min(parent + hi, lo);
    if (before >= hi || before < 0) return;                       // (< 0 is never stored for a member: see find)
    x = before;
    y = lo;
  }
}

struct Plain {                                                    // one thread: the twin, and the passes that only read
  static OCC4D_HD int load(const int32_t* p) { return *p; }
  static OCC4D_HD int fetch_min(int32_t* p, int v) {
    const int before = *p;
    if (v < before) *p = v;
    return before;
  }
};

// ---- pass 1, the local labelling of tile (tx, ty, tz): thread t = (lx * TY + ly) * TZ + lz of the tile.  Local order = flat
// order within a tile, so the lowest local index of a local component is its lowest flat index.
struct LocalPoint {
  int l[3];                                                       // coordinates in the tile
  int64_t p;                                                      // flat index, -1 outside the grid
};

OCC4D_HD LocalPoint local_point(const Grid& g, int64_t tile, int t) {
  LocalPoint q;
  const int tz = (int)(tile % g.tiles[2]), ty = (int)((tile / g.tiles[2]) % g.tiles[1]);
  const int tx = (int)(tile / ((int64_t)g.tiles[1] * g.tiles[2]));
  q.l[0] = t / (TY * TZ);
  q.l[1] = (t / TZ) % TY;
  q.l[2] = t % TZ;
  const int i[3] = {tx * TX + q.l[0], ty * TY + q.l[1], tz * TZ + q.l[2]};
  q.p = t < TILE_POINTS && i[0] < g.n[0] && i[1] < g.n[1] && i[2] < g.n[2] ? flat_of(g, i) : -1;
  return q;
}

// step 1 (then a barrier): the thread's own cell of the tile's parent and key arrays, and its point's zeroed size
OCC4D_HD void local_init(const LabelArgs& a, const LocalPoint& q, int t, int32_t* s_parent, int32_t* s_key) {
  const bool m = q.p >= 0 && member(a, q.p);
  s_parent[t] = m ? t : -1;
  s_key[t] = q.p >= 0 ? key_of(a, q.p, m) : -1;
  if (q.p >= 0) a.size[q.p] = 0;
}

// step 2 (then a barrier): the point joined with its backward neighbours inside the tile.  (A neighbour inside the tile's box whose
// point lies outside the grid has key -1.)
template <class A>
OCC4D_HD void local_link(const LabelArgs& a, const LocalPoint& q, int t, int32_t* s_parent, const int32_t* s_key) {
  const int key = s_key[t];
  if (key < 0) return;
  for (int c = 0; c < BACKWARD; ++c) {
    int d[3];
    if (!backward_offset(c, a.rank, d)) continue;
    const int lx = q.l[0] + d[0], ly = q.l[1] + d[1], lz = q.l[2] + d[2];
    if (lx < 0 || ly < 0 || lz < 0 || ly >= TY || lz >= TZ) continue;          // (lx <= l[0] < TX)
    const int u = (lx * TY + ly) * TZ + lz;
    if (s_key[u] == key) unite<A>(s_parent, t, u);
  }
}

// step 3: the flat index of the point's local root into parent[], -1 for a non-member
template <class A>
OCC4D_HD void local_write(const LabelArgs& a, const Grid& g, int64_t tile, const LocalPoint& q, int t, int32_t* s_parent) {
  if (q.p < 0) return;
  int32_t up = -1;
  if (s_parent[t] >= 0) up = (int32_t)local_point(g, tile, find<A>(s_parent, t)).p;
  a.parent[q.p] = up;
}

// ---- pass 2, the border merge of point p: unite with every backward neighbour in ANOTHER tile (those in its own tile are joined
// already).  parent[q] < 0 marks a non-member since pass 1 and never changes sign.  border_pairs hands each such pair to `each`.
template <class A, class F>
OCC4D_HD void border_pairs(const LabelArgs& a, int64_t p, F&& each) {
  if (A::load(a.parent + p) < 0) return;
  const int key = key_of(a, p, true);
  int i[3];
  coords_of(a.grid, p, i);
  for (int c = 0; c < BACKWARD; ++c) {
    int d[3];
    if (!backward_offset(c, a.rank, d)) continue;
    const int j[3] = {i[0] + d[0], i[1] + d[1], i[2] + d[2]};
    if (j[0] < 0 || j[1] < 0 || j[2] < 0 || j[1] >= a.grid.n[1] || j[2] >= a.grid.n[2]) continue;      // (j[0] <= i[0] < nx)
    if (j[0] / TX == i[0] / TX && j[1] / TY == i[1] / TY && j[2] / TZ == i[2] / TZ) continue;
    const int64_t q = flat_of(a.grid, j);
    if (A::load(a.parent + q) < 0 || key_of(a, q, true) != key) continue;
    each((int)p, (int)q);
  }
}

template <class A>
OCC4D_HD void border_item(const LabelArgs& a, int64_t p) {
  border_pairs<A>(a, p, [&a](int x, int y) { unite<A>(a.parent, x, y); });
}

// ---- pass 3, flatten: the root of p (-1 for a non-member) into root[]; the caller adds the point to size[root]
OCC4D_HD int flatten_item(const LabelArgs& a, int64_t p) {
  const int r = a.parent[p] < 0 ? -1 : find<Plain>(a.parent, (int)p);
  a.root[p] = r;
  return r;
}

// ---- pass 4, numbering.  What point p adds to its tile's three counts:
OCC4D_HD bool is_root(const LabelArgs& a, int64_t p) { return a.root[p] == (int32_t)p; }
OCC4D_HD bool is_kept_root(const LabelArgs& a, int64_t p) { return is_root(a, p) && a.size[p] >= a.min_size; }
OCC4D_HD bool is_kept_point(const LabelArgs& a, int64_t p) { return a.root[p] >= 0 && a.size[a.root[p]] >= a.min_size; }
// ... a kept root's number goes into parent[root] (free since pass 3), and then every point's label:
OCC4D_HD void label_item(const LabelArgs& a, int64_t p) { a.labels[p] = is_kept_point(a, p) ? a.parent[a.root[p]] : -1; }

// ---- the table.  Rows that exist: 0 <= k < min(cap, totals[0]).
OCC4D_HD int table_rows(const TableArgs& a) {
  const int kept = a.totals[0];
  return kept < a.cap ? (kept < 0 ? 0 : kept) : a.cap;
}

// a row before its first contribution: the identities of the sums, the minima and the maxima
OCC4D_HD void row_init(int64_t* row) {
  row[0] = 0;
  row[1] = INT64_MAX;
  row[2] = -1;
  for (int c = 3; c < 6; ++c) row[c] = 0;
  for (int c = 6; c < 9; ++c) row[c] = INT64_MAX;
  for (int c = 9; c < 12; ++c) row[c] = -1;
}

OCC4D_HD void table_init_row(const TableArgs& a, int k) { row_init(a.table + (int64_t)k * COLS); }

// one contribution: `count` points of component k with the lowest flat index `first`, class `klass`, coordinate sums / minima /
// maxima.
struct Contribution {
  int64_t count, first, klass, sum[3], lo[3], hi[3];
};

OCC4D_HD Contribution contribution_of(const TableArgs& a, int64_t p) {
  int i[3];
  coords_of(a.grid, p, i);
  return Contribution{1, p, a.klass ? (int64_t)a.klass[p] : -1, {i[0], i[1], i[2]}, {i[0], i[1], i[2]}, {i[0], i[1], i[2]}};
}

OCC4D_HD void combine(Contribution& c, const Contribution& o) {
  c.count += o.count;
  c.first = o.first < c.first ? o.first : c.first;
  c.klass = o.klass > c.klass ? o.klass : c.klass;
  for (int x = 0; x < 3; ++x) {
    c.sum[x] += o.sum[x];
    c.lo[x] = o.lo[x] < c.lo[x] ? o.lo[x] : c.lo[x];
    c.hi[x] = o.hi[x] > c.hi[x] ? o.hi[x] : c.hi[x];
  }
}

// a contribution onto a row; T: how the 64-bit atomics are spelled (add, min, max; results unused)
template <class T>
OCC4D_HD void row_add(int64_t* row, const Contribution& c) {
  T::add(row + 0, c.count);
  T::min(row + 1, c.first);
  T::max(row + 2, c.klass);
  for (int x = 0; x < 3; ++x) {
    T::add(row + 3 + x, c.sum[x]);
    T::min(row + 6 + x, c.lo[x]);
    T::max(row + 9 + x, c.hi[x]);
  }
}

// a row as a contribution: what a workgroup gathered for one label
OCC4D_HD Contribution contribution_of_row(const int64_t* row) {
  return Contribution{row[0], row[1], row[2], {row[3], row[4], row[5]}, {row[6], row[7], row[8]}, {row[9], row[10], row[11]}};
}

template <class T>
OCC4D_HD void table_add(const TableArgs& a, int k, int rows, const Contribution& c) {
  if (k < 0 || k >= rows) return;
  row_add<T>(a.table + (int64_t)k * COLS, c);
}

struct PlainTable {
  static OCC4D_HD void add(int64_t* p, int64_t v) { *p += v; }
  static OCC4D_HD void min(int64_t* p, int64_t v) { if (v < *p) *p = v; }
  static OCC4D_HD void max(int64_t* p, int64_t v) { if (v > *p) *p = v; }
};

// ---- argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_grid(const char* who, int nx, int ny, int nz, Grid& g) {
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX",
                who, nx, ny, nz);
  g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  g.tiles[0] = (nx + TX - 1) / TX; g.tiles[1] = (ny + TY - 1) / TY; g.tiles[2] = (nz + TZ - 1) / TZ;
  g.points = (int64_t)nx * ny * nz;
  g.local_tiles = (int64_t)g.tiles[0] * g.tiles[1] * g.tiles[2];
  g.number_tiles = (g.points + TILE - 1) / TILE;
  return OCC4D_OK;
}

inline int check_label(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                       const int32_t* klass, int nx, int ny, int nz, int connectivity, int min_size, int32_t* work, int32_t* labels,
                       int32_t* totals, bool& empty, LabelArgs& a) {
  const char* who = "occ4d_components_label_f32";
  Grid g;
  OCC4D_TRY(check_grid(who, nx, ny, nz, g));
  OCC4D_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity = %d must be 6, 18 or 26", who,
                connectivity);
  OCC4D_REQUIRE(min_size >= 1, "%s: min_size = %d must be >= 1", who, min_size);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(!mask || ld_mask >= 1, "%s: ld_mask = %lld must be >= 1", who, (long long)ld_mask);
  empty = g.points == 0;
  OCC4D_REQUIRE(empty || field, "%s: null field with n = %lld", who, (long long)g.points);
  OCC4D_REQUIRE(empty || (work && labels && totals), "%s: null work / labels / totals with n = %lld", who, (long long)g.points);
  const int64_t n = g.points, nt = g.number_tiles;
  a = LabelArgs{field, ld, mask, ld_mask, klass, work, work + n, work + 2 * n, work + 3 * n, work + 3 * n + nt, work + 3 * n + 2 * nt,
                labels, totals, g, level, mask_level, connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3, min_size};
  return OCC4D_OK;
}

inline int check_table(const int32_t* labels, const int32_t* klass, int nx, int ny, int nz, const int32_t* totals, int64_t* table,
                       int cap, bool& empty, TableArgs& a) {
  const char* who = "occ4d_components_table_i64";
  Grid g;
  OCC4D_TRY(check_grid(who, nx, ny, nz, g));
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  empty = g.points == 0 || cap == 0;
  OCC4D_REQUIRE(empty || (labels && totals && table), "%s: null labels / totals / table with n = %lld, cap = %d", who,
                (long long)g.points, cap);
  a = TableArgs{labels, klass, totals, table, g, cap};
  return OCC4D_OK;
}

}  // namespace occ4d_components
