// The watershed segments of an integer height map (include/ext/occ4d_watershed.h), shared WORD FOR WORD by the HIP kernels
// (csrc/watershed.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): ORDER, the ascent choice, the MERGE test, the item bodies of the
// passes, the packed key of the peaks and the two argument contracts (host only).  Integers only.  find, unite, the grid and its
// coordinates are those of csrc/components_math.hpp.
//
// The item bodies are templates over A, HOW A WORD IS READ AND WRITTEN where another thread of the same launch may touch it:
// A::load / A::store are relaxed atomics and A::fetch_min a relaxed atomic minimum -- agent scope in the kernels, plain memory in
// the twin.
#pragma once
#include <stdint.h>

#include "components_math.hpp"
#include "ext/occ4d_watershed.h"

namespace occ4d_watershed {

namespace cc = occ4d_components;

constexpr int TILE = OCC4D_WATERSHED_TILE;                        // numbering tile: consecutive flat indices
constexpr int TX = OCC4D_WATERSHED_TILE_X, TY = OCC4D_WATERSHED_TILE_Y, TZ = OCC4D_WATERSHED_TILE_Z;
constexpr int TILE_POINTS = TX * TY * TZ;                         // the ascent: one thread per point
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;              // the tile and its halo of one point
constexpr int HALO_POINTS = HX * HY * HZ;
constexpr int ROUND_WORDS = OCC4D_WATERSHED_ROUND_WORDS, TOTALS = OCC4D_WATERSHED_TOTALS, HOPS = OCC4D_WATERSHED_HOPS;
constexpr int NEIGHBOURS = 27, SELF = 13;                         // offsets c = 0 .. 26 in raster order = ascending flat index
static_assert(TILE == cc::TILE && TILE_POINTS <= 1024 && HOPS == 8 && ROUND_WORDS == 12, "a tile is one workgroup; 8^11 > INT32_MAX: 11 rounds and one word");

struct Args {
  const int32_t* height;
  int32_t *basin, *parent, *low, *size;                           // work: n each
  int32_t* counts[TOTALS];                                        // work: number_tiles each: kept roots, kept points, roots, basins
  int32_t* flags;                                                 // work: flags[0] = 1, flags[k] = jump round k changed a word
  int32_t *labels, *totals;
  cc::Grid grid;
  int tiles[3];                                                   // ascent tiles per axis
  int64_t n_tiles;
  int rank;                                                       // 1, 2, 3: the most axes two neighbours differ on
  int h, min_size, rounds;
};

struct PeakArgs {
  const int32_t *height, *labels, *totals;
  unsigned long long* keys;                                       // the rows of peaks, one 64-bit word each
  int32_t* peaks;
  int n, cap;
};

struct Plain : cc::Plain {                                        // one thread: the twin, and the passes that only read
  static OCC4D_HD void store(int32_t* p, int v) { *p = v; }
};

// ---- the rules
OCC4D_HD int32_t level_of(int32_t v) { return v >= 1 ? v : 0; }   // a member's height, 0 for no member

OCC4D_HD int offset_of(int c, int* d) {                           // -> the number of axes the offset changes
  d[0] = c / 9 - 1;
  d[1] = (c / 3) % 3 - 1;
  d[2] = c % 3 - 1;
  return (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
}

// THE ASCENT CHOICE of a member of height `own`: the offset c of up(p), SELF for a maximum.  at(dx, dy, dz): level_of the height
// at that offset, 0 outside the grid.  ORDER: higher wins; among equal heights the lower flat index, which is the lower c.
template <class F>
OCC4D_HD int ascent_choice(int rank, int32_t own, F&& at) {
  int best = SELF;
  int32_t top = own;
#pragma unroll
  for (int c = 0; c < NEIGHBOURS; ++c) {
    int d[3];
    const int kind = offset_of(c, d);
    if (kind == 0 || kind > rank) continue;
    const int32_t v = at(d[0], d[1], d[2]);
    if (v < 1) continue;
    if (v > top || (v == top && c < best)) {
      top = v;
      best = c;
    }
  }
  return best;
}

// THE MERGE TEST of an adjacent pair of heights hp, hq whose basins have the peaks peak_a >= hp, peak_b >= hq (all >= 1)
OCC4D_HD bool related(int32_t peak_a, int32_t peak_b, int32_t hp, int32_t hq, int32_t h) {
  return (peak_a < peak_b ? peak_a : peak_b) - (hp < hq ? hp : hq) <= h;
}

// the flat index of the coordinates, -1 outside the grid
OCC4D_HD int64_t flat_of(const cc::Grid& g, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0 || x >= g.n[0] || y >= g.n[1] || z >= g.n[2]) return -1;
  return ((int64_t)x * g.n[1] + y) * g.n[2] + z;
}

// the neighbour levels of point (i) straight from height[]: the twin's ascent
struct GridAt {
  const Args& a;
  const int* i;
  OCC4D_HD int32_t operator()(int dx, int dy, int dz) const {
    const int64_t q = flat_of(a.grid, i[0] + dx, i[1] + dy, i[2] + dz);
    return q < 0 ? 0 : level_of(a.height[q]);
  }
};

// ---- the tiling of the ascent kernel (the scheme of csrc/geodesic_math.hpp)
OCC4D_HD void tile_origin(const Args& a, int64_t b, int* o) {
  o[2] = (int)(b % a.tiles[2]) * TZ;
  o[1] = (int)((b / a.tiles[2]) % a.tiles[1]) * TY;
  o[0] = (int)(b / ((int64_t)a.tiles[1] * a.tiles[2])) * TX;
}
OCC4D_HD int64_t halo_point(const Args& a, const int* o, int s) {     // s in [0, HALO_POINTS) -> flat index, -1 outside the grid
  return flat_of(a.grid, o[0] + s / (HY * HZ) - 1, o[1] + (s / HZ) % HY - 1, o[2] + s % HZ - 1);
}
OCC4D_HD int own_slot(int t) { return ((t / (TY * TZ) + 1) * HY + (t / TZ) % TY + 1) * HZ + t % TZ + 1; }
OCC4D_HD int64_t own_point(const Args& a, const int* o, int t) {
  return flat_of(a.grid, o[0] + t / (TY * TZ), o[1] + (t / TZ) % TY, o[2] + t % TZ);
}

// ---- pass 1, the ascent of point p with the choice c (any c for a non-member of level 0): up(p) into basin[], the maxima as
// the roots of parent[], and the identities of low[] and size[]
OCC4D_HD void ascent_item(const Args& a, int64_t p, int32_t own, int c) {
  int d[3];
  offset_of(c, d);
  const int64_t up = own < 1 ? -1 : p + ((int64_t)d[0] * a.grid.n[1] + d[1]) * a.grid.n[2] + d[2];   // (in the grid: its level was >= 1)
  a.basin[p] = (int32_t)up;
  a.parent[p] = up == p ? (int32_t)p : -1;
  a.low[p] = INT32_MAX;
  a.size[p] = 0;
}

// the flags of the jump rounds, word k of ROUND_WORDS
OCC4D_HD void flag_init(const Args& a, int k) { a.flags[k] = k == 0 ? 1 : 0; }

// ---- pass 2, a jump round at point p: basin[p] = the pointer followed HOPS times, or to a maximum -> whether the word changed.
// When every pointer reaches d steps along up (or a maximum) before a round, it reaches HOPS * d after it.  Every value ever stored
// in basin[p] is p itself or an ancestor of p along up, so a load that meets another thread's store of the same launch returns an
// ancestor all the same (a longer jump), and a round that changes no word saw one array in which every pointer ends at a maximum.
template <class A>
OCC4D_HD bool jump_item(const Args& a, int64_t p) {
  const int u = A::load(a.basin + p);
  if (u < 0) return false;
  int cur = u;
  for (int k = 1; k < HOPS; ++k) {
    const int g = A::load(a.basin + cur);
    if (g < 0 || g == cur) break;                                 // (< 0 is never stored for a member)
    cur = g;
  }
  if (cur == u) return false;
  A::store(a.basin + p, cur);
  return true;
}

// ---- pass 3, the merge at point p: the MERGE test with every FORWARD neighbour q (each pair once), the basins united when it holds
template <class A>
OCC4D_HD void merge_item(const Args& a, int64_t p) {
  const int32_t hp = level_of(a.height[p]);
  if (hp < 1) return;
  const int32_t mine = a.basin[p];
  const int32_t peak = level_of(a.height[mine]);
  int i[3];
  cc::coords_of(a.grid, p, i);
  for (int c = SELF + 1; c < NEIGHBOURS; ++c) {
    int d[3];
    const int kind = offset_of(c, d);
    if (kind > a.rank) continue;
    const int64_t q = flat_of(a.grid, i[0] + d[0], i[1] + d[1], i[2] + d[2]);
    if (q < 0) continue;
    const int32_t hq = level_of(a.height[q]);
    if (hq < 1) continue;
    const int32_t other = a.basin[q];
    if (other == mine) continue;
    if (related(peak, level_of(a.height[other]), hp, hq, a.h)) cc::unite<A>(a.parent, mine, other);
  }
}

// ---- pass 4, flatten: the representative of p's segment (the lowest maximum of the class; -1 for a non-member) into basin[]; the
// caller adds the point to size[rep] and lowers low[rep] to p
OCC4D_HD int flatten_item(const Args& a, int64_t p) {
  const int b = a.basin[p];
  const int r = b < 0 ? -1 : cc::find<cc::Plain>(a.parent, b);
  a.basin[p] = r;
  return r;
}

// ---- passes 5 to 8, numbering.  What point p adds to its tile's four counts:
OCC4D_HD bool is_root(const Args& a, int64_t p) { return a.basin[p] >= 0 && a.low[a.basin[p]] == (int32_t)p; }
OCC4D_HD bool is_kept_point(const Args& a, int64_t p) { return a.basin[p] >= 0 && a.size[a.basin[p]] >= a.min_size; }
OCC4D_HD bool is_kept_root(const Args& a, int64_t p) { return is_root(a, p) && is_kept_point(a, p); }
OCC4D_HD bool is_basin(const Args& a, int64_t p) { return a.parent[p] >= 0; }        // (a maximum: >= 0 since pass 1, for ever)
OCC4D_HD bool flag_of(const Args& a, int64_t p, int which) {
  return which == 0 ? is_kept_root(a, p) : which == 1 ? is_kept_point(a, p) : which == 2 ? is_root(a, p) : is_basin(a, p);
}
// ... a kept segment's number goes into parent[rep] (a maximum's word, free since pass 4), and then every point's label:
OCC4D_HD void number_item(const Args& a, int64_t p, int number) { a.parent[a.basin[p]] = number; }
OCC4D_HD void label_item(const Args& a, int64_t p) { a.labels[p] = is_kept_point(a, p) ? a.parent[a.basin[p]] : -1; }

// ---- the peaks.  Rows that exist: 0 <= k < min(cap, totals[0]).
OCC4D_HD int peak_rows(const PeakArgs& a) {
  const int kept = a.totals[0];
  return kept < a.cap ? (kept < 0 ? 0 : kept) : a.cap;
}

// THE KEY of member p: (height, INT32_MAX - p), so that a greater key is above under ORDER; 0 is below every member's key
OCC4D_HD unsigned long long key_of(int32_t height, int64_t p) {
  return ((unsigned long long)(uint32_t)height << 32) | (uint32_t)(INT32_MAX - (int32_t)p);
}

// point p's row and key: -1 when it contributes nothing (no member, no label, a row that does not exist)
OCC4D_HD int peak_contribution(const PeakArgs& a, int64_t p, int rows, unsigned long long& key) {
  const int k = a.labels[p];
  const int32_t height = a.height[p];
  key = 0;
  if (k < 0 || k >= rows || height < 1) return -1;
  key = key_of(height, p);
  return k;
}

// the row's key into its two words: the flat index, the height
OCC4D_HD void peak_unpack(const PeakArgs& a, int k) {
  unsigned long long key;
  __builtin_memcpy(&key, a.peaks + 2 * (int64_t)k, sizeof key);   // (the row's two words, read as the one they were combined in)
  const int32_t index = key == 0 ? -1 : INT32_MAX - (int32_t)(uint32_t)(key & 0xffffffffull);
  const int32_t height = (int32_t)(uint32_t)(key >> 32);
  a.peaks[2 * (int64_t)k] = index;
  a.peaks[2 * (int64_t)k + 1] = height;
}

// ---- argument contracts (host): the status, `empty` = nothing to do, the arguments filled
OCC4D_HD int rounds_of(int64_t n) {                               // ceil(log8 n): the least R with HOPS^R >= n
  int r = 0;
  for (int k = 0; k < ROUND_WORDS - 1; ++k)
    if (((int64_t)1 << (3 * k)) < n) r = k + 1;
  return r;
}

inline int check_label(const int32_t* height, int nx, int ny, int nz, int connectivity, int h, int min_size, int32_t* work,
                       int32_t* labels, int32_t* totals, bool& empty, Args& a) {
  const char* who = "occ4d_watershed_label_i32";
  cc::Grid g;
  OCC4D_TRY(cc::check_grid(who, nx, ny, nz, g));
  OCC4D_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity = %d must be 6, 18 or 26", who,
                connectivity);
  OCC4D_REQUIRE(h >= 0, "%s: h = %d must be >= 0", who, h);
  OCC4D_REQUIRE(min_size >= 1, "%s: min_size = %d must be >= 1", who, min_size);
  empty = g.points == 0;
  OCC4D_REQUIRE(empty || height, "%s: null height with n = %lld", who, (long long)g.points);
  OCC4D_REQUIRE(empty || (work && labels && totals), "%s: null work / labels / totals with n = %lld", who, (long long)g.points);
  const int64_t n = g.points, nt = g.number_tiles;
  a.height = height;
  a.basin = work; a.parent = work + n; a.low = work + 2 * n; a.size = work + 3 * n;
  for (int c = 0; c < TOTALS; ++c) a.counts[c] = work + 4 * n + c * nt;
  a.flags = work + 4 * n + TOTALS * nt;
  a.labels = labels; a.totals = totals;
  a.grid = g;
  a.tiles[0] = (nx + TX - 1) / TX; a.tiles[1] = (ny + TY - 1) / TY; a.tiles[2] = (nz + TZ - 1) / TZ;
  a.n_tiles = (int64_t)a.tiles[0] * a.tiles[1] * a.tiles[2];
  a.rank = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  a.h = h; a.min_size = min_size; a.rounds = rounds_of(n);
  return OCC4D_OK;
}

inline int check_peaks(const int32_t* height, const int32_t* labels, int n, const int32_t* totals, int32_t* peaks, int cap, bool& empty,
                       PeakArgs& a) {
  const char* who = "occ4d_watershed_peaks_i32";
  OCC4D_REQUIRE(n >= 0, "%s: n = %d must be >= 0", who, n);
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  empty = n == 0 || cap == 0;
  OCC4D_REQUIRE(empty || (height && labels && totals && peaks), "%s: null height / labels / totals / peaks with n = %d, cap = %d", who,
                n, cap);
  OCC4D_REQUIRE(empty || (uintptr_t)peaks % 8 == 0, "%s: peaks must be aligned to 8 bytes", who);
  a = PeakArgs{height, labels, totals, (unsigned long long*)peaks, peaks, n, cap};
  return OCC4D_OK;
}

}  // namespace occ4d_watershed
