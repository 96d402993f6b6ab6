// The next best view over the grid (include/ext/occ4d_viewplan.h), shared WORD FOR WORD by the HIP kernels (csrc/viewplan.hip) and
// the g++ twin (csrc_cpu/occ4d_twin.cpp): DEAD, RANGE and the test of one (candidate, point) pair over the walk of
// csrc/sight_math.hpp (included, not restated), the layout of the work array, the rows and the keys of GREEDY and the two argument
// contracts (host only).  Integers only.
#pragma once
#include <stdint.h>

#include "ext/occ4d_viewplan.h"
#include "sight_math.hpp"         // walk, solid_at, GlobalWords; OCC4D_HD; contract.hpp

namespace occ4d_viewplan {

namespace sm = occ4d_sight;

constexpr int MAX_AXIS = OCC4D_SIGHT_MAX_AXIS;
constexpr int MAX_COORD = OCC4D_SIGHT_MAX_COORD;
constexpr int MAX_CANDIDATES = OCC4D_VIEWPLAN_MAX_CANDIDATES;
constexpr int MAX_PICKS = OCC4D_VIEWPLAN_MAX_PICKS;
constexpr int MAX_WEIGHT = OCC4D_VIEWPLAN_MAX_WEIGHT;
constexpr int CHUNK = OCC4D_VIEWPLAN_CHUNK;
constexpr int SLICE = OCC4D_VIEWPLAN_SLICE;
constexpr int KEY_BITS = 13;                                      // a key: the count above, 2^13 - 1 - c below
static_assert(MAX_CANDIDATES < (1 << KEY_BITS), "a candidate's number fits the low bits of a key");
// RANGE: |d| <= MAX_COORD + MAX_AXIS < 2^20.01, d^2 < 2^40.02, times a weight <= 2^10: each term < 2^51, their sum < 2^53

struct VisArgs {
  const uint32_t *solid, *targets;
  const int32_t* candidates;
  uint32_t* vis;
  int n[3];
  int32_t points;                                                 // nx * ny * nz <= 2^27
  int64_t words;                                                  // W = ceil(points / 32)
  int C;
  int64_t w[3], max_dist2;
};

struct GreedyArgs {
  const uint32_t *vis, *targets;
  int32_t *work, *gain, *picks, *pick_gain, *status;
  int C, k;
  int64_t W;
};

// ---- VIS
struct Candidate {
  int x, y, z;
  bool live;
};

// Candidate c of the list: DEAD beyond MAX_COORD -- tested before any coordinate is used -- or in a solid cell of the grid
template <class Words>
OCC4D_HD Candidate candidate_at(const VisArgs& a, const Words& words, int c) {
  const int32_t x = a.candidates[3 * c], y = a.candidates[3 * c + 1], z = a.candidates[3 * c + 2];
  Candidate k{x, y, z, false};
  if (x < -MAX_COORD || x > MAX_COORD || y < -MAX_COORD || y > MAX_COORD || z < -MAX_COORD || z > MAX_COORD) return k;
  bool inside;
  int32_t flat = 0;
  k.live = !sm::solid_at(a.n, words, x, y, z, inside, flat);
  return k;
}

// bit p % 32 of word p / 32 of `targets`, 0 behind the grid's last point
OCC4D_HD bool target_at(const VisArgs& a, int64_t p) { return p < a.points && ((a.targets[p >> 5] >> (p & 31)) & 1u); }

OCC4D_HD void point_of(const VisArgs& a, int32_t p, int& x, int& y, int& z) {
  x = p / (a.n[1] * a.n[2]), y = p / a.n[2] % a.n[1], z = p % a.n[2];
}

OCC4D_HD bool in_range(const VisArgs& a, int px, int py, int pz, const Candidate& k) {
  if (a.max_dist2 < 0) return true;
  const int64_t dx = (int64_t)k.x - px, dy = (int64_t)k.y - py, dz = (int64_t)k.z - pz;
  return a.w[0] * dx * dx + a.w[1] * dy * dy + a.w[2] * dz * dz <= a.max_dist2;
}

// ... whether the live-or-dead candidate k sees the TARGET point (px, py, pz): the last three conditions of VIS
template <class Words>
OCC4D_HD bool sees(const VisArgs& a, const Words& words, int px, int py, int pz, const Candidate& k) {
  return k.live && in_range(a, px, py, pz, k) && sm::walk(a.n, words, px, py, pz, k.x, k.y, k.z) == -1;
}

// ---- GREEDY.  The work array: remaining (W) | count (C + 1) | the flag word
OCC4D_HD int64_t work_len(int C, int64_t W) { return W + C + 2; }
OCC4D_HD uint32_t* remaining_of(const GreedyArgs& a) { return (uint32_t*)a.work; }
OCC4D_HD int32_t* count_of(const GreedyArgs& a) { return a.work + a.W; }
OCC4D_HD int32_t* flag_of(const GreedyArgs& a) { return a.work + a.W + a.C + 1; }

// word w of row `row` of the counting pass: a row of vis, or for row == C all ones -- that row counts `remaining` itself
OCC4D_HD uint32_t row_word(const GreedyArgs& a, int row, int64_t w) { return row < a.C ? a.vis[(int64_t)row * a.W + w] : ~0u; }

// the largest key is the largest count and, among equal counts, the lowest candidate
OCC4D_HD unsigned long long key_of(int32_t count, int c) {
  return ((unsigned long long)(uint32_t)count << KEY_BITS) | (unsigned long long)((1 << KEY_BITS) - 1 - c);
}
OCC4D_HD int32_t key_count(unsigned long long key) { return (int32_t)(key >> KEY_BITS); }
OCC4D_HD int key_pick(unsigned long long key) { return (1 << KEY_BITS) - 1 - (int)(key & ((1 << KEY_BITS) - 1)); }

// ... whether a round's best key is a pick: it reveals something, and its number is a row of vis
OCC4D_HD bool key_picks(const GreedyArgs& a, unsigned long long key) {
  return key_count(key) > 0 && key_pick(key) >= 0 && key_pick(key) < a.C;
}

// ---- the argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_visible(const uint32_t* solid, int nx, int ny, int nz, const uint32_t* targets, const int32_t* candidates, int C,
                         int wx, int wy, int wz, int64_t max_dist2, uint32_t* vis, bool& empty, VisArgs& a) {
  const char* who = "occ4d_viewplan_visible_u32";
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  OCC4D_REQUIRE(C >= 0 && C <= MAX_CANDIDATES, "%s: C = %d must be in [0, %d]", who, C, MAX_CANDIDATES);
  OCC4D_REQUIRE(wx >= 1 && wy >= 1 && wz >= 1 && wx <= MAX_WEIGHT && wy <= MAX_WEIGHT && wz <= MAX_WEIGHT,
                "%s: wx = %d, wy = %d, wz = %d must be in [1, %d]", who, wx, wy, wz, MAX_WEIGHT);
  const int64_t n = (int64_t)nx * ny * nz, W = (n + 31) / 32;     // n <= 2^27
  empty = n == 0 || C == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(C * W <= INT32_MAX, "%s: C * W = %d * %lld exceeds INT32_MAX", who, C, (long long)W);
  OCC4D_REQUIRE(solid, "%s: null solid with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(targets, "%s: null targets with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(candidates, "%s: null candidates with C = %d", who, C);
  OCC4D_REQUIRE(vis, "%s: null vis with C = %d, n = %lld", who, C, (long long)n);
  a = VisArgs{solid, targets, candidates, vis, {nx, ny, nz}, (int32_t)n, W, C, {wx, wy, wz}, max_dist2};
  return OCC4D_OK;
}

inline int check_greedy(const uint32_t* vis, int C, int64_t W, const uint32_t* targets, int k, int32_t* work, int32_t* gain,
                        int32_t* picks, int32_t* pick_gain, int32_t* status, bool& empty, GreedyArgs& a) {
  const char* who = "occ4d_viewplan_greedy_u32";
  OCC4D_REQUIRE(C >= 0 && C <= MAX_CANDIDATES, "%s: C = %d must be in [0, %d]", who, C, MAX_CANDIDATES);
  OCC4D_REQUIRE(W >= 0, "%s: W = %lld must be >= 0", who, (long long)W);
  OCC4D_REQUIRE(k >= 0 && k <= MAX_PICKS, "%s: k = %d must be in [0, %d]", who, k, MAX_PICKS);
  empty = W == 0 || C == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(W <= INT32_MAX / C, "%s: C * W = %d * %lld exceeds INT32_MAX", who, C, (long long)W);
  OCC4D_REQUIRE(vis, "%s: null vis with C = %d, W = %lld", who, C, (long long)W);
  OCC4D_REQUIRE(targets, "%s: null targets with W = %lld", who, (long long)W);
  OCC4D_REQUIRE(work, "%s: null work with C = %d, W = %lld", who, C, (long long)W);
  OCC4D_REQUIRE(gain && status, "%s: null gain / status with C = %d", who, C);
  OCC4D_REQUIRE(k == 0 || (picks && pick_gain), "%s: null picks / pick_gain with k = %d", who, k);
  a = GreedyArgs{vis, targets, work, gain, picks, pick_gain, status, C, k, W};
  return OCC4D_OK;
}

}  // namespace occ4d_viewplan
