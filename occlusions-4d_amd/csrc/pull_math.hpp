// Straight free legs over the grid (include/ext/occ4d_pull.h), shared WORD FOR WORD by the HIP kernels (csrc/pull.hip) and the g++
// twin (csrc_cpu/occ4d_twin.cpp): the blocked test, HIT over the walk of csrc/sight_math.hpp (included, not restated), the start of
// a goal, the test of one candidate, the tail of a row and the three argument contracts (host only).  Integers only.
#pragma once
#include <stdint.h>

#include "ext/occ4d_pull.h"
#include "sight_math.hpp"         // walk, solid_at, GlobalWords; OCC4D_HD; contract.hpp

namespace occ4d_pull {

namespace sm = occ4d_sight;

constexpr int MAX_AXIS = OCC4D_SIGHT_MAX_AXIS;
constexpr int ROUND = OCC4D_PULL_ROUND;
static_assert(ROUND % 64 == 0, "a round is whole waves");

struct BitsArgs {
  const int32_t* clear;
  uint32_t* blocked;
  int64_t n, words;
  int32_t min_clear;
};

struct PairArgs {
  const uint32_t* blocked;
  const int32_t *a, *b;
  int32_t* hit;
  int n[3];
  int32_t points;                                                 // nx * ny * nz <= 2^27
  int n_pairs;
};

struct PathArgs {
  const uint32_t* blocked;
  const int32_t *paths, *path_len;
  int32_t *waypoints, *waypoint_len;
  int n[3];
  int32_t points;
  int64_t words;                                                  // ceil(points / 32)
  int n_goals, cap, rounds;                                       // rounds = ceil(cap / ROUND)
};

// ---- the rules
OCC4D_HD bool blocked_at(const BitsArgs& a, int64_t p) { return !(a.clear[p] >= a.min_clear); }

// HIT(a, b).  An index becomes coordinates only after 0 <= v < points; a word is read only through solid_at.
template <class Words>
OCC4D_HD int32_t hit(const int* n, int32_t points, const Words& words, int32_t a, int32_t b) {
  if (a < 0 || a >= points || b < 0 || b >= points) return -2;
  const int ax = a / (n[1] * n[2]), ay = a / n[2] % n[1], az = a % n[2];
  const int bx = b / (n[1] * n[2]), by = b / n[2] % n[1], bz = b % n[2];
  bool inside;
  int32_t flat = 0;
  if (sm::solid_at(n, words, ax, ay, az, inside, flat)) return a;
  if (sm::solid_at(n, words, bx, by, bz, inside, flat)) return b;
  return sm::walk(n, words, ax, ay, az, bx, by, bz);
}

// ---- PULL.  The chain of goal g: its length where it is to be pulled, else 0 (the row is then all -1 and the length passes through)
OCC4D_HD int chain_length(const PathArgs& a, int g) {
  const int32_t L = a.path_len[g];
  return L > 0 && L <= a.cap ? L : 0;
}

// ... whether candidate j of the anchor at chain position k qualifies: j in (k + 1, L - 1] and FREE(p_k, p_j)
template <class Words>
OCC4D_HD bool candidate_free(const PathArgs& a, const Words& words, const int32_t* row, int L, int k, int j) {
  return j > k + 1 && j < L && hit(a.n, a.points, words, row[k], row[j]) == -1;
}

// ---- the argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_bits(const int32_t* clear, int min_clear, int64_t n, uint32_t* blocked, bool& empty, BitsArgs& a) {
  const char* who = "occ4d_pull_bits_i32";
  OCC4D_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld must be in [0, INT32_MAX]", who, (long long)n);
  empty = n == 0;
  OCC4D_REQUIRE(empty || clear, "%s: null clear with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(empty || blocked, "%s: null blocked with n = %lld", who, (long long)n);
  a = BitsArgs{clear, blocked, n, (n + 31) / 32, min_clear};
  return OCC4D_OK;
}

inline int check_axes(const char* who, int nx, int ny, int nz) {
  OCC4D_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: nx = %d, ny = %d, nz = %d must be >= 0", who, nx, ny, nz);
  OCC4D_REQUIRE(nx <= MAX_AXIS && ny <= MAX_AXIS && nz <= MAX_AXIS, "%s: nx = %d, ny = %d, nz = %d must be <= %d", who, nx, ny, nz,
                MAX_AXIS);
  return OCC4D_OK;
}

inline int check_pairs(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* a, const int32_t* b, int n_pairs, int32_t* hit,
                       bool& empty, PairArgs& args) {
  const char* who = "occ4d_pull_pairs_u32";
  OCC4D_TRY(check_axes(who, nx, ny, nz));
  OCC4D_REQUIRE(n_pairs >= 0, "%s: n_pairs = %d must be >= 0", who, n_pairs);
  const int64_t n = (int64_t)nx * ny * nz;                        // <= 2^27
  empty = n_pairs == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(n == 0 || blocked, "%s: null blocked with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(a && b, "%s: null a / b with n_pairs = %d", who, n_pairs);
  OCC4D_REQUIRE(hit, "%s: null hit with n_pairs = %d", who, n_pairs);
  args = PairArgs{blocked, a, b, hit, {nx, ny, nz}, (int32_t)n, n_pairs};
  return OCC4D_OK;
}

inline int check_paths(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* paths, const int32_t* path_len, int n_goals,
                       int cap, int32_t* waypoints, int32_t* waypoint_len, bool& empty, PathArgs& a) {
  const char* who = "occ4d_pull_paths_i32";
  OCC4D_TRY(check_axes(who, nx, ny, nz));
  OCC4D_REQUIRE(n_goals >= 0, "%s: n_goals = %d must be >= 0", who, n_goals);
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  OCC4D_REQUIRE((int64_t)n_goals * cap <= INT32_MAX, "%s: n_goals * cap = %d * %d exceeds INT32_MAX", who, n_goals, cap);
  const int64_t n = (int64_t)nx * ny * nz;                        // <= 2^27
  empty = n_goals == 0 || n == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(blocked, "%s: null blocked with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(path_len && waypoint_len, "%s: null path_len / waypoint_len with n_goals = %d", who, n_goals);
  OCC4D_REQUIRE(cap == 0 || (paths && waypoints), "%s: null paths / waypoints with n_goals = %d, cap = %d", who, n_goals, cap);
  a = PathArgs{blocked, paths, path_len, waypoints, waypoint_len, {nx, ny, nz}, (int32_t)n, (n + 31) / 32, n_goals, cap,
               (cap + ROUND - 1) / ROUND};
  return OCC4D_OK;
}

}  // namespace occ4d_pull
