// The running track merge (include/occ4d_track.h), shared WORD FOR WORD by the HIP kernels (csrc/trackmerge.hip) and the g++
// twin (csrc_cpu/occ4d_twin.cpp): the per-channel squash, the winner / best update with numpy's NaN rule, the two passes'
// element bodies (add_one, finish_one) and the two entry points' argument contracts (host only).  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>

#include "contract.hpp"

#if defined(__HIPCC__)
#define OCC4D_TRACK_HD __host__ __device__ __forceinline__
#else
#define OCC4D_TRACK_HD inline
#endif

namespace occ4d_track {

// the g <= 32 squash codes (0 identity, 1 sigmoid, 2 clamp), two bits per channel: no table lookup in the kernel
OCC4D_TRACK_HD uint64_t pack_codes(const int32_t* ops, int g) {
  uint64_t packed = 0;
  if (ops)
    for (int c = 0; c < g; ++c) packed |= (uint64_t)(ops[c] & 3) << (2 * c);
  return packed;
}
OCC4D_TRACK_HD int code_of(uint64_t packed, int c) { return (int)((packed >> (2 * c)) & 3u); }

// the expression of squash_kernel (csrc/pointops.hip), letter for letter
OCC4D_TRACK_HD float squash(float v, int op) {
  if (op == 1) v = 1.0f / (1.0f + expf(-v));
  else if (op == 2) v = fminf(fmaxf(v, 0.f), 1.f);
  return v;
}

// one rerun's score `s` of a row onto (best, winner): numpy's `winner[(s >= 0.5) & (s >= best)] = id; best = maximum(s, best)`.
// np.maximum hands a NaN of either operand on, and no comparison with a NaN best holds: after a NaN score the row's
// winner stays.  A tie goes to this (the later) rerun.
OCC4D_TRACK_HD void winner_update(float s, float inst_id, float& best, float& winner) {
  if (s >= 0.5f && s >= best) winner = inst_id;
  if (s != s) best = s;
  else if (best == best && s > best) best = s;
}

struct AddArgs {
  const float* out; int64_t ld_out;
  float* acc; int64_t ld_acc;
  float* best; float* winner;
  int64_t total;                          // n * g
  int g, track_col;
  float inst_id;
  uint64_t codes;
};

// element (row i, channel c): the rerun's raw value and the accumulator's value -> the accumulator's new value
template <bool FIRST>
OCC4D_TRACK_HD float add_one(const AddArgs& a, float raw, float prev, int64_t i, int c) {
  const float v = squash(raw, code_of(a.codes, c));
  if (c == a.track_col) {
    float best = FIRST ? 0.f : a.best[i], winner = FIRST ? -1.f : a.winner[i];
    winner_update(v, a.inst_id, best, winner);
    a.best[i] = best;
    a.winner[i] = winner;
  }
  return FIRST ? v : prev + v;
}

struct FinishArgs {
  float* acc; int64_t ld_acc;
  const float* winner;
  int64_t total;
  int g, track_col;
  float runs;
};

OCC4D_TRACK_HD float finish_one(const FinishArgs& f, float sum, int64_t i, int c) {
  return c == f.track_col ? f.winner[i] : sum / f.runs;
}

// ---- argument contracts (host): the status, `empty` = nothing to do, the pass's arguments filled
inline int check_merge_add(const float* out, int64_t ld_out, int n, int g, const int32_t* ops_host, int track_col, float inst_id,
                           int first, float* acc, int64_t ld_acc, float* best, float* winner, bool& empty, AddArgs& a) {
  const char* who = "occ4d_track_merge_add_f32";
  OCC4D_REQUIRE(n >= 0 && g >= 1 && g <= 32, "%s: n = %d, g = %d: need n >= 0, 1 <= g <= 32", who, n, g);
  OCC4D_REQUIRE(ld_out >= g && ld_acc >= g, "%s: ld_out = %lld, ld_acc = %lld must be >= g = %d", who, (long long)ld_out,
                (long long)ld_acc, g);
  OCC4D_REQUIRE(track_col >= -1 && track_col < g, "%s: track_col = %d must be -1 or in 0 .. g - 1 = %d", who, track_col, g - 1);
  OCC4D_REQUIRE(first == 0 || first == 1, "%s: first = %d must be 0 or 1", who, first);
  if (ops_host)
    for (int c = 0; c < g; ++c) OCC4D_REQUIRE(ops_host[c] >= 0 && ops_host[c] <= 2, "%s: op code %d", who, ops_host[c]);
  empty = n == 0;
  OCC4D_REQUIRE(empty || (out && acc), "%s: null out / acc", who);
  OCC4D_REQUIRE(empty || track_col < 0 || (best && winner), "%s: null best / winner with track_col = %d", who, track_col);
  a = AddArgs{out, ld_out, acc, ld_acc, best, winner, (int64_t)n * g, g, track_col, inst_id, pack_codes(ops_host, g)};
  return OCC4D_OK;
}

inline int check_merge_finish(float* acc, int64_t ld_acc, int n, int g, int n_runs, int track_col, const float* winner, bool& empty,
                              FinishArgs& f) {
  const char* who = "occ4d_track_merge_finish_f32";
  OCC4D_REQUIRE(n >= 0 && g >= 1 && g <= 32, "%s: n = %d, g = %d: need n >= 0, 1 <= g <= 32", who, n, g);
  OCC4D_REQUIRE(ld_acc >= g, "%s: ld_acc = %lld must be >= g = %d", who, (long long)ld_acc, g);
  OCC4D_REQUIRE(track_col >= -1 && track_col < g, "%s: track_col = %d must be -1 or in 0 .. g - 1 = %d", who, track_col, g - 1);
  OCC4D_REQUIRE(n_runs >= 1, "%s: n_runs = %d must be >= 1", who, n_runs);
  empty = n == 0;
  OCC4D_REQUIRE(empty || acc, "%s: null acc", who);
  OCC4D_REQUIRE(empty || track_col < 0 || winner, "%s: null winner with track_col = %d", who, track_col);
  f = FinishArgs{acc, ld_acc, winner, (int64_t)n * g, g, track_col, (float)n_runs};
  return OCC4D_OK;
}

}  // namespace occ4d_track
