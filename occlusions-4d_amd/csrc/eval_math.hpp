// Per-row classification of the evaluation statistics (include/occ4d_eval.h) and the entry points' argument contracts (host
// only), shared WORD FOR WORD by the HIP kernels (csrc/evalstats.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): which
// counters a row touches and what it adds to the sums.  Comparisons are fp32; every term of a sum is converted to double
// before any arithmetic.
#pragma once
#include <math.h>
#include <stdint.h>

#include "contract.hpp"
#include "occ4d_eval.h"

#if defined(__HIPCC__)
#define OCC4D_EVAL_HD __host__ __device__ __forceinline__
#else
#define OCC4D_EVAL_HD inline
#endif

namespace occ4d_eval {

struct QueryArgs {
  const float* out; int64_t ldo; int n, g_out;
  const int32_t* nn_idx; const float* nn_dist;
  const float* target; int64_t ldt; int m;
  int col_rgb, col_track, col_sem, out_track;      // a column < 0: that statistic is not scored
  const int32_t* group; int n_groups, n_classes;
  float threshold, radius;
};

// What query row i adds.  group < 0: a bad row (BAD_ROWS and nothing else).
struct QueryRow {
  int group;
  int occ;            // OCC4D_EVAL_OCC_TP .. OCC_TN
  bool solid;         // predicted solid: N_ACCURACY, d, d2
  double d, d2;
  bool color;         // N_COLOR, l1
  double l1;
  int track;          // OCC4D_EVAL_TRACK_TP .. TRACK_TN, or -1
  int seg;            // r * C + c of the confusion matrix, -1: not scored, -2: SEG_IGNORED
};

OCC4D_EVAL_HD int64_t group_stride(int n_classes) { return OCC4D_EVAL_GROUP_COUNTS + (int64_t)n_classes * n_classes; }

// group of target point j, -1 when j or the id is out of range
OCC4D_EVAL_HD int group_of(const int32_t* group, int j, int m, int n_groups) {
  if (j < 0 || j >= m) return -1;
  const int g = group ? group[j] : 0;
  return (g >= 0 && g < n_groups) ? g : -1;
}

OCC4D_EVAL_HD QueryRow classify_query(const QueryArgs& a, int i) {
  QueryRow r;
  r.occ = 0; r.solid = false; r.d = r.d2 = r.l1 = 0.0; r.color = false; r.track = -1; r.seg = -1;
  const int j = a.nn_idx[i];
  r.group = group_of(a.group, j, a.m, a.n_groups);
  if (r.group < 0) return r;
  const float* o = a.out + (int64_t)i * a.ldo;
  const float* t = a.target + (int64_t)j * a.ldt;
  const float dist = a.nn_dist[i];
  const bool pred = o[0] >= a.threshold, label = dist < a.radius;
  r.occ = pred ? (label ? OCC4D_EVAL_OCC_TP : OCC4D_EVAL_OCC_FP) : (label ? OCC4D_EVAL_OCC_FN : OCC4D_EVAL_OCC_TN);
  if (pred) {
    r.solid = true;
    r.d = (double)dist;
    r.d2 = r.d * r.d;
  }
  if (!(pred && label)) return r;
  if (a.col_rgb >= 0) {
    r.color = true;
    r.l1 = fabs((double)o[1] - (double)t[a.col_rgb]) + fabs((double)o[2] - (double)t[a.col_rgb + 1]) +
           fabs((double)o[3] - (double)t[a.col_rgb + 2]);
  }
  if (a.col_track >= 0) {
    const bool p = o[a.out_track] >= 0.5f, g = t[a.col_track] > 0.5f;
    r.track = p ? (g ? OCC4D_EVAL_TRACK_TP : OCC4D_EVAL_TRACK_FP) : (g ? OCC4D_EVAL_TRACK_FN : OCC4D_EVAL_TRACK_TN);
  }
  if (a.col_sem >= 0) {
    const int C = a.n_classes;
    const float tag = t[a.col_sem];
    if (tag >= 0.f && tag < (float)C && tag == floorf(tag)) {
      const float* s = o + (a.g_out - C);
      int best = 0;
      for (int c = 1; c < C; ++c)
        if (s[c] > s[best]) best = c;          // first argmax
      r.seg = (int)tag * C + best;
    } else {
      r.seg = -2;
    }
  }
  return r;
}

// ---- argument contracts (host): the status, `empty` = nothing to do
inline bool layout_ok(int n_groups, int n_classes) {
  return n_groups >= 1 && n_groups <= OCC4D_EVAL_MAX_GROUPS && n_classes >= 0 && n_classes <= OCC4D_EVAL_MAX_CLASSES;
}
inline int64_t counts_len(int n_groups, int n_classes) {
  return layout_ok(n_groups, n_classes) ? OCC4D_EVAL_HEAD + n_groups * group_stride(n_classes) : -1;
}
inline int64_t sums_len(int n_groups) { return layout_ok(n_groups, 0) ? (int64_t)n_groups * OCC4D_EVAL_GROUP_SUMS : -1; }

// fills `a`, its col_* reduced to -1 where the flags or the class count switch the statistic off
inline int check_query_stats(const float* out, int64_t ldo, int n, int g_out, const int32_t* nn_idx, const float* nn_dist,
                             const float* target, int64_t ldt, int m, int dt, int col_rgb, int col_track, int col_sem, int out_track,
                             const int32_t* target_group, int n_groups, int n_classes, float density_threshold, float radius,
                             int flags, const int64_t* counts, const double* sums, const void* workspace, bool& empty, QueryArgs& a) {
  const char* who = "occ4d_eval_query_stats_f32";
  OCC4D_REQUIRE(layout_ok(n_groups, n_classes), "%s: n_groups = %d must be in 1 .. 8, n_classes = %d in 0 .. 32", who, n_groups, n_classes);
  OCC4D_REQUIRE(n >= 0 && m >= 0 && g_out >= 1 && dt >= 1 && ldo >= g_out && ldt >= dt, "%s: n = %d, m = %d, g_out = %d, ldo = %lld, dt = %d, ldt = %lld",
                who, n, m, g_out, (long long)ldo, dt, (long long)ldt);
  OCC4D_REQUIRE(counts && sums && workspace && ((uintptr_t)workspace % 8) == 0, "%s: null counts / sums / workspace, or workspace not 8-byte aligned", who);
  empty = n == 0;
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(out && nn_idx && nn_dist && (target || m == 0), "%s: null pointer", who);
  const bool color = (flags & OCC4D_EVAL_FLAG_COLOR) && col_rgb >= 0;
  const bool track = (flags & OCC4D_EVAL_FLAG_TRACK) && col_track >= 0;
  const bool seg = (flags & OCC4D_EVAL_FLAG_SEG) && col_sem >= 0 && n_classes >= 1;
  OCC4D_REQUIRE(!color || (g_out >= 4 && col_rgb + 3 <= dt), "%s: colour needs g_out = %d >= 4 and col_rgb = %d + 3 <= dt = %d", who, g_out, col_rgb, dt);
  OCC4D_REQUIRE(!track || (out_track >= 0 && out_track < g_out && col_track < dt), "%s: tracking needs out_track = %d < g_out = %d and col_track = %d < dt = %d",
                who, out_track, g_out, col_track, dt);
  OCC4D_REQUIRE(!seg || (g_out >= n_classes && col_sem < dt), "%s: segmentation needs g_out = %d >= n_classes = %d and col_sem = %d < dt = %d", who,
                g_out, n_classes, col_sem, dt);
  a = QueryArgs{out, ldo, n, g_out, nn_idx, nn_dist, target, ldt, m, color ? col_rgb : -1, track ? col_track : -1,
                seg ? col_sem : -1, out_track, target_group, n_groups, n_classes, density_threshold, radius};
  return OCC4D_OK;
}

inline int check_target_stats(const float* dist, int m, int n_groups, int n_classes, const int64_t* counts, const double* sums,
                              const void* workspace, bool& empty) {
  const char* who = "occ4d_eval_target_stats_f32";
  OCC4D_REQUIRE(layout_ok(n_groups, n_classes), "%s: n_groups = %d must be in 1 .. 8, n_classes = %d in 0 .. 32", who, n_groups, n_classes);
  OCC4D_REQUIRE(m >= 0 && counts && sums && workspace && ((uintptr_t)workspace % 8) == 0, "%s: m = %d, null counts / sums / workspace, or workspace not 8-byte aligned", who, m);
  empty = m == 0;
  OCC4D_REQUIRE(empty || dist, "%s: null pointer", who);
  return OCC4D_OK;
}

}  // namespace occ4d_eval
