// Per-row classification of the evaluation statistics (include/occ4d_eval.h), shared WORD FOR WORD by the HIP kernels
// (csrc/evalstats.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): which counters a row touches and what it adds to the
// sums.  Comparisons are fp32; every term of a sum is converted to double before any arithmetic.
#pragma once
#include <math.h>
#include <stdint.h>

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

}  // namespace occ4d_eval
