// Per-row decisions of the instance statistics (include/occ4d_inst.h), the per-id arithmetic of the fold and the entry points'
// argument contracts (host only), shared WORD FOR WORD by the HIP kernels (csrc/inststats.hip) and the g++ twin
// (csrc_cpu/occ4d_twin.cpp).  Comparisons are fp32 and come BEFORE any conversion: a NaN fails them all, so no index and no
// fixed-point value is ever made from an unchecked float.  The class rule is that of the id histogram (csrc/occl_math.hpp:
// bin_of), restated on a single value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "contract.hpp"
#include "occ4d_inst.h"

#if defined(__HIPCC__)
#define OCC4D_INST_HD __host__ __device__ __forceinline__
#else
#define OCC4D_INST_HD inline
#endif

namespace occ4d_inst {

constexpr int CLASS_OTHER = -1;                  // id_class: no class; a row that consults it is a bad row
constexpr int ROW_BAD = -1, ROW_SKIP = -2;       // confusion_cell / point_row: BAD_ROWS and nothing else / nothing at all

// class of v: i in [0, n_ids), n_ids = NONE, or CLASS_OTHER
OCC4D_INST_HD int id_class(float v, int n_ids) {
  if (v < 0.f) return n_ids;
  if (v < (float)n_ids) {                        // 0 <= v < n_ids (-0.0 included; NaN fails both comparisons)
    const int k = (int)v;
    if ((float)k == v) return k;
  }
  return CLASS_OTHER;
}

OCC4D_INST_HD int64_t frame_confusion(int /*n_ids*/) { return OCC4D_INST_FRAME_HEAD; }
OCC4D_INST_HD int64_t frame_points(int n_ids, int side) {
  return OCC4D_INST_FRAME_HEAD + (int64_t)(n_ids + 1) * (n_ids + 1) + (int64_t)side * n_ids * OCC4D_INST_POINT_WORDS;
}

struct ConfusionArgs {
  const float* density; int64_t ld_density;
  const float* pred_id; int64_t ld_pred; int n;
  const int32_t* nn_idx; const float* nn_dist;
  const float* target_id; int64_t ld_target; int m;
  int n_ids; float threshold, radius;
};

// gt * (n_ids + 1) + pred of query i, or ROW_BAD.  target_id is read only after the range check of nn_idx, and only when the
// label consults it; the cell is built from validated classes only.
OCC4D_INST_HD int confusion_cell(const ConfusionArgs& a, int64_t i) {
  const int j = a.nn_idx[i];
  if (j < 0 || j >= a.m) return ROW_BAD;
  int pred = a.n_ids, gt = a.n_ids;
  if (a.density[i * a.ld_density] >= a.threshold) {
    pred = id_class(a.pred_id[i * a.ld_pred], a.n_ids);
    if (pred == CLASS_OTHER) return ROW_BAD;
  }
  if (a.nn_dist[i] < a.radius) {
    gt = id_class(a.target_id[(int64_t)j * a.ld_target], a.n_ids);
    if (gt == CLASS_OTHER) return ROW_BAD;
  }
  return gt * (a.n_ids + 1) + pred;
}

struct PointArgs {
  const float* rows; int64_t ld; int n;
  const float* id; int64_t ld_id;
  int n_ids;
};

// fixed point, 20 fractional bits; the caller has checked |c| <= 1024 (then the product is an exact double below 2^31)
OCC4D_INST_HD int64_t fixed_point(float c) { return (int64_t)llrint((double)c * 1048576.0); }

// id in [0, n_ids) of row i with q = its fixed-point coordinates, ROW_SKIP (class NONE) or ROW_BAD
OCC4D_INST_HD int point_row(const PointArgs& a, int64_t i, int64_t (&q)[3]) {
  const int c = id_class(a.id[i * a.ld_id], a.n_ids);
  if (c == a.n_ids) return ROW_SKIP;
  if (c == CLASS_OTHER) return ROW_BAD;
  const float* r = a.rows + i * a.ld;
  const float x = r[0], y = r[1], z = r[2];
  if (!(fabsf(x) <= 1024.f && fabsf(y) <= 1024.f && fabsf(z) <= 1024.f)) return ROW_BAD;   // (NaN, +-inf fail)
  q[0] = fixed_point(x);
  q[1] = fixed_point(y);
  q[2] = fixed_point(z);
  return c;
}

// What id i of a frame table adds.  group: -1 = skipped (neither annotated nor predicted), -2 = its group id is out of range.
struct IdTerms {
  int group;
  bool annotated, predicted, match, centroid;
  int64_t inter, uni;
  double iou, d, d2;                 // iou: annotated ids only; d, d2: `centroid` only
};

OCC4D_INST_HD IdTerms fold_id(const int64_t* frame, int n_ids, const int32_t* inst_group, int n_groups, int i) {
  IdTerms t;
  t.group = -1; t.annotated = t.predicted = t.match = t.centroid = false; t.inter = t.uni = 0; t.iou = t.d = t.d2 = 0.0;
  const int C = n_ids + 1;
  const int64_t* conf = frame + frame_confusion(n_ids);
  int64_t gt_q = 0, pr_q = 0;
  for (int c = 0; c < C; ++c) {
    gt_q += conf[(int64_t)i * C + c];
    pr_q += conf[(int64_t)c * C + i];
  }
  t.annotated = gt_q >= 1;
  t.predicted = pr_q >= 1;
  if (!t.annotated && !t.predicted) return t;
  const int g = inst_group ? inst_group[i] : 0;
  if (g < 0 || g >= n_groups) {
    t.group = -2;
    return t;
  }
  t.group = g;
  t.inter = conf[(int64_t)i * C + i];
  t.uni = gt_q + pr_q - t.inter;
  t.match = t.annotated && 2 * t.inter > t.uni;
  if (t.annotated) t.iou = (double)t.inter / (double)t.uni;
  const int64_t* p = frame + frame_points(n_ids, OCC4D_INST_SIDE_PRED) + (int64_t)i * OCC4D_INST_POINT_WORDS;
  const int64_t* q = frame + frame_points(n_ids, OCC4D_INST_SIDE_GT) + (int64_t)i * OCC4D_INST_POINT_WORDS;
  t.centroid = t.annotated && p[OCC4D_INST_POINT_COUNT] >= 1 && q[OCC4D_INST_POINT_COUNT] >= 1;
  if (t.centroid) {
    const double np_ = (double)p[OCC4D_INST_POINT_COUNT], nq = (double)q[OCC4D_INST_POINT_COUNT];
    const double dx = (double)p[OCC4D_INST_POINT_SX] / np_ / 1048576.0 - (double)q[OCC4D_INST_POINT_SX] / nq / 1048576.0;
    const double dy = (double)p[OCC4D_INST_POINT_SY] / np_ / 1048576.0 - (double)q[OCC4D_INST_POINT_SY] / nq / 1048576.0;
    const double dz = (double)p[OCC4D_INST_POINT_SZ] / np_ / 1048576.0 - (double)q[OCC4D_INST_POINT_SZ] / nq / 1048576.0;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;          // (separate roundings: no fused multiply-add)
    t.d2 = xx + yy + zz;
    t.d = sqrt(t.d2);
  }
  return t;
}

// The frame's totals of group g, over the ids ascending, from the per-id terms: c[GROUP_COUNTS], s[GROUP_SUMS] (zeroed here).
// Returns nothing for a group no id is in: zeros.
OCC4D_INST_HD void fold_group(const IdTerms* terms, int n_ids, int g, int64_t* c, double* s) {
  for (int k = 0; k < OCC4D_INST_GROUP_COUNTS; ++k) c[k] = 0;
  for (int k = 0; k < OCC4D_INST_GROUP_SUMS; ++k) s[k] = 0.0;
  for (int i = 0; i < n_ids; ++i) {
    const IdTerms& t = terms[i];
    if (t.group != g) continue;
    c[OCC4D_INST_N_GT] += t.annotated;
    c[OCC4D_INST_N_PRED] += t.predicted;
    c[OCC4D_INST_N_MATCH] += t.match;
    c[OCC4D_INST_SUM_INTER] += t.inter;
    c[OCC4D_INST_SUM_UNION] += t.uni;
    c[OCC4D_INST_N_CENTROID] += t.centroid;
    if (t.annotated) s[OCC4D_INST_SUM_IOU] += t.iou;
    if (t.match) s[OCC4D_INST_SUM_IOU_MATCHED] += t.iou;
    if (t.centroid) {
      s[OCC4D_INST_SUM_CENTROID_D] += t.d;
      s[OCC4D_INST_SUM_CENTROID_D2] += t.d2;
    }
  }
}

// ---- argument contracts (host): the status, `empty` = nothing to do
inline bool ids_ok(int n_ids) { return n_ids >= 1 && n_ids <= OCC4D_INST_MAX_IDS; }
inline bool groups_ok(int n_groups) { return n_groups >= 1 && n_groups <= OCC4D_INST_MAX_GROUPS; }
inline int64_t frame_len(int n_ids) {
  return ids_ok(n_ids) ? frame_points(n_ids, 2) : -1;
}
inline int64_t counts_len(int n_groups) { return groups_ok(n_groups) ? OCC4D_INST_HEAD + (int64_t)n_groups * OCC4D_INST_GROUP_COUNTS : -1; }
inline int64_t sums_len(int n_groups) { return groups_ok(n_groups) ? (int64_t)n_groups * OCC4D_INST_GROUP_SUMS : -1; }

inline int check_confusion(const float* density, int64_t ld_density, const float* pred_id, int64_t ld_pred, int n, const int32_t* nn_idx,
                           const float* nn_dist, const float* target_id, int64_t ld_target, int m, int n_ids, float density_threshold,
                           float radius, const int64_t* frame, bool& empty, ConfusionArgs& a) {
  const char* who = "occ4d_inst_confusion_f32";
  OCC4D_REQUIRE(ids_ok(n_ids), "%s: n_ids = %d must be in 1 .. %d", who, n_ids, OCC4D_INST_MAX_IDS);
  OCC4D_REQUIRE(n >= 0 && m >= 0, "%s: n = %d, m = %d", who, n, m);
  OCC4D_REQUIRE(ld_density >= 1 && ld_pred >= 1 && ld_target >= 1, "%s: ld_density = %lld, ld_pred = %lld, ld_target = %lld must be >= 1", who,
                (long long)ld_density, (long long)ld_pred, (long long)ld_target);
  OCC4D_REQUIRE(frame, "%s: null frame", who);
  empty = n == 0;
  OCC4D_REQUIRE(empty || (density && pred_id && nn_idx && nn_dist && (target_id || m == 0)),
                "%s: null density / pred_id / nn_idx / nn_dist / target_id", who);
  a = ConfusionArgs{density, ld_density, pred_id, ld_pred, n, nn_idx, nn_dist, target_id, ld_target, m, n_ids, density_threshold, radius};
  return OCC4D_OK;
}

inline int check_points(const float* rows, int64_t ld, int n, const float* id, int64_t ld_id, int n_ids, int side, const int64_t* frame,
                        bool& empty, PointArgs& a) {
  const char* who = "occ4d_inst_points_f32";
  OCC4D_REQUIRE(ids_ok(n_ids), "%s: n_ids = %d must be in 1 .. %d", who, n_ids, OCC4D_INST_MAX_IDS);
  OCC4D_REQUIRE(n >= 0, "%s: n = %d", who, n);
  OCC4D_REQUIRE(ld >= 3 && ld_id >= 1, "%s: ld = %lld must be >= 3, ld_id = %lld >= 1", who, (long long)ld, (long long)ld_id);
  OCC4D_REQUIRE(side == OCC4D_INST_SIDE_PRED || side == OCC4D_INST_SIDE_GT, "%s: side = %d must be 0 (predicted) or 1 (ground truth)", who, side);
  OCC4D_REQUIRE(frame, "%s: null frame", who);
  empty = n == 0;
  OCC4D_REQUIRE(empty || (rows && id), "%s: null rows / id", who);
  a = PointArgs{rows, ld, n, id, ld_id, n_ids};
  return OCC4D_OK;
}

inline int check_fold(const int64_t* frame, int n_ids, int n_groups, const int64_t* counts, const double* sums) {
  const char* who = "occ4d_inst_fold";
  OCC4D_REQUIRE(ids_ok(n_ids), "%s: n_ids = %d must be in 1 .. %d", who, n_ids, OCC4D_INST_MAX_IDS);
  OCC4D_REQUIRE(groups_ok(n_groups), "%s: n_groups = %d must be in 1 .. %d", who, n_groups, OCC4D_INST_MAX_GROUPS);
  OCC4D_REQUIRE(frame && counts && sums, "%s: null frame / counts / sums", who);
  return OCC4D_OK;
}

}  // namespace occ4d_inst
