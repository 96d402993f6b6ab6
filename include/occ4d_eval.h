/* occ4d_eval.h -- per-frame evaluation statistics of the decoded queries against a ground-truth frame, on the device.
 *
 * A third header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned) and occ4d_frontend.h: the same
 * conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * The statistics are ADDITIVE: two arrays, `counts` (int64) and `sums` (double), that every call adds onto.  Arrays of the
 * same (n_groups, n_classes) sum element-wise across frames, clips and ranks; the figures (precision, IoU, chamfer, ...)
 * are formed from the totals by the caller.  A fresh pair is all zeros.
 *
 * counts: OCC4D_EVAL_HEAD global words, then per group g a block of OCC4D_EVAL_GROUP_COUNTS + n_classes^2 words:
 *   counts[OCC4D_EVAL_BAD_ROWS]                                      rows skipped: nn_idx outside [0, m) or group id outside [0, n_groups)
 *   counts[OCC4D_EVAL_HEAD + g * stride + OCC4D_EVAL_<NAME>]         the scalar counts below, stride = GROUP_COUNTS + n_classes^2
 *   counts[OCC4D_EVAL_HEAD + g * stride + GROUP_COUNTS + r * C + c]  segmentation confusion: r = the target's tag, c = the prediction
 * sums: per group g a block of OCC4D_EVAL_GROUP_SUMS doubles, sums[g * GROUP_SUMS + OCC4D_EVAL_SUM_<NAME>].
 *
 * Reproducibility: the counts are integers (order-free).  Every term of a sum is formed in double from fp32 inputs; the
 * terms are added per thread, per wave, per workgroup and over the workgroups in a fixed order, on a grid that depends on
 * the row count alone: the same call on the same arrays gives the same bits on any device.  No floating-point atomics. */
#ifndef OCC4D_EVAL_H
#define OCC4D_EVAL_H

#include <stdint.h>

#define OCC4D_EVAL_MAX_GROUPS 8
#define OCC4D_EVAL_MAX_CLASSES 32

#define OCC4D_EVAL_HEAD 1
#define OCC4D_EVAL_BAD_ROWS 0

#define OCC4D_EVAL_GROUP_COUNTS 16
#define OCC4D_EVAL_OCC_TP 0
#define OCC4D_EVAL_OCC_FP 1
#define OCC4D_EVAL_OCC_FN 2
#define OCC4D_EVAL_OCC_TN 3
#define OCC4D_EVAL_TRACK_TP 4
#define OCC4D_EVAL_TRACK_FP 5
#define OCC4D_EVAL_TRACK_FN 6
#define OCC4D_EVAL_TRACK_TN 7
#define OCC4D_EVAL_SEG_IGNORED 8
#define OCC4D_EVAL_N_ACCURACY 9
#define OCC4D_EVAL_N_COMPLETENESS 10
#define OCC4D_EVAL_N_COLOR 11
#define OCC4D_EVAL_N_SEG 12

#define OCC4D_EVAL_GROUP_SUMS 8
#define OCC4D_EVAL_SUM_ACCURACY_D 0
#define OCC4D_EVAL_SUM_ACCURACY_D2 1
#define OCC4D_EVAL_SUM_COMPLETENESS_D 2
#define OCC4D_EVAL_SUM_COMPLETENESS_D2 3
#define OCC4D_EVAL_SUM_COLOR_L1 4

/* flags: which optional statistics a call scores (each also needs its target column, see below) */
#define OCC4D_EVAL_FLAG_COLOR 1
#define OCC4D_EVAL_FLAG_TRACK 2
#define OCC4D_EVAL_FLAG_SEG 4

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  Length of `counts` (int64 words) / of `sums` (doubles) for 1 <= n_groups <= 8, 0 <= n_classes <= 32;
 * -1 for arguments outside that. */
int64_t occ4d_eval_counts_len(int n_groups, int n_classes);
int64_t occ4d_eval_sums_len(int n_groups);

/* Host only.  Bytes of `workspace` for a call over n rows (either entry point; -1 for n < 0).  8-byte aligned. */
int64_t occ4d_eval_workspace_bytes(int n);

/* One pass over the n decoded queries of a frame.
 *   out (n, g_out), row stride ldo: the squashed implicit output; channel 0 is the density;
 *   nn_idx (n), nn_dist (n): the nearest target point of every query and its Euclidean distance;
 *   target (m, dt), row stride ldt: the ground-truth frame;
 *   col_rgb, col_track, col_sem: target columns of R (G, B follow), mark_track and the semantic tag; -1 = absent;
 *   out_track: output channel of mark_track (read only when tracking is scored);
 *   target_group (m) or null (every point in group 0): the query's group is that of its nearest target point.
 * A query is predicted solid when out[0] >= density_threshold (fp32), its label is nn_dist < radius (fp32).
 *   occupancy TP / FP / FN / TN: prediction against label; N_ACCURACY, SUM_ACCURACY_D / _D2: d, d^2 of nn_dist over the
 *     predicted-solid queries.
 * Over the occupancy-TP queries:
 *   FLAG_COLOR and col_rgb >= 0: N_COLOR, SUM_COLOR_L1 = |out[1] - R| + |out[2] - G| + |out[3] - B|;
 *   FLAG_TRACK and col_track >= 0: out[out_track] >= 0.5 against target[col_track] > 0.5;
 *   FLAG_SEG, col_sem >= 0 and n_classes >= 1: confusion[tag][first argmax of out's last n_classes channels], N_SEG; a tag
 *     that is no integer in [0, n_classes) counts in SEG_IGNORED instead.
 * A row whose nn_idx is outside [0, m) or whose group id is outside [0, n_groups) adds 1 to BAD_ROWS and nothing else.
 * n = 0 is a no-op.  n_classes fixes the layout of `counts` also where segmentation is not scored. */
int occ4d_eval_query_stats_f32(const float* out, int64_t ldo, int n, int g_out, const int32_t* nn_idx, const float* nn_dist,
                               const float* target, int64_t ldt, int m, int dt, int col_rgb, int col_track, int col_sem,
                               int out_track, const int32_t* target_group, int n_groups, int n_classes,
                               float density_threshold, float radius, int flags, int64_t* counts, double* sums,
                               void* workspace, void* stream);

/* Completeness: dist (m) = the distance of every target point to the nearest predicted-solid query; per group (the
 * point's own, target_group (m) or null) N_COMPLETENESS, SUM_COMPLETENESS_D / _D2.  A group id outside [0, n_groups)
 * adds 1 to BAD_ROWS and nothing else. */
int occ4d_eval_target_stats_f32(const float* dist, int m, const int32_t* target_group, int n_groups, int n_classes,
                                int64_t* counts, double* sums, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
