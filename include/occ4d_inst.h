/* occ4d_inst.h -- instance-level scoring of a dense instance labelling (perform_inference, track_mode 'all': after the merge
 * the mark_track channel of a query holds the id of the most confident rerun, or -1) against a ground-truth frame, on the device:
 * per-instance IoU, panoptic quality and centroids.
 *
 * A seventh header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned) and the other feature headers: the same
 * conventions as occ4d_eval.h -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * Classes.  For n_ids instance ids there are n_ids + 1 classes; class n_ids is NONE (air, background, unlabelled).  A float v is
 *   class i   when v equals an integer i in [0, n_ids) as fp32 (-0.0 counts as 0),
 *   NONE      when v < 0,
 *   OTHER     in every other case (non-integral, >= n_ids, NaN, +inf): the row that consults it is a bad row.
 *
 * The frame table, int64_t frame[occ4d_inst_frame_len(n_ids)], zero-filled by the caller before a frame, with C = n_ids + 1:
 *   frame[OCC4D_INST_BAD_ROWS]                                                      rows skipped
 *   frame[OCC4D_INST_FRAME_HEAD + gt * C + pred]                                    the confusion: row = ground truth, column = prediction
 *   frame[OCC4D_INST_FRAME_HEAD + C * C + (side * n_ids + i) * OCC4D_INST_POINT_WORDS + OCC4D_INST_POINT_<COUNT | SX | SY | SZ>]
 *                                                                                   the points of id i: side OCC4D_INST_SIDE_PRED / _GT
 * The coordinate sums are fixed point with 20 fractional bits, llrint((double)coord * 1048576.0): exact for every fp32 with
 * |coord| <= 1024, and integer sums are order-free.
 *
 * The statistics are ADDITIVE: `counts` (int64) and `sums` (double), that occ4d_inst_fold adds a frame table onto.
 *   counts[OCC4D_INST_BAD_ROWS]                                                        the frames' bad rows, and ids whose group is outside [0, n_groups)
 *   counts[OCC4D_INST_HEAD + g * OCC4D_INST_GROUP_COUNTS + OCC4D_INST_<N_GT ...>]     per group g
 *   sums[g * OCC4D_INST_GROUP_SUMS + OCC4D_INST_SUM_<IOU ...>]                        per group g
 * Arrays of the same n_groups sum element-wise across frames, clips and ranks; a fresh pair is all zeros. */
#ifndef OCC4D_INST_H
#define OCC4D_INST_H

#include <stdint.h>

#define OCC4D_INST_MAX_IDS 64
#define OCC4D_INST_MAX_GROUPS 8

#define OCC4D_INST_BAD_ROWS 0

#define OCC4D_INST_FRAME_HEAD 1
#define OCC4D_INST_POINT_WORDS 4
#define OCC4D_INST_POINT_COUNT 0
#define OCC4D_INST_POINT_SX 1
#define OCC4D_INST_POINT_SY 2
#define OCC4D_INST_POINT_SZ 3
#define OCC4D_INST_SIDE_PRED 0
#define OCC4D_INST_SIDE_GT 1
#define OCC4D_INST_FRACTION_BITS 20

#define OCC4D_INST_HEAD 1
#define OCC4D_INST_GROUP_COUNTS 8
#define OCC4D_INST_N_GT 0
#define OCC4D_INST_N_PRED 1
#define OCC4D_INST_N_MATCH 2
#define OCC4D_INST_SUM_INTER 3
#define OCC4D_INST_SUM_UNION 4
#define OCC4D_INST_N_CENTROID 5

#define OCC4D_INST_GROUP_SUMS 4
#define OCC4D_INST_SUM_IOU 0
#define OCC4D_INST_SUM_IOU_MATCHED 1
#define OCC4D_INST_SUM_CENTROID_D 2
#define OCC4D_INST_SUM_CENTROID_D2 3

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  Length of `frame` (int64 words) for 1 <= n_ids <= 64, of `counts` (int64 words) / `sums` (doubles) for
 * 1 <= n_groups <= 8; -1 for an argument outside that. */
int64_t occ4d_inst_frame_len(int n_ids);
int64_t occ4d_inst_counts_len(int n_groups);
int64_t occ4d_inst_sums_len(int n_groups);

/* One pass over ALL n queries of a frame (not only the occupancy hits: an instance the geometry misses costs IoU).
 *   density (n), element stride ld_density: the squashed density of every query;
 *   pred_id (n), element stride ld_pred: its predicted instance id (the merged mark_track channel);
 *   nn_idx (n), nn_dist (n): the nearest target point of every query and its Euclidean distance;
 *   target_id (m), element stride ld_target: the instance id of every target point.
 * Prediction class: density >= density_threshold ? class(pred_id) : NONE.  Ground-truth class: nn_dist < radius ?
 * class(target_id[nn_idx]) : NONE.  Both comparisons are fp32.  confusion[gt][pred] += 1.
 * A row adds 1 to BAD_ROWS and nothing else when nn_idx is outside [0, m), or when a class that is consulted is OTHER.
 * n = 0 is a no-op. */
int occ4d_inst_confusion_f32(const float* density, int64_t ld_density, const float* pred_id, int64_t ld_pred, int n,
                             const int32_t* nn_idx, const float* nn_dist, const float* target_id, int64_t ld_target, int m,
                             int n_ids, float density_threshold, float radius, int64_t* frame, void* stream);

/* The points of every instance: rows (n, >= 3), row stride ld, x y z first; id (n), element stride ld_id.  side:
 * OCC4D_INST_SIDE_PRED (the predicted-solid rows) or OCC4D_INST_SIDE_GT (the target frame's rows).
 * A row of class i < n_ids adds count += 1 and s{x,y,z} += llrint((double)coord * 1048576.0) to entry i of that side.
 * A row of class NONE is skipped silently (its coordinates are not looked at).  A row of class OTHER, or with a non-finite
 * coordinate or |coord| > 1024, adds 1 to BAD_ROWS and nothing else.  n = 0 is a no-op. */
int occ4d_inst_points_f32(const float* rows, int64_t ld, int n, const float* id, int64_t ld_id, int n_ids, int side,
                          int64_t* frame, void* stream);

/* Adds one frame table onto the running `counts` / `sums`; `frame` is left untouched.  inst_group (n_ids) or null (every id
 * in group 0).  Per id i: gt_q = row sum, pr_q = column sum of the confusion, inter = confusion[i][i], union = gt_q + pr_q -
 * inter; annotated: gt_q >= 1, predicted: pr_q >= 1.  An id that is neither is skipped; an id whose group is outside
 * [0, n_groups) adds 1 to counts[BAD_ROWS] and is skipped.  Per group:
 *   N_GT, N_PRED: the annotated / predicted ids; N_MATCH: annotated and 2 * inter > union (IoU > 0.5, in integers);
 *   SUM_INTER, SUM_UNION over the annotated or predicted ids;
 *   SUM_IOU over the annotated ids, each term (double)inter / (double)union; SUM_IOU_MATCHED over the matched ones;
 *   N_CENTROID: annotated and both point tables have count >= 1; SUM_CENTROID_D / _D2 over those: the centroid per coordinate
 *     is (double)s / (double)count / 1048576.0, d2 = dx*dx + dy*dy + dz*dz without fused multiply-add, d = sqrt(d2).
 * The frame's total per sum is formed first, over the ids ascending, and added onto the running value once: two identical
 * calls give identical bits, and one frame added twice onto zeros doubles every entry exactly.  frame[BAD_ROWS] is added to
 * counts[BAD_ROWS]. */
int occ4d_inst_fold(const int64_t* frame, int n_ids, const int32_t* inst_group, int n_groups, int64_t* counts, double* sums,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif
