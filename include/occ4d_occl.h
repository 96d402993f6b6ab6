/* occ4d_occl.h -- per-instance point counts for the live occlusion fractions (occlusion.valo_ids), on the device.
 *
 * A fourth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned), occ4d_frontend.h and occ4d_eval.h:
 * the same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation.  The symbol lives in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * The counts are int32 and ADDITIVE: every call adds onto `counts`; a fresh array is all zeros.  Integer addition makes
 * the result independent of scheduling: no floating-point atomics, nothing order-dependent. */
#ifndef OCC4D_OCCL_H
#define OCC4D_OCCL_H

#include <stdint.h>

#define OCC4D_OCCL_MAX_IDS 4096   /* bins of the workgroup's private table: 16 KB of LDS */
#define OCC4D_OCCL_EXTRA_BINS 2   /* a row of `counts` has n_ids + 2 words */
#define OCC4D_OCCL_NEGATIVE 0     /* bin n_ids + 0: values < 0 (-inf included) */
#define OCC4D_OCCL_OTHER 1        /* bin n_ids + 1: everything else (non-integral, >= n_ids, NaN, +inf) */

#ifdef __cplusplus
extern "C" {
#endif

/* Segmented histogram of column `col` of the row-strided fp32 array rows (n, > col), row stride ld.
 *   seg_offsets (n_segments + 1) int64 on the device, ascending, seg_offsets[0] = 0, seg_offsets[n_segments] = n: rows
 *     seg_offsets[s] .. seg_offsets[s + 1] - 1 are segment s (a frame); empty segments are allowed.  The HIP library
 *     cannot see the offsets and never reads outside `rows` / `counts` whatever they hold; the twin rejects offsets that
 *     do not ascend from 0 to n;
 *   key (n) or null: a row counts only when key > 0.5 (the compaction's keep key); null = every row;
 *   pred_col >= 0: a row counts only when rows[pred_col] == pred_a || rows[pred_col] == pred_b (fp32 ==); -1 = off;
 *   counts (n_segments, n_ids + 2) int32, contiguous: counts[s][i] += rows of segment s whose value compares equal to the
 *     integer i as fp32 (-0.0 is in bin 0); counts[s][n_ids + OCC4D_OCCL_NEGATIVE] += values < 0;
 *     counts[s][n_ids + OCC4D_OCCL_OTHER] += every other counted row.
 * 1 <= n_ids <= OCC4D_OCCL_MAX_IDS, 0 <= col < ld, -1 <= pred_col < ld.  n = 0 or n_segments = 0 is a no-op. */
int occ4d_id_histogram_f32(const float* rows, int64_t ld, int n, int col, const int64_t* seg_offsets, int n_segments,
                           int n_ids, const float* key, int pred_col, float pred_a, float pred_b, int32_t* counts,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif
