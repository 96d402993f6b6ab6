/* occ4d_track.h -- the merge of the per-instance reruns of track_mode 'all' (inference.multi_track_merge), on the device.
 *
 * A fifth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned), occ4d_frontend.h, occ4d_eval.h and
 * occ4d_occl.h: the same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message
 * through occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * The merge is a RUNNING one: one (n, g) accumulator and two (n) columns stand in for the K arrays of the host merge.
 *     acc = run_0;  acc += run_k  (k = 1 .. K - 1, in rerun order, fp32);  acc /= (float)K  (IEEE division)
 *     winner = -1, best = 0;  for every rerun in order, on the track column's squashed score s:
 *         if (s >= 0.5 && s >= best) winner = inst_id;      (a tie goes to the later rerun)
 *         best = max(s, best), NaN-propagating              (after a NaN score no later rerun wins that row)
 * which equals numpy's mean over the stacked reruns and the reference's winner loop bit for bit (utils/utils.py:343-397).
 * The kernels index nothing by data: no value in any array can move an access. */
#ifndef OCC4D_TRACK_H
#define OCC4D_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One rerun onto the running merge.
 *   out (n, g), row stride ld_out >= g: the rerun's RAW outputs; read only;
 *   ops_host: g codes of occ4d_squash_f32 on the HOST (0 identity, 1 sigmoid, 2 clamp to [0, 1]), or null = all identity.
 *     v = squash(out[i][c]) is the very expression of occ4d_squash_f32: squash-then-merge equals this fused pass bit for bit;
 *   track_col in [0, g): the channel of the tracking score, or -1: no track column (best / winner are not touched and may
 *     be null; they may be null ONLY then);
 *   inst_id: the id this rerun followed, as a float;
 *   first = 1: acc[i][c] = v and the row starts from best = 0, winner = -1 (nothing is read from acc / best / winner: no
 *     memset is needed, and -0 stays -0);  first = 0: acc[i][c] += v;
 *   acc (n, g), row stride ld_acc >= g; best (n); winner (n).  Columns g .. ld - 1 of a row are never touched.
 * 1 <= g <= 32.  n = 0 is a no-op. */
int occ4d_track_merge_add_f32(const float* out, int64_t ld_out, int n, int g, const int32_t* ops_host, int track_col,
                              float inst_id, int first, float* acc, int64_t ld_acc, float* best, float* winner, void* stream);

/* The end of the merge, in place: acc[i][c] = acc[i][c] / (float)n_runs (correctly rounded fp32 division, never a reciprocal
 * multiply), then acc[i][track_col] = winner[i] when track_col >= 0 (winner may be null only when track_col == -1).
 * 1 <= g <= 32, n_runs >= 1.  n = 0 is a no-op. */
int occ4d_track_merge_finish_f32(float* acc, int64_t ld_acc, int n, int g, int n_runs, int track_col, const float* winner,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif
