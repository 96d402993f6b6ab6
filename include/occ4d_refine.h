/* occ4d_refine.h -- one-level coarse-to-fine decode of the dense query grid (inference.perform_inference(refine=...)): which
 * grid points are decoded at all, and the dense (N, G) output rebuilt from the decoded ones.
 *
 * An eighth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned) and the other feature headers: the same
 * conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * The grid is the flat one of occ4d_grid_points_f32: (nx, ny, nz) points, x slowest, z fastest.  With a block edge b:
 *     nb_axis = ceil(n_axis / b) blocks per axis (edge blocks are clipped);  point (ix, iy, iz) lies in block
 *     (ix / b, iy / b, iz / b), whose flat index is (bx * nby + by) * nbz + bz;  the block's REPRESENTATIVE is the grid point
 *     with per-axis index min(b_axis * b + b / 2, n_axis - 1).
 *     hot(block)      = !(squash(rep_density[block], op) < low)   in fp32: a NaN is hot
 *     active(block)   = any block within Chebyshev distance `dilate` (clipped at the grid's faces) is hot
 *     selected(point) = its block is active and the point is not the block's representative
 * The caller decodes the representatives, marks, compacts the selected query rows in grid order (occ4d_compact_count_f32 /
 * occ4d_compact_rows_f32 of occ4d.h over `key` with threshold 0.5, strict), decodes those, and expands.
 * Limits of both entry points: 2 <= b <= 8, nx, ny, nz >= 0 with nx * ny * nz <= INT32_MAX; an empty grid is a no-op.
 * No array is indexed by data, but for one guarded position in the expansion (below). */
#ifndef OCC4D_REFINE_H
#define OCC4D_REFINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The mark.
 *   rep_density: one value per block in flat block order, element stride ld_rep >= 1 (a column of the representatives' output
 *     rows): RAW or squashed;
 *   op: a code of occ4d_squash_f32 (0 identity, 1 sigmoid, 2 clamp to [0, 1]), applied to the value before the comparison with
 *     the very expression of occ4d_squash_f32: mark-on-raw equals squash-then-mark bit for bit;
 *   0 <= dilate <= 2;
 *   active (nbx * nby * nbz) int32: written 0 / 1;  key (nx * ny * nz): written 1.0f (selected) / 0.0f.
 * Two launches: blocks -> active, then points -> key. */
int occ4d_refine_mark_f32(const float* rep_density, int64_t ld_rep, int nx, int ny, int nz, int b, int dilate, int op, float low,
                          int32_t* active, float* key, void* stream);

/* The expansion to the dense (nx * ny * nz, g) array `out`, row stride ld_out >= g, in one pass:
 *     a selected row (key > 0.5f) takes row p of fine_out, p = block_offsets[i / 256] + its rank among the selected rows of its
 *     256-row tile;  every other row, the representative included, takes row block(i) of rep_out.
 *   key: as occ4d_refine_mark_f32 wrote it;  block_offsets (ceil(n / 256)): the exclusive prefix occ4d_compact_count_f32 left
 *     for that key (what occ4d_compact_rows_f32 takes);
 *   rep_out (blocks, g), row stride ld_rep >= g;  fine_out (n_fine, g), row stride ld_fine >= g, may be null when n_fine == 0.
 * p is the only data-dependent position.  It is used only when 0 <= p < n_fine; a selected row whose p is outside takes its
 * block's representative row instead: whatever block_offsets holds, nothing outside fine_out's n_fine rows is read.
 * 1 <= g <= 32.  Columns g .. ld_out - 1 of a row are never touched. */
int occ4d_refine_expand_f32(const float* key, const int32_t* block_offsets, const float* rep_out, int64_t ld_rep,
                            const float* fine_out, int64_t ld_fine, int n_fine, int nx, int ny, int nz, int b, int g, float* out,
                            int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
