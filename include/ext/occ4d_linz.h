/* occ4d_linz.h -- the decoder's lin_z terms under the trunk kernels' matrix stream (csrc/trunk.hip).
 *
 * Every residual block of the decoder starts with  x += zconst + sum_j zw[:, j] ztab[zidx[:, j], :]  (model/implicit.py:416-417
 * in the exact-in-R form of occ4d_interp_add_f32).  As a pass of its own that is a read-modify-write of the activations six
 * times per mini-batch, and nothing runs beside the matrix kernels; the two entry points here put its memory operations
 * BETWEEN a matrix kernel's MFMAs instead:
 *   occ4d_rowlin_linz_f32       the gathers of up to two terms, software-pipelined through the stages of occ4d_rowlin_f32: the
 *                               first term is added to y, the second is STORED as dense rows;
 *   occ4d_resblock_addrows_f32  occ4d_resblock_f32 that adds such dense rows to its output rows last, from plain row loads
 *                               issued under the last hidden chunk into the registers of relu(x), which are dead by then.
 * Both use the operation order of the stand-alone pass -- s = (..((0 + w0 t0) + w1 t1) + ..) + zconst with separate
 * multiplies and adds, then `+ s` as the last operation on the row -- so a chain built from them equals, bit for bit, the
 * chain of occ4d_rowlin_f32 / occ4d_resblock_f32 launches with occ4d_interp_add_f32 passes between them.
 *
 * A header of include/ext/, a row of _lib.ADDON_HEADERS.  The conventions of occ4d.h: extern "C", int status (OCC4D_OK /
 * OCC4D_EINVAL / OCC4D_ELAUNCH), message through occ4d_last_error(), device pointers, the stream as void*, no allocation, no
 * synchronisation.  The symbols live in libocc4d.so only: the g++ twin's decoder is its own loop nest. */
#ifndef OCC4D_LINZ_H_
#define OCC4D_LINZ_H_

#include "occ4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A `flags` bit of the decoder's path-level forwards (beside OCC4D_PATH_* of occ4d.h, whose table is closed): every lin_z term
 * as the stand-alone occ4d_interp_add_f32 pass in front of its block -- the A/B partner of the default routing, which
 * (fp32 row-resident trunk only) adds the term of a block that directly follows a cross layer inside that layer's post
 * Linear, and has that launch store the term of the block after it as dense rows, which the block between adds.  Same
 * results bit for bit; the default's workspace holds one (rows, d_hidden) slice more per mini-batch (the query function is
 * given the same flags). */
#define OCC4D_LINZ_PATH_STANDALONE 512

/* y[:, 0..n_out) = ([res +] W [relu](x) + b) + s1,   dense[:, 0..n_out) = s2,   with, for t = 1, 2,
 *   s_t[i, :] = (..((0 + zw[i, 0] T_t[zidx[i, 0], :]) + zw[i, 1] T_t[zidx[i, 1], :]) + ..) + C_t[:]
 * over (T_1, C_1) = (ztab, zconst) and (T_2, C_2) = (ztab2, zconst2): both tables have zrows rows of stride ldz (ldz % 4 == 0,
 * ldz >= n_out, 16-byte aligned; zrows ldz < 2^30: 32-bit row offsets) and share the lists zidx (n, kz), entries in
 * [0, zrows), and weights zw (n, kz).  Either term may be absent (table and
 * constant NULL), not both; without the second, dense must be NULL.  kz must be 8: the kernel keeps a row's list in
 * registers (any other count: occ4d_rowlin_f32, then occ4d_interp_add_f32).  dense (n, n_out; row stride ldd, ldd % 4 == 0,
 * 16-byte aligned) must not overlap x, y or res.  y equals occ4d_rowlin_f32 followed by occ4d_interp_add_f32 bit for bit,
 * dense equals occ4d_interp_add_f32 applied to zero rows.  Everything else as occ4d_rowlin_f32 (occ4d.h): K = 416,
 * n_out % 32 == 0, w_packed in the "rows" packing, res may alias y.  Table indices are not checked. */
int occ4d_rowlin_linz_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed, const float* b,
                          int n_out, int relu_in, const float* res, int64_t ldr, const float* zconst, const float* ztab,
                          const float* zconst2, const float* ztab2, int64_t ldz, int zrows, const int32_t* zidx,
                          const float* zw, int kz, float* dense, int64_t ldd, int n, void* stream);

/* y = (x + W1 relu(W0 relu(x) + b0) + b1) + addrows: occ4d_resblock_f32 (occ4d.h; same packings and alignments) followed by an
 * fp32 row add, bit for bit, in one launch.  addrows (n, 416; row stride ld_add, ld_add % 4 == 0, 16-byte aligned) must not
 * overlap y (y may alias x as before); n ld_add < 2^30 (32-bit row offsets: chunk the rows). */
int occ4d_resblock_addrows_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w0_packed, const float* b0,
                               const float* w1_packed, const float* b1, const float* addrows, int64_t ld_add, int n,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCC4D_LINZ_H_ */
