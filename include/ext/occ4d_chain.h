/* occ4d_chain.h -- consecutive residual blocks of the decoder trunk as one launch (csrc/trunk.hip).
 *
 * Between two residual blocks that no cross layer separates nothing happens to a row but the next block's lin_z term.  As
 * launches of their own each block loads its (rows, 416) activations before its first MFMA and stores them after its last,
 * and every CU of the single round of workgroups is in that memory phase at the same time.  The entry points here remove
 * the phases instead of hiding them:
 *   occ4d_resblock_chain_f32   up to three residual blocks over the same rows, the rows in registers from the first block's
 *                              load to the last block's store; a block's dense rows (the contract of
 *                              occ4d_resblock_addrows_f32, occ4d_linz.h) are added in registers at the boundary; optionally
 *                              the "rows"-packed Linear that follows (a cross layer's query projection) in the same launch;
 *   occ4d_interp_dense_f32     the lin_z terms of such a run of blocks in ONE pass over the lists and weights: the first is
 *                              added to x in place, the others are stored as the dense rows the chain adds.
 * The loop bodies, and with them every accumulation order, are those of occ4d_resblock_f32 / occ4d_resblock_addrows_f32 /
 * occ4d_rowlin_f32 / occ4d_interp_add_f32: a chain equals, bit for bit, the launches it replaces.
 *
 * A header of include/ext/, a row of _lib.ADDON_HEADERS.  The conventions of occ4d.h: extern "C", int status (OCC4D_OK /
 * OCC4D_EINVAL / OCC4D_ELAUNCH), message through occ4d_last_error(), device pointers, the stream as void*, no allocation, no
 * synchronisation.  The symbols live in libocc4d.so only: the g++ twin's decoder is its own loop nest. */
#ifndef OCC4D_CHAIN_H_
#define OCC4D_CHAIN_H_

#include "occ4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A `flags` bit of the decoder's path-level forwards (beside OCC4D_PATH_* of occ4d.h and OCC4D_LINZ_PATH_STANDALONE): every
 * residual block as a launch of its own, every leading lin_z term as the stand-alone pass in front of its block -- the
 * launch sequence before this header, the A/B partner of the default routing (fp32 row-resident trunk, where the lin_z
 * terms are routed at all: maximal runs of blocks with no cross layer between them run as chains of at most three).  Same
 * results bit for bit; the workspace query is given the same flags. */
#define OCC4D_CHAIN_PATH_SEPARATE 1024

/* For i = 0 .. nb - 1 (nb = 1, 2 or 3):   x <- (x + W1_i relu(W0_i relu(x) + b0_i) + b1_i) [+ add_i],   then y = x, and with
 * a tail   y_tail[:, 0..n_tail) = W_tail [relu](x) + b_tail.
 * Block i: w0_i / w1_i in the "rows" / "cols" packing of occ4d_resblock_f32, b0_i / b1_i (416), all 16-byte aligned; add_i
 * NULL or dense rows (n, 416; row stride lda_i, lda_i % 4 == 0, 16-byte aligned, n lda_i < 2^30) that overlap neither y nor
 * y_tail.  The arguments of blocks nb .. 2 are ignored.  x, y: (n, 416), row strides % 4 == 0, 16-byte aligned; y may alias x.
 * Tail (w_tail NULL: none, then b_tail / y_tail must be NULL): w_tail in the "rows" packing for n_tail outputs, n_tail % 32
 * == 0, ld_tail >= n_tail, ld_tail % 4 == 0; y_tail overlaps neither x nor y.
 * y equals the nb launches of occ4d_resblock_f32 / occ4d_resblock_addrows_f32 bit for bit, y_tail equals occ4d_rowlin_f32 on
 * that y. */
int occ4d_resblock_chain_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int nb,
                             const float* w0_0, const float* b0_0, const float* w1_0, const float* b1_0, const float* add_0, int64_t lda_0,
                             const float* w0_1, const float* b0_1, const float* w1_1, const float* b1_1, const float* add_1, int64_t lda_1,
                             const float* w0_2, const float* b0_2, const float* w1_2, const float* b1_2, const float* add_2, int64_t lda_2,
                             const float* w_tail, const float* b_tail, int n_tail, int relu_in_tail, float* y_tail,
                             int64_t ld_tail, int n, void* stream);

/* With s_t[i, :] = (..((0 + zw[i, 0] T_t[zidx[i, 0], :]) + zw[i, 1] T_t[zidx[i, 1], :]) + ..) + C_t[:] for the terms
 * (T_t, C_t) = (ztab_t, zconst_t), t = 0, 1, 2:   x += s_0,   dense1 = s_1,   dense2 = s_2.
 * A term is absent where its table is NULL (then its constant, and for t = 1, 2 its dense rows, must be NULL too; without
 * term 0, x must be NULL); at least one is present.  The tables have zrows rows of d floats with the common row stride ldz
 * (ldz % 4 == 0, ldz >= d, 16-byte aligned; zrows ldz < 2^30: 32-bit row offsets) and share the lists zidx (n, kz), entries
 * in [0, zrows), and weights zw (n, kz), which are read once per row.  kz must be 8 (any other count: occ4d_interp_add_f32
 * per term).  d % 4 == 0; x (row stride ldx) and the dense rows (ldd1, ldd2): row strides % 4 == 0 and >= d, 16-byte aligned,
 * no two of them overlapping.  x equals occ4d_interp_add_f32 with term 0, dense_t equals occ4d_interp_add_f32 applied to zero
 * rows, bit for bit.  Table indices are not checked. */
int occ4d_interp_dense_f32(float* x, int64_t ldx, const float* zconst0, const float* ztab0, const float* zconst1,
                           const float* ztab1, float* dense1, int64_t ldd1, const float* zconst2, const float* ztab2,
                           float* dense2, int64_t ldd2, int64_t ldz, int zrows, const int32_t* zidx, const float* zw, int kz,
                           int n, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCC4D_CHAIN_H_ */
