/* occ4d_prelude.h -- the decoder's query prelude: the part of occ4d_decoder_query_fwd_f32 (occ4d.h) that needs only the
 * abstract cloud's COORDINATES and the raw weights, split off so that a caller can run it for all the queries of a step
 * beside the encoder, and the forward call that takes its results.
 *
 * The second header of include/ext/ (occ4d.h's symbol set and OCC4D_ABI_VERSION are pinned, the list of feature headers is
 * closed, and so is the table of ext/occ4d_raycast.h): its prototypes take occ4d.h's structs, so it is a row of
 * _lib.STRUCT_EXTENSION_HEADERS; include it as "ext/occ4d_prelude.h".  The conventions of occ4d.h: extern "C", int status,
 * message through occ4d_last_error(), device pointers, the stream as void*, no allocation, no synchronisation.  The symbols
 * live in libocc4d.so (csrc/path.hip) and in the g++ twin; the argument contracts are written once for both
 * (csrc/decoder_math.hpp). */
#ifndef OCC4D_PRELUDE_H_
#define OCC4D_PRELUDE_H_

#include "occ4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For ALL n queries (n, d_in; row stride q_stride), every kernel launched once (pieces of 2^22 rows): the k_local nearest
 * abstract points by Euclidean norm -> idx_local (n, k_local) and their normalised inverse-distance weights w_local (n,
 * k_local); the k_cross nearest by squared distance -> idx_cross (n, k_cross; NULL allowed when n_cross == 0); and, with
 * x0 != NULL, x0 (n, d_hidden; row stride ld_x0, ld_x0 % 4 == 0, 16-byte aligned) = lin_in(posenc(queries)).  x0 == NULL:
 * lists and weights only.  xyz (m, 3) packed.  Neither `prepared` nor `scene` is needed.  Row i depends on query i alone and
 * is bit for bit what occ4d_decoder_query_fwd_f32 computes for that query when it searches itself.  workspace:
 * occ4d_decoder_query_prelude_workspace_floats(w, n, with_x0) floats, 16-byte aligned (unused, may be NULL, without x0). */
int64_t occ4d_decoder_query_prelude_workspace_floats(const occ4d_decoder_weights* w, int n, int with_x0);
int occ4d_decoder_query_prelude_f32(const occ4d_decoder_weights* w, const float* xyz, int m, const float* queries,
                                    int64_t q_stride, int n, int32_t* idx_local, float* w_local, int32_t* idx_cross,
                                    float* x0, int64_t ld_x0, float* workspace, void* stream);

/* occ4d_decoder_query_fwd_f32 for n queries whose prelude rows exist: idx_local / w_local / idx_cross are the prelude's
 * rows OF THESE QUERIES (row 0 belongs to queries row 0; used as they are, not clamped: the prelude wrote them for this very
 * cloud of m points), and the searches, the weights and -- with x0 -- the Fourier features and lin_in are not launched.
 * x0 (n, d_hidden; ld_x0) or NULL: the prelude's lin_in rows of these queries; they serve IN PLACE as the trunk's
 * activation buffer and hold no defined values afterwards (with penult != NULL they are copied there first and stay
 * intact).  Everything else, the workspace size included (occ4d_decoder_query_workspace_floats), as
 * occ4d_decoder_query_fwd_f32; `out` is bit-identical to that call's without caller-supplied lists. */
int occ4d_decoder_query_fwd_prelude_f32(const occ4d_decoder_weights* w, const float* prepared, const float* scene, int m,
                                        const float* queries, int64_t q_stride, int n, const int32_t* idx_local,
                                        const float* w_local, const int32_t* idx_cross, float* x0, int64_t ld_x0, float* out,
                                        int64_t ld_out, float* penult, int64_t ld_pen, float* workspace, int flags,
                                        occ4d_launch_events* ev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCC4D_PRELUDE_H_ */
