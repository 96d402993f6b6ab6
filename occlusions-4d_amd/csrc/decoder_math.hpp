// Argument contracts of the decoder's query prelude (include/ext/occ4d_prelude.h: occ4d_decoder_query_prelude_f32,
// occ4d_decoder_query_fwd_prelude_f32), written once for libocc4d.so (csrc/path.hip) and the g++ twin
// (csrc_cpu/occ4d_twin.cpp): host-only, no HIP in here.  The weights struct itself is checked by each library's own
// check_decoder before these run.
#pragma once
#include <stdint.h>

#include "contract.hpp"
#include "ext/occ4d_prelude.h"

namespace occ4d_decoder {

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// Rows per pass of the prelude: its launches cover all n rows at once up to here (the element grids of the Fourier-feature
// and row-fill kernels, n * lin_in_ld threads, stay far below 2^31)
constexpr int PRELUDE_ROWS = 1 << 22;

// n == 0 is legal (nothing to do): `empty` tells the caller to return OCC4D_OK right away
inline int check_query_prelude(const occ4d_decoder_weights* w, const float* xyz, int m, const float* queries, int64_t q_stride,
                               int n, const int32_t* idx_local, const float* w_local, const int32_t* idx_cross, const float* x0,
                               int64_t ld_x0, const float* workspace, bool* empty) {
  const char* who = "occ4d_decoder_query_prelude_f32";
  OCC4D_REQUIRE(n >= 0, "%s: n = %d", who, n);
  *empty = n == 0;
  if (*empty) return OCC4D_OK;
  OCC4D_REQUIRE(xyz && queries && idx_local && w_local && (w->n_cross == 0 || idx_cross), "%s: null pointer (xyz, queries, "
                "idx_local, w_local%s)", who, w->n_cross ? ", idx_cross" : "");
  OCC4D_REQUIRE(q_stride >= w->d_in, "%s: q_stride = %lld < d_in = %d", who, (long long)q_stride, w->d_in);
  OCC4D_REQUIRE(m >= w->k_local && (w->n_cross == 0 || m >= w->k_cross), "%s: m = %d abstract points cannot serve the %d / %d "
                "neighbours the decoder asks for", who, m, w->k_local, w->k_cross);
  OCC4D_REQUIRE(!x0 || (al16(x0) && ld_x0 % 4 == 0 && ld_x0 >= w->d_hidden && workspace && al16(workspace)),
                "%s: x0 rows must be 16-byte aligned with ld_x0 %% 4 == 0, ld_x0 >= d_hidden = %d, and need the workspace", who,
                w->d_hidden);
  return OCC4D_OK;
}

inline int check_query_fwd_prelude(const occ4d_decoder_weights* w, const float* prepared, const float* scene, int m,
                                   const float* queries, int64_t q_stride, int n, const int32_t* idx_local, const float* w_local,
                                   const int32_t* idx_cross, const float* x0, int64_t ld_x0, const float* out, int64_t ld_out,
                                   const float* penult, int64_t ld_pen, const float* workspace, bool* empty) {
  const char* who = "occ4d_decoder_query_fwd_prelude_f32";
  OCC4D_REQUIRE(n >= 0, "%s: n = %d", who, n);
  *empty = n == 0;
  if (*empty) return OCC4D_OK;
  OCC4D_REQUIRE(prepared && scene && queries && out && workspace && al16(workspace) && q_stride >= w->d_in && ld_out >= w->d_out,
                "%s: null or misaligned buffer", who);
  OCC4D_REQUIRE(idx_local && w_local && (w->n_cross == 0 || idx_cross), "%s: the prelude's idx_local, w_local%s rows are "
                "required", who, w->n_cross ? ", idx_cross" : "");
  OCC4D_REQUIRE(!x0 || (al16(x0) && ld_x0 % 4 == 0 && ld_x0 >= w->d_hidden), "%s: x0 rows must be 16-byte aligned with "
                "ld_x0 %% 4 == 0 and ld_x0 >= d_hidden = %d", who, w->d_hidden);
  OCC4D_REQUIRE(!penult || (al16(penult) && ld_pen % 4 == 0 && ld_pen >= w->d_hidden), "%s: penult rows must be 16-byte aligned "
                "with ld_pen %% 4 == 0", who);
  OCC4D_REQUIRE(m >= w->k_local && (w->n_cross == 0 || m >= w->k_cross), "%s: m = %d abstract points", who, m);
  return OCC4D_OK;
}

}  // namespace occ4d_decoder
