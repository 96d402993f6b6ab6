// Shared helpers for libocc4d.so (gfx950 only; no CUDA dual path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "contract.hpp"      // occ4d::set_error, OCC4D_REQUIRE, OCC4D_TRY

namespace occ4d {

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return OCC4D_ELAUNCH;
  }
  return OCC4D_OK;
}

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Argument contract of the row-resident trunk launchers (csrc/trunk.hip: TrunkArgs; csrc/trunk4.hip: Trunk4Args): `who` is
// the entry point the error text names, `width` the row width the kernels are built for.
template <class Args>
int check_trunk_args(const Args& a, const char* who, int width) {
  OCC4D_REQUIRE(a.x && a.y && a.w0p && a.b0, "%s: null pointer", who);
  OCC4D_REQUIRE(a.n >= 0, "%s: n = %d", who, a.n);
  OCC4D_REQUIRE(a.ldx >= width && a.ldx % 4 == 0 && a.ldy % 4 == 0 && ((uintptr_t)a.x % 16) == 0 &&
                    ((uintptr_t)a.y % 16) == 0 && ((uintptr_t)a.w0p % 16) == 0 && ((uintptr_t)a.b0 % 16) == 0,
                "%s: x / y / weights / bias must be 16-byte aligned with row strides %% 4 == 0 (ldx >= %d)", who, width);
  if (a.ztab) {
    OCC4D_REQUIRE(a.zconst && a.zidx && a.zw && a.kz >= 1 && a.ldz % 4 == 0 && ((uintptr_t)a.ztab % 16) == 0 &&
                      ((uintptr_t)a.zconst % 16) == 0,
                  "%s: interpolation term needs zconst / zidx / zw, kz >= 1 and a 16-byte aligned table", who);
  }
  return OCC4D_OK;
}

// n rows of dp floats with row stride ldp from p / of dq floats with row stride ldq from q: do the two spans, each from its
// first to its last byte, share a byte?  (Conservative: two column slices of one wider buffer count as overlapping.)
inline bool spans_overlap(const float* p, int64_t ldp, int dp, const float* q, int64_t ldq, int dq, int n) {
  if (!p || !q || n <= 0) return false;
  const uintptr_t p0 = (uintptr_t)p, p1 = (uintptr_t)(p + (int64_t)(n - 1) * ldp + dp);
  const uintptr_t q0 = (uintptr_t)q, q1 = (uintptr_t)(q + (int64_t)(n - 1) * ldq + dq);
  return p0 < q1 && q0 < p1;
}

// ... the same for two row sets of one width d
inline bool rows_overlap(const float* p, int64_t ldp, const float* q, int64_t ldq, int n, int d) {
  return spans_overlap(p, ldp, d, q, ldq, d, n);
}

// ... and what the rowlin entry points add to it: n_out a multiple of the kernel's `stage` outputs, the residual rows
// (`skip`: the rows added after the mask, which that entry point requires) and, when `masked`, the mask rows.  y must not
// overlap x: a row tile split over several workgroups (csrc/trunk4.hip) has each of them read whole rows of x while the
// others store their share of y, so no rowlin runs in place (the residual rows may be y: every element is read by the
// thread that then writes it).
template <class Args>
int check_rowlin_args(const Args& a, const char* who, int width, int stage, int n_out, bool masked, bool skip = false) {
  if (int rc = check_trunk_args(a, who, width)) return rc;
  OCC4D_REQUIRE(n_out >= stage && n_out % stage == 0 && a.ldy >= n_out, "%s: n_out = %d must be a multiple of %d <= ldy", who,
                n_out, stage);
  OCC4D_REQUIRE(!spans_overlap(a.y, a.ldy, n_out, a.x, a.ldx, width, a.n), "%s: y must not overlap x", who);
  const bool res_ok = a.ldr % 4 == 0 && ((uintptr_t)a.res % 16) == 0 && a.ldr >= n_out;
  if (skip) {
    OCC4D_REQUIRE(a.res && res_ok, "%s: skip rows must be 16-byte aligned with lds %% 4 == 0 and lds >= n_out", who);
  } else {
    OCC4D_REQUIRE(!a.res || res_ok, "%s: residual rows must be 16-byte aligned with ldr %% 4 == 0", who);
  }
  OCC4D_REQUIRE(!masked || (a.mask && a.ldm % 4 == 0 && ((uintptr_t)a.mask % 16) == 0 && a.ldm >= n_out),
                "%s: mask rows must be 16-byte aligned with ldm %% 4 == 0 and ldm >= n_out", who);
  return OCC4D_OK;
}

// ... what occ4d_rowlin_linz_f32 (include/ext/occ4d_linz.h) adds to the rowlin contract: at least one of the two terms, exactly
// `zk` neighbours (the kernel holds a row's list in registers), and for the second term its table, its constant and the
// dense rows it is stored to, which no stage may read back (x, the residual) or write as well (y).
template <class Args>
int check_linz_args(const Args& a, const char* who, int zk, int n_out) {
  OCC4D_REQUIRE(a.ztab || a.ztab2, "%s: no interpolation term (ztab and ztab2 are both null; occ4d_rowlin_f32 is the plain launch)", who);
  OCC4D_REQUIRE(a.zidx && a.zw && a.kz == zk, "%s: the terms take zidx / zw with kz = %d neighbours (kz = %d: run "
                "occ4d_interp_add_f32 behind occ4d_rowlin_f32)", who, zk, a.kz);
  OCC4D_REQUIRE(a.ldz >= n_out && a.ldz % 4 == 0, "%s: ldz = %lld must be a multiple of 4 >= n_out", who, (long long)a.ldz);
  OCC4D_REQUIRE(a.zrows >= 1 && (int64_t)a.zrows * a.ldz < ((int64_t)1 << 30), "%s: zrows = %d table rows of stride %lld: zrows "
                "ldz must stay below 2^30 (32-bit row offsets)", who, a.zrows, (long long)a.ldz);
  if (a.ztab2) {
    OCC4D_REQUIRE(a.zconst2 && ((uintptr_t)a.ztab2 % 16) == 0 && ((uintptr_t)a.zconst2 % 16) == 0,
                  "%s: the second term needs zconst2 and a 16-byte aligned table", who);
    OCC4D_REQUIRE(a.dense && ((uintptr_t)a.dense % 16) == 0 && a.ldd % 4 == 0 && a.ldd >= n_out,
                  "%s: dense rows must be 16-byte aligned with ldd %% 4 == 0 and ldd >= n_out", who);
    OCC4D_REQUIRE(!rows_overlap(a.dense, a.ldd, a.y, a.ldy, a.n, n_out) && !rows_overlap(a.dense, a.ldd, a.x, a.ldx, a.n, n_out) &&
                      !rows_overlap(a.dense, a.ldd, a.res, a.ldr, a.n, n_out),
                  "%s: dense rows must not alias x, y or the residual rows", who);
  } else {
    OCC4D_REQUIRE(!a.dense && !a.zconst2, "%s: dense / zconst2 given without ztab2", who);
  }
  return OCC4D_OK;
}

// ... and occ4d_resblock_addrows_f32: the dense rows are read while other workgroups already store their y rows
template <class Args>
int check_addrows_args(const Args& a, const char* who, int width) {
  OCC4D_REQUIRE(a.addrows && ((uintptr_t)a.addrows % 16) == 0 && a.lda % 4 == 0 && a.lda >= width,
                "%s: addrows must be 16-byte aligned with ld_add %% 4 == 0 and ld_add >= %d", who, width);
  OCC4D_REQUIRE((int64_t)a.n * a.lda < ((int64_t)1 << 30), "%s: n ld_add = %lld must stay below 2^30 (32-bit row offsets: chunk "
                "the rows)", who, (long long)((int64_t)a.n * a.lda));
  OCC4D_REQUIRE(!rows_overlap(a.addrows, a.lda, a.y, a.ldy, a.n, width), "%s: addrows must not alias y", who);
  return OCC4D_OK;
}

// fps_bucket.hip: the pruned single-workgroup FPS (FPS_BUCKET_MIN_POINTS <= n <= 16384); -1 = n outside that range.
// Since a round of the pruned kernel accepts several samples (round 3) it also wins on the small encoder levels, whose
// step is bound by the serial argmax chain (profiles/time_fps.py, pruned vs exhaustive: 9558 points 1.84 vs 3.54 ms,
// 4779 points 0.91 vs 1.15 ms, 1593 points 0.27 vs 0.31 ms; 2049 uniform points in a half-empty second bucket row
// 0.42 vs 0.40 ms).  OCC4D_FPS_BUCKET_MIN overrides the threshold (ablation).
constexpr int FPS_BUCKET_MIN_POINTS = 1536;
int fps_bucket_launch(const float* xyz, int64_t stride, int n, int m, int start, int32_t* out_sorted,
                      int32_t* out_order, hipStream_t stream);


// wgrad16.hip: weight gradient for N a multiple of 416, K a multiple of 32 (>= 64), M >= 4096 (the wide decoder
// layers); false = the shape is not taken (backward.hip's wgrad_kernel then runs).
bool wgrad16_plan(int M, int N, int K, int* splits, int* m_per_split);
int wgrad16_launch(const float* g, int64_t ldg, const float* x, int64_t ldx, int M, int N, int K, int splits,
                   int m_per_split, float* part, float* part_b, int relu_x, hipStream_t stream);

// memops.hip: dst[i][0 .. d) = 0 / = src[i][0 .. d) for n rows with row strides (kernels, never hipMemset / hipMemcpy: those
// are not reliably replayed from a captured graph on this stack)
int zero_rows(float* dst, int64_t ld, int64_t n, int d, hipStream_t st);
int copy_rows(float* dst, int64_t ldd, const float* src, int64_t lds, int64_t n, int d, hipStream_t st);

// memops.hip: compute units of the current device (cached; 256 if the query fails)
int cu_count();

// path.hip: OCC4D_F16W=1 (default 0): the fp16 scheme's attention layers on csrc/crossattn_f16w.hip (A/B)
bool f16w_enabled();
// path.hip: OCC4D_F16_RESBLOCK=0 (default 1): the fp16 scheme's residual blocks as two row-kernel launches instead of the fused
// block of csrc/resblock_f16x3.hip (A/B)
bool f16_resblock_enabled();

// trunk_bf16x6.hip: the fp16 split row kernel for a weight the caller multiplied by the power of two `prescale`: packed as
// the unscaled weight (window |w / prescale| < 255.9), the factor restored in the epilogue (y = w x + b, w and b prescaled)
int pack_rowlin_f16x3_prescaled(const float* w, int64_t ldw, int n_out, float prescale, float* packed, hipStream_t st);
int rowlin_f16x3_prescaled(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed, const float* b,
                           int n_out, float prescale, int relu_in, const float* res, int64_t ldr, int n, hipStream_t st);

// path.hip: phase offset of the paired attention workgroups (units of s_sleep(127); OCC4D_CA16P_SKEW, default 6)
int attn16p_skew();

}  // namespace occ4d
