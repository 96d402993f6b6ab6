// Shared device vocabulary of the MFMA kernels (csrc/trunk.hip, trunk4.hip, crossattn16p.hip, wgrad16.hip and, through
// csrc/bf16x6.hpp, the split-precision kernels): vector types, the global -> LDS fragment DMA, ReLU on a register tile,
// the gfx950 lane swaps and the fp32 16 x 16 x 4 MFMA group.  Stage loops, fragment counts and everything tuned stay
// with each kernel.
#pragma once
#include "common.hpp"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS byte address of a __shared__ object (wave-uniform, for M0)
template <typename T>
__device__ __forceinline__ unsigned lds_addr(const T* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) T*)p;
}

// One fragment (1 KB = 64 lanes x 16 B), global (L2) -> LDS by DMA: one global_load_lds_dwordx4 with the LDS destination
// in M0 (wave-uniform), a scalar source base (the wave-uniform fragment address) and this lane's byte offset `lane16`
// (lane * 16 for a lane-linear fragment image).  No VALU address arithmetic: on gfx950 the fp32 MFMAs and the plain VALU
// share the SIMD's vector issue (profiles/micro/valu_beside_mfma.hip: every VALU instruction beside a saturated
// v_mfma_f32_16x16x4_f32 stream costs its ~4 cycles in full), so address arithmetic in a stage loop is paid for in
// matrix throughput.
// Issued through inline asm ON PURPOSE: with the __builtin the compiler, knowing that an asynchronous LDS write is
// in flight, degrades every s_waitcnt of the fragment ds_reads to lgkmcnt(0) -- each group of MFMAs then waits
// for the reads issued just before it (a full LDS round trip per 8 MFMAs; measured: a wave running alone kept the
// matrix pipe 65 % busy).  The asm is invisible to that bookkeeping; each kernel's stage protocol supplies the ordering:
// dma_wait() (s_waitcnt vmcnt(0)) + barrier before anybody reads the buffer, barrier before it is overwritten.
template <typename T>
__device__ __forceinline__ void dma_frag(const T* __restrict__ src_frag, unsigned lds_dst, unsigned lane16) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane16), "s"(lds_dst), "s"(src_frag) : "memory");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
  v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
  return v;
}

// gfx950 lane-swap exchanges (16-lane rows r0..r3 of a wave):
//   swap16(x, y) -> lo = (x.r0, y.r0, x.r2, y.r2), hi = (x.r1, y.r1, x.r3, y.r3)
//   swap32(x, y) -> lo = (x.r0, x.r1, y.r0, y.r1), hi = (x.r2, x.r3, y.r2, y.r3)
struct Pair { float lo, hi; };
__device__ __forceinline__ Pair swap16(float x, float y) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  return Pair{__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ Pair swap32(float x, float y) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  return Pair{__uint_as_float(r[0]), __uint_as_float(r[1])};
}

// 8 x v_mfma_f32_16x16x4_f32, K = 16: c0 += a0 b0, c1 += a1 b1, the two accumulators advanced alternately so that
// consecutive MFMAs never depend on each other (40-cycle latency vs 32-cycle issue).  With the weight fragments as the
// A operand the result tile is TRANSPOSED: lane (g, c) holds channels 4 g .. 4 g + 3 of row c (one float4 per row).
__device__ __forceinline__ void mfma16x2(const f32x4 a0, const f32x4 a1, const f32x4 b0, const f32x4 b1, f32x4& c0, f32x4& c1) {
  c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, c0, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, c1, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, c0, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, c1, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, c0, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, c1, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, c0, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, c1, 0, 0, 0);
}
// ... with one A / one B operand for both tiles
__device__ __forceinline__ void mfma16x2_a(const f32x4 a, const f32x4 b0, const f32x4 b1, f32x4& c0, f32x4& c1) {
  mfma16x2(a, a, b0, b1, c0, c1);
}
__device__ __forceinline__ void mfma16x2_b(const f32x4 a0, const f32x4 a1, const f32x4 b, f32x4& c0, f32x4& c1) {
  mfma16x2(a0, a1, b, b, c0, c1);
}

}  // namespace
