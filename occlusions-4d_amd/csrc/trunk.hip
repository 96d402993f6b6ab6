// Row-resident fused layers of the decoder trunk (D6 / K11 of SURVEY.md: ResnetBlockFC.forward,
// model/implicit.py:92-101, and the 416-wide Linear layers around the cross-attention blocks,
// model/modules.py:61-65): the activations of a row tile never leave the registers between the
// layers of a block; only the weights stream (L2 -> LDS, DMA) past them.
//
// Layout (wave64, v_mfma_f32_16x16x4_f32, exact fp32): a wave owns 16 rows; lane (g = lane >> 4,
// r = lane & 15) holds, for row r, the channels 16 t + 4 g + e (e = 0..3) of every 16-channel group
// t as one float4 -- 26 float4 = 104 registers for a 416-wide activation.  Every GEMM is run in
// TRANSPOSED form  out^T[n][row] = sum_k W[n][k] act^T[k][row]:
//   A operand = weight fragment W[n0 + r][16 t + 4 g + e]   (ds_read_b128 from LDS, element e per step)
//   B operand = act register (t, e)                          (lane (g, r) = row r, k = 16 t + 4 g + e)
//   C/D       = out^T[n0 + 4 g + reg][row r]                 -> again "row r, 4 consecutive channels":
// the output registers of one layer ARE the B operand of the next layer and, at the end, one float4
// global store per lane.  Two waves per SIMD (8 waves x 16 rows = 128 rows per workgroup) -- the
// 32x32x2 form would need 208 registers per activation and leave room for one wave per SIMD only.
//
// Residual block  y = x + W1 relu(W0 relu(x) + b0) + b1  as ONE rolled loop over 13 hidden chunks
// of 32 (the structure of the attention kernel): chunk j:  h_j = relu(W0[32 j.., :] relu(x) + b0)
// (2 accumulator tiles, 208 MFMAs), then  yacc += W1[:, 32 j..] h_j  (26 accumulator tiles, 208
// MFMAs); yacc is initialised with x + b1, so the residual costs nothing.  Weights are pre-packed on
// the host (ops.pack_trunk_weights) into the exact LDS image of each stage: 52 fragments of 1 KB
// (64 lanes x 16 B, lane-linear: conflict-free ds_read_b128, contiguous global_load_lds_dwordx4), two
// stage buffers of 52 KB: while a stage's MFMAs read one buffer the DMA fills the other; one
// s_waitcnt vmcnt(0) + barrier per stage ("my part of the next stage has landed" + "everybody's has").
#include <type_traits>

#include "ext/occ4d_chain.h"
#include "ext/occ4d_linz.h"
#include "tile.hpp"

namespace {

constexpr int TH = 416;                      // trunk width the kernels are built for
constexpr int TKG = TH / 16;                 // 26 channel groups of 16
constexpr int TNS = TH / 32;                 // 13 stages of 32 channels
constexpr int FRAG_FLOATS = 256;             // one (n-tile, k-group) fragment image: 64 lanes x float4
constexpr int STAGE_FRAGS = 2 * TKG;         // 52: (2 n-tiles x 26 k-groups) or (26 n-tiles x 2 k-groups)
constexpr int STAGE_FLOATS = STAGE_FRAGS * FRAG_FLOATS;   // 13312 floats = 53248 B
constexpr int TROWS = 128;                   // rows per workgroup

struct TrunkArgs {
  const float* x; int64_t ldx;               // input rows (n, 416)
  float* y; int64_t ldy;                     // output rows (n, N); may alias x (each workgroup reads its rows first)
  const float* w0p; const float* b0;         // stage-packed weights / bias of the first layer
  const float* w1p; const float* b1;         // ... of the second layer (residual block only)
  const float* res; int64_t ldr;             // rowlin: residual rows added to the output, or null
  // optional inverse-distance interpolation term added to the OUTPUT rows (the next block's lin_z):
  // y[i, :] += zconst[:] + sum_j zw[i, j] * ztab[zidx[i, j], :]
  const float* zconst; const float* ztab; int64_t ldz; const int32_t* zidx; const float* zw; int kz;
  int n;                                     // rows
  int n_stages;                              // rowlin: output channels / 32
  int relu_in;                               // rowlin: relu on the operand
  const float* mask; int64_t ldm;            // rowlin: output rows zeroed where mask <= 0 (ReLU mask of a data gradient), or null
  // rowlin, second interpolation term (same zidx / zw / ldz / kz), STORED as dense rows instead of added:
  // dense[i, :] = zconst2[:] + sum_j zw[i, j] * ztab2[zidx[i, j], :]
  const float* zconst2; const float* ztab2; float* dense; int64_t ldd; int zrows;
  const float* addrows; int64_t lda;         // resblock: dense rows added to the output rows last (y = block(x) + addrows), or null
};

// One stage = 52 fragments of 1 KB, global (L2) -> LDS by DMA (dma_frag, csrc/tile.hpp); wave w moves fragments w,
// w + 8, ...  Ordering: dma_wait() + barrier before anybody reads the buffer, barrier before it is overwritten.
__device__ __forceinline__ void dma_stage(const float* __restrict__ src, const float* dst, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int c = wave + 8 * i;                       // wave-uniform
    if (c < STAGE_FRAGS) dma_frag(src + c * FRAG_FLOATS, lds_addr(dst) + (unsigned)c * (FRAG_FLOATS * 4), (unsigned)lane * 16u);
  }
}

// the i-th of this wave's (up to 7) fragments of a stage: fragment wave + 8 i (i = 6 exists for waves 0-3 only)
__device__ __forceinline__ void dma_part(const float* __restrict__ src, const float* dst, int wave, int lane, int i) {
  const int c = wave + 8 * i;                         // wave-uniform
  if (c < STAGE_FRAGS) dma_frag(src + c * FRAG_FLOATS, lds_addr(dst) + (unsigned)c * (FRAG_FLOATS * 4), (unsigned)lane * 16u);
}

// ---------------------------------------------------------------------------------------------------
// y = x + W1 relu(W0 relu(x) + b0) + b1  [+ addrows]
// ADD: dense rows (the NEXT block's lin_z term, produced by an earlier rowlin launch) are added to the output rows as the
// last operation.  Their loads sit under the MFMAs of the LAST hidden chunk, in the registers of relu(x), which die tile
// by tile during that chunk's stage A: tiles 0 .. 10 after every second group of stage A (tile k after group 2 k + 1),
// tiles 11 .. 25 with the first 15 groups of stage B -- every load has at least four groups of MFMAs before the
// vmcnt(0) of the barrier that follows it.  The last chunk is peeled; chunks 0 .. 11 are the code of the plain kernel.
template <bool ADD>
__global__ __launch_bounds__(512, 2) void resblock_kernel(const TrunkArgs a) {
  // two separate LDS objects: the DMA into one is provably disjoint from the fragment reads of the other (one
  // array split by an offset made the compiler wait for vmcnt(0) -- the DMA just issued -- before the first ds_read)
  __shared__ __attribute__((aligned(16))) float bufA[STAGE_FLOATS];   // W0 chunk of the current hidden chunk
  __shared__ __attribute__((aligned(16))) float bufB[STAGE_FLOATS];   // W1 chunk
  __shared__ __attribute__((aligned(16))) float s_b0[TH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * TROWS + wave * 16 + r;
  const int rowc = min(row, a.n - 1);

  dma_stage(a.w0p, bufA, wave, lane);
  if (tid < TH) s_b0[tid] = a.b0[tid];
  f32x4 xr[TKG], yacc[TKG];
  {
    const float* xp = a.x + (int64_t)rowc * a.ldx + 4 * g;
#pragma unroll
    for (int t = 0; t < TKG; ++t) {
#ifdef OCC4D_TR_NOPRO
      const f32x4 v = {(float)t, (float)g, (float)r, 1.f};
#else
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + 16 * t);
#endif
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.b1 + 16 * t + 4 * g);
      xr[t] = relu4(v);
      yacc[t].x = v.x + b.x; yacc[t].y = v.y + b.y; yacc[t].z = v.z + b.z; yacc[t].w = v.w + b.w;
    }
  }
  dma_wait();
  __syncthreads();
  const float* const fa = bufA + lane * 4;   // this lane's float4 inside a fragment image
  const float* const fb = bufB + lane * 4;

#ifdef OCC4D_TR_STAMP
  // per-wave cycle accounting (debug build): [0] stage A issue -> last MFMA, [1] wait at barrier 1, [2] stage B, [3] wait 2
  unsigned long long tacc[4] = {0, 0, 0, 0};
  unsigned long long tprev = __builtin_amdgcn_s_memtime();
  const unsigned long long tstart = tprev;
#define STAMP(i) { const unsigned long long tn = __builtin_amdgcn_s_memtime(); tacc[i] += tn - tprev; tprev = tn; }
#else
#define STAMP(i)
#endif
  asm volatile("; OCC4D_MARK loop");
  // the packed W0 stream carries TNS + 1 stages (the last repeats stage 0), so "prefetch stage j + 1" is branch-free
  auto chunk = [&](const int j, auto last_chunk) __attribute__((always_inline)) {
    constexpr bool LAST = ADD && decltype(last_chunk)::value;
    // this lane's float4 of tile 0: scalar base + one 32-bit offset register (n ld_add < 2^30, checked by the launcher)
    // (formed HERE from the row number, which the epilogue keeps anyway: the empty asm keeps the offset out of the prologue
    // and the loop, where every register is taken)
    int arow = row;
    if (LAST) asm volatile("" : "+v"(arow));
    const float* const ap = LAST ? a.addrows + (unsigned)(min(arow, a.n - 1) * (int)a.lda + 4 * g) : nullptr;
    // ---- stage A: h = relu(W0[32 j .. 32 j + 32, :] relu(x) + b0); meanwhile W1's chunk j lands in bufB
    f32x4 h0 = *reinterpret_cast<const f32x4*>(s_b0 + 32 * j + 4 * g);
    f32x4 h1 = *reinterpret_cast<const f32x4*>(s_b0 + 32 * j + 16 + 4 * g);
    {
      // fragment pipeline: the ds_reads of group t + 1 are issued BEFORE the 8 MFMAs of group t and nothing may be
      // scheduled across the fences (left alone, the compiler sinks the reads to just before their use and every 16
      // MFMAs wait for a full LDS round trip: measured 65 % of the matrix pipe for a wave that runs alone)
      f32x4 wa = *reinterpret_cast<const f32x4*>(fa);
      f32x4 wb = *reinterpret_cast<const f32x4*>(fa + TKG * FRAG_FLOATS);
#pragma unroll
      for (int t = 0; t < TKG; ++t) {
#ifndef OCC4D_TR_NODMA
        // the other buffer's DMA, one fragment every third group, between MFMAs: issued back to back right after the
        // barrier, the eight waves' 52 KB queued up in the CU's single vector-memory path and every wave's
        // instruction stream -- MFMAs included -- sat behind its own stalled VMEM issue
        if (t >= 2 && t <= 20 && (t - 2) % 3 == 0) dma_part(a.w1p + (int64_t)j * STAGE_FLOATS, bufB, wave, lane, (t - 2) / 3);
#endif
        const f32x4 ca = wa, cb = wb;
        if (t + 1 < TKG) {
          wa = *reinterpret_cast<const f32x4*>(fa + (t + 1) * FRAG_FLOATS);
          wb = *reinterpret_cast<const f32x4*>(fa + (TKG + t + 1) * FRAG_FLOATS);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma16x2_b(ca, cb, xr[t], h0, h1);
        __builtin_amdgcn_sched_barrier(0);
        // (tile (t - 1) / 2 <= t of relu(x) has had its last use)
        if (LAST && (t & 1) && t <= 21) xr[(t - 1) / 2] = *reinterpret_cast<const f32x4*>(ap + 16 * ((t - 1) / 2));
      }
    }
    h0 = relu4(h0);
    h1 = relu4(h1);
    STAMP(0)
#ifndef OCC4D_TR_NOBAR
    dma_wait();
    __syncthreads();
#endif
    STAMP(1)
    // ---- stage B: yacc += W1[:, 32 j .. 32 j + 32] h; meanwhile W0's chunk j + 1 lands in bufA
    {
      // group (p, tt): output tiles 2 p and 2 p + 1, hidden half tt; same fenced pipeline
      f32x4 wa = *reinterpret_cast<const f32x4*>(fb);
      f32x4 wb = *reinterpret_cast<const f32x4*>(fb + 2 * FRAG_FLOATS);
#pragma unroll
      for (int q = 0; q < TKG; ++q) {
        const int p = q >> 1, tt = q & 1;
#ifndef OCC4D_TR_NODMA
        if (q >= 2 && q <= 20 && (q - 2) % 3 == 0) dma_part(a.w0p + (int64_t)(j + 1) * STAGE_FLOATS, bufA, wave, lane, (q - 2) / 3);
#endif
        if (LAST && q < TKG - 11) xr[11 + q] = *reinterpret_cast<const f32x4*>(ap + 16 * (11 + q));
        const f32x4 ca = wa, cb = wb;
        if (q + 1 < TKG) {
          const int pn = (q + 1) >> 1, tn = (q + 1) & 1;
          wa = *reinterpret_cast<const f32x4*>(fb + (4 * pn + tn) * FRAG_FLOATS);
          wb = *reinterpret_cast<const f32x4*>(fb + (4 * pn + 2 + tn) * FRAG_FLOATS);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma16x2_b(ca, cb, tt ? h1 : h0, yacc[2 * p], yacc[2 * p + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    STAMP(2)
#ifndef OCC4D_TR_NOBAR
    dma_wait();
    __syncthreads();
#endif
    STAMP(3)
  };
#pragma clang loop unroll(disable)
  for (int j = 0; j < (ADD ? TNS - 1 : TNS); ++j) chunk(j, std::false_type{});
  if (ADD) chunk(TNS - 1, std::true_type{});
  asm volatile("; OCC4D_MARK epilogue");
#ifdef OCC4D_TR_STAMP
  if (lane == 0 && a.zw) {     // debug build: a.zw doubles as the stamp buffer (5 x u64 per wave)
    unsigned long long* o = (unsigned long long*)a.zw + (size_t)(blockIdx.x * 8 + wave) * 6;
    o[0] = tacc[0]; o[1] = tacc[1]; o[2] = tacc[2]; o[3] = tacc[3]; o[4] = tprev - tstart; o[5] = tstart;
  }
#endif
  if (ADD) {       // xr holds this row's addrows by now
#pragma unroll
    for (int t = 0; t < TKG; ++t) { yacc[t].x += xr[t].x; yacc[t].y += xr[t].y; yacc[t].z += xr[t].z; yacc[t].w += xr[t].w; }
  }
#ifdef OCC4D_TR_NOEPI
  {
    float tsum = 0.f;
#pragma unroll
    for (int t = 0; t < TKG; ++t) tsum += yacc[t].x + yacc[t].y + yacc[t].z + yacc[t].w;
    if (tsum == 123.456f) a.y[0] = tsum;     // keep the accumulators live
    return;
  }
#endif
  if (row < a.n) {
    float* yp = a.y + (int64_t)row * a.ldy + 4 * g;
#pragma unroll
    for (int t = 0; t < TKG; ++t) *reinterpret_cast<f32x4*>(yp + 16 * t) = yacc[t];
  }
}

// ---------------------------------------------------------------------------------------------------
// y[:, 0 .. 32 S) = [res +] W [relu](x) + b  [+ interpolation term], K = 416, one stage per 32 output channels
//
// The interpolation terms (Z1: added to the output rows; Z2: a second table, stored as dense rows) take ZK = 8 neighbours.
// The kernel holds a row's weights and the BYTE OFFSETS of its table rows (zo[j] = 4 (zidx[j] ldz + 4 g): 32 bits, the
// launcher checks zrows ldz < 2^30) in registers, the same for every stage; a stage's table base is scalar, so a gather
// costs no vector arithmetic.  The gathers are software-pipelined under the stage's MFMAs, one neighbour per slot:
// neighbour j is ISSUED in group 3 j + 2, right after that group's DMA fragment, and CONSUMED three groups later, right
// before the next DMA fragment (neighbour 7 and zconst: issued in group 23, consumed after the loop).  The hardware's
// vmcnt is in order, and the DMA (inline asm) is invisible to the compiler's count: a wait for a gather therefore also
// waits for everything issued before it -- the DMA fragment of its own group, as old as itself -- and for nothing issued
// later.  The sums run in the order of interp_add4_kernel (csrc/pointops.hip), separate multiplies and adds:
//   s = (..((0 + w0 t0) + w1 t1) + ..) + zconst,   y = (acc + (b + res)) + s
// -- bit for bit the stand-alone pass behind the plain launch.
constexpr int ZK = 8;

__device__ __forceinline__ void zacc(f32x4& s, const float w, const f32x4 t) {
  s.x += w * t.x; s.y += w * t.y; s.z += w * t.z; s.w += w * t.w;
}
__device__ __forceinline__ void add4(f32x4& s, const f32x4 t) { s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
__device__ __forceinline__ f32x4 ld4(const float* base, unsigned byte_off) {    // scalar base + 32-bit lane offset
  return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + byte_off);
}

template <bool Z1, bool Z2>
__device__ __forceinline__ void rowlin_stage(const TrunkArgs& a, int s, const float* __restrict__ frag, const f32x4* xr,
                                             int row, int rowc, int g, const float* next_src, const float* next_dst,
                                             int wave, int lane, const unsigned* zo, const float* zwt) {
  constexpr bool Z = Z1 || Z2;
  const int c0 = 32 * s + 4 * g;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 s1a = zero4, s1b = zero4, s2a = zero4, s2b = zero4;       // the terms' sums for this stage's 2 x 4 channels
  f32x4 g1a, g1b, g2a, g2b;                                       // the neighbour in flight
  f32x4 k1a, k1b, k2a, k2b;                                       // zconst
  const float* const t1 = Z1 ? a.ztab + 32 * s : nullptr;         // (wave-uniform)
  const float* const t2 = Z2 ? a.ztab2 + 32 * s : nullptr;
  auto issue = [&](const int j) __attribute__((always_inline)) {
    if (Z1) { g1a = ld4(t1, zo[j]); g1b = ld4(t1 + 16, zo[j]); }
    if (Z2) { g2a = ld4(t2, zo[j]); g2b = ld4(t2 + 16, zo[j]); }
  };
  auto consume = [&](const int j) __attribute__((always_inline)) {
    // (the empty asm pins the arithmetic to this slot: left alone, instruction selection sinks every slot's adds to
    // the end of the stage and keeps all eight neighbours' gathers in registers until then)
    if (Z1) { zacc(s1a, zwt[j], g1a); zacc(s1b, zwt[j], g1b); asm volatile("" : "+v"(s1a), "+v"(s1b)); }
    if (Z2) { zacc(s2a, zwt[j], g2a); zacc(s2b, zwt[j], g2b); asm volatile("" : "+v"(s2a), "+v"(s2b)); }
  };
  // bias / residual: compiler-tracked global loads issued AFTER this stage's DMA and consumed at the END of the stage
  // (the hardware's vmcnt is in order: consuming them earlier would wait for the DMA as well; with terms, b + res is
  // formed at the first consume slot, which waits for them anyway, and four registers are held instead of eight)
  f32x4 bz0 = *reinterpret_cast<const f32x4*>(a.b0 + c0);
  f32x4 bz1 = *reinterpret_cast<const f32x4*>(a.b0 + c0 + 16);
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = {0.f, 0.f, 0.f, 0.f};
  if (a.res) {
    r0 = *reinterpret_cast<const f32x4*>(a.res + (int64_t)rowc * a.ldr + c0);
    r1 = *reinterpret_cast<const f32x4*>(a.res + (int64_t)rowc * a.ldr + c0 + 16);
  }
  {
    f32x4 wa = *reinterpret_cast<const f32x4*>(frag);
    f32x4 wb = *reinterpret_cast<const f32x4*>(frag + TKG * FRAG_FLOATS);
#pragma unroll
    for (int t = 0; t < TKG; ++t) {
      if (Z && t == 5) { add4(bz0, r0); add4(bz1, r1); asm volatile("" : "+v"(bz0), "+v"(bz1)); }
      if (Z && t >= 5 && t <= 3 * ZK - 1 && (t - 2) % 3 == 0) consume((t - 5) / 3);
      if (Z && t >= 2 && t <= 17 && (t - 2) % 3 == 0) {       // fragments wave + 8 i, i < 6, exist for every wave: no branch
        const int c = wave + 8 * ((t - 2) / 3);
        dma_frag(next_src + c * FRAG_FLOATS, lds_addr(next_dst) + (unsigned)c * (FRAG_FLOATS * 4), (unsigned)lane * 16u);
      } else if (t >= 2 && t <= 20 && (t - 2) % 3 == 0) {
        dma_part(next_src, next_dst, wave, lane, (t - 2) / 3);   // (see resblock_kernel)
      }
      if (Z && t >= 2 && t <= 3 * ZK - 1 && (t - 2) % 3 == 0) issue((t - 2) / 3);
      if (Z && t == 3 * ZK - 1) {
        if (Z1) { k1a = *reinterpret_cast<const f32x4*>(a.zconst + c0); k1b = *reinterpret_cast<const f32x4*>(a.zconst + c0 + 16); }
        if (Z2) { k2a = *reinterpret_cast<const f32x4*>(a.zconst2 + c0); k2b = *reinterpret_cast<const f32x4*>(a.zconst2 + c0 + 16); }
      }
      const f32x4 ca = wa, cb = wb;
      if (t + 1 < TKG) {
        wa = *reinterpret_cast<const f32x4*>(frag + (t + 1) * FRAG_FLOATS);
        wb = *reinterpret_cast<const f32x4*>(frag + (TKG + t + 1) * FRAG_FLOATS);
      }
      __builtin_amdgcn_sched_barrier(0);
      mfma16x2_b(ca, cb, xr[t], o0, o1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (Z) {
    static_assert(3 * ZK - 1 < TKG && STAGE_FRAGS > 7 + 8 * 5, "slots inside the group loop; six fragments per wave");
    add4(o0, bz0); add4(o1, bz1);
    consume(ZK - 1);
    if (Z1) { add4(s1a, k1a); add4(s1b, k1b); add4(o0, s1a); add4(o1, s1b); }
    if (Z2) { add4(s2a, k2a); add4(s2b, k2b); }
  } else {
    o0.x += bz0.x + r0.x; o0.y += bz0.y + r0.y; o0.z += bz0.z + r0.z; o0.w += bz0.w + r0.w;
    o1.x += bz1.x + r1.x; o1.y += bz1.y + r1.y; o1.z += bz1.z + r1.z; o1.w += bz1.w + r1.w;
  }
  if (Z2 && row < a.n) {
    float* dp = a.dense + (int64_t)row * a.ldd + c0;
    *reinterpret_cast<f32x4*>(dp) = s2a;
    *reinterpret_cast<f32x4*>(dp + 16) = s2b;
  }
  if (a.mask) {      // dx = (x > 0) ? dx : 0: the ReLU of a relu_in layer, applied to its data gradient in the epilogue
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(a.mask + (int64_t)rowc * a.ldm + c0);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(a.mask + (int64_t)rowc * a.ldm + c0 + 16);
    o0.x = m0.x > 0.f ? o0.x : 0.f; o0.y = m0.y > 0.f ? o0.y : 0.f; o0.z = m0.z > 0.f ? o0.z : 0.f; o0.w = m0.w > 0.f ? o0.w : 0.f;
    o1.x = m1.x > 0.f ? o1.x : 0.f; o1.y = m1.y > 0.f ? o1.y : 0.f; o1.z = m1.z > 0.f ? o1.z : 0.f; o1.w = m1.w > 0.f ? o1.w : 0.f;
  }
  if (row < a.n) {
    float* yp = a.y + (int64_t)row * a.ldy + c0;
    *reinterpret_cast<f32x4*>(yp) = o0;
    *reinterpret_cast<f32x4*>(yp + 16) = o1;
  }
}

template <bool Z1, bool Z2>
__global__ __launch_bounds__(512, 2) void rowlin_kernel(const TrunkArgs a) {
  __shared__ __attribute__((aligned(16))) float bufA[STAGE_FLOATS];
  __shared__ __attribute__((aligned(16))) float bufB[STAGE_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * TROWS + wave * 16 + r;
  const int rowc = min(row, a.n - 1);
  dma_stage(a.w0p, bufA, wave, lane);
  f32x4 xr[TKG];
  {
    const float* xp = a.x + (int64_t)rowc * a.ldx + 4 * g;
#pragma unroll
    for (int t = 0; t < TKG; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + 16 * t);
      xr[t] = a.relu_in ? relu4(v) : v;
    }
  }
  // this row's table row offsets (bytes, this lane's channels 4 g ..) and weights: the same for every stage
  unsigned zo[ZK];
  float zwt[ZK];
#pragma unroll
  for (int j = 0; j < ZK; ++j) {
    zo[j] = (Z1 || Z2) ? 4u * ((unsigned)a.zidx[(int64_t)rowc * ZK + j] * (unsigned)a.ldz + 4u * g) : 0u;
    zwt[j] = (Z1 || Z2) ? a.zw[(int64_t)rowc * ZK + j] : 0.f;
  }
  dma_wait();
  __syncthreads();
  // the packed stream carries n_stages + 1 stages (the last repeats stage 0): prefetching is branch-free
#pragma clang loop unroll(disable)
  for (int s = 0; s < a.n_stages; s += 2) {
    rowlin_stage<Z1, Z2>(a, s, bufA + lane * 4, xr, row, rowc, g, a.w0p + (int64_t)(s + 1) * STAGE_FLOATS, bufB, wave, lane, zo,
                         zwt);
    dma_wait();
    __syncthreads();
    if (s + 1 < a.n_stages)
      rowlin_stage<Z1, Z2>(a, s + 1, bufB + lane * 4, xr, row, rowc, g, a.w0p + (int64_t)(s + 2) * STAGE_FLOATS, bufA, wave, lane,
                           zo, zwt);
    dma_wait();
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// Up to CHAIN_MAX residual blocks over the same rows in one launch, then optionally a rowlin (include/ext/occ4d_chain.h):
// the rows stay in registers from the first block's load to the last block's store, so a block -> block boundary costs
// neither the store / reload of x nor the single-round memory phases that go with them.  chunk() is the body of
// resblock_kernel (without its ablation switches), kept apart so that kernel's code stays what it is; it takes the two
// weight streams as arguments: "prefetch stage j + 1" of a block's last chunk takes stage 0 of the NEXT stream -- the next
// block's W0, the tail's W, or this block's own extra stage -- a wave-uniform select.  At a boundary the work is what the
// store, the launch and the load did: yacc (+= the dense rows) is x, relu(x) the next operand, x + b1 the next accumulator;
// the biases of the blocks behind the first wait in LDS from the prologue on.
constexpr int CHAIN_MAX = 3;

struct ChainBlock {
  const float* w0p; const float* b0; const float* w1p; const float* b1;
  const float* addrows; int64_t lda;         // dense rows added to this block's output rows, or null
};

struct ChainArgs {
  const float* x; int64_t ldx;
  float* y; int64_t ldy;
  int n, nb;
  ChainBlock blk[CHAIN_MAX];
  TrunkArgs tail;                            // rowlin behind the last block (y, ldy, w0p, b0, n, n_stages, relu_in); w0p null: none
};

template <bool TAIL>
__global__ __launch_bounds__(512, 2) void resblock_chain_kernel(const ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float bufA[STAGE_FLOATS];
  __shared__ __attribute__((aligned(16))) float bufB[STAGE_FLOATS];
  __shared__ __attribute__((aligned(16))) float s_b0[TH];                     // b0 of the current block
  __shared__ __attribute__((aligned(16))) float s_bn[CHAIN_MAX - 1][2][TH];   // b0, b1 of the blocks behind the first
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * TROWS + wave * 16 + r;
  const int rowc = min(row, a.n - 1);

  dma_stage(a.blk[0].w0p, bufA, wave, lane);
  if (tid < TH) {
    s_b0[tid] = a.blk[0].b0[tid];
#pragma unroll
    for (int i = 1; i < CHAIN_MAX; ++i)
      if (i < a.nb) { s_bn[i - 1][0][tid] = a.blk[i].b0[tid]; s_bn[i - 1][1][tid] = a.blk[i].b1[tid]; }
  }
  f32x4 xr[TKG], yacc[TKG];
  {
    const float* xp = a.x + (int64_t)rowc * a.ldx + 4 * g;
    const float* bp = a.blk[0].b1 + 4 * g;
#pragma unroll
    for (int t = 0; t < TKG; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + 16 * t);
      const f32x4 b = *reinterpret_cast<const f32x4*>(bp + 16 * t);
      xr[t] = relu4(v);
      yacc[t].x = v.x + b.x; yacc[t].y = v.y + b.y; yacc[t].z = v.z + b.z; yacc[t].w = v.w + b.w;
    }
  }
  dma_wait();
  __syncthreads();
  const float* const fa = bufA + lane * 4;
  const float* const fb = bufB + lane * 4;

  // one hidden chunk j of the current block: w1s = its W1 stage, w0n = the W0 stage that lands in bufA meanwhile.
  // LAST (the block's last chunk): where the block has dense rows (`add`, wave-uniform), their loads under this chunk's
  // MFMAs in the slots of resblock_kernel<true>, each behind a scalar branch -- ONE body for both kinds of block: two
  // bodies behind one branch made the register allocator split the accumulators around them
  auto chunk = [&](const int j, const float* __restrict__ w1s, const float* __restrict__ w0n, const float* add, const int lda,
                   auto last_chunk) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last_chunk)::value;
    int arow = row;
    if (LAST) asm volatile("" : "+v"(arow));
    const float* const ap = LAST ? add + (unsigned)(min(arow, a.n - 1) * lda + 4 * g) : nullptr;
    f32x4 h0 = *reinterpret_cast<const f32x4*>(s_b0 + 32 * j + 4 * g);
    f32x4 h1 = *reinterpret_cast<const f32x4*>(s_b0 + 32 * j + 16 + 4 * g);
    {
      f32x4 wa = *reinterpret_cast<const f32x4*>(fa);
      f32x4 wb = *reinterpret_cast<const f32x4*>(fa + TKG * FRAG_FLOATS);
#pragma unroll
      for (int t = 0; t < TKG; ++t) {
        if (t >= 2 && t <= 20 && (t - 2) % 3 == 0) dma_part(w1s, bufB, wave, lane, (t - 2) / 3);
        const f32x4 ca = wa, cb = wb;
        if (t + 1 < TKG) {
          wa = *reinterpret_cast<const f32x4*>(fa + (t + 1) * FRAG_FLOATS);
          wb = *reinterpret_cast<const f32x4*>(fa + (TKG + t + 1) * FRAG_FLOATS);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma16x2_b(ca, cb, xr[t], h0, h1);
        __builtin_amdgcn_sched_barrier(0);
        if (LAST && (t & 1) && t <= 21 && add) xr[(t - 1) / 2] = *reinterpret_cast<const f32x4*>(ap + 16 * ((t - 1) / 2));
      }
    }
    h0 = relu4(h0);
    h1 = relu4(h1);
    dma_wait();
    __syncthreads();
    {
      f32x4 wa = *reinterpret_cast<const f32x4*>(fb);
      f32x4 wb = *reinterpret_cast<const f32x4*>(fb + 2 * FRAG_FLOATS);
#pragma unroll
      for (int q = 0; q < TKG; ++q) {
        const int p = q >> 1, tt = q & 1;
        if (q >= 2 && q <= 20 && (q - 2) % 3 == 0) dma_part(w0n, bufA, wave, lane, (q - 2) / 3);
        if (LAST && q < TKG - 11 && add) xr[11 + q] = *reinterpret_cast<const f32x4*>(ap + 16 * (11 + q));
        const f32x4 ca = wa, cb = wb;
        if (q + 1 < TKG) {
          const int pn = (q + 1) >> 1, tn = (q + 1) & 1;
          wa = *reinterpret_cast<const f32x4*>(fb + (4 * pn + tn) * FRAG_FLOATS);
          wb = *reinterpret_cast<const f32x4*>(fb + (4 * pn + 2 + tn) * FRAG_FLOATS);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma16x2_b(ca, cb, tt ? h1 : h0, yacc[2 * p], yacc[2 * p + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    dma_wait();
    __syncthreads();
  };

#pragma clang loop unroll(disable)
  for (int bi = 0; bi < a.nb; ++bi) {
    // (wave-uniform, as everything that steers this loop.  The block's arguments are read from the kernel arguments where
    // they are used -- the empty asm keeps the reads of the last chunk's out of the loop over the first twelve, which has
    // no scalar register to spare)
    {
      const float* const w0 = a.blk[bi].w0p;
      const float* const w1 = a.blk[bi].w1p;
#pragma clang loop unroll(disable)
      for (int j = 0; j < TNS - 1; ++j)
        chunk(j, w1 + (int64_t)j * STAGE_FLOATS, w0 + (int64_t)(j + 1) * STAGE_FLOATS, nullptr, 0, std::false_type{});
    }
    int bl = bi;
    asm volatile("" : "+s"(bl));
    const bool lastb = bl + 1 == a.nb;
    const float* const w0n = !lastb ? a.blk[bl + 1].w0p : TAIL ? a.tail.w0p : a.blk[bl].w0p + (int64_t)TNS * STAGE_FLOATS;
    const float* const add = a.blk[bl].addrows;
    chunk(TNS - 1, a.blk[bl].w1p + (int64_t)(TNS - 1) * STAGE_FLOATS, w0n, add, (int)a.blk[bl].lda, std::true_type{});
    if (add) {
#pragma unroll
      for (int t = 0; t < TKG; ++t) { yacc[t].x += xr[t].x; yacc[t].y += xr[t].y; yacc[t].z += xr[t].z; yacc[t].w += xr[t].w; }
    }
    if (!lastb) {
      // the boundary: yacc is x.  Every wave is past the chunk's last barrier, so past its last read of s_b0
      if (tid < TH) s_b0[tid] = s_bn[bl][0][tid];
      const float* const bp = &s_bn[bl][1][4 * g];
#pragma unroll
      for (int t = 0; t < TKG; ++t) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(bp + 16 * t);
        xr[t] = relu4(yacc[t]);
        yacc[t].x += b.x; yacc[t].y += b.y; yacc[t].z += b.z; yacc[t].w += b.w;
      }
      __syncthreads();
    }
  }
  if (row < a.n) {
    float* yp = a.y + (int64_t)row * a.ldy + 4 * g;
#pragma unroll
    for (int t = 0; t < TKG; ++t) *reinterpret_cast<f32x4*>(yp + 16 * t) = yacc[t];
  }
  if (TAIL) {
    // the stage loop of rowlin_kernel<false, false> on the rows in registers; stage 0 landed in bufA under the last chunk
#pragma unroll
    for (int t = 0; t < TKG; ++t) xr[t] = a.tail.relu_in ? relu4(yacc[t]) : yacc[t];
#pragma clang loop unroll(disable)
    for (int s = 0; s < a.tail.n_stages; s += 2) {
      rowlin_stage<false, false>(a.tail, s, bufA + lane * 4, xr, row, rowc, g, a.tail.w0p + (int64_t)(s + 1) * STAGE_FLOATS, bufB,
                                 wave, lane, nullptr, nullptr);
      dma_wait();
      __syncthreads();
      if (s + 1 < a.tail.n_stages)
        rowlin_stage<false, false>(a.tail, s + 1, bufB + lane * 4, xr, row, rowc, g, a.tail.w0p + (int64_t)(s + 2) * STAGE_FLOATS,
                                   bufA, wave, lane, nullptr, nullptr);
      dma_wait();
      __syncthreads();
    }
  }
}

// Host side of the rowlin entry points: the argument checks (`masked`: a mask is required) and the launch.  The terms of
// `a` (ztab: added; ztab2: stored to a.dense) run inside the stages: kz == 8 and 32-bit table offsets, which
// occ4d_rowlin_linz_f32 checks (occ4d_rowlin_f32 never passes a term down here).
int rowlin_launch(const char* who, const TrunkArgs& a, int n_out, bool masked, void* stream) {
  if (int rc = occ4d::check_rowlin_args(a, who, TH, 32, n_out, masked)) return rc;
  const dim3 grid(occ4d::cdiv(a.n, TROWS));
  hipStream_t st = (hipStream_t)stream;
  if (a.ztab && a.ztab2) rowlin_kernel<true, true><<<grid, 512, 0, st>>>(a);
  else if (a.ztab) rowlin_kernel<true, false><<<grid, 512, 0, st>>>(a);
  else if (a.ztab2) rowlin_kernel<false, true><<<grid, 512, 0, st>>>(a);
  else rowlin_kernel<false, false><<<grid, 512, 0, st>>>(a);
  return occ4d::check_launch(who);
}

TrunkArgs rowlin_args(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed, const float* b, int n_out,
                      int relu_in, const float* res, int64_t ldr, const float* mask, int64_t ldm, int n) {
  TrunkArgs a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w0p = w_packed; a.b0 = b; a.res = res; a.ldr = ldr;
  a.n = n; a.n_stages = n_out / 32; a.relu_in = relu_in; a.mask = mask; a.ldm = ldm;
  return a;
}

using occ4d::spans_overlap;

}  // namespace

extern "C" int occ4d_trunk_width(void) { return TH; }
extern "C" int64_t occ4d_trunk_packed_floats(int n_out) { return (int64_t)(n_out / 32 + 1) * STAGE_FLOATS; }

// occ4d_resblock_f32 keeps its interpolation arguments: the term is the stand-alone pass behind the block (the block's
// own epilogue of exposed gathers is gone; the decoder hides the term with occ4d_resblock_addrows_f32)
extern "C" int occ4d_resblock_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w0_packed,
                                  const float* b0, const float* w1_packed, const float* b1, const float* zconst,
                                  const float* ztab, int64_t ldz, const int32_t* zidx, const float* zw, int kz, int n,
                                  void* stream) {
  TrunkArgs a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w0p = w0_packed; a.b0 = b0; a.w1p = w1_packed; a.b1 = b1;
  a.zconst = zconst; a.ztab = ztab; a.ldz = ldz; a.zidx = zidx; a.zw = zw; a.kz = kz; a.n = n; a.n_stages = TNS; a.relu_in = 1;
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  if (int rc = occ4d::check_trunk_args(a, "occ4d_resblock_f32", TH)) return rc;
  OCC4D_REQUIRE(w1_packed && b1 && ((uintptr_t)w1_packed % 16) == 0 && ((uintptr_t)b1 % 16) == 0 && ldy >= TH,
                "occ4d_resblock_f32: second layer weights / bias missing or misaligned");
  resblock_kernel<false><<<occ4d::cdiv(n, TROWS), 512, 0, (hipStream_t)stream>>>(a);
  if (int rc = occ4d::check_launch("occ4d_resblock_f32")) return rc;
  return ztab ? occ4d_interp_add_f32(y, ldy, zconst, ztab, ldz, zidx, zw, n, kz, TH, stream) : OCC4D_OK;
}

// y = x + W1 relu(W0 relu(x) + b0) + b1 + addrows: the dense rows are added last, from loads that sit under the last
// hidden chunk's MFMAs (include/ext/occ4d_linz.h)
extern "C" int occ4d_resblock_addrows_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w0_packed,
                                          const float* b0, const float* w1_packed, const float* b1, const float* addrows,
                                          int64_t ld_add, int n, void* stream) {
  const char* who = "occ4d_resblock_addrows_f32";
  TrunkArgs a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w0p = w0_packed; a.b0 = b0; a.w1p = w1_packed; a.b1 = b1;
  a.addrows = addrows; a.lda = ld_add; a.n = n; a.n_stages = TNS; a.relu_in = 1;
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  if (int rc = occ4d::check_trunk_args(a, who, TH)) return rc;
  OCC4D_REQUIRE(w1_packed && b1 && ((uintptr_t)w1_packed % 16) == 0 && ((uintptr_t)b1 % 16) == 0 && ldy >= TH,
                "%s: second layer weights / bias missing or misaligned", who);
  if (int rc = occ4d::check_addrows_args(a, who, TH)) return rc;
  resblock_kernel<true><<<occ4d::cdiv(n, TROWS), 512, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch(who);
}

// nb residual blocks over the same rows in one launch, the rows in registers between them, optionally the rowlin behind the
// last one (include/ext/occ4d_chain.h)
extern "C" int occ4d_resblock_chain_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int nb,
                                        const float* w0_0, const float* b0_0, const float* w1_0, const float* b1_0,
                                        const float* add_0, int64_t lda_0, const float* w0_1, const float* b0_1,
                                        const float* w1_1, const float* b1_1, const float* add_1, int64_t lda_1,
                                        const float* w0_2, const float* b0_2, const float* w1_2, const float* b1_2,
                                        const float* add_2, int64_t lda_2, const float* w_tail, const float* b_tail,
                                        int n_tail, int relu_in_tail, float* y_tail, int64_t ld_tail, int n, void* stream) {
  const char* who = "occ4d_resblock_chain_f32";
  OCC4D_REQUIRE(nb >= 1 && nb <= CHAIN_MAX, "%s: nb = %d blocks (1 .. %d: split a longer run)", who, nb, CHAIN_MAX);
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  ChainArgs c{};
  c.x = x; c.ldx = ldx; c.y = y; c.ldy = ldy; c.n = n; c.nb = nb;
  const ChainBlock given[CHAIN_MAX] = {{w0_0, b0_0, w1_0, b1_0, add_0, lda_0}, {w0_1, b0_1, w1_1, b1_1, add_1, lda_1},
                                       {w0_2, b0_2, w1_2, b1_2, add_2, lda_2}};
  const bool tail = w_tail != nullptr;
  for (int i = 0; i < nb; ++i) {
    const ChainBlock& k = c.blk[i] = given[i];
    TrunkArgs a{};                           // the block as a launch of its own: the same checks, the same messages
    a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w0p = k.w0p; a.b0 = k.b0; a.w1p = k.w1p; a.b1 = k.b1;
    a.addrows = k.addrows; a.lda = k.lda; a.n = n;
    if (int rc = occ4d::check_trunk_args(a, who, TH)) return rc;
    OCC4D_REQUIRE(k.w1p && k.b1 && ((uintptr_t)k.w1p % 16) == 0 && ((uintptr_t)k.b1 % 16) == 0 && ldy >= TH,
                  "%s: second layer weights / bias missing or misaligned (block %d)", who, i);
    if (k.addrows) {
      if (int rc = occ4d::check_addrows_args(a, who, TH)) return rc;
      OCC4D_REQUIRE(!tail || !spans_overlap(k.addrows, k.lda, TH, y_tail, ld_tail, n_tail, n),
                    "%s: addrows must not alias y_tail (block %d)", who, i);
    }
  }
  if (!tail) {
    OCC4D_REQUIRE(!b_tail && !y_tail, "%s: b_tail / y_tail given without w_tail", who);
    resblock_chain_kernel<false><<<occ4d::cdiv(n, TROWS), 512, 0, (hipStream_t)stream>>>(c);
    return occ4d::check_launch(who);
  }
  c.tail = rowlin_args(y, ldy, y_tail, ld_tail, w_tail, b_tail, n_tail, relu_in_tail, nullptr, 0, nullptr, 0, n);
  OCC4D_REQUIRE(n_tail >= 32 && n_tail % 32 == 0, "%s: n_tail = %d must be a multiple of 32", who, n_tail);
  if (int rc = occ4d::check_rowlin_args(c.tail, who, TH, 32, n_tail, false)) return rc;
  OCC4D_REQUIRE(!spans_overlap(y_tail, ld_tail, n_tail, x, ldx, TH, n) && !spans_overlap(y_tail, ld_tail, n_tail, y, ldy, TH, n),
                "%s: y_tail must not alias x or y", who);
  resblock_chain_kernel<true><<<occ4d::cdiv(n, TROWS), 512, 0, (hipStream_t)stream>>>(c);
  return occ4d::check_launch(who);
}

extern "C" int occ4d_rowlin_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed,
                                const float* b, int n_out, int relu_in, const float* res, int64_t ldr,
                                const float* zconst, const float* ztab, int64_t ldz, const int32_t* zidx,
                                const float* zw, int kz, int n, void* stream) {
  const char* who = "occ4d_rowlin_f32";
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  TrunkArgs a = rowlin_args(x, ldx, y, ldy, w_packed, b, n_out, relu_in, res, ldr, nullptr, 0, n);
  a.zconst = zconst; a.ztab = ztab; a.ldz = ldz; a.zidx = zidx; a.zw = zw; a.kz = kz;
  if (!ztab) return rowlin_launch(who, a, n_out, false, stream);
  // the interpolation arguments keep working, for any kz and any table size: the contract as before, the term as the
  // stand-alone pass behind the plain launch (inside the stages: occ4d_rowlin_linz_f32)
  if (int rc = occ4d::check_rowlin_args(a, who, TH, 32, n_out, false)) return rc;
  a.zconst = a.ztab = nullptr;
  if (int rc = rowlin_launch(who, a, n_out, false, stream)) return rc;
  return occ4d_interp_add_f32(y, ldy, zconst, ztab, ldz, zidx, zw, n, kz, n_out, stream);
}

// occ4d_rowlin_f32 with up to two interpolation terms over the same neighbour lists, both inside the stages: the first
// added to y, the second stored to `dense` (include/ext/occ4d_linz.h)
extern "C" int occ4d_rowlin_linz_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed,
                                     const float* b, int n_out, int relu_in, const float* res, int64_t ldr,
                                     const float* zconst, const float* ztab, const float* zconst2, const float* ztab2,
                                     int64_t ldz, int zrows, const int32_t* zidx, const float* zw, int kz, float* dense,
                                     int64_t ldd, int n, void* stream) {
  const char* who = "occ4d_rowlin_linz_f32";
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  TrunkArgs a = rowlin_args(x, ldx, y, ldy, w_packed, b, n_out, relu_in, res, ldr, nullptr, 0, n);
  a.zconst = zconst; a.ztab = ztab; a.ldz = ldz; a.zidx = zidx; a.zw = zw; a.kz = kz;
  a.zconst2 = zconst2; a.ztab2 = ztab2; a.dense = dense; a.ldd = ldd; a.zrows = zrows;
  if (int rc = occ4d::check_linz_args(a, who, ZK, n_out)) return rc;
  return rowlin_launch(who, a, n_out, false, stream);
}

// y = mask > 0 ? ([res +] W [relu](x) + b) : 0 -- occ4d_rowlin_f32 with the ReLU mask of a data gradient applied in
// the epilogue (training: dx of a relu_in layer = (x > 0) . (g W); the separate masking pass read and wrote dx again)
extern "C" int occ4d_rowlin_masked_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w_packed,
                                       const float* b, int n_out, int relu_in, const float* res, int64_t ldr,
                                       const float* mask, int64_t ldm, int n, void* stream) {
  if (n == 0) return OCC4D_OK;               // (an empty batch has no storage: nothing to check)
  return rowlin_launch("occ4d_rowlin_masked_f32", rowlin_args(x, ldx, y, ldy, w_packed, b, n_out, relu_in, res, ldr, mask, ldm, n),
                       n_out, true, stream);
}
