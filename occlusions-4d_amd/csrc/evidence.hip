// Measured returns carved into the query grid (include/ext/occ4d_evidence.h).  The snap, the walk, the body of a return, the code of
// a cell and the argument contracts are csrc/evidence_math.hpp, shared with the g++ twin; where the marks land, the reductions and
// the launches are here.
//
// Two launches per entry point, whatever the data: a clear and the work.  (Kernels, never hipMemset: see csrc/common.hpp.)
//   carve     one return per thread, a wave takes 64 consecutive returns: neighbours of a sweep, whose walks share their cells near
//             the sensor.  Workgroups loop over their share of the returns, `rounds` times, a bound fixed on the host.  hits: one
//             global integer add per return.  passes (optional): global integer adds behind a wave match (below).  status: four ballots per
//             round, one LDS add per wave, one global add per workgroup and slot.
//             WHERE THE PASSED BITS ARE MARKED.  Both placements are built over the one body below and differ in a template
//             argument only:  (a) an integer OR straight into the global bit array -- the word is read first, and the OR is
//             issued only when the bit is not set yet: near a sensor thousands of rays mark the same few cells, and a stale read
//             costs one redundant OR, never a bit;  (b) the workgroup's own copy of the whole bit array in LDS (66 816 bytes at
//             96 x 96 x 58), marked with LDS ORs behind the same test, the non-zero words ORed into global memory at the end: at
//             most two workgroups of 512 threads per CU, each looping over its share of the returns.  Timed in the same runs at
//             96 x 96 x 58, three runs (profiles/r12_evidence_timing.txt): (a) took 2.7 - 8.9 x the device time of
//             (b) on every bundle -- 0.113 against 0.041 ms for 21 858 returns of one sweep, 0.52 against 0.091 ms for 46 092 of three
//             sensors, 0.49 against 0.135 ms for 172 000 over 36 sensors: the test before the OR puts a read of L2 on every step of
//             the walk, the same read of LDS costs a fraction -- the way csrc/pull.hip came out, the opposite of csrc/sight.hip.  So
//             the bits are staged whenever they fit OCC4D_EVIDENCE_LDS_WORDS (128 KiB: grids of up to 2^20 cells); a larger grid,
//             which no LDS holds, is marked where it is.  A rule of capacity, not a switch: no flag, no environment variable.
//             HOW passes IS ADDED.  It cannot be staged (2 MB of int32 at that grid).  One global add per lane and passed cell
//             serialises near a sensor -- every walk that reaches its sensor passes the sensor's own cell: 0.31 - 0.59 ms on the
//             lidar bundles.  THE WAVE MATCH (add_matched below) adds one count per distinct cell among the lanes of a step:
//             0.13 - 0.28 ms there, 0.34 - 0.57 x, and 1.05 x on 172 000 random returns (0.60 against 0.58 ms: nothing to match).
//             Kept.  A second match, of the cells in which the walks END at their sensor, made after the walk where the whole
//             wave meets, was built too: alone 0.20 - 0.31 ms, on top of the per-step match + 0.002 ms -- lanes that arrive in
//             one step are matched by that step already, PROVIDED the sensor's cell has a call site of its own in the walk
//             (arrive() below): with one site for all cells the lidar bundles took 0.14 - 0.44 ms.  The second match lost and is
//             removed.
//   classify  one thread per cell, `rounds` consecutive chunks per workgroup: the code, six ballots per chunk counted per wave,
//             one LDS add per wave and code, six 64-bit global adds per workgroup.
// Integer atomics only: sums and ORs commute, so every output bit is the same under any scheduling.  No workgroup waits for
// another one, no inline assembly.
#include "common.hpp"
#include "evidence_math.hpp"
#include "ext/occ4d_evidence.h"

namespace {

namespace ev = occ4d_evidence;
namespace sm = occ4d_sight;

constexpr int FLAT = 256;                                         // clear, classify, carve (a): grids above 2^20 cells
constexpr int STAGED = 512;                                       // carve (b): two workgroups of 8 waves share a CU's LDS
constexpr int64_t LDS_WORDS = OCC4D_EVIDENCE_LDS_WORDS;
static_assert(LDS_WORDS * 4 + 64 <= 160 * 1024, "the staged bits and the reduction words fit the LDS of a CU");

__global__ __launch_bounds__(FLAT) void evidence_clear_kernel(uint32_t* passed, int64_t words, int32_t* hits, int32_t* passes, int64_t n,
                                                              int32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (i < n) hits[i] = 0;
  if (passes && i < n) passes[i] = 0;
  if (i < words) passed[i] = 0u;
  if (i < 4) status[i] = 0;
}

__global__ __launch_bounds__(64) void evidence_clear_totals_kernel(int64_t* totals) {
  if (threadIdx.x < 6) totals[threadIdx.x] = 0;
}

// Experiments only (OCC4D_HIPCC_EXTRA, profiles/evidence_timing.py --other): -DOCC4D_EVIDENCE_MATCH=0 adds `passes` one lane at a
// time, without the wave match; -DOCC4D_EVIDENCE_GLOBAL_BITS marks the passed bits in global memory whatever the grid.  The
// library as built has neither define.
#ifndef OCC4D_EVIDENCE_MATCH
#define OCC4D_EVIDENCE_MATCH 1
#endif
constexpr bool MATCH = OCC4D_EVIDENCE_MATCH != 0;
constexpr int MATCH_ROUNDS = 2;

// THE WAVE MATCH of one step of the walk: the lanes that are here -- those whose walks are still under way -- add one count per
// distinct cell instead of one per lane.  Up to MATCH_ROUNDS times the lowest lane left is the leader, the lanes with its cell are
// counted with a ballot and the leader adds the count; who is left after that adds on its own.  Sums commute: the same counts.
__device__ __forceinline__ void add_matched(int32_t* passes, int32_t flat) {
  bool mine = true;
  unsigned long long todo = __ballot(mine);
  const int lane = threadIdx.x & 63;
  for (int i = 0; i < MATCH_ROUNDS && todo; ++i) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t cell = __shfl(flat, leader);
    const unsigned long long same = __ballot(mine && flat == cell);
    if (lane == leader) atomicAdd(passes + cell, (int32_t)__popcll(same));
    todo &= ~same;
    if (flat == cell) mine = false;
  }
  if (mine) atomicAdd(passes + flat, 1);
}

// the marks of a return: `words` is the global bit array or the workgroup's copy in LDS
template <bool LDS>
struct Marks {
  uint32_t* words;
  int32_t *hits, *passes;
  __device__ __forceinline__ void hit(int32_t flat) const { atomicAdd(hits + flat, 1); }
  __device__ __forceinline__ void pass(int32_t flat) const {
    uint32_t* w = words + (flat >> 5);
    const uint32_t bit = 1u << (flat & 31);
    const uint32_t now = LDS ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                             : __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!(now & bit)) {
      if (LDS) __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (passes) {
      if (MATCH) add_matched(passes, flat);
      else atomicAdd(passes + flat, 1);
    }
  }
  // The sensor's own cell, which ends a walk: the same marks, but a call site of its own in the walk, so that the lanes that
  // arrive in one step are matched among themselves -- in pass() the two leader rounds can go to lanes that pass other cells.
  __device__ __forceinline__ void arrive(int32_t flat) const { pass(flat); }
};

template <bool LDS>
__global__ __launch_bounds__(STAGED) void evidence_carve_kernel(const ev::CarveArgs a, const int rounds) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_words[];
  __shared__ int32_t s_status[4];
  const int t = threadIdx.x, threads = blockDim.x;
  if (LDS)
    for (int64_t i = t; i < a.words; i += threads) s_words[i] = 0u;
  if (t < 4) s_status[t] = 0;
  __syncthreads();
  const Marks<LDS> marks{LDS ? s_words : a.passed, a.hits, a.passes};
  int count[4] = {0, 0, 0, 0};                                    // the same in every lane of a wave
  for (int round = 0; round < rounds; ++round) {
    const int64_t r = ((int64_t)round * gridDim.x + blockIdx.x) * threads + t;
    const int slot = r < a.R ? ev::return_item(a, r, marks) : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) count[k] += __popcll(__ballot(slot == k));
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (count[k]) atomicAdd(&s_status[k], count[k]);
  }
  __syncthreads();
  if (LDS)
    for (int64_t i = t; i < a.words; i += threads) {
      const uint32_t w = s_words[i];
      if (w) atomicOr(a.passed + i, w);
    }
  if (t < 4 && s_status[t]) atomicAdd(a.status + t, s_status[t]);
}

__global__ __launch_bounds__(FLAT) void evidence_classify_kernel(const ev::ClassifyArgs a, const int rounds) {
  __shared__ int32_t s_totals[6];
  const int t = threadIdx.x;
  if (t < 6) s_totals[t] = 0;
  __syncthreads();
  int count[6] = {0, 0, 0, 0, 0, 0};                              // the same in every lane of a wave
  for (int round = 0; round < rounds; ++round) {
    const int64_t p = ((int64_t)blockIdx.x * rounds + round) * FLAT + t;
    int code = -1;
    if (p < a.solid.n) a.code[p] = code = ev::code_of(a, p);
#pragma unroll
    for (int k = 0; k < 6; ++k) count[k] += __popcll(__ballot(code == k));
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (count[k]) atomicAdd(&s_totals[k], count[k]);
  }
  __syncthreads();
  if (t < 6 && s_totals[t]) atomicAdd((unsigned long long*)a.totals + t, (unsigned long long)s_totals[t]);
}

}  // namespace

extern "C" int occ4d_evidence_carve_f32(const float* returns, int64_t ld_returns, int64_t R, const int32_t* sensor, const int32_t* origins,
                                        int V, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0, float sz,
                                        uint32_t* passed, int32_t* hits, int32_t* passes, int32_t* status, void* stream) {
  ev::CarveArgs a;
  OCC4D_TRY(ev::check_carve(returns, ld_returns, R, sensor, origins, V, nx, ny, nz, x0, sx, y0, sy, z0, sz, passed, hits, passes, status, a));
  hipStream_t st = (hipStream_t)stream;
  const int64_t cleared = a.points > 4 ? a.points : 4;            // <= 2^27
  evidence_clear_kernel<<<(unsigned)((cleared + FLAT - 1) / FLAT), FLAT, 0, st>>>(passed, a.words, hits, passes, a.points, status);
  OCC4D_TRY(occ4d::check_launch("occ4d_evidence_carve_f32"));
  if (R == 0) return OCC4D_OK;
  const int cus = occ4d::cu_count();
#ifdef OCC4D_EVIDENCE_GLOBAL_BITS
  const bool staged = false;
#else
  const bool staged = a.words <= LDS_WORDS;
#endif
  if (staged) {
    static thread_local int raised_on = -1;                       // the device whose limit of dynamic LDS was raised last
    int device = -1;
    if (hipGetDevice(&device) == hipSuccess && device != raised_on &&
        hipFuncSetAttribute((const void*)evidence_carve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_WORDS * 4)) == hipSuccess)
      raised_on = device;
    const int64_t want = (R + STAGED - 1) / STAGED, most = 2 * (int64_t)cus;
    const int blocks = (int)(want < most ? want : most);
    const int rounds = (int)((R + (int64_t)blocks * STAGED - 1) / ((int64_t)blocks * STAGED));
    evidence_carve_kernel<true><<<(unsigned)blocks, STAGED, (size_t)a.words * 4, st>>>(a, rounds);
  } else {
    const int64_t want = (R + FLAT - 1) / FLAT, most = 8 * (int64_t)cus;
    const int blocks = (int)(want < most ? want : most);
    const int rounds = (int)((R + (int64_t)blocks * FLAT - 1) / ((int64_t)blocks * FLAT));
    evidence_carve_kernel<false><<<(unsigned)blocks, FLAT, 0, st>>>(a, rounds);
  }
  return occ4d::check_launch("occ4d_evidence_carve_f32");
}

extern "C" int occ4d_evidence_classify_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                                           int64_t n, const uint32_t* passed, const int32_t* passes, int min_pass, const int32_t* hits,
                                           int32_t* code, int64_t* totals, void* stream) {
  ev::ClassifyArgs a;
  OCC4D_TRY(ev::check_classify(field, ld, level, mask, ld_mask, mask_level, n, passed, passes, min_pass, hits, code, totals, a));
  hipStream_t st = (hipStream_t)stream;
  evidence_clear_totals_kernel<<<1, 64, 0, st>>>(totals);
  OCC4D_TRY(occ4d::check_launch("occ4d_evidence_classify_f32"));
  if (n == 0) return OCC4D_OK;
  const int64_t chunks = (n + FLAT - 1) / FLAT, most = 4 * (int64_t)occ4d::cu_count();
  const int rounds = (int)((chunks + most - 1) / most);           // chunks of a workgroup
  const int blocks = (int)((chunks + rounds - 1) / rounds);
  evidence_classify_kernel<<<(unsigned)blocks, FLAT, 0, st>>>(a, rounds);
  return occ4d::check_launch("occ4d_evidence_classify_f32");
}
