// Straight free legs over the grid (include/ext/occ4d_pull.h).  The blocked test, HIT over the walk of csrc/sight_math.hpp, the test
// of one candidate and the argument contracts are csrc/pull_math.hpp, shared with the g++ twin; the ballots, the reduction through
// LDS, the barriers and the launches are here.
//
// One launch per entry point, whatever the data.
//   bits   one thread per grid point, the blocked test, a ballot: lanes 0 and 32 of a wave store its two words.  Lanes behind n vote
//          0, which clears the unused bits of the last word.
//   pairs  one thread per pair, one store per pair.
//   paths  one workgroup of 256 threads per goal; the chain position k of the anchor, the number of waypoints and every loop bound
//          are the same in every thread.  Per anchor the candidates are scanned from the far end in rounds of 256: thread t tests
//          j = top - t, so within a wave the lowest voting lane holds the wave's largest free j; lane 0 of each wave puts it in LDS,
//          one barrier, every thread takes the maximum of the four words.  The first round with a hit ends the scan.  The four
//          words are double-buffered by the parity of the round's number, so one barrier per round is enough: a thread writes a
//          buffer again only after the barrier of the round between, which every thread passes after its reads.  Thread 0 stores the
//          waypoints; behind the loop all threads store the -1 of the row's tail, which no thread wrote before.
//          Barriers stand in uniform control flow only.  The loops are `for`s with bounds fixed before they start: anchors <= cap,
//          rounds <= ceil(cap / 256), the walk's nx + ny + nz.
//          WHERE THE BITS ARE READ.  This kernel is latency-bound: few workgroups, and every step of a walk waits for a word.  Both
//          placements were built over the one body below and timed in the same runs at 96 x 96 x 58 (66 816 bytes of bits), 1, 16 and
//          256 goals on three fields, three runs: reads from global memory took 1.04 - 1.16 x the device time of the workgroup's own
//          copy in LDS, staged once, in all 27 comparisons (DESIGN 7c rank 20 has both sets of figures) -- the opposite of
//          csrc/sight.hip's throughput case, where the copy per workgroup lost.  So the bits are staged in LDS whenever they fit
//          OCC4D_PULL_LDS_WORDS (128 KiB: grids of up to 2^20 points); a larger grid, which no LDS holds, is read where it is.  That
//          is a rule of capacity, not a switch: no flag, no environment variable.
// No atomics, no inter-workgroup waits, no inline assembly, no floats.
#include "common.hpp"
#include "pull_math.hpp"
#include "ext/occ4d_pull.h"

namespace {

namespace pm = occ4d_pull;
namespace sm = occ4d_sight;

constexpr int FLAT = pm::ROUND;
constexpr int WAVES = FLAT / 64;
constexpr int64_t LDS_WORDS = OCC4D_PULL_LDS_WORDS;               // the most words staged
static_assert(LDS_WORDS * 4 + 64 <= 160 * 1024, "the staged bits and the reduction words fit the LDS of a CU");

__global__ __launch_bounds__(FLAT) void pull_bits_kernel(const pm::BitsArgs a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const unsigned long long votes = __ballot(p < a.n && pm::blocked_at(a, p));
  const int lane = threadIdx.x & 63;
  const int64_t word = p >> 5;                                    // (p of lanes 0 and 32 is a multiple of 32)
  if ((lane & 31) == 0 && word < a.words) a.blocked[word] = (uint32_t)(votes >> lane);
}

__global__ __launch_bounds__(FLAT) void pull_pairs_kernel(const pm::PairArgs a) {
  const int64_t i = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (i < a.n_pairs) a.hit[i] = pm::hit(a.n, a.points, sm::GlobalWords{a.blocked}, a.a[i], a.b[i]);
}

template <class Words>
__device__ __forceinline__ void pull_goal(const pm::PathArgs& a, const Words& words, int32_t (*s_best)[WAVES]) {
  const int g = blockIdx.x, t = threadIdx.x;
  const int32_t* row = a.paths + (int64_t)g * a.cap;
  int32_t* out = a.waypoints + (int64_t)g * a.cap;
  const int L = pm::chain_length(a, g);
  int k = 0, count = 0, flip = 0;
  for (int anchor = 0; anchor < a.cap && L > 0; ++anchor) {
    if (t == 0) out[count] = row[k];
    ++count;
    if (k >= L - 1) break;
    int next = k + 1;                                             // the fallback: the original move, untested
    for (int r = 0; r < a.rounds; ++r) {
      const int top = L - 1 - r * FLAT;
      if (top <= k + 1) break;                                    // (the same in every thread)
      const int j = top - t;
      const unsigned long long votes = __ballot(pm::candidate_free(a, words, row, L, k, j));
      if ((t & 63) == 0) s_best[flip][t >> 6] = votes ? top - (t + __builtin_ctzll(votes)) : -1;
      __syncthreads();
      int best = s_best[flip][0];
      for (int w = 1; w < WAVES; ++w) best = s_best[flip][w] > best ? s_best[flip][w] : best;
      flip ^= 1;
      if (best >= 0) { next = best; break; }
    }
    k = next;
  }
  for (int c = count + t; c < a.cap; c += FLAT) out[c] = -1;
  if (t == 0) a.waypoint_len[g] = L > 0 ? count : a.path_len[g];
}

__global__ __launch_bounds__(FLAT) void pull_paths_kernel(const pm::PathArgs a) {
  __shared__ int32_t s_best[2][WAVES];
  pull_goal(a, sm::GlobalWords{a.blocked}, s_best);
}

struct LdsWords {
  const uint32_t* bits;
  __device__ __forceinline__ uint32_t operator()(int32_t i) const { return bits[i]; }
};

__global__ __launch_bounds__(FLAT) void pull_paths_lds_kernel(const pm::PathArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_words[];
  __shared__ int32_t s_best[2][WAVES];
  for (int64_t i = threadIdx.x; i < a.words; i += FLAT) s_words[i] = a.blocked[i];
  __syncthreads();
  pull_goal(a, LdsWords{s_words}, s_best);
}

}  // namespace

extern "C" int occ4d_pull_bits_i32(const int32_t* clear, int min_clear, int64_t n, uint32_t* blocked, void* stream) {
  pm::BitsArgs a; bool empty;
  OCC4D_TRY(pm::check_bits(clear, min_clear, n, blocked, empty, a));
  if (empty) return OCC4D_OK;
  pull_bits_kernel<<<(unsigned)((n + FLAT - 1) / FLAT), FLAT, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch("occ4d_pull_bits_i32");
}

extern "C" int occ4d_pull_pairs_u32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* a, const int32_t* b, int n_pairs,
                                    int32_t* hit, void* stream) {
  pm::PairArgs args; bool empty;
  OCC4D_TRY(pm::check_pairs(blocked, nx, ny, nz, a, b, n_pairs, hit, empty, args));
  if (empty) return OCC4D_OK;
  pull_pairs_kernel<<<(unsigned)(((int64_t)n_pairs + FLAT - 1) / FLAT), FLAT, 0, (hipStream_t)stream>>>(args);
  return occ4d::check_launch("occ4d_pull_pairs_u32");
}

extern "C" int occ4d_pull_paths_i32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* paths, const int32_t* path_len,
                                    int n_goals, int cap, int32_t* waypoints, int32_t* waypoint_len, void* stream) {
  pm::PathArgs a; bool empty;
  OCC4D_TRY(pm::check_paths(blocked, nx, ny, nz, paths, path_len, n_goals, cap, waypoints, waypoint_len, empty, a));
  if (empty) return OCC4D_OK;
  if (a.words <= LDS_WORDS) {
    static thread_local int raised_on = -1;                       // the device whose limit of dynamic LDS was raised last
    int device = -1;
    if (hipGetDevice(&device) == hipSuccess && device != raised_on &&
        hipFuncSetAttribute((const void*)pull_paths_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_WORDS * 4)) == hipSuccess)
      raised_on = device;
    pull_paths_lds_kernel<<<(unsigned)n_goals, FLAT, (size_t)a.words * 4, (hipStream_t)stream>>>(a);
  } else {
    pull_paths_kernel<<<(unsigned)n_goals, FLAT, 0, (hipStream_t)stream>>>(a);
  }
  return occ4d::check_launch("occ4d_pull_paths_i32");
}
