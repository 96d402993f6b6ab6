// The next best view over the grid (include/ext/occ4d_viewplan.h).  DEAD, RANGE, the test of one (candidate, point) pair over the walk
// of csrc/sight_math.hpp, the layout of the work array, the keys of GREEDY and the argument contracts are csrc/viewplan_math.hpp,
// shared with the g++ twin; the ballots, the reductions, the barriers and the launches are here.
//
//   vis    ONE launch.  A thread owns one flat index p, a wave 64 consecutive ones: two words of a row, as in sight_bits_kernel.
//          blockIdx.y chooses CHUNK consecutive candidates, which the thread takes one after the other: p's coordinates and its
//          target bit are decoded once for all of them, and a wave without any target bit -- unobserved space comes in runs -- stores
//          its zeros and walks nothing.  The candidate's number is the same in every lane, so its coordinates, its DEAD test and the
//          word of `solid` it stands in are scalar work.  Lanes without a target bit, behind n, or out of range vote 0 without
//          walking.  Every bit of `solid` is read from global memory, as in csrc/sight.hip: this is that kernel's throughput shape.
//   init   remaining = targets, the C + 1 counts 0, the flag word 1.
//   count  grid (slices of SLICE words, rows): the popcounts of vis[row] & remaining over a slice, summed over the wave by shuffles,
//          over the workgroup through LDS, ONE integer atomicAdd per workgroup to count[row] (none for a sum of 0): integer addition,
//          so the order cannot matter.  Round 0 has one row more, all ones: popcount(targets).
//   pick   ONE workgroup of 1024 threads: the largest key (count, lowest c) over the candidates -- a thread's own, the wave's by
//          shuffles, the workgroup's through LDS --, round 0 also gain and status; then remaining &= ~vis[best] with its popcount,
//          the counts cleared for the next round.  Both launches of a round return at once where the flag word is 0.
// The flag word and the counts are written by an earlier launch than the one that reads them: no workgroup waits for another one.
// Barriers stand in uniform control flow only: the conditions before them depend on kernel arguments, on the flag word and on the
// workgroup's reduced key alone.  Every loop is a `for` with a bound fixed before it starts.  No inline assembly, no floats.
#include "common.hpp"
#include "viewplan_math.hpp"
#include "ext/occ4d_viewplan.h"

namespace {

namespace vm = occ4d_viewplan;
namespace sm = occ4d_sight;

constexpr int FLAT = 256;
constexpr int WAVES = FLAT / 64;
constexpr int PICK = 1024;
constexpr int PICK_WAVES = PICK / 64;
static_assert(vm::SLICE % FLAT == 0, "a slice is whole passes of a workgroup");
static_assert(vm::MAX_CANDIDATES % PICK == 0, "the candidates are whole passes of the picking workgroup");

__global__ __launch_bounds__(FLAT) void viewplan_vis_kernel(const vm::VisArgs a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t word = p >> 5;                                    // (p of lanes 0 and 32 is a multiple of 32)
  const bool owner = (lane & 31) == 0 && word < a.words;
  const bool target = vm::target_at(a, p);
  const bool walks = __ballot(target) != 0;                       // the same in every lane of the wave
  int px = 0, py = 0, pz = 0;
  if (target) vm::point_of(a, (int32_t)p, px, py, pz);
  const sm::GlobalWords words{a.solid};
  const int c0 = blockIdx.y * vm::CHUNK, c1 = c0 + vm::CHUNK < a.C ? c0 + vm::CHUNK : a.C;
  for (int c = c0; c < c1; ++c) {
    unsigned long long votes = 0;
    if (walks) {
      const vm::Candidate k = vm::candidate_at(a, words, c);
      votes = __ballot(target && vm::sees(a, words, px, py, pz, k));
    }
    if (owner) a.vis[(int64_t)c * a.words + word] = (uint32_t)(votes >> lane);
  }
}

__global__ __launch_bounds__(FLAT) void viewplan_init_kernel(const vm::GreedyArgs a) {
  const int64_t i = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (i < a.W) vm::remaining_of(a)[i] = a.targets[i];
  if (i <= a.C) vm::count_of(a)[i] = 0;
  if (i == 0) *vm::flag_of(a) = 1;
}

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                                                       // (lane 0 holds the wave's sum)
}

__global__ __launch_bounds__(FLAT) void viewplan_count_kernel(const vm::GreedyArgs a) {
  __shared__ int32_t s_sum[WAVES];
  if (*vm::flag_of(a) == 0) return;                               // (written by an earlier launch; the same for every thread)
  const int row = blockIdx.y, t = threadIdx.x;
  const uint32_t* remaining = vm::remaining_of(a);
  const int64_t w0 = (int64_t)blockIdx.x * vm::SLICE;
  int32_t mine = 0;
  for (int i = 0; i < vm::SLICE / FLAT; ++i) {
    const int64_t w = w0 + i * FLAT + t;
    if (w < a.W) mine += __popc(vm::row_word(a, row, w) & remaining[w]);
  }
  mine = wave_sum(mine);
  if ((t & 63) == 0) s_sum[t >> 6] = mine;
  __syncthreads();
  if (t == 0) {
    int32_t total = 0;
    for (int w = 0; w < WAVES; ++w) total += s_sum[w];
    if (total) atomicAdd(vm::count_of(a) + row, total);
  }
}

__global__ __launch_bounds__(PICK) void viewplan_pick_kernel(const vm::GreedyArgs a, const int round) {
  __shared__ unsigned long long s_key[PICK_WAVES];
  __shared__ int32_t s_left[PICK_WAVES];
  const int t = threadIdx.x;
  const bool chooses = round < a.k;                               // (k == 0: round 0 writes gain and status only)
  int32_t* count = vm::count_of(a);
  if (*vm::flag_of(a) == 0) {                                     // behind a -1 pick: the same for every thread
    if (t == 0 && chooses) a.picks[round] = -1, a.pick_gain[round] = 0;
    return;
  }
  unsigned long long key = 0;
  for (int i = 0; i < vm::MAX_CANDIDATES / PICK; ++i) {
    const int c = i * PICK + t;
    if (c < a.C) {
      const int32_t n = count[c];
      if (round == 0) a.gain[c] = n;
      const unsigned long long mine = vm::key_of(n, c);
      key = mine > key ? mine : key;
    }
  }
  const int32_t all = count[a.C];
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_down(key, off, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) s_key[t >> 6] = key;
  __syncthreads();                                                // (every read of the counts lies before it)
  key = s_key[0];
  for (int w = 1; w < PICK_WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;
  if (round == 0 && t == 0) a.status[0] = all, a.status[1] = all;
  if (!chooses) return;
  if (!vm::key_picks(a, key)) {                                   // nothing left to reveal: the same for every thread
    if (t == 0) a.picks[round] = -1, a.pick_gain[round] = 0, *vm::flag_of(a) = 0;
    return;
  }
  const int best = vm::key_pick(key);                             // in [0, C): key_picks
  uint32_t* remaining = vm::remaining_of(a);
  const uint32_t* row = a.vis + (int64_t)best * a.W;
  int32_t left = 0;
  for (int64_t w = t; w < a.W; w += PICK) {
    const uint32_t r = remaining[w] & ~row[w];
    remaining[w] = r;
    left += __popc(r);
  }
  for (int i = 0; i <= vm::MAX_CANDIDATES / PICK; ++i) {
    const int c = i * PICK + t;
    if (c <= a.C) count[c] = 0;
  }
  left = wave_sum(left);
  if ((t & 63) == 0) s_left[t >> 6] = left;
  __syncthreads();
  if (t == 0) {
    int32_t total = 0;
    for (int w = 0; w < PICK_WAVES; ++w) total += s_left[w];
    a.status[1] = total;
    a.picks[round] = best;
    a.pick_gain[round] = vm::key_count(key);
  }
}

}  // namespace

extern "C" int occ4d_viewplan_visible_u32(const uint32_t* solid, int nx, int ny, int nz, const uint32_t* targets,
                                          const int32_t* candidates, int C, int wx, int wy, int wz, int64_t max_dist2,
                                          uint32_t* vis, void* stream) {
  vm::VisArgs a; bool empty;
  OCC4D_TRY(vm::check_visible(solid, nx, ny, nz, targets, candidates, C, wx, wy, wz, max_dist2, vis, empty, a));
  if (empty) return OCC4D_OK;
  const dim3 grid((unsigned)(((int64_t)a.points + FLAT - 1) / FLAT), (unsigned)((C + vm::CHUNK - 1) / vm::CHUNK));   // <= 2^19, <= 512
  viewplan_vis_kernel<<<grid, FLAT, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch("occ4d_viewplan_visible_u32");
}

extern "C" int occ4d_viewplan_greedy_u32(const uint32_t* vis, int C, int64_t W, const uint32_t* targets, int k, int32_t* work,
                                         int32_t* gain, int32_t* picks, int32_t* pick_gain, int32_t* status, void* stream) {
  vm::GreedyArgs a; bool empty;
  OCC4D_TRY(vm::check_greedy(vis, C, W, targets, k, work, gain, picks, pick_gain, status, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t cells = W > C + 1 ? W : C + 1;
  viewplan_init_kernel<<<(unsigned)((cells + FLAT - 1) / FLAT), FLAT, 0, st>>>(a);
  const unsigned slices = (unsigned)((W + vm::SLICE - 1) / vm::SLICE);                    // <= 2^19
  const int rounds = k > 1 ? k : 1;
  for (int r = 0; r < rounds; ++r) {
    viewplan_count_kernel<<<dim3(slices, (unsigned)(C + (r == 0))), FLAT, 0, st>>>(a);
    viewplan_pick_kernel<<<1, PICK, 0, st>>>(a, r);
  }
  return occ4d::check_launch("occ4d_viewplan_greedy_u32");
}
