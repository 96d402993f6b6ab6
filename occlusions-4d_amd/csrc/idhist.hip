// Segmented id histogram (include/occ4d_occl.h): one pass over a column of the clip's rows, accumulated onto the caller's
// int32 counts.  The per-row decision and the argument contract are csrc/occl_math.hpp, shared with the g++ twin.
//
// Every workgroup takes a CONTIGUOUS run of 256-row tiles (so it changes segment as rarely as possible) and keeps an int32
// table of n_ids + 2 bins in LDS for the segment it is in.  Rows are added with LDS integer atomics; when all counted lanes
// of a wave hold the same bin (background runs, the all-one-id case) the wave adds its lane count once.  On leaving a
// segment, and at the end, the non-zero bins go to the global table with int32 atomics and the LDS table is cleared.
// Integers only: the result does not depend on scheduling.  The grid is a function of (n, S) alone.
//
// Memory safety does not hang on the offsets (the host cannot see them): rows are indexed by the tile walk in [0, n), the
// segment index by segment_end_index() in [0, S), and the walk over a tile always advances.
#include "common.hpp"
#include "occl_math.hpp"
#include "occ4d_occl.h"

namespace {

namespace oc = occ4d_occl;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more than GRID_CAP tiles: several tiles per workgroup

// S does not change the grid today (a workgroup walks through segment borders); it stays an argument: the grid is a
// function of (n, S) and of nothing else, never of the device
inline int grid_for(int n, int /*S*/) {
  const int tiles = occ4d::cdiv(n, THREADS);
  return tiles < GRID_CAP ? tiles : GRID_CAP;
}

__device__ __forceinline__ void flush_bins(int* s_bins, int bins, int32_t* __restrict__ dst) {
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += THREADS) {
    const int c = s_bins[k];
    if (c != 0) {
      atomicAdd(&dst[k], c);
      s_bins[k] = 0;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(THREADS) void id_histogram_kernel(const oc::HistArgs a, const int64_t* __restrict__ seg_offsets,
                                                                int S, int tiles, int tiles_per_wg,
                                                                int32_t* __restrict__ counts) {
  extern __shared__ int s_bins[];
  const int bins = a.n_ids + OCC4D_OCCL_EXTRA_BINS;
  for (int k = threadIdx.x; k < bins; k += THREADS) s_bins[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int first_tile = blockIdx.x * tiles_per_wg;
  const int last_tile = min(first_tile + tiles_per_wg, tiles);
  int cur = -1;                                                   // (workgroup-uniform) the segment the LDS table belongs to
  for (int tile = first_tile; tile < last_tile; ++tile) {
    const int64_t r0 = (int64_t)tile * THREADS;
    const int64_t r1 = r0 + THREADS < (int64_t)a.n ? r0 + THREADS : (int64_t)a.n;
    const int64_t i = r0 + threadIdx.x;
    const int bin = i < r1 ? oc::bin_of(a, i) : -1;
    for (int64_t lo = r0; lo < r1;) {                             // the tile's pieces, one per segment it touches
      const int k = oc::segment_end_index(seg_offsets, S, lo);   // uniform: every thread reads the same offsets
      const int seg = k <= S ? k - 1 : S - 1;
      int64_t hi = r1;
      if (k <= S && seg_offsets[k] < hi) hi = seg_offsets[k];     // (> lo by segment_end_index)
      if (seg != cur) {
        if (cur >= 0) flush_bins(s_bins, bins, counts + (int64_t)cur * bins);
        cur = seg;
      }
      const bool mine = bin >= 0 && i >= lo && i < hi;
      const unsigned long long active = __ballot(mine);
      if (active != 0ull) {                                       // (wave-uniform)
        const int leader = __ffsll((long long)active) - 1;
        const int leader_bin = __shfl(bin, leader, 64);
        if (__ballot(mine && bin == leader_bin) == active) {
          if (lane == leader) atomicAdd(&s_bins[leader_bin], __popcll(active));
        } else if (mine) {
          atomicAdd(&s_bins[bin], 1);
        }
      }
      lo = hi;
    }
  }
  if (cur >= 0) flush_bins(s_bins, bins, counts + (int64_t)cur * bins);
}

}  // namespace

extern "C" int occ4d_id_histogram_f32(const float* rows, int64_t ld, int n, int col, const int64_t* seg_offsets, int n_segments,
                                      int n_ids, const float* key, int pred_col, float pred_a, float pred_b, int32_t* counts,
                                      void* stream) {
  oc::HistArgs a; bool empty;
  OCC4D_TRY(oc::check_id_histogram(rows, ld, n, col, seg_offsets, n_segments, n_ids, key, pred_col, pred_a, pred_b, counts, empty, a));
  if (empty) return OCC4D_OK;
  const int tiles = occ4d::cdiv(n, THREADS);
  const int blocks = grid_for(n, n_segments);
  const int tiles_per_wg = occ4d::cdiv(tiles, blocks);
  const size_t lds = (size_t)(n_ids + OCC4D_OCCL_EXTRA_BINS) * sizeof(int);
  id_histogram_kernel<<<blocks, THREADS, lds, (hipStream_t)stream>>>(a, seg_offsets, n_segments, tiles, tiles_per_wg, counts);
  return occ4d::check_launch("occ4d_id_histogram_f32");
}
