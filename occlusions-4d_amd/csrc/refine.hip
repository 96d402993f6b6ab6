// Coarse-to-fine decode of the query grid (include/occ4d_refine.h): the MARK (blocks -> active, points -> key) and the
// EXPANSION of the decoded rows to the dense (N, G) array.  The per-element rules and the argument contracts are
// csrc/refine_math.hpp, shared with the g++ twin; the loops, the tile ranks and the launches are here.  Memory- and
// launch-bound: a few bytes per grid point beside a decode of 29 MFLOP per query.
//
// 256-thread workgroups (four wave64), the grid capped as a function of the sizes alone, grid-stride loops.  The expansion
// walks 256-row tiles -- the compaction's tiles -- with a trip count that is uniform over the workgroup: a selected row's
// position among the decoded rows is block_offsets[tile] + its rank in the tile (wave ballot, popcount, an LDS prefix over the
// four waves: the construction of split_write_kernel in csrc/postops.hip), every thread leaves its row's source in LDS, and the
// workgroup then copies the tile's rows * g elements with consecutive threads on consecutive elements of `out`.  No atomics,
// no index array, no scatter.
#include "common.hpp"
#include "refine_math.hpp"
#include "occ4d_refine.h"

namespace {

namespace rf = occ4d_refine;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more items than GRID_CAP * THREADS: further trips of the loop
static_assert(THREADS == rf::TILE, "one thread per row of a compaction tile");

inline int grid_for(int64_t items) {
  const int64_t blocks = (items + THREADS - 1) / THREADS;
  return (int)(blocks < GRID_CAP ? blocks : GRID_CAP);
}

__global__ __launch_bounds__(THREADS) void mark_blocks_kernel(const rf::MarkArgs a) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t blk = (int64_t)blockIdx.x * THREADS + threadIdx.x; blk < a.grid.blocks; blk += step)
    a.active[blk] = rf::active_of(a, blk);
}

__global__ __launch_bounds__(THREADS) void mark_points_kernel(const rf::MarkArgs a) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < a.grid.n; i += step) a.key[i] = rf::key_of(a, i);
}

__global__ __launch_bounds__(THREADS) void expand_kernel(const rf::ExpandArgs e) {
  __shared__ int s_cnt[THREADS / 64];
  __shared__ const float* s_src[THREADS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < e.tiles; tile += gridDim.x) {      // (uniform over the workgroup: barriers inside)
    const int64_t first = tile * THREADS;
    const int64_t i = first + threadIdx.x;
    const bool live = i < e.grid.n;
    const bool selected = live && rf::kept(e.key[i]);
    const unsigned long long m = __ballot(selected);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_cnt[w];
    const int64_t pos = (int64_t)e.block_offsets[tile] + before + __popcll(m & ((1ull << lane) - 1ull));
    s_src[threadIdx.x] = live ? rf::source_row(e, i, selected, pos) : nullptr;
    __syncthreads();
    const int64_t left = e.grid.n - first;
    const int total = (int)(left < THREADS ? left : THREADS) * e.g;
    float* dst = e.out + first * e.ld_out;
    for (int t = threadIdx.x; t < total; t += THREADS) {
      const int r = t / e.g, c = t - r * e.g;
      dst[(int64_t)r * e.ld_out + c] = s_src[r][c];
    }
    __syncthreads();                                                        // (the next trip rewrites s_cnt / s_src)
  }
}

}  // namespace

extern "C" int occ4d_refine_mark_f32(const float* rep_density, int64_t ld_rep, int nx, int ny, int nz, int b, int dilate, int op,
                                     float low, int32_t* active, float* key, void* stream) {
  rf::MarkArgs a; bool empty;
  OCC4D_TRY(rf::check_mark(rep_density, ld_rep, nx, ny, nz, b, dilate, op, low, active, key, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  mark_blocks_kernel<<<grid_for(a.grid.blocks), THREADS, 0, st>>>(a);
  mark_points_kernel<<<grid_for(a.grid.n), THREADS, 0, st>>>(a);
  return occ4d::check_launch("occ4d_refine_mark_f32");
}

extern "C" int occ4d_refine_expand_f32(const float* key, const int32_t* block_offsets, const float* rep_out, int64_t ld_rep,
                                       const float* fine_out, int64_t ld_fine, int n_fine, int nx, int ny, int nz, int b, int g,
                                       float* out, int64_t ld_out, void* stream) {
  rf::ExpandArgs e; bool empty;
  OCC4D_TRY(rf::check_expand(key, block_offsets, rep_out, ld_rep, fine_out, ld_fine, n_fine, nx, ny, nz, b, g, out, ld_out, empty, e));
  if (empty) return OCC4D_OK;
  const int grid = (int)(e.tiles < GRID_CAP ? e.tiles : GRID_CAP);
  expand_kernel<<<grid, THREADS, 0, (hipStream_t)stream>>>(e);
  return occ4d::check_launch("occ4d_refine_expand_f32");
}
