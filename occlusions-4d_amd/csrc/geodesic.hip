// Shortest free-space paths over the grid (include/ext/occ4d_geodesic.h): a block relaxation.  The neighbour table, the relax step,
// the parent rule, the seed test, the tiling, the trace and the argument contracts are csrc/geodesic_math.hpp, shared with the g++
// twin; the LDS tile, the barriers, the atomics' spelling and the launches are here.
//
// Launches, whatever the data: 1 + rounds + 1, and 1 more with `parent`.
//   seed    one workgroup per tile of 8 x 8 x 8 points: the tile's costs start as NONE in LDS, every thread walks the seed list with
//           the workgroup's stride and puts 0 where a seed is a source IN THIS TILE, and after the barrier the tile is written.  One
//           launch without a race between "NONE everywhere" and "0 at the seeds", at the price of tiles x n_seeds reads (a seed list
//           is short).  Workgroup 0 also sets flags[0] = 1 and clears flags[1 .. rounds].  With resume = 1 only the flags are made.
//   round k (k = 1 .. rounds)  returns at once when flags[k - 1] == 0: the round before lowered nothing.  Otherwise a workgroup loads
//           its tile and a halo of one point of `cost` into LDS (NONE outside the grid), and relaxes its own points there: every
//           thread takes the minimum over its point's neighbours (read phase), a barrier, the lowered values are written (write
//           phase), and a workgroup vote -- a barrier too -- ends the loop when none was; the loop is a `for` bounded by the tile's
//           points.  It writes back what it lowered and sets flags[k].  The halo is read only: ONLY A POINT'S OWNER WRITES IT.
//           Within a launch a halo read may return the neighbour tile's value from before or after that tile's write-back: both are
//           costs of real paths, upper bounds of the true cost, and values only ever decrease.  Those words are read and written with
//           relaxed AGENT-scope atomic loads and stores (eight XCDs, eight L2s; no formal data race); nothing is ordered by them and
//           NO WORKGROUP WAITS FOR ANOTHER: no flags between workgroups, no tickets, no spinning.  A round in which no workgroup
//           lowered anything saw one consistent array and found it a fixed point.
//   status  one workgroup counts the rounds that lowered a value.
//   parent  one thread per point, from the finished cost.
// No inline assembly, no floats, no scratch.  Per-tile skipping (flags per tile and round) is not built.
#include "common.hpp"
#include "geodesic_math.hpp"
#include "ext/occ4d_geodesic.h"

namespace {

namespace gm = occ4d_geodesic;

constexpr int THREADS = gm::TILE_POINTS;   // one thread per point of a tile
constexpr int FLAT = 256;                  // the passes without a tile

__device__ __forceinline__ int32_t agent_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void agent_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(THREADS) void geodesic_seed_kernel(const gm::Args a) {
  __shared__ int32_t s_cost[THREADS];
  const int t = threadIdx.x;
  if (blockIdx.x == 0)
    for (int k = t; k <= a.rounds; k += THREADS) a.flags[k] = k == 0 ? 1 : 0;
  if (a.resume) return;
  int o[3];
  gm::tile_origin(a, blockIdx.x, o);
  s_cost[t] = gm::NONE;
  __syncthreads();
  for (int k = t; k < a.n_seeds; k += THREADS) {
    const int64_t p = gm::seed_point(a, k);
    const int u = p < 0 ? -1 : gm::tile_index(a, o, p);
    if (u >= 0) __hip_atomic_store(s_cost + u, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // (several seeds may name one point)
  }
  __syncthreads();
  const int64_t p = gm::own_point(a, o, t);
  if (p >= 0) a.cost[p] = s_cost[t];
}

__global__ __launch_bounds__(THREADS) void geodesic_round_kernel(const gm::Args a, const int k) {
  if (a.flags[k - 1] == 0) return;                                // (written by an earlier launch; the same for every thread)
  __shared__ int32_t s_cost[gm::HALO_POINTS];
  const int t = threadIdx.x;
  int o[3];
  gm::tile_origin(a, blockIdx.x, o);
  for (int h = t; h < gm::HALO_POINTS; h += THREADS) {
    const int64_t q = gm::halo_point(a, o, h);
    s_cost[h] = q < 0 ? gm::NONE : agent_load(a.cost + q);
  }
  const int64_t p = gm::own_point(a, o, t);
  const bool open = p >= 0 && gm::passable(a, p);
  const int slot = gm::own_slot(t);
  __syncthreads();
  const int32_t first = s_cost[slot];
  int32_t mine = first;
  for (int it = 0; it < gm::TILE_POINTS; ++it) {
    int32_t best = mine;
    if (open)
      best = gm::relax_point(a.rank, a.step, mine, [&](int dx, int dy, int dz) { return s_cost[slot + (dx * gm::HY + dy) * gm::HZ + dz]; });
    __syncthreads();                                              // every read of this iteration is done
    const bool lowered = best < mine;
    if (lowered) s_cost[slot] = mine = best;
    if (!__syncthreads_or(lowered)) break;                        // the writes are visible; the same answer in every thread
  }
  const bool wrote = mine < first;                                // (then open, hence p >= 0)
  if (wrote) agent_store(a.cost + p, mine);
  if (__syncthreads_or(wrote) && t == 0) agent_store(a.flags + k, 1);
}

__global__ __launch_bounds__(FLAT) void geodesic_status_kernel(const gm::Args a) {
  __shared__ int s_changed;
  if (threadIdx.x == 0) s_changed = 0;
  __syncthreads();
  int mine = 0;
  for (int k = 1 + threadIdx.x; k <= a.rounds; k += FLAT) mine += a.flags[k] != 0;
  if (mine) atomicAdd(&s_changed, mine);
  __syncthreads();
  if (threadIdx.x == 0) gm::status_item(a, s_changed);
}

__global__ __launch_bounds__(FLAT) void geodesic_parent_kernel(const gm::Args a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (p < a.points) gm::parent_item(a, p);
}

__global__ __launch_bounds__(FLAT) void geodesic_trace_kernel(const gm::TraceArgs a) {
  const int g = blockIdx.x * FLAT + threadIdx.x;
  if (g < a.n_goals) gm::trace_item(a, g);
}

}  // namespace

extern "C" int occ4d_geodesic_grid_i32(const int32_t* clear, int min_clear, int nx, int ny, int nz, const int32_t* seeds, int n_seeds,
                                       int connectivity, int step_face, int step_edge, int step_corner, int rounds, int resume,
                                       int32_t* work, int32_t* cost, int32_t* parent, int32_t* status, void* stream) {
  gm::Args a; bool empty;
  OCC4D_TRY(gm::check_geodesic(clear, min_clear, nx, ny, nz, seeds, n_seeds, connectivity, step_face, step_edge, step_corner, rounds,
                               resume, work, cost, parent, status, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)a.n_tiles;                                           // <= 64^3
  geodesic_seed_kernel<<<tiles, THREADS, 0, st>>>(a);
  for (int k = 1; k <= rounds; ++k) geodesic_round_kernel<<<tiles, THREADS, 0, st>>>(a, k);
  geodesic_status_kernel<<<1, FLAT, 0, st>>>(a);
  if (parent) geodesic_parent_kernel<<<(unsigned)((a.points + FLAT - 1) / FLAT), FLAT, 0, st>>>(a);
  return occ4d::check_launch("occ4d_geodesic_grid_i32");
}

extern "C" int occ4d_geodesic_trace_i32(const int32_t* cost, const int32_t* parent, int n, const int32_t* goals, int n_goals, int cap,
                                        int32_t* paths, int32_t* path_len, void* stream) {
  gm::TraceArgs a; bool empty;
  OCC4D_TRY(gm::check_trace(cost, parent, n, goals, n_goals, cap, paths, path_len, empty, a));
  if (empty) return OCC4D_OK;
  geodesic_trace_kernel<<<(unsigned)((n_goals + FLAT - 1) / FLAT), FLAT, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch("occ4d_geodesic_trace_i32");
}
