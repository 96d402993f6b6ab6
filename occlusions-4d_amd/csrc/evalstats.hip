// Evaluation statistics (include/occ4d_eval.h): one grid-stride pass over the decoded queries / the target points of a
// frame, accumulated onto the caller's int64 counts and double sums.  The per-row decisions and the argument contracts are
// csrc/eval_math.hpp, shared with the g++ twin.
//
// Counts: int32 in LDS per workgroup (a workgroup sees at most n / gridDim + 256 < 2^31 rows), the non-zero ones added to
// the int64 totals with integer atomics -- order-free.
// Sums: NO floating atomics.  Every thread keeps one double accumulator per (group, sum), selected by predication (a row
// adds +0.0 to the groups it is not in, which changes nothing); lanes are added by a shuffle tree, the four waves and
// then the workgroups' partials (in the workspace) in index order by a second one-workgroup launch, which adds the call's
// total onto the running value.  The grid is a function of the row count alone (never of the device's CU count), so a
// call's bits do not depend on where it runs.
#include "common.hpp"
#include "eval_math.hpp"
#include "occ4d_eval.h"

namespace {

namespace ev = occ4d_eval;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more rows than GRID_CAP * THREADS: further trips of the loop
constexpr int NG = OCC4D_EVAL_MAX_GROUPS;
constexpr int QUERY_SUMS = 3;             // per group: accuracy d, d^2, colour L1
constexpr int TARGET_SUMS = 2;            // per group: completeness d, d^2
constexpr int MAX_SUMS = NG * QUERY_SUMS;
constexpr int FINISH_LANES = 8;           // partial chains per sum in the second launch

inline int grid_for(int n) { return n <= 0 ? 0 : (occ4d::cdiv(n, THREADS) < GRID_CAP ? occ4d::cdiv(n, THREADS) : GRID_CAP); }

// acc[v] of the 256 threads -> partial[v], v < V, in a fixed order: shuffle tree over the 64 lanes, then waves 0 .. 3
template <int V>
__device__ __forceinline__ void block_sums(const double (&acc)[V], double* __restrict__ partial) {
  __shared__ double s_wave[THREADS / 64][V];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    double x = acc[v];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) s_wave[wave][v] = x;
  }
  __syncthreads();
  if ((int)threadIdx.x < V) {
    double x = s_wave[0][threadIdx.x];
    for (int w = 1; w < THREADS / 64; ++w) x += s_wave[w][threadIdx.x];
    partial[threadIdx.x] = x;
  }
}

// the workgroup's LDS counts -> the int64 totals; word `words - 1` of the LDS block is BAD_ROWS
__device__ __forceinline__ void flush_counts(const int* s_counts, int words, int64_t* __restrict__ counts) {
  for (int k = threadIdx.x; k < words; k += THREADS) {
    const int c = s_counts[k];
    if (c == 0) continue;
    int64_t* dst = (k == words - 1) ? counts + OCC4D_EVAL_BAD_ROWS : counts + OCC4D_EVAL_HEAD + k;
    atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)c);
  }
}

__global__ __launch_bounds__(THREADS) void query_stats_kernel(const ev::QueryArgs a, int64_t* __restrict__ counts,
                                                               double* __restrict__ partial) {
  extern __shared__ int s_counts[];
  const int stride = (int)ev::group_stride(a.n_classes);
  const int words = a.n_groups * stride + 1;
  for (int k = threadIdx.x; k < words; k += THREADS) s_counts[k] = 0;
  __syncthreads();
  double acc[NG * QUERY_SUMS];
#pragma unroll
  for (int v = 0; v < NG * QUERY_SUMS; ++v) acc[v] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * THREADS) {
    const ev::QueryRow r = ev::classify_query(a, (int)i);
    if (r.group < 0) {
      atomicAdd(&s_counts[words - 1], 1);
      continue;
    }
    int* c = s_counts + r.group * stride;
    atomicAdd(&c[r.occ], 1);
    if (r.solid) atomicAdd(&c[OCC4D_EVAL_N_ACCURACY], 1);
    if (r.color) atomicAdd(&c[OCC4D_EVAL_N_COLOR], 1);
    if (r.track >= 0) atomicAdd(&c[r.track], 1);
    if (r.seg >= 0) {
      atomicAdd(&c[OCC4D_EVAL_GROUP_COUNTS + r.seg], 1);
      atomicAdd(&c[OCC4D_EVAL_N_SEG], 1);
    } else if (r.seg == -2) {
      atomicAdd(&c[OCC4D_EVAL_SEG_IGNORED], 1);
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool here = g == r.group;
      acc[g * QUERY_SUMS + 0] += here ? r.d : 0.0;
      acc[g * QUERY_SUMS + 1] += here ? r.d2 : 0.0;
      acc[g * QUERY_SUMS + 2] += here ? r.l1 : 0.0;
    }
  }
  block_sums(acc, partial + (int64_t)blockIdx.x * (NG * QUERY_SUMS));
  __syncthreads();
  flush_counts(s_counts, words, counts);
}

__global__ __launch_bounds__(THREADS) void target_stats_kernel(const float* __restrict__ dist, int m,
                                                                const int32_t* __restrict__ group, int n_groups, int n_classes,
                                                                int64_t* __restrict__ counts, double* __restrict__ partial) {
  extern __shared__ int s_counts[];
  const int stride = (int)ev::group_stride(n_classes);
  const int words = n_groups * stride + 1;
  for (int k = threadIdx.x; k < words; k += THREADS) s_counts[k] = 0;
  __syncthreads();
  double acc[NG * TARGET_SUMS];
#pragma unroll
  for (int v = 0; v < NG * TARGET_SUMS; ++v) acc[v] = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < m; j += (int64_t)gridDim.x * THREADS) {
    const int grp = ev::group_of(group, (int)j, m, n_groups);
    if (grp < 0) {
      atomicAdd(&s_counts[words - 1], 1);
      continue;
    }
    atomicAdd(&s_counts[grp * stride + OCC4D_EVAL_N_COMPLETENESS], 1);
    const double d = (double)dist[j];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool here = g == grp;
      acc[g * TARGET_SUMS + 0] += here ? d : 0.0;
      acc[g * TARGET_SUMS + 1] += here ? d * d : 0.0;
    }
  }
  block_sums(acc, partial + (int64_t)blockIdx.x * (NG * TARGET_SUMS));
  __syncthreads();
  flush_counts(s_counts, words, counts);
}

// partial (blocks, NG * per_group) -> sums[g * GROUP_SUMS + first + k] += total, g < n_groups, k < per_group (the colour
// sum, k = 2 of a query pass, sits at SUM_COLOR_L1).  One workgroup: FINISH_LANES chains per sum, each over the
// workgroups b = lane, lane + 8, ... ascending, then the chains ascending.
__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ partial, int blocks, int per_group, int n_groups,
                                                          int first, double* __restrict__ sums) {
  __shared__ double s_chain[MAX_SUMS][FINISH_LANES];
  const int V = NG * per_group;
  const int v = threadIdx.x / FINISH_LANES, lane = threadIdx.x % FINISH_LANES;
  if (v < V) {
    double x = 0.0;
    for (int b = lane; b < blocks; b += FINISH_LANES) x += partial[(int64_t)b * V + v];
    s_chain[v][lane] = x;
  }
  __syncthreads();
  if ((int)threadIdx.x < V) {
    const int g = threadIdx.x / per_group, k = threadIdx.x % per_group;
    if (g < n_groups) {
      double x = s_chain[threadIdx.x][0];
      for (int l = 1; l < FINISH_LANES; ++l) x += s_chain[threadIdx.x][l];
      const int slot = (k == 2) ? OCC4D_EVAL_SUM_COLOR_L1 : first + k;
      sums[g * OCC4D_EVAL_GROUP_SUMS + slot] += x;
    }
  }
}

}  // namespace

extern "C" int64_t occ4d_eval_counts_len(int n_groups, int n_classes) { return ev::counts_len(n_groups, n_classes); }

extern "C" int64_t occ4d_eval_sums_len(int n_groups) { return ev::sums_len(n_groups); }

extern "C" int64_t occ4d_eval_workspace_bytes(int n) {
  if (n < 0) return -1;
  const int blocks = grid_for(n);
  return (int64_t)(blocks > 0 ? blocks : 1) * MAX_SUMS * (int64_t)sizeof(double);
}

extern "C" int occ4d_eval_query_stats_f32(const float* out, int64_t ldo, int n, int g_out, const int32_t* nn_idx, const float* nn_dist,
                                          const float* target, int64_t ldt, int m, int dt, int col_rgb, int col_track, int col_sem,
                                          int out_track, const int32_t* target_group, int n_groups, int n_classes,
                                          float density_threshold, float radius, int flags, int64_t* counts, double* sums,
                                          void* workspace, void* stream) {
  ev::QueryArgs a; bool empty;
  OCC4D_TRY(ev::check_query_stats(out, ldo, n, g_out, nn_idx, nn_dist, target, ldt, m, dt, col_rgb, col_track, col_sem, out_track,
                                  target_group, n_groups, n_classes, density_threshold, radius, flags, counts, sums, workspace,
                                  empty, a));
  if (empty) return OCC4D_OK;
  const int blocks = grid_for(n);
  const size_t lds = (size_t)(n_groups * ev::group_stride(n_classes) + 1) * sizeof(int);
  double* partial = static_cast<double*>(workspace);
  query_stats_kernel<<<blocks, THREADS, lds, (hipStream_t)stream>>>(a, counts, partial);
  finish_kernel<<<1, THREADS, 0, (hipStream_t)stream>>>(partial, blocks, QUERY_SUMS, n_groups, OCC4D_EVAL_SUM_ACCURACY_D, sums);
  return occ4d::check_launch("occ4d_eval_query_stats_f32");
}

extern "C" int occ4d_eval_target_stats_f32(const float* dist, int m, const int32_t* target_group, int n_groups, int n_classes,
                                           int64_t* counts, double* sums, void* workspace, void* stream) {
  bool empty;
  OCC4D_TRY(ev::check_target_stats(dist, m, n_groups, n_classes, counts, sums, workspace, empty));
  if (empty) return OCC4D_OK;
  const int blocks = grid_for(m);
  const size_t lds = (size_t)(n_groups * ev::group_stride(n_classes) + 1) * sizeof(int);
  double* partial = static_cast<double*>(workspace);
  target_stats_kernel<<<blocks, THREADS, lds, (hipStream_t)stream>>>(dist, m, target_group, n_groups, n_classes, counts, partial);
  finish_kernel<<<1, THREADS, 0, (hipStream_t)stream>>>(partial, blocks, TARGET_SUMS, n_groups, OCC4D_EVAL_SUM_COMPLETENESS_D, sums);
  return occ4d::check_launch("occ4d_eval_target_stats_f32");
}
