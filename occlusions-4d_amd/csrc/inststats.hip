// Instance statistics (include/occ4d_inst.h): two grid-stride row passes onto the caller's int64 frame table and a
// one-workgroup fold of that table onto the running counts and sums.  The per-row decisions, the per-id arithmetic and the
// argument contracts are csrc/inst_math.hpp, shared with the g++ twin.
//
// Row passes: integers only.  Every workgroup keeps its part of the table in LDS (int32 counts: a workgroup sees at most
// n / gridDim + 256 < 2^31 rows; 64-bit coordinate sums: 2^31 rows of magnitude 2^30 stay below 2^63), rows are added with LDS
// integer atomics, and when all counted lanes of a wave fall in one cell (NONE x NONE is most of a grid; a run of one
// instance) the wave adds once.  At the end the NON-ZERO entries go to the frame table with 64-bit integer atomics: order-free,
// so the table does not depend on scheduling.  The grid is a function of the row count alone.
// Fold: the per-id terms in parallel, then one thread per group adds them over the ids ascending and adds the frame's total
// onto the running value once.  No floating atomics anywhere.
//
// Memory safety: rows are indexed by the loop in [0, n); the one data-indexed read, target_id[nn_idx], comes after the range
// check; an LDS cell index is built from validated classes only (inst_math.hpp).
#include "common.hpp"
#include "inst_math.hpp"
#include "occ4d_inst.h"

namespace {

namespace in = occ4d_inst;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more rows than GRID_CAP * THREADS: further trips of the loop
constexpr int MAX_IDS = OCC4D_INST_MAX_IDS;
constexpr int FOLD_THREADS = 64;          // one wave: a thread per id, then a thread per group

inline int grid_for(int n) { return n <= 0 ? 0 : (occ4d::cdiv(n, THREADS) < GRID_CAP ? occ4d::cdiv(n, THREADS) : GRID_CAP); }

__device__ __forceinline__ void add_i64(int64_t* dst, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);      // (two's complement: a negative sum adds too)
}

__global__ __launch_bounds__(THREADS) void confusion_kernel(const in::ConfusionArgs a, int64_t* __restrict__ frame) {
  extern __shared__ int s_cells[];                                  // (n_ids + 1)^2 cells, then the bad rows
  const int cells = (a.n_ids + 1) * (a.n_ids + 1);
  for (int k = threadIdx.x; k <= cells; k += THREADS) s_cells[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // `base` is uniform over the workgroup: every lane of a wave makes the same trips, so the ballots below are whole
  for (int64_t base = (int64_t)blockIdx.x * THREADS; base < a.n; base += (int64_t)gridDim.x * THREADS) {
    const int64_t i = base + threadIdx.x;
    const bool mine = i < a.n;
    int cell = 0;
    if (mine) {
      cell = in::confusion_cell(a, i);
      if (cell == in::ROW_BAD) cell = cells;
    }
    const unsigned long long active = __ballot(mine);
    if (active == 0ull) continue;                                   // (wave-uniform)
    const int leader = __ffsll((long long)active) - 1;
    const int leader_cell = __shfl(cell, leader, 64);
    if (__ballot(mine && cell == leader_cell) == active) {
      if (lane == leader) atomicAdd(&s_cells[leader_cell], __popcll(active));
    } else if (mine) {
      atomicAdd(&s_cells[cell], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= cells; k += THREADS) {
    const int c = s_cells[k];
    if (c == 0) continue;
    add_i64(k == cells ? frame + OCC4D_INST_BAD_ROWS : frame + in::frame_confusion(a.n_ids) + k, (int64_t)c);
  }
}

// sum over the 64 lanes of a wave, valid in lane 0
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

__global__ __launch_bounds__(THREADS) void points_kernel(const in::PointArgs a, int64_t* __restrict__ table,
                                                          int64_t* __restrict__ bad_rows) {
  __shared__ int s_count[MAX_IDS + 1];                              // per id, then the bad rows
  __shared__ unsigned long long s_sum[MAX_IDS * 3];
  for (int k = threadIdx.x; k <= MAX_IDS; k += THREADS) s_count[k] = 0;
  for (int k = threadIdx.x; k < MAX_IDS * 3; k += THREADS) s_sum[k] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * THREADS; base < a.n; base += (int64_t)gridDim.x * THREADS) {
    const int64_t i = base + threadIdx.x;
    int64_t q[3] = {0, 0, 0};
    int id = in::ROW_SKIP;
    if (i < a.n) {
      id = in::point_row(a, i, q);
      if (id == in::ROW_BAD) id = MAX_IDS;
    }
    const bool mine = id >= 0;                                      // an id's row, or a bad row (q = 0)
    const unsigned long long active = __ballot(mine);
    if (active == 0ull) continue;                                   // (wave-uniform)
    const int leader = __ffsll((long long)active) - 1;
    const int leader_id = __shfl(id, leader, 64);
    if (__ballot(mine && id == leader_id) == active) {              // one entry for the whole wave: add the lanes first
      const long long sx = wave_sum(mine ? q[0] : 0), sy = wave_sum(mine ? q[1] : 0), sz = wave_sum(mine ? q[2] : 0);
      if (lane == 0) {
        atomicAdd(&s_count[leader_id], __popcll(active));
        if (leader_id < MAX_IDS) {
          atomicAdd(&s_sum[leader_id * 3 + 0], (unsigned long long)sx);
          atomicAdd(&s_sum[leader_id * 3 + 1], (unsigned long long)sy);
          atomicAdd(&s_sum[leader_id * 3 + 2], (unsigned long long)sz);
        }
      }
    } else if (mine) {
      atomicAdd(&s_count[id], 1);
      if (id < MAX_IDS) {
        atomicAdd(&s_sum[id * 3 + 0], (unsigned long long)q[0]);
        atomicAdd(&s_sum[id * 3 + 1], (unsigned long long)q[1]);
        atomicAdd(&s_sum[id * 3 + 2], (unsigned long long)q[2]);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= MAX_IDS; k += THREADS) {
    const int c = s_count[k];
    if (c == 0) continue;
    if (k == MAX_IDS) {
      add_i64(bad_rows, (int64_t)c);
    } else if (k < a.n_ids) {                                       // (always: point_row gives ids below n_ids)
      int64_t* e = table + (int64_t)k * OCC4D_INST_POINT_WORDS;
      add_i64(e + OCC4D_INST_POINT_COUNT, (int64_t)c);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const unsigned long long s = s_sum[k * 3 + d];
        if (s != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(e + OCC4D_INST_POINT_SX + d), s);
      }
    }
  }
}

__global__ __launch_bounds__(FOLD_THREADS) void fold_kernel(const int64_t* __restrict__ frame, int n_ids,
                                                             const int32_t* __restrict__ inst_group, int n_groups,
                                                             int64_t* __restrict__ counts, double* __restrict__ sums) {
  __shared__ in::IdTerms s_terms[MAX_IDS];
  const int t = threadIdx.x;
  if (t < n_ids) s_terms[t] = in::fold_id(frame, n_ids, inst_group, n_groups, t);
  __syncthreads();
  if (t < n_groups) {                                               // this frame's totals of group t, ids ascending, added once
    int64_t c[OCC4D_INST_GROUP_COUNTS];
    double s[OCC4D_INST_GROUP_SUMS];
    in::fold_group(s_terms, n_ids, t, c, s);
    for (int k = 0; k < OCC4D_INST_GROUP_COUNTS; ++k) counts[OCC4D_INST_HEAD + t * OCC4D_INST_GROUP_COUNTS + k] += c[k];
    for (int k = 0; k < OCC4D_INST_GROUP_SUMS; ++k) sums[t * OCC4D_INST_GROUP_SUMS + k] += s[k];
  }
  if (t == FOLD_THREADS - 1) {                                      // the one writer of BAD_ROWS
    int64_t bad = frame[OCC4D_INST_BAD_ROWS];
    for (int i = 0; i < n_ids; ++i) bad += s_terms[i].group == -2;
    counts[OCC4D_INST_BAD_ROWS] += bad;
  }
}

}  // namespace

extern "C" int64_t occ4d_inst_frame_len(int n_ids) { return in::frame_len(n_ids); }
extern "C" int64_t occ4d_inst_counts_len(int n_groups) { return in::counts_len(n_groups); }
extern "C" int64_t occ4d_inst_sums_len(int n_groups) { return in::sums_len(n_groups); }

extern "C" int occ4d_inst_confusion_f32(const float* density, int64_t ld_density, const float* pred_id, int64_t ld_pred, int n,
                                        const int32_t* nn_idx, const float* nn_dist, const float* target_id, int64_t ld_target, int m,
                                        int n_ids, float density_threshold, float radius, int64_t* frame, void* stream) {
  in::ConfusionArgs a; bool empty;
  OCC4D_TRY(in::check_confusion(density, ld_density, pred_id, ld_pred, n, nn_idx, nn_dist, target_id, ld_target, m, n_ids,
                                density_threshold, radius, frame, empty, a));
  if (empty) return OCC4D_OK;
  const size_t lds = (size_t)((n_ids + 1) * (n_ids + 1) + 1) * sizeof(int);
  confusion_kernel<<<grid_for(n), THREADS, lds, (hipStream_t)stream>>>(a, frame);
  return occ4d::check_launch("occ4d_inst_confusion_f32");
}

extern "C" int occ4d_inst_points_f32(const float* rows, int64_t ld, int n, const float* id, int64_t ld_id, int n_ids, int side,
                                     int64_t* frame, void* stream) {
  in::PointArgs a; bool empty;
  OCC4D_TRY(in::check_points(rows, ld, n, id, ld_id, n_ids, side, frame, empty, a));
  if (empty) return OCC4D_OK;
  points_kernel<<<grid_for(n), THREADS, 0, (hipStream_t)stream>>>(a, frame + in::frame_points(n_ids, side), frame + OCC4D_INST_BAD_ROWS);
  return occ4d::check_launch("occ4d_inst_points_f32");
}

extern "C" int occ4d_inst_fold(const int64_t* frame, int n_ids, const int32_t* inst_group, int n_groups, int64_t* counts, double* sums,
                               void* stream) {
  OCC4D_TRY(in::check_fold(frame, n_ids, n_groups, counts, sums));
  fold_kernel<<<1, FOLD_THREADS, 0, (hipStream_t)stream>>>(frame, n_ids, inst_group, n_groups, counts, sums);
  return occ4d::check_launch("occ4d_inst_fold");
}
