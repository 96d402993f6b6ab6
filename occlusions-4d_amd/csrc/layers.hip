// The labelled objects as depth layers in camera views (include/ext/occ4d_layers.h).  The OWNER of a sample, the find-or-open step,
// the march of a pixel, the rows it writes and the argument contract are csrc/layers_math.hpp, shared with the g++ twin; the tiling,
// the match across the lanes, the gather table, the atomics, the barriers and the launches are here.
//
//   fill    every word of table becomes its fill value, status [0, 0].
//   march   ONE launch.  One thread per pixel, 256-thread workgroups over tiles of 16 x 16 pixels of one view, a wave an 8 x 8
//           sub-tile (the tiling of csrc/raycast.hip: the rays of a wave stay in neighbouring cells, the label volume is 2 MB at the
//           published grid and stays in L2).  A lane keeps its L <= 8 layers in registers -- lm::Layers is only ever indexed by
//           constants, the find-or-open step is an unrolled compare-and-select -- and writes its pixel's rows itself: one owner per
//           element.  THE TABLE: per layer slot the wave matches equal labels across its lanes with a ballot loop: the first
//           unhandled lane's label is read with a readlane, so it and all control flow are wave-uniform; a ballot gives the lanes
//           that hold it, and since lane = 8 * row + column of the sub-tile, the number of pixels and the box are bit counts of that
//           mask; only the least `first` takes a reduction over the lanes.  At most 64 rounds.  The wave hands ONE contribution per
//           label to the workgroup's gather table in LDS -- SLOTS objects keyed by label, lane 0 claims a slot with a
//           compare-and-swap over at most PROBES slots -- or, when no slot is free, straight to table with global integer atomics.
//           After ONE barrier each claimed slot goes to global memory once: one atomic per word and workgroup; status gets one
//           atomic add per word and workgroup.
// Barriers stand in uniform control flow only: a thread whose pixel lies beyond the image edge is masked, it does not leave.  Every
// loop is a `for` with a bound fixed before it starts.  No workgroup waits for another one.  No inline assembly.
// Experiments only, through OCC4D_HIPCC_EXTRA: -DOCC4D_LAYERS_NO_GATHER takes the LDS table away (every wave's contribution goes to
// global memory), -DOCC4D_LAYERS_PER_LANE also the match across the lanes (every lane's layers go to global memory one by one).
#include "common.hpp"
#include "layers_math.hpp"
#include "ext/occ4d_layers.h"

namespace {

namespace lm = occ4d_layers;

constexpr int THREADS = 256;
constexpr int TILE = 16;                  // pixels per workgroup edge
constexpr int SUB = 8;                    // pixels per wave edge
static_assert(TILE * TILE == THREADS && SUB * SUB == 64 && TILE == 2 * SUB, "four 8 x 8 waves per 16 x 16 tile");
static_assert(lm::SLOTS * lm::COLS <= THREADS, "one thread per word of the gather table");

__global__ __launch_bounds__(THREADS) void layers_fill_kernel(const lm::Args a, const int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < words) a.table[i] = lm::fill_value((int)(i % lm::COLS));
  if (a.status && i < 2) a.status[i] = 0;
}

__device__ __forceinline__ bool is_max(int c) { return c == OCC4D_LAYERS_XMAX || c == OCC4D_LAYERS_YMAX; }

// word c of a table row (in LDS or in global memory) takes the value x: a sum, a maximum or a minimum
__device__ __forceinline__ void combine(int32_t* row, int c, int32_t x) {
  if (c < OCC4D_LAYERS_NEAR) {
    if (x != 0) atomicAdd(row + c, x);
  } else if (is_max(c)) {
    atomicMax(row + c, x);
  } else {
    atomicMin(row + c, x);
  }
}

// the slot of label k in the workgroup's table, claimed now or before, or -1 when the PROBES slots from k on hold other labels
__device__ __forceinline__ int claim_slot(int32_t* s_key, int32_t k, int lane) {
  int slot = -1;
#ifndef OCC4D_LAYERS_NO_GATHER
  for (int p = 0; p < lm::PROBES; ++p) {
    const int cand = (k + p) % lm::SLOTS;                         // (0 <= k < K < 2^29)
    if (slot < 0) {                                               // wave-uniform
      int32_t owner = 0;
      if (lane == 0) owner = atomicCAS(s_key + cand, -1, k);
      owner = __builtin_amdgcn_readfirstlane(owner);
      if (owner == -1 || owner == k) slot = cand;
    }
  }
#endif
  return slot;
}

// One layer slot of a wave: lab = the lane's label there (-1: none, and in every masked lane), first = its first sample, front =
// whether this is layer 0, (bx, by) = the sub-tile's first pixel.  rows = the view's K rows of table.
__device__ __forceinline__ void wave_slot(int32_t* rows, int32_t lab, int32_t first, bool front, int32_t* s_key, int32_t* s_row, int lane,
                                          int bx, int by) {
  unsigned long long todo = __ballot(lab >= 0);
  for (int r = 0; r < 64; ++r) {
    if (todo == 0) break;                                         // wave-uniform
    const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int32_t k = __builtin_amdgcn_readlane(lab, lead);       // 0 <= k < K: owner_of's test
    const unsigned long long mine = __ballot(lab == k);
    todo &= ~mine;
    int32_t near = lab == k ? first : INT32_MAX;
    for (int off = 32; off > 0; off >>= 1) near = min(near, __shfl_xor(near, off, 64));
    unsigned long long fold = mine | (mine >> 32);                // bit 8 y + x of mine: the pixel (bx + x, by + y)
    fold |= fold >> 16, fold |= fold >> 8;
    const unsigned cols = (unsigned)(fold & 0xffu);               // != 0: lane `lead` is in mine
    const int32_t amodal = __popcll(mine);
    const int32_t vals[lm::COLS] = {amodal, front ? amodal : 0, near, bx + (int)__builtin_ctz(cols), bx + 31 - (int)__builtin_clz(cols),
                                    by + ((int)__builtin_ctzll(mine) >> 3), by + ((63 - (int)__builtin_clzll(mine)) >> 3)};
    const int slot = claim_slot(s_key, k, lane);
    if (lane == 0) {
      int32_t* row = slot >= 0 ? s_row + slot * lm::COLS : rows + (int64_t)k * lm::COLS;
#pragma unroll
      for (int c = 0; c < lm::COLS; ++c) combine(row, c, vals[c]);
    }
  }
}

__global__ __launch_bounds__(THREADS) void layers_march_kernel(const lm::Args a, const int tiles_x, const int tiles_y) {
  __shared__ int32_t s_key[lm::SLOTS], s_row[lm::SLOTS * lm::COLS], s_status[2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (t < lm::SLOTS) s_key[t] = -1;
  if (t < lm::SLOTS * lm::COLS) s_row[t] = lm::fill_value(t % lm::COLS);
  if (t < 2) s_status[t] = 0;
  __syncthreads();

  const int tile = blockIdx.x % (tiles_x * tiles_y), v = blockIdx.x / (tiles_x * tiles_y);
  const int bx = (tile % tiles_x) * TILE + (wave & 1) * SUB, by = (tile / tiles_x) * TILE + (wave >> 1) * SUB;
  const int px = bx + (lane & (SUB - 1)), py = by + (lane / SUB);
  lm::Layers s;
  lm::reset(s);                                                   // (a masked lane keeps this: no label, count 0)
  if (px < a.ray.W && py < a.ray.H) {
    lm::march(a, v, px, py, s);
    lm::write_pixel(a, ((int64_t)v * a.ray.H + py) * a.ray.W + px, s);
  }
  if (a.status) {                                                 // (uniform)
    const int over = __popcll(__ballot(s.count == a.L + 1)), some = __popcll(__ballot(s.count >= 1));
    if (lane == 0 && over) atomicAdd(s_status, over);
    if (lane == 0 && some) atomicAdd(s_status + 1, some);
  }
  int32_t* rows = a.table ? a.table + (int64_t)v * a.K * lm::COLS : nullptr;
  if (a.table) {                                                  // (uniform)
#ifdef OCC4D_LAYERS_PER_LANE
#pragma unroll
    for (int j = 0; j < lm::MAX_LAYERS; ++j)
      if (j < a.L && s.label[j] >= 0) {
        const int32_t vals[lm::COLS] = {1, j == 0 ? 1 : 0, s.first[j], px, px, py, py};
#pragma unroll
        for (int c = 0; c < lm::COLS; ++c) combine(rows + (int64_t)s.label[j] * lm::COLS, c, vals[c]);
      }
#else
#pragma unroll
    for (int j = 0; j < lm::MAX_LAYERS; ++j)
      if (j < a.L) wave_slot(rows, s.label[j], s.first[j], j == 0, s_key, s_row, lane, bx, by);      // (uniform)
#endif
  }
  __syncthreads();

  if (a.table && t < lm::SLOTS * lm::COLS) {                      // each claimed slot once: one atomic per word
    const int32_t k = s_key[t / lm::COLS];                        // -1, or a label that passed owner_of's test
    if (k >= 0) combine(rows + (int64_t)k * lm::COLS, t % lm::COLS, s_row[t]);
  }
  if (a.status && t < 2 && s_status[t] != 0) atomicAdd(a.status + t, s_status[t]);
}

}  // namespace

extern "C" int occ4d_layers_march_i32(const int32_t* labels, int nx, int ny, int nz, int K, float x0, float sx, float y0, float sy,
                                      float z0, float sz, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth,
                                      float step, int n_steps, int L, int32_t* label, int32_t* first, int32_t* samples, int32_t* point,
                                      int32_t* count, int32_t* table, int32_t* status, void* stream) {
  lm::Args a; bool empty;
  OCC4D_TRY(lm::check_layers(labels, nx, ny, nz, K, x0, sx, y0, sy, z0, sz, k_inv, rt_inv, V, H, W, near_depth, step, n_steps, L, label,
                             first, samples, point, count, table, status, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t words = a.table ? (int64_t)V * K * lm::COLS : 0;  // < 2^31
  if (a.table || a.status) layers_fill_kernel<<<(unsigned)(((words > 2 ? words : 2) + THREADS - 1) / THREADS), THREADS, 0, st>>>(a, words);
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;      // V tiles_x tiles_y <= V H W < 2^31
  layers_march_kernel<<<(unsigned)((int64_t)V * tiles_x * tiles_y), THREADS, 0, st>>>(a, tiles_x, tiles_y);
  return occ4d::check_launch("occ4d_layers_march_i32");
}
