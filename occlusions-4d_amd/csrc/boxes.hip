// Oriented boxes of the labelled objects (include/ext/occ4d_boxes.h).  The DEAD test, the projections, the EMPTY rows, the keys of
// CHOICE, the row a choice writes and the argument contracts are csrc/boxes_math.hpp, shared with the g++ twin; the walk over the
// columns, the gather table, the atomics, the barriers and the launches are here.
//
//   fill    every word of extent and zr becomes its EMPTY value.
//   reduce  ONE launch.  A workgroup of 256 owns a tile of TILE x TILE columns (ix, iy), a wave CPW consecutive ones of them.  THE
//           DIRECTIONS LIE ACROSS THE LANES: lane l holds rows l, l + 64, l + 128, l + 192 of the table, DEAD-tested once, and per
//           column their u and v: u and v do not depend on iz, so a column costs 4 multiplications per lane and direction, not per
//           point.  The wave loads 64 labels of the column with one vector load, turns every value that names no object into -1,
//           marks the heads of the runs of equal labels with a ballot and steps through the RUNS, not the points: a run's label is
//           read with a readlane, so it and all control flow are wave-uniform, and a run gives [first iz, last iz, length] from two
//           bit positions.  Runs of -1 are skipped without ending the object in hand, so air between two parts of one object costs
//           nothing.  The running minima and maxima of the object in hand stay in registers; when another object begins they go
//           to the workgroup's gather table in LDS -- SLOTS objects keyed by label, lane 0 claims a slot with a compare-and-swap
//           over at most PROBES slots, the lanes then use LDS atomic minima / maxima at addresses of their own (layout [slot][word]
//           [a]: consecutive lanes, consecutive banks) -- or, when no slot is free, straight to extent / zr with global integer
//           atomics.  After ONE barrier each claimed slot goes to global memory once: one atomic per destination and workgroup.
//   choose  a wave per object, the lanes over the directions (a = lane, lane + 64, ...), the least (area, a) key by xor shuffles,
//           lane 0 writes the row.
// Barriers stand in uniform control flow only: the two of the reduce kernel are reached by every thread, whatever its columns hold.
// Every loop is a `for` with a bound fixed before it starts.  No workgroup waits for another one.  No inline assembly, no floats.
// -DOCC4D_BOXES_NO_GATHER (experiments only, through OCC4D_HIPCC_EXTRA) takes the table away: every hand-over goes to global memory.
#include "common.hpp"
#include "boxes_math.hpp"
#include "ext/occ4d_boxes.h"

namespace {

namespace bm = occ4d_boxes;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PER_LANE = bm::MAX_DIRS / 64;                       // directions a lane holds
constexpr int CPW = bm::TILE * bm::TILE / WAVES;                  // columns per wave
static_assert(bm::MAX_DIRS % 64 == 0 && bm::TILE * bm::TILE % WAVES == 0, "whole lanes, whole waves");

__global__ __launch_bounds__(THREADS) void boxes_fill_kernel(const bm::ExtentArgs a) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t words = (int64_t)a.K * a.A * 4;
  if (i < words) a.extent[i] = bm::empty_extent((int)(i & 3));
  else if (i < words + (int64_t)a.K * 3) a.zr[i - words] = bm::empty_zr((int)((i - words) % 3));
}

// the object in hand of one wave: the label and the z range and count (wave-uniform), the extents of the lane's directions
struct Hand {
  int32_t label, zmin, zmax, count;
  int32_t e[PER_LANE][4];
};

__device__ __forceinline__ void hand_reset(Hand& h, int32_t label) {
  h.label = label, h.zmin = INT32_MAX, h.zmax = INT32_MIN, h.count = 0;
#pragma unroll
  for (int j = 0; j < PER_LANE; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) h.e[j][c] = bm::empty_extent(c);
}

// the slot of label k in the workgroup's table, claimed now or before, or -1 when the PROBES slots from k on hold other labels
__device__ __forceinline__ int claim_slot(int32_t* s_key, int32_t k, int lane) {
  int slot = -1;
#ifndef OCC4D_BOXES_NO_GATHER
  for (int p = 0; p < bm::PROBES; ++p) {
    const int cand = (k + p) % bm::SLOTS;                         // (k >= 0, k + p < 2^30)
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

// hands the object over: to its slot of the gather table, or to global memory.  live[j]: the lane's direction j exists and is
// not DEAD; the others keep their EMPTY rows.
__device__ __forceinline__ void hand_over(const bm::ExtentArgs& a, const Hand& h, const bool* live, int32_t* s_key, int32_t* s_ext,
                                          int32_t* s_zr, int lane) {
  const int slot = claim_slot(s_key, h.label, lane);
  if (slot >= 0) {
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j)
      if (live[j]) {
        int32_t* row = s_ext + (int64_t)slot * 4 * a.A + lane + 64 * j;
        atomicMin(row, h.e[j][0]), atomicMax(row + a.A, h.e[j][1]), atomicMin(row + 2 * a.A, h.e[j][2]), atomicMax(row + 3 * a.A, h.e[j][3]);
      }
    if (lane == 0) atomicMin(s_zr + 3 * slot, h.zmin), atomicMax(s_zr + 3 * slot + 1, h.zmax), atomicAdd(s_zr + 3 * slot + 2, h.count);
    return;
  }
#pragma unroll
  for (int j = 0; j < PER_LANE; ++j)
    if (live[j]) {
      int32_t* row = a.extent + ((int64_t)h.label * a.A + lane + 64 * j) * 4;        // (0 <= label < K: the run's test)
      atomicMin(row, h.e[j][0]), atomicMax(row + 1, h.e[j][1]), atomicMin(row + 2, h.e[j][2]), atomicMax(row + 3, h.e[j][3]);
    }
  if (lane == 0) {
    int32_t* z = a.zr + (int64_t)h.label * 3;
    atomicMin(z, h.zmin), atomicMax(z + 1, h.zmax), atomicAdd(z + 2, h.count);
  }
}

__global__ __launch_bounds__(THREADS) void boxes_reduce_kernel(const bm::ExtentArgs a, const int tiles_y) {
  extern __shared__ int32_t s_ext[];                              // [SLOTS][4][A]
  __shared__ int32_t s_key[bm::SLOTS], s_zr[bm::SLOTS * 3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int A = a.A, K = a.K, nx = a.n[0], ny = a.n[1], nz = a.n[2];
  for (int i = t; i < bm::SLOTS * 4 * A; i += THREADS) s_ext[i] = bm::empty_extent(i / A);       // (word c = (i / A) % 4: its parity)
  if (t < bm::SLOTS) s_key[t] = -1;
  if (t < bm::SLOTS * 3) s_zr[t] = bm::empty_zr(t % 3);
  __syncthreads();

  bm::Dir d[PER_LANE];
  bool live[PER_LANE];
#pragma unroll
  for (int j = 0; j < PER_LANE; ++j) {
    const int aj = lane + 64 * j;
    d[j] = aj < A ? bm::dir_at(a.dirs, aj) : bm::Dir{0, 0, 0, 0, false};
    live[j] = d[j].live;
  }
  Hand h;
  hand_reset(h, -1);
  const int x0 = (blockIdx.x / tiles_y) * bm::TILE, y0 = (blockIdx.x % tiles_y) * bm::TILE;
  for (int c = 0; c < CPW; ++c) {
    const int ix = x0 + (wave * CPW + c) / bm::TILE, iy = y0 + (wave * CPW + c) % bm::TILE;
    if (ix >= nx || iy >= ny) continue;                           // wave-uniform
    int32_t u[PER_LANE], v[PER_LANE];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) u[j] = bm::along(d[j], ix, iy), v[j] = bm::across(d[j], ix, iy);
    const int64_t base = ((int64_t)ix * ny + iy) * nz;
    for (int z0 = 0; z0 < nz; z0 += 64) {
      const int len = nz - z0 < 64 ? nz - z0 : 64;
      int32_t lab = lane < len ? a.labels[base + z0 + lane] : -1;
      if (!bm::object_of(lab, K)) lab = -1;
      const int32_t before = __shfl_up(lab, 1, 64);
      unsigned long long heads = __ballot(lane < len && (lane == 0 || lab != before));
      const int runs = __popcll(heads);
      for (int r = 0; r < runs; ++r) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)heads) - 1);
        heads &= heads - 1;
        const int end = heads ? __builtin_amdgcn_readfirstlane(__ffsll((long long)heads) - 1) : len;
        const int32_t k = __builtin_amdgcn_readlane(lab, first);
        if (k < 0) continue;                                      // no object: the one in hand stays
        if (k != h.label) {
          if (h.label >= 0) hand_over(a, h, live, s_key, s_ext, s_zr, lane);
          hand_reset(h, k);
        }
        h.zmin = min(h.zmin, z0 + first), h.zmax = max(h.zmax, z0 + end - 1), h.count += end - first;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j)
          h.e[j][0] = min(h.e[j][0], u[j]), h.e[j][1] = max(h.e[j][1], u[j]), h.e[j][2] = min(h.e[j][2], v[j]), h.e[j][3] = max(h.e[j][3], v[j]);
      }
    }
  }
  if (h.label >= 0) hand_over(a, h, live, s_key, s_ext, s_zr, lane);
  __syncthreads();

  for (int i = t; i < bm::SLOTS * A; i += THREADS) {              // each claimed slot once: one atomic per destination
    const int slot = i / A, aj = i % A;
    const int32_t k = s_key[slot];                                // -1, or a label that passed object_of
    const int32_t* row = s_ext + (int64_t)slot * 4 * A + aj;
    if (k >= 0 && row[0] <= row[A]) {                             // (a DEAD direction's row stayed EMPTY)
      int32_t* out = a.extent + ((int64_t)k * A + aj) * 4;
      atomicMin(out, row[0]), atomicMax(out + 1, row[A]), atomicMin(out + 2, row[2 * A]), atomicMax(out + 3, row[3 * A]);
    }
  }
  if (t < bm::SLOTS && s_key[t] >= 0) {
    int32_t* z = a.zr + (int64_t)s_key[t] * 3;
    atomicMin(z, s_zr[3 * t]), atomicMax(z + 1, s_zr[3 * t + 1]), atomicAdd(z + 2, s_zr[3 * t + 2]);
  }
}

__global__ __launch_bounds__(THREADS) void boxes_choose_kernel(const bm::ChooseArgs c) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (k >= c.K) return;                                           // (no barrier in this kernel)
  bm::Key key{bm::NO_AREA, -1};
  for (int j = 0; j < PER_LANE; ++j) {
    const int a = lane + 64 * j;
    if (a < c.A) key = bm::better(key, bm::key_of(c, (int)k, a));
  }
  for (int off = 32; off > 0; off >>= 1) {
    const bm::Key other{(int64_t)__shfl_xor((long long)key.area, off, 64), __shfl_xor(key.a, off, 64)};
    key = bm::better(key, other);
  }
  if (lane == 0) bm::write_box(c, (int)k, key);
}

}  // namespace

extern "C" int occ4d_boxes_extents_i32(const int32_t* labels, int nx, int ny, int nz, int K, const int32_t* dirs, int A,
                                       int32_t* extent, int32_t* zr, void* stream) {
  bm::ExtentArgs a; bool empty;
  OCC4D_TRY(bm::check_extents(labels, nx, ny, nz, K, dirs, A, extent, zr, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t words = (int64_t)K * A * 4 + (int64_t)K * 3;      // < 2^32
  boxes_fill_kernel<<<(unsigned)((words + THREADS - 1) / THREADS), THREADS, 0, st>>>(a);
  if ((int64_t)nx * ny * nz > 0) {
    const int tiles_x = (nx + bm::TILE - 1) / bm::TILE, tiles_y = (ny + bm::TILE - 1) / bm::TILE;       // <= 256 each
    boxes_reduce_kernel<<<(unsigned)(tiles_x * tiles_y), THREADS, (size_t)bm::SLOTS * 4 * A * sizeof(int32_t), st>>>(a, tiles_y);
  }
  return occ4d::check_launch("occ4d_boxes_extents_i32");
}

extern "C" int occ4d_boxes_choose_i32(const int32_t* extent, const int32_t* zr, const int32_t* dirs, int K, int A, int32_t* box,
                                      void* stream) {
  bm::ChooseArgs c; bool empty;
  OCC4D_TRY(bm::check_choose(extent, zr, dirs, K, A, box, empty, c));
  if (empty) return OCC4D_OK;
  boxes_choose_kernel<<<(unsigned)(((int64_t)K + WAVES - 1) / WAVES), THREADS, 0, (hipStream_t)stream>>>(c);
  return occ4d::check_launch("occ4d_boxes_choose_i32");
}
