// The watershed segments of an integer height map (include/ext/occ4d_watershed.h).  The rules, the ascent choice, the MERGE test,
// the item bodies and the argument contracts are csrc/watershed_math.hpp, shared with the g++ twin; find and unite are those of
// csrc/components_math.hpp; the LDS tile, the atomics' spelling, the wave aggregation and the launches are here.
//
// 7 + R launches for the labels, R = ceil(log8 n), whatever the data:
//   1 ascent   one workgroup per tile of 8 x 8 x 8 points: the levels of the tile and of a halo of one point into LDS (0: no member,
//              outside the grid), then up(p) of the own points into basin[], the maxima as roots of parent[], low[] and size[]
//              cleared.  Workgroup 0 also makes the rounds' flags.  No traffic between workgroups.
//   R jump     basin[p] = the pointer followed 8 times, in place; round k returns at once when flags[k - 1] == 0.  A word may be read while
//              another workgroup stores it: relaxed AGENT-scope atomic loads and stores (eight XCDs, eight L2s), and either value is
//              an ancestor of p.  Nothing is ordered by them, no workgroup waits for another one.
//   1 merge    one thread per point, its forward neighbours: unite(basin(p), basin(q)) where MERGE holds.  parent[] through relaxed
//              agent-scope atomics, correctness on the atomic minimum's return value alone (csrc/components.hip, pass 2).
//   1 flatten  basin[p] = find(basin[p]), parent[] read only; ONE atomic add to size[rep] and one atomic minimum on low[rep] per run
//              of equal representatives in a wave.
//   4 count, scan, number, label: the scheme of csrc/components.hip with a fourth count, the basins.
//   peaks: clear rows 0 .. min(cap, totals[0]) - 1, then one 64-bit atomic maximum per run of equal labels in a wave, gathered per
//          workgroup and label in LDS first, then the keys unpacked in place.
// No float, no inline assembly, no scratch.
#include "common.hpp"
#include "watershed_math.hpp"
#include "ext/occ4d_watershed.h"

namespace {

namespace ws = occ4d_watershed;
namespace cc = occ4d_components;

constexpr int THREADS = ws::TILE_POINTS;  // the ascent: one thread per point of a tile
constexpr int FLAT = 256;                 // the passes without a tile
constexpr int WAVES = FLAT / 64;
constexpr int SCAN_THREADS = 1024;
constexpr int SLOTS = 64;                 // labels a workgroup of the peaks kernel gathers in LDS
static_assert(FLAT == ws::TILE, "one thread per point of a numbering tile");

struct Agent {                                                    // words that another workgroup may touch in the same launch
  static __device__ __forceinline__ int load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int fetch_min(int32_t* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The lanes of a wave hold consecutive flat indices.  A RUN is a maximal stretch of lanes with the same `value`; -> whether this lane
// heads its run, and the lane behind the run's last one.  Every lane of the wave calls this.  (csrc/components.hip)
__device__ __forceinline__ bool run_of(int value, int& end) {
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(value, 1, 64);
  const bool head = lane == 0 || before != value;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  end = above ? __ffsll((long long)above) - 1 : 64;
  return head;
}

__global__ __launch_bounds__(THREADS) void watershed_ascent_kernel(const ws::Args a) {
  __shared__ int32_t s_level[ws::HALO_POINTS];
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && t < ws::ROUND_WORDS) ws::flag_init(a, t);
  int o[3];
  ws::tile_origin(a, blockIdx.x, o);
  for (int s = t; s < ws::HALO_POINTS; s += THREADS) {
    const int64_t q = ws::halo_point(a, o, s);
    s_level[s] = q < 0 ? 0 : ws::level_of(a.height[q]);
  }
  __syncthreads();
  const int64_t p = ws::own_point(a, o, t);
  if (p < 0) return;
  const int slot = ws::own_slot(t);
  const int32_t own = s_level[slot];
  int c = ws::SELF;
  if (own >= 1) c = ws::ascent_choice(a.rank, own, [&](int dx, int dy, int dz) { return s_level[slot + (dx * ws::HY + dy) * ws::HZ + dz]; });
  ws::ascent_item(a, p, own, c);
}

__global__ __launch_bounds__(FLAT) void watershed_jump_kernel(const ws::Args a, const int k) {
  if (a.flags[k - 1] == 0) return;                                // (written by an earlier launch; the same for every thread)
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const bool changed = p < a.grid.points && ws::jump_item<Agent>(a, p);
  if (__syncthreads_or(changed) && threadIdx.x == 0) Agent::store(a.flags + k, 1);
}

__global__ __launch_bounds__(FLAT) void watershed_merge_kernel(const ws::Args a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (p < a.grid.points) ws::merge_item<Agent>(a, p);
}

__global__ __launch_bounds__(FLAT) void watershed_flatten_kernel(const ws::Args a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const int r = p < a.grid.points ? ws::flatten_item(a, p) : -1;
  int end;
  const bool head = run_of(r, end);
  if (head && r >= 0) {
    atomicAdd(a.size + r, end - (int)(threadIdx.x & 63));
    atomicMin(a.low + r, (int)p);                                 // (the head is the run's lowest index)
  }
}

__global__ __launch_bounds__(FLAT) void watershed_count_kernel(const ws::Args a) {
  __shared__ int s[ws::TOTALS][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const bool in = p < a.grid.points;
  for (int c = 0; c < ws::TOTALS; ++c) {
    const unsigned long long m = __ballot(in && ws::flag_of(a, p, c));
    if (lane == 0) s[c][wave] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < ws::TOTALS) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += s[threadIdx.x][w];
    a.counts[threadIdx.x][blockIdx.x] = sum;
  }
}

// workgroup b: the exclusive prefix of count array b and its total (chunks of 1024 tiles with a carry)
__global__ __launch_bounds__(SCAN_THREADS) void watershed_scan_kernel(const ws::Args a) {
  __shared__ int s[SCAN_THREADS];
  int32_t* counts = a.counts[blockIdx.x];
  const int64_t tiles = a.grid.number_tiles;
  int carry = 0;
  for (int64_t base = 0; base < tiles; base += SCAN_THREADS) {            // (uniform over the workgroup: barriers inside)
    const int64_t i = base + threadIdx.x;
    const int v = i < tiles ? counts[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < tiles) counts[i] = carry + s[threadIdx.x] - v;
    const int chunk_total = s[SCAN_THREADS - 1];
    __syncthreads();
    carry += chunk_total;
  }
  if (threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(FLAT) void watershed_number_kernel(const ws::Args a) {
  __shared__ int s[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const bool kept = p < a.grid.points && ws::is_kept_root(a, p);
  const unsigned long long m = __ballot(kept);
  if (lane == 0) s[wave] = __popcll(m);
  __syncthreads();
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += s[w];
  if (kept) ws::number_item(a, p, a.counts[0][blockIdx.x] + rank);
}

__global__ __launch_bounds__(FLAT) void watershed_label_kernel(const ws::Args a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (p < a.grid.points) ws::label_item(a, p);
}

__global__ __launch_bounds__(FLAT) void watershed_peaks_init_kernel(const ws::PeakArgs a) {
  const int64_t k = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (k < ws::peak_rows(a)) a.keys[k] = 0;
}

__device__ __forceinline__ void key_max(unsigned long long* p, unsigned long long key, bool lds) {
  if (lds) __hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One key per run of equal labels in a wave, the run's maximum, gathered per workgroup before it reaches the row: a run's head claims
// LDS slot (label mod SLOTS) for its label with a compare-and-swap and raises the key there; a head that finds the slot taken by
// another label raises the row directly.  After the barrier each claimed slot goes to its row once (csrc/components.hip, the table).
__global__ __launch_bounds__(FLAT) void watershed_peaks_kernel(const ws::PeakArgs a) {
  __shared__ int32_t s_label[SLOTS];
  __shared__ unsigned long long s_key[SLOTS];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < SLOTS) {
    s_label[threadIdx.x] = -1;
    s_key[threadIdx.x] = 0;
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const int rows = ws::peak_rows(a);
  unsigned long long key = 0;
  const int k = p < a.n ? ws::peak_contribution(a, p, rows, key) : -1;    // (0 <= k < rows, or -1)
  int end;
  const bool head = run_of(k, end);
  for (int off = 1; off < 64; off <<= 1) {                                // after the step `off` a lane holds lanes [lane, min(lane + 2 off, end))
    const unsigned long long o = __shfl_down(key, off, 64);
    if (lane + off < end && o > key) key = o;
  }
  if (head && k >= 0) {
    const int slot = k % SLOTS;
    const int owner = atomicCAS(s_label + slot, -1, k);                   // -1: claimed now;  k: claimed before, for this label
    if (owner == -1 || owner == k) key_max(s_key + slot, key, true);
    else key_max(a.keys + k, key, false);
  }
  __syncthreads();
  if (threadIdx.x < SLOTS) {
    const int label = s_label[threadIdx.x];
    if (label >= 0 && label < rows) key_max(a.keys + label, s_key[threadIdx.x], false);
  }
}

__global__ __launch_bounds__(FLAT) void watershed_peaks_unpack_kernel(const ws::PeakArgs a) {
  const int64_t k = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  if (k < ws::peak_rows(a)) ws::peak_unpack(a, (int)k);
}

}  // namespace

extern "C" int occ4d_watershed_label_i32(const int32_t* height, int nx, int ny, int nz, int connectivity, int h, int min_size,
                                         int32_t* work, int32_t* labels, int32_t* totals, void* stream) {
  ws::Args a; bool empty;
  OCC4D_TRY(ws::check_label(height, nx, ny, nz, connectivity, h, min_size, work, labels, totals, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)a.grid.number_tiles;                   // n <= INT32_MAX: both tile counts fit
  watershed_ascent_kernel<<<(unsigned)a.n_tiles, THREADS, 0, st>>>(a);
  for (int k = 1; k <= a.rounds; ++k) watershed_jump_kernel<<<tiles, FLAT, 0, st>>>(a, k);
  watershed_merge_kernel<<<tiles, FLAT, 0, st>>>(a);
  watershed_flatten_kernel<<<tiles, FLAT, 0, st>>>(a);
  watershed_count_kernel<<<tiles, FLAT, 0, st>>>(a);
  watershed_scan_kernel<<<ws::TOTALS, SCAN_THREADS, 0, st>>>(a);
  watershed_number_kernel<<<tiles, FLAT, 0, st>>>(a);
  watershed_label_kernel<<<tiles, FLAT, 0, st>>>(a);
  return occ4d::check_launch("occ4d_watershed_label_i32");
}

extern "C" int occ4d_watershed_peaks_i32(const int32_t* height, const int32_t* labels, int n, const int32_t* totals, int32_t* peaks,
                                         int cap, void* stream) {
  ws::PeakArgs a; bool empty;
  OCC4D_TRY(ws::check_peaks(height, labels, n, totals, peaks, cap, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned row_groups = (unsigned)(((int64_t)cap + FLAT - 1) / FLAT);
  watershed_peaks_init_kernel<<<row_groups, FLAT, 0, st>>>(a);
  watershed_peaks_kernel<<<(unsigned)(((int64_t)n + FLAT - 1) / FLAT), FLAT, 0, st>>>(a);
  watershed_peaks_unpack_kernel<<<row_groups, FLAT, 0, st>>>(a);
  return occ4d::check_launch("occ4d_watershed_peaks_i32");
}
