// The connected components of the grid's solid set (include/ext/occ4d_components.h): label-equivalence union-find.  The rules, find
// and unite, the item bodies and the argument contracts are csrc/components_math.hpp, shared with the g++ twin; the tiling, the
// atomics' spelling, the wave aggregation and the launches are here.
//
// THE INVARIANT: parent[x] <= x and parent[x] lies in x's component.  A root is only ever linked, by an atomic minimum, to a lower
// flat index of its own component, so every chain strictly decreases and a component's final root is its lowest index whatever the
// order of events.  Seven launches for the labels, two for the table, whatever the data:
//   1 local    one workgroup per tile of 6 x 7 x 6 points, union-find in LDS (workgroup-scope atomics), then parent[p] = the flat
//              index of the point's local root (-1: no member), size[p] = 0.  No traffic between workgroups.
//   2 border   one thread per point: unite(p, q) for every backward neighbour q in another tile.  The eight XCDs have L2s of their
//              own, so a plain load of parent[] could return an old value for as long as the kernel runs: every load here is a
//              relaxed AGENT-scope atomic load, and correctness rests on the atomic minimum's return value alone (an old parent is
//              still an ancestor).  No workgroup waits for another one: no flags, no tickets, no spinning; each loop ends because
//              an integer strictly decreases (the argument stands above find and unite).
//   3 flatten  root[p] = find(p), parent[] read only (a kernel boundary after pass 2), size[root] += 1: ONE atomic add per run of
//              equal roots in a wave -- an all-solid grid, the floor, adds once per wave, not once per point.
//   4 count    per tile of 256 points: kept roots, points of kept components, all roots.
//   5 scan     exclusive prefixes of the three and their totals (surface_scan_kernel's construction).
//   6 number   a kept root's number = its tile's prefix + its rank in the tile, into parent[root].
//   7 label    labels[p] = the number of root[p], or -1.
//   table: init rows 0 .. min(cap, totals[0]) - 1, then one contribution per run of equal labels in a wave, reduced over the run
//          with shuffles, gathered per workgroup and label in LDS, and added to the row with 64-bit integer atomics (add / min /
//          max: any order gives the same bits).
// Passes 1 and 3 .. 7 rely on kernel boundaries only.  No float atomics, no inline assembly.
#include "common.hpp"
#include "components_math.hpp"
#include "ext/occ4d_components.h"

namespace {

namespace cc = occ4d_components;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 1024;
constexpr int SLOTS = 64;                 // labels a workgroup of the table kernel gathers in LDS
static_assert(THREADS == cc::TILE && cc::TILE_POINTS <= THREADS, "one thread per point of either tile");

struct Lds {                                                      // pass 1: the tile's arrays in LDS
  static __device__ __forceinline__ int load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ int fetch_min(int32_t* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

struct Agent {                                                    // pass 2: parent[] across workgroups and XCDs
  static __device__ __forceinline__ int load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int fetch_min(int32_t* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

struct LdsTable {                                                 // the table kernel's slots in LDS
  static __device__ __forceinline__ void add(int64_t* p, int64_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ void min(int64_t* p, int64_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ void max(int64_t* p, int64_t v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

struct AgentTable {
  static __device__ __forceinline__ void add(int64_t* p, int64_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void min(int64_t* p, int64_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void max(int64_t* p, int64_t v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The lanes of a wave hold consecutive flat indices.  A RUN is a maximal stretch of lanes with the same `value`; -> whether this lane
// heads its run, and the lane behind the run's last one.  Every lane of the wave calls this.
__device__ __forceinline__ bool run_of(int value, int& end) {
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(value, 1, 64);
  const bool head = lane == 0 || before != value;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  end = above ? __ffsll((long long)above) - 1 : 64;
  return head;
}

__global__ __launch_bounds__(THREADS) void components_local_kernel(const cc::LabelArgs a) {
  __shared__ int32_t s_parent[THREADS], s_key[THREADS];
  const int t = threadIdx.x;
  const cc::LocalPoint q = cc::local_point(a.grid, blockIdx.x, t);
  cc::local_init(a, q, t, s_parent, s_key);
  __syncthreads();
  cc::local_link<Lds>(a, q, t, s_parent, s_key);
  __syncthreads();
  cc::local_write<Lds>(a, a.grid, blockIdx.x, q, t, s_parent);
}

__global__ __launch_bounds__(THREADS) void components_border_kernel(const cc::LabelArgs a) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (p < a.grid.points) cc::border_item<Agent>(a, p);
}

__global__ __launch_bounds__(THREADS) void components_flatten_kernel(const cc::LabelArgs a) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int r = p < a.grid.points ? cc::flatten_item(a, p) : -1;
  int end;
  const bool head = run_of(r, end);
  if (head && r >= 0) atomicAdd(a.size + r, end - (int)(threadIdx.x & 63));
}

// the three flags of point p, and their ranks / sums over the tile; s: 3 * WAVES ints
struct Flags {
  bool kept_root, kept_point, root;
};

__device__ __forceinline__ Flags flags_of(const cc::LabelArgs& a, int64_t p) {
  if (p >= a.grid.points) return Flags{false, false, false};
  return Flags{cc::is_kept_root(a, p), cc::is_kept_point(a, p), cc::is_root(a, p)};
}

__global__ __launch_bounds__(THREADS) void components_count_kernel(const cc::LabelArgs a) {
  __shared__ int s[3][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Flags f = flags_of(a, (int64_t)blockIdx.x * THREADS + threadIdx.x);
  const unsigned long long m0 = __ballot(f.kept_root), m1 = __ballot(f.kept_point), m2 = __ballot(f.root);
  if (lane == 0) {
    s[0][wave] = __popcll(m0);
    s[1][wave] = __popcll(m1);
    s[2][wave] = __popcll(m2);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += s[threadIdx.x][w];
    (threadIdx.x == 0 ? a.kept_roots : threadIdx.x == 1 ? a.kept_points : a.all_roots)[blockIdx.x] = sum;
  }
}

// workgroup b: the exclusive prefix of count array b and its total (chunks of 1024 tiles with a carry)
__global__ __launch_bounds__(SCAN_THREADS) void components_scan_kernel(const cc::LabelArgs a) {
  __shared__ int s[SCAN_THREADS];
  int32_t* counts = blockIdx.x == 0 ? a.kept_roots : blockIdx.x == 1 ? a.kept_points : a.all_roots;
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

__global__ __launch_bounds__(THREADS) void components_number_kernel(const cc::LabelArgs a) {
  __shared__ int s[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const bool kept = p < a.grid.points && cc::is_kept_root(a, p);
  const unsigned long long m = __ballot(kept);
  if (lane == 0) s[wave] = __popcll(m);
  __syncthreads();
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += s[w];
  if (kept) a.parent[p] = a.kept_roots[blockIdx.x] + rank;
}

__global__ __launch_bounds__(THREADS) void components_label_kernel(const cc::LabelArgs a) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (p < a.grid.points) cc::label_item(a, p);
}

__global__ __launch_bounds__(THREADS) void components_table_init_kernel(const cc::TableArgs a) {
  const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (k < cc::table_rows(a)) cc::table_init_row(a, (int)k);
}

// One contribution per run of equal labels in a wave, gathered per workgroup before it reaches the table: a run's head claims LDS
// slot (label mod SLOTS) for its label with a compare-and-swap and adds there with 64-bit LDS atomics; a head that finds the slot
// taken by another label adds to the table's row directly.  After the barrier each claimed slot goes to its row once.  So a large
// component -- the floor, an all-solid grid -- costs a row one set of atomics per WORKGROUP, not per run: atomics on one address
// are served one after the other.  Integer add / min / max: the order changes no bit.
__global__ __launch_bounds__(THREADS) void components_table_kernel(const cc::TableArgs a) {
  __shared__ int32_t s_label[SLOTS];
  __shared__ int64_t s_row[SLOTS][cc::COLS];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < SLOTS) {
    s_label[threadIdx.x] = -1;
    cc::row_init(s_row[threadIdx.x]);
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const bool in = p < a.grid.points;
  const int rows = cc::table_rows(a);
  int k = in ? a.labels[p] : -1;
  if (k >= rows) k = -1;                                                  // (a row that does not exist: the guard)
  cc::Contribution c = cc::contribution_of(a, in ? p : 0);
  int end;
  const bool head = run_of(k, end);
  // the run's sums, minima and maxima into its head: after the step `off` a lane holds lanes [lane, min(lane + 2 off, end))
  for (int off = 1; off < 64; off <<= 1) {
    cc::Contribution o = c;
    for (int x = 0; x < 3; ++x) {
      o.sum[x] = __shfl_down(c.sum[x], off, 64);
      o.lo[x] = __shfl_down(c.lo[x], off, 64);
      o.hi[x] = __shfl_down(c.hi[x], off, 64);
    }
    if (lane + off < end) {
      for (int x = 0; x < 3; ++x) {
        c.sum[x] += o.sum[x];
        c.lo[x] = o.lo[x] < c.lo[x] ? o.lo[x] : c.lo[x];
        c.hi[x] = o.hi[x] > c.hi[x] ? o.hi[x] : c.hi[x];
      }
    }
  }
  c.count = end - lane;                          // (first and klass are the head's own: the run's lowest index, one class per component)
  if (head && k >= 0) {
    const int slot = k % SLOTS;
    const int owner = atomicCAS(s_label + slot, -1, k);                   // -1: claimed now;  k: claimed before, for this label
    if (owner == -1 || owner == k) cc::row_add<LdsTable>(s_row[slot], c);
    else cc::table_add<AgentTable>(a, k, rows, c);
  }
  __syncthreads();
  if (threadIdx.x < SLOTS && s_label[threadIdx.x] >= 0)
    cc::table_add<AgentTable>(a, s_label[threadIdx.x], rows, cc::contribution_of_row(s_row[threadIdx.x]));
}

}  // namespace

extern "C" int occ4d_components_label_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask,
                                          float mask_level, const int32_t* klass, int nx, int ny, int nz, int connectivity,
                                          int min_size, int32_t* work, int32_t* labels, int32_t* totals, void* stream) {
  cc::LabelArgs a; bool empty;
  OCC4D_TRY(cc::check_label(field, ld, level, mask, ld_mask, mask_level, klass, nx, ny, nz, connectivity, min_size, work, labels, totals,
                            empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)a.grid.number_tiles;                   // n <= INT32_MAX: both tile counts fit
  components_local_kernel<<<(unsigned)a.grid.local_tiles, THREADS, 0, st>>>(a);
  components_border_kernel<<<tiles, THREADS, 0, st>>>(a);
  components_flatten_kernel<<<tiles, THREADS, 0, st>>>(a);
  components_count_kernel<<<tiles, THREADS, 0, st>>>(a);
  components_scan_kernel<<<3, SCAN_THREADS, 0, st>>>(a);
  components_number_kernel<<<tiles, THREADS, 0, st>>>(a);
  components_label_kernel<<<tiles, THREADS, 0, st>>>(a);
  return occ4d::check_launch("occ4d_components_label_f32");
}

extern "C" int occ4d_components_table_i64(const int32_t* labels, const int32_t* klass, int nx, int ny, int nz, const int32_t* totals,
                                          int64_t* table, int cap, void* stream) {
  cc::TableArgs a; bool empty;
  OCC4D_TRY(cc::check_table(labels, klass, nx, ny, nz, totals, table, cap, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  components_table_init_kernel<<<(unsigned)(((int64_t)cap + THREADS - 1) / THREADS), THREADS, 0, st>>>(a);
  components_table_kernel<<<(unsigned)a.grid.number_tiles, THREADS, 0, st>>>(a);
  return occ4d::check_launch("occ4d_components_table_i64");
}
