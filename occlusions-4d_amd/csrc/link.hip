// The components of two frames linked (include/ext/occ4d_link.h).  The rules, the open-addressing insert, the order relation, the
// item bodies and the argument contracts are csrc/link_math.hpp, shared with the g++ twin; the atomics' spelling, the wave
// aggregation, the LDS gather and the launches are here.
//
// THE OVERLAP, six launches whatever the data:
//   1 clear    the table's keys EMPTY, counts 0, roots INT32_MAX; at[p] = -1; the overflow word 0.
//   2 insert   one thread per point, one workgroup per numbering tile.  The lanes of a wave hold consecutive flat indices: each run
//              of equal (a, b) is reduced with a ballot and only its head inserts, with the run's length and its own index (the
//              run's lowest).  The heads of a workgroup are gathered per key in a table of 64 slots in LDS first (workgroup-scope
//              atomics, the same insert); after the barrier each used LDS slot goes to the global table ONCE.  So a large pair --
//              an all-solid pair of frames is one pair of n points -- costs one global insert per WORKGROUP, not per point or per
//              run: atomics on one address are served one after the other.  A head that finds no LDS slot inserts globally itself.
//              The global insert is a 64-bit compare-and-swap on the key, an integer add on the count, an integer minimum on the
//              root.  The eight XCDs have L2s of their own: every load of a key another workgroup may write in this launch is a
//              relaxed AGENT-scope atomic load, and correctness rests on the value the compare-and-swap returns alone (a slot never
//              changes its key once it has one, so an old EMPTY only costs a compare-and-swap that reports the key).  Add and
//              minimum of integers: any order gives the same bits.  The probe sequence is a `for` over at most `slots` slots, which
//              then sets totals[2]; it is never a spin.  No workgroup waits for another: no flags, no tickets.
//   3 mark     (a kernel boundary later: plain loads) each used slot writes its number at at[root]; roots are distinct.
//   4 count    per tile of 256 points: the roots of pairs.  (The member points per tile come from pass 2.)
//   5 scan     exclusive prefixes of the two and their totals (components_scan_kernel's construction).
//   6 number   a pair's number = its tile's prefix + its root's rank in the tile; row i < cap of `pairs`.
// The hash function and the slot order reach no output: a pair's number comes from its root alone.
//
// THE MATCH, five launches whatever the data:
//   1 init     link and best_a rows.
//   2 best     one thread per pair: a compare-and-swap loop raises link[b][2] and best_a[a][0], the index of the best pair so far,
//              under the strict total order of link_math.hpp (agent-scope atomics).  It ends because the slot only ever moves up
//              that order; the `for` is bounded by the number of pairs.
//   3 resolve  one thread per b: linked when both slots hold the same pair and the threshold holds; the id hand-over.
//   4 finish   one thread per a: the pair index replaced by b and the count (pass 3 has read it).
//   5 rank     ONE workgroup: the unlinked b ranked by a chunked scan (k_b is small), next_out.
// No float atomics, no inline assembly.
#include "common.hpp"
#include "link_math.hpp"
#include "ext/occ4d_link.h"

namespace {

namespace lk = occ4d_link;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 1024;
constexpr int LDS_SLOTS = 64;             // keys a workgroup of the insert kernel gathers in LDS
constexpr int LDS_SHIFT = 58;             // 64 - log2(LDS_SLOTS)
constexpr int LDS_PROBES = 8;
static_assert(THREADS == lk::TILE, "one thread per point of a numbering tile");
static_assert((1 << (64 - LDS_SHIFT)) == LDS_SLOTS && LDS_SLOTS <= THREADS && LDS_PROBES <= LDS_SLOTS, "the LDS table");

template <int SCOPE>
struct Atomics {
  static __device__ __forceinline__ int64_t load64(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ int64_t cas64(int64_t* p, int64_t expected, int64_t desired) {
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return expected;                                                      // (the value before, whether it was exchanged or not)
  }
  static __device__ __forceinline__ int32_t load32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ int32_t cas32(int32_t* p, int32_t expected, int32_t desired) {
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return expected;
  }
  static __device__ __forceinline__ void add32(int32_t* p, int32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ void min32(int32_t* p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ void store32(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
};
using Lds = Atomics<__HIP_MEMORY_SCOPE_WORKGROUP>;
using Agent = Atomics<__HIP_MEMORY_SCOPE_AGENT>;

// The lanes of a wave hold consecutive flat indices.  A RUN is a maximal stretch of lanes with the same key; -> whether this lane
// heads its run, and the lane behind the run's last one.  Every lane of the wave calls this.
__device__ __forceinline__ bool run_of(int64_t key, int& end) {
  const int lane = threadIdx.x & 63;
  const int lo = __shfl_up((int)(key & 0xffffffffll), 1, 64), hi = __shfl_up((int)(key >> 32), 1, 64);
  const bool head = lane == 0 || lo != (int)(key & 0xffffffffll) || hi != (int)(key >> 32);
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  end = above ? __ffsll((long long)above) - 1 : 64;
  return head;
}

__global__ __launch_bounds__(THREADS) void link_clear_kernel(const lk::OverlapArgs a, int64_t items) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < items) lk::clear_item(a, i);
}

__global__ __launch_bounds__(THREADS) void link_insert_kernel(const lk::OverlapArgs a) {
  __shared__ int64_t s_keys[LDS_SLOTS];
  __shared__ int32_t s_count[LDS_SLOTS], s_root[LDS_SLOTS];
  __shared__ int s_members[WAVES];
  const lk::Table lds{s_keys, s_count, s_root, LDS_SLOTS, LDS_SHIFT};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < LDS_SLOTS) lk::table_clear(lds, threadIdx.x);
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t key = p < a.n ? lk::key_of(a, p) : lk::EMPTY;
  const unsigned long long members = __ballot(key != lk::EMPTY);
  if (lane == 0) s_members[wave] = __popcll(members);
  int end;
  const bool head = run_of(key, end);
  if (head && key != lk::EMPTY) {
    const int32_t count = end - lane;
    if (!lk::insert<Lds>(lds, key, count, (int32_t)p, LDS_PROBES)) lk::insert_item<Agent>(a, key, count, p);
  }
  __syncthreads();
  if (threadIdx.x < LDS_SLOTS && s_keys[threadIdx.x] != lk::EMPTY)
    lk::insert_item<Agent>(a, s_keys[threadIdx.x], s_count[threadIdx.x], s_root[threadIdx.x]);
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += s_members[w];
    a.tile_members[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(THREADS) void link_mark_kernel(const lk::OverlapArgs a) {
  const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (s < a.table.slots) lk::mark_item(a, s);
}

__global__ __launch_bounds__(THREADS) void link_count_kernel(const lk::OverlapArgs a) {
  __shared__ int s[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const unsigned long long m = __ballot(p < a.n && lk::is_pair_root(a, p));
  if (lane == 0) s[wave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += s[w];
    a.tile_pairs[blockIdx.x] = sum;
  }
}

// the exclusive prefix of counts[0 .. items) in place and its total (chunks of 1024 with a carry), by one workgroup
__device__ __forceinline__ int scan_in_place(int32_t* counts, int64_t items, int* s) {
  int carry = 0;
  for (int64_t base = 0; base < items; base += SCAN_THREADS) {            // (uniform over the workgroup: barriers inside)
    const int64_t i = base + threadIdx.x;
    const int v = i < items ? counts[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < items) counts[i] = carry + s[threadIdx.x] - v;
    const int chunk_total = s[SCAN_THREADS - 1];
    __syncthreads();
    carry += chunk_total;
  }
  return carry;
}

// workgroup 0: the pairs, workgroup 1: the member points
__global__ __launch_bounds__(SCAN_THREADS) void link_scan_kernel(const lk::OverlapArgs a) {
  __shared__ int s[SCAN_THREADS];
  const int total = scan_in_place(blockIdx.x == 0 ? a.tile_pairs : a.tile_members, a.tiles, s);
  if (threadIdx.x == 0) a.totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(THREADS) void link_number_kernel(const lk::OverlapArgs a) {
  __shared__ int s[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const bool root = p < a.n && lk::is_pair_root(a, p);
  const unsigned long long m = __ballot(root);
  if (lane == 0) s[wave] = __popcll(m);
  __syncthreads();
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += s[w];
  if (root) lk::pair_write(a, p, (int64_t)a.tile_pairs[blockIdx.x] + rank);
}

__global__ __launch_bounds__(THREADS) void link_init_kernel(const lk::MatchArgs m) {
  lk::init_item(m, (int64_t)blockIdx.x * THREADS + threadIdx.x);
}

__global__ __launch_bounds__(THREADS) void link_best_kernel(const lk::MatchArgs m) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int rows = lk::pair_rows(m);
  if (i < rows) lk::best_item<Agent>(m, rows, (int)i);
}

__global__ __launch_bounds__(THREADS) void link_resolve_kernel(const lk::MatchArgs m) {
  const int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (b < m.k_b) lk::resolve_item(m, lk::pair_rows(m), b);
}

__global__ __launch_bounds__(THREADS) void link_finish_kernel(const lk::MatchArgs m) {
  const int64_t ka = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (ka < m.k_a) lk::finish_item(m, lk::pair_rows(m), ka);
}

// one workgroup: the unlinked b numbered from next_in[0] on, in order (chunks of 1024 with a carry)
__global__ __launch_bounds__(SCAN_THREADS) void link_rank_kernel(const lk::MatchArgs m) {
  __shared__ int s[SCAN_THREADS];
  const int32_t next = m.next_in[0];
  int carry = 0;
  for (int64_t base = 0; base < m.k_b; base += SCAN_THREADS) {            // (uniform over the workgroup: barriers inside)
    const int64_t b = base + threadIdx.x;
    const int v = b < m.k_b && lk::is_new(m, b) ? 1 : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (v) lk::new_id(m, b, next + carry + s[threadIdx.x] - 1);
    const int chunk_total = s[SCAN_THREADS - 1];
    __syncthreads();
    carry += chunk_total;
  }
  __syncthreads();                                                        // (next_out may be next_in: every thread has read it)
  if (threadIdx.x == 0) m.next_out[0] = next + carry;
}

unsigned blocks(int64_t items) { return (unsigned)((items + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int occ4d_link_overlap_i32(const int32_t* labels_a, const int32_t* labels_b, int k_a, int k_b, int64_t n, int32_t* work,
                                      int64_t* pairs, int cap, int32_t* totals, void* stream) {
  lk::OverlapArgs a; bool empty;
  OCC4D_TRY(lk::check_overlap(labels_a, labels_b, k_a, k_b, n, work, pairs, cap, totals, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)a.tiles;                               // n <= INT32_MAX, slots <= 2^31: every grid fits
  const int64_t items = a.table.slots > n ? a.table.slots : n;
  link_clear_kernel<<<blocks(items), THREADS, 0, st>>>(a, items);
  link_insert_kernel<<<tiles, THREADS, 0, st>>>(a);
  link_mark_kernel<<<blocks(a.table.slots), THREADS, 0, st>>>(a);
  link_count_kernel<<<tiles, THREADS, 0, st>>>(a);
  link_scan_kernel<<<2, SCAN_THREADS, 0, st>>>(a);
  link_number_kernel<<<tiles, THREADS, 0, st>>>(a);
  return occ4d::check_launch("occ4d_link_overlap_i32");
}

extern "C" int occ4d_link_match_i32(const int64_t* pairs, const int32_t* totals, int cap, const int64_t* table_a, int64_t ld_a,
                                    const int64_t* table_b, int64_t ld_b, int k_a, int k_b, const int32_t* track_a, int iou_num,
                                    int iou_den, const int32_t* next_in, int32_t* link, int32_t* best_a, int32_t* next_out, void* stream) {
  lk::MatchArgs m;
  OCC4D_TRY(lk::check_match(pairs, totals, cap, table_a, ld_a, table_b, ld_b, k_a, k_b, track_a, iou_num, iou_den, next_in, link, best_a,
                            next_out, m));
  const hipStream_t st = (hipStream_t)stream;
  // (a grid of at least one workgroup each, so that the launch count does not depend on the sizes)
  const auto at_least_one = [](int64_t items) { return items > 0 ? blocks(items) : 1u; };
  link_init_kernel<<<at_least_one(k_a > k_b ? k_a : k_b), THREADS, 0, st>>>(m);
  link_best_kernel<<<at_least_one(m.used ? cap : 0), THREADS, 0, st>>>(m);
  link_resolve_kernel<<<at_least_one(k_b), THREADS, 0, st>>>(m);
  link_finish_kernel<<<at_least_one(k_a), THREADS, 0, st>>>(m);
  link_rank_kernel<<<1, SCAN_THREADS, 0, st>>>(m);
  return occ4d::check_launch("occ4d_link_match_i32");
}
