// Host concurrency check of the two passes of the frame linking that race (csrc/link_math.hpp): the open-addressing insert and the
// compare-and-swap loop on the best pair, with the atomics spelled as relaxed std::atomic_ref operations, run on 16 std::threads
// under ThreadSanitizer.  No GPU, no Python.
//
//   g++ -std=c++20 -O1 -g -fsanitize=thread -pthread -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/link_threads.cpp \
//       -o link_threads && ./link_threads
//
// Per pair of label volumes of 19 200 points -- striped labels with holes against the same moved by 9 points (100 pairs), one pair throughout (every thread on
// one slot), foreign labels with k = cap = n (the fullest table the contract allows) and the same with cap = 1 (64 slots for 19 200
// keys: every probe sequence must end and set the overflow word) -- the points are dealt round-robin to 16 threads, each calling
// insert_item on the shared table; then the pairs are dealt round-robin to 16 threads, each calling best_item.  The pair rows, the
// totals, link, best_a and next_out are compared with those of one thread.  Exits non-zero on a mismatch (or when ThreadSanitizer
// reports a race).
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "link_math.hpp"

void occ4d::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

namespace lk = occ4d_link;

struct Atomic {
  template <class T>
  static std::atomic_ref<T> ref(const T* p) { return std::atomic_ref<T>(*const_cast<T*>(p)); }
  static int64_t load64(const int64_t* p) { return ref(p).load(std::memory_order_relaxed); }
  static int64_t cas64(int64_t* p, int64_t expected, int64_t desired) {
    ref(p).compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
    return expected;
  }
  static int32_t load32(const int32_t* p) { return ref(p).load(std::memory_order_relaxed); }
  static int32_t cas32(int32_t* p, int32_t expected, int32_t desired) {
    ref(p).compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
    return expected;
  }
  static void add32(int32_t* p, int32_t v) { ref(p).fetch_add(v, std::memory_order_relaxed); }
  static void min32(int32_t* p, int32_t v) {                                // (std::atomic has no fetch_min before C++26)
    int32_t before = ref(p).load(std::memory_order_relaxed);
    while (v < before && !ref(p).compare_exchange_weak(before, v, std::memory_order_relaxed, std::memory_order_relaxed)) {
    }
  }
  static void store32(int32_t* p, int32_t v) { ref(p).store(v, std::memory_order_relaxed); }
};

constexpr int N = 19200, THREADS = 16;

struct Result {
  std::vector<int64_t> pairs;
  std::vector<int32_t> totals, link, best_a;
  int32_t next_out;
  bool operator==(const Result& o) const {
    return pairs == o.pairs && totals == o.totals && link == o.link && best_a == o.best_a && next_out == o.next_out;
  }
};

template <class F>
static void on_threads(int threads, int64_t items, F&& body) {
  if (threads == 1) {
    for (int64_t i = 0; i < items; ++i) body(i);
    return;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      for (int64_t i = t; i < items; i += threads) body(i);
    });
  for (std::thread& th : pool) th.join();
}

static std::vector<int64_t> table_of(const std::vector<int32_t>& labels, int k) {
  std::vector<int64_t> table((size_t)k * 12, -7);
  for (int i = 0; i < k; ++i) table[(size_t)i * 12] = 0;
  for (int32_t l : labels)
    if (l >= 0 && l < k) table[(size_t)l * 12] += 1;
  return table;
}

// the overlap and the match of one pair of volumes, the two racing passes on `threads` threads
static bool link_frames(const std::vector<int32_t>& la, const std::vector<int32_t>& lb, int k_a, int k_b, int cap, int threads, Result& r) {
  const int64_t slots = lk::slots_for(N, cap);
  std::vector<int64_t> work64(2 * slots + (N + 2 * ((N + lk::TILE - 1) / lk::TILE) + 1) / 2 + 1);     // (int64: 8-byte aligned)
  r.pairs.assign((size_t)cap * 4, -1);
  r.totals.assign(3, -1);
  lk::OverlapArgs a;
  bool empty;
  if (lk::check_overlap(la.data(), lb.data(), k_a, k_b, N, (int32_t*)work64.data(), r.pairs.data(), cap, r.totals.data(), empty, a) != OCC4D_OK)
    return false;
  for (int64_t i = 0; i < std::max<int64_t>(slots, N); ++i) lk::clear_item(a, i);
  on_threads(threads, N, [&](int64_t p) {
    const int64_t key = lk::key_of(a, p);
    if (key != lk::EMPTY) lk::insert_item<Atomic>(a, key, 1, p);
  });
  for (int64_t s = 0; s < slots; ++s) lk::mark_item(a, s);
  int32_t numbered = 0, members = 0;
  for (int64_t p = 0; p < N; ++p) {
    members += lk::key_of(a, p) != lk::EMPTY;
    if (lk::is_pair_root(a, p)) lk::pair_write(a, p, numbered++);
  }
  r.totals[0] = numbered;
  r.totals[1] = members;
  if (r.totals[2]) r.pairs.assign((size_t)cap * 4, -1);                    // (overflow: the rows are unspecified)

  const std::vector<int64_t> table_a = table_of(la, k_a), table_b = table_of(lb, k_b);
  std::vector<int32_t> track_a(k_a);
  for (int i = 0; i < k_a; ++i) track_a[i] = 3 * i + 5;
  const int32_t next_in = 1000;
  r.link.assign((size_t)k_b * 4, -9);
  r.best_a.assign((size_t)k_a * 2, -9);
  lk::MatchArgs m;
  if (lk::check_match(r.pairs.data(), r.totals.data(), cap, table_a.data(), 12, table_b.data(), 12, k_a, k_b, track_a.data(), 1, 4, &next_in,
                      r.link.data(), r.best_a.data(), &r.next_out, m) != OCC4D_OK)
    return false;
  const int rows = lk::pair_rows(m);
  for (int64_t k = 0; k < std::max(k_a, k_b); ++k) lk::init_item(m, k);
  on_threads(threads, rows, [&](int64_t i) { lk::best_item<Atomic>(m, rows, (int)i); });
  for (int64_t b = 0; b < k_b; ++b) lk::resolve_item(m, rows, b);
  for (int64_t ka = 0; ka < k_a; ++ka) lk::finish_item(m, rows, ka);
  int32_t next = next_in;
  for (int64_t b = 0; b < k_b; ++b)
    if (lk::is_new(m, b)) lk::new_id(m, b, next++);
  r.next_out = next;
  return true;
}

static int run(const char* name, const std::vector<int32_t>& la, const std::vector<int32_t>& lb, int k_a, int k_b, int cap, int overflow) {
  Result one, many;
  if (!link_frames(la, lb, k_a, k_b, cap, 1, one) || !link_frames(la, lb, k_a, k_b, cap, THREADS, many)) return 1;
  const int bad = !(one == many) || one.totals[2] != overflow;
  printf("%-16s k_a %5d k_b %5d cap %5d: %5d pairs of %5d points, overflow %d, next id %d on %d threads, %d mismatches\n", name, k_a, k_b,
         cap, many.totals[0], many.totals[1], many.totals[2], many.next_out, THREADS, bad);
  return bad;
}

int main() {
  std::vector<int32_t> stripes_a(N), stripes_b(N), solid(N, 0), foreign(N);
  for (int p = 0; p < N; ++p) {
    stripes_a[p] = p % 11 == 0 ? -1 : (p / 37) % 50;
    stripes_b[p] = p % 7 == 0 ? 50 : ((p + 9) / 37) % 50;                    // (50: outside [0, k_b); the stripes moved by 9 points)
    foreign[p] = p;
  }
  int failed = 0;
  failed += run("stripes", stripes_a, stripes_b, 50, 50, 2000, 0);
  failed += run("one pair", solid, solid, 1, 1, 1, 0);
  failed += run("foreign", foreign, foreign, N, N, N, 0);
  failed += run("foreign cap 1", foreign, foreign, N, N, 1, 1);
  if (failed) {
    printf("FAILED: %d runs differ from the result of one thread\n", failed);
    return 1;
  }
  printf("ok: every threaded overlap and match equals that of one thread\n");
  return 0;
}
