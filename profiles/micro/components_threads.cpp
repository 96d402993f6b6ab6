// Host concurrency check of the border merge of the connected components (csrc/components_math.hpp): find and unite with the atomics
// spelled as relaxed std::atomic_ref operations, run on 16 std::threads under ThreadSanitizer.  No GPU, no Python.
//
//   g++ -std=c++20 -O1 -g -fsanitize=thread -pthread -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/components_threads.cpp \
//       -o components_threads && ./components_threads
//
// Per field of the (40, 24, 20) grid -- the serpentine, the comb and a random field of density 0.31, at every connectivity -- : pass 1
// (the tile-local labelling) runs on one thread; the pairs that straddle a tile border are listed in the order of the border pass
// and dealt round-robin to 16 threads, each calling unite on the shared parent array; the flattened roots are compared with those of
// the sequential border pass, and every root must be the lowest index of its component.  Then, for more contention than the border
// pass ever sees, the same without the local pass: every member its own root and ALL adjacent pairs on the threads.  Exits non-zero
// on a mismatch (or when ThreadSanitizer reports a race).
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "components_math.hpp"

void occ4d::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

namespace cc = occ4d_components;

struct Atomic {
  static int load(const int32_t* p) { return std::atomic_ref<int32_t>(*const_cast<int32_t*>(p)).load(std::memory_order_relaxed); }
  static int fetch_min(int32_t* p, int v) {                                 // (std::atomic has no fetch_min before C++26)
    std::atomic_ref<int32_t> ref(*p);
    int32_t before = ref.load(std::memory_order_relaxed);
    while (v < before && !ref.compare_exchange_weak(before, v, std::memory_order_relaxed, std::memory_order_relaxed)) {
    }
    return before;
  }
};

constexpr int NX = 40, NY = 24, NZ = 20, N = NX * NY * NZ, THREADS = 16;

static int at(int x, int y, int z) { return (x * NY + y) * NZ + z; }

static std::vector<float> serpentine() {
  std::vector<float> f(N, 0.f);
  std::vector<std::pair<int, int>> lines;
  for (int xi = 0, x = 0; x < NX; x += 2, ++xi)
    for (int k = 0; k < NY / 2; ++k) lines.push_back({x, xi % 2 == 0 ? 2 * k : NY - 2 - 2 * k});
  for (size_t i = 0; i < lines.size(); ++i) {
    for (int z = 0; z < NZ; ++z) f[at(lines[i].first, lines[i].second, z)] = 1.f;
    if (i + 1 < lines.size())
      f[at((lines[i].first + lines[i + 1].first) / 2, (lines[i].second + lines[i + 1].second) / 2, i % 2 == 0 ? NZ - 1 : 0)] = 1.f;
  }
  return f;
}

static std::vector<float> comb() {
  std::vector<float> f(N, 0.f);
  for (int z : {1, 8, 15}) {
    for (int x = 0; x < NX - 1; ++x)
      for (int y = 0; y < NY; y += 2) f[at(x, y, z)] = 1.f;
    for (int y = 0; y < NY; ++y) f[at(NX - 1, y, z)] = 1.f;
  }
  for (int z = 0; z < NZ; ++z) f[at(NX - 1, NY - 1, z)] = 1.f;
  return f;
}

static std::vector<float> random_field() {
  std::mt19937 gen(12);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  std::vector<float> f(N);
  for (float& v : f) v = u(gen) < 0.31f ? 1.f : 0.f;
  return f;
}

static int run(const char* name, const std::vector<float>& field, int connectivity) {
  std::vector<int32_t> work(3 * N + 3 * ((N + cc::TILE - 1) / cc::TILE)), labels(N), totals(3);
  cc::LabelArgs a;
  bool empty;
  if (cc::check_label(field.data(), 1, 0.5f, nullptr, 0, 0.f, nullptr, NX, NY, NZ, connectivity, 1, work.data(), labels.data(),
                      totals.data(), empty, a) != OCC4D_OK)
    return 1;
  int32_t s_parent[256], s_key[256];
  for (int64_t tile = 0; tile < a.grid.local_tiles; ++tile) {
    for (int t = 0; t < 256; ++t) cc::local_init(a, cc::local_point(a.grid, tile, t), t, s_parent, s_key);
    for (int t = 0; t < 256; ++t) cc::local_link<cc::Plain>(a, cc::local_point(a.grid, tile, t), t, s_parent, s_key);
    for (int t = 0; t < 256; ++t) cc::local_write<cc::Plain>(a, a.grid, tile, cc::local_point(a.grid, tile, t), t, s_parent);
  }
  const std::vector<int32_t> local(a.parent, a.parent + N);
  std::vector<std::pair<int, int>> pairs;
  for (int64_t p = 0; p < N; ++p) cc::border_pairs<cc::Plain>(a, p, [&pairs](int x, int y) { pairs.push_back({x, y}); });

  // the sequential border pass, flattened
  for (int64_t p = 0; p < N; ++p) cc::border_item<cc::Plain>(a, p);
  std::vector<int32_t> want(N);
  for (int64_t p = 0; p < N; ++p) want[p] = cc::flatten_item(a, p);

  // 16 threads, the pairs dealt round-robin
  std::copy(local.begin(), local.end(), a.parent);
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
      pool.emplace_back([&, t] {
        for (size_t i = t; i < pairs.size(); i += THREADS) cc::unite<Atomic>(a.parent, pairs[i].first, pairs[i].second);
      });
    for (std::thread& th : pool) th.join();
  }
  int bad = 0, roots = 0;
  for (int64_t p = 0; p < N; ++p) {
    const int r = cc::flatten_item(a, p);
    bad += r != want[p] || r > p;
    roots += r == p;
  }

  // more contention than the border pass ever sees: no local pass, every member its own root, ALL adjacent pairs on the threads
  std::vector<std::pair<int, int>> all;
  for (int64_t p = 0; p < N; ++p) {
    a.parent[p] = local[p] < 0 ? -1 : (int32_t)p;
    int i[3], d[3];
    cc::coords_of(a.grid, p, i);
    for (int c = 0; c < cc::BACKWARD && local[p] >= 0; ++c) {
      if (!cc::backward_offset(c, a.rank, d)) continue;
      const int j[3] = {i[0] + d[0], i[1] + d[1], i[2] + d[2]};
      if (j[0] < 0 || j[1] < 0 || j[2] < 0 || j[1] >= NY || j[2] >= NZ || local[at(j[0], j[1], j[2])] < 0) continue;
      all.push_back({(int)p, at(j[0], j[1], j[2])});
    }
  }
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
      pool.emplace_back([&, t] {
        for (size_t i = t; i < all.size(); i += THREADS) cc::unite<Atomic>(a.parent, all[i].first, all[i].second);
      });
    for (std::thread& th : pool) th.join();
  }
  int bad_all = 0;
  for (int64_t p = 0; p < N; ++p) bad_all += cc::flatten_item(a, p) != want[p];
  printf("%-12s connectivity %2d: %5zu border pairs / %6zu pairs in all on %d threads, %5d components, %d / %d mismatches\n", name,
         connectivity, pairs.size(), all.size(), THREADS, roots, bad, bad_all);
  return bad != 0 || bad_all != 0;
}

int main() {
  int failed = 0;
  for (int connectivity : {6, 18, 26}) {
    failed += run("serpentine", serpentine(), connectivity);
    failed += run("comb", comb(), connectivity);
    failed += run("random 0.31", random_field(), connectivity);
  }
  if (failed) {
    printf("FAILED: %d runs differ from the sequential result\n", failed);
    return 1;
  }
  printf("ok: every threaded border merge equals the sequential one\n");
  return 0;
}
