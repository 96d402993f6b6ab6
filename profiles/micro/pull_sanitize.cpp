// A stand-alone host program that drives the g++ twin's three pull entry points (include/ext/occ4d_pull.h) over grids of awkward
// shapes with buffers of EXACTLY the documented sizes, for a run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/pull_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/pull_sanitize && /tmp/pull_sanitize
//
// It checks what can be checked without a second implementation: the status, the packed bits against the blocked test, the unused
// bits of the last word, every hit within [-2, n) and >= 0 only at a blocked cell, -2 exactly for an index outside, FREE symmetric,
// every pair free on an all-free grid; the waypoints a subsequence of the chain from its first to its last point with -1 behind
// them, lengths that pass through, chains of arbitrary values.  Prints "ok" and the number of calls.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_geodesic.h"
#include "ext/occ4d_pull.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (uint32_t)(state >> 32);
}

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, occ4d_last_error()); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

static int calls = 0;

// share: per mille of blocked points;  min_clear: the cut of a clearance with the values 0 .. 2 * min_clear (or 0 / 1)
static void run(int nx, int ny, int nz, int share, int min_clear, int n_pairs, int n_goals, int cap) {
  const int64_t n = (int64_t)nx * ny * nz, words = (n + 31) / 32;
  std::vector<int32_t> clear(n);
  for (auto& v : clear) v = (int)(rnd() % 1000) < share ? min_clear - 1 - (int)(rnd() % 3) : min_clear + (int)(rnd() % 3);
  std::vector<uint32_t> blocked(words);
  CHECK(occ4d_pull_bits_i32(n ? clear.data() : nullptr, min_clear, n, n ? blocked.data() : nullptr, nullptr) == OCC4D_OK);
  ++calls;
  for (int64_t p = 0; p < n; ++p) CHECK(((blocked[p >> 5] >> (p & 31)) & 1u) == (uint32_t)!(clear[p] >= min_clear));
  if (n % 32) CHECK((blocked[words - 1] >> (n % 32)) == 0);

  std::vector<int32_t> a(n_pairs), b(n_pairs), hit(n_pairs), back(n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    a[i] = i % 7 == 0 ? (int32_t)rnd() : (int32_t)(rnd() % (uint32_t)(n + 2)) - 1;      // -1 and n among them, any value now and then
    b[i] = i % 11 == 0 ? a[i] : (int32_t)(rnd() % (uint32_t)(n + 2)) - 1;
  }
  const auto ptr = [](std::vector<int32_t>& v) { return v.empty() ? nullptr : v.data(); };
  CHECK(occ4d_pull_pairs_u32(n ? blocked.data() : nullptr, nx, ny, nz, ptr(a), ptr(b), n_pairs, ptr(hit), nullptr) == OCC4D_OK);
  CHECK(occ4d_pull_pairs_u32(n ? blocked.data() : nullptr, nx, ny, nz, ptr(b), ptr(a), n_pairs, ptr(back), nullptr) == OCC4D_OK);
  calls += 2;
  for (int i = 0; i < n_pairs; ++i) {
    const bool outside = a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n;
    CHECK((hit[i] == -2) == outside && hit[i] >= -2 && hit[i] < n);
    CHECK(hit[i] < 0 || !(clear[hit[i]] >= min_clear));
    CHECK((hit[i] == -1) == (back[i] == -1));
    if (share == 0 && !outside) CHECK(hit[i] == -1);
  }

  // chains: the library's own trace from a seed in the first corner, then rows of arbitrary values and lengths
  std::vector<int32_t> cost(n), parent(n), status(2), work(65), seeds(1, 0), goals(n_goals);
  std::vector<int32_t> paths((size_t)n_goals * cap), path_len(n_goals), way((size_t)n_goals * cap), way_len(n_goals);
  for (auto& g : goals) g = (int32_t)(rnd() % (uint32_t)(n + 2)) - 1;
  if (n) {
    CHECK(occ4d_geodesic_grid_i32(clear.data(), min_clear, nx, ny, nz, seeds.data(), 1, 26, 3, 4, 5, 64, 0, work.data(), cost.data(),
                                  parent.data(), status.data(), nullptr) == OCC4D_OK);
    CHECK(occ4d_geodesic_trace_i32(cost.data(), parent.data(), (int)n, ptr(goals), n_goals, cap, ptr(paths), ptr(path_len), nullptr) == OCC4D_OK);
  }
  for (int round = 0; round < 2; ++round) {
    if (round == 1) {
      for (auto& v : paths) v = rnd() % 5 == 0 ? (int32_t)rnd() : (int32_t)(rnd() % (uint32_t)(n + 2)) - 1;
      for (auto& v : path_len) v = rnd() % 4 == 0 ? (int32_t)rnd() : (int32_t)(rnd() % (uint32_t)(cap + 3)) - 1;
    }
    for (auto& v : way) v = 12345;
    for (auto& v : way_len) v = 12345;
    CHECK(occ4d_pull_paths_i32(n ? blocked.data() : nullptr, nx, ny, nz, ptr(paths), ptr(path_len), n_goals, cap, ptr(way), ptr(way_len),
                               nullptr) == OCC4D_OK);
    ++calls;
    for (int g = 0; n && g < n_goals; ++g) {
      const int32_t L = path_len[g], W = way_len[g];
      const int32_t *row = paths.data() + (size_t)g * cap, *out = way.data() + (size_t)g * cap;
      if (L <= 0 || L > cap) {
        CHECK(W == L);
        for (int k = 0; k < cap; ++k) CHECK(out[k] == -1);
        continue;
      }
      CHECK(W >= 1 && W <= L && out[0] == row[0] && out[W - 1] == row[L - 1]);
      int at = 0;
      for (int k = 1; k < W; ++k) {                                // a subsequence: by position, the values may repeat in round 1
        ++at;
        while (at < L && row[at] != out[k]) ++at;
        CHECK(at < L);
      }
      for (int k = W; k < cap; ++k) CHECK(out[k] == -1);
      if (share == 0 && round == 0) CHECK(W <= 2);                 // nothing blocked: the goal sees the seed
    }
  }
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 70}, {5, 1, 4}, {3, 2, 5}, {6, 7, 5}, {17, 9, 33}, {0, 5, 5}, {33, 2, 5}, {1, 512, 1}};
  for (const auto& s : shapes)
    for (int share : {0, 100, 300, 1000})
      for (int min_clear : {1, 4}) {
        run(s[0], s[1], s[2], share, min_clear, 257, 5, 40);
        run(s[0], s[1], s[2], share, min_clear, 0, 0, 7);
        run(s[0], s[1], s[2], share, min_clear, 64, 3, 0);
        run(s[0], s[1], s[2], share, min_clear, 1, 2, 600);        // chains over more than two rounds of 256 candidates
      }
  // rejected calls leave a message and touch nothing
  uint32_t word = 0;
  int32_t one = 0;
  CHECK(occ4d_pull_bits_i32(nullptr, 1, 8, &word, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_pull_pairs_u32(&word, 513, 1, 1, &one, &one, 1, &one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_pull_pairs_u32(&word, 2, 2, 2, &one, nullptr, 1, &one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_pull_paths_i32(&word, 2, 2, 2, nullptr, &one, 1, 4, &one, &one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_pull_paths_i32(&word, 2, 2, 2, &one, &one, -1, 4, &one, &one, nullptr) == OCC4D_EINVAL);
  std::printf("ok %d calls\n", calls);
  return 0;
}
