// A stand-alone host program that drives the g++ twin's two viewplan entry points (include/ext/occ4d_viewplan.h), and with them the
// shared bodies of csrc/viewplan_math.hpp over csrc/sight_math.hpp, over grids of awkward shapes with buffers of EXACTLY the
// documented sizes, for a run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/viewplan_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/viewplan_sanitize && /tmp/viewplan_sanitize
//
// It checks what can be checked without a second implementation: the status; vis & ~targets == 0 and the unused bits of every row's
// last word; a candidate beyond 2^20 or in a solid cell sees nothing; on an all-free grid without a range limit every live candidate
// sees every target; with max_dist2 = 0 a candidate sees at most its own cell; gain = the popcount of the row; picks in [-1, C), none
// twice, -1 only behind the last pick; pick_gain never increasing; status[0] = popcount(targets), status[0] - status[1] = the sum of
// pick_gain = the popcount of the union of the picked rows.  Candidates of arbitrary int32 values.  Prints "ok" and the number of calls.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_viewplan.h"

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

// share, target_share: per mille of solid points and of target points;  max_dist2 < 0: no limit
static void run(int nx, int ny, int nz, int share, int target_share, int C, int k, int64_t max_dist2, int wx, int wy, int wz) {
  const int64_t n = (int64_t)nx * ny * nz, W = (n + 31) / 32;
  std::vector<uint32_t> solid(W, 0), targets(W, 0), vis((size_t)C * W, 0xdeadbeefu);
  for (int64_t p = 0; p < n; ++p) {
    if ((int)(rnd() % 1000) < share) solid[p >> 5] |= 1u << (p & 31);
    if ((int)(rnd() % 1000) < target_share) targets[p >> 5] |= 1u << (p & 31);
  }
  std::vector<int32_t> cand((size_t)C * 3);
  for (int c = 0; c < C; ++c)
    for (int a = 0; a < 3; ++a) {
      const int len = a == 0 ? nx : a == 1 ? ny : nz;
      const uint32_t kind = rnd() % 8;
      cand[3 * c + a] = kind == 0 ? (int32_t)rnd()                                              // any value: mostly beyond 2^20
                      : kind == 1 ? (rnd() % 2 ? 1048576 : -1048576)
                      : kind == 2 ? (int32_t)(rnd() % (uint32_t)(len + 7)) - 3                  // round the grid
                                  : (int32_t)(rnd() % (uint32_t)(len > 0 ? len : 1));           // inside
    }
  const auto u = [](std::vector<uint32_t>& v) { return v.empty() ? nullptr : v.data(); };
  const auto i = [](std::vector<int32_t>& v) { return v.empty() ? nullptr : v.data(); };
  CHECK(occ4d_viewplan_visible_u32(u(solid), nx, ny, nz, u(targets), i(cand), C, wx, wy, wz, max_dist2, u(vis), nullptr) == OCC4D_OK);
  ++calls;
  const auto bit = [](const uint32_t* words, int64_t p) { return (words[p >> 5] >> (p & 31)) & 1u; };
  for (int c = 0; c < C && n; ++c) {
    const uint32_t* row = vis.data() + (size_t)c * W;
    const int32_t x = cand[3 * c], y = cand[3 * c + 1], z = cand[3 * c + 2];
    const bool far = x < -1048576 || x > 1048576 || y < -1048576 || y > 1048576 || z < -1048576 || z > 1048576;
    const bool inside = !far && x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz;
    const int64_t at = inside ? ((int64_t)x * ny + y) * nz + z : -1;
    const bool dead = far || (inside && bit(solid.data(), at));
    for (int64_t w = 0; w < W; ++w) {
      CHECK((row[w] & ~targets[w]) == 0);
      if (dead) CHECK(row[w] == 0);
      if (!dead && share == 0 && max_dist2 < 0) CHECK(row[w] == targets[w]);
      if (max_dist2 == 0) CHECK(row[w] == (inside && !dead && (at >> 5) == w ? targets[w] & (1u << (at & 31)) : 0u));
    }
    if (n % 32) CHECK((row[W - 1] >> (n % 32)) == 0);
  }

  std::vector<int32_t> work((size_t)(W + C + 2)), gain(C, 12345), picks(k, 12345), pick_gain(k, 12345), status(2, 12345);
  CHECK(occ4d_viewplan_greedy_u32(u(vis), C, W, u(targets), k, n && C ? work.data() : nullptr, i(gain), i(picks), i(pick_gain), status.data(),
                                  nullptr) == OCC4D_OK);
  ++calls;
  if (n == 0 || C == 0) return;
  int64_t total = 0, covered = 0, sum = 0;
  std::vector<uint32_t> join(W, 0);
  for (int64_t w = 0; w < W; ++w) total += __builtin_popcount(targets[w]);
  for (int c = 0; c < C; ++c) {
    int64_t mine = 0;
    for (int64_t w = 0; w < W; ++w) mine += __builtin_popcount(vis[(size_t)c * W + w]);
    CHECK(gain[c] == mine);
  }
  std::vector<char> taken(C, 0);
  for (int r = 0; r < k; ++r) {
    CHECK(picks[r] >= -1 && picks[r] < C && pick_gain[r] >= 0);
    CHECK(r == 0 || pick_gain[r] <= pick_gain[r - 1]);
    CHECK(r == 0 || picks[r - 1] >= 0 || picks[r] == -1);
    CHECK((picks[r] == -1) == (pick_gain[r] == 0));
    if (picks[r] < 0) continue;
    CHECK(!taken[picks[r]]);
    taken[picks[r]] = 1;
    for (int64_t w = 0; w < W; ++w) join[w] |= vis[(size_t)picks[r] * W + w];
    sum += pick_gain[r];
  }
  for (int64_t w = 0; w < W; ++w) covered += __builtin_popcount(join[w]);
  CHECK(status[0] == total && status[0] - status[1] == sum && sum == covered);
  if (k > 0 && picks[k - 1] == -1)
    for (int c = 0; c < C; ++c)                                    // nothing is left that any candidate sees
      for (int64_t w = 0; w < W; ++w) CHECK((vis[(size_t)c * W + w] & ~join[w]) == 0);
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 70}, {5, 1, 4}, {3, 2, 5}, {6, 7, 5}, {17, 9, 33}, {0, 5, 5}, {33, 2, 5}, {1, 512, 1}};
  for (const auto& s : shapes)
    for (int share : {0, 100, 450, 1000})
      for (int target_share : {0, 400, 1000}) {
        run(s[0], s[1], s[2], share, target_share, 1, 1, -1, 1, 1, 1);
        run(s[0], s[1], s[2], share, target_share, 3, 0, -1, 1, 1, 1);
        run(s[0], s[1], s[2], share, target_share, 65, 4, 0, 3, 1, 2);
        run(s[0], s[1], s[2], share, target_share, 130, 32, 40, 3, 1, 2);
        run(s[0], s[1], s[2], share, target_share, 0, 2, 9, 1, 1024, 1);
      }
  // rejected calls leave a message and touch nothing
  uint32_t word = 0;
  int32_t one[8] = {0};
  CHECK(occ4d_viewplan_visible_u32(&word, 513, 1, 1, &word, one, 1, 1, 1, 1, -1, &word, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_viewplan_visible_u32(&word, 2, 2, 2, &word, nullptr, 1, 1, 1, 1, -1, &word, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_viewplan_visible_u32(&word, 2, 2, 2, &word, one, 4097, 1, 1, 1, -1, &word, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_viewplan_visible_u32(&word, 2, 2, 2, &word, one, 1, 1, 0, 1, -1, &word, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_viewplan_greedy_u32(&word, 1, 1, &word, 33, one, one, one, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_viewplan_greedy_u32(&word, 1, 1, &word, 1, nullptr, one, one, one, one, nullptr) == OCC4D_EINVAL);
  std::printf("ok %d calls\n", calls);
  return 0;
}
