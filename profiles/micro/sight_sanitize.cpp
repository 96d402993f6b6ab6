// A stand-alone host program that drives the g++ twin's two sight entry points (include/ext/occ4d_sight.h) over grids of awkward
// shapes with buffers of EXACTLY the documented sizes, for a run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/sight_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/sight_sanitize && /tmp/sight_sanitize
//
// It checks what can be checked without a second implementation: the status, the packed bits against the member test, the unused
// bits of the last word, seen within framed and within the V low bits, every blocker a solid cell of the grid and -1 exactly where
// the query is seen or not framed, an empty solid set hiding nothing.  Prints "ok" and the number of calls.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_sight.h"

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

// share: per mille of solid points;  ld: the stride of the field column;  with_mask: a second column;  V origins round the grid
static void run(int nx, int ny, int nz, int share, int ld, bool with_mask, int V, bool with_framed, bool with_blocker, int flags) {
  const int64_t n = (int64_t)nx * ny * nz, words = (n + 31) / 32;
  std::vector<float> field((size_t)n * ld), mask(with_mask ? (size_t)n * 2 : 0);
  for (auto& v : field) v = rnd() % 17 == 0 ? NAN : (float)(rnd() % 1000) / 1000.f;
  for (auto& v : mask) v = (float)(rnd() % 1000) / 1000.f;
  const float level = 1.f - (float)share / 1000.f;
  std::vector<uint32_t> bits(words);
  CHECK(occ4d_sight_bits_f32(n ? field.data() : nullptr, ld, level, with_mask && n ? mask.data() + 1 : nullptr, 2, 0.25f, n,
                             n ? bits.data() : nullptr, nullptr) == OCC4D_OK);
  ++calls;
  std::vector<char> solid(n);
  for (int64_t p = 0; p < n; ++p) {
    solid[p] = field[p * ld] >= level && (!with_mask || mask[p * 2 + 1] >= 0.25f);
    CHECK(((bits[p >> 5] >> (p & 31)) & 1u) == (uint32_t)solid[p]);
  }
  if (n % 32) CHECK((bits[words - 1] >> (n % 32)) == 0);
  std::vector<int32_t> origins((size_t)V * 3), framed(with_framed ? n : 0), seen(n), blocker(with_blocker ? (size_t)V * n : 0);
  const int dims[3] = {nx, ny, nz};
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k) {
      const int kind = (v + k) % 4;
      origins[v * 3 + k] = kind == 0 ? (int)(rnd() % (dims[k] + 1)) : kind == 1 ? -1 - (int)(rnd() % 3)
                           : kind == 2 ? dims[k] + (int)(rnd() % 3) : (rnd() % 2 ? OCC4D_SIGHT_MAX_COORD : -OCC4D_SIGHT_MAX_COORD);
    }
  for (auto& f : framed) f = (int32_t)rnd();
  CHECK(occ4d_sight_grid_u32(n ? bits.data() : nullptr, nx, ny, nz, n ? origins.data() : nullptr, V, with_framed && n ? framed.data() : nullptr,
                             n ? seen.data() : nullptr, with_blocker && n ? blocker.data() : nullptr, flags, nullptr) == OCC4D_OK);
  ++calls;
  for (int64_t p = 0; p < n; ++p) {
    const int32_t fr = with_framed ? framed[p] : -1;
    CHECK((seen[p] & ~fr) == 0 && (V == 31 || (seen[p] >> V) == 0) && seen[p] >= 0);
    if (share == 0) CHECK(seen[p] == (int32_t)(fr & (int32_t)((1u << V) - 1u)));          // nothing solid: nothing hidden
    for (int v = 0; with_blocker && v < V; ++v) {
      const int32_t b = blocker[(size_t)v * n + p];
      const bool is_seen = (seen[p] >> v) & 1, is_framed = (fr >> v) & 1;
      CHECK((b == -1) == (is_seen || !is_framed));
      CHECK(b == -1 || (b >= 0 && b < n && solid[b] && b != p));
    }
  }
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 70}, {5, 1, 1}, {3, 2, 5}, {9, 10, 11}, {17, 9, 33}, {0, 5, 5}, {33, 2, 5}, {1, 512, 1}};
  for (const auto& s : shapes)
    for (int share : {0, 100, 450, 1000})
      for (int V : {1, 3, 31}) {
        run(s[0], s[1], s[2], share, 1, false, V, false, true, 0);
        run(s[0], s[1], s[2], share, 3, true, V, true, true, 0);
        run(s[0], s[1], s[2], share, 2, false, V, true, false, 0);
      }
  // rejected calls leave a message and touch nothing
  int32_t far[3] = {0, OCC4D_SIGHT_MAX_COORD + 1, 0};
  uint32_t word = 0;
  int32_t one = 0;
  CHECK(occ4d_sight_grid_u32(&word, 1, 1, 1, far, 1, nullptr, &one, nullptr, 0, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_sight_grid_u32(nullptr, 2, 2, 2, nullptr, 32, nullptr, nullptr, nullptr, 0, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_sight_grid_u32(nullptr, 2, 2, 2, nullptr, 1, nullptr, nullptr, nullptr, 1, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_sight_bits_f32(nullptr, 0, 0.5f, nullptr, 0, 0.f, 8, nullptr, nullptr) == OCC4D_EINVAL);
  std::printf("ok %d calls\n", calls);
  return 0;
}
