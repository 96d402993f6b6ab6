// A stand-alone host program that drives the g++ twin's two watershed entry points (include/ext/occ4d_watershed.h) and the
// components table over grids of awkward shapes with buffers of EXACTLY the documented sizes, for a run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/watershed_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/watershed_sanitize && /tmp/watershed_sanitize
//
// It checks what can be checked without a second implementation: the status, labels in [-1, K), the totals against a count of the
// labels, every peak a point of its segment with the segment's largest height.  Prints "ok" and the number of calls.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_components.h"
#include "ext/occ4d_watershed.h"

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

static void run(const std::vector<int32_t>& height, int nx, int ny, int nz, int connectivity, int h, int min_size, int cap_delta) {
  const int64_t n = (int64_t)nx * ny * nz;
  const int64_t tiles = (n + OCC4D_WATERSHED_TILE - 1) / OCC4D_WATERSHED_TILE;
  std::vector<int32_t> work(4 * n + 4 * tiles + OCC4D_WATERSHED_ROUND_WORDS), labels(n), totals(OCC4D_WATERSHED_TOTALS, 0);
  CHECK(occ4d_watershed_label_i32(n ? height.data() : nullptr, nx, ny, nz, connectivity, h, min_size, work.data(), n ? labels.data() : nullptr,
                                  totals.data(), nullptr) == OCC4D_OK);
  ++calls;
  const int kept = totals[0];
  CHECK(kept >= 0 && totals[2] >= kept && totals[3] >= totals[2] && totals[1] <= n);
  std::vector<int64_t> size(kept, 0);
  int64_t members = 0;
  for (int64_t p = 0; p < n; ++p) {
    CHECK(labels[p] >= -1 && labels[p] < kept);
    CHECK(labels[p] < 0 || height[p] >= 1);
    if (labels[p] >= 0) ++size[labels[p]], ++members;
  }
  CHECK(members == totals[1]);
  for (int k = 0; k < kept; ++k) CHECK(size[k] >= min_size);
  const int cap = kept + cap_delta < 0 ? 0 : kept + cap_delta;
  const int rows = cap < kept ? cap : kept;
  std::vector<int64_t> table((size_t)cap * OCC4D_COMPONENTS_COLS);
  std::vector<int64_t> peaks_words(cap);                                   // (cap, 2) int32, aligned to 8 bytes
  int32_t* peaks = reinterpret_cast<int32_t*>(peaks_words.data());
  CHECK(occ4d_components_table_i64(labels.data(), nullptr, nx, ny, nz, totals.data(), table.data(), cap, nullptr) == OCC4D_OK);
  CHECK(occ4d_watershed_peaks_i32(height.data(), labels.data(), (int)n, totals.data(), peaks, cap, nullptr) == OCC4D_OK);
  for (int k = 0; k < rows; ++k) {
    const int32_t at = peaks[2 * k], top = peaks[2 * k + 1];
    CHECK(at >= 0 && at < n && labels[at] == k && height[at] == top && table[(size_t)k * OCC4D_COMPONENTS_COLS] == size[k]);
    for (int64_t p = 0; p < n; ++p)
      if (labels[p] == k) CHECK(height[p] < top || (height[p] == top && p >= at));
  }
}

int main() {
  const int shapes[][3] = {{9, 10, 11}, {17, 8, 9}, {16, 16, 16}, {1, 1, 30}, {30, 1, 1}, {1, 7, 1}, {1, 1, 1}, {0, 5, 5}, {33, 2, 5}};
  const int connectivities[] = {6, 18, 26};
  for (const auto& s : shapes) {
    const int64_t n = (int64_t)s[0] * s[1] * s[2];
    std::vector<int32_t> random(n), plateau(n, INT32_MAX), mixed(n);
    for (int64_t p = 0; p < n; ++p) {
      random[p] = rnd() % 5 == 0 ? -(int32_t)(rnd() % 3) : 1 + (int32_t)(rnd() % 3);
      mixed[p] = rnd() % 4 == 0 ? INT32_MIN + (int32_t)(rnd() % 2) : (rnd() % 2 ? INT32_MAX : 1);
    }
    for (int connectivity : connectivities)
      for (int h : {0, 1, 2, INT32_MAX})
        for (int min_size : {1, 5}) {
          run(random, s[0], s[1], s[2], connectivity, h, min_size, h == 1 ? -2 : h == 2 ? 3 : 0);
          run(mixed, s[0], s[1], s[2], connectivity, h, min_size, 0);
        }
    run(plateau, s[0], s[1], s[2], 26, 0, 1, 0);
    run(plateau, s[0], s[1], s[2], 6, 0, 1, 1);
  }
  // rejected calls leave a message and touch nothing
  CHECK(occ4d_watershed_label_i32(nullptr, 2, 2, 2, 26, -1, 1, nullptr, nullptr, nullptr, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_watershed_peaks_i32(nullptr, nullptr, 8, nullptr, nullptr, -1, nullptr) == OCC4D_EINVAL);
  std::printf("ok %d calls\n", calls);
  return 0;
}
