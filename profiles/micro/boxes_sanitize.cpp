// A stand-alone host program that drives the g++ twin's two boxes entry points (include/ext/occ4d_boxes.h), and with them the shared
// bodies of csrc/boxes_math.hpp, over grids of awkward shapes with buffers of EXACTLY the documented sizes, for a run under the host
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/boxes_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/boxes_sanitize && /tmp/boxes_sanitize
//
// Labels of arbitrary int32 values (foreign ones mixed in, K below the largest label), directions with coefficients up to the
// limit, beyond it and at the int32 extremes.  It checks what can be checked without a second implementation: the status; an extent
// row is EMPTY exactly where the object has no point or the direction is DEAD, and has min <= max elsewhere; the counts of zr sum
// to the number of labels in [0, K) and min iz <= max iz wherever the count is positive; box[k][0] lies in [-1, A) and never names a
// DEAD row; a row without points is [-1, 0, ...]; the kept columns equal zr.  A second choice over foreign extents (any int32
// values) only has to stay inside its buffers.  Prints "ok" and the number of calls.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_boxes.h"

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

static bool dead(const int32_t* row) {
  for (int c = 0; c < 4; ++c)
    if (row[c] < -OCC4D_BOXES_MAX_COEF || row[c] > OCC4D_BOXES_MAX_COEF) return true;
  return false;
}

// air: per mille of -1 labels;  strange: per mille of foreign values;  spread: labels are drawn from [0, spread)
static void run(int nx, int ny, int nz, int K, int A, int air, int strange, int spread, int dead_share) {
  const int64_t n = (int64_t)nx * ny * nz;
  std::vector<int32_t> labels((size_t)n), dirs((size_t)A * 4), extent((size_t)K * A * 4, 12345), zr((size_t)K * 3, 12345),
      box((size_t)K * OCC4D_BOXES_COLS, 12345);
  const int32_t foreign[] = {-1, -7, K, K + 5, INT32_MAX, INT32_MIN};
  int64_t in_range = 0;
  for (int64_t p = 0; p < n; ++p) {
    const int dice = (int)(rnd() % 1000);
    labels[(size_t)p] = dice < air ? -1 : dice < air + strange ? foreign[rnd() % 6] : (int32_t)(rnd() % (uint32_t)spread);
    in_range += labels[(size_t)p] >= 0 && labels[(size_t)p] < K;
  }
  const int32_t bad[] = {32769, -32769, INT32_MAX, INT32_MIN};
  for (int a = 0; a < A; ++a) {
    for (int c = 0; c < 4; ++c) {
      const uint32_t kind = rnd() % 8;
      dirs[(size_t)a * 4 + c] = kind == 0 ? OCC4D_BOXES_MAX_COEF : kind == 1 ? -OCC4D_BOXES_MAX_COEF
                                                                              : (int32_t)(rnd() % 65537u) - OCC4D_BOXES_MAX_COEF;
    }
    if ((int)(rnd() % 1000) < dead_share) dirs[(size_t)a * 4 + rnd() % 4] = bad[rnd() % 4];
  }
  const auto ptr = [](std::vector<int32_t>& v) { return v.empty() ? nullptr : v.data(); };
  CHECK(occ4d_boxes_extents_i32(ptr(labels), nx, ny, nz, K, dirs.data(), A, ptr(extent), ptr(zr), nullptr) == OCC4D_OK);
  CHECK(occ4d_boxes_choose_i32(ptr(extent), ptr(zr), dirs.data(), K, A, ptr(box), nullptr) == OCC4D_OK);
  calls += 2;
  int64_t counted = 0;
  for (int k = 0; k < K; ++k) {
    const int32_t* z = &zr[(size_t)k * 3];
    const int32_t* b = &box[(size_t)k * OCC4D_BOXES_COLS];
    CHECK(z[2] >= 0);
    counted += z[2];
    if (z[2] == 0) CHECK(z[0] == INT32_MAX && z[1] == INT32_MIN);
    else CHECK(0 <= z[0] && z[0] <= z[1] && z[1] < nz);
    bool any_live = false;
    for (int a = 0; a < A; ++a) {
      const int32_t* e = &extent[((size_t)k * A + a) * 4];
      const bool empty = e[0] == INT32_MAX && e[1] == INT32_MIN && e[2] == INT32_MAX && e[3] == INT32_MIN;
      CHECK(empty == (z[2] == 0 || dead(&dirs[(size_t)a * 4])));
      if (!empty) CHECK(e[0] <= e[1] && e[2] <= e[3]);
      any_live = any_live || !dead(&dirs[(size_t)a * 4]);
    }
    CHECK(b[0] >= -1 && b[0] < A);
    if (b[0] >= 0) CHECK(!dead(&dirs[(size_t)b[0] * 4]) && z[2] > 0);
    if (z[2] == 0) {
      for (int c = 0; c < OCC4D_BOXES_COLS; ++c) CHECK(b[c] == (c == 0 ? -1 : 0));
    } else {
      CHECK((b[0] >= 0) == any_live && b[5] == z[0] && b[6] == z[1] && b[7] == z[2]);
      if (b[0] >= 0)
        for (int c = 0; c < 4; ++c) CHECK(b[1 + c] == extent[((size_t)k * A + b[0]) * 4 + c]);
    }
  }
  CHECK(counted == in_range);
  // foreign extents and ranges: any int32 values; the choice reads them and writes box only
  for (auto& v : extent) v = rnd() % 4 == 0 ? (rnd() % 2 ? INT32_MAX : INT32_MIN) : (int32_t)rnd();
  for (auto& v : zr) v = (int32_t)rnd();
  CHECK(occ4d_boxes_choose_i32(ptr(extent), ptr(zr), dirs.data(), K, A, ptr(box), nullptr) == OCC4D_OK);
  ++calls;
  for (int k = 0; k < K; ++k) {
    const int32_t a = box[(size_t)k * OCC4D_BOXES_COLS];
    CHECK(a >= -1 && a < A && (a < 0 || !dead(&dirs[(size_t)a * 4])));
  }
}

int main() {
  const int grids[][3] = {{1, 1, 1}, {1, 1, 5}, {5, 1, 1}, {3, 2, 5}, {7, 9, 4}, {20, 19, 3}, {2, 3, 131}, {0, 4, 4}, {17, 1, 66}, {12, 12, 2}};
  const int dirs[] = {1, 2, 63, 64, 65, 90, 256};
  for (const auto& g : grids)
    for (const int A : dirs)
      for (int variant = 0; variant < 4; ++variant) {
        const int K = variant == 0 ? 0 : variant == 1 ? 1 : variant == 2 ? 7 : 150;
        run(g[0], g[1], g[2], K, A, variant == 1 ? 0 : 300, variant == 2 ? 300 : 0, variant == 2 ? 12 : K + 1, variant == 3 ? 1000 : 200);
      }
  run(2048, 1, 1, 2, 4, 100, 100, 2, 0);
  run(1, 2048, 1, 2, 4, 100, 100, 2, 0);
  run(1, 1, 2048, 2, 4, 100, 100, 2, 500);
  // the rejected calls leave their buffers alone
  int32_t one[8] = {0};
  CHECK(occ4d_boxes_extents_i32(one, 1, 1, 1, 1, one, 0, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_boxes_extents_i32(one, 2049, 1, 1, 1, one, 1, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_boxes_choose_i32(one, one, one, -1, 1, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_boxes_choose_i32(nullptr, nullptr, nullptr, 0, 1, nullptr, nullptr) == OCC4D_OK);
  std::printf("ok: %d calls\n", calls);
  return 0;
}
