// A stand-alone host program that drives the g++ twin's layers entry point (include/ext/occ4d_layers.h), and with it the shared
// bodies of csrc/layers_math.hpp, over a few hundred random small cases with buffers of EXACTLY the documented sizes, for a run
// under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/layers_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/layers_sanitize && /tmp/layers_sanitize
//
// Labels of arbitrary int32 values (out of range ones mixed in, K below the largest label, K = 0), cameras outside the grid, inside
// it, behind it and degenerate ones (zero and non-finite matrices), every output null in turn.  It checks what can be checked
// without a second implementation: the status; count in 0 .. L + 1; the stored layers are the first min(count, L) slots, distinct,
// with labels in [0, K), first strictly increasing, samples >= 1 and labels[point] == label; the unused slots hold -1 / 0; status
// counts the pixels; the table's AMODAL and VISIBLE columns are the counts of the per-pixel labels, its NEAR and box columns their
// minima and maxima, and the fill values where an object covers no pixel.  Prints "ok", the number of calls and how many pixels
// held an object and dropped one (neither may be 0).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_layers.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (uint32_t)(state >> 32);
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 100000) / 100000.0f; }

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, occ4d_last_error()); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

static int calls = 0;
static long long seen = 0, dropped = 0;                              // pixels with an object, pixels that dropped one
static const int32_t FILL[OCC4D_LAYERS_COLS] = {0, 0, INT32_MAX, INT32_MAX, -1, INT32_MAX, -1};

// The inverse matrices of a camera at `eye` whose axes are the world's, permuted by `turn`: k_inv = diag(1 / f, 1 / f, 1, 1) with
// the principal point taken off, rt_inv = the rotation and the eye.  kind 1: all zeros;  kind 2: a NaN and an infinity inside.
static void camera(float* k_inv, float* rt_inv, int W, int H, const float* eye, int turn, int kind) {
  for (int i = 0; i < 16; ++i) k_inv[i] = rt_inv[i] = 0.0f;
  if (kind == 1) return;
  const float f = uniform(2.0f, 30.0f);
  k_inv[0] = 1.0f / f, k_inv[2] = -0.5f * (float)(W - 1) / f, k_inv[5] = 1.0f / f, k_inv[6] = -0.5f * (float)(H - 1) / f;
  k_inv[10] = k_inv[15] = 1.0f;
  const float sign = (turn & 4) ? -1.0f : 1.0f;                     // looking along +axis or -axis
  const int axis = turn % 3;                                        // camera z = world axis `axis`
  rt_inv[4 * axis + 2] = sign, rt_inv[4 * ((axis + 1) % 3) + 0] = 1.0f, rt_inv[4 * ((axis + 2) % 3) + 1] = sign;
  for (int a = 0; a < 3; ++a) rt_inv[4 * a + 3] = eye[a];
  rt_inv[15] = 1.0f;
  if (kind == 2) rt_inv[rnd() % 12] = NAN, k_inv[rnd() % 12] = INFINITY;
}

static void run(int nx, int ny, int nz, int K, int V, int H, int W, int L, int n_steps, int air, int strange, int spread, unsigned nulls) {
  const int64_t n = (int64_t)nx * ny * nz, pixels = (int64_t)V * H * W;
  std::vector<int32_t> labels((size_t)n);
  const int32_t foreign[] = {-2, -7, K, K + 5, INT32_MAX, INT32_MIN};
  for (auto& v : labels) {
    const int dice = (int)(rnd() % 1000);
    v = dice < air ? -1 : dice < air + strange ? foreign[rnd() % 6] : (int32_t)(rnd() % (uint32_t)spread);
  }
  const float origin[3] = {uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f)};
  const float spacing[3] = {uniform(0.1f, 0.8f), uniform(0.1f, 0.8f), uniform(0.1f, 0.8f)};
  const float size[3] = {spacing[0] * (float)nx, spacing[1] * (float)ny, spacing[2] * (float)nz};
  std::vector<float> k_inv((size_t)V * 16 + 1), rt_inv((size_t)V * 16 + 1);
  for (int v = 0; v < V; ++v) {
    const int where = (int)(rnd() % 4);                              // 0: outside, looking in;  1: inside;  2: behind;  3: anywhere
    const int turn = (int)(rnd() % 8);
    float eye[3];
    for (int a = 0; a < 3; ++a) eye[a] = origin[a] + size[a] * (where == 1 ? uniform(0.2f, 0.8f) : where == 3 ? uniform(-2.0f, 3.0f) : 0.5f);
    if (where == 0 || where == 2) {
      const bool along = !(turn & 4);
      eye[turn % 3] = origin[turn % 3] + ((where == 0) == along ? -0.7f : 1.7f) * size[turn % 3];
    }
    camera(&k_inv[(size_t)v * 16], &rt_inv[(size_t)v * 16], W, H, eye, turn, rnd() % 16 == 0 ? 1 + (int)(rnd() % 2) : 0);
  }
  const float reach = std::sqrt(size[0] * size[0] + size[1] * size[1] + size[2] * size[2]);
  const float step = 2.5f * reach / (float)n_steps, near_depth = (rnd() % 4 == 0) ? -step : step;
  std::vector<int32_t> label((size_t)(pixels * L), 12345), first((size_t)(pixels * L), 12345), samples((size_t)(pixels * L), 12345),
      point((size_t)(pixels * L), 12345), count((size_t)pixels, 12345), table((size_t)V * K * OCC4D_LAYERS_COLS, 12345), status(2, 12345);
  std::vector<int32_t>* outs[7] = {&label, &first, &samples, &point, &count, &table, &status};
  int32_t* ptr[7];
  for (int o = 0; o < 7; ++o) ptr[o] = ((nulls >> o) & 1) || outs[o]->empty() ? nullptr : outs[o]->data();
  CHECK(occ4d_layers_march_i32(labels.data(), nx, ny, nz, K, origin[0], spacing[0], origin[1], spacing[1], origin[2], spacing[2],
                               k_inv.data(), rt_inv.data(), V, H, W, near_depth, step, n_steps, L, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4],
                               ptr[5], ptr[6], nullptr) == OCC4D_OK);
  ++calls;
  if (nulls != 0 || pixels == 0) return;                             // (what follows reads every array)
  std::vector<int32_t> want((size_t)V * K * OCC4D_LAYERS_COLS);
  for (size_t i = 0; i < want.size(); ++i) want[i] = FILL[i % OCC4D_LAYERS_COLS];
  int32_t over = 0, some = 0;
  for (int64_t pix = 0; pix < pixels; ++pix) {
    const int c = count[(size_t)pix];
    CHECK(c >= 0 && c <= L + 1);
    over += c == L + 1, some += c >= 1;
    const int stored = c < L ? c : L;
    const int v = (int)(pix / ((int64_t)H * W)), py = (int)(pix / W % H), px = (int)(pix % W);
    for (int j = 0; j < L; ++j) {
      const size_t e = (size_t)(pix * L + j);
      if (j >= stored) {
        CHECK(label[e] == -1 && first[e] == -1 && point[e] == -1 && samples[e] == 0);
        continue;
      }
      CHECK(label[e] >= 0 && label[e] < K && samples[e] >= 1 && first[e] >= 0 && first[e] < n_steps);
      CHECK(point[e] >= 0 && point[e] < n && labels[(size_t)point[e]] == label[e]);
      if (j > 0) CHECK(first[e] > first[e - 1]);
      for (int i = 0; i < j; ++i) CHECK(label[(size_t)(pix * L + i)] != label[e]);
      int32_t* row = &want[((size_t)v * K + label[e]) * OCC4D_LAYERS_COLS];
      row[0] += 1, row[1] += j == 0;
      row[2] = first[e] < row[2] ? first[e] : row[2];
      row[3] = px < row[3] ? px : row[3], row[4] = px > row[4] ? px : row[4];
      row[5] = py < row[5] ? py : row[5], row[6] = py > row[6] ? py : row[6];
    }
  }
  CHECK(status[0] == over && status[1] == some);
  seen += some, dropped += over;
  CHECK(table == want);
}

int main() {
  const int grids[][3] = {{2, 2, 2}, {3, 2, 5}, {5, 4, 2}, {12, 7, 9}, {9, 9, 9}};
  const int images[][2] = {{1, 1}, {5, 7}, {16, 16}, {9, 20}};
  for (int round = 0; round < 3; ++round)
    for (const auto& g : grids)
      for (const auto& im : images)
        for (int variant = 0; variant < 6; ++variant) {
          // 0: K = 0;  1: one object, no air;  2: out-of-range values mixed in, K below the largest label;  3: a label per draw
          // (overflow everywhere);  4: a few objects;  5: some outputs null
          const int K = variant == 0 ? 0 : variant == 1 ? 1 : variant == 2 ? 7 : variant == 3 ? 150 : 5;
          const int L = 1 + (int)(rnd() % OCC4D_LAYERS_MAX);
          run(g[0], g[1], g[2], K, 1 + (int)(rnd() % 3), im[0], im[1], variant == 3 ? 1 + (int)(rnd() % 2) : L,
              variant == 4 ? 1 + (int)(rnd() % 3) : 48, variant == 1 ? 0 : 300, variant == 2 ? 300 : 0, variant == 2 ? 12 : K + 1,
              variant == 5 ? 1u + rnd() % 126u : 0u);
        }
  run(3, 2, 5, 4, 0, 4, 4, 2, 8, 100, 100, 4, 0);                     // V == 0
  run(3, 2, 5, 4, 2, 0, 4, 2, 8, 100, 100, 4, 0);                     // H == 0
  run(3, 2, 5, 4, 2, 4, 4, 2, 8, 100, 100, 4, 127);                   // every output null
  // the rejected calls leave their buffers alone; the no-ops take null pointers
  int32_t one[8] = {0};
  float cam[16] = {0};
  CHECK(occ4d_layers_march_i32(one, 1, 2, 2, 1, 0, 1, 0, 1, 0, 1, cam, cam, 1, 1, 1, 0.1f, 0.1f, 1, 1, one, one, one, one, one, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_layers_march_i32(one, 2, 2, 2, 1, 0, 1, 0, 1, 0, 1, cam, cam, 1, 1, 1, 0.1f, 0.1f, 1, 9, one, one, one, one, one, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_layers_march_i32(one, 2, 2, 2, 1, 0, 1, 0, 1, 0, 1, cam, cam, 1, 1, 1, 0.1f, 0.0f, 1, 1, one, one, one, one, one, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_layers_march_i32(nullptr, 2, 2, 2, 1, 0, 1, 0, 1, 0, 1, cam, cam, 1, 1, 1, 0.1f, 0.1f, 1, 1, one, one, one, one, one, one, one, nullptr) == OCC4D_EINVAL);
  CHECK(occ4d_layers_march_i32(nullptr, 2, 2, 2, 1, 0, 1, 0, 1, 0, 1, nullptr, nullptr, 0, 1, 1, 0.1f, 0.1f, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == OCC4D_OK);
  for (int i = 0; i < 8; ++i) CHECK(one[i] == 0);
  CHECK(seen > 0 && dropped > 0);                                    // (the cases are not empty ones)
  std::printf("ok: %d calls, %lld pixels with an object, %lld of them dropped one\n", calls, seen, dropped);
  return 0;
}
