// A stand-alone host program that drives the g++ twin's sweep entry point (include/ext/occ4d_sweep.h), and with it the shared
// bodies of csrc/sweep_math.hpp and csrc/raycast_math.hpp, over the shapes of the test matrix with buffers of EXACTLY the
// documented sizes (strided field and attributes included), for a run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/sweep_sanitize.cpp occlusions-4d_amd/csrc_cpu/occ4d_twin.cpp \
//       -o /tmp/sweep_sanitize && /tmp/sweep_sanitize
//
// Grids 2 x 2 x 2, 3 x 2 x 5, 17 x 9 x 33; V in 0 / 1 / 3; ray images (1, 1), (1, 63), (1, 65), (8, 8), (9, 17), (7, 40); shared and
// per-view tables; 1 / 2 / 64 steps; fields all air, all solid, a blob and one with NaN and infinities; 0 / 1 / 3 channels; 0 / 1 / 5
// classes; labels null, in range and out of range; sensors outside, inside and degenerate (zero, NaN and infinite poses and
// directions); every output null in turn.  It checks what can be checked without a second implementation: the status; a return has
// 0 <= cell, owner < n, the owner is a corner of the cell, near <= range <= near + (n_steps - 1) step, 0 <= cos <= 1, sem in [0,
// n_sem) and inst == labels[owner] or -1; a ray without one has the backgrounds, -1 and 0.  Prints "ok", the number of calls and
// how many rays had a return and how many had none (neither may be 0).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occ4d.h"
#include "ext/occ4d_sweep.h"

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
static long long returns = 0, none = 0;
static const float LEVEL = 0.46f, RANGE_BG = -1.5f, FEAT_BG = -2.5f;

static void run(int nx, int ny, int nz, int V, int B, int A, int per_view, int n_steps, int field_kind, int C, int n_sem, int label_kind,
                int pad, unsigned nulls) {
  const int64_t n = (int64_t)nx * ny * nz, R = (int64_t)B * A, rays = (int64_t)V * R;
  const int K = 4, d = 6;
  const int64_t ld = 1 + pad, ld_attr = d + pad;
  const float origin[3] = {uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f)};
  const float spacing[3] = {uniform(0.1f, 0.8f), uniform(0.1f, 0.8f), uniform(0.1f, 0.8f)};
  const float size[3] = {spacing[0] * (float)nx, spacing[1] * (float)ny, spacing[2] * (float)nz};
  const float strange[] = {NAN, INFINITY, -INFINITY, LEVEL, 0.0f, -0.0f, 100.0f, -100.0f};
  std::vector<float> field((size_t)((n - 1) * ld + 1));             // exactly the last element read
  for (int64_t p = 0; p < n; ++p) {
    const int ix = (int)(p / ((int64_t)ny * nz)), iy = (int)(p / nz % ny), iz = (int)(p % nz);
    const float r = std::sqrt(std::pow((ix + 0.5f) / nx - 0.5f, 2.0f) + std::pow((iy + 0.5f) / ny - 0.5f, 2.0f) + std::pow((iz + 0.5f) / nz - 0.5f, 2.0f));
    field[(size_t)(p * ld)] = field_kind == 0 ? -2.0f : field_kind == 1 ? 0.9f : field_kind == 2 ? 1.0f - 1.4f * r + uniform(-0.02f, 0.02f)
                              : (rnd() % 3 == 0 ? strange[rnd() % 8] : uniform(-0.5f, 1.2f));
  }
  std::vector<float> attrs(C > 0 || n_sem > 0 ? (size_t)((n - 1) * ld_attr + d) : 0);
  for (auto& v : attrs) v = rnd() % 50 == 0 ? NAN : uniform(-2.0f, 2.0f);
  std::vector<int32_t> labels(label_kind ? (size_t)n : 0);
  const int32_t foreign[] = {-1, -7, K, K + 5, INT32_MAX, INT32_MIN};
  for (auto& v : labels) v = label_kind == 2 && rnd() % 3 == 0 ? foreign[rnd() % 6] : (int32_t)(rnd() % (uint32_t)K);
  int32_t cols[3] = {(int32_t)(rnd() % d), (int32_t)(rnd() % d), (int32_t)(rnd() % d)};
  std::vector<float> pose((size_t)V * 12), dirs((size_t)(per_view ? rays : R) * 3);
  for (int v = 0; v < V; ++v) {
    float* m = &pose[(size_t)v * 12];
    for (int i = 0; i < 12; ++i) m[i] = 0.0f;
    const int where = (int)(rnd() % 4), turn = (int)(rnd() % 3);     // 0: outside;  1: inside;  2: far away;  3: degenerate
    const float sign = (rnd() & 1) ? -1.0f : 1.0f;
    for (int a = 0; a < 3; ++a) m[4 * ((a + turn) % 3) + a] = a == 2 ? 1.0f : sign;          // a signed permutation
    for (int a = 0; a < 3; ++a)
      m[4 * a + 3] = origin[a] + size[a] * (where == 1 ? uniform(0.2f, 0.8f) : where == 2 ? uniform(-30.0f, 30.0f) : uniform(-0.6f, 1.6f));
    if (where == 3) m[rnd() % 12] = strange[rnd() % 3], m[rnd() % 12] = 0.0f;
  }
  for (size_t r = 0; r < dirs.size() / 3; ++r) {
    const float az = uniform(-3.14159f, 3.14159f), el = uniform(-0.7f, 0.7f);
    dirs[3 * r] = std::cos(el) * std::cos(az), dirs[3 * r + 1] = std::cos(el) * std::sin(az), dirs[3 * r + 2] = std::sin(el);
    if (rnd() % 40 == 0) dirs[3 * r + rnd() % 3] = strange[rnd() % 3];
    if (rnd() % 40 == 0) dirs[3 * r] = dirs[3 * r + 1] = dirs[3 * r + 2] = 0.0f;
  }
  const float reach = std::sqrt(size[0] * size[0] + size[1] * size[1] + size[2] * size[2]);
  const float step = 2.5f * reach / 64.0f, near_range = (rnd() % 4 == 0) ? 0.0f : step;
  std::vector<float> range((size_t)rays, 12345.0f), point((size_t)rays * 3, 12345.0f), cosine((size_t)rays, 12345.0f),
      feat((size_t)rays * C, 12345.0f);
  std::vector<int32_t> cell((size_t)rays, 12345), owner((size_t)rays, 12345), sem((size_t)rays, 12345), inst((size_t)rays, 12345);
  auto fp = [&](std::vector<float>& v, int bit) { return ((nulls >> bit) & 1) || v.empty() ? nullptr : v.data(); };
  auto ip = [&](std::vector<int32_t>& v, int bit) { return ((nulls >> bit) & 1) || v.empty() ? nullptr : v.data(); };
  CHECK(occ4d_sweep_rays_f32(field.data(), ld, nx, ny, nz, origin[0], spacing[0], origin[1], spacing[1], origin[2], spacing[2], LEVEL,
                             pose.empty() ? nullptr : pose.data(), dirs.empty() ? nullptr : dirs.data(), V, B, A, per_view, near_range,
                             step, n_steps, attrs.empty() ? nullptr : attrs.data(), ld_attr, attrs.empty() ? 0 : d, cols, C, d - n_sem,
                             n_sem, labels.empty() ? nullptr : labels.data(), K, RANGE_BG, FEAT_BG, fp(range, 0), fp(point, 1), ip(cell, 2),
                             ip(owner, 3), fp(cosine, 4), ip(sem, 5), ip(inst, 6), fp(feat, 7), nullptr) == OCC4D_OK);
  ++calls;
  if (nulls != 0) return;                                            // (what follows reads every array)
  const float last = near_range + (float)(n_steps - 1) * step;
  for (int64_t r = 0; r < rays; ++r) {
    const size_t e = (size_t)r;
    if (cell[e] < 0) {
      ++none;
      CHECK(cell[e] == -1 && owner[e] == -1 && range[e] == RANGE_BG && cosine[e] == 0.0f);
      CHECK(point[3 * e] == RANGE_BG && point[3 * e + 1] == RANGE_BG && point[3 * e + 2] == RANGE_BG);
      CHECK(n_sem == 0 ? sem[e] == 12345 : sem[e] == -1);
      CHECK(label_kind == 0 ? inst[e] == 12345 : inst[e] == -1);
      for (int c = 0; c < C; ++c) CHECK(feat[e * C + c] == FEAT_BG);
      continue;
    }
    ++returns;
    CHECK(cell[e] < n && owner[e] >= 0 && owner[e] < n);
    const int off = owner[e] - cell[e];                               // a corner of the cell: (x * ny + y) * nz + z with x, y, z in 0 / 1
    bool corner = false;
    for (int j = 0; j < 8; ++j) corner |= off == ((j >> 2) * ny + ((j >> 1) & 1)) * nz + (j & 1);
    CHECK(corner);
    CHECK(range[e] >= near_range && range[e] <= last);
    CHECK(cosine[e] >= 0.0f && cosine[e] <= 1.0f);
    CHECK(n_sem == 0 ? sem[e] == 12345 : (sem[e] >= 0 && sem[e] < n_sem));
    if (label_kind == 0) CHECK(inst[e] == 12345);
    else {
      const int32_t lab = labels[(size_t)owner[e]];
      CHECK(inst[e] == (lab >= 0 && lab < K ? lab : -1));
    }
  }
}

int main() {
  const int grids[][3] = {{2, 2, 2}, {3, 2, 5}, {17, 9, 33}};
  const int images[][2] = {{1, 1}, {1, 63}, {1, 65}, {8, 8}, {9, 17}, {7, 40}};
  const int views[] = {0, 1, 3}, steps[] = {1, 2, 64}, few[] = {0, 1, 3}, classes[] = {0, 1, 5};
  int k = 0;
  for (int round = 0; round < 2; ++round)
    for (const auto& g : grids)
      for (const auto& im : images)
        for (int V : views)
          for (int field_kind = 0; field_kind < 4; ++field_kind, ++k)
            run(g[0], g[1], g[2], V, im[0], im[1], k % 2, steps[(k + round) % 3], field_kind, few[k % 3], classes[(k / 3) % 3], (k / 2) % 3,
                (k / 4) % 2 ? 3 : 0, k % 5 == 4 ? 1u + rnd() % 254u : 0u);
  run(3, 2, 5, 2, 0, 7, 0, 8, 2, 1, 1, 1, 0, 0);                       // B == 0
  run(3, 2, 5, 2, 7, 0, 1, 8, 2, 1, 1, 1, 0, 0);                       // A == 0
  run(3, 2, 5, 2, 4, 4, 0, 8, 2, 3, 5, 2, 3, 255);                     // every output null
  // the rejected calls leave their buffers alone; the no-ops take null pointers
  int32_t one[8] = {0};
  float f[16] = {0};
#define CALL(field, nx, V, per_view, step, out)                                                                                      \
  occ4d_sweep_rays_f32(field, 1, nx, 2, 2, 0, 1, 0, 1, 0, 1, 0.5f, V ? f : nullptr, V ? f : nullptr, V, 1, 1, per_view, 0.1f, step, 1, \
                       nullptr, 0, 0, nullptr, 0, 0, 0, nullptr, 0, 0.0f, 0.0f, out, out, one, one, out, one, one, out, nullptr)
  CHECK(CALL(f, 1, 1, 0, 0.1f, f) == OCC4D_EINVAL);
  CHECK(CALL(f, 2, 1, 2, 0.1f, f) == OCC4D_EINVAL);
  CHECK(CALL(f, 2, 1, 0, 0.0f, f) == OCC4D_EINVAL);
  CHECK(CALL((const float*)nullptr, 2, 1, 0, 0.1f, f) == OCC4D_EINVAL);
  CHECK(CALL((const float*)nullptr, 2, 0, 0, 0.1f, (float*)nullptr) == OCC4D_OK);
  for (int i = 0; i < 8; ++i) CHECK(one[i] == 0);
  for (int i = 0; i < 16; ++i) CHECK(f[i] == 0.0f);
  CHECK(returns > 0 && none > 0);                                    // (the cases are not empty ones)
  std::printf("ok: %d calls, %lld rays with a return, %lld without\n", calls, returns, none);
  return 0;
}
