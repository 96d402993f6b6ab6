// The labelled objects as depth layers in camera views (include/ext/occ4d_layers.h), shared WORD FOR WORD by the HIP kernel
// (csrc/layers.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the OWNER of a sample, the find-or-open step of LAYERS, the march
// of one pixel, the rows it writes, the fill values of the table and the argument contract (host only).  The ray, the samples, the
// grid coordinate and the IN test are csrc/raycast_math.hpp's own functions, called, not restated.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ext/occ4d_layers.h"
#include "raycast_math.hpp"       // ray_point, depth_of, grid_coord, in_axis; OCC4D_HD; contract.hpp

namespace occ4d_layers {

namespace ry = occ4d_raycast;

constexpr int MAX_LAYERS = OCC4D_LAYERS_MAX;
constexpr int COLS = OCC4D_LAYERS_COLS;
constexpr int SLOTS = OCC4D_LAYERS_GATHER_SLOTS;
constexpr int PROBES = OCC4D_LAYERS_GATHER_PROBES;
static_assert(PROBES <= SLOTS, "a probe sequence visits no slot twice");
static_assert(OCC4D_LAYERS_AMODAL == 0 && OCC4D_LAYERS_VISIBLE == 1 && OCC4D_LAYERS_NEAR == 2 && OCC4D_LAYERS_XMIN == 3 &&
              OCC4D_LAYERS_XMAX == 4 && OCC4D_LAYERS_YMIN == 5 && OCC4D_LAYERS_YMAX == 6 && COLS == 7, "the columns of table");

struct Args {
  ry::Args ray;                                         // the cameras, the grid's frame and the march: what depth_of and the ray take
  const int32_t* labels;
  int32_t *label, *first, *samples, *point, *count, *table, *status;
  int K, L;
};

// the layers of one pixel.  Only ever indexed by constants (the loops below unroll): on the device they are registers.
struct Layers {
  int32_t label[MAX_LAYERS], first[MAX_LAYERS], samples[MAX_LAYERS], point[MAX_LAYERS];
  int32_t count;
};

OCC4D_HD void reset(Layers& s) {
#pragma unroll
  for (int j = 0; j < MAX_LAYERS; ++j) s.label[j] = -1, s.first[j] = -1, s.samples[j] = 0, s.point[j] = -1;
  s.count = 0;
}

// word c of a table row no pixel contributed to
OCC4D_HD int32_t fill_value(int c) { return c < OCC4D_LAYERS_NEAR ? 0 : (c == OCC4D_LAYERS_XMAX || c == OCC4D_LAYERS_YMAX) ? -1 : INT32_MAX; }

// the nearest grid point of a coordinate that has passed in_axis: 0 <= r <= n - 1
OCC4D_HD int nearest(float g, int n) {
  const int r = (int)floorf(g + 0.5f);
  return r < n - 1 ? r : n - 1;
}

// OWNER of the sample at position p: whether it is IN the grid; then *point = r and *owner = labels[r], or -1 outside [0, K)
OCC4D_HD bool owner_of(const Args& a, const float* p, int32_t* owner, int32_t* point) {
  const float gx = ry::grid_coord(p[0], a.ray.origin[0], a.ray.spacing[0]);
  const float gy = ry::grid_coord(p[1], a.ray.origin[1], a.ray.spacing[1]);
  const float gz = ry::grid_coord(p[2], a.ray.origin[2], a.ray.spacing[2]);
  if (!(ry::in_axis(gx, a.ray.n[0]) && ry::in_axis(gy, a.ray.n[1]) && ry::in_axis(gz, a.ray.n[2]))) return false;
  const int rx = nearest(gx, a.ray.n[0]), ry_ = nearest(gy, a.ray.n[1]), rz = nearest(gz, a.ray.n[2]);
  const int64_t r = ((int64_t)rx * a.ray.n[1] + ry_) * a.ray.n[2] + rz;              // < n <= INT32_MAX
  const int32_t o = a.labels[r];
  *point = (int32_t)r;
  *owner = (o >= 0 && o < a.K) ? o : -1;
  return true;
}

// the find-or-open step for a sample i with owner o >= 0 at grid point `point`: compare-and-select over constant indices
OCC4D_HD void visit(Layers& s, int L, int32_t o, int i, int32_t point) {
  bool found = false;
#pragma unroll
  for (int j = 0; j < MAX_LAYERS; ++j) {
    const bool hit = s.label[j] == o;                   // (an unused layer holds -1, o >= 0)
    s.samples[j] += hit ? 1 : 0;
    found = found || hit;
  }
  if (found) return;
  if (s.count >= L) {                                   // L layers are stored: the object is dropped
    s.count = L + 1;
    return;
  }
#pragma unroll
  for (int j = 0; j < MAX_LAYERS; ++j) {
    const bool open = j == s.count;
    s.label[j] = open ? o : s.label[j];
    s.first[j] = open ? i : s.first[j];
    s.samples[j] = open ? 1 : s.samples[j];
    s.point[j] = open ? point : s.point[j];
  }
  s.count += 1;
}

// the march of pixel (px, py) of view v: its layers.  The samples IN the grid are one contiguous range (SHORTCUT of the header):
// the loop ends once the ray has been in and is out again.
OCC4D_HD void march(const Args& a, int v, int px, int py, Layers& s) {
  float P0[3], P1[3];
  ry::ray_point(a.ray.k_inv + 16 * v, a.ray.rt_inv + 16 * v, (float)px, (float)py, 0.0f, P0);
  ry::ray_point(a.ray.k_inv + 16 * v, a.ray.rt_inv + 16 * v, (float)px, (float)py, 1.0f, P1);
  const float dir[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]};
  reset(s);
  bool been_in = false;
  for (int i = 0; i < a.ray.n_steps; ++i) {
    const float d = ry::depth_of(a.ray, i);
    const float p[3] = {P0[0] + d * dir[0], P0[1] + d * dir[1], P0[2] + d * dir[2]};
    int32_t o = -1, point = -1;
    const bool in = owner_of(a, p, &o, &point);
    if (been_in && !in) break;
    been_in = in;
    if (o >= 0) visit(s, a.L, o, i, point);
  }
}

// the rows of pixel number `pixel` = (v * H + py) * W + px
OCC4D_HD void write_pixel(const Args& a, int64_t pixel, const Layers& s) {
  if (a.count) a.count[pixel] = s.count;
#pragma unroll
  for (int j = 0; j < MAX_LAYERS; ++j)
    if (j < a.L) {
      const int64_t e = pixel * a.L + j;
      if (a.label) a.label[e] = s.label[j];
      if (a.first) a.first[e] = s.first[j];
      if (a.samples) a.samples[e] = s.samples[j];
      if (a.point) a.point[e] = s.point[j];
    }
}

// ---- argument contract (host): the status, `empty` = nothing to do, the arguments filled
inline int check_layers(const int32_t* labels, int nx, int ny, int nz, int K, float x0, float sx, float y0, float sy, float z0, float sz,
                        const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth, float step, int n_steps, int L,
                        int32_t* label, int32_t* first, int32_t* samples, int32_t* point, int32_t* count, int32_t* table,
                        int32_t* status, bool& empty, Args& a) {
  const char* who = "occ4d_layers_march_i32";
  OCC4D_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: nx = %d, ny = %d, nz = %d must be >= 2", who, nx, ny, nz);
  OCC4D_REQUIRE((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX",
                who, nx, ny, nz);
  OCC4D_REQUIRE(V >= 0 && H >= 0 && W >= 0 && H <= ry::MAX_SIDE && W <= ry::MAX_SIDE, "%s: V = %d must be >= 0, H = %d, W = %d in 0 .. %d",
                who, V, H, W, ry::MAX_SIDE);
  OCC4D_REQUIRE((int64_t)V * H * W < ((int64_t)1 << 31), "%s: V H W = %lld must be < 2^31", who, (long long)V * H * W);
  OCC4D_REQUIRE(step > 0.0f && step < INFINITY, "%s: step = %g must be finite and > 0", who, (double)step);
  OCC4D_REQUIRE(near_depth > -INFINITY && near_depth < INFINITY, "%s: near = %g must be finite", who, (double)near_depth);
  OCC4D_REQUIRE(n_steps >= 1 && n_steps <= ry::MAX_STEPS, "%s: n_steps = %d must be in 1 .. %d", who, n_steps, ry::MAX_STEPS);
  OCC4D_REQUIRE(K >= 0, "%s: K = %d must be >= 0", who, K);
  OCC4D_REQUIRE((int64_t)V * (K > 1 ? K : 1) * COLS < ((int64_t)1 << 31), "%s: V max(K, 1) %d = %d * %d * %d must be < 2^31", who, COLS, V,
                K > 1 ? K : 1, COLS);
  OCC4D_REQUIRE(L >= 1 && L <= MAX_LAYERS, "%s: L = %d must be in 1 .. %d", who, L, MAX_LAYERS);
  OCC4D_REQUIRE((int64_t)V * H * W * L < ((int64_t)1 << 31), "%s: V H W L = %lld must be < 2^31", who, (long long)V * H * W * L);
  int32_t* const rows = K > 0 ? table : nullptr;        // (K == 0: a table without rows)
  empty = V == 0 || H == 0 || W == 0 || !(label || first || samples || point || count || rows || status);
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(labels, "%s: null labels with n = %lld", who, (long long)nx * ny * nz);
  OCC4D_REQUIRE(k_inv && rt_inv, "%s: null k_inv / rt_inv", who);
  a.ray = ry::Args{};
  a.ray.k_inv = k_inv, a.ray.rt_inv = rt_inv;
  a.ray.n[0] = nx, a.ray.n[1] = ny, a.ray.n[2] = nz;
  a.ray.origin[0] = x0, a.ray.origin[1] = y0, a.ray.origin[2] = z0;
  a.ray.spacing[0] = sx, a.ray.spacing[1] = sy, a.ray.spacing[2] = sz;
  a.ray.near_depth = near_depth, a.ray.step = step;
  a.ray.V = V, a.ray.H = H, a.ray.W = W, a.ray.n_steps = n_steps;
  a.labels = labels;
  a.label = label, a.first = first, a.samples = samples, a.point = point, a.count = count;
  a.table = rows, a.status = status;
  a.K = K, a.L = L;
  return OCC4D_OK;
}

}  // namespace occ4d_layers
