// The ray cast of the decoded field into camera views (include/ext/occ4d_raycast.h), shared WORD FOR WORD by the HIP kernel
// (csrc/raycast.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the ray of a pixel, the grid coordinate, the trilinear value,
// the march with its refinement, the item body of one pixel and the entry point's argument contract (host only).  Both builds
// compile with -ffp-contract=off: only the explicit fmaf() of row4 (the ray's two end points) fuses.  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ext/occ4d_raycast.h"
#include "frontend_math.hpp"      // row4: the fused chain of a (4, 4) @ (4, N) float32 product; OCC4D_HD; contract.hpp

namespace occ4d_raycast {

using occ4d_frontend::row4;

constexpr int MAX_CHANNELS = OCC4D_RAYCAST_MAX_CHANNELS;
constexpr int MAX_STEPS = OCC4D_RAYCAST_MAX_STEPS;
constexpr int MAX_SIDE = 32768;                         // (float)px is exact, a pixel index fits an int

struct Args {
  const float* field; int64_t ld;
  const float* attrs; int64_t ld_attr;
  const float* k_inv; const float* rt_inv;
  float* depth; int32_t* cell; float* feat;
  int n[3];                                             // nx, ny, nz
  float origin[3], spacing[3];
  float level, near_depth, step, depth_background, feat_background;
  int V, H, W, n_steps, C;
  int32_t cols[MAX_CHANNELS];
};

// P(d) = rt_inv (k_inv (px d, py d, d, 1)): the first three components
OCC4D_HD void ray_point(const float* __restrict__ k_inv, const float* __restrict__ rt_inv, float px, float py, float d, float* P) {
  const float q0 = px * d, q1 = py * d;
  const float s0 = row4(k_inv + 0, q0, q1, d, 1.f);
  const float s1 = row4(k_inv + 4, q0, q1, d, 1.f);
  const float s2 = row4(k_inv + 8, q0, q1, d, 1.f);
  const float s3 = row4(k_inv + 12, q0, q1, d, 1.f);
  P[0] = row4(rt_inv + 0, s0, s1, s2, s3);
  P[1] = row4(rt_inv + 4, s0, s1, s2, s3);
  P[2] = row4(rt_inv + 8, s0, s1, s2, s3);
}

OCC4D_HD float grid_coord(float p, float origin, float spacing) { return (p - origin) / spacing - 0.5f; }

// float comparisons: a NaN fails
OCC4D_HD bool in_axis(float g, int n) { return 0.0f <= g && g <= (float)(n - 1); }

// the cell of a coordinate that has passed in_axis or the clamp: 0 <= c <= n - 2
OCC4D_HD int cell_of(float g, int n) {
  const int c = (int)floorf(g);
  return c < n - 2 ? c : n - 2;
}

OCC4D_HD float lerp(float a, float b, float w) { return a + w * (b - a); }

// trilinear over the cell whose low corner is at `base` (element strides sx, sy, sz): z first, then y, then x
OCC4D_HD float trilinear(const float* __restrict__ base, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz) {
  const float v00 = lerp(base[0], base[sz], wz);
  const float v01 = lerp(base[sy], base[sy + sz], wz);
  const float v10 = lerp(base[sx], base[sx + sz], wz);
  const float v11 = lerp(base[sx + sy], base[sx + sy + sz], wz);
  return lerp(lerp(v00, v01, wy), lerp(v10, v11, wy), wx);
}

// the sample at position p: whether it is in the grid, and then its value
OCC4D_HD bool sample(const Args& a, const float* p, float* value) {
  const float gx = grid_coord(p[0], a.origin[0], a.spacing[0]);
  const float gy = grid_coord(p[1], a.origin[1], a.spacing[1]);
  const float gz = grid_coord(p[2], a.origin[2], a.spacing[2]);
  if (!(in_axis(gx, a.n[0]) && in_axis(gy, a.n[1]) && in_axis(gz, a.n[2]))) return false;
  const int cx = cell_of(gx, a.n[0]), cy = cell_of(gy, a.n[1]), cz = cell_of(gz, a.n[2]);
  const int64_t flat = ((int64_t)cx * a.n[1] + cy) * a.n[2] + cz;
  *value = trilinear(a.field + flat * a.ld, (int64_t)a.n[1] * a.n[2] * a.ld, (int64_t)a.n[2] * a.ld, a.ld, gx - (float)cx,
                     gy - (float)cy, gz - (float)cz);
  return true;
}

OCC4D_HD float depth_of(const Args& a, int i) { return a.near_depth + (float)i * a.step; }

// the march of one ray: whether it hits, and the hit's depth
OCC4D_HD bool march(const Args& a, const float* P0, const float* dir, float* depth) {
  bool prev_in = false;
  float prev_v = 0.0f;
  for (int i = 0; i < a.n_steps; ++i) {
    const float d = depth_of(a, i);
    const float p[3] = {P0[0] + d * dir[0], P0[1] + d * dir[1], P0[2] + d * dir[2]};
    float v = 0.0f;
    const bool in = sample(a, p, &v);
    if (in && v >= a.level) {
      if (i >= 1 && prev_in && prev_v < a.level) {
        float t = (a.level - prev_v) / (v - prev_v);
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
        const float d0 = depth_of(a, i - 1);
        *depth = d0 + t * (d - d0);
      } else {
        *depth = d;
      }
      return true;
    }
    prev_in = in;
    prev_v = v;
  }
  return false;
}

OCC4D_HD float clamped_coord(float p, float origin, float spacing, int n) {
  return fminf(fmaxf(grid_coord(p, origin, spacing), 0.0f), (float)(n - 1));
}

// pixel (px, py) of view v: the three outputs
OCC4D_HD void pixel_item(const Args& a, int v, int px, int py) {
  float P0[3], P1[3], depth = 0.0f;
  ray_point(a.k_inv + 16 * v, a.rt_inv + 16 * v, (float)px, (float)py, 0.0f, P0);
  ray_point(a.k_inv + 16 * v, a.rt_inv + 16 * v, (float)px, (float)py, 1.0f, P1);
  const float dir[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]};
  const bool hit = march(a, P0, dir, &depth);
  const int64_t pixel = ((int64_t)v * a.H + py) * a.W + px;
  if (a.depth) a.depth[pixel] = hit ? depth : a.depth_background;
  if (!a.cell && !a.feat) return;                       // (feat is null when C == 0)
  if (!hit) {
    if (a.cell) a.cell[pixel] = -1;
    if (a.feat)
      for (int c = 0; c < a.C; ++c) a.feat[pixel * a.C + c] = a.feat_background;
    return;
  }
  const float gx = clamped_coord(P0[0] + depth * dir[0], a.origin[0], a.spacing[0], a.n[0]);
  const float gy = clamped_coord(P0[1] + depth * dir[1], a.origin[1], a.spacing[1], a.n[1]);
  const float gz = clamped_coord(P0[2] + depth * dir[2], a.origin[2], a.spacing[2], a.n[2]);
  const int cx = cell_of(gx, a.n[0]), cy = cell_of(gy, a.n[1]), cz = cell_of(gz, a.n[2]);
  const int64_t flat = ((int64_t)cx * a.n[1] + cy) * a.n[2] + cz;
  if (a.cell) a.cell[pixel] = (int32_t)flat;
  if (a.feat) {
    const float wx = gx - (float)cx, wy = gy - (float)cy, wz = gz - (float)cz;
    const int64_t sz = a.ld_attr, sy = (int64_t)a.n[2] * sz, sx = (int64_t)a.n[1] * sy;
    const float* row = a.attrs + flat * a.ld_attr;
    for (int c = 0; c < a.C; ++c) a.feat[pixel * a.C + c] = trilinear(row + a.cols[c], sx, sy, sz, wx, wy, wz);
  }
}

// ---- argument contract (host): the status, `empty` = nothing to do, the arguments filled
inline int check_raycast(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                         float sz, float level, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth,
                         float step, int n_steps, const float* attrs, int64_t ld_attr, int d, const int32_t* cols_host, int C,
                         float depth_background, float feat_background, float* depth, int32_t* cell, float* feat, bool& empty,
                         Args& a) {
  const char* who = "occ4d_raycast_grid_f32";
  OCC4D_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: nx = %d, ny = %d, nz = %d must be >= 2", who, nx, ny, nz);
  OCC4D_REQUIRE((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX",
                who, nx, ny, nz);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(V >= 0 && H >= 0 && W >= 0 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: V = %d must be >= 0, H = %d, W = %d in 0 .. %d", who, V,
                H, W, MAX_SIDE);
  OCC4D_REQUIRE((int64_t)V * H * W < ((int64_t)1 << 31), "%s: V H W = %lld must be < 2^31", who, (long long)V * H * W);
  OCC4D_REQUIRE(step > 0.0f && step < INFINITY, "%s: step = %g must be finite and > 0", who, (double)step);
  OCC4D_REQUIRE(near_depth > -INFINITY && near_depth < INFINITY, "%s: near = %g must be finite", who, (double)near_depth);
  OCC4D_REQUIRE(n_steps >= 1 && n_steps <= MAX_STEPS, "%s: n_steps = %d must be in 1 .. %d", who, n_steps, MAX_STEPS);
  OCC4D_REQUIRE(C >= 0 && C <= MAX_CHANNELS, "%s: C = %d must be in 0 .. %d", who, C, MAX_CHANNELS);
  empty = V == 0 || H == 0 || W == 0;
  a = Args{field, ld, attrs, ld_attr, k_inv, rt_inv, depth, cell, C > 0 ? feat : nullptr, {nx, ny, nz}, {x0, y0, z0}, {sx, sy, sz},
           level, near_depth, step, depth_background, feat_background, V, H, W, n_steps, C, {0}};
  if (C > 0) {
    OCC4D_REQUIRE(cols_host, "%s: null cols_host with C = %d", who, C);
    OCC4D_REQUIRE(d >= 1 && ld_attr >= d, "%s: d = %d, ld_attr = %lld: need 1 <= d <= ld_attr", who, d, (long long)ld_attr);
    for (int c = 0; c < C; ++c) {
      OCC4D_REQUIRE(cols_host[c] >= 0 && cols_host[c] < d, "%s: column %d must be in 0 .. d - 1 = %d", who, cols_host[c], d - 1);
      a.cols[c] = cols_host[c];
    }
    OCC4D_REQUIRE(empty || !feat || attrs, "%s: null attrs with C = %d", who, C);
  }
  OCC4D_REQUIRE(empty || field, "%s: null field with n = %lld", who, (long long)nx * ny * nz);
  OCC4D_REQUIRE(empty || (k_inv && rt_inv), "%s: null k_inv / rt_inv", who);
  return OCC4D_OK;
}

}  // namespace occ4d_raycast
