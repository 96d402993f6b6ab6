// The decoded field scanned by a virtual lidar (include/ext/occ4d_sweep.h), shared WORD FOR WORD by the HIP kernel
// (csrc/sweep.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the ray of a pose and a direction, the gradient of the trilinear
// interpolant, the incidence cosine, the owner corner, the item body of one ray and the entry point's argument contract (host
// only).  The march, the sample, the grid coordinate, the cell, the clamp and the trilinear value are those of
// csrc/raycast_math.hpp, CALLED here and restated nowhere.  Both builds compile with -ffp-contract=off: only the explicit fmaf()
// of ray_direction fuses.  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ext/occ4d_sweep.h"
#include "raycast_math.hpp"       // ry::march and what it is made of; OCC4D_HD; contract.hpp

namespace occ4d_sweep {

namespace ry = occ4d_raycast;

static_assert(OCC4D_SWEEP_MAX_STEPS == OCC4D_RAYCAST_MAX_STEPS && OCC4D_SWEEP_MAX_CHANNELS == OCC4D_RAYCAST_MAX_CHANNELS,
              "the march and the feature columns are the ray cast's");

struct Args {
  ry::Args m;                                           // the grid, the field, the attribute columns, level, near, step, n_steps
  const float* pose; const float* dirs;
  const int32_t* labels;
  float* range; float* point; int32_t* cell; int32_t* owner; float* cosine; int32_t* sem; int32_t* inst; float* feat;
  float range_background, feat_background;
  int V, B, A, R, per_view, sem_first, n_sem, K;
};

// dir = Rm d: the one fused chain
OCC4D_HD void ray_direction(const float* __restrict__ pose, const float* __restrict__ d, float* dir) {
  for (int a = 0; a < 3; ++a) dir[a] = fmaf(pose[4 * a + 2], d[2], fmaf(pose[4 * a + 1], d[1], pose[4 * a] * d[0]));
}

// the eight corner values of the cell whose low corner is at `base`, index x * 4 + y * 2 + z
OCC4D_HD void corners(const float* __restrict__ base, int64_t sx, int64_t sy, int64_t sz, float* f) {
  f[0] = base[0];       f[1] = base[sz];
  f[2] = base[sy];      f[3] = base[sy + sz];
  f[4] = base[sx];      f[5] = base[sx + sz];
  f[6] = base[sx + sy]; f[7] = base[sx + sy + sz];
}

// the gradient of the trilinear interpolant: per axis the differences along it, then the two lerps over the other axes
OCC4D_HD void gradient(const float* f, float wx, float wy, float wz, const float* spacing, float* g) {
  g[0] = ry::lerp(ry::lerp(f[4] - f[0], f[5] - f[1], wz), ry::lerp(f[6] - f[2], f[7] - f[3], wz), wy) / spacing[0];
  g[1] = ry::lerp(ry::lerp(f[2] - f[0], f[3] - f[1], wz), ry::lerp(f[6] - f[4], f[7] - f[5], wz), wx) / spacing[1];
  g[2] = ry::lerp(ry::lerp(f[1] - f[0], f[3] - f[2], wy), ry::lerp(f[5] - f[4], f[7] - f[6], wy), wx) / spacing[2];
}

// the non-negative cosine between the gradient and the ray; a NaN or zero denominator gives 0
OCC4D_HD float incidence(const float* g, const float* dir) {
  const float nd = g[0] * dir[0] + g[1] * dir[1] + g[2] * dir[2];
  const float nn = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
  const float dd = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  const float den = sqrtf(nn * dd);
  return den > 0.0f ? fminf(fabsf(nd) / den, 1.0f) : 0.0f;
}

// the corner with the greatest value, the first of them; a NaN never wins
OCC4D_HD int owner_corner(const float* f) {
  float best = -INFINITY;
  int k = 0;
  for (int j = 0; j < 8; ++j)
    if (f[j] > best) { best = f[j]; k = j; }
  return k;
}

// the first maximum of n_sem >= 1 columns
OCC4D_HD int argmax_first(const float* __restrict__ row, int n_sem) {
  float m = row[0];
  int k = 0;
  for (int j = 1; j < n_sem; ++j)
    if (row[j] > m) { m = row[j]; k = j; }
  return k;
}

// ray r of view v: the eight outputs
OCC4D_HD void ray_item(const Args& a, int v, int r) {
  const ry::Args& m = a.m;
  const float* pose = a.pose + 12 * (int64_t)v;
  const float* d = a.dirs + 3 * ((a.per_view ? (int64_t)v * a.R : (int64_t)0) + r);
  const float P0[3] = {pose[3], pose[7], pose[11]};
  float dir[3], range = 0.0f;
  ray_direction(pose, d, dir);
  const bool hit = ry::march(m, P0, dir, &range);
  const int64_t ray = (int64_t)v * a.R + r;
  if (a.range) a.range[ray] = hit ? range : a.range_background;
  if (!hit) {
    if (a.point)
      for (int c = 0; c < 3; ++c) a.point[ray * 3 + c] = a.range_background;
    if (a.cell) a.cell[ray] = -1;
    if (a.owner) a.owner[ray] = -1;
    if (a.cosine) a.cosine[ray] = 0.0f;
    if (a.sem) a.sem[ray] = -1;
    if (a.inst) a.inst[ray] = -1;
    if (a.feat)
      for (int c = 0; c < m.C; ++c) a.feat[ray * m.C + c] = a.feat_background;
    return;
  }
  const float h[3] = {P0[0] + range * dir[0], P0[1] + range * dir[1], P0[2] + range * dir[2]};
  if (a.point)
    for (int c = 0; c < 3; ++c) a.point[ray * 3 + c] = h[c];
  if (!a.cell && !a.owner && !a.cosine && !a.sem && !a.inst && !a.feat) return;
  const float gx = ry::clamped_coord(h[0], m.origin[0], m.spacing[0], m.n[0]);
  const float gy = ry::clamped_coord(h[1], m.origin[1], m.spacing[1], m.n[1]);
  const float gz = ry::clamped_coord(h[2], m.origin[2], m.spacing[2], m.n[2]);
  const int cx = ry::cell_of(gx, m.n[0]), cy = ry::cell_of(gy, m.n[1]), cz = ry::cell_of(gz, m.n[2]);
  const int64_t flat = ((int64_t)cx * m.n[1] + cy) * m.n[2] + cz;
  const float wx = gx - (float)cx, wy = gy - (float)cy, wz = gz - (float)cz;
  if (a.cell) a.cell[ray] = (int32_t)flat;
  if (a.owner || a.cosine || a.sem || a.inst) {
    float f[8];
    corners(m.field + flat * m.ld, (int64_t)m.n[1] * m.n[2] * m.ld, (int64_t)m.n[2] * m.ld, m.ld, f);
    if (a.cosine) {
      float g[3];
      gradient(f, wx, wy, wz, m.spacing, g);
      a.cosine[ray] = incidence(g, dir);
    }
    if (a.owner || a.sem || a.inst) {
      const int k = owner_corner(f);
      const int64_t own = flat + ((int64_t)(k >> 2) * m.n[1] + ((k >> 1) & 1)) * m.n[2] + (k & 1);
      if (a.owner) a.owner[ray] = (int32_t)own;
      if (a.sem) a.sem[ray] = argmax_first(m.attrs + own * m.ld_attr + a.sem_first, a.n_sem);
      if (a.inst) {
        const int32_t label = a.labels[own];
        a.inst[ray] = label >= 0 && label < a.K ? label : -1;
      }
    }
  }
  if (a.feat) {
    const int64_t sz = m.ld_attr, sy = (int64_t)m.n[2] * sz, sx = (int64_t)m.n[1] * sy;
    const float* row = m.attrs + flat * m.ld_attr;
    for (int c = 0; c < m.C; ++c) a.feat[ray * m.C + c] = ry::trilinear(row + m.cols[c], sx, sy, sz, wx, wy, wz);
  }
}

// ---- argument contract (host): the status, `empty` = nothing to do, the arguments filled.  The texts of the grid, near, step and
// n_steps conditions are check_raycast's.
inline int check_sweep(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                       float sz, float level, const float* pose, const float* dirs, int V, int B, int A, int per_view, float near_range,
                       float step, int n_steps, const float* attrs, int64_t ld_attr, int d, const int32_t* cols_host, int C,
                       int sem_first, int n_sem, const int32_t* labels, int K, float range_background, float feat_background,
                       float* range, float* point, int32_t* cell, int32_t* owner, float* cosine, int32_t* sem, int32_t* inst, float* feat,
                       bool& empty, Args& a) {
  const char* who = "occ4d_sweep_rays_f32";
  OCC4D_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: nx = %d, ny = %d, nz = %d must be >= 2", who, nx, ny, nz);
  OCC4D_REQUIRE((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, "%s: nx * ny * nz = %d * %d * %d exceeds INT32_MAX",
                who, nx, ny, nz);
  OCC4D_REQUIRE(ld >= 1, "%s: ld = %lld must be >= 1", who, (long long)ld);
  OCC4D_REQUIRE(V >= 0 && B >= 0 && A >= 0, "%s: V = %d, B = %d, A = %d must be >= 0", who, V, B, A);
  OCC4D_REQUIRE((int64_t)B * A < ((int64_t)1 << 31) && (int64_t)V * B * A < ((int64_t)1 << 31), "%s: V R = %d * %d * %d must be < 2^31", who,
                V, B, A);
  OCC4D_REQUIRE(per_view == 0 || per_view == 1, "%s: per_view = %d must be 0 or 1", who, per_view);
  OCC4D_REQUIRE(step > 0.0f && step < INFINITY, "%s: step = %g must be finite and > 0", who, (double)step);
  OCC4D_REQUIRE(near_range > -INFINITY && near_range < INFINITY, "%s: near = %g must be finite", who, (double)near_range);
  OCC4D_REQUIRE(n_steps >= 1 && n_steps <= ry::MAX_STEPS, "%s: n_steps = %d must be in 1 .. %d", who, n_steps, ry::MAX_STEPS);
  OCC4D_REQUIRE(C >= 0 && C <= ry::MAX_CHANNELS, "%s: C = %d must be in 0 .. %d", who, C, ry::MAX_CHANNELS);
  OCC4D_REQUIRE(n_sem >= 0, "%s: n_sem = %d must be >= 0", who, n_sem);
  OCC4D_REQUIRE(K >= 0, "%s: K = %d must be >= 0", who, K);
  empty = V == 0 || B == 0 || A == 0;
  a = Args{};
  a.m = ry::Args{field, ld, attrs, ld_attr, nullptr, nullptr, nullptr, nullptr, nullptr, {nx, ny, nz}, {x0, y0, z0}, {sx, sy, sz},
                 level, near_range, step, range_background, feat_background, V, B, A, n_steps, C, {0}};
  a.pose = pose; a.dirs = dirs; a.labels = labels;
  a.range = range; a.point = point; a.cell = cell; a.owner = owner; a.cosine = cosine;
  a.sem = n_sem > 0 ? sem : nullptr; a.inst = labels ? inst : nullptr; a.feat = C > 0 ? feat : nullptr;
  a.range_background = range_background; a.feat_background = feat_background;
  a.V = V; a.B = B; a.A = A; a.R = B * A; a.per_view = per_view; a.sem_first = sem_first; a.n_sem = n_sem; a.K = K;
  if (C > 0 || n_sem > 0)
    OCC4D_REQUIRE(d >= 1 && ld_attr >= d, "%s: d = %d, ld_attr = %lld: need 1 <= d <= ld_attr", who, d, (long long)ld_attr);
  if (C > 0) {
    OCC4D_REQUIRE(cols_host, "%s: null cols_host with C = %d", who, C);
    for (int c = 0; c < C; ++c) {
      OCC4D_REQUIRE(cols_host[c] >= 0 && cols_host[c] < d, "%s: column %d must be in 0 .. d - 1 = %d", who, cols_host[c], d - 1);
      a.m.cols[c] = cols_host[c];
    }
  }
  if (n_sem > 0)
    OCC4D_REQUIRE(sem_first >= 0 && (int64_t)sem_first + n_sem <= d, "%s: sem_first = %d, n_sem = %d: need 0 <= sem_first and sem_first + n_sem <= d = %d",
                  who, sem_first, n_sem, d);
  OCC4D_REQUIRE(empty || !((a.feat || a.sem) && !attrs), "%s: null attrs with C = %d, n_sem = %d", who, C, n_sem);
  OCC4D_REQUIRE(empty || field, "%s: null field with n = %lld", who, (long long)nx * ny * nz);
  OCC4D_REQUIRE(empty || (pose && dirs), "%s: null pose / dirs", who);
  return OCC4D_OK;
}

// whether a checked call has anything to write
inline bool writes_nothing(const Args& a) {
  return !a.range && !a.point && !a.cell && !a.owner && !a.cosine && !a.sem && !a.inst && !a.feat;
}

}  // namespace occ4d_sweep
