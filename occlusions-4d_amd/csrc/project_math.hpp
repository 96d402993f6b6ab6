// The camera projection, the z-buffer and the visibility test (include/occ4d_project.h), shared WORD FOR WORD by the HIP
// kernels (csrc/project.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the per-element decisions, the four passes' item
// bodies and the four entry points' argument contracts (host only).  Both are compiled with -ffp-contract=off: only the
// explicit fmaf() of row4 fuses.  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "frontend_math.hpp"      // row4: the fused chain of a (4, 4) @ (4, N) float32 product; contract.hpp

namespace occ4d_project {

using occ4d_frontend::row4;

constexpr int MAX_RADIUS = 4;
constexpr int MAX_CHANNELS = 32;
constexpr int MAX_SIDE = 32768;                         // (float)W is exact, a pixel index fits an int
constexpr unsigned long long EMPTY_KEY = ~0ull;

// pixel_coords_from_point_cloud (utils/geometry.py:67-115) for one point: RT4 (x, y, z, 1), the first two components divided
// by the third (true divisions), the third set to 1, then rows 0 and 1 of K4 of that.  uvz = (u, v, depth).
OCC4D_HD void project(const float* __restrict__ rt, const float* __restrict__ k, float x, float y, float z, float* uvz) {
  const float c0 = row4(rt + 0, x, y, z, 1.f);
  const float c1 = row4(rt + 4, x, y, z, 1.f);
  const float c2 = row4(rt + 8, x, y, z, 1.f);
  const float c3 = row4(rt + 12, x, y, z, 1.f);
  const float un = c0 / c2, vn = c1 / c2;
  uvz[0] = row4(k + 0, un, vn, 1.f, c3);
  uvz[1] = row4(k + 4, un, vn, 1.f, c3);
  uvz[2] = c2;
}

// The pixel rule: the row takes part when its depth is finite and > 0 and its rounded centre lies on the image.  Every
// comparison is made on the floats (NaN fails each of them); the conversions to int come last, on values in [0, MAX_SIDE).
OCC4D_HD bool centre_pixel(const float* uvz, int H, int W, int* px, int* py) {
  const float z = uvz[2];
  if (!(z > 0.f && z < INFINITY)) return false;
  const float ru = rintf(uvz[0]), rv = rintf(uvz[1]);
  if (!(ru >= 0.f && ru < (float)W && rv >= 0.f && rv < (float)H)) return false;
  *px = (int)ru;
  *py = (int)rv;
  return true;
}

OCC4D_HD uint32_t float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
OCC4D_HD float bits_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// positive finite depths order as their bit patterns: the minimum key of a pixel is its nearest row, lowest index on a tie
OCC4D_HD unsigned long long pack_key(float depth, uint32_t row) { return ((unsigned long long)float_bits(depth) << 32) | row; }
OCC4D_HD uint32_t key_row(unsigned long long key) { return (uint32_t)(key & 0xffffffffull); }
OCC4D_HD float key_depth(unsigned long long key) { return bits_float((uint32_t)(key >> 32)); }
// a pixel nothing was splatted on, or whose row index the caller's n does not cover
OCC4D_HD bool key_is_background(unsigned long long key, int n) { return key == EMPTY_KEY || key_row(key) >= (uint32_t)n; }

constexpr int VISIBLE = 0, OCCLUDED = 1, OUTSIDE = 2;

// inside: centre_pixel's answer; z: the row's depth; d: the image's depth at the centre pixel (read only when inside)
OCC4D_HD int visibility_code(bool inside, float z, float d, float margin) {
  if (!inside) return OUTSIDE;
  return (d > 0.f && z - d > margin) ? OCCLUDED : VISIBLE;
}

// ---- the item bodies.  An item of the three point passes is e = (view, row), views outermost; an item of the resolve is a pixel.
struct PointArgs {
  const float* rows; int64_t ld;
  const float* rt; const float* k;
  int64_t items;                          // V * n
  int n;
};

// item e = (view, row) -> (u, v, depth)
OCC4D_HD void project_item(const PointArgs& a, int64_t e, int* view, int* row, float* uvz) {
  const int v = (int)(e / a.n);
  const int i = (int)(e - (int64_t)v * a.n);
  const float* p = a.rows + (int64_t)i * a.ld;
  project(a.rt + 16 * v, a.k + 16 * v, p[0], p[1], p[2], uvz);
  *view = v;
  *row = i;
}

// item e -> out[3 e ..] = (u, v, depth), or (v, u, depth)
OCC4D_HD void points_item(const PointArgs& a, int64_t e, bool flip_xy, float* out) {
  int v, i;
  float uvz[3];
  project_item(a, e, &v, &i, uvz);
  float* o = out + 3 * e;
  o[0] = flip_xy ? uvz[1] : uvz[0];
  o[1] = flip_xy ? uvz[0] : uvz[1];
  o[2] = uvz[2];
}

// the row's key onto the clipped (2 radius + 1)^2 window round its centre pixel.  min_key(address, key): the atomic minimum on
// the device, a plain one in the twin
template <class MinKey>
OCC4D_HD void splat_item(const PointArgs& a, int64_t e, int H, int W, int radius, unsigned long long* keys, MinKey min_key) {
  int v, i, px, py;
  float uvz[3];
  project_item(a, e, &v, &i, uvz);
  if (!centre_pixel(uvz, H, W, &px, &py)) return;
  const unsigned long long key = pack_key(uvz[2], (uint32_t)i);
  const int x0 = px - radius > 0 ? px - radius : 0, x1 = px + radius < W - 1 ? px + radius : W - 1;
  const int y0 = py - radius > 0 ? py - radius : 0, y1 = py + radius < H - 1 ? py + radius : H - 1;
  unsigned long long* image = keys + (int64_t)v * H * W;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) min_key(image + (int64_t)y * W + x, key);
}

OCC4D_HD void visibility_item(const PointArgs& a, int64_t e, const float* depth, int64_t ld_depth, int H, int W, float margin,
                              int32_t* code) {
  int v, i, px = 0, py = 0;
  float uvz[3];
  project_item(a, e, &v, &i, uvz);
  const bool inside = centre_pixel(uvz, H, W, &px, &py);
  const float d = inside ? depth[((int64_t)v * H + py) * ld_depth + px] : 0.f;
  code[e] = visibility_code(inside, uvz[2], d, margin);
}

struct ResolveArgs {
  const unsigned long long* keys;
  const float* rows; int64_t ld;
  float* depth; int32_t* index; float* feat;
  int64_t pixels;                         // V * H * W
  int n, C;
  float depth_background, feat_background;
  int32_t cols[MAX_CHANNELS];
};

// pixel p: the background values, or the key's depth, its row and that row's columns (the only access indexed by data)
OCC4D_HD void resolve_item(const ResolveArgs& r, int64_t p) {
  const unsigned long long key = r.keys[p];
  const bool background = key_is_background(key, r.n);
  if (r.depth) r.depth[p] = background ? r.depth_background : key_depth(key);
  if (r.index) r.index[p] = background ? -1 : (int32_t)key_row(key);
  if (r.C > 0) {
    float* f = r.feat + p * r.C;
    const float* src = background ? nullptr : r.rows + (int64_t)key_row(key) * r.ld;      // (key_row < n here)
    const float empty = r.feat_background;      // (a value, not a second address to choose from: `r` stays kernel arguments)
    for (int c = 0; c < r.C; ++c) f[c] = background ? empty : src[r.cols[c]];
  }
}

// ---- argument contracts (host): the status, `empty` = nothing to do, the pass's arguments filled
inline int check_points(const char* who, const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, bool& empty,
                        PointArgs& a) {
  OCC4D_REQUIRE(n >= 0 && V >= 0, "%s: n = %d, V = %d must be >= 0", who, n, V);
  OCC4D_REQUIRE(ld >= 3, "%s: ld = %lld must be >= 3", who, (long long)ld);
  a = PointArgs{rows, ld, rt, k, (int64_t)V * n, n};
  empty = n == 0 || V == 0;
  OCC4D_REQUIRE(empty || (rows && rt && k), "%s: null rows / rt / k", who);
  return OCC4D_OK;
}

inline int check_image(const char* who, int V, int H, int W) {
  OCC4D_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H = %d, W = %d must be in 1 .. %d", who, H, W, MAX_SIDE);
  OCC4D_REQUIRE((int64_t)V * H * W < ((int64_t)1 << 31), "%s: V H W = %lld must be < 2^31", who, (long long)V * H * W);
  return OCC4D_OK;
}

inline int check_project_points(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* uvz,
                                bool& empty, PointArgs& a) {
  const char* who = "occ4d_project_points_f32";
  OCC4D_TRY(check_points(who, rows, ld, n, rt, k, V, empty, a));
  OCC4D_REQUIRE(empty || uvz, "%s: null uvz", who);
  return OCC4D_OK;
}

inline int check_zbuffer_splat(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int H, int W, int radius,
                               const unsigned long long* keys, bool& empty, PointArgs& a) {
  const char* who = "occ4d_zbuffer_splat_f32";
  OCC4D_TRY(check_points(who, rows, ld, n, rt, k, V, empty, a));
  OCC4D_TRY(check_image(who, V, H, W));
  OCC4D_REQUIRE(radius >= 0 && radius <= MAX_RADIUS, "%s: radius = %d must be in 0 .. %d", who, radius, MAX_RADIUS);
  OCC4D_REQUIRE(empty || keys, "%s: null keys", who);
  return OCC4D_OK;
}

inline int check_zbuffer_resolve(const unsigned long long* keys, int V, int H, int W, const float* rows, int64_t ld, int n, int d,
                                 float depth_background, float* depth, int32_t* index, const int32_t* cols_host, int C,
                                 float feat_background, float* feat, bool& empty, ResolveArgs& r) {
  const char* who = "occ4d_zbuffer_resolve_f32";
  OCC4D_REQUIRE(n >= 0 && V >= 0, "%s: n = %d, V = %d must be >= 0", who, n, V);
  OCC4D_TRY(check_image(who, V, H, W));
  OCC4D_REQUIRE(C >= 0 && C <= MAX_CHANNELS, "%s: C = %d must be in 0 .. %d", who, C, MAX_CHANNELS);
  r = ResolveArgs{keys, rows, ld, depth, index, feat, (int64_t)V * H * W, n, C, depth_background, feat_background, {0}};
  if (C > 0) {
    OCC4D_REQUIRE(cols_host && feat, "%s: null cols_host / feat with C = %d", who, C);
    OCC4D_REQUIRE(d >= 1 && ld >= d, "%s: d = %d, ld = %lld: need 1 <= d <= ld", who, d, (long long)ld);
    OCC4D_REQUIRE(rows || n == 0, "%s: null rows with C = %d", who, C);
    for (int c = 0; c < C; ++c) {
      OCC4D_REQUIRE(cols_host[c] >= 0 && cols_host[c] < d, "%s: column %d must be in 0 .. d - 1 = %d", who, cols_host[c], d - 1);
      r.cols[c] = cols_host[c];
    }
  }
  empty = V == 0;
  OCC4D_REQUIRE(empty || keys, "%s: null keys", who);
  return OCC4D_OK;
}

inline int check_visibility(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* depth,
                            int64_t ld_depth, int H, int W, const int32_t* code, bool& empty, PointArgs& a) {
  const char* who = "occ4d_visibility_f32";
  OCC4D_TRY(check_points(who, rows, ld, n, rt, k, V, empty, a));
  OCC4D_TRY(check_image(who, V, H, W));
  OCC4D_REQUIRE(ld_depth >= W, "%s: ld_depth = %lld must be >= W = %d", who, (long long)ld_depth, W);
  OCC4D_REQUIRE(empty || (depth && code), "%s: null depth / code", who);
  return OCC4D_OK;
}

}  // namespace occ4d_project
