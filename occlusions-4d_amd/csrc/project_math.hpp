// Per-element decisions of the camera projection, the z-buffer and the visibility test (include/occ4d_project.h), shared WORD
// FOR WORD by the HIP kernels (csrc/project.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp).  Both are compiled with
// -ffp-contract=off: only the explicit fmaf() of row4 fuses.  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "frontend_math.hpp"      // row4: the fused chain of a (4, 4) @ (4, N) float32 product

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

}  // namespace occ4d_project
