// Per-element arithmetic of the clip front end (include/occ4d_frontend.h), the lidar row and the two entry points' argument
// contracts (host only), shared WORD FOR WORD by the HIP kernels (csrc/frontend.hip) and the g++ twin
// (csrc_cpu/occ4d_twin.cpp): both are compiled with -ffp-contract=off, so only the explicit fmaf() below fuses and the two
// agree bit for bit with each other and with the reference's numpy results.
#pragma once
#include <math.h>
#include <stdint.h>

#include "contract.hpp"

#if defined(__HIPCC__)
#define OCC4D_HD __host__ __device__ __forceinline__
#else
#define OCC4D_HD inline
#endif

namespace occ4d_frontend {

// Row i of a (4, 4) float32 matrix times a column (b0 .. b3): np.matmul / np.dot of a (4, 4) with a (4, N) operand
// accumulates k = 0 .. 3 ascending with fused multiply-adds, the first product rounded on its own.  Probe (numpy 2.2 /
// OpenBLAS 0.3.29, this expression compiled by g++ -ffp-contract=off against the four products of one 240 x 320 frame
// and one 76 800-row sweep, compared bitwise): this chain 100 % in all four; ascending multiply-then-add 76 - 82 %,
// the descending fused chain 55 - 65 % in the three products with dense operands (K^-1 has two non-zero terms per row
// and separates less: 100 % / 75 %).  DESIGN 7c rank 5 has the table.
// EXCEPTION: a (4, 4) @ (4, 1) product -- a frame with exactly ONE valid pixel, a sweep of one row -- takes numpy's
// matrix-vector path with another summation order (88 % of such columns differ in a bit); the fixtures hold no such frame.
OCC4D_HD float row4(const float* __restrict__ a, float b0, float b1, float b2, float b3) {
  return fmaf(a[3], b3, fmaf(a[2], b2, fmaf(a[1], b1, a[0] * b0)));
}

// point_cloud_from_pixel_coords: K^-1 (x, y, 1, 1), the first three scaled by the depth (rounded on their own, the
// fourth not scaled), then RT^-1 of that; the first three components are the world point.
OCC4D_HD void unproject(const float* __restrict__ k_inv, const float* __restrict__ rt_inv, float px, float py, float z,
                        float* __restrict__ xyz) {
  const float s0 = row4(k_inv + 0, px, py, 1.f, 1.f) * z;
  const float s1 = row4(k_inv + 4, px, py, 1.f, 1.f) * z;
  const float s2 = row4(k_inv + 8, px, py, 1.f, 1.f) * z;
  const float s3 = row4(k_inv + 12, px, py, 1.f, 1.f);
  xyz[0] = row4(rt_inv + 0, s0, s1, s2, s3);
  xyz[1] = row4(rt_inv + 4, s0, s1, s2, s3);
  xyz[2] = row4(rt_inv + 8, s0, s1, s2, s3);
}

// filter_pcl_bounds_numpy: inclusive fp32 comparisons; floor_fix: z > (max(|x|, |y|) - 4.5) / 3.5, a true division.
OCC4D_HD bool in_cuboid(const float* xyz, float x_min, float x_max, float y_min, float y_max, float z_min, float z_max,
                        bool floor_fix) {
  bool keep = x_min <= xyz[0] && xyz[0] <= x_max && y_min <= xyz[1] && xyz[1] <= y_max && z_min <= xyz[2] && xyz[2] <= z_max;
  if (floor_fix) {
    const float pyramid = fmaxf(fabsf(xyz[0]), fabsf(xyz[1]));
    keep = keep && xyz[2] > (pyramid - 4.5f) / 3.5f;
  }
  return keep;
}

// matplotlib.colors.rgb_to_hsv on float32, hue and saturation only.  A later channel that equals the maximum overrides
// an earlier one (blue over green over red), as the reference's three masked assignments do; `% 1.0` is numpy's
// remainder (sign of the divisor, +0 for a zero result).
OCC4D_HD void hue_sat(float r, float g, float b, float* hue, float* sat) {
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const float delta = mx - mn;
  *sat = mx > 0.f ? delta / mx : 0.f;
  float q = 0.f;
  if (delta > 0.f) {
    if (b == mx) q = 4.f + (r - g) / delta;
    else if (g == mx) q = 2.f + (b - r) / delta;
    else q = (g - b) / delta;
  }
  float m = fmodf(q / 6.0f, 1.0f);
  if (m != 0.f) {
    if (m < 0.f) m += 1.0f;
  } else {
    m = 0.f;
  }
  *hue = m;
}

// data/data_greater.py:394-399: np.round(h * 360) (half to even), first argmin of |. - cluster| (the reference subtracts
// its integer list from the float32 value in float64), -1 where the saturation is below 0.9.
OCC4D_HD float instance_id(float r, float g, float b, const float* __restrict__ clusters, int n_clusters) {
  float h, s;
  hue_sat(r, g, b, &h, &s);
  if (s < 0.9f) return -1.f;
  const double deg = (double)rintf(h * 360.0f);
  int best = 0;
  double best_d = fabs(deg - (double)clusters[0]);
  for (int c = 1; c < n_clusters; ++c) {
    const double dist = fabs(deg - (double)clusters[c]);
    if (dist < best_d) { best_d = dist; best = c; }
  }
  return (float)best;
}

// transform_lidar_frame: source (x, y, z, 1), then inv(target) of ALL FOUR components of that, each stage rounded.
OCC4D_HD void lidar_transform(const float* __restrict__ source, const float* __restrict__ inv_target, float* xyz) {
  const float w0 = row4(source + 0, xyz[0], xyz[1], xyz[2], 1.f);
  const float w1 = row4(source + 4, xyz[0], xyz[1], xyz[2], 1.f);
  const float w2 = row4(source + 8, xyz[0], xyz[1], xyz[2], 1.f);
  const float w3 = row4(source + 12, xyz[0], xyz[1], xyz[2], 1.f);
  xyz[0] = row4(inv_target + 0, w0, w1, w2, w3);
  xyz[1] = row4(inv_target + 4, w0, w1, w2, w3);
  xyz[2] = row4(inv_target + 8, w0, w1, w2, w3);
}

// filter_pcl_bounds_carla_input_numpy: the six bounds of cube_mode 1 .. 4, formed in double as the reference's Python
// floats are and rounded to float32 where numpy compares them with the float32 coordinates.
struct Cuboid { float x_min, x_max, y_min, y_max, z_min, z_max; };
inline Cuboid carla_input_cuboid(int cube_mode, double min_z, double ob) {
  const double x_lo[5] = {0, 0.5, 0.6, 0.7, 0.7}, x_hi[5] = {0, 2.0, 2.4, 2.2, 2.5}, y_hi[5] = {0, 1.0, 0.8, 1.0, 1.0},
               z_hi[5] = {0, 0.5, 0.6, 0.5, 0.5};
  return Cuboid{(float)(-ob * x_lo[cube_mode]), (float)(ob * x_hi[cube_mode]), (float)(-ob * y_hi[cube_mode]),
                (float)(ob * y_hi[cube_mode]), (float)min_z, (float)(ob * z_hi[cube_mode])};
}

// one lidar row i: the optional transform and ground offset on x, y, z, the other d - 3 columns copied, the cuboid key
OCC4D_HD void lidar_row(const float* __restrict__ rows, int64_t ld, int d, const float* source, const float* inv_target,
                        bool transform, float z_offset, bool filter, const Cuboid& c, float* __restrict__ out, int64_t ldo,
                        float* __restrict__ key, int64_t i) {
  const float* src = rows + i * ld;
  float* dst = out + i * ldo;
  float xyz[3] = {src[0], src[1], src[2]};
  if (transform) lidar_transform(source, inv_target, xyz);
  if (z_offset != 0.f) xyz[2] += z_offset;
  dst[0] = xyz[0]; dst[1] = xyz[1]; dst[2] = xyz[2];
  for (int k = 3; k < d; ++k) dst[k] = src[k];
  key[i] = (!filter || in_cuboid(xyz, c.x_min, c.x_max, c.y_min, c.y_max, c.z_min, c.z_max, false)) ? 1.f : 0.f;
}

// ---- argument contracts (host): the status, and what the call covers
constexpr int MAX_CLUSTERS = 64;

// total = T * H * W pixels; 0: nothing to do (libocc4d.so checks its outputs' alignment before it says so)
inline int check_rgbd_rows(const float* depth, const float* rgb, const float* flat, const float* k_inv, const float* rt_inv,
                           const float* hue_clusters, int n_clusters, int T, int H, int W, const float* out_rows,
                           const float* out_key, int64_t& total) {
  OCC4D_REQUIRE(depth && rgb && k_inv && rt_inv && out_rows && out_key, "occ4d_rgbd_rows_f32: null pointer");
  OCC4D_REQUIRE(T >= 0 && H >= 1 && W >= 1 && (int64_t)T * H * W < ((int64_t)1 << 31), "occ4d_rgbd_rows_f32: T = %d, H = %d, W = %d", T, H, W);
  OCC4D_REQUIRE(!flat || (hue_clusters && n_clusters >= 1 && n_clusters <= MAX_CLUSTERS),
                "occ4d_rgbd_rows_f32: n_clusters = %d must be in 1 .. %d", n_clusters, MAX_CLUSTERS);
  total = (int64_t)T * H * W;
  return OCC4D_OK;
}

inline int check_lidar_rows(const float* rows, int64_t ld, int n, int d, const float* source, const float* inv_target, int cube_mode,
                            const float* out_rows, int64_t ldo, const float* out_key, bool& empty) {
  OCC4D_REQUIRE(rows && out_rows && out_key, "occ4d_lidar_rows_f32: null pointer");
  OCC4D_REQUIRE(n >= 0 && d >= 3 && ld >= d && ldo >= d, "occ4d_lidar_rows_f32: n = %d, d = %d, ld = %lld, ldo = %lld", n, d,
                (long long)ld, (long long)ldo);
  OCC4D_REQUIRE((source != nullptr) == (inv_target != nullptr), "occ4d_lidar_rows_f32: source and inv_target go together");
  OCC4D_REQUIRE(cube_mode >= 0 && cube_mode <= 4, "occ4d_lidar_rows_f32: cube_mode %d (0 = no filter, 1 .. 4)", cube_mode);
  empty = n == 0;
  return OCC4D_OK;
}

}  // namespace occ4d_frontend
