// The clip front end (include/occ4d_frontend.h): RGB-D frames / lidar sweeps -> cloud rows + keep keys.  Element-wise,
// one thread per pixel / lidar row, every access behind a bounds check, no shared state.  The arithmetic, the lidar row and
// the argument contracts are csrc/frontend_math.hpp, shared with the g++ twin.
#include "common.hpp"
#include "frontend_math.hpp"
#include "occ4d_frontend.h"

namespace {

namespace fe = occ4d_frontend;

constexpr int MAX_CLUSTERS = fe::MAX_CLUSTERS;

struct RgbdArgs {
  const float* depth; const float* rgb; const float* flat; const float* k_inv; const float* rt_inv; const float* clusters;
  int n_clusters, H, W;
  int64_t total;              // T * H * W
  float x_min, x_max, y_min, y_max, z_min, z_max;
  int floor_fix;
  float view;
  float* rows; float* target; float* key;
};

__global__ __launch_bounds__(256) void rgbd_rows_kernel(const RgbdArgs a) {
  __shared__ float s_clusters[MAX_CLUSTERS];
  if ((int)threadIdx.x < a.n_clusters) s_clusters[threadIdx.x] = a.clusters[threadIdx.x];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.total) return;
  const int hw = a.H * a.W;
  const int t = (int)(p / hw), pix = (int)(p % hw);
  const int py = pix / a.W, px = pix % a.W;
  const float z = a.depth[p];
  float xyz[3];
  fe::unproject(a.k_inv + 16 * t, a.rt_inv + 16 * t, (float)px, (float)py, z, xyz);
  const bool keep = z > 0.f && fe::in_cuboid(xyz, a.x_min, a.x_max, a.y_min, a.y_max, a.z_min, a.z_max, a.floor_fix != 0);
  const float r = a.rgb[3 * p], g = a.rgb[3 * p + 1], b = a.rgb[3 * p + 2];
  const float inst = a.flat ? fe::instance_id(a.flat[3 * p], a.flat[3 * p + 1], a.flat[3 * p + 2], s_clusters, a.n_clusters) : -1.f;
  float4* row = reinterpret_cast<float4*>(a.rows + 8 * p);             // (8 floats per row: 32-byte aligned)
  row[0] = make_float4(xyz[0], xyz[1], xyz[2], inst);
  row[1] = make_float4(r, g, b, (float)t);
  if (a.target) {
    float4* tgt = reinterpret_cast<float4*>(a.target + 8 * p);
    tgt[0] = make_float4(xyz[0], xyz[1], xyz[2], inst);
    tgt[1] = make_float4(a.view, r, g, b);
  }
  a.key[p] = keep ? 1.f : 0.f;
}

struct Mat4 { float m[16]; };

__global__ __launch_bounds__(256) void lidar_rows_kernel(const float* __restrict__ rows, int64_t ld, int n, int d, const Mat4 source,
                                                         const Mat4 inv_target, int transform, float z_offset, int filter,
                                                         const fe::Cuboid c, float* __restrict__ out, int64_t ldo,
                                                         float* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe::lidar_row(rows, ld, d, source.m, inv_target.m, transform != 0, z_offset, filter != 0, c, out, ldo, key, i);
}

}  // namespace

extern "C" int occ4d_rgbd_rows_f32(const float* depth, const float* rgb, const float* flat, const float* k_inv, const float* rt_inv,
                                   const float* hue_clusters, int n_clusters, int T, int H, int W, float x_min, float x_max,
                                   float y_min, float y_max, float z_min, float z_max, int floor_fix, int view_idx,
                                   float* out_rows, float* out_target, float* out_key, void* stream) {
  int64_t total;
  OCC4D_TRY(fe::check_rgbd_rows(depth, rgb, flat, k_inv, rt_inv, hue_clusters, n_clusters, T, H, W, out_rows, out_key, total));
  OCC4D_REQUIRE(((uintptr_t)out_rows % 16) == 0 && (!out_target || ((uintptr_t)out_target % 16) == 0),
                "occ4d_rgbd_rows_f32: output rows must be 16-byte aligned");
  if (total == 0) return OCC4D_OK;
  const RgbdArgs a{depth, rgb, flat, k_inv, rt_inv, hue_clusters, flat ? n_clusters : 0, H, W, total, x_min, x_max, y_min, y_max,
                   z_min, z_max, floor_fix, (float)view_idx, out_rows, out_target, out_key};
  rgbd_rows_kernel<<<occ4d::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch("occ4d_rgbd_rows_f32");
}

// `source` / `inv_target` are 64-byte HOST matrices passed by value in the kernel arguments (no upload, no extra launch)
extern "C" int occ4d_lidar_rows_f32(const float* rows, int64_t ld, int n, int d, const float* source, const float* inv_target,
                                    float z_offset, int cube_mode, double min_z, double other_bounds, float* out_rows,
                                    int64_t ldo, float* out_key, void* stream) {
  bool empty;
  OCC4D_TRY(fe::check_lidar_rows(rows, ld, n, d, source, inv_target, cube_mode, out_rows, ldo, out_key, empty));
  if (empty) return OCC4D_OK;
  Mat4 s{}, it{};
  if (source) {
    for (int k = 0; k < 16; ++k) { s.m[k] = source[k]; it.m[k] = inv_target[k]; }
  }
  const fe::Cuboid c = fe::carla_input_cuboid(cube_mode, min_z, other_bounds);
  lidar_rows_kernel<<<occ4d::cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(rows, ld, n, d, s, it, source ? 1 : 0, z_offset,
                                                                         cube_mode != 0, c, out_rows, ldo, out_key);
  return occ4d::check_launch("occ4d_lidar_rows_f32");
}
