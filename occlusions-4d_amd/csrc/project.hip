// Clouds into camera views (include/occ4d_project.h): the projection, the z-buffer in two passes (splat: one 64-bit atomic
// minimum per covered pixel; resolve: key image -> depth / index / gathered features) and the fused per-point visibility
// test.  Four element-wise, memory-bound kernels; the per-element decisions are csrc/project_math.hpp, shared with the g++ twin.
//
// 256-thread workgroups, a grid-stride loop, the grid capped as a function of the item count alone.  An item of the three
// point kernels is (view, row), views outermost: a wave reads consecutive rows and, but for the at most V - 1 waves that
// straddle two views, one camera (24 floats that stay in the cache).  An item of the resolve is a pixel.  The splat's
// atomicMin on unsigned long long is a vector global atomic without return; its target is computed from integers that
// project_math's centre_pixel produced from range-checked floats and that are clipped to the image again here.  The
// resolve's gather is the only access indexed by data and runs behind `index < n`.  No LDS, no inline assembly.
#include "common.hpp"
#include "project_math.hpp"
#include "occ4d_project.h"

namespace {

namespace pj = occ4d_project;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more items than GRID_CAP * THREADS: further trips of the loop

inline int grid_for(int64_t items) {
  const int64_t blocks = (items + THREADS - 1) / THREADS;
  return (int)(blocks < GRID_CAP ? blocks : GRID_CAP);
}

struct PointArgs {
  const float* rows; int64_t ld;
  const float* rt; const float* k;
  int64_t items;                          // V * n
  int n;
};

// item e = (view, row) -> (u, v, depth)
__device__ __forceinline__ void project_item(const PointArgs& a, int64_t e, int* view, int* row, float* uvz) {
  const int v = (int)(e / a.n);
  const int i = (int)(e - (int64_t)v * a.n);
  const float* p = a.rows + (int64_t)i * a.ld;
  pj::project(a.rt + 16 * v, a.k + 16 * v, p[0], p[1], p[2], uvz);
  *view = v;
  *row = i;
}

__global__ __launch_bounds__(THREADS) void project_kernel(const PointArgs a, const int flip_xy, float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step) {
    int v, i;
    float uvz[3];
    project_item(a, e, &v, &i, uvz);
    float* o = out + 3 * e;
    o[0] = flip_xy ? uvz[1] : uvz[0];
    o[1] = flip_xy ? uvz[0] : uvz[1];
    o[2] = uvz[2];
  }
}

__global__ __launch_bounds__(THREADS) void splat_kernel(const PointArgs a, const int H, const int W, const int radius,
                                                        unsigned long long* __restrict__ keys) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step) {
    int v, i, px, py;
    float uvz[3];
    project_item(a, e, &v, &i, uvz);
    if (!pj::centre_pixel(uvz, H, W, &px, &py)) continue;
    const unsigned long long key = pj::pack_key(uvz[2], (uint32_t)i);
    const int x0 = max(px - radius, 0), x1 = min(px + radius, W - 1);
    const int y0 = max(py - radius, 0), y1 = min(py + radius, H - 1);
    unsigned long long* image = keys + (int64_t)v * H * W;
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x) atomicMin(image + (int64_t)y * W + x, key);
  }
}

__global__ __launch_bounds__(THREADS) void visibility_kernel(const PointArgs a, const float* __restrict__ depth,
                                                             const int64_t ld_depth, const int H, const int W,
                                                             const float margin, int32_t* __restrict__ code) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step) {
    int v, i, px = 0, py = 0;
    float uvz[3];
    project_item(a, e, &v, &i, uvz);
    const bool inside = pj::centre_pixel(uvz, H, W, &px, &py);
    const float d = inside ? depth[((int64_t)v * H + py) * ld_depth + px] : 0.f;
    code[e] = pj::visibility_code(inside, uvz[2], d, margin);
  }
}

struct ResolveArgs {
  const unsigned long long* keys;
  const float* rows; int64_t ld;
  float* depth; int32_t* index; float* feat;
  int64_t pixels;                         // V * H * W
  int n, C;
  float depth_background, feat_background;
  int32_t cols[pj::MAX_CHANNELS];
};

__global__ __launch_bounds__(THREADS) void resolve_kernel(const ResolveArgs r) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < r.pixels; p += step) {
    const unsigned long long key = r.keys[p];
    const bool background = pj::key_is_background(key, r.n);
    if (r.depth) r.depth[p] = background ? r.depth_background : pj::key_depth(key);
    if (r.index) r.index[p] = background ? -1 : (int32_t)pj::key_row(key);
    if (r.C > 0) {
      float* f = r.feat + p * r.C;
      const float* src = background ? nullptr : r.rows + (int64_t)pj::key_row(key) * r.ld;      // (key_row < n here)
      for (int c = 0; c < r.C; ++c) f[c] = background ? r.feat_background : src[r.cols[c]];
    }
  }
}

int check_points(const char* who, const float* rows, int64_t ld, int n, const float* rt, const float* k, int V) {
  OCC4D_REQUIRE(n >= 0 && V >= 0, "%s: n = %d, V = %d must be >= 0", who, n, V);
  OCC4D_REQUIRE(ld >= 3, "%s: ld = %lld must be >= 3", who, (long long)ld);
  if (n == 0 || V == 0) return OCC4D_OK;
  OCC4D_REQUIRE(rows && rt && k, "%s: null rows / rt / k", who);
  return OCC4D_OK;
}

int check_image(const char* who, int V, int H, int W) {
  OCC4D_REQUIRE(H >= 1 && W >= 1 && H <= pj::MAX_SIDE && W <= pj::MAX_SIDE, "%s: H = %d, W = %d must be in 1 .. %d", who, H, W,
                pj::MAX_SIDE);
  OCC4D_REQUIRE((int64_t)V * H * W < ((int64_t)1 << 31), "%s: V H W = %lld must be < 2^31", who, (long long)V * H * W);
  return OCC4D_OK;
}

}  // namespace

extern "C" int occ4d_project_points_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int flip_xy,
                                        float* uvz, void* stream) {
  const char* who = "occ4d_project_points_f32";
  if (int rc = check_points(who, rows, ld, n, rt, k, V)) return rc;
  if (n == 0 || V == 0) return OCC4D_OK;
  OCC4D_REQUIRE(uvz, "%s: null uvz", who);
  const PointArgs a{rows, ld, rt, k, (int64_t)V * n, n};
  project_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, flip_xy != 0, uvz);
  return occ4d::check_launch(who);
}

extern "C" int occ4d_zbuffer_splat_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int H, int W,
                                       int radius, unsigned long long* keys, void* stream) {
  const char* who = "occ4d_zbuffer_splat_f32";
  if (int rc = check_points(who, rows, ld, n, rt, k, V)) return rc;
  if (int rc = check_image(who, V, H, W)) return rc;
  OCC4D_REQUIRE(radius >= 0 && radius <= pj::MAX_RADIUS, "%s: radius = %d must be in 0 .. %d", who, radius, pj::MAX_RADIUS);
  if (n == 0 || V == 0) return OCC4D_OK;
  OCC4D_REQUIRE(keys, "%s: null keys", who);
  const PointArgs a{rows, ld, rt, k, (int64_t)V * n, n};
  splat_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, H, W, radius, keys);
  return occ4d::check_launch(who);
}

extern "C" int occ4d_zbuffer_resolve_f32(const unsigned long long* keys, int V, int H, int W, const float* rows, int64_t ld, int n,
                                         int d, float depth_background, float* depth, int32_t* index, const int32_t* cols_host,
                                         int C, float feat_background, float* feat, void* stream) {
  const char* who = "occ4d_zbuffer_resolve_f32";
  OCC4D_REQUIRE(n >= 0 && V >= 0, "%s: n = %d, V = %d must be >= 0", who, n, V);
  if (int rc = check_image(who, V, H, W)) return rc;
  OCC4D_REQUIRE(C >= 0 && C <= pj::MAX_CHANNELS, "%s: C = %d must be in 0 .. %d", who, C, pj::MAX_CHANNELS);
  ResolveArgs r{keys, rows, ld, depth, index, feat, (int64_t)V * H * W, n, C, depth_background, feat_background, {0}};
  if (C > 0) {
    OCC4D_REQUIRE(cols_host && feat, "%s: null cols_host / feat with C = %d", who, C);
    OCC4D_REQUIRE(d >= 1 && ld >= d, "%s: d = %d, ld = %lld: need 1 <= d <= ld", who, d, (long long)ld);
    OCC4D_REQUIRE(rows || n == 0, "%s: null rows with C = %d", who, C);
    for (int c = 0; c < C; ++c) {
      OCC4D_REQUIRE(cols_host[c] >= 0 && cols_host[c] < d, "%s: column %d must be in 0 .. d - 1 = %d", who, cols_host[c], d - 1);
      r.cols[c] = cols_host[c];
    }
  }
  if (V == 0) return OCC4D_OK;
  OCC4D_REQUIRE(keys, "%s: null keys", who);
  resolve_kernel<<<grid_for(r.pixels), THREADS, 0, (hipStream_t)stream>>>(r);
  return occ4d::check_launch(who);
}

extern "C" int occ4d_visibility_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* depth,
                                    int64_t ld_depth, int H, int W, float margin, int32_t* code, void* stream) {
  const char* who = "occ4d_visibility_f32";
  if (int rc = check_points(who, rows, ld, n, rt, k, V)) return rc;
  if (int rc = check_image(who, V, H, W)) return rc;
  OCC4D_REQUIRE(ld_depth >= W, "%s: ld_depth = %lld must be >= W = %d", who, (long long)ld_depth, W);
  if (n == 0 || V == 0) return OCC4D_OK;
  OCC4D_REQUIRE(depth && code, "%s: null depth / code", who);
  const PointArgs a{rows, ld, rt, k, (int64_t)V * n, n};
  visibility_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, depth, ld_depth, H, W, margin, code);
  return occ4d::check_launch(who);
}
