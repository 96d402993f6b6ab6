// Clouds into camera views (include/occ4d_project.h): the projection, the z-buffer in two passes (splat: one 64-bit atomic
// minimum per covered pixel; resolve: key image -> depth / index / gathered features) and the fused per-point visibility
// test.  Four element-wise, memory-bound kernels; the per-element decisions, the item bodies and the argument contracts are
// csrc/project_math.hpp, shared with the g++ twin: the loops, the atomic and the launches are here.
//
// 256-thread workgroups, a grid-stride loop, the grid capped as a function of the item count alone.  An item of the three
// point kernels is (view, row), views outermost: a wave reads consecutive rows and, but for the at most V - 1 waves that
// straddle two views, one camera (24 floats that stay in the cache).  An item of the resolve is a pixel.  The splat's
// atomicMin on unsigned long long is a vector global atomic without return; its target is computed from integers that
// project_math's centre_pixel produced from range-checked floats and that splat_item clips to the image again.  The
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

struct AtomicMin {
  __device__ void operator()(unsigned long long* dst, unsigned long long key) const { atomicMin(dst, key); }
};

__global__ __launch_bounds__(THREADS) void project_kernel(const pj::PointArgs a, const int flip_xy, float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step)
    pj::points_item(a, e, flip_xy != 0, out);
}

__global__ __launch_bounds__(THREADS) void splat_kernel(const pj::PointArgs a, const int H, const int W, const int radius,
                                                        unsigned long long* __restrict__ keys) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step)
    pj::splat_item(a, e, H, W, radius, keys, AtomicMin());
}

__global__ __launch_bounds__(THREADS) void visibility_kernel(const pj::PointArgs a, const float* __restrict__ depth,
                                                             const int64_t ld_depth, const int H, const int W,
                                                             const float margin, int32_t* __restrict__ code) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.items; e += step)
    pj::visibility_item(a, e, depth, ld_depth, H, W, margin, code);
}

__global__ __launch_bounds__(THREADS) void resolve_kernel(const pj::ResolveArgs r) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < r.pixels; p += step) pj::resolve_item(r, p);
}

}  // namespace

extern "C" int occ4d_project_points_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int flip_xy,
                                        float* uvz, void* stream) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_project_points(rows, ld, n, rt, k, V, uvz, empty, a));
  if (empty) return OCC4D_OK;
  project_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, flip_xy != 0, uvz);
  return occ4d::check_launch("occ4d_project_points_f32");
}

extern "C" int occ4d_zbuffer_splat_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int H, int W,
                                       int radius, unsigned long long* keys, void* stream) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_zbuffer_splat(rows, ld, n, rt, k, V, H, W, radius, keys, empty, a));
  if (empty) return OCC4D_OK;
  splat_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, H, W, radius, keys);
  return occ4d::check_launch("occ4d_zbuffer_splat_f32");
}

extern "C" int occ4d_zbuffer_resolve_f32(const unsigned long long* keys, int V, int H, int W, const float* rows, int64_t ld, int n,
                                         int d, float depth_background, float* depth, int32_t* index, const int32_t* cols_host,
                                         int C, float feat_background, float* feat, void* stream) {
  pj::ResolveArgs r; bool empty;
  OCC4D_TRY(pj::check_zbuffer_resolve(keys, V, H, W, rows, ld, n, d, depth_background, depth, index, cols_host, C, feat_background,
                                      feat, empty, r));
  if (empty) return OCC4D_OK;
  resolve_kernel<<<grid_for(r.pixels), THREADS, 0, (hipStream_t)stream>>>(r);
  return occ4d::check_launch("occ4d_zbuffer_resolve_f32");
}

extern "C" int occ4d_visibility_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* depth,
                                    int64_t ld_depth, int H, int W, float margin, int32_t* code, void* stream) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_visibility(rows, ld, n, rt, k, V, depth, ld_depth, H, W, code, empty, a));
  if (empty) return OCC4D_OK;
  visibility_kernel<<<grid_for(a.items), THREADS, 0, (hipStream_t)stream>>>(a, depth, ld_depth, H, W, margin, code);
  return occ4d::check_launch("occ4d_visibility_f32");
}
