// The decoded field scanned by a virtual lidar (include/ext/occ4d_sweep.h).  The ray, the gradient, the owner corner and the
// argument contract are csrc/sweep_math.hpp (the march under them is csrc/raycast_math.hpp's), shared with the g++ twin; the lane
// mapping and the launch are here.
//
// One thread per ray, 256-thread workgroups (four wave64), one launch: a workgroup takes 256 consecutive rays of a view, a wave 64
// of them -- in a (B, A) lidar table 64 neighbouring azimuths of one beam, whose rays fan out in one plane and stay in neighbouring
// cells.  Ragged ends are masked per thread.  The loop of a ray is bounded by n_steps and leaves on the hit; a wave runs as long as
// its longest ray; the gradient and the owner scan run once per ray after the loop.  No LDS, no atomics, no communication between
// threads: every output element has one owner, so the result depends on neither the stream nor the run.
//
// An 8 x 8 tile of the ray image per wave (the ray cast's pixel tiles) was measured
// against this mapping (profiles/r11_sweep_timing.txt): neither wins by more than the spread on every pattern -- the tiles are up to
// 6 % faster on one sensor inside the grid, this mapping up to 25 % faster with sensors outside it, where the tiles pack the few
// busy rays into few workgroups --, so the simpler one stays.
#include "common.hpp"
#include "sweep_math.hpp"
#include "ext/occ4d_sweep.h"

namespace {

namespace sw = occ4d_sweep;

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void sweep_kernel(const sw::Args a, const int blocks_per_view) {
  const int v = blockIdx.x / blocks_per_view, block = blockIdx.x % blocks_per_view;
  const int64_t r = (int64_t)block * THREADS + threadIdx.x;
  if (r < a.R) sw::ray_item(a, v, (int)r);
}

}  // namespace

extern "C" int occ4d_sweep_rays_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy,
                                    float z0, float sz, float level, const float* pose, const float* dirs, int V, int B, int A,
                                    int per_view, float near_range, float step, int n_steps, const float* attrs, int64_t ld_attr, int d,
                                    const int32_t* cols_host, int C, int sem_first, int n_sem, const int32_t* labels, int K,
                                    float range_background, float feat_background, float* range, float* point, int32_t* cell,
                                    int32_t* owner, float* cosine, int32_t* sem, int32_t* inst, float* feat, void* stream) {
  sw::Args a; bool empty;
  OCC4D_TRY(sw::check_sweep(field, ld, nx, ny, nz, x0, sx, y0, sy, z0, sz, level, pose, dirs, V, B, A, per_view, near_range, step, n_steps,
                            attrs, ld_attr, d, cols_host, C, sem_first, n_sem, labels, K, range_background, feat_background, range, point,
                            cell, owner, cosine, sem, inst, feat, empty, a));
  if (empty || sw::writes_nothing(a)) return OCC4D_OK;
  const int blocks = (int)(((int64_t)a.R + THREADS - 1) / THREADS);                    // V blocks <= V R < 2^31
  sweep_kernel<<<(unsigned)((int64_t)V * blocks), THREADS, 0, (hipStream_t)stream>>>(a, blocks);
  return occ4d::check_launch("occ4d_sweep_rays_f32");
}
