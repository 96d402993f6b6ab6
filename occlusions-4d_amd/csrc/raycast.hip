// The decoded field ray-cast into camera views (include/ext/occ4d_raycast.h).  The ray, the march, the trilinear value and the
// argument contract are csrc/raycast_math.hpp, shared with the g++ twin; the tiling and the launch are here.
//
// One thread per pixel, 256-thread workgroups (four wave64) over tiles of 16 x 16 pixels; each wave owns an 8 x 8 sub-tile, so
// the rays of a wave stay in neighbouring cells and their eight corner reads per sample fall into few cache lines (a gather:
// the field is a 2 MB column at the published grid and stays in L2).  Ragged image edges are masked per thread.  The loop of a
// ray is bounded by n_steps and leaves on the hit; a wave runs as long as its longest ray.  No LDS, no atomics, no communication
// between threads: every output element has one owner, so the result depends on neither the stream nor the run.
#include "common.hpp"
#include "raycast_math.hpp"
#include "ext/occ4d_raycast.h"

namespace {

namespace rc = occ4d_raycast;

constexpr int THREADS = 256;
constexpr int TILE = 16;                  // pixels per workgroup edge
constexpr int SUB = 8;                    // pixels per wave edge
static_assert(TILE * TILE == THREADS && SUB * SUB == 64 && TILE == 2 * SUB, "four 8 x 8 waves per 16 x 16 tile");

__global__ __launch_bounds__(THREADS) void raycast_kernel(const rc::Args a, const int tiles_x, const int tiles_y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x % (tiles_x * tiles_y), v = blockIdx.x / (tiles_x * tiles_y);
  const int px = (tile % tiles_x) * TILE + (wave & 1) * SUB + (lane & (SUB - 1));
  const int py = (tile / tiles_x) * TILE + (wave >> 1) * SUB + (lane / SUB);
  if (px < a.W && py < a.H) rc::pixel_item(a, v, px, py);
}

}  // namespace

extern "C" int occ4d_raycast_grid_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy,
                                      float z0, float sz, float level, const float* k_inv, const float* rt_inv, int V, int H, int W,
                                      float near_depth, float step, int n_steps, const float* attrs, int64_t ld_attr, int d,
                                      const int32_t* cols_host, int C, float depth_background, float feat_background, float* depth,
                                      int32_t* cell, float* feat, void* stream) {
  rc::Args a; bool empty;
  OCC4D_TRY(rc::check_raycast(field, ld, nx, ny, nz, x0, sx, y0, sy, z0, sz, level, k_inv, rt_inv, V, H, W, near_depth, step, n_steps,
                              attrs, ld_attr, d, cols_host, C, depth_background, feat_background, depth, cell, feat, empty, a));
  if (empty || (!a.depth && !a.cell && !a.feat)) return OCC4D_OK;
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;      // V tiles_x tiles_y <= V H W < 2^31
  raycast_kernel<<<(unsigned)((int64_t)V * tiles_x * tiles_y), THREADS, 0, (hipStream_t)stream>>>(a, tiles_x, tiles_y);
  return occ4d::check_launch("occ4d_raycast_grid_f32");
}
