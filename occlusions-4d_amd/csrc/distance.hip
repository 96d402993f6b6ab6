// The exact Euclidean distance transform of the grid's solid set (include/ext/occ4d_distance.h).  The rules, the order relation, a
// line's minimum, the tiling and the two item bodies are csrc/distance_math.hpp, shared with the g++ twin; the LDS tile, the barrier
// and the launches are here.
//
// Three launches of ONE kernel, whatever the data: the stages z, y, x of the header, the array viewed as (outer, L, inner).
//   A workgroup owns a tile of whole lines.  It stages their (cost, site) pairs in LDS -- stage z makes them from the site test, so
//   there is no member pass --, and after the barrier every thread takes, for each of its points, the minimum over the L candidates of
//   the point's line under the order (cost, then the lower axis index), and writes it IN PLACE into dist2 / nearest: the workgroup
//   has read every line it writes, and no other workgroup touches them.  No work array.
//   Stage z: the tile is a contiguous run of max(1, 1024 / nz) lines; the lanes of one line read the same LDS word (a broadcast).
//   Stages y, x: the tile is L x T with T consecutive `inner` indices, T = 16 halved until L * T <= 4096 (two int32 per point: 32 KiB
//   at most; the project's L <= 96 runs at T = 16 with 12 KiB, several workgroups per CU).  Global access is coalesced along `inner`
//   in pieces of T words, and the LDS reads [l'][t] of a wave are T consecutive words read by four rows of lanes: conflict-free.
//   T = 64 gave the 96 x 96 x 58 grid 96 and 87 workgroups for 256 CUs, and 0.17 ms for the three launches; T = 16 gives it 384 and 348.
// A plain minimum over the line and not the lower-envelope algorithm, which is serial per line and data-dependent: here every point
// does the same L steps, without a branch or a product (distance_math.hpp: line_min).  Only the winner's axis index is tracked in
// the loop; its site is one LDS read at the end.
// No atomics, no inter-workgroup waits, no inline assembly, no floats beyond the member comparison.
#include "common.hpp"
#include "distance_math.hpp"
#include "ext/occ4d_distance.h"

namespace {

namespace dm = occ4d_distance;

constexpr int THREADS = 256;              // a tile is about 1024 points (stage z), up to 4096 (stages y, x; 1536 at L = 96)

__global__ __launch_bounds__(THREADS) void distance_pass_kernel(const dm::Args a, const dm::Pass ps) {
  extern __shared__ int32_t s_tile[];
  const int slots = dm::tile_slots(ps);
  int32_t* s_cost = s_tile;
  int32_t* s_site = a.nearest ? s_tile + slots : nullptr;
  const dm::Tile t = dm::tile_of(ps, blockIdx.x);
  for (int s = threadIdx.x; s < slots; s += THREADS) dm::stage_item(a, ps, t, s, s_cost, s_site);
  __syncthreads();
  for (int s = threadIdx.x; s < slots; s += THREADS) dm::min_item(a, ps, t, s, s_cost, s_site);
}

void launch(const dm::Args& a, int stage, hipStream_t st) {
  const dm::Pass ps = dm::pass_of(a, stage, 0);
  const size_t lds = (size_t)dm::tile_slots(ps) * sizeof(int32_t) * (a.nearest ? 2 : 1);       // <= 32 KiB (distance_math.hpp)
  distance_pass_kernel<<<(unsigned)ps.tiles, THREADS, lds, st>>>(a, ps);              // tiles <= 512 * 512 * 512 / 8
}

}  // namespace

extern "C" int occ4d_distance_grid_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                                       int target, int nx, int ny, int nz, int wx, int wy, int wz, int32_t* dist2, int32_t* nearest,
                                       void* stream) {
  dm::Args a; bool empty;
  OCC4D_TRY(dm::check_distance(field, ld, level, mask, ld_mask, mask_level, target, nx, ny, nz, wx, wy, wz, dist2, nearest, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  for (int stage = 0; stage < 3; ++stage) launch(a, stage, st);
  return occ4d::check_launch("occ4d_distance_grid_f32");
}
