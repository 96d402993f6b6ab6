// Line of sight through the grid's solid set (include/ext/occ4d_sight.h).  The rules, the bit test, the choice of T, the SQUEEZE, the
// walk and the body of a query are csrc/sight_math.hpp, shared with the g++ twin; the ballots, the blocks of a workgroup and the
// launches are here.
//
// One launch per entry point, whatever the data.
//   bits   one thread per grid point, the member test, a ballot: lanes 0 and 32 of a wave store its two words.  Lanes behind n vote 0,
//          which clears the unused bits of the last word.
//   walk   one thread per query, a wave owns a compact 4 x 4 x 4 block of them, a workgroup four neighbouring blocks: towards one
//          origin a wave's 64 walks cross neighbouring cells, so their lengths and the words they read stay together.  The thread
//          loops over the V origins (kernel arguments: scalar loads), gathers the seen bits in a register and stores once per
//          output.  Every bit is read from global memory: the whole array is 67 KB at 96 x 96 x 58 and stays in the caches.
//          A second variant -- persistent workgroups of 1024 threads, two to a CU, each with a copy of the whole array in 80 KiB of
//          LDS -- was built and timed in the same runs: 1.04 - 1.37 x the time of this one on every field, every origin set (DESIGN 7c
//          rank 19 has the figures), so it is gone.
// No atomics, no LDS, no inter-workgroup waits, no inline assembly, no floats beyond the member comparison.
#include "common.hpp"
#include "sight_math.hpp"
#include "ext/occ4d_sight.h"

namespace {

namespace sm = occ4d_sight;

constexpr int FLAT = 256;
constexpr int WAVES = FLAT / 64;

__global__ __launch_bounds__(FLAT) void sight_bits_kernel(const sm::BitsArgs a) {
  const int64_t p = (int64_t)blockIdx.x * FLAT + threadIdx.x;
  const unsigned long long votes = __ballot(p < a.n && sm::member(a, p));
  const int lane = threadIdx.x & 63;
  const int64_t word = p >> 5;                                    // (p of lanes 0 and 32 is a multiple of 32)
  if ((lane & 31) == 0 && word < a.words) a.bits[word] = (uint32_t)(votes >> lane);
}

__global__ __launch_bounds__(FLAT) void sight_walk_kernel(const sm::Args a) {
  const int64_t k = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  int x, y, z;
  if (k < a.blocks && sm::block_query(a, k, threadIdx.x & 63, x, y, z)) sm::query_item(a, sm::GlobalWords{a.bits}, x, y, z);
}

}  // namespace

extern "C" int occ4d_sight_bits_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                                    int64_t n, uint32_t* bits, void* stream) {
  sm::BitsArgs a; bool empty;
  OCC4D_TRY(sm::check_bits(field, ld, level, mask, ld_mask, mask_level, n, bits, empty, a));
  if (empty) return OCC4D_OK;
  sight_bits_kernel<<<(unsigned)((n + FLAT - 1) / FLAT), FLAT, 0, (hipStream_t)stream>>>(a);
  return occ4d::check_launch("occ4d_sight_bits_f32");
}

extern "C" int occ4d_sight_grid_u32(const uint32_t* bits, int nx, int ny, int nz, const int32_t* origins_host, int V,
                                    const int32_t* framed, int32_t* seen, int32_t* blocker, int flags, void* stream) {
  sm::Args a; bool empty;
  OCC4D_TRY(sm::check_grid(bits, nx, ny, nz, origins_host, V, framed, seen, blocker, flags, empty, a));
  if (empty) return OCC4D_OK;
  sight_walk_kernel<<<(unsigned)((a.blocks + WAVES - 1) / WAVES), FLAT, 0, (hipStream_t)stream>>>(a);       // blocks <= 128^3
  return occ4d::check_launch("occ4d_sight_grid_u32");
}
