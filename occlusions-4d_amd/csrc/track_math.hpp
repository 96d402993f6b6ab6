// Per-element decisions of the running track merge (include/occ4d_track.h), shared WORD FOR WORD by the HIP kernels
// (csrc/trackmerge.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): the per-channel squash and the winner / best update with
// numpy's NaN rule.  All arithmetic is fp32.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OCC4D_TRACK_HD __host__ __device__ __forceinline__
#else
#define OCC4D_TRACK_HD inline
#endif

namespace occ4d_track {

// the g <= 32 squash codes (0 identity, 1 sigmoid, 2 clamp), two bits per channel: no table lookup in the kernel
OCC4D_TRACK_HD uint64_t pack_codes(const int32_t* ops, int g) {
  uint64_t packed = 0;
  if (ops)
    for (int c = 0; c < g; ++c) packed |= (uint64_t)(ops[c] & 3) << (2 * c);
  return packed;
}
OCC4D_TRACK_HD int code_of(uint64_t packed, int c) { return (int)((packed >> (2 * c)) & 3u); }

// the expression of squash_kernel (csrc/pointops.hip), letter for letter
OCC4D_TRACK_HD float squash(float v, int op) {
  if (op == 1) v = 1.0f / (1.0f + expf(-v));
  else if (op == 2) v = fminf(fmaxf(v, 0.f), 1.f);
  return v;
}

// one rerun's score `s` of a row onto (best, winner): numpy's `winner[(s >= 0.5) & (s >= best)] = id; best = maximum(s, best)`.
// np.maximum hands a NaN of either operand on, and no comparison with a NaN best holds: after a NaN score the row's
// winner stays.  A tie goes to this (the later) rerun.
OCC4D_TRACK_HD void winner_update(float s, float inst_id, float& best, float& winner) {
  if (s >= 0.5f && s >= best) winner = inst_id;
  if (s != s) best = s;
  else if (best == best && s > best) best = s;
}

}  // namespace occ4d_track
