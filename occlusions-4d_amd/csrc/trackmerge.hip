// Running merge of the per-instance reruns of track_mode 'all' (include/occ4d_track.h): two element-wise, memory-bound
// passes -- one rerun ADDED onto the accumulator with the per-channel squash and the winner / best update folded in, and the
// FINISH (division by the run count, the winner into the track column).  The element bodies and the argument contracts are
// csrc/track_math.hpp, shared with the g++ twin; the loops, the flat path and the launches are here.
//
// 256-thread workgroups, a grid-stride loop, the grid capped as a function of the element count alone.  Contiguous arrays
// (ld == g) whose bases are 16-byte aligned take the flat path: an item is four consecutive floats, one 16-byte load and
// store each, the channel of an element = flat index mod g; the at most three elements behind the last whole item are
// taken one by one.  Everything else takes the one-element-per-item loop with explicit row strides.  The thread that owns
// a row's track-column element does that row's winner / best update: no atomics, no LDS.  Nothing is indexed by data.
#include "common.hpp"
#include "track_math.hpp"
#include "occ4d_track.h"

namespace {

namespace tk = occ4d_track;

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;            // workgroups of a pass; more items than GRID_CAP * THREADS: further trips of the loop

inline int grid_for(int64_t items) {
  const int64_t blocks = (items + THREADS - 1) / THREADS;
  return (int)(blocks < GRID_CAP ? blocks : GRID_CAP);
}

template <bool FIRST>
__global__ __launch_bounds__(THREADS) void merge_add_kernel(const tk::AddArgs a) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.total; e += step) {
    const int64_t i = e / a.g;
    const int c = (int)(e - i * a.g);
    float* dst = a.acc + i * a.ld_acc + c;
    *dst = tk::add_one<FIRST>(a, a.out[i * a.ld_out + c], FIRST ? 0.f : *dst, i, c);
  }
}

// ld_out == ld_acc == g, both bases 16-byte aligned
template <bool FIRST>
__global__ __launch_bounds__(THREADS) void merge_add_flat4_kernel(const tk::AddArgs a) {
  const int64_t items = a.total / 4;
  const int64_t step = (int64_t)gridDim.x * THREADS;
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  for (int64_t j = t; j < items; j += step) {
    const int64_t e = 4 * j;
    int64_t i = e / a.g;
    int c = (int)(e - i * a.g);
    const float4 raw = *reinterpret_cast<const float4*>(a.out + e);
    float4 prev = {0.f, 0.f, 0.f, 0.f};
    if (!FIRST) prev = *reinterpret_cast<const float4*>(a.acc + e);
    float4 r;
    r.x = tk::add_one<FIRST>(a, raw.x, prev.x, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.y = tk::add_one<FIRST>(a, raw.y, prev.y, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.z = tk::add_one<FIRST>(a, raw.z, prev.z, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.w = tk::add_one<FIRST>(a, raw.w, prev.w, i, c);
    *reinterpret_cast<float4*>(a.acc + e) = r;
  }
  const int64_t e = 4 * items + t;          // (t < 3 only: the elements behind the last whole item)
  if (e < a.total) {
    const int64_t i = e / a.g;
    const int c = (int)(e - i * a.g);
    a.acc[e] = tk::add_one<FIRST>(a, a.out[e], FIRST ? 0.f : a.acc[e], i, c);
  }
}

__global__ __launch_bounds__(THREADS) void merge_finish_kernel(const tk::FinishArgs f) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < f.total; e += step) {
    const int64_t i = e / f.g;
    const int c = (int)(e - i * f.g);
    float* p = f.acc + i * f.ld_acc + c;
    *p = tk::finish_one(f, *p, i, c);
  }
}

__global__ __launch_bounds__(THREADS) void merge_finish_flat4_kernel(const tk::FinishArgs f) {
  const int64_t items = f.total / 4;
  const int64_t step = (int64_t)gridDim.x * THREADS;
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  for (int64_t j = t; j < items; j += step) {
    const int64_t e = 4 * j;
    int64_t i = e / f.g;
    int c = (int)(e - i * f.g);
    float4 v = *reinterpret_cast<const float4*>(f.acc + e);
    v.x = tk::finish_one(f, v.x, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.y = tk::finish_one(f, v.y, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.z = tk::finish_one(f, v.z, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.w = tk::finish_one(f, v.w, i, c);
    *reinterpret_cast<float4*>(f.acc + e) = v;
  }
  const int64_t e = 4 * items + t;
  if (e < f.total) {
    const int64_t i = e / f.g;
    f.acc[e] = tk::finish_one(f, f.acc[e], i, (int)(e - i * f.g));
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int occ4d_track_merge_add_f32(const float* out, int64_t ld_out, int n, int g, const int32_t* ops_host, int track_col,
                                         float inst_id, int first, float* acc, int64_t ld_acc, float* best, float* winner,
                                         void* stream) {
  tk::AddArgs a; bool empty;
  OCC4D_TRY(tk::check_merge_add(out, ld_out, n, g, ops_host, track_col, inst_id, first, acc, ld_acc, best, winner, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (ld_out == g && ld_acc == g && aligned16(out) && aligned16(acc)) {
    const int grid = grid_for(a.total / 4 > 0 ? a.total / 4 : 1);
    if (first) merge_add_flat4_kernel<true><<<grid, THREADS, 0, st>>>(a);
    else merge_add_flat4_kernel<false><<<grid, THREADS, 0, st>>>(a);
  } else {
    const int grid = grid_for(a.total);
    if (first) merge_add_kernel<true><<<grid, THREADS, 0, st>>>(a);
    else merge_add_kernel<false><<<grid, THREADS, 0, st>>>(a);
  }
  return occ4d::check_launch("occ4d_track_merge_add_f32");
}

extern "C" int occ4d_track_merge_finish_f32(float* acc, int64_t ld_acc, int n, int g, int n_runs, int track_col,
                                            const float* winner, void* stream) {
  tk::FinishArgs f; bool empty;
  OCC4D_TRY(tk::check_merge_finish(acc, ld_acc, n, g, n_runs, track_col, winner, empty, f));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (ld_acc == g && aligned16(acc))
    merge_finish_flat4_kernel<<<grid_for(f.total / 4 > 0 ? f.total / 4 : 1), THREADS, 0, st>>>(f);
  else
    merge_finish_kernel<<<grid_for(f.total), THREADS, 0, st>>>(f);
  return occ4d::check_launch("occ4d_track_merge_finish_f32");
}
