// Running merge of the per-instance reruns of track_mode 'all' (include/occ4d_track.h): two element-wise, memory-bound
// passes -- one rerun ADDED onto the accumulator with the per-channel squash and the winner / best update folded in, and the
// FINISH (division by the run count, the winner into the track column).  The per-element decisions are csrc/track_math.hpp,
// shared with the g++ twin.
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

struct AddArgs {
  const float* out; int64_t ld_out;
  float* acc; int64_t ld_acc;
  float* best; float* winner;
  int64_t total;                          // n * g
  int g, track_col;
  float inst_id;
  uint64_t codes;
};

// element (row i, channel c): the rerun's raw value and the accumulator's value -> the accumulator's new value
template <bool FIRST>
__device__ __forceinline__ float add_one(const AddArgs& a, float raw, float prev, int64_t i, int c) {
  const float v = tk::squash(raw, tk::code_of(a.codes, c));
  if (c == a.track_col) {
    float best = FIRST ? 0.f : a.best[i], winner = FIRST ? -1.f : a.winner[i];
    tk::winner_update(v, a.inst_id, best, winner);
    a.best[i] = best;
    a.winner[i] = winner;
  }
  return FIRST ? v : prev + v;
}

template <bool FIRST>
__global__ __launch_bounds__(THREADS) void merge_add_kernel(const AddArgs a) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < a.total; e += step) {
    const int64_t i = e / a.g;
    const int c = (int)(e - i * a.g);
    float* dst = a.acc + i * a.ld_acc + c;
    *dst = add_one<FIRST>(a, a.out[i * a.ld_out + c], FIRST ? 0.f : *dst, i, c);
  }
}

// ld_out == ld_acc == g, both bases 16-byte aligned
template <bool FIRST>
__global__ __launch_bounds__(THREADS) void merge_add_flat4_kernel(const AddArgs a) {
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
    r.x = add_one<FIRST>(a, raw.x, prev.x, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.y = add_one<FIRST>(a, raw.y, prev.y, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.z = add_one<FIRST>(a, raw.z, prev.z, i, c);
    if (++c == a.g) { c = 0; ++i; }
    r.w = add_one<FIRST>(a, raw.w, prev.w, i, c);
    *reinterpret_cast<float4*>(a.acc + e) = r;
  }
  const int64_t e = 4 * items + t;          // (t < 3 only: the elements behind the last whole item)
  if (e < a.total) {
    const int64_t i = e / a.g;
    const int c = (int)(e - i * a.g);
    a.acc[e] = add_one<FIRST>(a, a.out[e], FIRST ? 0.f : a.acc[e], i, c);
  }
}

struct FinishArgs {
  float* acc; int64_t ld_acc;
  const float* winner;
  int64_t total;
  int g, track_col;
  float runs;
};

__device__ __forceinline__ float finish_one(const FinishArgs& f, float sum, int64_t i, int c) {
  return c == f.track_col ? f.winner[i] : sum / f.runs;
}

__global__ __launch_bounds__(THREADS) void merge_finish_kernel(const FinishArgs f) {
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < f.total; e += step) {
    const int64_t i = e / f.g;
    const int c = (int)(e - i * f.g);
    float* p = f.acc + i * f.ld_acc + c;
    *p = finish_one(f, *p, i, c);
  }
}

__global__ __launch_bounds__(THREADS) void merge_finish_flat4_kernel(const FinishArgs f) {
  const int64_t items = f.total / 4;
  const int64_t step = (int64_t)gridDim.x * THREADS;
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  for (int64_t j = t; j < items; j += step) {
    const int64_t e = 4 * j;
    int64_t i = e / f.g;
    int c = (int)(e - i * f.g);
    float4 v = *reinterpret_cast<const float4*>(f.acc + e);
    v.x = finish_one(f, v.x, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.y = finish_one(f, v.y, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.z = finish_one(f, v.z, i, c);
    if (++c == f.g) { c = 0; ++i; }
    v.w = finish_one(f, v.w, i, c);
    *reinterpret_cast<float4*>(f.acc + e) = v;
  }
  const int64_t e = 4 * items + t;
  if (e < f.total) {
    const int64_t i = e / f.g;
    f.acc[e] = finish_one(f, f.acc[e], i, (int)(e - i * f.g));
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int occ4d_track_merge_add_f32(const float* out, int64_t ld_out, int n, int g, const int32_t* ops_host, int track_col,
                                         float inst_id, int first, float* acc, int64_t ld_acc, float* best, float* winner,
                                         void* stream) {
  const char* who = "occ4d_track_merge_add_f32";
  OCC4D_REQUIRE(n >= 0 && g >= 1 && g <= 32, "%s: n = %d, g = %d: need n >= 0, 1 <= g <= 32", who, n, g);
  OCC4D_REQUIRE(ld_out >= g && ld_acc >= g, "%s: ld_out = %lld, ld_acc = %lld must be >= g = %d", who, (long long)ld_out,
                (long long)ld_acc, g);
  OCC4D_REQUIRE(track_col >= -1 && track_col < g, "%s: track_col = %d must be -1 or in 0 .. g - 1 = %d", who, track_col, g - 1);
  OCC4D_REQUIRE(first == 0 || first == 1, "%s: first = %d must be 0 or 1", who, first);
  if (ops_host)
    for (int c = 0; c < g; ++c) OCC4D_REQUIRE(ops_host[c] >= 0 && ops_host[c] <= 2, "%s: op code %d", who, ops_host[c]);
  if (n == 0) return OCC4D_OK;
  OCC4D_REQUIRE(out && acc, "%s: null out / acc", who);
  OCC4D_REQUIRE(track_col < 0 || (best && winner), "%s: null best / winner with track_col = %d", who, track_col);
  const AddArgs a{out, ld_out, acc, ld_acc, best, winner, (int64_t)n * g, g, track_col, inst_id, tk::pack_codes(ops_host, g)};
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
  return occ4d::check_launch(who);
}

extern "C" int occ4d_track_merge_finish_f32(float* acc, int64_t ld_acc, int n, int g, int n_runs, int track_col,
                                            const float* winner, void* stream) {
  const char* who = "occ4d_track_merge_finish_f32";
  OCC4D_REQUIRE(n >= 0 && g >= 1 && g <= 32, "%s: n = %d, g = %d: need n >= 0, 1 <= g <= 32", who, n, g);
  OCC4D_REQUIRE(ld_acc >= g, "%s: ld_acc = %lld must be >= g = %d", who, (long long)ld_acc, g);
  OCC4D_REQUIRE(track_col >= -1 && track_col < g, "%s: track_col = %d must be -1 or in 0 .. g - 1 = %d", who, track_col, g - 1);
  OCC4D_REQUIRE(n_runs >= 1, "%s: n_runs = %d must be >= 1", who, n_runs);
  if (n == 0) return OCC4D_OK;
  OCC4D_REQUIRE(acc, "%s: null acc", who);
  OCC4D_REQUIRE(track_col < 0 || winner, "%s: null winner with track_col = %d", who, track_col);
  const FinishArgs f{acc, ld_acc, winner, (int64_t)n * g, g, track_col, (float)n_runs};
  const hipStream_t st = (hipStream_t)stream;
  if (ld_acc == g && aligned16(acc))
    merge_finish_flat4_kernel<<<grid_for(f.total / 4 > 0 ? f.total / 4 : 1), THREADS, 0, st>>>(f);
  else
    merge_finish_kernel<<<grid_for(f.total), THREADS, 0, st>>>(f);
  return occ4d::check_launch(who);
}
