// Per-row decision of the id histogram (include/occ4d_occl.h) and the entry point's argument contract (host only), shared
// WORD FOR WORD by the HIP kernel (csrc/idhist.hip) and the g++ twin (csrc_cpu/occ4d_twin.cpp): is the row counted, and in
// which bin.  Comparisons are fp32.
#pragma once
#include <stdint.h>

#include "contract.hpp"
#include "occ4d_occl.h"

#if defined(__HIPCC__)
#define OCC4D_OCCL_HD __host__ __device__ __forceinline__
#else
#define OCC4D_OCCL_HD inline
#endif

namespace occ4d_occl {

struct HistArgs {
  const float* rows; int64_t ld; int n, col;
  const float* key;                       // null: every row
  int pred_col; float pred_a, pred_b;     // pred_col < 0: off
  int n_ids;
};

// bin of row i in 0 .. n_ids + 1, or -1 when the row is not counted
OCC4D_OCCL_HD int bin_of(const HistArgs& a, int64_t i) {
  if (a.key && !(a.key[i] > 0.5f)) return -1;
  const float* r = a.rows + i * a.ld;
  if (a.pred_col >= 0) {
    const float p = r[a.pred_col];
    if (!(p == a.pred_a || p == a.pred_b)) return -1;
  }
  const float v = r[a.col];
  if (v < 0.f) return a.n_ids + OCC4D_OCCL_NEGATIVE;
  if (v < (float)a.n_ids) {               // 0 <= v < n_ids (-0.0 included; NaN fails both comparisons)
    const int k = (int)v;
    if ((float)k == v) return k;
  }
  return a.n_ids + OCC4D_OCCL_OTHER;
}

// first k in 1 .. S with off[k] > row, S + 1 when there is none (then the offsets do not end at n).  Whatever the offsets
// hold, the result is in 1 .. S + 1 and, when <= S, off[result] > row: the caller's walk over a tile always advances.
OCC4D_OCCL_HD int segment_end_index(const int64_t* off, int S, int64_t row) {
  int lo = 1, hi = S + 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] > row) hi = mid; else lo = mid + 1;
  }
  return hi;
}

// ---- argument contract (host): the status, `empty` = nothing to do, `a` filled.  What the offsets HOLD is not in here: only
// a library that has them in host memory can look (the twin does, after this).
inline int check_id_histogram(const float* rows, int64_t ld, int n, int col, const int64_t* seg_offsets, int n_segments, int n_ids,
                              const float* key, int pred_col, float pred_a, float pred_b, const int32_t* counts, bool& empty,
                              HistArgs& a) {
  const char* who = "occ4d_id_histogram_f32";
  OCC4D_REQUIRE(n_ids >= 1 && n_ids <= OCC4D_OCCL_MAX_IDS, "%s: n_ids = %d must be in 1 .. %d", who, n_ids, OCC4D_OCCL_MAX_IDS);
  OCC4D_REQUIRE(n >= 0 && n_segments >= 0 && ld >= 1, "%s: n = %d, n_segments = %d, ld = %lld", who, n, n_segments, (long long)ld);
  OCC4D_REQUIRE(col >= 0 && col < ld, "%s: col = %d must be in 0 .. ld - 1 = %lld", who, col, (long long)ld - 1);
  OCC4D_REQUIRE(pred_col >= -1 && pred_col < ld, "%s: pred_col = %d must be -1 or in 0 .. ld - 1 = %lld", who, pred_col, (long long)ld - 1);
  empty = n == 0 || n_segments == 0;
  OCC4D_REQUIRE(empty || (rows && seg_offsets && counts), "%s: null rows / seg_offsets / counts", who);
  a = HistArgs{rows, ld, n, col, key, pred_col, pred_a, pred_b, n_ids};
  return OCC4D_OK;
}

}  // namespace occ4d_occl
