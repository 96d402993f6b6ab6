// The training loss as two launches (loss.MyLosses.per_example + entire_batch, loss.py:50-194, 243-250, 276-277;
// restated in occlusions-4d_amd/training.py:implicit_loss), value and gradient with respect to the raw decoder outputs.
//   occ4d_implicit_loss_f32 (round 6): the two terms of the published CARLA command,
//     total = sum over (frame, example) cells of  [ density_lw * mean_i BCEwithLogits(o[i, 0], y[i, 0])
//                                                   + segm_lw * mean_{i: label_i >= 0} CE(o[i, G - C :], label_i) ] / cells
//   occ4d_implicit_loss_terms_f32: all four terms (the published GREATER command weights density, colour and tracking), the four
//     colour modes, the pre-loss squash of pipeline.py:198-212 folded in and differentiated through, and the per-term values
//     the reference logs every step.
// The torch glue they replace is ~60 element-wise launches and 6.6 ms of host time per step for 0.5 ms of device work (two-term
// form; more with colour and tracking).  Deterministic: every cell is reduced by NB blocks into fixed slots, summed in order by
// the second kernel.
#include "common.hpp"

namespace {

constexpr int LT = 256;
constexpr int NB = 64;                    // partial-sum blocks per cell

// partial[(cell * NB + b) * 4 + {0: sum bce, 1: sum masked ce, 2: count}]
__global__ __launch_bounds__(LT) void loss_sums_kernel(const float* __restrict__ o, int64_t ldo, const float* __restrict__ y,
                                                       int64_t ldy, int n, int G, int C, int ycol_label,
                                                       float* __restrict__ partial) {
  const int cell = blockIdx.y, b = blockIdx.x;
  const float* oc = o + (int64_t)cell * n * ldo;
  const float* yc = y + (int64_t)cell * n * ldy;
  float s_bce = 0.f, s_ce = 0.f, s_cnt = 0.f;
  for (int i = b * LT + threadIdx.x; i < n; i += NB * LT) {
    const float* row = oc + (int64_t)i * ldo;
    const float x = row[0], t = yc[(int64_t)i * ldy];
    s_bce += fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    if (C > 0) {
      const int lab = (int)yc[(int64_t)i * ldy + ycol_label];
      if (lab >= 0) {
        const float* z = row + G - C;
        float m = z[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - m);
        s_ce += m + logf(se) - z[min(lab, C - 1)];
        s_cnt += 1.f;
      }
    }
  }
  __shared__ float red[3][LT / 64];
  float v[3] = {s_bce, s_ce, s_cnt};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float a = v[k];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float a = 0.f;
    for (int w = 0; w < LT / 64; ++w) a += red[threadIdx.x][w];
    partial[((int64_t)cell * NB + b) * 4 + threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(LT) void loss_grad_kernel(const float* __restrict__ o, int64_t ldo, const float* __restrict__ y,
                                                       int64_t ldy, int n, int G, int C, int ycol_label, int cells,
                                                       float density_lw, float segm_lw, const float* __restrict__ partial,
                                                       float* __restrict__ loss, float* __restrict__ grad, int64_t ldg) {
  const int cell = blockIdx.y;
  __shared__ float tot[3];
  if (threadIdx.x < 3) {
    float a = 0.f;
    for (int b = 0; b < NB; ++b) a += partial[((int64_t)cell * NB + b) * 4 + threadIdx.x];
    tot[threadIdx.x] = a;
  }
  __syncthreads();
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {      // the scalar: every cell's totals once more, in order
    float total = 0.f;
    for (int cl = 0; cl < cells; ++cl) {
      float t[3] = {0.f, 0.f, 0.f};
      for (int b = 0; b < NB; ++b)
        for (int k = 0; k < 3; ++k) t[k] += partial[((int64_t)cl * NB + b) * 4 + k];
      total += density_lw * (t[0] / (float)n) / (float)cells;
      if (C > 0 && segm_lw > 0.f) total += segm_lw * (t[1] / t[2]) / (float)cells;
    }
    loss[0] = total;
  }
  if (!grad) return;
  const float gd = density_lw / (float)cells / (float)n;
  const float gs = (C > 0 && segm_lw > 0.f) ? segm_lw / (float)cells / tot[2] : 0.f;
  const float* oc = o + (int64_t)cell * n * ldo;
  const float* yc = y + (int64_t)cell * n * ldy;
  float* gc = grad + (int64_t)cell * n * ldg;
  for (int i = blockIdx.x * LT + threadIdx.x; i < n; i += gridDim.x * LT) {
    const float* row = oc + (int64_t)i * ldo;
    float* g = gc + (int64_t)i * ldg;
    const float x = row[0], t = yc[(int64_t)i * ldy];
    g[0] = density_lw > 0.f ? gd * (1.f / (1.f + expf(-x)) - t) : 0.f;
    for (int c = 1; c < G - C; ++c) g[c] = 0.f;
    if (C > 0) {
      const int lab = (int)yc[(int64_t)i * ldy + ycol_label];
      const float* z = row + G - C;
      if (lab >= 0 && gs != 0.f) {
        float m = z[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - m);
        const float inv = 1.f / se;
        for (int c = 0; c < C; ++c) g[G - C + c] = gs * (expf(z[c] - m) * inv - (c == min(lab, C - 1) ? 1.f : 0.f));
      } else {
        for (int c = 0; c < C; ++c) g[G - C + c] = 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------- all four terms (occ4d_implicit_loss_terms_f32)
// Per-cell sums, partial[(cell * NB + b) * NS + slot]:
enum { S_BCE = 0, S_SEG, S_SEG_N, S_COL, S_COL_N, S_VAL, S_HUE, S_HUE_N, S_TRK, S_TRK_N, NS };
constexpr int HUE_MIN_ROWS = 16;          // loss.py:104: fewer hue-supervised rows in a cell -> no hue term

struct TermsCfg {
  int n, G, C;                            // C: segmentation classes when that term is weighted, else 0
  int mode, track_idx, cells;
  float w_dens, w_col, w_seg, w_trk;
};

__device__ inline float bce_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }
__device__ inline float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
__device__ inline float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ inline float signf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// cross entropy of K logits against class `cls`; with g: g[c] = scale * (softmax_c - [c == cls])
__device__ inline float ce_row(const float* z, int K, int cls, float* g, float scale) {
  float m = z[0];
  for (int c = 1; c < K; ++c) m = fmaxf(m, z[c]);
  float se = 0.f;
  for (int c = 0; c < K; ++c) se += expf(z[c] - m);
  if (g) {
    const float inv = 1.f / se;
    for (int c = 0; c < K; ++c) g[c] = scale * (expf(z[c] - m) * inv - (c == cls ? 1.f : 0.f));
  }
  return m + logf(se) - z[cls];
}

// utils.rgb_to_hsv (utils/utils.py:169-191) in its own fp32 operation order (the file is compiled with -ffp-contract=off; the
// divisions are correctly rounded): the class targets below must be the integers torch computes on the device, half-way cases
// included.
struct Hsv { float h, s, v; };
__device__ inline Hsv rgb_to_hsv(float r, float g, float b) {
  const float mx = fmaxf(fmaxf(r, g), b);
  float mn = r;
  int arg = 0;                                      // first minimum on ties, as torch.min
  if (g < mn) { mn = g; arg = 1; }
  if (b < mn) { mn = b; arg = 2; }
  const float mm = (mx - mn) + 1e-10f;
  float h;
  if (arg == 0) h = 60.f * (b - g) / mm + 180.f;
  else if (arg == 1) h = 60.f * (r - b) / mm + 300.f;
  else h = 60.f * (g - r) / mm + 60.f;
  return {h, mm / (mx + 1e-10f), mx};
}

// round(h / 360 * bins) (half to even, torch.round), `bins` -> 0.  On the device torch divides a tensor by a host scalar as a
// multiplication by the scalar's fp32 reciprocal (ATen's div_true kernel), so the reference's `hue / 360.0` is h * (1 / 360)
// where it trains; the quotient and the product differ in the last bit for some hues, and colours on a hue-bin edge are
// exact half-way cases of the rounding (hue 15 + 30 k degrees at 12 bins), so the form decides their class.
__device__ inline int hue_class(float h, int bins) {
  const int c = (int)rintf(h * (1.f / 360.f) * (float)bins);
  return c >= bins || c < 0 ? 0 : c;
}

// loss.py:116-149: 6 saturated colours, overridden by black / gray / white where the colour is bland
__device__ inline int bins_class(Hsv q) {
  if (q.s < 0.3f || q.v < 0.3f) return q.v < 0.2f ? 6 : (q.v < 0.6f ? 7 : 8);
  return hue_class(q.h, 6);
}

__global__ __launch_bounds__(LT) void terms_sums_kernel(const float* __restrict__ o, int64_t ldo, const float* __restrict__ y,
                                                        int64_t ldy, TermsCfg cfg, float* __restrict__ partial) {
  const int cell = blockIdx.y, b = blockIdx.x, n = cfg.n, G = cfg.G, C = cfg.C;
  const float* oc = o + (int64_t)cell * n * ldo;
  const float* yc = y + (int64_t)cell * n * ldy;
  float s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.f;
  for (int i = b * LT + threadIdx.x; i < n; i += NB * LT) {
    const float* row = oc + (int64_t)i * ldo;
    const float* yr = yc + (int64_t)i * ldy;
    const float t = yr[0];
    if (cfg.w_dens > 0.f) s[S_BCE] += bce_logits(row[0], t);
    if (C > 0) {
      const int lab = (int)yr[5];
      if (lab >= 0) {
        s[S_SEG] += ce_row(row + G - C, C, min(lab, C - 1), nullptr, 0.f);
        s[S_SEG_N] += 1.f;
      }
    }
    const bool solid = t >= 0.1f;
    if (cfg.w_col > 0.f && solid && yr[1] >= 0.f) {
      s[S_COL_N] += 1.f;
      if (cfg.mode <= 1) {
        for (int c = 1; c < 4; ++c) s[S_COL] += fabsf((cfg.mode == 0 ? sigmoidf(row[c]) : clamp01(row[c])) - yr[c]);
      } else {
        const Hsv q = rgb_to_hsv(yr[1], yr[2], yr[3]);
        if (cfg.mode == 2) {
          s[S_COL] += fabsf(clamp01(row[13]) - q.s);
          s[S_VAL] += fabsf(clamp01(row[14]) - q.v);
          if (q.s >= 0.2f && q.v >= 0.2f) {
            s[S_HUE] += ce_row(row + 1, 12, hue_class(q.h, 12), nullptr, 0.f);
            s[S_HUE_N] += 1.f;
          }
        } else {
          s[S_COL] += ce_row(row + 1, 9, bins_class(q), nullptr, 0.f);
        }
      }
    }
    if (cfg.w_trk > 0.f && solid && yr[4] >= 0.f) {
      s[S_TRK] += bce_logits(row[cfg.track_idx], yr[4]);
      s[S_TRK_N] += 1.f;
    }
  }
  __shared__ float red[NS][LT / 64];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    float a = s[k];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    float a = 0.f;
    for (int w = 0; w < LT / 64; ++w) a += red[threadIdx.x][w];
    partial[((int64_t)cell * NB + b) * NS + threadIdx.x] = a;
  }
}

// one cell's unweighted terms (colour, density, segmentation, tracking) from its sums; 0 for a term without weight.  A mean
// over an empty selection is 0 / 0 = NaN, as the reference's.
__device__ inline void cell_terms(const float* t, const TermsCfg& cfg, float* out) {
  out[0] = out[1] = out[2] = out[3] = 0.f;
  if (cfg.w_dens > 0.f) out[1] = t[S_BCE] / (float)cfg.n;
  if (cfg.w_col > 0.f) {
    if (cfg.mode <= 1) {
      out[0] = t[S_COL] / (t[S_COL_N] * 3.f);
    } else if (cfg.mode == 2) {
      const float hue = t[S_HUE_N] >= (float)HUE_MIN_ROWS ? t[S_HUE] / t[S_HUE_N] / 2.f : 0.f;
      out[0] = (hue + t[S_COL] / t[S_COL_N] + t[S_VAL] / t[S_COL_N]) / 3.f;
    } else {
      out[0] = t[S_COL] / t[S_COL_N] / 3.f;
    }
  }
  if (cfg.C > 0) out[2] = t[S_SEG] / t[S_SEG_N];
  if (cfg.w_trk > 0.f) out[3] = t[S_TRK] / t[S_TRK_N];
}

__global__ __launch_bounds__(LT) void terms_grad_kernel(const float* __restrict__ o, int64_t ldo, const float* __restrict__ y,
                                                        int64_t ldy, TermsCfg cfg, const float* __restrict__ partial,
                                                        float* __restrict__ loss, float* __restrict__ terms,
                                                        float* __restrict__ grad, int64_t ldg) {
  const int cell = blockIdx.y, n = cfg.n, G = cfg.G, C = cfg.C, cells = cfg.cells;
  __shared__ float tot[NS];
  if (threadIdx.x < NS) {
    float a = 0.f;
    for (int b = 0; b < NB; ++b) a += partial[((int64_t)cell * NB + b) * NS + threadIdx.x];
    tot[threadIdx.x] = a;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {      // the scalars: every cell's totals once more (16 cells at a time), added in cell order
    __shared__ float all[LT / 16][16];
    float total = 0.f, tm[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cells; c0 += LT / 16) {
      const int cl = c0 + (threadIdx.x >> 4), k = threadIdx.x & 15;
      if (cl < cells && k < NS) {
        float a = 0.f;
        for (int b = 0; b < NB; ++b) a += partial[((int64_t)cl * NB + b) * NS + k];
        all[threadIdx.x >> 4][k] = a;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int j = 0; j < LT / 16 && c0 + j < cells; ++j) {
          float t4[4];
          cell_terms(all[j], cfg, t4);
          if (cfg.w_dens > 0.f) total += cfg.w_dens * t4[1] / (float)cells;
          if (cfg.w_col > 0.f) total += cfg.w_col * t4[0] / (float)cells;
          if (C > 0) total += cfg.w_seg * t4[2] / (float)cells;
          if (cfg.w_trk > 0.f) total += cfg.w_trk * t4[3] / (float)cells;
          for (int k2 = 0; k2 < 4; ++k2) tm[k2] += t4[k2];
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      loss[0] = total;
      for (int k2 = 0; k2 < 4; ++k2) terms[k2] = tm[k2] / (float)cells;
    }
  }
  __syncthreads();
  if (!grad) return;
  const float fc = (float)cells;
  const float gd = cfg.w_dens / fc / (float)n;
  const float gs = C > 0 ? cfg.w_seg / fc / tot[S_SEG_N] : 0.f;
  const float gt = cfg.w_trk / fc / tot[S_TRK_N];
  const float gc_l1 = cfg.w_col / fc / (tot[S_COL_N] * 3.f);          // rgb: mean over rows x 3 channels; hsv: (L1 sat + L1 val) / 3
  const float gc_ce = cfg.w_col / fc / 3.f / tot[S_COL_N];            // bins
  const bool hue_on = tot[S_HUE_N] >= (float)HUE_MIN_ROWS;
  const float gc_hue = cfg.w_col / fc / 3.f / 2.f / tot[S_HUE_N];     // hsv hue (used when hue_on)
  const float* oc = o + (int64_t)cell * n * ldo;
  const float* yc = y + (int64_t)cell * n * ldy;
  float* gcell = grad + (int64_t)cell * n * ldg;
  for (int i = blockIdx.x * LT + threadIdx.x; i < n; i += gridDim.x * LT) {
    const float* row = oc + (int64_t)i * ldo;
    const float* yr = yc + (int64_t)i * ldy;
    float* g = gcell + (int64_t)i * ldg;
    const float t = yr[0];
    g[0] = cfg.w_dens > 0.f ? gd * (sigmoidf(row[0]) - t) : 0.f;
    for (int c = 1; c < G; ++c) g[c] = 0.f;
    if (C > 0) {
      const int lab = (int)yr[5];
      if (lab >= 0) ce_row(row + G - C, C, min(lab, C - 1), g + G - C, gs);
    }
    const bool solid = t >= 0.1f;
    if (cfg.w_col > 0.f && solid && yr[1] >= 0.f) {
      if (cfg.mode == 0) {
        for (int c = 1; c < 4; ++c) {
          const float s = sigmoidf(row[c]);
          g[c] = gc_l1 * signf(s - yr[c]) * (1.f - s) * s;
        }
      } else if (cfg.mode == 1) {                  // torch's clamp passes the gradient on the closed interval [0, 1]
        for (int c = 1; c < 4; ++c) g[c] = row[c] >= 0.f && row[c] <= 1.f ? gc_l1 * signf(row[c] - yr[c]) : 0.f;
      } else {
        const Hsv q = rgb_to_hsv(yr[1], yr[2], yr[3]);
        if (cfg.mode == 2) {
          g[13] = row[13] >= 0.f && row[13] <= 1.f ? gc_l1 * signf(row[13] - q.s) : 0.f;
          g[14] = row[14] >= 0.f && row[14] <= 1.f ? gc_l1 * signf(row[14] - q.v) : 0.f;
          if (hue_on && q.s >= 0.2f && q.v >= 0.2f) ce_row(row + 1, 12, hue_class(q.h, 12), g + 1, gc_hue);
        } else {
          ce_row(row + 1, 9, bins_class(q), g + 1, gc_ce);
        }
      }
    }
    if (cfg.w_trk > 0.f && solid && yr[4] >= 0.f) g[cfg.track_idx] = gt * (sigmoidf(row[cfg.track_idx]) - yr[4]);
  }
}

}  // namespace

extern "C" int64_t occ4d_implicit_loss_workspace_floats(int cells) { return (int64_t)cells * NB * 4; }

extern "C" int occ4d_implicit_loss_f32(const float* out, int64_t ldo, const float* target, int64_t ldt, int cells, int n, int g,
                                       int label_col, int semantic_classes, float density_lw, float segmentation_lw,
                                       float* workspace, float* loss, float* grad, int64_t ldg, void* stream) {
  const char* who = "occ4d_implicit_loss_f32";
  OCC4D_REQUIRE(out && target && workspace && loss && cells >= 1 && n >= 1 && g >= 1 && ldo >= g && label_col >= 1 && ldt > label_col && (!grad || ldg >= g),
                "%s: null pointer or bad sizes", who);
  OCC4D_REQUIRE(semantic_classes >= 0 && semantic_classes < g && density_lw >= 0.f && segmentation_lw >= 0.f,
                "%s: semantic_classes = %d must be below the output width %d; weights >= 0", who, semantic_classes, g);
  const int C = segmentation_lw > 0.f ? semantic_classes : 0;
  hipStream_t st = (hipStream_t)stream;
  loss_sums_kernel<<<dim3(NB, cells), LT, 0, st>>>(out, ldo, target, ldt, n, g, C, label_col, workspace);
  const int gx = occ4d::cdiv(n, LT) < 1024 ? occ4d::cdiv(n, LT) : 1024;
  loss_grad_kernel<<<dim3(gx, cells), LT, 0, st>>>(out, ldo, target, ldt, n, g, C, label_col, cells, density_lw, segmentation_lw, workspace,
                                                   loss, grad, ldg);
  return occ4d::check_launch(who);
}

extern "C" int64_t occ4d_implicit_loss_terms_workspace_floats(int cells) { return (int64_t)cells * NB * NS; }

extern "C" int occ4d_implicit_loss_terms_f32(const float* out, int64_t ldo, const float* target, int64_t ldt, int cells, int n, int g,
                                             int color_mode, int semantic_classes, float density_lw, float color_lw,
                                             float segmentation_lw, float tracking_lw, float* workspace, float* loss, float* terms,
                                             float* grad, int64_t ldg, void* stream) {
  const char* who = "occ4d_implicit_loss_terms_f32";
  OCC4D_REQUIRE(out && target && workspace && loss && terms && cells >= 1 && n >= 1 && g >= 1 && ldo >= g && ldt >= 6 && (!grad || ldg >= g),
                "%s: null pointer or bad sizes", who);
  OCC4D_REQUIRE(color_mode >= 0 && color_mode <= 3, "%s: color_mode = %d (0 rgb, 1 rgb_nosigmoid, 2 hsv, 3 bins)", who, color_mode);
  OCC4D_REQUIRE(density_lw >= 0.f && color_lw >= 0.f && segmentation_lw >= 0.f && tracking_lw >= 0.f, "%s: weights >= 0", who);
  const int color_end = color_mode <= 1 ? 4 : (color_mode == 2 ? 15 : 10);      // one past the last colour channel
  const int track_idx = color_end;                                               // utils.get_track_idx
  int used = 1;                                                                  // channels the weighted non-segmentation terms read
  if (color_lw > 0.f) {
    OCC4D_REQUIRE(g >= color_end, "%s: color_mode %d reads channels 1 .. %d, the output width is %d", who, color_mode, color_end - 1, g);
    used = color_end;
  }
  if (tracking_lw > 0.f) {
    OCC4D_REQUIRE(g > track_idx, "%s: the tracking logit of color_mode %d is channel %d, the output width is %d", who, color_mode,
                  track_idx, g);
    used = track_idx + 1;
  }
  if (segmentation_lw > 0.f)
    OCC4D_REQUIRE(semantic_classes >= 1 && semantic_classes <= g - used,
                  "%s: semantic_classes = %d must fit behind the %d channels of the other weighted terms (output width %d)", who,
                  semantic_classes, used, g);
  TermsCfg cfg;
  cfg.n = n, cfg.G = g, cfg.C = segmentation_lw > 0.f ? semantic_classes : 0;
  cfg.mode = color_mode, cfg.track_idx = track_idx, cfg.cells = cells;
  cfg.w_dens = density_lw, cfg.w_col = color_lw, cfg.w_seg = segmentation_lw, cfg.w_trk = tracking_lw;
  hipStream_t st = (hipStream_t)stream;
  terms_sums_kernel<<<dim3(NB, cells), LT, 0, st>>>(out, ldo, target, ldt, cfg, workspace);
  const int gx = occ4d::cdiv(n, LT) < 1024 ? occ4d::cdiv(n, LT) : 1024;
  terms_grad_kernel<<<dim3(gx, cells), LT, 0, st>>>(out, ldo, target, ldt, cfg, workspace, loss, terms, grad, ldg);
  return occ4d::check_launch(who);
}
