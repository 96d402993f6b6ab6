// CPU twin of the C ABI (include/occ4d.h), compiled by g++ -- SURVEY.md 8(b), last line of "What a C-ABI replacement
// must export": "each with a CPU twin compiled by g++ for config 1" (BASELINE configs[0]: "runs without a GPU").
//
// What this is: the SAME entry points, prototypes and contracts as libocc4d.so for the inference path (kNN, FPS, Linear,
// PointTransformerLayer / Block, DownTransition pooling, the LocalPclResnetFC decoder, post-ops, grid, split), written as
// plain host loops in the reference's AS-WRITTEN op order (model/point_transformer_layer.py:167-179,
// model/implicit.py:328-443, model/modules.py:126-158) -- no merged weights, no packed streams, no tables beyond the
// per-scene to_k / to_v rows.  `prepared` / `workspace` buffers are unused (their size queries return a token size);
// `stream` is ignored (every call is synchronous).  Pointers are HOST pointers.
//
// What this is NOT: a fallback.  libocc4d_cpu.so is never loaded unless the caller asks for it by name
// (occlusions4d_amd.cpu_twin.enable(), tests only); the product on a GPU box fails loudly without libocc4d.so and rejects
// CPU tensors.  Its job is to let BASELINE configs[0] run without a GPU and to let the REFERENCE's own caller
// (eval/inference.py:perform_inference) drive the product modules in the build container (tests/test_cpu_twin.py).
// Entry points outside the inference path (training kernels, packers, the A/B kernels) are not here; a call through the
// twin to one of them raises in Python.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "occ4d.h"
#include "occ4d_frontend.h"
#include "occ4d_eval.h"
#include "occ4d_occl.h"
#include "occ4d_track.h"
#include "occ4d_project.h"
#include "occ4d_inst.h"
#include "occ4d_refine.h"
#include "occ4d_surface.h"
#include "ext/occ4d_raycast.h"
#include "ext/occ4d_components.h"
#include "ext/occ4d_link.h"
#include "ext/occ4d_distance.h"
#include "ext/occ4d_geodesic.h"
#include "ext/occ4d_watershed.h"
#include "ext/occ4d_sight.h"
#include "ext/occ4d_pull.h"
#include "ext/occ4d_viewplan.h"
#include "ext/occ4d_boxes.h"
#include "ext/occ4d_layers.h"
#include "ext/occ4d_evidence.h"
// csrc/, the HIP library's own source: each feature's per-element arithmetic, item bodies and argument contracts (contract.hpp)
#include "frontend_math.hpp"
#include "eval_math.hpp"
#include "occl_math.hpp"
#include "track_math.hpp"
#include "project_math.hpp"
#include "inst_math.hpp"
#include "refine_math.hpp"
#include "surface_math.hpp"
#include "raycast_math.hpp"
#include "components_math.hpp"
#include "link_math.hpp"
#include "distance_math.hpp"
#include "geodesic_math.hpp"
#include "watershed_math.hpp"
#include "sight_math.hpp"
#include "pull_math.hpp"
#include "viewplan_math.hpp"
#include "boxes_math.hpp"
#include "layers_math.hpp"
#include "sweep_math.hpp"
#include "evidence_math.hpp"
#include "decoder_math.hpp"

namespace fe = occ4d_frontend;
namespace ev = occ4d_eval;
namespace oc = occ4d_occl;
namespace tk = occ4d_track;
namespace pj = occ4d_project;
namespace in = occ4d_inst;
namespace rf = occ4d_refine;
namespace sf = occ4d_surface;
namespace ry = occ4d_raycast;
namespace sw = occ4d_sweep;
namespace ed = occ4d_evidence;
namespace cc = occ4d_components;
namespace lk = occ4d_link;
namespace dm = occ4d_distance;
namespace gm = occ4d_geodesic;
namespace ws = occ4d_watershed;
namespace sm = occ4d_sight;
namespace pm = occ4d_pull;
namespace vm = occ4d_viewplan;
namespace bm = occ4d_boxes;
namespace lm = occ4d_layers;

static thread_local char g_err[512] = "";

void occ4d::set_error(const char* fmt, ...) {      // csrc/contract.hpp: OCC4D_REQUIRE / OCC4D_TRY, the HIP library's own macros
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

namespace {

inline float act(float v, int code) {      // 0 identity, 1 relu, 2 swish (model/implicit.py:46-64)
  if (code == 1) return v > 0.f ? v : 0.f;
  if (code == 2) return v * (1.f / (1.f + std::exp(-v)));
  return v;
}

inline float dot(const float* __restrict__ a, const float* __restrict__ b, int k) {
  float s = 0.f;
#pragma omp simd reduction(+ : s)
  for (int i = 0; i < k; ++i) s += a[i] * b[i];
  return s;
}

// y[0..n) = W (n, k; row stride ldw) x + b
inline void matvec(const float* w, int64_t ldw, const float* b, const float* x, int n, int k, float* y) {
  for (int o = 0; o < n; ++o) y[o] = dot(w + (int64_t)o * ldw, x, k) + (b ? b[o] : 0.f);
}

// the two distance expressions of occ4d_knn_f32
inline float dist_metric(const float* q, const float* p, int metric) {
  const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  if (metric == 0) {
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;     // ((dx*dx + dy*dy) + dz*dz), fp32, no FMA (-ffp-contract=off)
    return (xx + yy) + zz;
  }
  return std::sqrt(std::fma(dz, dz, std::fma(dy, dy, dx * dx)));
}

// k nearest of one query: nearest first, lowest index on equal distances
void knn_one(const float* q, const float* data, int64_t ds, int n_data, int k, int metric, int32_t* idx, float* dist) {
  float bd[16];
  int32_t bi[16];
  int have = 0;
  for (int j = 0; j < n_data; ++j) {
    const float d = dist_metric(q, data + (int64_t)j * ds, metric);
    if (have == k && !(d < bd[k - 1])) continue;               // (ties keep the earlier index)
    int p = have < k ? have++ : k - 1;
    while (p > 0 && d < bd[p - 1]) {
      bd[p] = bd[p - 1];
      bi[p] = bi[p - 1];
      --p;
    }
    bd[p] = d;
    bi[p] = j;
  }
  for (int j = 0; j < k; ++j) {
    idx[j] = bi[j];
    if (dist) dist[j] = bd[j];
  }
}

// ---- one vector-attention query, as written (model/point_transformer_layer.py:168-179): q_i (D), its K neighbours'
// keys / values (rows of kf / vf) and positions -> agg (D)
struct AttnScratch {
  std::vector<float> r, pe, a, hid, logit;
  AttnScratch(int k, int d, int h) : r(h), pe((size_t)k * d), a(d), hid(2 * d), logit((size_t)k * d) {}
};
void attn_one(const occ4d_pt_layer_weights& w, const float* qi, const float* pi, const float* pos2, int64_t p2s,
              const float* kf, const float* vf, const int32_t* idx, int k, float divisor, AttnScratch& s, float* agg) {
  const int D = w.dim, h = w.pos_hidden;
  for (int j = 0; j < k; ++j) {
    const float* pj = pos2 + (int64_t)idx[j] * p2s;
    const float rel[3] = {pi[0] - pj[0], pi[1] - pj[1], pi[2] - pj[2]};
    for (int u = 0; u < h; ++u) {
      const float v = (w.pos0_w[3 * u] * rel[0] + w.pos0_w[3 * u + 1] * rel[1]) + w.pos0_w[3 * u + 2] * rel[2] + w.pos0_b[u];
      s.r[u] = v > 0.f ? v : 0.f;
    }
    float* pe = s.pe.data() + (size_t)j * D;
    matvec(w.pos2_w, h, w.pos2_b, s.r.data(), D, h, pe);                     // pos_enc = pos_mlp(rel)          (:174)
    const float* kj = kf + (int64_t)idx[j] * D;
    for (int c = 0; c < D; ++c) s.a[c] = qi[c] - kj[c] + pe[c];              // q - k + pos_enc                 (:176)
    matvec(w.attn0_w, D, w.attn0_b, s.a.data(), 2 * D, D, s.hid.data());
    for (int c = 0; c < 2 * D; ++c) s.hid[c] = s.hid[c] > 0.f ? s.hid[c] : 0.f;
    matvec(w.attn2_w, 2 * D, w.attn2_b, s.hid.data(), D, 2 * D, s.logit.data() + (size_t)j * D);
  }
  for (int c = 0; c < D; ++c) {                                              // softmax over the neighbours, per channel (:177)
    float mx = -INFINITY;
    for (int j = 0; j < k; ++j) mx = std::max(mx, s.logit[(size_t)j * D + c] / divisor);
    float den = 0.f, num = 0.f;
    for (int j = 0; j < k; ++j) {
      const float e = std::exp(s.logit[(size_t)j * D + c] / divisor - mx);
      den += e;
      num += e * (vf[(int64_t)idx[j] * D + c] + s.pe[(size_t)j * D + c]);    // attn * (v + pos_enc)            (:179)
    }
    agg[c] = num / den;
  }
}

int check_layer(const occ4d_pt_layer_weights* w, const char* who) {
  OCC4D_REQUIRE(w, "%s: null weights", who);
  OCC4D_REQUIRE(w->dim >= 1 && w->pos_hidden >= 1 && w->dim2 >= 1, "%s: bad dimensions", who);
  OCC4D_REQUIRE(w->to_q && w->to_k && w->to_v && w->pos0_w && w->pos0_b && w->pos2_w && w->pos2_b && w->attn0_w && w->attn0_b &&
          w->attn2_w && w->attn2_b,
      "%s: null parameter pointer", who);
  OCC4D_REQUIRE(!w->post_w || (w->post_b && w->d_out == (w->pre_w ? w->d_in : w->dim)), "%s: layer3 + residual needs d_out == d_in", who);
  return OCC4D_OK;
}

int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

// scene tables of a cross layer in the twin: kf = to_k(x2) (m, D), vf = to_v(x2) (m, D)
void layer_tables(const occ4d_pt_layer_weights& w, const float* x2, int64_t ldx2, int m, float* kf, float* vf) {
  const int D = w.dim, D2 = w.dim2;
#pragma omp parallel for schedule(static)
  for (int j = 0; j < m; ++j) {
    matvec(w.to_k, D2, nullptr, x2 + (int64_t)j * ldx2, D, D2, kf + (int64_t)j * D);
    matvec(w.to_v, D2, nullptr, x2 + (int64_t)j * ldx2, D, D2, vf + (int64_t)j * D);
  }
}

struct DecScene { int64_t xyz, feats, fglobal, layer[OCC4D_MAX_CROSS], total; };
DecScene dec_scene(const occ4d_decoder_weights& w, int m) {
  DecScene s{};
  int64_t o = 0;
  s.xyz = o; o += up4((int64_t)m * 3);
  s.feats = o; o += up4((int64_t)m * w.d_latent_local);
  s.fglobal = o; o += up4(w.d_latent - w.d_latent_local);
  for (int j = 0; j < w.n_cross; ++j) { s.layer[j] = o; o += up4((int64_t)2 * m * w.cross[j].dim); }
  s.total = o;
  return s;
}

}  // namespace

extern "C" {

int occ4d_abi_version(void) { return OCC4D_ABI_VERSION; }
const char* occ4d_last_error(void) { return g_err; }
int occ4d_is_cpu_twin(void) { return 1; }      // (only this library exports it)

// ---------------------------------------------------------------------------------------------------------------- geometry
int occ4d_knn_f32(const float* query, int64_t q_stride, int n_query, const float* data, int64_t d_stride, int n_data, int k,
                  int metric, void* out_idx, int idx_is_i64, float* out_dist, void*) {
  OCC4D_REQUIRE(query && data && out_idx && n_query >= 0, "occ4d_knn_f32: null pointer");
  OCC4D_REQUIRE(k >= 1 && k <= 16 && n_data >= k, "occ4d_knn_f32: k = %d must be in 1 .. 16 and <= n_data = %d", k, n_data);
  OCC4D_REQUIRE(metric == 0 || metric == 1, "occ4d_knn_f32: metric %d", metric);
#pragma omp parallel for schedule(static)
  for (int i = 0; i < n_query; ++i) {
    int32_t idx[16];
    knn_one(query + (int64_t)i * q_stride, data, d_stride, n_data, k, metric, idx, out_dist ? out_dist + (int64_t)i * k : nullptr);
    for (int j = 0; j < k; ++j) {
      if (idx_is_i64) static_cast<int64_t*>(out_idx)[(int64_t)i * k + j] = idx[j];
      else static_cast<int32_t*>(out_idx)[(int64_t)i * k + j] = idx[j];
    }
  }
  return OCC4D_OK;
}

int occ4d_knn_dists_f32(const float* query, int64_t q_stride, int n_query, const float* data, int64_t d_stride, int n_data,
                        const int32_t* idx, int k, int metric, float* out_dist, void*) {
  OCC4D_REQUIRE(query && data && idx && out_dist && n_data >= 1 && k >= 1, "occ4d_knn_dists_f32: bad arguments");
  for (int64_t p = 0; p < (int64_t)n_query * k; ++p) {
    const int j = std::min(std::max(idx[p], 0), n_data - 1);
    out_dist[p] = dist_metric(query + (p / k) * q_stride, data + (int64_t)j * d_stride, metric);
  }
  return OCC4D_OK;
}

int occ4d_fps_start_f32(const float* xyz, int64_t stride, int n, int m, int start, int32_t* out_sorted, int32_t* out_order,
                        void*) {
  OCC4D_REQUIRE(xyz && out_sorted && n >= 1 && m >= 1 && m <= n && start >= 0 && start < n, "occ4d_fps_f32: bad arguments");
  std::vector<float> best((size_t)n, INFINITY);
  std::vector<int32_t> order((size_t)m);
  int cur = start;
  for (int t = 0; t < m; ++t) {
    order[t] = cur;
    const float* pc = xyz + (int64_t)cur * stride;
    float bv = -1.f;
    int bi = 0;
    for (int i = 0; i < n; ++i) {
      const float d = dist_metric(xyz + (int64_t)i * stride, pc, 0);
      if (d < best[i]) best[i] = d;
      if (best[i] > bv) { bv = best[i]; bi = i; }          // first argmax: lowest index on ties
    }
    cur = bi;
  }
  if (out_order) std::copy(order.begin(), order.end(), out_order);
  std::sort(order.begin(), order.end());
  order.erase(std::unique(order.begin(), order.end()), order.end());
  for (int t = 0; t < m; ++t) out_sorted[t] = order[std::min<size_t>(t, order.size() - 1)];
  return OCC4D_OK;
}
int occ4d_fps_f32(const float* xyz, int64_t stride, int n, int m, int32_t* out_sorted, int32_t* out_order, void* st) {
  return occ4d_fps_start_f32(xyz, stride, n, m, 0, out_sorted, out_order, st);
}
// the dataloader's clip reduction (the front end's last step): the same selection, status word 0
int64_t occ4d_fps_coop_workspace_bytes(void) { return 64; }
int occ4d_fps_coop_f32(const float* xyz, int64_t stride, int n, int m, int start, int, int32_t* out_sorted, int32_t* out_order,
                       void* workspace, void* st) {
  OCC4D_REQUIRE(workspace, "occ4d_fps_coop_f32: null workspace");
  std::memset(workspace, 0, 64);
  return occ4d_fps_start_f32(xyz, stride, n, m, start, out_sorted, out_order, st);
}

int occ4d_nested_fps_level_i32(const int32_t* order, const int32_t* orig, int n, int m, int32_t* out_pos, int32_t* out_orig,
                               void*) {
  OCC4D_REQUIRE(order && orig && out_pos && out_orig && n >= 1 && m >= 1 && m <= n, "occ4d_nested_fps_level_i32: bad arguments");
  std::vector<int32_t> pos((size_t)m);
  for (int t = 0; t < m; ++t) pos[t] = (int32_t)(std::lower_bound(orig, orig + n, order[t]) - orig);
  std::sort(pos.begin(), pos.end());
  pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
  for (int t = 0; t < m; ++t) {
    out_pos[t] = pos[std::min<size_t>(t, pos.size() - 1)];
    out_orig[t] = orig[out_pos[t]];
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- rows
int occ4d_copy_rows_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int n, int d, void*) {
  OCC4D_REQUIRE(dst && src && n >= 0 && d >= 1, "occ4d_copy_rows_f32: bad arguments");
  for (int i = 0; i < n; ++i) std::memmove(dst + (int64_t)i * ldd, src + (int64_t)i * lds, sizeof(float) * d);
  return OCC4D_OK;
}
int occ4d_fill_rows_f32(float* dst, int64_t ld, int n, int d, float value, void*) {
  OCC4D_REQUIRE(dst && n >= 0 && d >= 1, "occ4d_fill_rows_f32: bad arguments");
  for (int i = 0; i < n; ++i) std::fill(dst + (int64_t)i * ld, dst + (int64_t)i * ld + d, value);
  return OCC4D_OK;
}
int occ4d_gather_rows_f32(const float* src, int64_t lds, const int32_t* idx, int n_out, int d, float* out, int64_t ldo, void*) {
  OCC4D_REQUIRE(src && idx && out && n_out >= 0 && d >= 1, "occ4d_gather_rows_f32: bad arguments");
  for (int i = 0; i < n_out; ++i) std::memcpy(out + (int64_t)i * ldo, src + (int64_t)idx[i] * lds, sizeof(float) * d);
  return OCC4D_OK;
}
int occ4d_mean_rows_f32(const float* x, int64_t ldx, int n, int d, float* out, void*) {
  OCC4D_REQUIRE(x && out && n >= 1 && d >= 1, "occ4d_mean_rows_f32: bad arguments");
  for (int c = 0; c < d; ++c) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[(int64_t)i * ldx + c];
    out[c] = (float)(s / n);
  }
  return OCC4D_OK;
}
int occ4d_maxpool_gather_f32(const float* y, int64_t ldy, const int32_t* idx, int n_out, int k, int d, float* z, int64_t ldz,
                             void*) {
  OCC4D_REQUIRE(y && idx && z && k >= 1 && d >= 1, "occ4d_maxpool_gather_f32: bad arguments");
  for (int i = 0; i < n_out; ++i)
    for (int c = 0; c < d; ++c) {
      float m = -INFINITY;
      for (int j = 0; j < k; ++j) m = std::max(m, y[(int64_t)idx[(int64_t)i * k + j] * ldy + c]);
      z[(int64_t)i * ldz + c] = m;
    }
  return OCC4D_OK;
}
int occ4d_layernorm_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int relu_out, float* y,
                        int64_t ldy, int n, int d, void*) {
  OCC4D_REQUIRE(x && y && n >= 0 && d >= 1, "occ4d_layernorm_f32: bad arguments");
  for (int i = 0; i < n; ++i) {
    const float* r = x + (int64_t)i * ldx;
    double mu = 0.0, var = 0.0;
    for (int c = 0; c < d; ++c) mu += r[c];
    mu /= d;
    for (int c = 0; c < d; ++c) var += (r[c] - mu) * (r[c] - mu);
    var /= d;                                                            // biased, as torch.nn.LayerNorm
    const float inv = (float)(1.0 / std::sqrt(var + (double)eps));
    for (int c = 0; c < d; ++c) {
      float v = (float)(r[c] - mu) * inv;
      if (gamma) v = v * gamma[c] + beta[c];
      y[(int64_t)i * ldy + c] = relu_out && v < 0.f ? 0.f : v;
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- Linear
int occ4d_linear_f32(const occ4d_linear_args* a, void*) {
  OCC4D_REQUIRE(a && a->x && a->w && a->y && a->M >= 0 && a->K >= 1 && a->N >= 1, "occ4d_linear_f32: bad arguments");
  OCC4D_REQUIRE(a->relu_in >= 0 && a->relu_in <= 2, "occ4d_linear_f32: Unknown activation: %d", a->relu_in);
  const int M = a->M, K = a->K, N = a->N;
#pragma omp parallel
  {
    std::vector<float> xin((size_t)K), t((size_t)N);
#pragma omp for schedule(static)
    for (int i = 0; i < M; ++i) {
      const float* xr = a->x + (int64_t)i * a->ldx;
      for (int c = 0; c < K; ++c) xin[c] = act(xr[c], a->relu_in);
      for (int o = 0; o < N; ++o) {
        float v = dot(a->w + (int64_t)o * a->ldw, xin.data(), K) + (a->bias ? a->bias[o] : 0.f);
        if (a->add_rows) v += a->add_rows[(int64_t)(i / a->add_div) * a->ld_add + o];
        if (a->sub_rows) v -= a->sub_rows[(int64_t)a->sub_idx[i] * a->ld_sub + o];
        if (a->relu_out && v < 0.f) v = 0.f;
        t[o] = v;
      }
      for (int o = 0; o < N; ++o)
        a->y[(int64_t)i * a->ldy + o] = t[o] + (a->residual ? a->residual[(int64_t)i * a->ldr + o] : 0.f);
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- decoder pieces
int occ4d_posenc_f32(const float* pts, int64_t stride, int n, int c, int n_freq, double base_freq, float* out, int64_t ldo,
                     void*) {
  OCC4D_REQUIRE(pts && out && n >= 0 && c >= 1 && n_freq >= 0, "occ4d_posenc_f32: bad arguments");
  for (int i = 0; i < n; ++i) {
    const float* p = pts + (int64_t)i * stride;
    float* o = out + (int64_t)i * ldo;
    for (int ch = 0; ch < c; ++ch) o[ch] = p[ch];
    for (int f = 0; f < n_freq; ++f) {
      const float w = (float)(2.0 * M_PI * base_freq * std::ldexp(1.0, f));   // double, rounded once (model/implicit.py:33-36)
      for (int ch = 0; ch < c; ++ch) {
        const float arg = p[ch] * w;
        o[c + 2 * c * f + ch] = std::sin(arg);
        o[c + 2 * c * f + c + ch] = std::cos(arg);
      }
    }
  }
  return OCC4D_OK;
}
int occ4d_interp_weights_f32(const float* dist, int n, int k, float* w, void*) {
  OCC4D_REQUIRE(dist && w && n >= 0 && k >= 1, "occ4d_interp_weights_f32: bad arguments");
  for (int i = 0; i < n; ++i) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) {
      w[(int64_t)i * k + j] = 1.f / (dist[(int64_t)i * k + j] + 1e-4f);
      s += std::fabs(w[(int64_t)i * k + j]);
    }
    s = std::max(s, 1e-12f);
    for (int j = 0; j < k; ++j) w[(int64_t)i * k + j] /= s;
  }
  return OCC4D_OK;
}
int occ4d_interp_add_f32(float* x, int64_t ldx, const float* cvec, const float* table, int64_t ldt, const int32_t* idx,
                         const float* w, int n, int k, int d, void*) {
  OCC4D_REQUIRE(x && table && idx && w && n >= 0 && k >= 1 && d >= 1, "occ4d_interp_add_f32: bad arguments");
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < d; ++c) {
      float s = cvec ? cvec[c] : 0.f;
      for (int j = 0; j < k; ++j) s += w[(int64_t)i * k + j] * table[(int64_t)idx[(int64_t)i * k + j] * ldt + c];
      x[(int64_t)i * ldx + c] += s;
    }
  return OCC4D_OK;
}
int occ4d_squash_f32(float* out, int64_t ld, int n, int g, const int32_t* ops_host, void*) {
  OCC4D_REQUIRE(out && ops_host && n >= 0 && g >= 1, "occ4d_squash_f32: bad arguments");
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < g; ++c) {
      float& v = out[(int64_t)i * ld + c];
      v = occ4d_track::squash(v, ops_host[c]);      // (csrc/track_math.hpp: squash_kernel's expression, the merge's too)
    }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pre / post steps
int occ4d_grid_points_f32(int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0, float sz, float t, float* out,
                          void*) {
  OCC4D_REQUIRE(out && nx >= 1 && ny >= 1 && nz >= 1, "occ4d_grid_points_f32: bad arguments");
  int64_t i = 0;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; ++iz, ++i) {
        const float ax = (float)ix + 0.5f, ay = (float)iy + 0.5f, az = (float)iz + 0.5f;   // numpy's order, no FMA
        const float mx = ax * sx, my = ay * sy, mz = az * sz;
        out[4 * i + 0] = mx + x0;
        out[4 * i + 1] = my + y0;
        out[4 * i + 2] = mz + z0;
        out[4 * i + 3] = t;
      }
  return OCC4D_OK;
}
int occ4d_compact_count_f32(const float* key, int64_t ld, int n, float threshold, int strict, int* block_counts, int* total_kept,
                            void*) {
  OCC4D_REQUIRE(key && block_counts && total_kept && n >= 0 && ld >= 1, "occ4d_compact_count_f32: bad arguments");
  int total = 0;
  for (int b = 0; b * 256 < n; ++b) {
    block_counts[b] = total;                                              // exclusive prefix
    for (int i = b * 256; i < std::min(n, (b + 1) * 256); ++i) {
      const float kv = key[(int64_t)i * ld];
      total += strict ? kv > threshold : kv >= threshold;
    }
  }
  *total_kept = total;
  return OCC4D_OK;
}
int occ4d_compact_rows_f32(const float* src, int64_t ld, int n, int d, const float* key, int64_t ld_key, float threshold,
                           int strict, const int* block_offsets, float* out_rows, float* out_key, void*) {
  // (out_rows may be null when no row is kept -- an empty torch tensor has no storage --, as in csrc/postops.hip)
  OCC4D_REQUIRE(src && key && block_offsets && n >= 0 && d >= 1 && ld >= d && ld_key >= 1, "occ4d_compact_rows_f32: bad arguments");
  int64_t kept = 0;
  for (int i = 0; i < n; ++i) {
    const float kv = key[(int64_t)i * ld_key];
    if (strict ? kv > threshold : kv >= threshold) {
      std::memcpy(out_rows + kept * d, src + (int64_t)i * ld, sizeof(float) * d);
      if (out_key) out_key[kept] = kv;
      ++kept;
    }
  }
  return OCC4D_OK;
}
int occ4d_split_count_f32(const float* implicit_output, int64_t ld, int n, float threshold, int* block_counts, int* total_solid,
                          void* st) {
  return occ4d_compact_count_f32(implicit_output, ld, n, threshold, 0, block_counts, total_solid, st);
}
int occ4d_split_write_f32(const float* pts, const float* outp, int64_t ld, int n, int g, float threshold, const int*, int compress,
                          int n_cls, float* solid, float* air, void*) {
  OCC4D_REQUIRE(pts && outp && n >= 0 && g >= 1 && ld >= g, "occ4d_split_write_f32: bad arguments");
  OCC4D_REQUIRE(!compress || n_cls >= 1, "occ4d_split_write_f32: bad n_classes");
  int64_t ns = 0, na = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = pts + (int64_t)i * 4;
    const float* o = outp + (int64_t)i * ld;
    if (o[0] >= threshold) {
      float* d = solid + ns++ * (4 + g);
      std::memcpy(d, p, 16);
      std::memcpy(d + 4, o, sizeof(float) * g);
    } else if (compress) {
      float* d = air + na++ * 5;
      const int width = 4 + g, start = width > n_cls ? width - n_cls : 0;   // numpy negative-slice semantics (:299-305)
      int best = 0;
      float bv = start < 4 ? p[start] : o[start - 4];
      for (int c = start + 1; c < width; ++c) {
        const float v = c < 4 ? p[c] : o[c - 4];
        if (v > bv) { bv = v; best = c - start; }
      }
      d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = o[0]; d[4] = (float)best;
    } else {
      float* d = air + na++ * (4 + g);
      std::memcpy(d, p, 16);
      std::memcpy(d + 4, o, sizeof(float) * g);
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- front end
// include/occ4d_frontend.h: the loops of csrc/frontend.hip over csrc/frontend_math.hpp
int occ4d_rgbd_rows_f32(const float* depth, const float* rgb, const float* flat, const float* k_inv, const float* rt_inv,
                        const float* hue_clusters, int n_clusters, int T, int H, int W, float x_min, float x_max, float y_min,
                        float y_max, float z_min, float z_max, int floor_fix, int view_idx, float* out_rows, float* out_target,
                        float* out_key, void*) {
  int64_t total;
  OCC4D_TRY(fe::check_rgbd_rows(depth, rgb, flat, k_inv, rt_inv, hue_clusters, n_clusters, T, H, W, out_rows, out_key, total));
  const int64_t hw = (int64_t)H * W;
#pragma omp parallel for schedule(static)
  for (int64_t p = 0; p < total; ++p) {
    const int t = (int)(p / hw), pix = (int)(p % hw);
    const float z = depth[p];
    float xyz[3];
    fe::unproject(k_inv + 16 * t, rt_inv + 16 * t, (float)(pix % W), (float)(pix / W), z, xyz);
    const bool keep = z > 0.f && fe::in_cuboid(xyz, x_min, x_max, y_min, y_max, z_min, z_max, floor_fix != 0);
    const float inst = flat ? fe::instance_id(flat[3 * p], flat[3 * p + 1], flat[3 * p + 2], hue_clusters, n_clusters) : -1.f;
    const float row[8] = {xyz[0], xyz[1], xyz[2], inst, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], (float)t};
    std::memcpy(out_rows + 8 * p, row, sizeof row);
    if (out_target) {
      const float tgt[8] = {xyz[0], xyz[1], xyz[2], inst, (float)view_idx, row[4], row[5], row[6]};
      std::memcpy(out_target + 8 * p, tgt, sizeof tgt);
    }
    out_key[p] = keep ? 1.f : 0.f;
  }
  return OCC4D_OK;
}

int occ4d_lidar_rows_f32(const float* rows, int64_t ld, int n, int d, const float* source, const float* inv_target, float z_offset,
                         int cube_mode, double min_z, double other_bounds, float* out_rows, int64_t ldo, float* out_key, void*) {
  bool empty;
  OCC4D_TRY(fe::check_lidar_rows(rows, ld, n, d, source, inv_target, cube_mode, out_rows, ldo, out_key, empty));
  if (empty) return OCC4D_OK;
  const fe::Cuboid c = fe::carla_input_cuboid(cube_mode, min_z, other_bounds);
#pragma omp parallel for schedule(static)
  for (int i = 0; i < n; ++i)
    fe::lidar_row(rows, ld, d, source, inv_target, source != nullptr, z_offset, cube_mode != 0, c, out_rows, ldo, out_key, i);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- evaluation
// include/occ4d_eval.h: the loops of csrc/evalstats.hip over csrc/eval_math.hpp, rows in order, sums sequential
int64_t occ4d_eval_counts_len(int n_groups, int n_classes) { return ev::counts_len(n_groups, n_classes); }
int64_t occ4d_eval_sums_len(int n_groups) { return ev::sums_len(n_groups); }
int64_t occ4d_eval_workspace_bytes(int n) { return n < 0 ? -1 : 8; }

int occ4d_eval_query_stats_f32(const float* out, int64_t ldo, int n, int g_out, const int32_t* nn_idx, const float* nn_dist,
                               const float* target, int64_t ldt, int m, int dt, int col_rgb, int col_track, int col_sem, int out_track,
                               const int32_t* target_group, int n_groups, int n_classes, float density_threshold, float radius,
                               int flags, int64_t* counts, double* sums, void* workspace, void*) {
  ev::QueryArgs a; bool empty;
  OCC4D_TRY(ev::check_query_stats(out, ldo, n, g_out, nn_idx, nn_dist, target, ldt, m, dt, col_rgb, col_track, col_sem, out_track,
                                  target_group, n_groups, n_classes, density_threshold, radius, flags, counts, sums, workspace,
                                  empty, a));
  if (empty) return OCC4D_OK;
  const int64_t stride = ev::group_stride(n_classes);
  double call[OCC4D_EVAL_MAX_GROUPS * OCC4D_EVAL_GROUP_SUMS] = {};      // the call's own totals, added onto the running values at the end
  for (int i = 0; i < n; ++i) {
    const ev::QueryRow r = ev::classify_query(a, i);
    if (r.group < 0) {
      ++counts[OCC4D_EVAL_BAD_ROWS];
      continue;
    }
    int64_t* c = counts + OCC4D_EVAL_HEAD + r.group * stride;
    double* s = call + r.group * OCC4D_EVAL_GROUP_SUMS;
    ++c[r.occ];
    if (r.solid) {
      ++c[OCC4D_EVAL_N_ACCURACY];
      s[OCC4D_EVAL_SUM_ACCURACY_D] += r.d;
      s[OCC4D_EVAL_SUM_ACCURACY_D2] += r.d2;
    }
    if (r.color) {
      ++c[OCC4D_EVAL_N_COLOR];
      s[OCC4D_EVAL_SUM_COLOR_L1] += r.l1;
    }
    if (r.track >= 0) ++c[r.track];
    if (r.seg >= 0) {
      ++c[OCC4D_EVAL_GROUP_COUNTS + r.seg];
      ++c[OCC4D_EVAL_N_SEG];
    } else if (r.seg == -2) {
      ++c[OCC4D_EVAL_SEG_IGNORED];
    }
  }
  for (int k = 0; k < n_groups * OCC4D_EVAL_GROUP_SUMS; ++k) sums[k] += call[k];
  return OCC4D_OK;
}

int occ4d_eval_target_stats_f32(const float* dist, int m, const int32_t* target_group, int n_groups, int n_classes, int64_t* counts,
                                double* sums, void* workspace, void*) {
  bool empty;
  OCC4D_TRY(ev::check_target_stats(dist, m, n_groups, n_classes, counts, sums, workspace, empty));
  if (empty) return OCC4D_OK;
  const int64_t stride = ev::group_stride(n_classes);
  double call[OCC4D_EVAL_MAX_GROUPS * OCC4D_EVAL_GROUP_SUMS] = {};
  for (int j = 0; j < m; ++j) {
    const int g = ev::group_of(target_group, j, m, n_groups);
    if (g < 0) {
      ++counts[OCC4D_EVAL_BAD_ROWS];
      continue;
    }
    ++counts[OCC4D_EVAL_HEAD + g * stride + OCC4D_EVAL_N_COMPLETENESS];
    const double d = (double)dist[j];
    call[g * OCC4D_EVAL_GROUP_SUMS + OCC4D_EVAL_SUM_COMPLETENESS_D] += d;
    call[g * OCC4D_EVAL_GROUP_SUMS + OCC4D_EVAL_SUM_COMPLETENESS_D2] += d * d;
  }
  for (int k = 0; k < n_groups * OCC4D_EVAL_GROUP_SUMS; ++k) sums[k] += call[k];
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- id histogram
// include/occ4d_occl.h: the walk of csrc/idhist.hip over csrc/occl_math.hpp, rows in order.  The offsets are host memory
// here, so the contract on them is checked.
int occ4d_id_histogram_f32(const float* rows, int64_t ld, int n, int col, const int64_t* seg_offsets, int n_segments, int n_ids,
                           const float* key, int pred_col, float pred_a, float pred_b, int32_t* counts, void*) {
  const char* who = "occ4d_id_histogram_f32";
  oc::HistArgs a; bool empty;
  OCC4D_TRY(oc::check_id_histogram(rows, ld, n, col, seg_offsets, n_segments, n_ids, key, pred_col, pred_a, pred_b, counts, empty, a));
  if (empty) return OCC4D_OK;
  OCC4D_REQUIRE(seg_offsets[0] == 0 && seg_offsets[n_segments] == n, "%s: seg_offsets must run from 0 to n = %d, got %lld .. %lld", who, n,
                (long long)seg_offsets[0], (long long)seg_offsets[n_segments]);
  for (int s = 0; s < n_segments; ++s)
    OCC4D_REQUIRE(seg_offsets[s] <= seg_offsets[s + 1], "%s: seg_offsets must ascend (segment %d: %lld > %lld)", who, s,
                  (long long)seg_offsets[s], (long long)seg_offsets[s + 1]);
  const int bins = n_ids + OCC4D_OCCL_EXTRA_BINS;
  for (int64_t i = 0; i < n; ++i) {
    const int bin = oc::bin_of(a, i);
    if (bin < 0) continue;
    const int seg = oc::segment_end_index(seg_offsets, n_segments, i) - 1;
    ++counts[(int64_t)seg * bins + bin];
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- track merge
// include/occ4d_track.h: the passes of csrc/trackmerge.hip over csrc/track_math.hpp, elements in order.
int occ4d_track_merge_add_f32(const float* out, int64_t ld_out, int n, int g, const int32_t* ops_host, int track_col, float inst_id,
                              int first, float* acc, int64_t ld_acc, float* best, float* winner, void*) {
  tk::AddArgs a; bool empty;
  OCC4D_TRY(tk::check_merge_add(out, ld_out, n, g, ops_host, track_col, inst_id, first, acc, ld_acc, best, winner, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < g; ++c) {
      float& dst = acc[i * ld_acc + c];
      const float raw = out[i * ld_out + c];
      dst = first ? tk::add_one<true>(a, raw, 0.f, i, c) : tk::add_one<false>(a, raw, dst, i, c);
    }
  return OCC4D_OK;
}
int occ4d_track_merge_finish_f32(float* acc, int64_t ld_acc, int n, int g, int n_runs, int track_col, const float* winner, void*) {
  tk::FinishArgs f; bool empty;
  OCC4D_TRY(tk::check_merge_finish(acc, ld_acc, n, g, n_runs, track_col, winner, empty, f));
  if (empty) return OCC4D_OK;
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < g; ++c) {
      float& v = acc[i * ld_acc + c];
      v = tk::finish_one(f, v, i, c);
    }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- grid refinement
// include/occ4d_refine.h: the passes of csrc/refine.hip over csrc/refine_math.hpp, blocks, points and rows in order.  A selected
// row's position is block_offsets[tile] + its rank in the tile, as on the device: never a running count over the whole grid.
int occ4d_refine_mark_f32(const float* rep_density, int64_t ld_rep, int nx, int ny, int nz, int b, int dilate, int op, float low,
                          int32_t* active, float* key, void*) {
  rf::MarkArgs a; bool empty;
  OCC4D_TRY(rf::check_mark(rep_density, ld_rep, nx, ny, nz, b, dilate, op, low, active, key, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t blk = 0; blk < a.grid.blocks; ++blk) active[blk] = rf::active_of(a, blk);
  for (int64_t i = 0; i < a.grid.n; ++i) key[i] = rf::key_of(a, i);
  return OCC4D_OK;
}
int occ4d_refine_expand_f32(const float* key, const int32_t* block_offsets, const float* rep_out, int64_t ld_rep, const float* fine_out,
                            int64_t ld_fine, int n_fine, int nx, int ny, int nz, int b, int g, float* out, int64_t ld_out, void*) {
  rf::ExpandArgs e; bool empty;
  OCC4D_TRY(rf::check_expand(key, block_offsets, rep_out, ld_rep, fine_out, ld_fine, n_fine, nx, ny, nz, b, g, out, ld_out, empty, e));
  if (empty) return OCC4D_OK;
  for (int64_t tile = 0; tile < e.tiles; ++tile) {
    int64_t rank = 0;
    for (int64_t i = tile * rf::TILE; i < std::min(e.grid.n, (tile + 1) * rf::TILE); ++i) {
      const bool selected = rf::kept(key[i]);
      std::memcpy(out + i * ld_out, rf::source_row(e, i, selected, (int64_t)block_offsets[tile] + rank), sizeof(float) * g);
      rank += selected;
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- surface nets
// include/occ4d_surface.h: the passes of csrc/surface.hip over csrc/surface_math.hpp, tiles and points in order.  A vertex or face
// number is its tile's offset + the rank in the tile, as on the device: never a running count over the whole grid.
int occ4d_surface_count_f32(const float* density, int64_t ld, int nx, int ny, int nz, float level, int32_t* cell_offsets,
                            int32_t* face_offsets, int32_t* totals, void*) {
  sf::CountArgs a; bool empty;
  OCC4D_TRY(sf::check_count(density, ld, nx, ny, nz, level, cell_offsets, face_offsets, totals, empty, a));
  if (empty) return OCC4D_OK;
  int32_t cells = 0, quads = 0;
  float v[8];
  for (int64_t tile = 0; tile < a.tiles; ++tile) {
    cell_offsets[tile] = cells;                                           // exclusive prefixes
    face_offsets[tile] = quads;
    for (int64_t i = tile * sf::TILE; i < std::min(a.f.grid.points, (tile + 1) * sf::TILE); ++i) {
      const sf::Item it = sf::item_of(a.f, i, v);
      cells += sf::crossed(it.mask);
      quads += sf::quads_of(it.axes);
    }
  }
  totals[0] = cells;
  totals[1] = quads;
  return OCC4D_OK;
}
int occ4d_surface_write_f32(const float* density, int64_t ld, const float* attrs, int64_t ld_attr, int n_attr, int nx, int ny, int nz,
                            float level, float x0, float sx, float y0, float sy, float z0, float sz, const int32_t* cell_offsets,
                            const int32_t* face_offsets, int32_t* work, float* vertices, int64_t ld_v, int vertex_cap,
                            int32_t* faces, int face_cap, void*) {
  sf::WriteArgs w; bool empty;
  OCC4D_TRY(sf::check_write(density, ld, attrs, ld_attr, n_attr, nx, ny, nz, level, x0, sx, y0, sy, z0, sz, cell_offsets, face_offsets,
                            work, vertices, ld_v, vertex_cap, faces, face_cap, empty, w));
  if (empty) return OCC4D_OK;
  float v[8];
  for (int pass = 0; pass < 2; ++pass)                                    // the vertex pass, then the face pass (it reads work)
    for (int64_t tile = 0; tile < w.tiles; ++tile) {
      int64_t cells = 0, quads = 0;
      for (int64_t i = tile * sf::TILE; i < std::min(w.f.grid.points, (tile + 1) * sf::TILE); ++i) {
        const sf::Item it = sf::item_of(w.f, i, v);
        if (pass == 0) sf::vertex_item(w, i, it, v, (int64_t)cell_offsets[tile] + cells);
        else sf::face_item(w, i, it, (int64_t)face_offsets[tile] + quads);
        cells += sf::crossed(it.mask);
        quads += sf::quads_of(it.axes);
      }
    }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ray cast
// include/ext/occ4d_raycast.h: the item body of csrc/raycast.hip over csrc/raycast_math.hpp, pixels in order.
int occ4d_raycast_grid_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                           float sz, float level, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth,
                           float step, int n_steps, const float* attrs, int64_t ld_attr, int d, const int32_t* cols_host, int C,
                           float depth_background, float feat_background, float* depth, int32_t* cell, float* feat, void*) {
  ry::Args a; bool empty;
  OCC4D_TRY(ry::check_raycast(field, ld, nx, ny, nz, x0, sx, y0, sy, z0, sz, level, k_inv, rt_inv, V, H, W, near_depth, step, n_steps,
                              attrs, ld_attr, d, cols_host, C, depth_background, feat_background, depth, cell, feat, empty, a));
  if (empty || (!a.depth && !a.cell && !a.feat)) return OCC4D_OK;
#pragma omp parallel for collapse(2) schedule(dynamic, 4)
  for (int v = 0; v < V; ++v)
    for (int py = 0; py < H; ++py)
      for (int px = 0; px < W; ++px) ry::pixel_item(a, v, px, py);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- sweep
// include/ext/occ4d_sweep.h: the item body of csrc/sweep.hip over csrc/sweep_math.hpp, rays in order.
int occ4d_sweep_rays_f32(const float* field, int64_t ld, int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0,
                         float sz, float level, const float* pose, const float* dirs, int V, int B, int A, int per_view,
                         float near_range, float step, int n_steps, const float* attrs, int64_t ld_attr, int d,
                         const int32_t* cols_host, int C, int sem_first, int n_sem, const int32_t* labels, int K,
                         float range_background, float feat_background, float* range, float* point, int32_t* cell, int32_t* owner,
                         float* cosine, int32_t* sem, int32_t* inst, float* feat, void*) {
  sw::Args a; bool empty;
  OCC4D_TRY(sw::check_sweep(field, ld, nx, ny, nz, x0, sx, y0, sy, z0, sz, level, pose, dirs, V, B, A, per_view, near_range, step, n_steps,
                            attrs, ld_attr, d, cols_host, C, sem_first, n_sem, labels, K, range_background, feat_background, range, point,
                            cell, owner, cosine, sem, inst, feat, empty, a));
  if (empty || sw::writes_nothing(a)) return OCC4D_OK;
#pragma omp parallel for collapse(2) schedule(dynamic, 64)
  for (int v = 0; v < V; ++v)
    for (int r = 0; r < a.R; ++r) sw::ray_item(a, v, r);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- evidence
// include/ext/occ4d_evidence.h: the body of a return and the code of a cell of csrc/evidence_math.hpp, RETURNS AND CELLS IN ORDER,
// the atomics spelled as plain memory operations (one thread).
namespace {
struct PlainMarks {
  uint32_t* words;
  int32_t *hits, *passes;
  void hit(int32_t flat) const { hits[flat] += 1; }
  void pass(int32_t flat) const {
    words[flat >> 5] |= 1u << (flat & 31);
    if (passes) passes[flat] += 1;
  }
  void arrive(int32_t flat) const { pass(flat); }
};
}  // namespace
int occ4d_evidence_carve_f32(const float* returns, int64_t ld_returns, int64_t R, const int32_t* sensor, const int32_t* origins, int V,
                             int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0, float sz, uint32_t* passed,
                             int32_t* hits, int32_t* passes, int32_t* status, void*) {
  ed::CarveArgs a;
  OCC4D_TRY(ed::check_carve(returns, ld_returns, R, sensor, origins, V, nx, ny, nz, x0, sx, y0, sy, z0, sz, passed, hits, passes, status, a));
  for (int64_t p = 0; p < a.points; ++p) hits[p] = 0;
  for (int64_t p = 0; passes && p < a.points; ++p) passes[p] = 0;
  for (int64_t w = 0; w < a.words; ++w) passed[w] = 0u;
  for (int k = 0; k < 4; ++k) status[k] = 0;
  const PlainMarks marks{passed, hits, passes};
  for (int64_t r = 0; r < R; ++r) status[ed::return_item(a, r, marks)] += 1;
  return OCC4D_OK;
}
int occ4d_evidence_classify_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                                int64_t n, const uint32_t* passed, const int32_t* passes, int min_pass, const int32_t* hits,
                                int32_t* code, int64_t* totals, void*) {
  ed::ClassifyArgs a;
  OCC4D_TRY(ed::check_classify(field, ld, level, mask, ld_mask, mask_level, n, passed, passes, min_pass, hits, code, totals, a));
  for (int k = 0; k < 6; ++k) totals[k] = 0;
  for (int64_t p = 0; p < n; ++p) totals[code[p] = ed::code_of(a, p)] += 1;
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- components
// include/ext/occ4d_components.h: the passes of csrc/components.hip over csrc/components_math.hpp, tiles and points in order, the
// atomics spelled as plain memory operations (one thread).  A kept root's number is its tile's prefix + its rank in the tile.
int occ4d_components_label_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                               const int32_t* klass, int nx, int ny, int nz, int connectivity, int min_size, int32_t* work,
                               int32_t* labels, int32_t* totals, void*) {
  cc::LabelArgs a; bool empty;
  OCC4D_TRY(cc::check_label(field, ld, level, mask, ld_mask, mask_level, klass, nx, ny, nz, connectivity, min_size, work, labels, totals,
                            empty, a));
  if (empty) return OCC4D_OK;
  const cc::Grid& g = a.grid;
  int32_t s_parent[256], s_key[256];
  for (int64_t tile = 0; tile < g.local_tiles; ++tile) {                  // pass 1: its three steps, a barrier = the end of a loop
    for (int t = 0; t < 256; ++t) cc::local_init(a, cc::local_point(g, tile, t), t, s_parent, s_key);
    for (int t = 0; t < 256; ++t) cc::local_link<cc::Plain>(a, cc::local_point(g, tile, t), t, s_parent, s_key);
    for (int t = 0; t < 256; ++t) cc::local_write<cc::Plain>(a, g, tile, cc::local_point(g, tile, t), t, s_parent);
  }
  for (int64_t p = 0; p < g.points; ++p) cc::border_item<cc::Plain>(a, p);                    // pass 2
  for (int64_t p = 0; p < g.points; ++p) {                                                    // pass 3
    const int r = cc::flatten_item(a, p);
    if (r >= 0) a.size[r] += 1;
  }
  int32_t sums[3] = {0, 0, 0};
  for (int64_t tile = 0; tile < g.number_tiles; ++tile) {                 // passes 4 to 6: counts, exclusive prefixes, numbers
    a.kept_roots[tile] = sums[0];
    a.kept_points[tile] = sums[1];
    a.all_roots[tile] = sums[2];
    for (int64_t p = tile * cc::TILE; p < std::min(g.points, (tile + 1) * cc::TILE); ++p) {
      if (cc::is_kept_root(a, p)) a.parent[p] = sums[0]++;               // (parent[p] is read by no test of this loop)
      sums[1] += cc::is_kept_point(a, p);
      sums[2] += cc::is_root(a, p);
    }
  }
  for (int c = 0; c < 3; ++c) totals[c] = sums[c];
  for (int64_t p = 0; p < g.points; ++p) cc::label_item(a, p);                                // pass 7
  return OCC4D_OK;
}
int occ4d_components_table_i64(const int32_t* labels, const int32_t* klass, int nx, int ny, int nz, const int32_t* totals,
                               int64_t* table, int cap, void*) {
  cc::TableArgs a; bool empty;
  OCC4D_TRY(cc::check_table(labels, klass, nx, ny, nz, totals, table, cap, empty, a));
  if (empty) return OCC4D_OK;
  const int rows = cc::table_rows(a);
  for (int k = 0; k < rows; ++k) cc::table_init_row(a, k);
  for (int64_t p = 0; p < a.grid.points; ++p)                             // one contribution per point: a run of one
    if (labels[p] >= 0) cc::table_add<cc::PlainTable>(a, labels[p], rows, cc::contribution_of(a, p));
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- link
// include/ext/occ4d_link.h: the passes of csrc/link.hip over csrc/link_math.hpp, items in order, the atomics spelled as plain memory
// operations (one thread); every point is a run of one, and a pair's number is its tile's prefix + its root's rank in the tile.
int occ4d_link_overlap_i32(const int32_t* labels_a, const int32_t* labels_b, int k_a, int k_b, int64_t n, int32_t* work,
                           int64_t* pairs, int cap, int32_t* totals, void*) {
  lk::OverlapArgs a; bool empty;
  OCC4D_TRY(lk::check_overlap(labels_a, labels_b, k_a, k_b, n, work, pairs, cap, totals, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t i = 0; i < std::max(a.table.slots, n); ++i) lk::clear_item(a, i);              // pass 1
  int32_t members = 0, numbered = 0;
  for (int64_t tile = 0; tile < a.tiles; ++tile) {                                            // pass 2
    a.tile_members[tile] = members;
    for (int64_t p = tile * lk::TILE; p < std::min(n, (tile + 1) * lk::TILE); ++p) {
      const int64_t key = lk::key_of(a, p);
      if (key == lk::EMPTY) continue;
      lk::insert_item<lk::Plain>(a, key, 1, p);
      ++members;
    }
  }
  for (int64_t s = 0; s < a.table.slots; ++s) lk::mark_item(a, s);                            // pass 3
  for (int64_t tile = 0; tile < a.tiles; ++tile) {                                            // passes 4 to 6
    a.tile_pairs[tile] = numbered;
    for (int64_t p = tile * lk::TILE; p < std::min(n, (tile + 1) * lk::TILE); ++p)
      if (lk::is_pair_root(a, p)) lk::pair_write(a, p, numbered++);
  }
  totals[0] = numbered;
  totals[1] = members;
  return OCC4D_OK;
}
int occ4d_link_match_i32(const int64_t* pairs, const int32_t* totals, int cap, const int64_t* table_a, int64_t ld_a,
                         const int64_t* table_b, int64_t ld_b, int k_a, int k_b, const int32_t* track_a, int iou_num, int iou_den,
                         const int32_t* next_in, int32_t* link, int32_t* best_a, int32_t* next_out, void*) {
  lk::MatchArgs m;
  OCC4D_TRY(lk::check_match(pairs, totals, cap, table_a, ld_a, table_b, ld_b, k_a, k_b, track_a, iou_num, iou_den, next_in, link, best_a,
                            next_out, m));
  const int rows = lk::pair_rows(m);
  for (int64_t k = 0; k < std::max(k_a, k_b); ++k) lk::init_item(m, k);                       // pass 1
  for (int i = 0; i < rows; ++i) lk::best_item<lk::Plain>(m, rows, i);                        // pass 2
  for (int64_t b = 0; b < k_b; ++b) lk::resolve_item(m, rows, b);                             // pass 3
  for (int64_t ka = 0; ka < k_a; ++ka) lk::finish_item(m, rows, ka);                          // pass 4
  int32_t next = next_in[0];                                                                  // pass 5
  for (int64_t b = 0; b < k_b; ++b)
    if (lk::is_new(m, b)) lk::new_id(m, b, next++);
  next_out[0] = next;
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- distance
// include/ext/occ4d_distance.h: the three stages of csrc/distance.hip over csrc/distance_math.hpp, LINE BY LINE (a tile of width 1):
// the line's pairs staged, then each of its points' minimum written in place.
int occ4d_distance_grid_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                            int target, int nx, int ny, int nz, int wx, int wy, int wz, int32_t* dist2, int32_t* nearest, void*) {
  dm::Args a; bool empty;
  OCC4D_TRY(dm::check_distance(field, ld, level, mask, ld_mask, mask_level, target, nx, ny, nz, wx, wy, wz, dist2, nearest, empty, a));
  if (empty) return OCC4D_OK;
  std::vector<int32_t> s_cost(dm::MAX_AXIS), s_site(dm::MAX_AXIS);
  for (int stage = 0; stage < 3; ++stage) {
    const dm::Pass ps = dm::pass_of(a, stage, 1);
    const int slots = dm::tile_slots(ps);
    for (int64_t b = 0; b < ps.tiles; ++b) {
      const dm::Tile t = dm::tile_of(ps, b);
      for (int s = 0; s < slots; ++s) dm::stage_item(a, ps, t, s, s_cost.data(), nearest ? s_site.data() : nullptr);
      for (int s = 0; s < slots; ++s) dm::min_item(a, ps, t, s, s_cost.data(), nearest ? s_site.data() : nullptr);
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- geodesic
// include/ext/occ4d_geodesic.h: the passes of csrc/geodesic.hip over csrc/geodesic_math.hpp with ONE TILE, THE WHOLE GRID, relaxed in
// place: a round sweeps the points forwards and backwards in turn until a sweep lowers nothing (a `for` bounded by the grid's points)
// -- another tiling and another order of events than the kernel's, the same fixed point.
int occ4d_geodesic_grid_i32(const int32_t* clear, int min_clear, int nx, int ny, int nz, const int32_t* seeds, int n_seeds,
                            int connectivity, int step_face, int step_edge, int step_corner, int rounds, int resume, int32_t* work,
                            int32_t* cost, int32_t* parent, int32_t* status, void*) {
  gm::Args a; bool empty;
  OCC4D_TRY(gm::check_geodesic(clear, min_clear, nx, ny, nz, seeds, n_seeds, connectivity, step_face, step_edge, step_corner, rounds,
                               resume, work, cost, parent, status, empty, a));
  if (empty) return OCC4D_OK;
  for (int k = 0; k <= rounds; ++k) a.flags[k] = k == 0 ? 1 : 0;
  if (!resume) {
    for (int64_t p = 0; p < a.points; ++p) a.cost[p] = gm::NONE;
    for (int k = 0; k < n_seeds; ++k) {
      const int64_t p = gm::seed_point(a, k);
      if (p >= 0) a.cost[p] = 0;
    }
  }
  for (int k = 1; k <= rounds && a.flags[k - 1]; ++k) {
    for (int64_t it = 0; it < a.points; ++it) {
      bool lowered = false;
      for (int64_t u = 0; u < a.points; ++u) {
        const int64_t p = it % 2 ? a.points - 1 - u : u;
        if (!gm::passable(a, p)) continue;
        int i[3];
        gm::coords_of(a, p, i);
        const int32_t best = gm::relax_point(a.rank, a.step, a.cost[p], gm::GridAt{a, i});
        if (best < a.cost[p]) {
          a.cost[p] = best;
          lowered = true;
        }
      }
      if (!lowered) break;
      a.flags[k] = 1;
    }
  }
  int changed = 0;
  for (int k = 1; k <= rounds; ++k) changed += a.flags[k] != 0;
  gm::status_item(a, changed);
  if (parent)
    for (int64_t p = 0; p < a.points; ++p) gm::parent_item(a, p);
  return OCC4D_OK;
}

int occ4d_geodesic_trace_i32(const int32_t* cost, const int32_t* parent, int n, const int32_t* goals, int n_goals, int cap,
                             int32_t* paths, int32_t* path_len, void*) {
  gm::TraceArgs a; bool empty;
  OCC4D_TRY(gm::check_trace(cost, parent, n, goals, n_goals, cap, paths, path_len, empty, a));
  if (empty) return OCC4D_OK;
  for (int g = 0; g < n_goals; ++g) gm::trace_item(a, g);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- watershed
// include/ext/occ4d_watershed.h: the passes of csrc/watershed.hip over csrc/watershed_math.hpp with ONE TILE, THE WHOLE GRID (the
// ascent reads its neighbours straight from height[]), points in order, the atomics spelled as plain memory operations (one
// thread); every point is a run of one.
int occ4d_watershed_label_i32(const int32_t* height, int nx, int ny, int nz, int connectivity, int h, int min_size, int32_t* work,
                              int32_t* labels, int32_t* totals, void*) {
  ws::Args a; bool empty;
  OCC4D_TRY(ws::check_label(height, nx, ny, nz, connectivity, h, min_size, work, labels, totals, empty, a));
  if (empty) return OCC4D_OK;
  const int64_t n = a.grid.points;
  for (int k = 0; k < ws::ROUND_WORDS; ++k) ws::flag_init(a, k);
  for (int64_t p = 0; p < n; ++p) {                                                           // ascent
    int i[3];
    cc::coords_of(a.grid, p, i);
    const int32_t own = ws::level_of(height[p]);
    ws::ascent_item(a, p, own, own < 1 ? ws::SELF : ws::ascent_choice(a.rank, own, ws::GridAt{a, i}));
  }
  for (int k = 1; k <= a.rounds && a.flags[k - 1]; ++k)                                       // jump rounds
    for (int64_t p = 0; p < n; ++p)
      if (ws::jump_item<ws::Plain>(a, p)) a.flags[k] = 1;
  for (int64_t p = 0; p < n; ++p) ws::merge_item<ws::Plain>(a, p);                            // merge
  for (int64_t p = 0; p < n; ++p) {                                                           // flatten
    const int r = ws::flatten_item(a, p);
    if (r < 0) continue;
    a.size[r] += 1;
    a.low[r] = std::min(a.low[r], (int32_t)p);
  }
  int32_t sums[ws::TOTALS] = {0, 0, 0, 0};
  for (int64_t tile = 0; tile < a.grid.number_tiles; ++tile) {                                // counts and their exclusive prefixes
    for (int c = 0; c < ws::TOTALS; ++c) a.counts[c][tile] = sums[c];
    for (int64_t p = tile * ws::TILE; p < std::min(n, (tile + 1) * ws::TILE); ++p)
      for (int c = 0; c < ws::TOTALS; ++c) sums[c] += ws::flag_of(a, p, c);
  }
  for (int c = 0; c < ws::TOTALS; ++c) totals[c] = sums[c];
  for (int64_t tile = 0; tile < a.grid.number_tiles; ++tile) {                                // numbers: the prefix + the rank in the tile
    int rank = 0;
    for (int64_t p = tile * ws::TILE; p < std::min(n, (tile + 1) * ws::TILE); ++p)
      if (ws::is_kept_root(a, p)) ws::number_item(a, p, a.counts[0][tile] + rank++);
  }
  for (int64_t p = 0; p < n; ++p) ws::label_item(a, p);                                       // labels
  return OCC4D_OK;
}
int occ4d_watershed_peaks_i32(const int32_t* height, const int32_t* labels, int n, const int32_t* totals, int32_t* peaks, int cap,
                              void*) {
  ws::PeakArgs a; bool empty;
  OCC4D_TRY(ws::check_peaks(height, labels, n, totals, peaks, cap, empty, a));
  if (empty) return OCC4D_OK;
  const int rows = ws::peak_rows(a);
  for (int k = 0; k < rows; ++k) a.keys[k] = 0;
  for (int64_t p = 0; p < n; ++p) {
    unsigned long long key;
    const int k = ws::peak_contribution(a, p, rows, key);
    if (k >= 0) a.keys[k] = std::max(a.keys[k], key);
  }
  for (int k = 0; k < rows; ++k) ws::peak_unpack(a, k);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- sight
// include/ext/occ4d_sight.h: the member test, the walk and the body of a query of csrc/sight_math.hpp, ALL QUERIES IN FLAT ORDER,
// another order than the kernel's blocks.
int occ4d_sight_bits_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level, int64_t n,
                         uint32_t* bits, void*) {
  sm::BitsArgs a; bool empty;
  OCC4D_TRY(sm::check_bits(field, ld, level, mask, ld_mask, mask_level, n, bits, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t w = 0; w < a.words; ++w) {
    uint32_t word = 0;
    for (int64_t p = w * 32; p < n && p < w * 32 + 32; ++p) word |= (uint32_t)sm::member(a, p) << (p & 31);
    bits[w] = word;
  }
  return OCC4D_OK;
}
int occ4d_sight_grid_u32(const uint32_t* bits, int nx, int ny, int nz, const int32_t* origins_host, int V, const int32_t* framed,
                         int32_t* seen, int32_t* blocker, int flags, void*) {
  sm::Args a; bool empty;
  OCC4D_TRY(sm::check_grid(bits, nx, ny, nz, origins_host, V, framed, seen, blocker, flags, empty, a));
  if (empty) return OCC4D_OK;
  for (int x = 0; x < nx; ++x)
    for (int y = 0; y < ny; ++y)
      for (int z = 0; z < nz; ++z) sm::query_item(a, sm::GlobalWords{bits}, x, y, z);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pull
// include/ext/occ4d_pull.h: the blocked test, HIT and the candidate test of csrc/pull_math.hpp, GOALS AND CANDIDATES IN ORDER: per
// anchor the candidates from the far end one at a time, the first free one is the largest.
int occ4d_pull_bits_i32(const int32_t* clear, int min_clear, int64_t n, uint32_t* blocked, void*) {
  pm::BitsArgs a; bool empty;
  OCC4D_TRY(pm::check_bits(clear, min_clear, n, blocked, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t w = 0; w < a.words; ++w) {
    uint32_t word = 0;
    for (int64_t p = w * 32; p < n && p < w * 32 + 32; ++p) word |= (uint32_t)pm::blocked_at(a, p) << (p & 31);
    blocked[w] = word;
  }
  return OCC4D_OK;
}
int occ4d_pull_pairs_u32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* a, const int32_t* b, int n_pairs, int32_t* hit,
                         void*) {
  pm::PairArgs args; bool empty;
  OCC4D_TRY(pm::check_pairs(blocked, nx, ny, nz, a, b, n_pairs, hit, empty, args));
  if (empty) return OCC4D_OK;
  for (int i = 0; i < n_pairs; ++i) hit[i] = pm::hit(args.n, args.points, sm::GlobalWords{blocked}, a[i], b[i]);
  return OCC4D_OK;
}
int occ4d_pull_paths_i32(const uint32_t* blocked, int nx, int ny, int nz, const int32_t* paths, const int32_t* path_len, int n_goals,
                         int cap, int32_t* waypoints, int32_t* waypoint_len, void*) {
  pm::PathArgs a; bool empty;
  OCC4D_TRY(pm::check_paths(blocked, nx, ny, nz, paths, path_len, n_goals, cap, waypoints, waypoint_len, empty, a));
  if (empty) return OCC4D_OK;
  const sm::GlobalWords words{blocked};
  for (int g = 0; g < n_goals; ++g) {
    const int32_t* row = paths + (int64_t)g * cap;
    int32_t* out = waypoints + (int64_t)g * cap;
    const int L = pm::chain_length(a, g);
    int k = 0, count = 0;
    for (int anchor = 0; anchor < cap && L > 0; ++anchor) {
      out[count++] = row[k];
      if (k >= L - 1) break;
      int next = k + 1;                                           // the fallback: the original move, untested
      for (int j = L - 1; j > k + 1; --j)
        if (pm::candidate_free(a, words, row, L, k, j)) { next = j; break; }
      k = next;
    }
    for (int c = count; c < cap; ++c) out[c] = -1;
    waypoint_len[g] = L > 0 ? count : path_len[g];
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- viewplan
// include/ext/occ4d_viewplan.h: DEAD, RANGE and the pair test of csrc/viewplan_math.hpp, CANDIDATES, WORDS AND BITS IN ORDER; GREEDY
// over the same work array, rows and keys, each count a plain sum and the best key a plain maximum.
int occ4d_viewplan_visible_u32(const uint32_t* solid, int nx, int ny, int nz, const uint32_t* targets, const int32_t* candidates, int C,
                               int wx, int wy, int wz, int64_t max_dist2, uint32_t* vis, void*) {
  vm::VisArgs a; bool empty;
  OCC4D_TRY(vm::check_visible(solid, nx, ny, nz, targets, candidates, C, wx, wy, wz, max_dist2, vis, empty, a));
  if (empty) return OCC4D_OK;
  const sm::GlobalWords words{solid};
  for (int c = 0; c < C; ++c) {
    const vm::Candidate k = vm::candidate_at(a, words, c);
    for (int64_t w = 0; w < a.words; ++w) {
      uint32_t word = 0;
      for (int64_t p = w * 32; p < w * 32 + 32; ++p) {
        if (!vm::target_at(a, p)) continue;
        int px, py, pz;
        vm::point_of(a, (int32_t)p, px, py, pz);
        word |= (uint32_t)vm::sees(a, words, px, py, pz, k) << (p & 31);
      }
      vis[(int64_t)c * a.words + w] = word;
    }
  }
  return OCC4D_OK;
}
int occ4d_viewplan_greedy_u32(const uint32_t* vis, int C, int64_t W, const uint32_t* targets, int k, int32_t* work, int32_t* gain,
                              int32_t* picks, int32_t* pick_gain, int32_t* status, void*) {
  vm::GreedyArgs a; bool empty;
  OCC4D_TRY(vm::check_greedy(vis, C, W, targets, k, work, gain, picks, pick_gain, status, empty, a));
  if (empty) return OCC4D_OK;
  uint32_t* remaining = vm::remaining_of(a);
  int32_t *count = vm::count_of(a), *flag = vm::flag_of(a);
  for (int64_t w = 0; w < W; ++w) remaining[w] = targets[w];
  *flag = 1;
  for (int round = 0; round < std::max(k, 1); ++round) {
    if (*flag == 0) {                                             // behind a -1 pick
      picks[round] = -1, pick_gain[round] = 0;
      continue;
    }
    unsigned long long key = 0;
    for (int row = 0; row < C + (round == 0); ++row) {
      int32_t sum = 0;
      for (int64_t w = 0; w < W; ++w) sum += __builtin_popcount(vm::row_word(a, row, w) & remaining[w]);
      count[row] = sum;
      if (row < C) key = std::max(key, vm::key_of(sum, row));
      if (row < C && round == 0) gain[row] = sum;
    }
    if (round == 0) status[0] = status[1] = count[C];
    if (round >= k) break;                                        // k == 0: gain and status only
    if (!vm::key_picks(a, key)) {
      picks[round] = -1, pick_gain[round] = 0, *flag = 0;
      continue;
    }
    const int best = vm::key_pick(key);
    int32_t left = 0;
    for (int64_t w = 0; w < W; ++w) {
      remaining[w] &= ~vis[(int64_t)best * W + w];
      left += __builtin_popcount(remaining[w]);
    }
    status[1] = left, picks[round] = best, pick_gain[round] = vm::key_count(key);
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- boxes
// include/ext/occ4d_boxes.h: the DEAD test, the projections and the keys of csrc/boxes_math.hpp, POINTS IN ORDER, every atomic
// minimum / maximum / add a plain one; the choice OBJECT BY OBJECT, directions in order.
int occ4d_boxes_extents_i32(const int32_t* labels, int nx, int ny, int nz, int K, const int32_t* dirs, int A, int32_t* extent,
                            int32_t* zr, void*) {
  bm::ExtentArgs a; bool empty;
  OCC4D_TRY(bm::check_extents(labels, nx, ny, nz, K, dirs, A, extent, zr, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t i = 0; i < (int64_t)K * A * 4; ++i) extent[i] = bm::empty_extent((int)(i & 3));
  for (int64_t i = 0; i < (int64_t)K * 3; ++i) zr[i] = bm::empty_zr((int)(i % 3));
  std::vector<bm::Dir> d((size_t)A);
  for (int j = 0; j < A; ++j) d[(size_t)j] = bm::dir_at(dirs, j);
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; ++iz) {
        const int32_t k = labels[((int64_t)ix * ny + iy) * nz + iz];
        if (!bm::object_of(k, K)) continue;
        int32_t* z = zr + (int64_t)k * 3;
        z[0] = std::min(z[0], (int32_t)iz), z[1] = std::max(z[1], (int32_t)iz), z[2] += 1;
        for (int j = 0; j < A; ++j) {
          if (!d[(size_t)j].live) continue;
          int32_t* e = extent + ((int64_t)k * A + j) * 4;
          const int32_t u = bm::along(d[(size_t)j], ix, iy), v = bm::across(d[(size_t)j], ix, iy);
          e[0] = std::min(e[0], u), e[1] = std::max(e[1], u), e[2] = std::min(e[2], v), e[3] = std::max(e[3], v);
        }
      }
  return OCC4D_OK;
}
int occ4d_boxes_choose_i32(const int32_t* extent, const int32_t* zr, const int32_t* dirs, int K, int A, int32_t* box, void*) {
  bm::ChooseArgs c; bool empty;
  OCC4D_TRY(bm::check_choose(extent, zr, dirs, K, A, box, empty, c));
  if (empty) return OCC4D_OK;
  for (int k = 0; k < K; ++k) {
    bm::Key key{bm::NO_AREA, -1};
    for (int j = 0; j < A; ++j) key = bm::better(key, bm::key_of(c, k, j));
    bm::write_box(c, k, key);
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- layers
// include/ext/occ4d_layers.h: the march and the rows of csrc/layers_math.hpp, PIXELS IN ORDER, every atomic add / minimum / maximum
// of csrc/layers.hip a plain one.
int occ4d_layers_march_i32(const int32_t* labels, int nx, int ny, int nz, int K, float x0, float sx, float y0, float sy, float z0,
                           float sz, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth, float step,
                           int n_steps, int L, int32_t* label, int32_t* first, int32_t* samples, int32_t* point, int32_t* count,
                           int32_t* table, int32_t* status, void*) {
  lm::Args a; bool empty;
  OCC4D_TRY(lm::check_layers(labels, nx, ny, nz, K, x0, sx, y0, sy, z0, sz, k_inv, rt_inv, V, H, W, near_depth, step, n_steps, L, label,
                             first, samples, point, count, table, status, empty, a));
  if (empty) return OCC4D_OK;
  if (a.table)
    for (int64_t i = 0; i < (int64_t)V * K * lm::COLS; ++i) a.table[i] = lm::fill_value((int)(i % lm::COLS));
  if (a.status) a.status[0] = a.status[1] = 0;
  for (int v = 0; v < V; ++v)
    for (int py = 0; py < H; ++py)
      for (int px = 0; px < W; ++px) {
        lm::Layers s;
        lm::march(a, v, px, py, s);
        lm::write_pixel(a, ((int64_t)v * H + py) * W + px, s);
        if (a.status) a.status[0] += s.count == L + 1, a.status[1] += s.count >= 1;
        if (!a.table) continue;
        for (int j = 0; j < L; ++j) {
          if (s.label[j] < 0) continue;
          int32_t* row = a.table + ((int64_t)v * K + s.label[j]) * lm::COLS;              // (0 <= label < K: owner_of's test)
          row[OCC4D_LAYERS_AMODAL] += 1, row[OCC4D_LAYERS_VISIBLE] += j == 0;
          row[OCC4D_LAYERS_NEAR] = std::min(row[OCC4D_LAYERS_NEAR], s.first[j]);
          row[OCC4D_LAYERS_XMIN] = std::min(row[OCC4D_LAYERS_XMIN], (int32_t)px), row[OCC4D_LAYERS_XMAX] = std::max(row[OCC4D_LAYERS_XMAX], (int32_t)px);
          row[OCC4D_LAYERS_YMIN] = std::min(row[OCC4D_LAYERS_YMIN], (int32_t)py), row[OCC4D_LAYERS_YMAX] = std::max(row[OCC4D_LAYERS_YMAX], (int32_t)py);
        }
      }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- projection
// include/occ4d_project.h: the passes of csrc/project.hip over csrc/project_math.hpp, items in order; the atomic minimum of the
// splat is a plain minimum here.
int occ4d_project_points_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int flip_xy, float* uvz,
                             void*) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_project_points(rows, ld, n, rt, k, V, uvz, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t e = 0; e < a.items; ++e) pj::points_item(a, e, flip_xy != 0, uvz);
  return OCC4D_OK;
}
int occ4d_zbuffer_splat_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, int H, int W, int radius,
                            unsigned long long* keys, void*) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_zbuffer_splat(rows, ld, n, rt, k, V, H, W, radius, keys, empty, a));
  if (empty) return OCC4D_OK;
  const auto plain_min = [](unsigned long long* dst, unsigned long long key) { *dst = std::min(*dst, key); };
  for (int64_t e = 0; e < a.items; ++e) pj::splat_item(a, e, H, W, radius, keys, plain_min);
  return OCC4D_OK;
}
int occ4d_zbuffer_resolve_f32(const unsigned long long* keys, int V, int H, int W, const float* rows, int64_t ld, int n, int d,
                              float depth_background, float* depth, int32_t* index, const int32_t* cols_host, int C,
                              float feat_background, float* feat, void*) {
  pj::ResolveArgs r; bool empty;
  OCC4D_TRY(pj::check_zbuffer_resolve(keys, V, H, W, rows, ld, n, d, depth_background, depth, index, cols_host, C, feat_background,
                                      feat, empty, r));
  if (empty) return OCC4D_OK;
  for (int64_t p = 0; p < r.pixels; ++p) pj::resolve_item(r, p);
  return OCC4D_OK;
}
int occ4d_visibility_f32(const float* rows, int64_t ld, int n, const float* rt, const float* k, int V, const float* depth,
                         int64_t ld_depth, int H, int W, float margin, int32_t* code, void*) {
  pj::PointArgs a; bool empty;
  OCC4D_TRY(pj::check_visibility(rows, ld, n, rt, k, V, depth, ld_depth, H, W, code, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t e = 0; e < a.items; ++e) pj::visibility_item(a, e, depth, ld_depth, H, W, margin, code);
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- instance statistics
// include/occ4d_inst.h: the passes of csrc/inststats.hip over csrc/inst_math.hpp, rows and ids in order.
int64_t occ4d_inst_frame_len(int n_ids) { return in::frame_len(n_ids); }
int64_t occ4d_inst_counts_len(int n_groups) { return in::counts_len(n_groups); }
int64_t occ4d_inst_sums_len(int n_groups) { return in::sums_len(n_groups); }

int occ4d_inst_confusion_f32(const float* density, int64_t ld_density, const float* pred_id, int64_t ld_pred, int n, const int32_t* nn_idx,
                             const float* nn_dist, const float* target_id, int64_t ld_target, int m, int n_ids, float density_threshold,
                             float radius, int64_t* frame, void*) {
  in::ConfusionArgs a; bool empty;
  OCC4D_TRY(in::check_confusion(density, ld_density, pred_id, ld_pred, n, nn_idx, nn_dist, target_id, ld_target, m, n_ids,
                                density_threshold, radius, frame, empty, a));
  if (empty) return OCC4D_OK;
  for (int64_t i = 0; i < n; ++i) {
    const int cell = in::confusion_cell(a, i);
    if (cell == in::ROW_BAD) ++frame[OCC4D_INST_BAD_ROWS];
    else ++frame[in::frame_confusion(n_ids) + cell];
  }
  return OCC4D_OK;
}

int occ4d_inst_points_f32(const float* rows, int64_t ld, int n, const float* id, int64_t ld_id, int n_ids, int side, int64_t* frame,
                          void*) {
  in::PointArgs a; bool empty;
  OCC4D_TRY(in::check_points(rows, ld, n, id, ld_id, n_ids, side, frame, empty, a));
  if (empty) return OCC4D_OK;
  int64_t* table = frame + in::frame_points(n_ids, side);
  for (int64_t i = 0; i < n; ++i) {
    int64_t q[3];
    const int k = in::point_row(a, i, q);
    if (k == in::ROW_SKIP) continue;
    if (k == in::ROW_BAD) {
      ++frame[OCC4D_INST_BAD_ROWS];
      continue;
    }
    int64_t* e = table + (int64_t)k * OCC4D_INST_POINT_WORDS;
    ++e[OCC4D_INST_POINT_COUNT];
    for (int d = 0; d < 3; ++d) e[OCC4D_INST_POINT_SX + d] += q[d];
  }
  return OCC4D_OK;
}

int occ4d_inst_fold(const int64_t* frame, int n_ids, const int32_t* inst_group, int n_groups, int64_t* counts, double* sums, void*) {
  OCC4D_TRY(in::check_fold(frame, n_ids, n_groups, counts, sums));
  in::IdTerms terms[OCC4D_INST_MAX_IDS];
  int64_t bad = frame[OCC4D_INST_BAD_ROWS];
  for (int i = 0; i < n_ids; ++i) {
    terms[i] = in::fold_id(frame, n_ids, inst_group, n_groups, i);
    bad += terms[i].group == -2;
  }
  for (int g = 0; g < n_groups; ++g) {
    int64_t c[OCC4D_INST_GROUP_COUNTS];
    double s[OCC4D_INST_GROUP_SUMS];
    in::fold_group(terms, n_ids, g, c, s);
    for (int k = 0; k < OCC4D_INST_GROUP_COUNTS; ++k) counts[OCC4D_INST_HEAD + g * OCC4D_INST_GROUP_COUNTS + k] += c[k];
    for (int k = 0; k < OCC4D_INST_GROUP_SUMS; ++k) sums[g * OCC4D_INST_GROUP_SUMS + k] += s[k];
  }
  counts[OCC4D_INST_BAD_ROWS] += bad;
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- E3 / E2
int64_t occ4d_pt_layer_prepared_floats(const occ4d_pt_layer_weights* w, int) { return w ? 64 : -1; }
int occ4d_pt_layer_prepare_f32(const occ4d_pt_layer_weights* w, float* prepared, int, void*) {
  OCC4D_TRY(check_layer(w, "occ4d_pt_layer_prepare_f32"));
  OCC4D_REQUIRE(prepared, "occ4d_pt_layer_prepare_f32: null buffer");
  return OCC4D_OK;                       // (as written: nothing is derived from the weights)
}
int64_t occ4d_pt_layer_scene_floats(const occ4d_pt_layer_weights* w, int m) { return w ? up4((int64_t)2 * m * w->dim) : -1; }
int occ4d_pt_layer_scene_f32(const occ4d_pt_layer_weights* w, const float*, const float* x2, int64_t ldx2, int m, float* scene,
                             int, void*) {
  OCC4D_TRY(check_layer(w, "occ4d_pt_layer_scene_f32"));
  OCC4D_REQUIRE(x2 && scene && m >= 1 && w->cross, "occ4d_pt_layer_scene_f32: bad arguments");
  layer_tables(*w, x2, ldx2, m, scene, scene + (int64_t)m * w->dim);
  return OCC4D_OK;
}
int64_t occ4d_pt_layer_workspace_floats(const occ4d_pt_layer_weights* w, int, int, int, int) { return w ? 64 : -1; }

int occ4d_pt_layer_fwd_f32(const occ4d_pt_layer_weights* w, const float*, const float* x, int64_t ldx, const float* pos,
                           int64_t ps, int n, const float* x2, int64_t ldx2, const float* pos2, int64_t p2s, int m, int k,
                           const int32_t* knn_idx, const float* scene, float* out, int64_t ldo, float*, int,
                           occ4d_launch_events* ev, void*) {
  const char* who = "occ4d_pt_layer_fwd_f32";
  OCC4D_TRY(check_layer(w, who));
  OCC4D_REQUIRE(x && pos && out && n >= 0 && k >= 1 && k <= 16, "%s: bad arguments (k = %d)", who, k);
  OCC4D_REQUIRE(!w->cross || (pos2 && m >= k && (x2 || scene)), "%s: cross-attention needs x2 / pos2 with m >= k", who);
  if (ev) ev->used = 0;
  const int D = w->dim, d_in = w->pre_w ? w->d_in : D;
  if (n == 0) return OCC4D_OK;
  // layer1 (model/modules.py:61)
  std::vector<float> y((size_t)n * D);
#pragma omp parallel for schedule(static)
  for (int i = 0; i < n; ++i) {
    if (w->pre_w) matvec(w->pre_w, d_in, w->pre_b, x + (int64_t)i * ldx, D, d_in, y.data() + (size_t)i * D);
    else std::memcpy(y.data() + (size_t)i * D, x + (int64_t)i * ldx, sizeof(float) * D);
  }
  if (!w->cross) { pos2 = pos; p2s = ps; m = n; OCC4D_REQUIRE(m >= k, "%s: n = %d < k = %d", who, n, k); }
  // to_k / to_v of the key cloud (:171-172), to_q of the queries (:170)
  std::vector<float> tab;
  const float *kf, *vf;
  if (w->cross && scene) {
    kf = scene; vf = scene + (int64_t)m * D;
  } else {
    tab.resize((size_t)2 * m * D);
    layer_tables(*w, w->cross ? x2 : y.data(), w->cross ? ldx2 : D, m, tab.data(), tab.data() + (size_t)m * D);
    kf = tab.data(); vf = tab.data() + (size_t)m * D;
  }
  const float divisor = std::sqrt((float)D);
  const int d_out = w->post_w ? w->d_out : D;
#pragma omp parallel
  {
    AttnScratch s(k, D, w->pos_hidden);
    std::vector<float> q((size_t)D), agg((size_t)D);
    int32_t idx[16];
#pragma omp for schedule(dynamic, 8)
    for (int i = 0; i < n; ++i) {
      const float* pi = pos + (int64_t)i * ps;
      if (knn_idx) std::copy(knn_idx + (int64_t)i * k, knn_idx + (int64_t)i * k + k, idx);
      else knn_one(pi, pos2, p2s, m, k, 0, idx, nullptr);                  // kNN_torch(pos, pos2, k)          (:167)
      matvec(w->to_q, D, nullptr, y.data() + (size_t)i * D, D, D, q.data());
      attn_one(*w, q.data(), pi, pos2, p2s, kf, vf, idx, k, divisor, s, agg.data());
      float* o = out + (int64_t)i * ldo;
      if (w->post_w) {                                                       // z = x + layer3(agg)            (model/modules.py:64-66)
        for (int c = 0; c < d_out; ++c) o[c] = x[(int64_t)i * ldx + c] + dot(w->post_w + (int64_t)c * D, agg.data(), D) + w->post_b[c];
      } else {
        std::memcpy(o, agg.data(), sizeof(float) * D);
      }
    }
  }
  return OCC4D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- E6
int occ4d_down_pool_fwd_f32(const float* x, int64_t ldx, int n, int d_in, const float* w, const float* b, int d_out, int norm,
                            const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                            const int32_t* nn_idx, int n_new, int k, float* z, int64_t ldz, float* workspace, void* st) {
  const char* who = "occ4d_down_pool_fwd_f32";
  OCC4D_REQUIRE(x && w && b && nn_idx && z && workspace && n >= 1 && n_new >= 1 && k >= 1, "%s: bad arguments", who);
  OCC4D_REQUIRE(norm >= 0 && norm <= 2, "%s: Unknown norm type: %d", who, norm);
  OCC4D_REQUIRE(norm == 0 || (gamma && beta), "%s: norm needs gamma / beta", who);
  OCC4D_REQUIRE(norm != 2 || (mean && var), "%s: batch norm needs running statistics", who);
  float* y = workspace;                                                      // (n, d_out): the MLP on ALL points   (model/modules.py:152)
#pragma omp parallel for schedule(static)
  for (int i = 0; i < n; ++i) matvec(w, d_in, b, x + (int64_t)i * ldx, d_out, d_in, y + (int64_t)i * d_out);
  if (norm == 1) {
    OCC4D_TRY(occ4d_layernorm_f32(y, d_out, gamma, beta, eps, 1, y, d_out, n, d_out, st));
  } else {
    for (int64_t i = 0; i < (int64_t)n; ++i)
      for (int c = 0; c < d_out; ++c) {
        float v = y[i * d_out + c];
        if (norm == 2) v = (v - mean[c]) / std::sqrt(var[c] + eps) * gamma[c] + beta[c];
        y[i * d_out + c] = v > 0.f ? v : 0.f;
      }
  }
  return occ4d_maxpool_gather_f32(y, d_out, nn_idx, n_new, k, d_out, z, ldz, st);   // max over the k neighbours   (:156-158)
}

// ---------------------------------------------------------------------------------------------------------------- D1-D7
static int check_decoder(const occ4d_decoder_weights* w, const char* who) {
  OCC4D_REQUIRE(w, "%s: null weights", who);
  OCC4D_REQUIRE(w->n_blocks >= 1 && w->n_blocks <= OCC4D_MAX_BLOCKS && w->n_cross >= 0 && w->n_cross <= OCC4D_MAX_CROSS,
      "%s: n_blocks = %d, n_cross = %d", who, w->n_blocks, w->n_cross);
  OCC4D_REQUIRE(w->activation == 0 || w->activation == 1, "%s: Unknown activation: %d", who, w->activation);
  OCC4D_REQUIRE(w->k_local >= 1 && w->k_local <= 16 && (w->n_cross == 0 || (w->k_cross >= 1 && w->k_cross <= 16)),
      "%s: k_local = %d, k_cross = %d (1 .. 16)", who, w->k_local, w->k_cross);
  OCC4D_REQUIRE(w->lin_in_w && w->lin_in_b && w->lin_out_w && w->lin_out_b, "%s: lin_in / lin_out missing", who);
  for (int j = 0; j < w->n_cross; ++j) OCC4D_TRY(check_layer(&w->cross[j], who));
  return OCC4D_OK;
}
int64_t occ4d_decoder_prepared_floats(const occ4d_decoder_weights* w, int) { return w ? 64 : -1; }
int occ4d_decoder_prepare_f32(const occ4d_decoder_weights* w, float* prepared, int, void*) {
  OCC4D_TRY(check_decoder(w, "occ4d_decoder_prepare_f32"));
  OCC4D_REQUIRE(prepared, "occ4d_decoder_prepare_f32: null buffer");
  return OCC4D_OK;
}
int64_t occ4d_decoder_scene_floats(const occ4d_decoder_weights* w, int m) { return w && m >= 1 ? dec_scene(*w, m).total : -1; }
int occ4d_decoder_prepare_scene_f32(const occ4d_decoder_weights* w, const float*, const float* xyz, int64_t xyz_stride,
                                    const float* feats, int64_t ld_feats, const float* fglobal, int m, float* scene, int, void* st) {
  const char* who = "occ4d_decoder_prepare_scene_f32";
  OCC4D_TRY(check_decoder(w, who));
  const int dg = w->d_latent - w->d_latent_local;                            // 0: a decoder without a global part takes no fglobal
  OCC4D_REQUIRE(xyz && feats && scene && m >= 1 && dg >= 0 && (dg == 0 || fglobal), "%s: bad arguments", who);
  const DecScene S = dec_scene(*w, m);
  OCC4D_TRY(occ4d_copy_rows_f32(scene + S.xyz, 3, xyz, xyz_stride, m, 3, st));
  OCC4D_TRY(occ4d_copy_rows_f32(scene + S.feats, w->d_latent_local, feats, ld_feats, m, w->d_latent_local, st));
  if (dg > 0) std::memcpy(scene + S.fglobal, fglobal, sizeof(float) * dg);
  for (int j = 0; j < w->n_cross; ++j)      // to_k / to_v rows of the abstract cloud: once per scene instead of once per call (D7)
    layer_tables(w->cross[j], scene + S.feats, w->d_latent_local, m, scene + S.layer[j], scene + S.layer[j] + (int64_t)m * w->cross[j].dim);
  return OCC4D_OK;
}
int64_t occ4d_decoder_query_workspace_floats(const occ4d_decoder_weights* w, int, int, int) { return w ? 64 : -1; }

// The prelude's rows of the queries of a forward call (occ4d_decoder_query_fwd_prelude_f32), or none
struct QueryPrelude {
  const int32_t* idx_local;
  const float* w_local;
  const int32_t* idx_cross;
  const float* x0;
  int64_t ld_x0;
};

// D2 + D3 of one query: the k_local nearest abstract points by Euclidean norm (or the caller's list, clamped) and their
// normalised inverse-distance weights, in occ4d_interp_weights_f32's expressions
static void local_list_one(const float* qi, const float* xyz, int m, int kl, const int32_t* given, int32_t* i8, float* w8) {
  float d8[16];
  if (given) {
    for (int j = 0; j < kl; ++j) {
      i8[j] = std::min(std::max(given[j], 0), m - 1);
      d8[j] = dist_metric(qi, xyz + 3 * (int64_t)i8[j], 1);
    }
  } else {
    knn_one(qi, xyz, 3, m, kl, 1, i8, d8);
  }
  float ws = 0.f;
  for (int j = 0; j < kl; ++j) { w8[j] = 1.f / (d8[j] + 1e-4f); ws += std::fabs(w8[j]); }
  ws = std::max(ws, 1e-12f);
  for (int j = 0; j < kl; ++j) w8[j] /= ws;
}
// D5 + lin_in of one query (:405-408); pe: d_in (2 n_freq + 1) floats of scratch
static void embed_one(const occ4d_decoder_weights* w, const float* qi, int64_t qs, float* pe, float* x) {
  const int P = w->d_in * (2 * w->n_freq + 1);
  if (w->n_freq > 0) occ4d_posenc_f32(qi, qs, 1, w->d_in, w->n_freq, (double)w->base_frequency, pe, P, nullptr);
  else std::copy(qi, qi + w->d_in, pe);
  matvec(w->lin_in_w, w->lin_in_ld, w->lin_in_b, pe, w->d_hidden, P, x);
}

static int decoder_rows(const occ4d_decoder_weights* w, const float* scene, int m, const float* queries, int64_t qs, int n,
                        const int32_t* knn_local, const int32_t* knn_cross, const QueryPrelude* pre, float* out, int64_t ld_out,
                        float* penult, int64_t ld_pen) {
  const DecScene S = dec_scene(*w, m);
  const float *xyz = scene + S.xyz, *feats = scene + S.feats, *fglobal = scene + S.fglobal;
  const int H = w->d_hidden, E = w->d_latent_local, dg = w->d_latent - E, DL = w->d_latent;
  const int P = w->d_in * (2 * w->n_freq + 1), A = w->activation == 1 ? 2 : 1;
  const int kl = w->k_local, kc = w->k_cross;
#pragma omp parallel
  {
    std::vector<float> fq((size_t)DL), pe((size_t)std::max(P, 1)), x((size_t)H), h((size_t)H), t((size_t)H), y, agg, q;
    std::vector<AttnScratch> scr;
    for (int j = 0; j < w->n_cross; ++j) scr.emplace_back(kc, w->cross[j].dim, w->cross[j].pos_hidden);
    int maxd = 1;
    for (int j = 0; j < w->n_cross; ++j) maxd = std::max(maxd, (int)w->cross[j].dim);
    y.resize(maxd); agg.resize(maxd); q.resize(maxd);
#pragma omp for schedule(dynamic, 16)
    for (int i = 0; i < n; ++i) {
      const float* qi = queries + (int64_t)i * qs;
      // D2 + D3: 8 nearest abstract points by Euclidean norm, inverse-distance interpolation (model/implicit.py:328-342)
      int32_t i8[16], ia[16];
      float w8[16];
      if (pre) {
        std::copy(pre->idx_local + (int64_t)i * kl, pre->idx_local + (int64_t)(i + 1) * kl, i8);
        std::copy(pre->w_local + (int64_t)i * kl, pre->w_local + (int64_t)(i + 1) * kl, w8);
      } else {
        local_list_one(qi, xyz, m, kl, knn_local ? knn_local + (int64_t)i * kl : nullptr, i8, w8);
      }
      for (int c = 0; c < dg; ++c) fq[c] = fglobal[c];                     // [global | local]                (:342)
      for (int c = 0; c < E; ++c) {
        float s = 0.f;
        for (int j = 0; j < kl; ++j) s += w8[j] * feats[(int64_t)i8[j] * E + c];
        fq[dg + c] = s;
      }
      // one kNN_torch serves every cross layer (same coordinates, same K)   (model/point_transformer_layer.py:167)
      if (w->n_cross) {
        if (pre) std::copy(pre->idx_cross + (int64_t)i * kc, pre->idx_cross + (int64_t)(i + 1) * kc, ia);
        else if (knn_cross) for (int j = 0; j < kc; ++j) ia[j] = std::min(std::max(knn_cross[(int64_t)i * kc + j], 0), m - 1);
        else knn_one(qi, xyz, 3, m, kc, 0, ia, nullptr);
      }
      // D5 + lin_in (:405-408)
      if (pre && pre->x0) std::copy(pre->x0 + (int64_t)i * pre->ld_x0, pre->x0 + (int64_t)i * pre->ld_x0 + H, x.begin());
      else embed_one(w, qi, qs, pe.data(), x.data());
      int next_cross = 0;
      for (int bl = 0; bl < w->n_blocks; ++bl) {
        matvec(w->lin_z_w[bl], DL, w->lin_z_b[bl], fq.data(), H, DL, t.data());                    // x += lin_z[i](features_query)   (:416-417)
        for (int c = 0; c < H; ++c) x[c] += t[c];
        for (int c = 0; c < H; ++c) t[c] = act(x[c], A);                                            // ResnetBlockFC                   (:92-101)
        matvec(w->fc0_w[bl], H, w->fc0_b[bl], t.data(), H, H, h.data());
        for (int c = 0; c < H; ++c) h[c] = act(h[c], A);
        matvec(w->fc1_w[bl], H, w->fc1_b[bl], h.data(), H, H, t.data());
        for (int c = 0; c < H; ++c) x[c] += t[c];
        if (next_cross < w->n_cross && w->cross_after[next_cross] == bl) {                          // PointTransformerBlock           (:421-439)
          const int j = next_cross++;
          const occ4d_pt_layer_weights& cw = w->cross[j];
          const int D = cw.dim;
          matvec(cw.pre_w, H, cw.pre_b, x.data(), D, H, y.data());
          matvec(cw.to_q, D, nullptr, y.data(), D, D, q.data());
          const float* kf = scene + S.layer[j];
          attn_one(cw, q.data(), qi, xyz, 3, kf, kf + (int64_t)m * D, ia, kc, std::sqrt((float)D), scr[j], agg.data());
          matvec(cw.post_w, D, cw.post_b, agg.data(), H, D, t.data());
          for (int c = 0; c < H; ++c) x[c] += t[c];
        }
      }
      if (penult) std::copy(x.begin(), x.end(), penult + (int64_t)i * ld_pen);
      for (int c = 0; c < H; ++c) t[c] = act(x[c], A);
      matvec(w->lin_out_w, H, w->lin_out_b, t.data(), w->d_out, H, out + (int64_t)i * ld_out);     // lin_out(act(x))                 (:441-443)
    }
  }
  return OCC4D_OK;
}

int occ4d_decoder_query_fwd_f32(const occ4d_decoder_weights* w, const float*, const float* scene, int m, const float* queries,
                                int64_t qs, int n, const int32_t* knn_local, const int32_t* knn_cross, float* out, int64_t ld_out,
                                float* penult, int64_t ld_pen, float*, int, occ4d_launch_events* ev, void*) {
  const char* who = "occ4d_decoder_query_fwd_f32";
  OCC4D_TRY(check_decoder(w, who));
  OCC4D_REQUIRE(scene && queries && out && n >= 0 && m >= w->k_local && (w->n_cross == 0 || m >= w->k_cross), "%s: bad arguments", who);
  if (ev) ev->used = 0;
  return decoder_rows(w, scene, m, queries, qs, n, knn_local, knn_cross, nullptr, out, ld_out, penult, ld_pen);
}

// ---- the query prelude (csrc/path.hip; argument contracts shared through csrc/decoder_math.hpp)
int64_t occ4d_decoder_query_prelude_workspace_floats(const occ4d_decoder_weights* w, int n, int) { return w && n >= 0 ? 64 : -1; }
int occ4d_decoder_query_prelude_f32(const occ4d_decoder_weights* w, const float* xyz, int m, const float* queries, int64_t qs, int n,
                                    int32_t* idx_local, float* w_local, int32_t* idx_cross, float* x0, int64_t ld_x0,
                                    float* workspace, void*) {
  OCC4D_TRY(check_decoder(w, "occ4d_decoder_query_prelude_f32"));
  bool empty = false;
  OCC4D_TRY(occ4d_decoder::check_query_prelude(w, xyz, m, queries, qs, n, idx_local, w_local, idx_cross, x0, ld_x0, workspace, &empty));
  if (empty) return OCC4D_OK;
  const int kl = w->k_local, kc = w->k_cross;
#pragma omp parallel
  {
    std::vector<float> pe((size_t)std::max(w->d_in * (2 * w->n_freq + 1), 1));
#pragma omp for schedule(dynamic, 64)
    for (int i = 0; i < n; ++i) {
      const float* qi = queries + (int64_t)i * qs;
      local_list_one(qi, xyz, m, kl, nullptr, idx_local + (int64_t)i * kl, w_local + (int64_t)i * kl);
      if (w->n_cross) knn_one(qi, xyz, 3, m, kc, 0, idx_cross + (int64_t)i * kc, nullptr);
      if (x0) embed_one(w, qi, qs, pe.data(), x0 + (int64_t)i * ld_x0);
    }
  }
  return OCC4D_OK;
}
int occ4d_decoder_query_fwd_prelude_f32(const occ4d_decoder_weights* w, const float* prepared, const float* scene, int m,
                                        const float* queries, int64_t qs, int n, const int32_t* idx_local, const float* w_local,
                                        const int32_t* idx_cross, float* x0, int64_t ld_x0, float* out, int64_t ld_out,
                                        float* penult, int64_t ld_pen, float* workspace, int, occ4d_launch_events* ev, void*) {
  OCC4D_TRY(check_decoder(w, "occ4d_decoder_query_fwd_prelude_f32"));
  if (ev) ev->used = 0;
  bool empty = false;
  OCC4D_TRY(occ4d_decoder::check_query_fwd_prelude(w, prepared, scene, m, queries, qs, n, idx_local, w_local, idx_cross, x0, ld_x0,
                                                   out, ld_out, penult, ld_pen, workspace, &empty));
  if (empty) return OCC4D_OK;
  const QueryPrelude pre{idx_local, w_local, idx_cross, x0, ld_x0};
  return decoder_rows(w, scene, m, queries, qs, n, nullptr, nullptr, &pre, out, ld_out, penult, ld_pen);
}

}  // extern "C"
