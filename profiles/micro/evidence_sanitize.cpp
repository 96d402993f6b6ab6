// A stand-alone host program over the host bodies of csrc/evidence_math.hpp (include/ext/occ4d_evidence.h) -- the snap, the walk,
// the body of a return, the code of a cell and the two argument contracts -- with buffers of EXACTLY the documented sizes, for a run
// under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude -Iocclusions-4d_amd/csrc profiles/micro/evidence_sanitize.cpp -o /tmp/evidence_sanitize && /tmp/evidence_sanitize
//
// Grids 1 x 1 x 1, 5 x 4 x 3, 33 x 2 x 7, 70 x 3 x 5, 40 x 40 x 40 and one without cells; R in 0 / 1 / 63 / 64 / 65 / 1000; V in 1 / 3 /
// 40; sensors inside, outside and at the eight corners (+-2^20, +-2^20, +-2^20), also one step beyond them (dropped); returns in the
// grid, outside it, NaN, infinite, at +-FLT_MAX and 2^20 cells away on either side of the limit; sensor indices below 0 and at V; a
// null sensor table; a row stride; with and without counts.  It checks what can be checked without a second implementation: the
// statuses and texts of the rejected calls; status sums to R and its slots match the kinds that were planted; hits sums to the
// carved returns; passes > 0 equals the bits; a walk passes at most nx + ny + nz cells and never its own start; the unused bits of the
// last word stay 0; the codes lie in [0, 6) and totals is their histogram.  Prints "ok", the calls and the marks.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "evidence_math.hpp"

static char g_err[512] = "";
void occ4d::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

namespace ev = occ4d_evidence;

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (uint32_t)(state >> 32);
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 100000) / 100000.0f; }

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_err);    \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

struct PlainMarks {
  uint32_t* words;
  int32_t *hits, *passes;
  long long* marks;
  void hit(int32_t flat) const { hits[flat] += 1; }
  void pass(int32_t flat) const {
    words[flat >> 5] |= 1u << (flat & 31);
    if (passes) passes[flat] += 1;
    ++*marks;
  }
  void arrive(int32_t flat) const { pass(flat); }
};

static int calls = 0;
static long long marks = 0, dropped[4] = {0, 0, 0, 0};
static const int FAR = OCC4D_EVIDENCE_MAX_COORD;

static void run(int nx, int ny, int nz, int64_t R, int V, int pad, bool counts, bool null_sensor) {
  const int64_t n = (int64_t)nx * ny * nz, ld = 3 + pad;
  const float mn[3] = {uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f), uniform(-2.0f, 2.0f)};
  const float sp[3] = {uniform(0.1f, 0.8f), uniform(0.1f, 0.8f), uniform(0.1f, 0.8f)};
  const int dims[3] = {nx, ny, nz};
  std::vector<int32_t> origins((size_t)V * 3);
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k) {
      const int kind = (v + calls) % 5;
      origins[(size_t)v * 3 + k] = kind == 0 ? (int)(rnd() % (unsigned)(dims[k] > 0 ? dims[k] : 1))
                                   : kind == 1 ? (int)(rnd() % 200) - 100
                                   : kind == 2 ? ((rnd() & 1) ? FAR : -FAR)
                                   : kind == 3 ? ((rnd() & 1) ? FAR + 1 : -FAR - 1)                 // dropped for the sensor
                                               : ((rnd() & 1) ? INT32_MAX : INT32_MIN);
    }
  std::vector<float> returns((size_t)(R > 0 ? (R - 1) * ld + 3 : 0));                                // exactly the last float read
  std::vector<int32_t> sensor((size_t)R);
  long long planted[4] = {0, 0, 0, 0};
  const float strange[] = {NAN, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX};
  for (int64_t r = 0; r < R; ++r) {
    float* p = returns.data() + r * ld;
    for (int k = 0; k < 3; ++k) p[k] = mn[k] + uniform(-0.1f, 1.1f) * sp[k] * (float)dims[k];
    sensor[(size_t)r] = (int32_t)(rnd() % (unsigned)V);
    const unsigned what = rnd() % 16;
    if (what == 0) p[rnd() % 3] = strange[rnd() % 5];
    if (what == 1) p[rnd() % 3] = mn[0] + sp[0] * ((float)FAR + ((rnd() & 1) ? 8.0f : -8.0f)) * ((rnd() & 1) ? 1.0f : -1.0f);
    if (what == 2) sensor[(size_t)r] = (rnd() & 1) ? V : -1 - (int32_t)(rnd() % 5);
    if (what == 3) sensor[(size_t)r] = (rnd() & 1) ? INT32_MAX : INT32_MIN;
  }
  const int64_t words = (n + 31) / 32;
  std::vector<uint32_t> passed((size_t)words, 0u);
  std::vector<int32_t> hits((size_t)n, 0), passes(counts ? (size_t)n : 0, 0);
  int32_t status[4] = {0, 0, 0, 0};
  ev::CarveArgs a;
  CHECK(ev::check_carve(returns.data(), ld, R, null_sensor ? nullptr : sensor.data(), origins.data(), V, nx, ny, nz, mn[0], sp[0], mn[1], sp[1],
                        mn[2], sp[2], n ? passed.data() : nullptr, n ? hits.data() : nullptr, counts ? passes.data() : nullptr, status, a) == OCC4D_OK);
  long long before = marks;
  const PlainMarks m{passed.data(), hits.data(), counts ? passes.data() : nullptr, &marks};
  for (int64_t r = 0; r < R; ++r) {
    const long long at = marks;
    const int slot = ev::return_item(a, r, m);
    CHECK(slot >= 0 && slot < 4);
    CHECK(slot == ev::CARVED || marks == at);                        // a dropped return marks nothing
    CHECK(marks - at <= nx + ny + nz);
    status[slot] += 1;
    planted[slot] += 1;
  }
  long long sum_hits = 0, sum_passes = 0;
  for (int64_t p = 0; p < n; ++p) {
    sum_hits += hits[(size_t)p];
    const bool bit = (passed[(size_t)(p >> 5)] >> (p & 31)) & 1u;
    if (counts) {
      CHECK((passes[(size_t)p] > 0) == bit);
      sum_passes += passes[(size_t)p];
    }
  }
  CHECK(status[0] + status[1] + status[2] + status[3] == R && sum_hits == status[0]);
  CHECK(!counts || sum_passes == marks - before);
  CHECK(n % 32 == 0 || words == 0 || (passed[(size_t)words - 1] >> (n % 32)) == 0u);
  CHECK(n > 0 || status[0] == 0);
  for (int k = 0; k < 4; ++k) dropped[k] += planted[k];
  // classify: a strided field, the bits and the counts
  const int64_t ldf = 1 + pad;
  std::vector<float> field((size_t)(n > 0 ? (n - 1) * ldf + 1 : 0));
  for (int64_t p = 0; p < n; ++p) field[(size_t)(p * ldf)] = (rnd() % 7 == 0) ? NAN : uniform(0.0f, 1.0f);
  std::vector<int32_t> code((size_t)n, -1);
  for (int variant = 0; variant < (counts && n > 0 ? 3 : 1); ++variant) {  // (an empty vector's data() is null)
    int64_t totals[6] = {0, 0, 0, 0, 0, 0};
    ev::ClassifyArgs c;
    CHECK(ev::check_classify(field.data(), ldf, 0.5f, nullptr, 0, 0.0f, n, variant ? nullptr : passed.data(), variant ? passes.data() : nullptr,
                             variant == 2 ? 2 : 1, hits.data(), code.data(), totals, c) == OCC4D_OK);
    for (int64_t p = 0; p < n; ++p) {
      const int k = ev::code_of(c, p);
      CHECK(k >= 0 && k < 6 && (k % 3 == 2) == (hits[(size_t)p] > 0));
      totals[code[(size_t)p] = k] += 1;
    }
    CHECK(totals[0] + totals[1] + totals[2] + totals[3] + totals[4] + totals[5] == n);
  }
  ++calls;
}

static void rejected() {
  ev::CarveArgs a;
  ev::ClassifyArgs c;
  float f[3] = {0, 0, 0};
  int32_t i4[4], org[3] = {0, 0, 0};
  uint32_t w[1];
  int64_t t[6];
#define BAD_CARVE(...) CHECK(ev::check_carve(__VA_ARGS__, a) == OCC4D_EINVAL && std::strstr(g_err, "occ4d_evidence_carve_f32"))
  BAD_CARVE(f, 3, -1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, (int64_t)INT32_MAX + 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 2, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 4097, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, -1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 513, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, NAN, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, INFINITY, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, NAN, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, nullptr);
  BAD_CARVE(f, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, nullptr, i4, nullptr, i4);
  BAD_CARVE(nullptr, 3, 1, nullptr, org, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
  BAD_CARVE(f, 3, 1, nullptr, nullptr, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, w, i4, nullptr, i4);
#define BAD_CLASSIFY(...) CHECK(ev::check_classify(__VA_ARGS__, c) == OCC4D_EINVAL && std::strstr(g_err, "occ4d_evidence_classify_f32"))
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, -1, w, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, (int64_t)INT32_MAX + 1, w, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 0, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, f, 0, 0.0f, 1, w, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 0, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 2, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 1, i4, i4, nullptr);
  BAD_CLASSIFY(nullptr, 1, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, 1, nullptr, nullptr, 1, i4, i4, t);
  BAD_CLASSIFY(f, 1, 0.5f, nullptr, 0, 0.0f, 1, w, nullptr, 1, nullptr, i4, t);
}

// the snap at its limits and a walk between two of the 2^20 corners' neighbours: terms below 2^43, no overflow
static void corners() {
  int cell = 0;
  CHECK(ev::snap(1048576.0f, 0.0f, 1.0f, cell) && cell == FAR);
  CHECK(ev::snap(-1048576.0f, 0.0f, 1.0f, cell) && cell == -FAR);
  CHECK(!ev::snap(1048577.0f, 0.0f, 1.0f, cell) && !ev::snap(-1048576.5f, 0.0f, 1.0f, cell));
  CHECK(!ev::snap(NAN, 0.0f, 1.0f, cell) && !ev::snap(INFINITY, 0.0f, 1.0f, cell) && !ev::snap(FLT_MAX, -FLT_MAX, FLT_MIN, cell));
  CHECK(ev::snap(-0.0f, 0.0f, 1.0f, cell) && cell == 0 && ev::snap(-1e-30f, 0.0f, 1.0f, cell) && cell == -1);
  CHECK(ev::coord_ok(FAR) && ev::coord_ok(-FAR) && !ev::coord_ok(FAR + 1) && !ev::coord_ok(INT32_MIN) && !ev::coord_ok(INT32_MAX));
  const int n[3] = {512, 512, 512};
  std::vector<uint32_t> words(512 * 512 * 16, 0u);
  for (int sx = -1; sx <= 1; sx += 2)
    for (int sy = -1; sy <= 1; sy += 2)
      for (int sz = -1; sz <= 1; sz += 2)
        for (int e = 0; e < 512; e += 511) {
          const long long at = marks;
          const PlainMarks m{words.data(), nullptr, nullptr, &marks};          // (the walk never hits)
          ev::walk(n, m, e, 511 - e, e, sx * FAR, sy * FAR, sz * (FAR - 7));
          CHECK(marks - at <= 3 * 512);
        }
}

int main() {
  const int grids[][3] = {{1, 1, 1}, {5, 4, 3}, {33, 2, 7}, {70, 3, 5}, {40, 40, 40}, {4, 0, 9}};
  const int64_t counts[] = {0, 1, 63, 64, 65, 1000};
  const int sensors[] = {1, 3, 40};
  for (const auto& g : grids)
    for (int64_t R : counts)
      for (int V : sensors)
        for (int variant = 0; variant < 2; ++variant) run(g[0], g[1], g[2], R, V, variant ? 2 : 0, variant == 1, V == 1 && variant == 0);
  rejected();
  corners();
  CHECK(marks > 0 && dropped[0] > 0 && dropped[1] > 0 && dropped[2] > 0 && dropped[3] > 0);
  std::printf("ok: %d calls, %lld marks, returns carved / dropped %lld / %lld / %lld / %lld\n", calls, marks, dropped[0], dropped[1], dropped[2],
              dropped[3]);
  return 0;
}
