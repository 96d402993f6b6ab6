// The occupancy surface of the query grid as a quad mesh (include/occ4d_surface.h: naive surface nets).  The per-element rules
// and the argument contracts are csrc/surface_math.hpp, shared with the g++ twin; the tile ranks, the prefix and the launches are
// here.  Launch- and latency-bound: 2 MB of density and a few thousand crossed cells beside a decode of 29 MFLOP per query, so
// four launches and nothing else: count, prefix, vertex pass, face pass.
//
// One thread per grid point, 256-thread workgroups (four wave64), one workgroup per tile of 256 points.  A thread owns the cell at
// its low corner and the three edges that leave it in +x, +y, +z.  A cell's rank in its tile is a 64-bit ballot and a popcount
// plus an LDS prefix over the four waves (the construction of split_write_kernel in csrc/postops.hip); a thread emits 0 .. 3
// quads, and the scan of that count over the wave is two ballots, one per bit of the count.  The tile prefix is the
// single-workgroup scan of occ4d_compact_count_f32, once per array, any number of tiles.  No atomics: every element of work,
// vertices and faces has one owner, so the result depends on neither the stream nor the run.
#include "common.hpp"
#include "surface_math.hpp"
#include "occ4d_surface.h"

namespace {

namespace sf = occ4d_surface;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 1024;
static_assert(THREADS == sf::TILE, "one thread per point of a tile");

// what a point owns, and nothing for the threads behind the grid's end
__device__ __forceinline__ sf::Item item_at(const sf::Field& f, int64_t i, float v[8]) {
  return i < f.grid.points ? sf::item_of(f, i, v) : sf::Item{0u, 0u};
}

// (crossed cells, quads) of the threads of this tile in front of the caller; s_*: WAVES ints each.  `tile_*`: the tile's sums.
__device__ __forceinline__ void tile_ranks(const sf::Item& it, int* s_cells, int* s_quads, int& cells_before, int& quads_before,
                                           int& tile_cells, int& tile_quads) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int quads = sf::quads_of(it.axes);
  const unsigned long long m = __ballot(sf::crossed(it.mask));
  const unsigned long long q0 = __ballot(quads & 1), q1 = __ballot(quads & 2);
  if (lane == 0) {
    s_cells[wave] = __popcll(m);
    s_quads[wave] = __popcll(q0) + 2 * __popcll(q1);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  cells_before = __popcll(m & below);
  quads_before = __popcll(q0 & below) + 2 * __popcll(q1 & below);
  tile_cells = 0;
  tile_quads = 0;
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) {
      cells_before += s_cells[w];
      quads_before += s_quads[w];
    }
    tile_cells += s_cells[w];
    tile_quads += s_quads[w];
  }
}

// pass 1: per tile, the number of crossed cells and of quads
__global__ __launch_bounds__(THREADS) void surface_count_kernel(const sf::CountArgs a) {
  __shared__ int s_cells[WAVES], s_quads[WAVES];
  float v[8];
  const sf::Item it = item_at(a.f, (int64_t)blockIdx.x * THREADS + threadIdx.x, v);
  int cells_before, quads_before, tile_cells, tile_quads;
  tile_ranks(it, s_cells, s_quads, cells_before, quads_before, tile_cells, tile_quads);
  if (threadIdx.x == 0) {
    a.cell_offsets[blockIdx.x] = tile_cells;
    a.face_offsets[blockIdx.x] = tile_quads;
  }
}

// pass 2: the exclusive prefix of the tile counts and their total: workgroup 0 the cells, workgroup 1 the faces
// (split_scan_kernel of csrc/postops.hip: chunks of 1024 tiles with a carry)
__global__ __launch_bounds__(SCAN_THREADS) void surface_scan_kernel(const sf::CountArgs a) {
  __shared__ int s[SCAN_THREADS];
  int32_t* counts = blockIdx.x == 0 ? a.cell_offsets : a.face_offsets;
  int carry = 0;
  for (int64_t base = 0; base < a.tiles; base += SCAN_THREADS) {          // (uniform over the workgroup: barriers inside)
    const int64_t i = base + threadIdx.x;
    const int v = i < a.tiles ? counts[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < a.tiles) counts[i] = carry + s[threadIdx.x] - v;
    const int chunk_total = s[SCAN_THREADS - 1];
    __syncthreads();
    carry += chunk_total;
  }
  if (threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}

// pass 3: every point's vertex number into work, every crossed cell's vertex row
__global__ __launch_bounds__(THREADS) void surface_vertex_kernel(const sf::WriteArgs w) {
  __shared__ int s_cells[WAVES], s_quads[WAVES];
  float v[8];
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const sf::Item it = item_at(w.f, i, v);
  int cells_before, quads_before, tile_cells, tile_quads;
  tile_ranks(it, s_cells, s_quads, cells_before, quads_before, tile_cells, tile_quads);
  if (i < w.f.grid.points) sf::vertex_item(w, i, it, v, (int64_t)w.cell_offsets[blockIdx.x] + cells_before);
}

// pass 4: every point's quads, from the vertex numbers of the four cells around each of its edges
__global__ __launch_bounds__(THREADS) void surface_face_kernel(const sf::WriteArgs w) {
  __shared__ int s_cells[WAVES], s_quads[WAVES];
  float v[8];
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const sf::Item it = item_at(w.f, i, v);
  int cells_before, quads_before, tile_cells, tile_quads;
  tile_ranks(it, s_cells, s_quads, cells_before, quads_before, tile_cells, tile_quads);
  if (it.axes != 0u) sf::face_item(w, i, it, (int64_t)w.face_offsets[blockIdx.x] + quads_before);
}

}  // namespace

extern "C" int occ4d_surface_count_f32(const float* density, int64_t ld, int nx, int ny, int nz, float level, int32_t* cell_offsets,
                                       int32_t* face_offsets, int32_t* totals, void* stream) {
  sf::CountArgs a; bool empty;
  OCC4D_TRY(sf::check_count(density, ld, nx, ny, nz, level, cell_offsets, face_offsets, totals, empty, a));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  surface_count_kernel<<<(unsigned)a.tiles, THREADS, 0, st>>>(a);
  surface_scan_kernel<<<2, SCAN_THREADS, 0, st>>>(a);
  return occ4d::check_launch("occ4d_surface_count_f32");
}

extern "C" int occ4d_surface_write_f32(const float* density, int64_t ld, const float* attrs, int64_t ld_attr, int n_attr, int nx,
                                       int ny, int nz, float level, float x0, float sx, float y0, float sy, float z0, float sz,
                                       const int32_t* cell_offsets, const int32_t* face_offsets, int32_t* work, float* vertices,
                                       int64_t ld_v, int vertex_cap, int32_t* faces, int face_cap, void* stream) {
  sf::WriteArgs w; bool empty;
  OCC4D_TRY(sf::check_write(density, ld, attrs, ld_attr, n_attr, nx, ny, nz, level, x0, sx, y0, sy, z0, sz, cell_offsets, face_offsets,
                            work, vertices, ld_v, vertex_cap, faces, face_cap, empty, w));
  if (empty) return OCC4D_OK;
  const hipStream_t st = (hipStream_t)stream;
  surface_vertex_kernel<<<(unsigned)w.tiles, THREADS, 0, st>>>(w);
  surface_face_kernel<<<(unsigned)w.tiles, THREADS, 0, st>>>(w);
  return occ4d::check_launch("occ4d_surface_write_f32");
}
