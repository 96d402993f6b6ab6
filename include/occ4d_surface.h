/* occ4d_surface.h -- the occupancy surface of the dense query grid as a quad mesh (inference.perform_inference(surface=...),
 * surface.py): naive surface nets over one column of the dense (N, G) array, with the other columns interpolated onto the
 * vertices.  No case tables, one vertex per crossed cell, one quad per crossed interior grid edge, no atomics: every output
 * element has one owner, and the orders below fix the result bit for bit.
 *
 * A ninth header beside occ4d.h (whose symbol set and OCC4D_ABI_VERSION are pinned) and the other feature headers: the same
 * conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through
 * occ4d_last_error()), device pointers, explicit sizes and strides, the stream as void*, no allocation, no hidden
 * synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin (libocc4d_cpu.so: host pointers,
 * synchronous).
 *
 * THE RULES.  The grid is the flat one of occ4d_grid_points_f32: (nx, ny, nz) points (ix, iy, iz), x slowest, z fastest, flat
 * index (ix * ny + iy) * nz + iz = n points.  f(p) = density[p * ld], fp32.
 *   inside(p) = f(p) >= level          (fp32; a NaN is outside: the comparison of the solid split)
 *   CELL (cx, cy, cz), 0 <= c_axis <= n_axis - 2, has the corners p + {0, 1}^3 and is CROSSED when its corners are neither all
 *     inside nor all outside.  A cell is identified by the flat index of its low corner: cell order is point order, and one
 *     tiling of the points in tiles of 256 serves cells and edges alike.
 *   EDGE PARAMETER, from the lower-index endpoint l to the upper endpoint u:
 *     t = (level - f(l)) / (f(u) - f(l));  if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;       (the fallback: NaN, +-inf)
 *   VERTEX of a crossed cell.  Its 12 edges are visited in this order: axis a = 0, 1, 2; with (b, c) = ((a + 1) % 3,
 *     (a + 2) % 3), the corner offsets (j on b, k on c) = (0,0), (0,1), (1,0), (1,1).  For every edge whose endpoints differ in
 *     `inside`: its crossing position in cell units is added to a running fp32 sum s (on axis a the position is t, on the other
 *     two the corner offset as 0.0f / 1.0f), for every attribute column A(l) + t * (A(u) - A(l)) is added to that column's
 *     running sum, and the edge is counted in k.  Then u = s / (float)k per axis, the attribute sums are divided in the same way,
 *     and the world position per axis is (((float)c + 0.5f) + u) * spacing + origin: the grid's own expression with the offset
 *     added.  No FMA anywhere.  The vertex row is (x, y, z, attr[0 .. n_attr)); vertices are numbered in cell order.
 *   FACES.  For a point p and an axis a with q = p + e_a in the grid and inside(p) != inside(q), a quad is emitted only when
 *     1 <= p_b <= n_b - 2 and 1 <= p_c <= n_c - 2, so that four cells share the edge.  It is the vertices of the cells
 *     p + (db, dc) for (db, dc) = (-1,-1), (0,-1), (0,0), (-1,0), in that order when inside(p), reversed otherwise: normals
 *     point from inside to outside.  Edges on the grid's faces emit nothing: the mesh is open there.  Faces are ordered by
 *     p * 3 + a; their entries are int32 vertex numbers.
 *
 * Limits of both entry points: nx, ny, nz >= 0 with 3 * nx * ny * nz <= INT32_MAX; ld >= 1; an empty grid (n == 0) is a no-op
 * that touches no pointer.  A grid with an axis of 1 has no cells: its totals are written as 0. */
#ifndef OCC4D_SURFACE_H
#define OCC4D_SURFACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The count.
 *   density: one value per grid point, element stride ld (a column of the dense array, the pointer already at that column);
 *   cell_offsets (ceil(n / 256)) int32: the exclusive prefix of the crossed cells per tile of 256 points;
 *   face_offsets (ceil(n / 256)) int32: the exclusive prefix of the faces per tile of 256 points;
 *   totals int32[2]: the number of vertices and the number of faces.
 * Two launches: tiles -> counts, then the prefix of both arrays (one workgroup each, any number of tiles). */
int occ4d_surface_count_f32(const float* density, int64_t ld, int nx, int ny, int nz, float level, int32_t* cell_offsets,
                            int32_t* face_offsets, int32_t* totals, void* stream);

/* The mesh.
 *   density, ld, nx, ny, nz, level, cell_offsets, face_offsets: as given to / left by occ4d_surface_count_f32;
 *   attrs (n, n_attr), row stride ld_attr >= n_attr, 0 <= n_attr <= 32: the columns interpolated onto the vertices (may be
 *     null when n_attr == 0; may be the dense array itself);
 *   x0, sx, y0, sy, z0, sz: origin and spacing per axis, the floats of occ4d_grid_points_f32;
 *   work (n) int32: receives the vertex number of every point's cell, or -1 (no cell there, or not crossed);
 *   vertices (vertex_cap, 3 + n_attr), row stride ld_v >= 3 + n_attr; faces (face_cap, 4) int32, dense.
 * A vertex number is cell_offsets[tile] + the cell's rank among the crossed cells of its tile, a face number
 * face_offsets[tile] + the face's rank in its tile: the only data-dependent positions.  A vertex row is written only when its
 * number lies in [0, vertex_cap), a face only when its number lies in [0, face_cap): whatever the offset arrays hold, nothing
 * outside the two output arrays is written (the guard of occ4d_refine_expand_f32); offsets other than the count's may send two
 * items to one position, which then holds one of them.  Columns 3 + n_attr .. ld_v - 1 of a vertex
 * row are never touched.  vertices / faces may be null when their capacity is 0.
 * Two launches: the vertex pass (work, vertices), then the face pass (reads work). */
int occ4d_surface_write_f32(const float* density, int64_t ld, const float* attrs, int64_t ld_attr, int n_attr, int nx, int ny, int nz,
                            float level, float x0, float sx, float y0, float sy, float z0, float sz, const int32_t* cell_offsets,
                            const int32_t* face_offsets, int32_t* work, float* vertices, int64_t ld_v, int vertex_cap,
                            int32_t* faces, int face_cap, void* stream);

#ifdef __cplusplus
}
#endif

#endif
