/* occ4d_layers.h -- the labelled objects of the query grid as depth layers in camera views, on the device
 * (projection.object_layers, projection.ObjectLayers, inference.perform_inference(layers=...)): per pixel the objects its ray
 * passes through in the order it first enters them -- layer 0 is the object a viewer sees there, the later layers are the objects
 * behind it -- and per view and object the number of pixels its full extent covers (the AMODAL mask), the number in which it is in
 * front (the VISIBLE mask), its nearest sample and its amodal 2-D box.  The march does not stop at the first object.
 *
 * A header of include/ext/ beside occ4d_raycast.h and occ4d_boxes.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C",
 * int status (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit
 * sizes, the stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbol lives in libocc4d.so and in
 * the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.  The floats are fp32, every operation rounded on its own (the builds have -ffp-contract=off); everything that is
 * stored is an integer.
 *   GRID, CAMERAS, RAY, SAMPLES, GRID COORDINATE, IN the grid.  Those of occ4d_raycast.h, by reference, and in the source the very
 *     functions of csrc/raycast_math.hpp (ray_point, depth_of, grid_coord, in_axis): sample i = 0 .. n_steps - 1 of pixel (px, py)
 *     of view v lies at depth d_i = near + (float)i * step, at p_a = P0_a + d_i * dir_a, with the grid coordinate
 *     g_a = (p_a - origin_a) / spacing_a - 0.5f, and is IN the grid when 0.0f <= g_a && g_a <= (float)(n_a - 1) on all three axes.
 *   OBJECTS.  labels (n) int32 for n = nx * ny * nz, any values, K >= 0 objects: a value outside [0, K) names no object.
 *   OWNER of sample i.  Not in the grid: -1.  In the grid: the label of the NEAREST grid point,
 *         r_a = min((int)floorf(g_a + 0.5f), n_a - 1) per axis,      r = (rx * ny + ry) * nz + rz,      o = labels[r];
 *     an o outside [0, K) counts as -1.  The labelled region is thus the union of the cells centred on the labelled points.  No
 *     density and no level is read: the set is the label product's own.
 *   LAYERS of a pixel, 1 <= L <= OCC4D_LAYERS_MAX.  Walk i = 0 .. n_steps - 1 with count = 0.  For a sample with owner o >= 0 one of
 *     three cases holds:
 *       o is the label of a stored layer j:   samples[j] += 1;
 *       fewer than L layers are stored:       layer j = count is opened with label = o, first = i, samples = 1, point = r, and
 *                                             count += 1;
 *       otherwise:                            the object is dropped and count = L + 1.
 *     The march never ends early on overflow: re-entries of stored objects still add to samples.  Unused layers hold
 *     label = first = point = -1 and samples = 0.  So layer 0 is the object seen at the pixel, layers 1 .. those behind it in the
 *     order of first entry, and an object the ray enters twice is ONE layer.
 *   PER-PIXEL OUTPUTS, each may be null: label, first, samples, point (V, H, W, L) int32, and count (V, H, W) int32 in 0 .. L + 1.
 *     The depth of a layer is d_first = near + (float)first * step: the first sample inside a labelled cell, a depth quantised to
 *     the step, NOT the refined surface crossing of occ4d_raycast.h.
 *   TABLE (V, K, OCC4D_LAYERS_COLS) int32, may be null.  Per view and object, over the pixels in which the object is a STORED layer:
 *       OCC4D_LAYERS_AMODAL   number of pixels
 *       OCC4D_LAYERS_VISIBLE  pixels where it is layer 0
 *       OCC4D_LAYERS_NEAR     least first, INT32_MAX if none
 *       OCC4D_LAYERS_XMIN, OCC4D_LAYERS_XMAX   the amodal box along px (INT32_MAX / -1 if none)
 *       OCC4D_LAYERS_YMIN, OCC4D_LAYERS_YMAX   the amodal box along py (INT32_MAX / -1 if none)
 *   STATUS (2) int32, may be null: [pixels with count == L + 1, pixels with count >= 1].
 *   CONTRACT.  With status[0] == 0 the table is exact.  Otherwise AMODAL and VISIBLE are lower bounds (so are the boxes), and
 *     every stored layer is still right.  Everything in the table and in status is an integer sum, minimum or maximum, and every
 *     per-pixel element has one owner: the bits are the same under any scheduling.
 *   SHORTCUT.  Each g_a is weakly monotone in i -- (float)i, the product with step > 0, the sum with near, the product with dir_a,
 *     the sum with P0_a, the difference, the division and the last difference are each monotone under rounding, and a NaN stays
 *     one -- so the samples IN the grid are one contiguous range of i, and a ray ends once it has been in the grid and is out
 *     again.  The outputs are those of the walk over every sample.
 *
 * LAUNCHES.  TWO, whatever the data (csrc/layers.hip); ONE without table and status; none in the no-op cases below.  fill: every
 *   row of table becomes [0, 0, INT32_MAX, INT32_MAX, -1, INT32_MAX, -1], status [0, 0] -- the caller passes uninitialised arrays.
 *   march: 256 threads
 *   over 16 x 16 pixels of one view, a wave an 8 x 8 sub-tile (the tiling of csrc/raycast.hip); a lane keeps its layers in registers,
 *   writes its pixel's rows, and the wave then matches equal labels across its lanes per layer slot, reduces count, minimum and
 *   box over them and hands ONE contribution per label to the workgroup's gather table in LDS (OCC4D_LAYERS_GATHER_SLOTS objects
 *   keyed by label, a bounded probe sequence of OCC4D_LAYERS_GATHER_PROBES slots), or straight to table with integer atomics when
 *   that is full.  After one barrier each claimed slot goes to global memory once; status gets one atomic add per word and
 *   workgroup.  No workgroup waits for another one.  Every loop is a `for` whose bound is fixed before it starts.  Barriers stand
 *   in uniform control flow only.
 *
 * ACCESS SAFETY.  The one read indexed by data is labels[r]: every r_a is converted to an integer from a float that has just
 * passed 0 <= g_a <= n_a - 1 and is then limited to n_a - 1, so r is a grid point whatever the arrays, matrices and scalars hold.
 * The one write indexed by data is row (v, o) of table: o becomes a row number only after 0 <= o < K, so foreign labels move no
 * write.  A gather slot is (o + probe) mod OCC4D_LAYERS_GATHER_SLOTS.  The per-pixel rows are indexed by the thread's own pixel. */
#ifndef OCC4D_LAYERS_H
#define OCC4D_LAYERS_H

#include <stdint.h>

#define OCC4D_LAYERS_MAX 8                 /* L: the most layers kept per pixel */
#define OCC4D_LAYERS_COLS 7                /* columns of table */
#define OCC4D_LAYERS_AMODAL 0
#define OCC4D_LAYERS_VISIBLE 1
#define OCC4D_LAYERS_NEAR 2
#define OCC4D_LAYERS_XMIN 3
#define OCC4D_LAYERS_XMAX 4
#define OCC4D_LAYERS_YMIN 5
#define OCC4D_LAYERS_YMAX 6
#define OCC4D_LAYERS_GATHER_SLOTS 32       /* objects a workgroup gathers in LDS before global memory */
#define OCC4D_LAYERS_GATHER_PROBES 4       /* slots tried for an object before it goes to global memory directly */

#ifdef __cplusplus
extern "C" {
#endif

/* labels (n) int32, any values;  nx, ny, nz >= 2 with nx * ny * nz <= INT32_MAX;  K >= 0 with V * max(K, 1) * 7 < 2^31;
 *   x0, sx, y0, sy, z0, sz: origin and spacing per axis, the floats of occ4d_grid_points_f32.
 * k_inv, rt_inv (V, 16): the INVERSES of the expanded camera matrices;  V >= 0;  0 <= H, W <= 32768;  V * H * W < 2^31.
 * near finite, step finite and > 0, 1 <= n_steps <= OCC4D_RAYCAST_MAX_STEPS (65536).
 * 1 <= L <= OCC4D_LAYERS_MAX with V * H * W * L < 2^31.
 * label, first, samples, point (V, H, W, L), count (V, H, W), table (V, K, 7), status (2): int32, contiguous, each may be null.
 * V == 0, H * W == 0 or all seven outputs null is a no-op that touches no pointer.  Otherwise labels, k_inv and rt_inv must not be
 * null; with K == 0 table is not touched. */
int occ4d_layers_march_i32(const int32_t* labels, int nx, int ny, int nz, int K, float x0, float sx, float y0, float sy, float z0,
                           float sz, const float* k_inv, const float* rt_inv, int V, int H, int W, float near_depth, float step,
                           int n_steps, int L, int32_t* label, int32_t* first, int32_t* samples, int32_t* point, int32_t* count,
                           int32_t* table, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif
