/* occ4d_boxes.h -- upright oriented boxes of the labelled objects of the query grid, on the device (components.Boxes,
 * inference.perform_inference(boxes=...)): for every object of a label volume and every heading of a fixed table, the extent of
 * the object's footprint along that heading and across it, and per object the heading whose rectangle has the least area -- the
 * search-based rectangle fit.  Integers only, no floats anywhere: the rules below fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_components.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes, the
 * stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.  Integers only.
 *   GRID.  That of occ4d_components.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  Every axis lies in [0, OCC4D_BOXES_MAX_AXIS] and n <= INT32_MAX.  An axis of length 1 is legal.
 *   OBJECTS.  labels (n) int32, any values.  Point p belongs to object labels[p] when 0 <= labels[p] < K; every other value belongs
 *     to no object.  The array comes from occ4d_components_label_f32 or occ4d_watershed_label_i32, but nothing here trusts that.
 *     K >= 0 and K * A * 4 <= INT32_MAX.
 *   DIRECTIONS.  dirs (A, 4) int32 ON THE DEVICE, 1 <= A <= OCC4D_BOXES_MAX_DIRS.  Row a is (ax, ay, bx, by); a point's coordinates
 *     along and across direction a are
 *         u = ax * ix + ay * iy,        v = bx * ix + by * iy.
 *     The values are device data: a row with a coefficient outside [-OCC4D_BOXES_MAX_COEF, OCC4D_BOXES_MAX_COEF] is DEAD, and the
 *     kernel makes that test before a coefficient is used.  With live rows |u|, |v| <= 2 * 2^15 * 2047 < 2^28: int32 never overflows.
 *     Nothing asks the two vectors to be orthogonal or of one length; components.yaw_directions makes them so in world space.
 *   EXTENTS.  extent (K, A, 4) int32: row (k, a) is [min u, max u, min v, max v] over the points of object k, and the EMPTY row
 *     [INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN] when k has no point or a is DEAD.
 *   RANGE.  zr (K, 3) int32: [min iz, max iz, number of points] of object k, [INT32_MAX, INT32_MIN, 0] for an object without
 *     points.  Every combination above is a minimum, a maximum or an integer sum: any order gives the same bits.
 *   CHOICE.  box (K, OCC4D_BOXES_COLS) int32: [a*, min u, max u, min v, max v, min iz, max iz, points].
 *     points <= 0: the row is [-1, 0, 0, 0, 0, 0, 0, 0].
 *     Otherwise, over the directions a that are not DEAD and whose extent row has 0 <= max - min < 2^30 on both axes (the
 *     difference in 64 bits):
 *         W1 = max u - min u + |ax| + |ay|,        W2 = max v - min v + |bx| + |by|
 *       -- the added term is the width of one cell's square along the direction, so the rectangle covers the cells, not just their
 *       centres, and a one-cell object has a box of one cell, not of area 0 --,
 *         area = W1 * W2 in int64 (W < 2^30 + 2^16, the product below 2^61);
 *       a* is THE LOWEST a of least area, and the row carries that direction's four extents.
 *     If no direction qualifies: a* = -1, the four extents 0, the z range and the count kept.
 *     extent and zr are CALLER data in that call: any values.  Nothing read from them becomes an index.
 *
 * LAUNCHES.  A fixed number, whatever the data (csrc/boxes.hip).
 *   occ4d_boxes_extents_i32: TWO.  fill: every row of extent and zr becomes its EMPTY row.  reduce: a workgroup owns a tile of
 *     OCC4D_BOXES_TILE x OCC4D_BOXES_TILE columns (ix, iy); a wave walks its share of them with the DIRECTIONS ACROSS ITS LANES
 *     (lane l takes a = l, l + 64, ...): u and v do not depend on iz, so a column costs one projection per lane and direction.  The
 *     wave loads 64 labels of a column at once, steps through the runs of equal labels -- the label is the same in every lane --,
 *     keeps the running minima and maxima of one object in registers and hands them over when another object begins: first to the
 *     workgroup's gather table in LDS (OCC4D_BOXES_GATHER_SLOTS objects, keyed by label, a bounded probe sequence of
 *     OCC4D_BOXES_GATHER_PROBES slots), and straight to extent and zr with integer atomic minima, maxima and adds when the table is
 *     full.  After one barrier each claimed slot goes to global memory once.  With n == 0 only fill is launched.
 *   occ4d_boxes_choose_i32: ONE.  A wave per object, the lanes over the directions, the least (area, a) key reduced over the wave.
 *   No workgroup waits for another one.  Every loop is a `for` whose bound is fixed before it starts.  Barriers stand in uniform
 *   control flow only.
 *
 * ACCESS SAFETY.  labels is read at p in [0, n) only, with p made of the wave's own column and lane.  A label becomes a row number
 * only after 0 <= k < K, so foreign labels move no write out of extent or zr; a direction's number is the lane's own, below A.  A
 * gather slot is (k + probe) mod OCC4D_BOXES_GATHER_SLOTS.  In the choice, a* is a lane number that passed a < A; no value of
 * extent, zr or dirs is ever an index. */
#ifndef OCC4D_BOXES_H
#define OCC4D_BOXES_H

#include <stdint.h>

#define OCC4D_BOXES_MAX_AXIS 2048          /* nx, ny, nz */
#define OCC4D_BOXES_MAX_DIRS 256           /* A */
#define OCC4D_BOXES_MAX_COEF 32768         /* |ax|, |ay|, |bx|, |by| of a live direction */
#define OCC4D_BOXES_COLS 8                 /* columns of box */
#define OCC4D_BOXES_TILE 8                 /* the columns per axis of a workgroup's share in x and in y */
#define OCC4D_BOXES_GATHER_SLOTS 8         /* objects a workgroup gathers in LDS before global memory */
#define OCC4D_BOXES_GATHER_PROBES 4        /* slots tried for an object before it goes to global memory directly */

#ifdef __cplusplus
extern "C" {
#endif

/* labels (n) int32 for n = nx * ny * nz, any values;  0 <= nx, ny, nz <= OCC4D_BOXES_MAX_AXIS, n <= INT32_MAX;  K >= 0;  dirs (A, 4)
 * int32, any values, 1 <= A <= OCC4D_BOXES_MAX_DIRS, K * A * 4 <= INT32_MAX;  extent (K, A, 4) int32;  zr (K, 3) int32.
 * K == 0 is a no-op that touches no pointer.  n == 0 with K > 0 writes the EMPTY rows and reads no label (labels may be null). */
int occ4d_boxes_extents_i32(const int32_t* labels, int nx, int ny, int nz, int K, const int32_t* dirs, int A, int32_t* extent,
                            int32_t* zr, void* stream);

/* extent (K, A, 4) int32, zr (K, 3) int32, any values;  dirs (A, 4) int32 as above;  K >= 0, 1 <= A <= OCC4D_BOXES_MAX_DIRS,
 * K * A * 4 <= INT32_MAX;  box (K, OCC4D_BOXES_COLS) int32.  K == 0 is a no-op that touches no pointer. */
int occ4d_boxes_choose_i32(const int32_t* extent, const int32_t* zr, const int32_t* dirs, int K, int A, int32_t* box, void* stream);

#ifdef __cplusplus
}
#endif

#endif
