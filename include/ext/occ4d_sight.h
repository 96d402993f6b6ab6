/* occ4d_sight.h -- line of sight through the solid set of the query grid, on the device (sight.look, inference.perform_inference(
 * sight=...)): per grid point and per sensor origin whether the straight segment between the two passes through free cells only --
 * the point is SEEN -- or meets predicted solid first -- it is HIDDEN --, and which cell did the hiding.  Integers only: the float
 * operations are the >= comparisons of the member test, and the rules below fix every output bit whatever the scheduling.
 *
 * A header of include/ext/ beside occ4d_distance.h; a row of _lib.ADDON_HEADERS.  The same conventions -- extern "C", int status
 * (OCC4D_OK / OCC4D_EINVAL / OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and
 * strides, the stream as void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in
 * the g++ twin (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_distance.h: (nx, ny, nz) points, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal.  Every axis is <= OCC4D_SIGHT_MAX_AXIS.
 *   MEMBER.  The member test of occ4d_distance.h: solid(p) = field[p * ld] >= level, an fp32 comparison, a NaN value or a NaN level is
 *     no member; with `mask` not null also mask[p * ld_mask] >= mask_level (the same comparison).  A lattice point outside the grid
 *     is free.
 *   BITS.  bits is an array of ceil(n / 32) uint32 words: bit p % 32 of word p / 32 is solid(p); the unused bits of the last word
 *     are 0.  occ4d_sight_bits_f32 makes it, occ4d_sight_grid_u32 reads nothing else of the field.
 *   ORIGINS.  V lattice points o_v = (ox, oy, oz), int32, 1 <= V <= OCC4D_SIGHT_MAX_ORIGINS.  They may lie outside the grid; every
 *     coordinate is in [-OCC4D_SIGHT_MAX_COORD, OCC4D_SIGHT_MAX_COORD], anything else is OCC4D_EINVAL.  A sensor position becomes
 *     the cell that contains it, floor((position - mins) / spacings), in float64 on the host (sight.grid_origin).  THAT SNAP, OF AT
 *     MOST ONE CELL, IS THE ONLY APPROXIMATION: everything below is exact on the lattice.
 *   WALK from a query q to an origin o: the supercover of the segment between the two cell centres.
 *     d_a = o_a - q_a, s_a = sign(d_a), m_a = |d_a| for the three axes a;  c = q, j_a = 0.  If every m_a is 0, q is seen.  Otherwise
 *     repeat:
 *       1. The live axes are those with j_a < m_a.  Axis a crosses its next cell boundary at t_a = (2 j_a + 1) / (2 m_a).
 *       2. Compared exactly, in 64-bit integers:  t_a < t_b  iff  (2 j_a + 1) * m_b < (2 j_b + 1) * m_a.
 *       3. T = the live axes that attain the least t.
 *       4. SQUEEZE, only when |T| >= 2 (the segment passes exactly through an edge or a corner of the cell).  The step passes iff
 *          there is an order of the axes of T such that the cells reached by stepping them one at a time in that order, the last one
 *          excluded, are all free: for |T| = 2 one of the two side cells, for |T| = 3 one of the six two-cell staircases.  If the
 *          step does not pass, q is hidden from o; its blocker is the lowest flat index among the solid ones of those intermediate
 *          cells (two for |T| = 2, six for |T| = 3).
 *       5. Step every axis of T:  c_a += s_a, j_a += 1.
 *       6. If c == o, q is seen: o itself is never tested.
 *       7. If c is outside the grid, q is seen: the grid is convex, the rest of the segment lies outside it.
 *       8. If solid(c), q is hidden and its blocker is flat(c).
 *     q itself is never tested either: a solid query on the surface that faces the sensor is seen, one inside an object is hidden.
 *     The loop is a `for` bounded by nx + ny + nz: a step moves at least one axis by one cell towards o and ends at the first cell
 *     outside the grid.
 *   OUTPUTS.
 *     framed (n) int32, or null: an INPUT, bit v says whether origin v may look at the query at all (its frustum); null = every bit.
 *     seen (n) int32: bit v is set iff bit v of framed is set and q is seen from o_v.  Bits V .. 31 are 0.
 *     blocker (V, n) int32, or null (not computed): blocker[v * n + q] = the blocking cell's flat index; -1 where q is seen from
 *       o_v or not framed by it.
 *     Every output element has one owner, there are no atomics: the same bits under any scheduling.
 *
 * LAUNCHES.  One per entry point, whatever the data (csrc/sight.hip).  occ4d_sight_bits_f32: a wave makes two words with a ballot
 *   each.  occ4d_sight_grid_u32: one thread per query, a wave owns a compact block of OCC4D_SIGHT_BLOCK_X x _Y x _Z queries; the
 *   thread loops over the V origins, which travel in the kernel's arguments, gathers its bits in a register and stores once per
 *   output.  `bits` is read where it is, in global memory (67 KB at 96 x 96 x 58: it stays in the caches).  A variant that walked
 *   a copy of `bits` in LDS was built and measured slower on every field; it is gone, and `flags`, which chose between the two,
 *   must be 0.  No work array, no workgroup waits for another one.
 *
 * ACCESS SAFETY.  No value read from memory reaches an address without a range test.  field and mask are read at p in [0, n) only,
 * with p from the thread's own index; seen, framed and blocker are indexed by the thread's own query, which is tested against the
 * grid.  A word of bits is read only for a cell whose three coordinates were tested against [0, nx) x [0, ny) x
 * [0, nz) immediately before, so its index is < ceil(n / 32).  The origins are range-checked on the host before the launch and only
 * enter comparisons, additions and the cell coordinates that pass the same test.  A value of bits, framed or blocker is never an
 * index. */
#ifndef OCC4D_SIGHT_H
#define OCC4D_SIGHT_H

#include <stdint.h>

#define OCC4D_SIGHT_MAX_AXIS 512           /* the longest axis */
#define OCC4D_SIGHT_MAX_ORIGINS 31         /* V: one bit of seen / framed each, the sign bit stays free */
#define OCC4D_SIGHT_MAX_COORD 1048576      /* |coordinate| of an origin: 2^20 */
#define OCC4D_SIGHT_BLOCK_X 4              /* the block of queries of one wave */
#define OCC4D_SIGHT_BLOCK_Y 4
#define OCC4D_SIGHT_BLOCK_Z 4

#ifdef __cplusplus
extern "C" {
#endif

/* field: one value per grid point, element stride ld >= 1 (a column of the dense array, the pointer already at that column);
 * mask: null, or a second such column with stride ld_mask >= 1;  0 <= n <= INT32_MAX;  bits (ceil(n / 32)) uint32.
 * n == 0 is a no-op that touches no pointer. */
int occ4d_sight_bits_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                         int64_t n, uint32_t* bits, void* stream);

/* bits: as above, for n = nx * ny * nz;  0 <= nx, ny, nz <= OCC4D_SIGHT_MAX_AXIS;  origins_host (V, 3) int32 ON THE HOST, read and
 * range-checked before the call returns and handed to the kernel by value;  framed (n) int32 or null;  seen (n) int32;  blocker
 * (V, n) int32 or null;  flags: 0, no bit exists.  n == 0 is a no-op that touches no pointer. */
int occ4d_sight_grid_u32(const uint32_t* bits, int nx, int ny, int nz, const int32_t* origins_host, int V, const int32_t* framed,
                         int32_t* seen, int32_t* blocker, int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif
