/* occ4d_evidence.h -- measured returns carved into the query grid, on the device (evidence.py, ops.grid_carve / ops.grid_evidence,
 * inference.perform_inference(evidence=...)): what the sensors actually established about the scene, and how the predicted solid
 * set stands against it.  A measured return proves that the cells between its sensor and itself were empty and that its own cell was
 * not; everything else is unknown.  Per grid cell: how many returns end in it, whether any ray passed through it, and one of six
 * codes that cross that state with the predicted solid set.  Integer marks, sums and ORs only: every output bit is the same under
 * any scheduling and any order of the returns.
 *
 * One more header of include/ext/ (_lib.ADDON_HEADERS, whose list is open; include it as "ext/occ4d_evidence.h") beside occ4d.h,
 * whose symbol set and OCC4D_ABI_VERSION are pinned.  The same conventions -- extern "C", int status (OCC4D_OK / OCC4D_EINVAL /
 * OCC4D_ELAUNCH of occ4d.h, message through occ4d_last_error()), device pointers, explicit sizes and strides, the stream as
 * void*, no allocation, no hidden synchronisation, nothing read back.  The symbols live in libocc4d.so and in the g++ twin
 * (libocc4d_cpu.so: host pointers, synchronous).
 *
 * THE RULES.
 *   GRID.  That of occ4d_sight.h: (nx, ny, nz) cells, x slowest, z fastest, flat index p = (ix * ny + iy) * nz + iz,
 *     n = nx * ny * nz.  An axis of length 1 is legal; an axis of length 0 makes a grid without cells, which every return lies
 *     outside of.  Every axis is <= OCC4D_SIGHT_MAX_AXIS.  min_a, spacing_a: the floats the ray cast is handed for the same grid
 *     (occ4d_raycast.h's origin and spacing): cell i of axis a covers [min_a + i * spacing_a, min_a + (i + 1) * spacing_a).
 *   INPUTS.  returns (R, >= 3) float32 world points, row stride ld >= 3, 0 <= R <= INT32_MAX.  sensor (R) int32: the sensor of
 *     every return, or null: every return belongs to sensor 0.  origins (V, 3) int32 lattice cells ON THE DEVICE, one per sweep and
 *     view, 1 <= V <= OCC4D_EVIDENCE_MAX_SENSORS: a table, not kernel arguments -- a clip of 3 views x 12 frames has 36 sensors.
 *     The kernel checks every value it reads of `sensor` and `origins` (DROPPED 1), as occ4d_viewplan.h does for its candidates.
 *   SNAP.  The cell of a return p is, per axis, in float32, each operation rounded on its own (IEEE subtraction and division, the
 *     builds have -ffp-contract=off):
 *         g_a = floorf((p_a - min_a) / spacing_a)
 *     the cell that CONTAINS the point: the convention of geodesic.grid_index / sight.grid_origin.  A numpy float32 restatement
 *     is equal.  The sensors are snapped on the host in float64 by sight.grid_origin: the same one approximation as occ4d_sight.h's.
 *   DROPPED.  A return falls out, in this fixed priority, and is counted in `status`:
 *       1. its sensor index v is outside [0, V), or origin v has a coordinate outside [-OCC4D_EVIDENCE_MAX_COORD,
 *          OCC4D_EVIDENCE_MAX_COORD];
 *       2. for some axis !(fabsf(g_a) <= 1048576.0f): a coordinate or its quotient is not finite (a NaN fails the comparison), or
 *          the cell lies beyond 2^20 cells;
 *       3. its cell e = (g_x, g_y, g_z) lies outside the grid.
 *     A dropped return marks nothing.  OUT OF SCOPE: a return outside the grid whose ray crosses the grid.  Carving it needs an
 *     exact rule for where the segment enters the grid; there is none here, so such a return is dropped (3) and its ray stays unknown.
 *   WALK from the return's cell e towards its sensor's cell o: the stepping rule of occ4d_sight.h's WALK, steps 1 - 3 and 5, with
 *     q = e: d_a = o_a - e_a, s_a = sign(d_a), m_a = |d_a|; axis a crosses its next cell boundary at t_a = (2 j_a + 1) / (2 m_a),
 *     compared exactly in 64-bit integers whose six terms grow by additions; THE LIVE AXES THAT ATTAIN THE LEAST t ADVANCE
 *     TOGETHER.  There is no SQUEEZE and no solid test.  Every cell stepped into after e is PASSED, up to and including o, as long as
 *     it lies in the grid; the walk ends at o or with the first cell outside the grid (the grid is convex: the rest of the segment
 *     lies outside it).  The loop is a `for` bounded by nx + ny + nz.  A cell the segment touches only at an edge or a corner is not
 *     stepped into, so it is not carved: THE SIDE THE RULE ERRS ON IS "UNKNOWN".  e is HIT.  e == o is a hit and nothing else.
 *   PER CELL.  hits[p]: the number of returns that end in p.  passed: bit p % 32 of word p / 32 says that at least one walk passed
 *     through p; the unused bits of the last word are 0.  passes[p] (optional): how many walks did.
 *   STATE.  HIT (2) when hits[p] > 0 -- a hit wins over grazing rays --; else FREE (1) when p is passed: with `passes` given when
 *     passes[p] >= min_pass, else when its bit of `passed` is set; else UNKNOWN (0).
 *   SOLID.  The member test of occ4d_sight.h (MEMBER): field[p * ld] >= level, and with mask also mask[p * ld_mask] >= mask_level;
 *     the implementation calls that function.
 *   CODE = STATE + 3 * SOLID:
 *         0 UNKNOWN_FREE      1 CONFIRMED_FREE    2 MISSED            (a return in predicted air)
 *         3 COMPLETED         4 CONTRADICTED      5 CONFIRMED_SOLID   (3: a predicted solid no ray reached; 4: one in measured free space)
 *   OUTPUTS.  code (n) int32;  totals (6) int64: the histogram of code;  status (4) int32 = [returns carved, dropped for the
 *     sensor (1), dropped as not finite or too far (2), dropped outside the grid (3)]: status sums to R.
 *
 * LAUNCHES (csrc/evidence.hip).  occ4d_evidence_carve_f32: one clear of the outputs, one carve.  occ4d_evidence_classify_f32: one clear of
 *   totals, one classify.  The count is fixed whatever the data, nothing is read on the host, no workgroup waits for another, and
 *   every loop is a `for` with a bound fixed before it starts.  Carve: one return per thread, a wave takes 64 consecutive returns
 *   (neighbours of a sweep, whose walks share their cells near the sensor).  The passed bits are marked in the workgroup's own
 *   copy of the whole bit array in LDS and the non-zero words are ORed into `passed` at the end, whenever the array fits
 *   OCC4D_EVIDENCE_LDS_WORDS; a larger grid, which no LDS holds, is marked with integer ORs straight into `passed`.  That is a
 *   rule of capacity, not a switch: both give the same bits, and there is no flag.  hits and passes are global integer adds.
 *   Classify: one thread per cell, totals reduced per wave and per workgroup before six 64-bit adds per workgroup.
 *
 * ACCESS SAFETY.  returns and sensor are indexed by the thread's own return r < R.  A sensor index read from memory is tested
 * against [0, V) before it indexes origins.  A flat cell index is formed only from three coordinates that have just passed the test
 * against [0, nx) x [0, ny) x [0, nz): it is < n, and its word < ceil(n / 32).  The snap's float is tested against 2^20 before it
 * becomes an integer.  An origin's coordinates are tested against 2^20 and then only enter comparisons and additions.  field, mask,
 * hits, passes, passed and code are read and written at the thread's own p < n.  No value of hits, passes or passed is an index. */
#ifndef OCC4D_EVIDENCE_H
#define OCC4D_EVIDENCE_H

#include <stdint.h>

#define OCC4D_EVIDENCE_MAX_SENSORS 4096        /* V */
#define OCC4D_EVIDENCE_MAX_COORD 1048576       /* |coordinate| of an origin and of a return's cell: 2^20 (OCC4D_SIGHT_MAX_COORD) */
#define OCC4D_EVIDENCE_UNKNOWN 0               /* STATE */
#define OCC4D_EVIDENCE_FREE 1
#define OCC4D_EVIDENCE_HIT 2
#define OCC4D_EVIDENCE_LDS_WORDS 32768         /* the most words of `passed` a workgroup stages in LDS: 128 KiB, grids of up to 2^20 cells */

#ifdef __cplusplus
extern "C" {
#endif

/* returns (R, >= 3) with row stride ld_returns >= 3;  sensor (R) int32 or null;  origins (V, 3) int32 on the device;
 * 0 <= nx, ny, nz <= OCC4D_SIGHT_MAX_AXIS, n = nx * ny * nz;  x0, sx, y0, sy, z0, sz: min and spacing per axis, finite, spacing > 0;
 * passed (ceil(n / 32)) uint32, hits (n) int32: required with n > 0;  passes (n) int32 or null (not counted);  status (4) int32;
 * All outputs are cleared first: R == 0 leaves zeros. */
int occ4d_evidence_carve_f32(const float* returns, int64_t ld_returns, int64_t R, const int32_t* sensor, const int32_t* origins, int V,
                             int nx, int ny, int nz, float x0, float sx, float y0, float sy, float z0, float sz, uint32_t* passed,
                             int32_t* hits, int32_t* passes, int32_t* status, void* stream);

/* field, ld, level, mask, ld_mask, mask_level: the operands of occ4d_sight_bits_f32;  0 <= n <= INT32_MAX;  hits (n) int32;
 * passes (n) int32 with min_pass >= 1, or null: then passed (ceil(n / 32)) uint32 and min_pass == 1;  code (n) int32;
 * totals (6) int64.  n == 0 clears totals and touches nothing else. */
int occ4d_evidence_classify_f32(const float* field, int64_t ld, float level, const float* mask, int64_t ld_mask, float mask_level,
                                int64_t n, const uint32_t* passed, const int32_t* passes, int min_pass, const int32_t* hits,
                                int32_t* code, int64_t* totals, void* stream);

#ifdef __cplusplus
}
#endif

#endif
