// What one row chunk of the decoder launches, as a value: plan_chunk() decides, decoder_forward (csrc/path.hip) walks the
// result -- it takes the workspace and issues the launches and decides nothing.  Host-only, no HIP: tests/decoder_plan_main.cpp
// enumerates the inputs under plain g++ and holds every plan to the invariants below.
//
// Where the lin_z term of block i (x += lin_z[i](features_query), the exact-in-R form of DESIGN.md 4 (ii)) is added
// (the lin_z and chain rows).  On the fp32 row-resident trunk, for a cross layer j behind block b - 1 whose post
// Linear is the fp32 row kernel (post_rows_ok): the term of block b rides in that launch (added to its output rows:
// Run::post_add), and where no cross layer sits behind block b, the same launch stores the term of block b + 1 as dense rows
// (Run::post_dense), which block b's launch adds from loads under its last chunk.  Every other term (the leading blocks of
// the published layouts; k_local != 8; the penult output; trunk4; the split-precision trunks; OCC4D_LINZ_PATH_STANDALONE) is
// formed by a pass in front of its block: the stand-alone one (PASS_INTERP_ADD), or the joint pass in front of a chain of
// blocks (PASS_INTERP_DENSE), which stores the later blocks' terms as dense rows too.  All placements add the same s last
// onto the same row: one result, bit for bit.  OCC4D_PATH_FUSED_INTERP (the exposed gathers in the block's epilogue, measured
// neutral) is accepted and selects nothing: what it moved is where the default puts it now, hidden.
//
// Consecutive blocks with no cross layer between them run as ONE launch (occ4d_resblock_chain_f32), at most CHAIN_BLOCKS of
// them, where the terms are routed at all (`linz`) and OCC4D_CHAIN_PATH_SEPARATE is not set.  The term of a chained block
// other than the first must arrive as dense rows: from the post Linear in front of the chain or from the joint pass, which
// also adds the first block's term.  With chain_tail the merged query projection of the cross layer behind the chain runs in
// the chain's launch too (Run::n_tail outputs).
//
// Dense rows live in the chunk's one `dense` buffer (taken when any post Linear stores a term) or in a fresh row buffer of the
// run.  A post Linear's dense rows are read by the first block of the run behind it, so a run whose first block reads none
// may reuse `dense` for the first term its pass stores.
//
// What every plan satisfies: the runs tile blocks 0 .. nB - 1 in order; the cross layers come in order, each behind the block
// cross_after names; every term 0 .. nB - 1 is delivered exactly once -- as a pass's slot 0, as a post Linear's added term, or as
// dense rows written once and read by exactly the block in front of the term's block; no buffer is written while an earlier
// write is unread, or read before it is written.
#pragma once
#include <stdint.h>

#include "ext/occ4d_chain.h"   // occ4d.h (OCC4D_MAX_BLOCKS, OCC4D_MAX_CROSS) + OCC4D_CHAIN_PATH_SEPARATE
#include "ext/occ4d_linz.h"    // OCC4D_LINZ_PATH_STANDALONE

namespace occ4d_plan {

constexpr int CHAIN_BLOCKS = 3;       // most residual blocks of one occ4d_resblock_chain_f32 launch

struct Inputs {
  int nB, nC, cross_after[OCC4D_MAX_CROSS];
  bool resblock, trunk4, x6trunk, f16block;     // DecoderLayout's kernel families
  bool post_rows_ok[OCC4D_MAX_CROSS];           // the layer's post Linear is the fp32 row kernel (takes lin_z terms along)
  bool tail_ok[OCC4D_MAX_CROSS];                // ... its merged query projection too (may run as a chain's tail)
  int D[OCC4D_MAX_CROSS];                       // the layer's width: the tail has 2 D outputs
  int flags;                                    // only OCC4D_LINZ_PATH_STANDALONE and OCC4D_CHAIN_PATH_SEPARATE are read
  int k_local, H, m, c;                         // c: rows of this chunk
  bool penult_given, chain_tail;
  bool one_pass;                                // the cross layers run the chunk's c rows as one pass of their own
};

// where rows are written to / read from; >= 0: fresh row buffer number k of the run, (c, H), taken in slot order
enum : int { ROWS_NONE = -3, ROWS_X = -2, ROWS_DENSE = -1 };
enum Pass { PASS_NONE, PASS_INTERP_ADD, PASS_INTERP_DENSE };
enum Kernel { K_CHAIN, K_F16_BLOCK, K_SPLIT_PAIR, K_RESBLOCK4, K_RESBLOCK_ADDROWS, K_RESBLOCK, K_GENERIC_PAIR };

struct Run {
  int first, nb;                 // blocks first .. first + nb - 1
  int cross;                     // the cross layer behind the run's last block, or -1
  int n_tail;                    // outputs of that layer's query projection in the run's launch (K_CHAIN), or 0
  Pass pass;                     // the lin_z pass in front of the run
  int slot_term[3];              // its terms, -1: none.  Slot 0 is added to x, slots 1, 2 are stored as dense rows
  int slot_rows[3];              // ROWS_X / ROWS_NONE for slot 0; ROWS_DENSE / fresh k / ROWS_NONE for slots 1, 2
  int n_fresh;                   // fresh row buffers of the run
  int addrows[CHAIN_BLOCKS];     // per block of the run: the dense rows its launch adds (the NEXT block's term), or ROWS_NONE
  Kernel kernel;
  int post_add, post_dense;      // terms the cross layer's post Linear adds to its output / stores into `dense`, or -1
};

struct ChunkPlan {
  bool linz, chain, any_dense;   // terms routed at all / blocks chained / the chunk has a `dense` buffer
  int n_runs;
  Run run[OCC4D_MAX_BLOCKS];
};

inline ChunkPlan plan_chunk(const Inputs& in) {
  ChunkPlan P{};
  const int nB = in.nB, nC = in.nC;
  const int64_t lim = (int64_t)1 << 30;           // the routed kernels' 32-bit row offsets
  P.linz = !(in.flags & OCC4D_LINZ_PATH_STANDALONE) && in.resblock && !in.trunk4 && !in.x6trunk && !in.penult_given &&
           in.k_local == 8 && (int64_t)in.m * nB * in.H < lim && (int64_t)in.c * in.H < lim;
  P.chain = P.linz && !(in.flags & OCC4D_CHAIN_PATH_SEPARATE);
  // terms a post Linear delivers: in_rowlin[b] added to its output, as_dense[b] stored into `dense`
  bool in_rowlin[OCC4D_MAX_BLOCKS + 2] = {}, as_dense[OCC4D_MAX_BLOCKS + 2] = {};
  for (int j = 0; P.linz && j < nC; ++j) {
    const int b = in.cross_after[j] + 1;
    if (b >= nB || !in.post_rows_ok[j]) continue;
    in_rowlin[b] = true;
    const bool cross_behind_b = j + 1 < nC && in.cross_after[j + 1] == b;
    if (b + 1 < nB && !cross_behind_b) as_dense[b + 1] = P.any_dense = true;
  }
  int next_cross = 0;
  for (int i = 0; i < nB;) {
    const auto cross_behind = [&](int b) { return next_cross < nC && in.cross_after[next_cross] == b; };
    int e = i;
    while (P.chain && e - i + 1 < CHAIN_BLOCKS && e + 1 < nB && !cross_behind(e)) ++e;
    Run& R = P.run[P.n_runs++];
    R.first = i; R.nb = e - i + 1;
    R.cross = cross_behind(e) ? next_cross++ : -1;
    if (P.chain && in.chain_tail && R.cross >= 0 && in.tail_ok[R.cross] && in.one_pass) R.n_tail = 2 * in.D[R.cross];
    const bool first = !in_rowlin[i] && !as_dense[i];
    for (int s = 0; s < 3; ++s) { R.slot_term[s] = -1; R.slot_rows[s] = ROWS_NONE; }
    for (int k = 0; k < CHAIN_BLOCKS; ++k) R.addrows[k] = ROWS_NONE;
    if (first) { R.slot_term[0] = i; R.slot_rows[0] = ROWS_X; }
    bool dense_free = P.any_dense && !as_dense[i + 1];     // (a post Linear's dense rows are consumed by the run behind it)
    int slots = 0;
    for (int k = i; k <= e; ++k) {
      if (as_dense[k + 1]) { R.addrows[k - i] = ROWS_DENSE; continue; }
      if (k == e) continue;
      const int rows = dense_free ? ROWS_DENSE : R.n_fresh++;
      dense_free = false;
      ++slots;
      R.slot_term[slots] = k + 1; R.slot_rows[slots] = rows; R.addrows[k - i] = rows;
    }
    R.pass = slots ? PASS_INTERP_DENSE : first ? PASS_INTERP_ADD : PASS_NONE;
    R.kernel = R.nb > 1 || R.n_tail ? K_CHAIN
               : in.f16block         ? K_F16_BLOCK
               : in.x6trunk          ? K_SPLIT_PAIR
               : !in.resblock        ? K_GENERIC_PAIR
               : in.trunk4           ? K_RESBLOCK4
               : R.addrows[0] != ROWS_NONE ? K_RESBLOCK_ADDROWS : K_RESBLOCK;
    R.post_add = R.cross >= 0 && in_rowlin[e + 1] ? e + 1 : -1;
    R.post_dense = R.post_add >= 0 && as_dense[e + 2] ? e + 2 : -1;
    i = e + 1;
  }
  return P;
}

}  // namespace occ4d_plan
