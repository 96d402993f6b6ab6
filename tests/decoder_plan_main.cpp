// Host program of tests/test_decoder_plan_host.py: csrc/decoder_plan.hpp alone, under plain g++.
//   (no argument)  every input of the enumeration below through plan_chunk and check(); prints "cases N", exit status 0, or the
//                  first plan that breaks an invariant and exit status 1
//   --layouts      one input per line of stdin (name nB nC cross_after.. flags penult k_local chain_tail one_pass resblock trunk4
//                  x6trunk f16block post_mask tail_mask): prints its plan, one line per run, and checks it too
#include <stdio.h>
#include <string.h>

#include "decoder_plan.hpp"

using namespace occ4d_plan;

static const char* rows_name(int where, char* buf) {
  if (where >= 0) { snprintf(buf, 16, "f%d", where); return buf; }
  return where == ROWS_X ? "x" : where == ROWS_DENSE ? "dense" : "-";
}

static void print_plan(const char* name, const ChunkPlan& P) {
  static const char* pass[] = {"none", "interp_add", "interp_dense"};
  static const char* kernel[] = {"chain", "f16_block", "split_pair", "resblock4", "resblock_addrows", "resblock", "generic_pair"};
  printf("%s: linz=%d chain=%d any_dense=%d runs=%d\n", name, P.linz, P.chain, P.any_dense, P.n_runs);
  for (int r = 0; r < P.n_runs; ++r) {
    const Run& R = P.run[r];
    char b[6][16];
    printf("  blocks %d+%d cross=%d tail=%d pass=%s slots=[%d>%s %d>%s %d>%s] fresh=%d addrows=[%s %s %s] kernel=%s post=[%d %d]\n",
           R.first, R.nb, R.cross, R.n_tail, pass[R.pass], R.slot_term[0], rows_name(R.slot_rows[0], b[0]), R.slot_term[1],
           rows_name(R.slot_rows[1], b[1]), R.slot_term[2], rows_name(R.slot_rows[2], b[2]), R.n_fresh,
           rows_name(R.addrows[0], b[3]), rows_name(R.addrows[1], b[4]), rows_name(R.addrows[2], b[5]), kernel[R.kernel],
           R.post_add, R.post_dense);
  }
}

static void print_inputs(const Inputs& in) {
  printf("nB=%d nC=%d cross_after=[", in.nB, in.nC);
  for (int j = 0; j < in.nC; ++j) printf("%d(post_rows_ok=%d tail_ok=%d) ", in.cross_after[j], in.post_rows_ok[j], in.tail_ok[j]);
  printf("] resblock=%d trunk4=%d x6trunk=%d f16block=%d flags=%d k_local=%d H=%d m=%d c=%d penult=%d chain_tail=%d one_pass=%d\n",
         in.resblock, in.trunk4, in.x6trunk, in.f16block, in.flags, in.k_local, in.H, in.m, in.c, in.penult_given, in.chain_tail,
         in.one_pass);
}

#define HOLD(cond)                         \
  do {                                     \
    if (!(cond)) return #cond;             \
  } while (0)

// The invariants of a plan (the header's last paragraph) -> nullptr, or the text of the first one that does not hold.
static const char* check(const Inputs& in, const ChunkPlan& P) {
  const int nB = in.nB;
  int delivered[OCC4D_MAX_BLOCKS + 2] = {};
  int dense = -1;                                // the term the chunk's dense buffer holds, unread
  int next = 0, next_cross = 0;
  HOLD(P.n_runs >= 1 && P.n_runs <= OCC4D_MAX_BLOCKS);
  HOLD(!P.chain || P.linz);
  HOLD(!P.linz || (in.resblock && !in.trunk4 && !in.x6trunk && !in.penult_given && in.k_local == 8 &&
                   !(in.flags & OCC4D_LINZ_PATH_STANDALONE)));
  HOLD(!(P.chain && (in.flags & OCC4D_CHAIN_PATH_SEPARATE)));
  for (int r = 0; r < P.n_runs; ++r) {
    const Run& R = P.run[r];
    const int last = R.first + R.nb - 1;
    // the runs tile the blocks in order; more than one block only in a chain, and with no cross layer inside
    HOLD(R.first == next && R.nb >= 1 && R.nb <= CHAIN_BLOCKS && last < nB);
    HOLD(R.nb == 1 || P.chain);
    for (int b = R.first; b < last; ++b) HOLD(!(next_cross < in.nC && in.cross_after[next_cross] == b));
    next = last + 1;
    // the cross layers in order, each behind the block cross_after names
    if (next_cross < in.nC && in.cross_after[next_cross] == last) HOLD(R.cross == next_cross++);
    else HOLD(R.cross == -1);
    // the tail: only behind a chain-eligible run with a cross layer behind it that allows it
    if (R.n_tail) {
      HOLD(P.chain && in.chain_tail && in.one_pass && R.cross >= 0 && in.tail_ok[R.cross]);
      HOLD(R.n_tail == 2 * in.D[R.cross] && R.kernel == K_CHAIN);
    }
    // the pass in front of the run
    int fresh[CHAIN_BLOCKS] = {-1, -1, -1};
    int n_slots = 0, n_fresh = 0;
    HOLD(R.n_fresh >= 0 && R.n_fresh < CHAIN_BLOCKS);
    for (int s = 0; s < 3; ++s) {
      const int t = R.slot_term[s], where = R.slot_rows[s];
      HOLD((t < 0) == (where == ROWS_NONE));
      if (t < 0) continue;
      ++n_slots;
      if (s == 0) {
        HOLD(t == R.first && where == ROWS_X);
        delivered[t] += 1;
        continue;
      }
      HOLD(R.slot_term[s - 1] >= 0 || s == 1);            // (slots 1, 2 are filled in order)
      HOLD(t > R.first && t <= last);
      if (where == ROWS_DENSE) {
        HOLD(P.any_dense && dense < 0);                    // never written while an earlier write is unread
        dense = t;
      } else {
        HOLD(where == n_fresh && where < R.n_fresh && fresh[where] < 0);     // fresh buffers in slot order
        fresh[n_fresh++] = t;
      }
    }
    HOLD(n_fresh == R.n_fresh && n_slots <= 3);
    HOLD(R.pass == (R.slot_term[1] >= 0 || R.slot_term[2] >= 0 ? PASS_INTERP_DENSE : R.slot_term[0] >= 0 ? PASS_INTERP_ADD : PASS_NONE));
    // the blocks: each reads the dense rows of the NEXT block's term, and only a kernel that adds rows has any
    for (int k = 0; k < CHAIN_BLOCKS; ++k) {
      const int where = R.addrows[k];
      if (where == ROWS_NONE) continue;
      HOLD(k < R.nb && (R.kernel == K_CHAIN || R.kernel == K_RESBLOCK_ADDROWS));
      HOLD(where == ROWS_DENSE || (where >= 0 && where < R.n_fresh));
      int& held = where == ROWS_DENSE ? dense : fresh[where];
      HOLD(held == R.first + k + 1);                       // never read before written, and read by exactly this block
      delivered[held] += 1;
      held = -1;
    }
    for (int k = 0; k < CHAIN_BLOCKS; ++k) HOLD(fresh[k] < 0);     // (the run's buffers are released behind it)
    // the block kernel
    if (R.kernel == K_CHAIN) HOLD(P.chain && (R.nb > 1 || R.n_tail));
    else
      HOLD(R.kernel == (in.f16block ? K_F16_BLOCK : in.x6trunk ? K_SPLIT_PAIR : !in.resblock ? K_GENERIC_PAIR : in.trunk4 ? K_RESBLOCK4
                        : R.addrows[0] != ROWS_NONE ? K_RESBLOCK_ADDROWS : K_RESBLOCK));
    // the cross layer's post Linear
    HOLD(R.post_add >= -1 && R.post_dense >= -1);
    if (R.post_add >= 0) {
      HOLD(P.linz && R.cross >= 0 && in.post_rows_ok[R.cross] && R.post_add == last + 1 && R.post_add < nB);
      delivered[R.post_add] += 1;
    }
    if (R.post_dense >= 0) {
      HOLD(R.post_add >= 0 && R.post_dense == last + 2 && R.post_dense < nB && P.any_dense && dense < 0);
      dense = R.post_dense;
    }
    if (!P.linz) HOLD(R.pass == PASS_INTERP_ADD && R.nb == 1 && R.n_tail == 0 && R.n_fresh == 0 && R.post_add < 0 && R.post_dense < 0);
  }
  HOLD(next == nB && next_cross == in.nC && dense < 0);
  HOLD(P.linz || (!P.chain && !P.any_dense));
  for (int t = 0; t < nB; ++t) HOLD(delivered[t] == 1);      // every term exactly once
  return nullptr;
}

static int run_one(const char* name, const Inputs& in, bool print) {
  const ChunkPlan P = plan_chunk(in);
  if (print) print_plan(name, P);
  const char* broken = check(in, P);
  if (!broken) return 0;
  printf("does not hold: %s\n", broken);
  print_inputs(in);
  print_plan(name, P);
  return 1;
}

static Inputs defaults() {
  Inputs in{};
  in.resblock = true;
  in.k_local = 8; in.H = 416; in.m = 40; in.c = 130;
  in.chain_tail = in.one_pass = true;
  for (int j = 0; j < OCC4D_MAX_CROSS; ++j) { in.D[j] = 416; in.post_rows_ok[j] = in.tail_ok[j] = true; }
  return in;
}

static int layouts() {
  char name[64];
  int failed = 0;
  for (;;) {
    Inputs in = defaults();
    if (scanf("%63s %d %d", name, &in.nB, &in.nC) != 3) break;
    if (in.nB < 1 || in.nB > OCC4D_MAX_BLOCKS || in.nC < 0 || in.nC > OCC4D_MAX_CROSS) return 2;
    for (int j = 0; j < in.nC; ++j)
      if (scanf("%d", &in.cross_after[j]) != 1) return 2;
    int v[11];
    for (int& x : v)
      if (scanf("%d", &x) != 1) return 2;
    in.flags = v[0]; in.penult_given = v[1]; in.k_local = v[2]; in.chain_tail = v[3]; in.one_pass = v[4];
    in.resblock = v[5]; in.trunk4 = v[6]; in.x6trunk = v[7]; in.f16block = v[8];
    for (int j = 0; j < in.nC; ++j) { in.post_rows_ok[j] = v[9] >> j & 1; in.tail_ok[j] = v[10] >> j & 1; }
    failed |= run_one(name, in, true);
  }
  return failed;
}

// nB 1..6 x every ascending cross_after of 0..min(4, nB) layers x post_rows_ok / tail_ok per layer x the six kernel families
// decoder_layout can produce x the two flag bits x penult x k_local {7, 8} x chain_tail x one_pass
static int enumerate() {
  static const bool family[6][4] = {{0, 0, 0, 0}, {0, 1, 0, 0}, {1, 1, 0, 0}, {1, 0, 0, 0}, {1, 0, 1, 0}, {1, 0, 1, 1}};
  long cases = 0;
  for (int nB = 1; nB <= 6; ++nB)
    for (int set = 0; set < 1 << nB; ++set) {
      Inputs in = defaults();
      in.nB = nB;
      for (int b = 0; b < nB; ++b)
        if (set >> b & 1) {
          if (in.nC < OCC4D_MAX_CROSS) in.cross_after[in.nC] = b;
          ++in.nC;
        }
      if (in.nC > OCC4D_MAX_CROSS) continue;
      for (int ok = 0; ok < 1 << (2 * in.nC); ++ok)
        for (const bool* f : family)
          for (int bits = 0; bits < 64; ++bits) {
            for (int j = 0; j < in.nC; ++j) { in.post_rows_ok[j] = ok >> (2 * j) & 1; in.tail_ok[j] = ok >> (2 * j + 1) & 1; }
            in.resblock = f[0]; in.trunk4 = f[1]; in.x6trunk = f[2]; in.f16block = f[3];
            in.flags = (bits & 1 ? OCC4D_LINZ_PATH_STANDALONE : 0) | (bits & 2 ? OCC4D_CHAIN_PATH_SEPARATE : 0);
            in.penult_given = bits & 4; in.k_local = bits & 8 ? 7 : 8; in.chain_tail = bits & 16; in.one_pass = bits & 32;
            if (run_one("enumeration", in, false)) return 1;
            ++cases;
          }
    }
  // the 2^30 bounds of the routed kernels' 32-bit row offsets: m nB H and c H, first value outside / last inside
  Inputs in = defaults();
  in.nB = 4; in.H = 512;
  const int edge[4][3] = {{1 << 19, 130, 0}, {(1 << 19) - 1, 130, 1}, {40, 1 << 21, 0}, {40, (1 << 21) - 1, 1}};
  for (const int* e : edge) {
    in.m = e[0]; in.c = e[1];
    if (plan_chunk(in).linz != (bool)e[2] || run_one("bounds", in, false)) {
      printf("m = %d, c = %d: linz expected %d\n", in.m, in.c, e[2]);
      return 1;
    }
  }
  printf("cases %ld\n", cases);
  return 0;
}

int main(int argc, char** argv) { return argc > 1 && !strcmp(argv[1], "--layouts") ? layouts() : enumerate(); }
