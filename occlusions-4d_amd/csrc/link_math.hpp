// The components of two frames linked (include/ext/occ4d_link.h), shared WORD FOR WORD by the HIP kernels (csrc/link.hip) and the
// g++ twin (csrc_cpu/occ4d_twin.cpp): the member test, the open-addressing insert, the order relation of the match, the item bodies
// of the passes and the two argument contracts (host only).  Integers only.
//
// The bodies that other threads may run at the same time are templates over A, HOW THE ATOMIC IS SPELLED: relaxed, returning the
// value before -- agent scope on the work table and on the best-pair slots, workgroup scope on LDS, plain memory in the twin.
//   A::load64(p)  A::cas64(p, expected, desired)  A::load32(p)  A::cas32(p, expected, desired)  A::add32(p, v)  A::min32(p, v)
//   A::store32(p, v)
#pragma once
#include <stdint.h>

#include "ext/occ4d_link.h"
#include "frontend_math.hpp"      // OCC4D_HD; contract.hpp

namespace occ4d_link {

constexpr int PAIR_COLS = OCC4D_LINK_PAIR_COLS;
constexpr int TILE = OCC4D_LINK_TILE;
constexpr int64_t EMPTY = -1;                                     // a key is (a << 32) | b with a, b >= 0: never negative

// ---- the overlap
struct Table {                                                    // open addressing: `slots` a power of two, shift = 64 - log2(slots)
  int64_t* keys;
  int32_t *count, *root;
  int64_t slots;
  int shift;
};

struct OverlapArgs {
  const int32_t *labels_a, *labels_b;
  Table table;                                                    // work: 4 * slots
  int32_t *at;                                                    // work: n, the slot of the pair rooted at p, or -1
  int32_t *tile_pairs, *tile_members;                             // work: tiles each
  int64_t* pairs;
  int32_t* totals;
  int64_t n, tiles;
  int k_a, k_b, cap;
};

// the slots of the header's WORK formula
inline int64_t slots_for(int64_t n, int cap) {
  const int64_t want = 2 * (cap < n ? (int64_t)cap : n);
  int64_t slots = OCC4D_LINK_MIN_SLOTS;
  while (slots < want && slots < ((int64_t)1 << 31)) slots <<= 1;
  return slots;
}

// MEMBER: the point's key, or EMPTY.  The labels are tested before they become part of anything; with k_a == 0 or k_b == 0 they
// are not read (the pointers may be null).
OCC4D_HD int64_t key_of(const OverlapArgs& a, int64_t p) {
  if (a.k_a == 0 || a.k_b == 0) return EMPTY;
  const int32_t la = a.labels_a[p], lb = a.labels_b[p];
  if (la < 0 || la >= a.k_a || lb < 0 || lb >= a.k_b) return EMPTY;
  return ((int64_t)la << 32) | (int64_t)lb;
}

// where a key's probe sequence starts: reaches no output (nor does the order of the slots)
OCC4D_HD int64_t slot_of(const Table& t, int64_t key) { return (int64_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> t.shift); }

// `count` points of pair `key` with the lowest flat index `root` into the table: at most `probes` <= t.slots slots are looked at,
// linearly.  A slot belongs to a key for good once a compare-and-swap has put it there, so THE VALUE THE COMPARE-AND-SWAP RETURNS
// decides: EMPTY (ours now) or the key (another thread's insert of the same pair) -> add there; any other key -> the next slot.
// -> false when none of the `probes` slots took the key: with probes == slots that means slots other keys are in the table.
// The loop's bound is fixed before it starts; no thread waits for another.
template <class A>
OCC4D_HD bool insert(const Table& t, int64_t key, int32_t count, int32_t root, int64_t probes) {
  int64_t s = slot_of(t, key);
  for (int64_t i = 0; i < probes; ++i) {
    int64_t k = A::load64(t.keys + s);
    if (k == EMPTY) {
      k = A::cas64(t.keys + s, EMPTY, key);
      if (k == EMPTY) k = key;
    }
    if (k == key) {
      A::add32(t.count + s, count);
      A::min32(t.root + s, root);
      return true;
    }
    s = (s + 1) & (t.slots - 1);
  }
  return false;
}

OCC4D_HD void table_clear(const Table& t, int64_t s) {
  t.keys[s] = EMPTY;
  t.count[s] = 0;
  t.root[s] = INT32_MAX;
}

// pass 1, item i of max(slots, n): an empty table, no roots, the overflow word
OCC4D_HD void clear_item(const OverlapArgs& a, int64_t i) {
  if (i < a.table.slots) table_clear(a.table, i);
  if (i < a.n) a.at[i] = -1;
  if (i == 0) a.totals[2] = 0;
}

// pass 2: a run of `count` member points of one pair headed by p (the twin: every point a run of one)
template <class A>
OCC4D_HD void insert_item(const OverlapArgs& a, int64_t key, int32_t count, int64_t p) {
  if (!insert<A>(a.table, key, count, (int32_t)p, a.table.slots)) A::store32(a.totals + 2, 1);
}

// pass 3 (after a kernel boundary), slot s: a used slot's number to its root
OCC4D_HD void mark_item(const OverlapArgs& a, int64_t s) {
  if (a.table.keys[s] == EMPTY) return;
  const int32_t r = a.table.root[s];
  if (r >= 0 && r < a.n) a.at[r] = (int32_t)s;
}

// passes 4 to 6: the pairs numbered in the order of their roots by a tile prefix
OCC4D_HD bool is_pair_root(const OverlapArgs& a, int64_t p) { return a.at[p] >= 0; }

OCC4D_HD void pair_write(const OverlapArgs& a, int64_t p, int64_t i) {
  if (i < 0 || i >= a.cap) return;
  const int64_t s = a.at[p];
  if (s < 0 || s >= a.table.slots) return;
  const int64_t key = a.table.keys[s];
  int64_t* row = a.pairs + i * PAIR_COLS;
  row[0] = key >> 32;
  row[1] = key & 0xffffffffll;
  row[2] = a.table.count[s];
  row[3] = p;
}

// ---- the match
struct MatchArgs {
  const int64_t* pairs;
  const int32_t* totals;
  const int64_t *table_a, *table_b;
  int64_t ld_a, ld_b;
  const int32_t *track_a, *next_in;
  int32_t *link, *best_a, *next_out;
  int cap, k_a, k_b;
  uint32_t iou_num, iou_den;
  bool used;                                                      // k_a > 0, k_b > 0 and cap > 0: there may be pairs to read
};

// the rows of `pairs` that exist
OCC4D_HD int pair_rows(const MatchArgs& a) {
  if (!a.used || a.totals[2] != 0) return 0;
  const int t = a.totals[0];
  return t < a.cap ? (t < 0 ? 0 : t) : a.cap;
}

struct Pair {
  int64_t a, b;
  uint64_t count, uni;
  bool ok;                                                        // 0 <= a < k_a and 0 <= b < k_b: only then were the sizes read
};

OCC4D_HD Pair load_pair(const MatchArgs& m, int64_t i) {
  const int64_t* row = m.pairs + i * PAIR_COLS;
  Pair p{row[0], row[1], (uint64_t)row[2], 0, false};
  p.ok = p.a >= 0 && p.a < m.k_a && p.b >= 0 && p.b < m.k_b;
  if (p.ok) p.uni = (uint64_t)m.table_a[p.a * m.ld_a] + (uint64_t)m.table_b[p.b * m.ld_b] - p.count;
  return p;
}

// BEATS: the greater intersection over union, compared by cross-multiplication; a tie goes to the lower `tie` (a for a fixed b,
// b for a fixed a).  Two pairs of one b have different a, so on sizes within the contract this is a strict total order.
OCC4D_HD bool beats(const Pair& i, int64_t tie_i, const Pair& j, int64_t tie_j) {
  const uint64_t l = i.count * j.uni, r = j.count * i.uni;
  return l > r || (l == r && tie_i < tie_j);
}

// Raises the slot -- the index of the best pair so far, -1 for none -- to pair i if i beats what is there.  The slot only ever
// moves up the order: a failed compare-and-swap returns what another thread raised it to, and the comparison is repeated against
// that.  It can change at most `rows` times in all, which bounds the loop whatever the other threads do.
template <class A>
OCC4D_HD void best_update(const MatchArgs& m, int32_t* slot, int rows, int i, const Pair& me, bool for_b) {
  int cur = A::load32(slot);
  for (int round = 0; round <= rows; ++round) {
    if (cur >= 0) {
      if (cur >= rows) return;
      const Pair o = load_pair(m, cur);
      if (!o.ok || !beats(me, for_b ? me.a : me.b, o, for_b ? o.a : o.b)) return;
    }
    const int before = A::cas32(slot, cur, i);
    if (before == cur) return;
    cur = before;
  }
}

// pass 1, item k of max(k_a, k_b)
OCC4D_HD void init_item(const MatchArgs& m, int64_t k) {
  if (k < m.k_b) {
    int32_t* row = m.link + k * 4;
    row[0] = 0; row[1] = -1; row[2] = -1; row[3] = 0;
  }
  if (k < m.k_a) {
    m.best_a[k * 2] = -1;
    m.best_a[k * 2 + 1] = 0;
  }
}

// pass 2, pair i: link[b][2] and best_a[a][0] hold pair indices until passes 3 and 4
template <class A>
OCC4D_HD void best_item(const MatchArgs& m, int rows, int i) {
  const Pair me = load_pair(m, i);
  if (!me.ok) return;
  best_update<A>(m, m.link + me.b * 4 + 2, rows, i, me, true);
  best_update<A>(m, m.best_a + me.a * 2, rows, i, me, false);
}

// pass 3, component b of the later frame: its row but for the id of an unlinked one
OCC4D_HD void resolve_item(const MatchArgs& m, int rows, int64_t b) {
  int32_t* row = m.link + b * 4;
  const int j = row[2];
  row[0] = 0; row[1] = -1; row[2] = -1; row[3] = 0;
  if (j < 0 || j >= rows) return;
  const Pair p = load_pair(m, j);
  if (!p.ok) return;
  row[2] = (int32_t)p.a;
  row[3] = (int32_t)p.count;
  if (m.best_a[p.a * 2] == j && p.count * (uint64_t)m.iou_den >= (uint64_t)m.iou_num * p.uni) {
    row[0] = m.track_a[p.a];
    row[1] = (int32_t)p.a;
  }
}

// pass 4 (after a kernel boundary: pass 3 reads the pair indices), component a of the earlier frame
OCC4D_HD void finish_item(const MatchArgs& m, int rows, int64_t ka) {
  int32_t* row = m.best_a + ka * 2;
  const int j = row[0];
  row[0] = -1; row[1] = 0;
  if (j < 0 || j >= rows) return;
  const Pair p = load_pair(m, j);
  if (!p.ok) return;
  row[0] = (int32_t)p.b;
  row[1] = (int32_t)p.count;
}

// pass 5: the unlinked b take new ids in order
OCC4D_HD bool is_new(const MatchArgs& m, int64_t b) { return m.link[b * 4 + 1] < 0; }
OCC4D_HD void new_id(const MatchArgs& m, int64_t b, int32_t id) { m.link[b * 4] = id; }

struct Plain {                                                    // one thread: the twin
  static OCC4D_HD int64_t load64(const int64_t* p) { return *p; }
  static OCC4D_HD int64_t cas64(int64_t* p, int64_t expected, int64_t desired) {
    const int64_t before = *p;
    if (before == expected) *p = desired;
    return before;
  }
  static OCC4D_HD int32_t load32(const int32_t* p) { return *p; }
  static OCC4D_HD int32_t cas32(int32_t* p, int32_t expected, int32_t desired) {
    const int32_t before = *p;
    if (before == expected) *p = desired;
    return before;
  }
  static OCC4D_HD void add32(int32_t* p, int32_t v) { *p += v; }
  static OCC4D_HD void min32(int32_t* p, int32_t v) { if (v < *p) *p = v; }
  static OCC4D_HD void store32(int32_t* p, int32_t v) { *p = v; }
};

// ---- argument contracts (host): the status, `empty` = nothing to do, the arguments filled
inline int check_overlap(const int32_t* labels_a, const int32_t* labels_b, int k_a, int k_b, int64_t n, int32_t* work, int64_t* pairs,
                         int cap, int32_t* totals, bool& empty, OverlapArgs& a) {
  const char* who = "occ4d_link_overlap_i32";
  OCC4D_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld must be in [0, INT32_MAX]", who, (long long)n);
  OCC4D_REQUIRE(k_a >= 0 && k_b >= 0, "%s: k_a = %d, k_b = %d must be >= 0", who, k_a, k_b);
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  empty = n == 0;
  OCC4D_REQUIRE(empty || (work && totals), "%s: null work / totals with n = %lld", who, (long long)n);
  OCC4D_REQUIRE(empty || ((uintptr_t)work & 7) == 0, "%s: work must be 8-byte aligned", who);
  OCC4D_REQUIRE(empty || k_a == 0 || k_b == 0 || (labels_a && labels_b), "%s: null labels with n = %lld, k_a = %d, k_b = %d", who,
                (long long)n, k_a, k_b);
  OCC4D_REQUIRE(empty || cap == 0 || pairs, "%s: null pairs with cap = %d", who, cap);
  const int64_t slots = slots_for(n, cap), tiles = (n + TILE - 1) / TILE;
  int shift = 64;
  for (int64_t s = slots; s > 1; s >>= 1) --shift;
  int32_t* rest = work + 2 * slots;
  a = OverlapArgs{labels_a, labels_b, Table{(int64_t*)work, rest, rest + slots, slots, shift}, rest + 2 * slots, rest + 2 * slots + n,
                  rest + 2 * slots + n + tiles, pairs, totals, n, tiles, k_a, k_b, cap};
  return OCC4D_OK;
}

inline int check_match(const int64_t* pairs, const int32_t* totals, int cap, const int64_t* table_a, int64_t ld_a, const int64_t* table_b,
                       int64_t ld_b, int k_a, int k_b, const int32_t* track_a, int iou_num, int iou_den, const int32_t* next_in,
                       int32_t* link, int32_t* best_a, int32_t* next_out, MatchArgs& a) {
  const char* who = "occ4d_link_match_i32";
  OCC4D_REQUIRE(cap >= 0, "%s: cap = %d must be >= 0", who, cap);
  OCC4D_REQUIRE(k_a >= 0 && k_b >= 0, "%s: k_a = %d, k_b = %d must be >= 0", who, k_a, k_b);
  OCC4D_REQUIRE(iou_den >= 1 && iou_den <= OCC4D_LINK_MAX_DEN, "%s: iou_den = %d must be in [1, %d]", who, iou_den, OCC4D_LINK_MAX_DEN);
  OCC4D_REQUIRE(iou_num >= 0 && iou_num <= iou_den, "%s: iou_num = %d must be in [0, iou_den = %d]", who, iou_num, iou_den);
  const bool used = k_a > 0 && k_b > 0 && cap > 0;
  OCC4D_REQUIRE(!used || (pairs && totals), "%s: null pairs / totals with k_a = %d, k_b = %d, cap = %d", who, k_a, k_b, cap);
  OCC4D_REQUIRE(!used || (table_a && table_b && track_a), "%s: null table_a / table_b / track_a with k_a = %d, k_b = %d, cap = %d", who,
                k_a, k_b, cap);
  OCC4D_REQUIRE(!used || (ld_a >= 1 && ld_b >= 1), "%s: ld_a = %lld, ld_b = %lld must be >= 1", who, (long long)ld_a, (long long)ld_b);
  OCC4D_REQUIRE(k_b == 0 || link, "%s: null link with k_b = %d", who, k_b);
  OCC4D_REQUIRE(k_a == 0 || best_a, "%s: null best_a with k_a = %d", who, k_a);
  OCC4D_REQUIRE(next_in && next_out, "%s: null next_in / next_out", who);
  a = MatchArgs{pairs, totals, table_a, table_b, ld_a, ld_b, track_a, next_in, link, best_a, next_out, cap, k_a, k_b, (uint32_t)iou_num,
                (uint32_t)iou_den, used};
  return OCC4D_OK;
}

}  // namespace occ4d_link
