// The lane-adjacency relation of the shield's classification (decentral_layer.py:23-39 is_adj_lane) and the "relation word"
// a pose's owner publishes for relate_word() in mm_kernels.hip.  Plain C++17 without device calls, so that a host compiler can
// build the same table for tests/test_relation_word_host.py (MM_HD is empty there).
#pragma once
#include "../../include/mm_abi.h"

#ifdef __HIPCC__
#define MM_HD __host__ __device__ __forceinline__
#else
#define MM_HD inline
#endif

// is_adj_lane(vehicle, lane2) given vehicle.lane and its next_lane.  Only road (b,c) has two lanes, so "same road and ids
// differ by one" means the pair {bc0, bc1}: bc0 sees bc1 at -1 (to its right), bc1 sees bc0 at +1.
MM_HD constexpr int adj_pair(int l1, int l2) {
  return (l1 == MM_LANE_BC0 && l2 == MM_LANE_BC1) ? -1 : ((l1 == MM_LANE_BC1 && l2 == MM_LANE_BC0) ? 1 : 0);
}
MM_HD constexpr int adj_lane(int l1, int nl1, int l2) {
  const int f = adj_pair(l1, l2);
  return f != 0 ? f : adj_pair(nl1, l2);
}
// The same relation as 2-bit codes (0: none, 1: +1, 3: -1) in packed 6-entry tables, for the classification
// loops (one table build per ego instead of four compare chains per pair):
//   adj_row(l1) >> 2*l2 & 3 = code of adj_pair(l1, l2);   adj_col(l2) >> 2*l1 & 3 = code of adj_pair(l1, l2)
MM_HD constexpr unsigned adj_row(int l1) { return l1 == MM_LANE_BC0 ? (3u << (2 * MM_LANE_BC1)) : (l1 == MM_LANE_BC1 ? (1u << (2 * MM_LANE_BC0)) : 0u); }
MM_HD constexpr unsigned adj_col(int l2) { return l2 == MM_LANE_BC1 ? (3u << (2 * MM_LANE_BC0)) : (l2 == MM_LANE_BC0 ? (1u << (2 * MM_LANE_BC1)) : 0u); }
// v_a = adj_lane(elane, enl, olane) and a_v = adj_lane(olane, onl, elane) as relate() forms them from the packed tables
MM_HD constexpr unsigned adj_va_code(int elane, int enl, int olane) {
  // row of elane, entries it leaves empty filled from the row of enl
  const unsigned rowE = adj_row(elane), rowN = adj_row(enl);
  const unsigned nzE = (rowE | rowE >> 1) & 0x555u;
  const unsigned rowEN = rowE | (rowN & ~(nzE * 3u));
  return (rowEN >> (2 * olane)) & 3u;
}
MM_HD constexpr unsigned adj_av_code(int elane, int olane, int onl) {
  const unsigned colE = adj_col(elane);
  const unsigned g1 = (colE >> (2 * olane)) & 3u, g2 = (colE >> (2 * onl)) & 3u;
  return g1 != 0 ? g1 : g2;
}

// ---- relation word (MM_RELATION_WORD) ----------------------------------------------------------------------------------------
// road.py:67-109 next_lane admits eight (lane, next lane) pairs only -- (ab0,bc0) (ab0,bc1) (bc0,cd0) (bc1,cd0) (cd0,cd0) (jk0,kb0)
// (kb0,bc0) (kb0,bc1) -- and what relate() derives from the lanes of a reader e and of a partner's pose o depends on the two
// pairs alone.  pair_index numbers them 0 .. 7: the lane itself, and 6 / 7 for ab0 / kb0 heading for bc1.
constexpr int kRelPairs = 8;
MM_HD constexpr int pair_index(int lane, int nl) {
  return lane + (((nl == MM_LANE_BC1) & ((lane == MM_LANE_AB0) | (lane == MM_LANE_KB0))) ? 6 - (lane & 4) : 0);
}
constexpr int kRelPairLane[kRelPairs] = {MM_LANE_AB0, MM_LANE_BC0, MM_LANE_BC1, MM_LANE_CD0, MM_LANE_JK0, MM_LANE_KB0, MM_LANE_AB0, MM_LANE_KB0};
constexpr int kRelPairNext[kRelPairs] = {MM_LANE_BC0, MM_LANE_CD0, MM_LANE_CD0, MM_LANE_CD0, MM_LANE_KB0, MM_LANE_BC0, MM_LANE_BC1, MM_LANE_BC1};
// The word of a pose with pair o: for every reader pair e, bit 2e = "adjacent either way" ((v_a | a_v) != 0) and bit 2e + 1 =
// "the left front corner is the relevant one" (v_a == -1 or a_v == 1), from the expressions above.
MM_HD constexpr unsigned rel_word(int o) {
  unsigned w = 0;
  for (int e = 0; e < kRelPairs; e++) {
    const unsigned va_c = adj_va_code(kRelPairLane[e], kRelPairNext[e], kRelPairLane[o]);
    const unsigned av_c = adj_av_code(kRelPairLane[e], kRelPairLane[o], kRelPairNext[o]);
    w |= (((va_c | av_c) != 0) ? 1u : 0u) << (2 * e) | (((va_c == 3u) | (av_c == 1u)) ? 2u : 0u) << (2 * e);
  }
  return w;
}
struct RelTable { unsigned w[kRelPairs]; };
MM_HD constexpr RelTable rel_table() {
  RelTable t{};
  for (int o = 0; o < kRelPairs; o++) t.w[o] = rel_word(o);
  return t;
}
constexpr RelTable kRelTable = rel_table();
// The word rides in bits 11 .. 26 of the pose code (bits 0 .. 10: lane, next lane, corner bits, present mark, heading bits).
constexpr int kRelShift = 11;
// What the owner of a pose evaluates: the word depends on the lane where that is bc0 / bc1 (their next lane, cd0, adds
// nothing) and on the next lane where the lane is ab0 / kb0; cd0 and jk0 are adjacent to nothing.  Two selects each instead of
// an indexed load; rel_checks() below holds it to the table.
MM_HD constexpr int pose_relw(int lane, int nl) {
  const unsigned by_lane = lane == MM_LANE_BC0 ? kRelTable.w[pair_index(MM_LANE_BC0, MM_LANE_CD0)]
                                               : (lane == MM_LANE_BC1 ? kRelTable.w[pair_index(MM_LANE_BC1, MM_LANE_CD0)] : 0u);
  const unsigned by_next = nl == MM_LANE_BC0 ? kRelTable.w[pair_index(MM_LANE_AB0, MM_LANE_BC0)]
                                             : (nl == MM_LANE_BC1 ? kRelTable.w[pair_index(MM_LANE_AB0, MM_LANE_BC1)] : 0u);
  return (int)((by_lane | by_next) << kRelShift);
}
MM_HD constexpr bool rel_checks() {
  for (int o = 0; o < kRelPairs; o++) {
    if (pair_index(kRelPairLane[o], kRelPairNext[o]) != o) return false;
    if (kRelTable.w[o] >> 16) return false;
    if ((unsigned)pose_relw(kRelPairLane[o], kRelPairNext[o]) != kRelTable.w[o] << kRelShift) return false;
    for (int e = 0; e < kRelPairs; e++) {
      // against the packed-table expressions relate() evaluates, and against is_adj_lane's compare chains
      const unsigned va_c = adj_va_code(kRelPairLane[e], kRelPairNext[e], kRelPairLane[o]);
      const unsigned av_c = adj_av_code(kRelPairLane[e], kRelPairLane[o], kRelPairNext[o]);
      const int v_a = adj_lane(kRelPairLane[e], kRelPairNext[e], kRelPairLane[o]);
      const int a_v = adj_lane(kRelPairLane[o], kRelPairNext[o], kRelPairLane[e]);
      if (va_c != (v_a == 0 ? 0u : (v_a == 1 ? 1u : 3u)) || av_c != (a_v == 0 ? 0u : (a_v == 1 ? 1u : 3u))) return false;
      const unsigned bits = (kRelTable.w[o] >> (2 * e)) & 3u;
      if (((bits & 1u) != 0) != ((va_c | av_c) != 0)) return false;
      if (((bits & 2u) != 0) != ((va_c == 3u) | (av_c == 1u))) return false;
    }
  }
  return true;
}
static_assert(rel_checks(), "relation word: the table, pair_index or pose_relw drifted from adj_row / adj_col / adj_lane");
