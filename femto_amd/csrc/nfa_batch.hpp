// nfa_batch.hpp -- the host side of a batch of automaton searches (regexp_search.hip) that is plain arithmetic on host data:
// the checks of an automaton, the flat upload form, the kernel's LDS plan, the order the automata are taken in, the arena of
// a pass, the clock of a pass and the way from raw result ranges to the caller's lists.  No HIP here: femto_amd_nfa_search_batch
// calls these between its device steps, and tests/nfa_batch_check.cpp runs them on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/femto_amd.h"
#include "device_tables.h"
#include "regexp_nfa.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NFA_BATCH_FN __host__ __device__ inline
#else
#define NFA_BATCH_FN inline
#endif

namespace femto_amd {

constexpr int kNfaMaxNodes = 2048;        // cost vectors of one automaton live in LDS
constexpr int kNfaDead = 255;             // MAX_NFA_ERRCNT (src/main/nfa.h:75)

struct NfaQueryDev {
  int64_t node_off;       // first node's flag byte (bit 0: start node, bit 1: final node)
  int64_t ent_off;        // first transition entry (sorted by character)
  int64_t bychar_off;     // this automaton's 262 by-character starts
  int32_t num_nodes, num_ents;
  int32_t cost_bound, subst, del, ins;
};
struct NfaResultDev {
  int64_t first, last;
  int32_t query, len, cost, pass;   // pass: the attempt that produced it (a search that ran out of stack is run again)
};
struct NfaHostResult { int64_t first, last; int32_t len, cost; int64_t seq; };

// bytes of a workgroup's dynamic LDS: nn nodes, cc children, ne transition entries in LDS (0: none), `group` rows of tmp_states
// (the layout: "Dynamic LDS of one workgroup" in regexp_search.hip)
constexpr int kNfaLdsEnts = 2048;
NFA_BATCH_FN size_t nfa_lds_bytes(int nn, int cc, int ne, int group) {
  return size_t(nn) * 4 + size_t(cc) * (8 + 8 + 4 + 4 + 4 + 4 + 4 + 2) + size_t(nn) * 3 + 16 + size_t(ne) * 6 + (ne ? size_t(nn) + 16 : 0) +
         (group ? size_t(group) * size_t(nn) * 4 + 16 : 0);
}

// ---- check ------------------------------------------------------------------------------------------------------------------
// what is wrong with an automaton, or null
inline const char* validate_nfa(const femto_amd_nfa_t& a) {
  if (a.num_nodes < 1 || a.num_nodes > kNfaMaxNodes) return "1 <= num_nodes <= 2048";
  if (a.num_transitions < 0 || int64_t(a.num_transitions) > kNfaMaxTransitions) return "too many transitions";
  if (!a.trans_start || !a.is_start || !a.is_final || (a.num_transitions && (!a.trans_char || !a.trans_dest))) return "null array";
  // regexp_settings_t as compile_regexp_from_ast accepts them (src/main/compile_regexp.c:673-685); errors are counted in one byte
  if (a.cost_bound < 1 || a.cost_bound > kNfaDead) return "1 <= cost_bound <= 255";
  if (a.subst_cost < 1 || a.subst_cost > kNfaDead || a.delete_cost < 1 || a.delete_cost > kNfaDead || a.insert_cost < 1 || a.insert_cost > kNfaDead)
    return "1 <= subst_cost, delete_cost, insert_cost <= 255";
  if (a.trans_start[0] != 0 || a.trans_start[a.num_nodes] != a.num_transitions) return "trans_start does not span the transitions";
  for (int i = 0; i < a.num_nodes; i++)
    if (a.trans_start[i + 1] < a.trans_start[i]) return "trans_start is not monotone";
  for (int e = 0; e < a.num_transitions; e++) {
    if (a.trans_char[e] < 0 || a.trans_char[e] >= kAlphaSize) return "transition character >= ALPHA_SIZE (261)";
    if (a.trans_dest[e] < 0 || a.trans_dest[e] >= a.num_nodes) return "transition destination out of range";
  }
  return nullptr;
}

// ---- flatten ----------------------------------------------------------------------------------------------------------------
// the automata of a batch, flat: transitions sorted by character (reading ch touches only its own entries), the source-node
// order kept inside a character
struct NfaFlat {
  std::vector<NfaQueryDev> hq;
  std::vector<uint8_t> flags;       // per node: bit 0 start, bit 1 final
  std::vector<uint32_t> ent_sd;     // source node | destination node << 16
  std::vector<uint16_t> ent_ch;
  std::vector<int32_t> bychar;      // [nq][262]: where every character's entries start (within the automaton)
  int max_nodes = 1;
  size_t max_ents = 0;
};
// (the arrays are locals of the loop and handed over at the end: filled through the returned struct, 20 000 motifs took 9.5 ms
// instead of 8.8)
inline NfaFlat nfa_flatten(const femto_amd_nfa_t* nfas, int64_t nq) {
  std::vector<NfaQueryDev> hq(static_cast<size_t>(nq));
  std::vector<uint8_t> h_flags;
  std::vector<uint32_t> h_sd;
  std::vector<uint16_t> h_ch;
  std::vector<int32_t> h_bychar(size_t(nq) * 262);
  int max_nodes = 1;
  size_t max_ents = 0;
  for (int64_t qi = 0; qi < nq; qi++) {
    const femto_amd_nfa_t& a = nfas[qi];
    NfaQueryDev& Q = hq[size_t(qi)];
    Q.node_off = int64_t(h_flags.size());
    Q.ent_off = int64_t(h_sd.size());
    Q.bychar_off = qi * 262;
    Q.num_nodes = a.num_nodes;
    Q.num_ents = a.num_transitions;
    Q.cost_bound = a.cost_bound;
    Q.subst = a.subst_cost;
    Q.del = a.delete_cost;
    Q.ins = a.insert_cost;
    max_nodes = std::max(max_nodes, int(a.num_nodes));
    max_ents = std::max(max_ents, size_t(a.num_transitions));
    for (int i = 0; i < a.num_nodes; i++) h_flags.push_back(uint8_t((a.is_start[i] ? 1 : 0) | (a.is_final[i] ? 2 : 0)));
    int32_t* bc = h_bychar.data() + qi * 262;
    std::fill(bc, bc + 262, 0);
    for (int e = 0; e < a.num_transitions; e++) bc[a.trans_char[e] + 1]++;
    for (int c = 0; c < 261; c++) bc[c + 1] += bc[c];
    std::vector<int32_t> fill(bc, bc + 261);
    const size_t base = h_sd.size();
    h_sd.resize(base + size_t(a.num_transitions));
    h_ch.resize(base + size_t(a.num_transitions));
    for (int i = 0; i < a.num_nodes; i++)
      for (int e = a.trans_start[i]; e < a.trans_start[i + 1]; e++) {
        const int c = a.trans_char[e];
        const size_t at = base + size_t(fill[size_t(c)]++);
        h_sd[at] = uint32_t(i) | (uint32_t(a.trans_dest[e]) << 16);
        h_ch[at] = uint16_t(c);
      }
  }
  return {std::move(hq), std::move(h_flags), std::move(h_sd), std::move(h_ch), std::move(h_bychar), max_nodes, max_ents};
}

// ---- the kernel's LDS plan -----------------------------------------------------------------------------------------------------
// characters the text holds, from the index's C[]: the most children a pop can have
inline int nfa_text_chars(const std::vector<int64_t>& C) {
  int nchars = 0;
  for (int c = 0; c < kAlphaSize && size_t(c) + 1 < C.size(); c++)
    if (C[size_t(c) + 1] > C[size_t(c)]) nchars++;
  return nchars;
}
struct NfaLdsPlan {
  int32_t cost_stride;               // bytes of one stack entry's cost vector in the arena
  int32_t lds_nodes, lds_children;   // sizes of the workgroup's dynamic LDS arrays (nfa_lds_bytes)
  int32_t lds_ents;                  // > 0: every automaton's transitions and node flags are copied to LDS (room for this many entries)
  int32_t lds_group;                 // children merged together per round of the child phase
  int32_t lds_tc;                    // > 0: tmp_states of EVERY character of the text fit (this many characters): the by-character pass
  size_t bytes;                      // the launch's dynamic LDS
};
inline NfaLdsPlan nfa_lds_plan(int text_chars, int max_nodes, size_t max_ents) {
  NfaLdsPlan P;
  P.cost_stride = (max_nodes + 3) & ~3;
  P.lds_nodes = (max_nodes + 7) & ~7;
  P.lds_children = (std::max(text_chars, 4) + 3) & ~3;
  P.lds_ents = max_ents <= size_t(kNfaLdsEnts) ? int32_t((std::max<size_t>(max_ents, 2) + 1) & ~size_t(1)) : 0;
  P.lds_group = std::max(1, std::min({int(P.lds_children), 64, 16384 / (int(P.lds_nodes) * 4)}));
  // small alphabets and automata (DNA motifs: 5 characters x ~24 nodes): one row of tmp_states per character of the TEXT
  P.lds_tc = (text_chars <= 64 && text_chars <= P.lds_group && size_t(text_chars) * size_t(P.lds_nodes) * 4 <= 4096) ? text_chars : 0;
  P.bytes = nfa_lds_bytes(P.lds_nodes, P.lds_children, P.lds_ents, P.lds_group);
  return P;
}

// ---- order ------------------------------------------------------------------------------------------------------------------
// LONGEST-PREDICTED-FIRST.  The workgroups take automata off one counter, and the kernel lasts as long as its longest search
// (profiles/r05_regexp_final.txt: 156 k pops of a mean of 6.3 k) -- plus however long that search waited to be taken.  The
// order of the result lists is per automaton, not per batch, so the batch is handed out by falling predicted work: errors
// allowed x transitions (an automaton that accepts more strings branches more) x nodes.  A search taken at t = 0 ends the
// kernel at its own length; concurrent callers' kernels fill the workgroups the short searches leave.
inline void nfa_lpt_order(const std::vector<NfaQueryDev>& hq, std::vector<int32_t>& todo) {
  auto weight = [&](int32_t q) { const NfaQueryDev& Q = hq[size_t(q)]; return int64_t(Q.cost_bound) * int64_t(Q.num_ents) * int64_t(Q.num_nodes); };
  std::stable_sort(todo.begin(), todo.end(), [&](int32_t a, int32_t b) { return weight(a) > weight(b); });
}

// ---- the arena of a pass ----------------------------------------------------------------------------------------------------
// `ntodo` searches with stacks of `cap` entries: a fair share of the GPU's `slots` workgroups when `active_now` batches are in
// flight on the handle (see "FAIR SHARE" in the kernel), fewer when their arenas would not fit `budget` bytes
struct NfaArenaPlan {
  int blocks;
  int32_t hash_size;      // heads of the pending-range hash: a power of two >= 2 * cap
  size_t per_block;       // bytes of one workgroup's arena
};
inline NfaArenaPlan nfa_arena_plan(int64_t cap, int32_t cost_stride, int32_t slots, int active_now, size_t ntodo, size_t budget) {
  NfaArenaPlan A;
  A.blocks = int(std::min<int64_t>(int64_t(ntodo), (int64_t(slots) + active_now - 1) / active_now));
  int64_t hsize = 64;
  while (hsize < 2 * cap) hsize <<= 1;
  A.hash_size = int32_t(hsize);
  const size_t entry_bytes = 24 + size_t(cost_stride);      // first, last, match length, hash link, costs
  A.per_block = (size_t(cap) * entry_bytes + size_t(hsize) * 4 + 255) & ~size_t(255);
  if (size_t(A.blocks) * A.per_block > budget) A.blocks = int(std::max<size_t>(1, budget / A.per_block));
  return A;
}

// ---- the clock of a pass ----------------------------------------------------------------------------------------------------
// From the kernel's four words per automaton (it[q] entries popped | it[nq + q] shader cycles / 1024 | it[2 nq + q] start |
// it[3 nq + q] duration, the last two on the device's wall clock in units of 16 ticks) and the automata of the pass: pops, the
// span of the pass and how busy its workgroups were.  Starts are 32-bit counts: differences to one of them, as signed
// numbers, survive the wrap.  Times here are in those units, counted from the earliest start.
struct NfaPassClock {
  struct Search { int32_t q; int64_t start, run; };
  double pops = 0, pops_max = 0;      // entries popped: all searches, the largest one
  double busy = 0;                    // sum of the searches' durations
  int64_t span = 0;                   // the end of the search that ended last
  Search most = {0, 0, 0};            // the search with the most pops (the first of them in the order taken) ...
  Search last = {0, 0, 0};            // ... and the one that ended last
};
inline NfaPassClock nfa_pass_clock(const std::vector<int32_t>& it, int64_t nq, const std::vector<int32_t>& todo) {
  NfaPassClock K;
  if (todo.empty()) return K;
  const uint32_t ref = uint32_t(it[size_t(2 * nq + todo[0])]);
  auto start_of = [&](int32_t q) { return int64_t(int32_t(uint32_t(it[size_t(2 * nq + q)]) - ref)); };
  int64_t t0 = INT64_MAX, tend = INT64_MIN;
  for (int32_t q : todo) t0 = std::min(t0, start_of(q));
  K.pops_max = -1;
  for (int32_t q : todo) {
    const NfaPassClock::Search s = {q, start_of(q) - t0, int64_t(uint32_t(it[size_t(3 * nq + q)]))};
    K.busy += double(s.run);
    K.pops += double(it[size_t(q)]);
    if (double(it[size_t(q)]) > K.pops_max) { K.pops_max = double(it[size_t(q)]); K.most = s; }
    if (s.start + s.run > tend) { tend = s.start + s.run; K.last = s; }
  }
  K.span = tend;
  return K;
}
// what femto_amd_nfa_stats reports of a batch: its passes' clocks summed, in seconds
struct NfaBatchStats {
  double pops = 0, max = 0, busy = 0, span = 0, blocks = 0, late = 0;
  void add(const NfaPassClock& K, int pass, int blocks_now, double tick_s) {
    pops += K.pops;
    max = std::max(max, K.pops_max);
    busy += K.busy * tick_s;
    span += double(K.span) * tick_s;
    blocks = std::max(blocks, double(blocks_now));
    if (pass == 0) late = double(K.most.start) * tick_s;
  }
};

// ---- collect ----------------------------------------------------------------------------------------------------------------
// regexp_result_list_sort (src/main/server.c:1528-1573) of one automaton's raw results, in place: sort by first ascending, last
// descending; drop equal ranges (the one appended first stays: glibc's qsort is a stable merge sort) and ranges inside the
// last kept one; returns how many are kept
inline size_t sort_results(NfaHostResult* r, size_t count) {
  std::stable_sort(r, r + count, [](const NfaHostResult& a, const NfaHostResult& b) {
    if (a.first != b.first) return a.first < b.first;
    if (a.last != b.last) return a.last > b.last;
    return a.seq < b.seq;
  });
  size_t n = 0;
  for (size_t k = 0; k < count; k++) {
    if (n && r[k].first == r[n - 1].first && r[k].last == r[n - 1].last) continue;
    r[n++] = r[k];
  }
  if (n == 0) return 0;
  int64_t first = r[0].first, last = r[0].last;
  size_t i = 1;
  for (size_t k = 1; k < n; k++) {
    if (r[k].first >= first && r[k].last <= last) continue;
    first = r[k].first;
    last = r[k].last;
    r[i++] = r[k];
  }
  return i;
}
// The raw results grouped by automaton in one flat array (count, prefix, scatter): automaton qi's are flat[seg[qi] .. seg[qi + 1]),
// the first kept[qi] of them its list once sort() has run.  A search that was run again appended its earlier attempts'
// results too: only the last attempt's count; a search that ended with an error has none (the reference: RETURN_ERROR).
struct NfaLists {
  std::vector<int64_t> seg, kept;
  std::vector<NfaHostResult> flat;
  // every t-th automaton of nt: the handle's host threads share the work (2.98 M raw ranges of 20 000 APPROX 1 motifs took one
  // thread 167 ms -- a quarter of the call, next to 490 ms of search)
  void sort(int t, int nt) {
    for (size_t qi = size_t(t); qi < kept.size(); qi += size_t(nt)) kept[qi] = int64_t(sort_results(flat.data() + seg[qi], size_t(seg[qi + 1] - seg[qi])));
  }
};
inline NfaLists nfa_group_results(const std::vector<NfaResultDev>& raw, const std::vector<int32_t>& last_pass, const std::vector<int32_t>& status) {
  const size_t nq = status.size();
  auto counts = [&](const NfaResultDev& r) { return r.pass == last_pass[size_t(r.query)] && status[size_t(r.query)] == 0; };
  std::vector<int64_t> seg(nq + 1, 0);
  for (const NfaResultDev& r : raw)
    if (counts(r)) seg[size_t(r.query) + 1]++;
  for (size_t qi = 0; qi < nq; qi++) seg[qi + 1] += seg[qi];
  std::vector<NfaHostResult> flat(static_cast<size_t>(seg[nq]));
  std::vector<int64_t> at(seg.begin(), seg.end() - 1);
  for (size_t k = 0; k < raw.size(); k++)
    if (counts(raw[k])) flat[size_t(at[size_t(raw[k].query)]++)] = {raw[k].first, raw[k].last, raw[k].len, raw[k].cost, int64_t(k)};
  return {std::move(seg), std::vector<int64_t>(nq, 0), std::move(flat)};
}

// ---- deliver ----------------------------------------------------------------------------------------------------------------
// result_start[0 .. nq] from the kept counts; returns the total
inline int64_t nfa_result_starts(const NfaLists& L, int64_t* result_start) {
  int64_t n = 0;
  for (size_t qi = 0; qi < L.kept.size(); qi++) {
    result_start[qi] = n;
    n += L.kept[qi];
  }
  result_start[L.kept.size()] = n;
  return n;
}
inline void nfa_copy_results(const NfaLists& L, const int64_t* result_start, int64_t* first_out, int64_t* last_out, int32_t* len_out, int32_t* cost_out) {
  for (size_t qi = 0; qi < L.kept.size(); qi++) {
    const NfaHostResult* r = L.flat.data() + L.seg[qi];
    int64_t at = result_start[qi];
    for (int64_t k = 0; k < L.kept[qi]; k++, at++) {
      first_out[at] = r[k].first;
      last_out[at] = r[k].last;
      if (len_out) len_out[at] = r[k].len;
      if (cost_out) cost_out[at] = r[k].cost;
    }
  }
}

}  // namespace femto_amd
