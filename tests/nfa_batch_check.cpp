// nfa_batch_check.cpp -- femto_amd/csrc/nfa_batch.hpp on the CPU (tests/test_nfa_batch_plan.py builds this with
// -fsanitize=address,undefined and runs it): the host arithmetic of a batch of automaton searches -- the checks of an automaton,
// the flat form, the kernel's LDS plan, the order, the arena of a pass, the clock of a pass, and the way from raw ranges to the
// caller's lists.  Every expected value is worked out by hand from the formulas; the LDS tuples are those of
// tests/test_regexp_large.py::test_lds_plan_by_hand, here from the C++ itself.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../femto_amd/csrc/nfa_batch.hpp"

using namespace femto_amd;
typedef std::vector<int64_t> V64;
typedef std::vector<int32_t> V32;

#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// ---- the LDS plan ------------------------------------------------------------------------------------------------------------
static bool plan_is(int nchars, int nodes, size_t ents, int lds_nodes, int lds_children, int lds_group, int lds_tc, bool klds) {
  const NfaLdsPlan p = nfa_lds_plan(nchars, nodes, ents);
  return p.lds_nodes == lds_nodes && p.lds_children == lds_children && p.lds_group == lds_group && p.lds_tc == lds_tc && (p.lds_ents != 0) == klds &&
         p.bytes == nfa_lds_bytes(p.lds_nodes, p.lds_children, p.lds_ents, p.lds_group);
}
static int case_lds() {
  CHECK(plan_is(5, 16, 777, 16, 8, 8, 5, true));
  CHECK(plan_is(5, 200, 2048, 200, 8, 8, 5, true) && plan_is(5, 201, 2049, 208, 8, 8, 0, false));      // 5 * 208 * 4 = 4160 > 4096
  CHECK(plan_is(5, 816, 1, 816, 8, 5, 0, true) && plan_is(5, 817, 1, 824, 8, 4, 0, true));            // 4096 / 824 = 4 < 5
  CHECK(plan_is(5, 2041, 2040, 2048, 8, 2, 0, true) && plan_is(5, 2048, 2049, 2048, 8, 2, 0, false));
  CHECK(plan_is(94, 16, 777, 16, 96, 64, 0, true) && plan_is(94, 65, 1, 72, 96, 56, 0, true));
  CHECK(plan_is(94, 1001, 1, 1008, 96, 4, 0, true) && plan_is(257, 2041, 1, 2048, 260, 2, 0, true));
  CHECK(plan_is(4, 256, 1, 256, 4, 4, 4, true) && plan_is(4, 257, 1, 264, 4, 4, 0, true));            // the text_chars * N * 4 <= 4096 edge
  CHECK(plan_is(64, 16, 1, 16, 64, 64, 64, true) && plan_is(65, 16, 1, 16, 68, 64, 0, true));
  CHECK(plan_is(3, 1, 0, 8, 4, 4, 3, true));
  const NfaLdsPlan a = nfa_lds_plan(5, 16, 777), b = nfa_lds_plan(3, 1, 0), c = nfa_lds_plan(5, 201, 2049), d = nfa_lds_plan(5, 200, 2048);
  CHECK(a.cost_stride == 16 && a.lds_ents == 778 && b.cost_stride == 4 && b.lds_ents == 2 && c.cost_stride == 204 && c.lds_ents == 0 && d.lds_ents == 2048);
  // 64 + 8 * 38 + 48 + 16 + 778 * 6 + 32 + (8 * 16 * 4 + 16)
  CHECK(a.bytes == 64 + 304 + 48 + 16 + 4668 + 32 + 528);
  // the most a launch can ask for: 8192 + 264 * 38 + 6144 + 16 + 12288 + 2064 + 16400, with the kernel's static arrays (4232 bytes)
  // and the dynamic array's alignment under the 65536 of one workgroup
  CHECK(nfa_lds_bytes(2048, 264, 2048, 2) == 55136);
  size_t worst = 0;
  const int nchars[] = {1, 5, 64, 65, 94, 257, 261};
  const size_t ents[] = {0, 2047, 2048, 2049, size_t(1) << 22};
  for (int nc : nchars)
    for (int nodes = 1; nodes <= 2048; nodes = nodes == 2045 ? 2048 : nodes + 7)      // 1, 8, ..., 2045, 2048
      for (size_t ne : ents) {
        const NfaLdsPlan p = nfa_lds_plan(nc, nodes, ne);
        worst = std::max(worst, p.bytes);
        CHECK(p.lds_group * p.lds_nodes * 4 <= 16384 || p.lds_group == 1);
      }
  CHECK(worst == 55136 && worst + 4232 + 16 <= 65536);
  V64 C(262, 0);                       // characters 2, 70 and 260 occur
  for (int ch = 0; ch < 261; ch++) C[size_t(ch) + 1] = C[size_t(ch)] + (ch == 2 ? 3 : ch == 70 ? 1 : ch == 260 ? 9 : 0);
  CHECK(nfa_text_chars(C) == 3 && nfa_text_chars(V64({0, 0, 4})) == 1 && nfa_text_chars(V64()) == 0);
  return 0;
}

// ---- flattening ---------------------------------------------------------------------------------------------------------------
static femto_amd_nfa_t nfa_of(const V32& ts, const V32& tc, const V32& td, const std::vector<uint8_t>& st, const std::vector<uint8_t>& fi) {
  femto_amd_nfa_t a;
  std::memset(&a, 0, sizeof a);
  a.num_nodes = int32_t(st.size());
  a.num_transitions = int32_t(tc.size());
  a.trans_start = ts.data();
  a.trans_char = tc.empty() ? nullptr : tc.data();
  a.trans_dest = td.empty() ? nullptr : td.data();
  a.is_start = st.data();
  a.is_final = fi.data();
  a.cost_bound = a.subst_cost = a.delete_cost = a.insert_cost = 1;
  return a;
}
static int case_flatten() {
  const V32 ts0 = {0, 0, 0}, none;
  const std::vector<uint8_t> st0 = {1, 0}, fi0 = {0, 1};
  // node 0: 260 -> 1, 7 -> 2; node 1: 0 -> 2, 7 -> 0; node 2: 7 -> 1
  const V32 ts1 = {0, 2, 4, 5}, tc1 = {260, 7, 0, 7, 7}, td1 = {1, 2, 2, 0, 1};
  const std::vector<uint8_t> st1 = {7, 0, 0}, fi1 = {0, 0, 1};
  const V32 ts2 = {0, 1}, tc2 = {5}, td2 = {0};
  const std::vector<uint8_t> st2 = {1}, fi2 = {1};
  femto_amd_nfa_t in[3] = {nfa_of(ts0, none, none, st0, fi0), nfa_of(ts1, tc1, td1, st1, fi1), nfa_of(ts2, tc2, td2, st2, fi2)};
  in[1].cost_bound = 3, in[1].subst_cost = 2, in[1].delete_cost = 4, in[1].insert_cost = 5;
  for (const femto_amd_nfa_t& a : in) CHECK(validate_nfa(a) == nullptr);
  const NfaFlat F = nfa_flatten(in, 3);
  CHECK(F.hq.size() == 3 && F.max_nodes == 3 && F.max_ents == 5 && F.bychar.size() == 3 * 262);
  CHECK(F.hq[0].node_off == 0 && F.hq[0].ent_off == 0 && F.hq[0].bychar_off == 0 && F.hq[0].num_nodes == 2 && F.hq[0].num_ents == 0);
  CHECK(F.hq[1].node_off == 2 && F.hq[1].ent_off == 0 && F.hq[1].bychar_off == 262 && F.hq[1].num_nodes == 3 && F.hq[1].num_ents == 5);
  CHECK(F.hq[1].cost_bound == 3 && F.hq[1].subst == 2 && F.hq[1].del == 4 && F.hq[1].ins == 5);
  CHECK(F.hq[2].node_off == 5 && F.hq[2].ent_off == 5 && F.hq[2].bychar_off == 524 && F.hq[2].num_nodes == 1 && F.hq[2].num_ents == 1);
  CHECK(F.flags == std::vector<uint8_t>({1, 2, 1, 0, 2, 3}));
  // by character, the source-node order kept inside character 7
  CHECK(F.ent_ch == std::vector<uint16_t>({0, 7, 7, 7, 260, 5}));
  CHECK(F.ent_sd == std::vector<uint32_t>({1u | 2u << 16, 0u | 2u << 16, 1u | 0u << 16, 2u | 1u << 16, 0u | 1u << 16, 0u}));
  for (int c = 0; c <= 261; c++) {
    CHECK(F.bychar[size_t(c)] == 0);
    CHECK(F.bychar[262 + size_t(c)] == (c == 0 ? 0 : c <= 7 ? 1 : c <= 260 ? 4 : 5));
    CHECK(F.bychar[524 + size_t(c)] == (c <= 5 ? 0 : 1));
  }
  CHECK(F.bychar[262 + 261] == in[1].num_transitions && F.bychar[524 + 261] == in[2].num_transitions);
  const NfaFlat E = nfa_flatten(in, 1);      // a batch without a transition
  CHECK(E.max_nodes == 2 && E.max_ents == 0 && E.ent_sd.empty() && E.ent_ch.empty() && E.flags.size() == 2);
  return 0;
}

// ---- validation ---------------------------------------------------------------------------------------------------------------
static bool refused(const femto_amd_nfa_t& a, const char* why) {
  const char* got = validate_nfa(a);
  return got && !std::strcmp(got, why);
}
static int case_validate() {
  const V32 ts = {0, 1, 2, 2}, tc = {0, 260}, td = {1, 2};
  const std::vector<uint8_t> st = {1, 0, 0}, fi = {0, 0, 1};
  const femto_amd_nfa_t ok = nfa_of(ts, tc, td, st, fi);
  CHECK(validate_nfa(ok) == nullptr);
  femto_amd_nfa_t a = ok;
  a.num_nodes = 0;
  CHECK(refused(a, "1 <= num_nodes <= 2048"));
  a.num_nodes = 2049;
  CHECK(refused(a, "1 <= num_nodes <= 2048"));
  a = ok, a.num_transitions = -1;
  CHECK(refused(a, "too many transitions"));
  a.num_transitions = (1 << 22) + 1;
  CHECK(refused(a, "too many transitions"));
  a = ok, a.trans_start = nullptr;
  CHECK(refused(a, "null array"));
  a = ok, a.is_start = nullptr;
  CHECK(refused(a, "null array"));
  a = ok, a.is_final = nullptr;
  CHECK(refused(a, "null array"));
  a = ok, a.trans_char = nullptr;
  CHECK(refused(a, "null array"));
  a = ok, a.trans_dest = nullptr;
  CHECK(refused(a, "null array"));
  a = ok, a.cost_bound = 0;
  CHECK(refused(a, "1 <= cost_bound <= 255"));
  a.cost_bound = 256;
  CHECK(refused(a, "1 <= cost_bound <= 255"));
  a = ok, a.subst_cost = 0;
  CHECK(refused(a, "1 <= subst_cost, delete_cost, insert_cost <= 255"));
  a = ok, a.delete_cost = 256;
  CHECK(refused(a, "1 <= subst_cost, delete_cost, insert_cost <= 255"));
  a = ok, a.insert_cost = 0;
  CHECK(refused(a, "1 <= subst_cost, delete_cost, insert_cost <= 255"));
  const V32 ts_first = {1, 1, 2, 2}, ts_end = {0, 1, 2, 3}, ts_down = {0, 2, 1, 2};
  a = ok, a.trans_start = ts_first.data();
  CHECK(refused(a, "trans_start does not span the transitions"));
  a.trans_start = ts_end.data();
  CHECK(refused(a, "trans_start does not span the transitions"));
  a.trans_start = ts_down.data();
  CHECK(refused(a, "trans_start is not monotone"));
  const V32 tc_low = {-1, 260}, tc_high = {0, 261}, td_low = {1, -1}, td_high = {3, 2};
  a = ok, a.trans_char = tc_low.data();
  CHECK(refused(a, "transition character >= ALPHA_SIZE (261)"));
  a.trans_char = tc_high.data();
  CHECK(refused(a, "transition character >= ALPHA_SIZE (261)"));
  a = ok, a.trans_dest = td_low.data();
  CHECK(refused(a, "transition destination out of range"));
  a.trans_dest = td_high.data();
  CHECK(refused(a, "transition destination out of range"));
  // the accepted edges
  a = ok, a.cost_bound = 255, a.subst_cost = 255, a.delete_cost = 255, a.insert_cost = 255;
  CHECK(validate_nfa(a) == nullptr);
  const V32 one_ts = {0, 0}, none, big_ts(2049, 0);
  const std::vector<uint8_t> one = {1}, big(2048, 0);
  CHECK(validate_nfa(nfa_of(one_ts, none, none, one, one)) == nullptr);
  CHECK(validate_nfa(nfa_of(big_ts, none, none, big, big)) == nullptr);
  return 0;
}

// ---- order ------------------------------------------------------------------------------------------------------------------
static int case_lpt() {
  std::vector<NfaQueryDev> hq(5);
  const int32_t cne[5][3] = {{1, 2, 3}, {2, 3, 1}, {1, 10, 10}, {3, 1, 2}, {9, 0, 9}};      // weights 6, 6, 100, 6, 0
  for (int q = 0; q < 5; q++) {
    hq[size_t(q)] = NfaQueryDev();
    hq[size_t(q)].cost_bound = cne[q][0], hq[size_t(q)].num_ents = cne[q][1], hq[size_t(q)].num_nodes = cne[q][2];
  }
  V32 up = {0, 1, 2, 3, 4}, down = {4, 3, 2, 1, 0}, none;
  nfa_lpt_order(hq, up);
  nfa_lpt_order(hq, down);
  nfa_lpt_order(hq, none);
  CHECK(up == V32({2, 0, 1, 3, 4}) && down == V32({2, 3, 1, 0, 4}) && none.empty());      // equal weights keep their order
  hq[0].cost_bound = 255, hq[0].num_ents = 1 << 22, hq[0].num_nodes = 2048;               // 2.2e12: no 32-bit product
  hq[2].cost_bound = 1, hq[2].num_ents = 1 << 22, hq[2].num_nodes = 2048;
  nfa_lpt_order(hq, up);
  CHECK(up == V32({0, 2, 1, 3, 4}));
  return 0;
}

// ---- the arena of a pass ----------------------------------------------------------------------------------------------------
static int case_arena() {
  const size_t big = size_t(16) << 30;
  NfaArenaPlan a = nfa_arena_plan(1024, 16, 2048, 1, 5000, big);
  CHECK(a.blocks == 2048 && a.hash_size == 2048 && a.per_block == 1024 * 40 + 2048 * 4);      // 49152, a multiple of 256
  a = nfa_arena_plan(1025, 16, 2048, 1, 5000, big);
  CHECK(a.blocks == 2048 && a.hash_size == 4096 && a.per_block == 57600);                      // 41000 + 16384 = 57384, rounded up
  a = nfa_arena_plan(1, 4, 2048, 1, 5000, big);
  CHECK(a.hash_size == 64 && a.per_block == 512);                                              // 28 + 256
  CHECK(nfa_arena_plan(1024, 16, 2048, 1, 5000, 1000).blocks == 1);                            // less than one block's arena
  CHECK(nfa_arena_plan(1024, 16, 2048, 1, 5000, 3 * 49152 + 100).blocks == 3);
  CHECK(nfa_arena_plan(1024, 16, 2048, 1, 5000, 2048 * size_t(49152)).blocks == 2048);
  CHECK(nfa_arena_plan(1024, 16, 2048, 1, 5000, 2048 * size_t(49152) - 1).blocks == 2047);
  CHECK(nfa_arena_plan(1024, 16, 2048, 3, 5000, big).blocks == 683);                           // (2048 + 2) / 3
  CHECK(nfa_arena_plan(1024, 16, 10, 3, 5000, big).blocks == 4 && nfa_arena_plan(1024, 16, 10, 1, 5000, big).blocks == 10);
  CHECK(nfa_arena_plan(1024, 16, 2048, 1, 7, big).blocks == 7 && nfa_arena_plan(1024, 16, 2048, 3, 7, big).blocks == 7);
  return 0;
}

// ---- the clock of a pass ----------------------------------------------------------------------------------------------------
static int case_clock() {
  // three automata taken in the order 2, 0, 1; starts either side of the 32-bit wrap.  Counted from the earliest (automaton 1):
  // automaton 1 starts at 0 and runs 120, automaton 2 starts at 16 and runs 100, automaton 0 starts at 48 and runs 50
  const V32 it = {9, 9, 7,   11, 12, 13,   0x00000010, int32_t(0xffffffe0u), int32_t(0xfffffff0u),   50, 120, 100};
  const V32 todo = {2, 0, 1};
  const NfaPassClock k = nfa_pass_clock(it, 3, todo);
  CHECK(k.pops == 25 && k.pops_max == 9 && k.busy == 270 && k.span == 120);
  CHECK(k.last.q == 1 && k.last.start == 0 && k.last.run == 120);
  CHECK(k.most.q == 0 && k.most.start == 48 && k.most.run == 50);      // 0 and 1 popped 9 each: 0 was taken first
  const NfaPassClock one = nfa_pass_clock(it, 3, V32({2}));           // a later pass: one automaton of the three
  CHECK(one.pops == 7 && one.pops_max == 7 && one.busy == 100 && one.span == 100 && one.last.q == 2 && one.most.q == 2 && one.most.start == 0);
  const V32 tie = {1, 1, 1,   0, 0, 0,   5, 15, 25,   40, 30, 20};      // all end at 45: the first taken is "last"
  const NfaPassClock t = nfa_pass_clock(tie, 3, V32({1, 0, 2}));
  CHECK(t.span == 40 && t.last.q == 1 && t.last.start == 10 && t.most.q == 1 && t.busy == 90);
  const V32 longrun = {4, 0, 0, int32_t(0x90000000u)};                  // a duration past 2^31 ticks is unsigned
  CHECK(nfa_pass_clock(longrun, 1, V32({0})).span == int64_t(0x90000000u));
  const NfaPassClock none = nfa_pass_clock(it, 3, V32());
  CHECK(none.pops == 0 && none.pops_max == 0 && none.busy == 0 && none.span == 0);
  NfaBatchStats s;
  s.add(k, 0, 200, 0.5);
  CHECK(s.pops == 25 && s.max == 9 && s.busy == 135 && s.span == 60 && s.blocks == 200 && s.late == 24);
  s.add(one, 1, 1, 0.5);                                                // passes add up; the late start is the first pass's
  CHECK(s.pops == 32 && s.max == 9 && s.busy == 185 && s.span == 110 && s.blocks == 200 && s.late == 24);
  return 0;
}

// ---- from raw ranges to the caller's lists ------------------------------------------------------------------------------------
static int case_lists() {
  // automaton 1 was run twice (its pass 0 ranges do not count), automaton 2 ended with an error, automaton 3 found nothing
  const V32 last_pass = {0, 1, 0, 0}, status = {0, 0, 5, 0};
  const std::vector<NfaResultDev> raw = {
      {10, 20, 1, 9, 9, 0},      // 0: an earlier pass of automaton 1
      {5, 9, 0, 3, 0, 0},        // 1
      {10, 20, 1, 4, 1, 1},      // 2: inside (10, 25)
      {1, 2, 2, 1, 0, 0},        // 3: automaton 2's status is not 0
      {5, 9, 0, 7, 1, 0},        // 4: the same range as 1, appended later
      {6, 8, 0, 2, 0, 0},        // 5: inside (5, 9)
      {2, 4, 0, 1, 0, 0},        // 6
      {10, 25, 1, 5, 0, 1},      // 7
      {9, 12, 0, 6, 2, 0},       // 8: starts inside (5, 9), ends after it
      {30, 31, 1, 8, 3, 1},      // 9
  };
  NfaLists one = nfa_group_results(raw, last_pass, status), three = nfa_group_results(raw, last_pass, status);
  CHECK(one.seg == V64({0, 5, 8, 8, 8}) && one.flat.size() == 8 && one.kept == V64({0, 0, 0, 0}));
  CHECK(one.flat[0].seq == 1 && one.flat[1].seq == 4 && one.flat[4].seq == 8 && one.flat[5].seq == 2 && one.flat[7].seq == 9);
  one.sort(0, 1);
  for (int t = 0; t < 3; t++) three.sort(t, 3);
  CHECK(one.kept == V64({3, 2, 0, 0}) && three.kept == one.kept);
  V64 start(5, -1), first(5, -1), last(5, -1), start3(5, -1), first3(5, -1), last3(5, -1);
  V32 len(5, -1), cost(5, -1);
  CHECK(nfa_result_starts(one, start.data()) == 5 && nfa_result_starts(three, start3.data()) == 5);
  CHECK(start == V64({0, 3, 5, 5, 5}) && start3 == start);
  nfa_copy_results(one, start.data(), first.data(), last.data(), len.data(), cost.data());
  nfa_copy_results(three, start3.data(), first3.data(), last3.data(), nullptr, nullptr);
  CHECK(first == V64({2, 5, 9, 10, 30}) && last == V64({4, 9, 12, 25, 31}) && first3 == first && last3 == last);
  CHECK(len == V32({1, 3, 6, 5, 8}) && cost == V32({0, 0, 2, 0, 3}));      // of the equal ranges the one appended first
  NfaLists none = nfa_group_results(std::vector<NfaResultDev>(), last_pass, status);
  none.sort(0, 1);
  CHECK(none.flat.empty() && none.kept == V64({0, 0, 0, 0}) && nfa_result_starts(none, start.data()) == 0 && start == V64({0, 0, 0, 0, 0}));
  return 0;
}

int main() {
  if (case_lds() || case_flatten() || case_validate() || case_lpt() || case_arena() || case_clock() || case_lists()) return 1;
  std::printf("nfa_batch ok\n");
  return 0;
}
