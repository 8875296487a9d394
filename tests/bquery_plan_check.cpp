// bquery_plan_check.cpp -- femto_amd/bquery/bquery_plan.hpp on the CPU (tests/test_bquery_plan.py builds this with
// -fsanitize=address,undefined and runs it): the forest, the range table and the level schedule of a batch of boolean trees.
// Trees come from query text through BqParser; the leaves' row counts are given as a leaf_starts array.  Small cases are pinned
// to values derived by hand from the arithmetic of run_batch; the 2 048-leaf chain and random trees are checked for the
// invariants that keep one call of the schedule from writing over another.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../femto_amd/bquery/bquery_plan.hpp"

using namespace femto_amd;
typedef std::vector<int64_t> V64;
typedef std::vector<int32_t> V32;

#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static bool parse(const std::string& text, BqTree* t, bool* type_error = nullptr) {
  std::string err;
  bool te = false;
  *t = BqTree();
  const bool ok = BqParser(reinterpret_cast<const uint8_t*>(text.data()), int64_t(text.size())).parse(t, &err, &te);
  if (type_error) *type_error = te;
  else if (!ok) std::printf("parse \"%.60s\": %s\n", text.c_str(), err.c_str());
  return ok;
}

static V64 starts_of(const V64& rows) {
  V64 s(1, 0);
  for (int64_t r : rows) s.push_back(s.back() + r);
  return s;
}

static int64_t rows_below(const BqForest& f, int g, const V64& ls) {      // the bound, restated
  const BqForest::Node& n = f.nodes[size_t(g)];
  if (n.op == BQ_LEAF) return ls[size_t(n.leaf) + 1] - ls[size_t(n.leaf)];
  const int64_t l = rows_below(f, n.left, ls), r = rows_below(f, n.right, ls);
  return n.op == BQ_AND ? std::min(l, r) : n.op == BQ_NOT ? l : l + r;
}

// what must hold of every schedule
static int invariants(const BqForest& f, const V64& ls, const BqSchedule& s) {
  const size_t G = f.nodes.size(), J = s.job_node.size();
  const int64_t rows = ls[f.node_of_leaf.size()];
  CHECK(ls.size() == f.node_of_leaf.size() + 1);
  CHECK(s.job_left.size() == J && s.job_right.size() == J && s.job_op.size() == J && s.job_dist.size() == J);
  CHECK(s.calls[0].size() == size_t(f.height) + 1 && s.calls[1].size() == size_t(f.height) + 1);
  std::vector<int> jobs_of(G, 0), under_and_not(G, 0);
  std::vector<char> done(G, 0);
  size_t operators = 0;
  for (size_t g = 0; g < G; g++) {
    const BqForest::Node& n = f.nodes[g];
    if (n.op == BQ_LEAF) { done[g] = 1; continue; }
    operators++;
    if (n.op == BQ_AND || n.op == BQ_NOT) under_and_not[size_t(n.left)] = under_and_not[size_t(n.right)] = 1;
  }
  CHECK(J == operators);
  int64_t doc_at = rows, pair_at = rows, slot = 0, at = 0, widest = 1;
  for (int h = 0; h <= f.height; h++)
    for (int fam = 0; fam < 2; fam++) {
      const BqCall& c = s.calls[fam][size_t(h)];
      CHECK(c.n >= 0 && (h > 0 || c.n == 0));
      if (!c.n) continue;
      CHECK(c.begin == at);                                         // the calls tile the job arrays in schedule order
      at += c.n;
      widest = std::max(widest, c.n);
      int64_t bound = 0;
      bool to_documents = false;
      for (int64_t j = c.begin; j < c.begin + c.n; j++) {
        const int32_t g = s.job_node[size_t(j)];
        CHECK(g >= 0 && size_t(g) < G);
        const BqForest::Node& n = f.nodes[size_t(g)];
        const bool pairs = n.op == BQ_THEN || n.op == BQ_WITHIN || (n.op == BQ_OR && n.type == BQ_PAIRS);
        CHECK(n.op != BQ_LEAF && n.height == h && pairs == (fam == 1));
        CHECK(s.job_left[size_t(j)] == n.left && s.job_right[size_t(j)] == n.right && s.job_dist[size_t(j)] == n.distance);
        CHECK(s.job_op[size_t(j)] == (n.op == BQ_AND ? FEMTO_AMD_DOCSET_AND : n.op == BQ_NOT ? FEMTO_AMD_DOCSET_NOT : n.op == BQ_THEN ? FEMTO_AMD_DOCPOS_THEN :
                                      n.op == BQ_WITHIN ? FEMTO_AMD_DOCPOS_WITHIN : pairs ? FEMTO_AMD_DOCPOS_OR : FEMTO_AMD_DOCSET_OR));
        CHECK(done[size_t(n.left)] && done[size_t(n.right)]);      // both operands belong to an earlier call
        jobs_of[size_t(g)]++;
        bound += rows_below(f, g, ls);
        if (pairs && under_and_not[size_t(g)]) to_documents = true;
      }
      for (int64_t j = c.begin; j < c.begin + c.n; j++) done[size_t(s.job_node[size_t(j)])] = 1;
      CHECK(c.bound == bound && c.to_documents == to_documents);
      CHECK(c.tot == slot);
      slot += to_documents ? 2 : 1;
      if (fam) {                                                    // each slice starts where the one before it in its arena ends
        CHECK(c.pair_at == pair_at);
        pair_at += c.bound;
      }
      if (!fam || to_documents) {
        CHECK(c.doc_at == doc_at);
        doc_at += c.bound;
      }
    }
  for (size_t g = 0; g < G; g++) CHECK(jobs_of[g] == (f.nodes[g].op == BQ_LEAF ? 0 : 1));      // every operator node is exactly one job
  CHECK(at == int64_t(J) && s.max_jobs == widest);
  CHECK(doc_at == s.doc_cap && pair_at == s.pair_cap);             // the last slice ends at the arena's capacity
  CHECK(slot == s.ncalls);                                          // non-empty calls plus read-as-documents calls
  return 0;
}

static const char* kA = "(a THEN 5 b) AND (c OR d) NOT e";
static const char* kB = "a THEN 3 b OR (c WITHIN 2 d)";

static int case_a() {
  BqTree t;
  CHECK(parse(kA, &t));
  CHECK(t.nodes.size() == 9 && t.nodes[2].op == BQ_THEN && t.nodes[5].op == BQ_OR && t.nodes[6].op == BQ_AND && t.nodes[8].op == BQ_NOT);
  BqForest f;
  CHECK(f.append(t));
  CHECK(f.height == 3 && f.node_of_leaf == V32({0, 1, 3, 4, 7}) && f.root == V32({8}) && f.rtype == V32({BQ_DOCUMENTS}));
  const V64 ls = starts_of({3, 4, 5, 6, 7});
  const BqSchedule s = bq_schedule(f, ls);
  CHECK(!invariants(f, ls, s));
  CHECK(s.job_node == V32({5, 2, 6, 8}) && s.job_left == V32({3, 0, 2, 6}) && s.job_right == V32({4, 1, 5, 7}));
  CHECK(s.job_op == V32({FEMTO_AMD_DOCSET_OR, FEMTO_AMD_DOCPOS_THEN, FEMTO_AMD_DOCSET_AND, FEMTO_AMD_DOCSET_NOT}) && s.job_dist == V32({0, 5, 0, 0}));
  CHECK(s.ncalls == 5 && s.max_jobs == 1 && s.doc_cap == 57 && s.pair_cap == 32);
  const BqCall &o = s.calls[0][1], &th = s.calls[1][1], &an = s.calls[0][2], &no = s.calls[0][3];
  CHECK(o.n == 1 && o.bound == 11 && o.doc_at == 25 && o.tot == 0 && !o.to_documents);
  CHECK(th.n == 1 && th.bound == 7 && th.pair_at == 25 && th.doc_at == 36 && th.tot == 1 && th.to_documents);
  CHECK(an.n == 1 && an.bound == 7 && an.doc_at == 43 && an.tot == 3);
  CHECK(no.n == 1 && no.bound == 7 && no.doc_at == 50 && no.tot == 4);
  CHECK(s.calls[1][2].n == 0 && s.calls[1][3].n == 0);
  return 0;
}

static int case_b() {
  BqTree t;
  CHECK(parse(kB, &t));
  BqForest f;
  CHECK(f.append(t));
  CHECK(f.nodes.size() == 7 && f.height == 2 && f.nodes[6].op == BQ_OR && f.rtype == V32({BQ_PAIRS}));
  const V64 ls = starts_of({2, 3, 4, 5});
  const BqSchedule s = bq_schedule(f, ls);
  CHECK(!invariants(f, ls, s));
  CHECK(s.job_node == V32({2, 5, 6}) && s.job_op == V32({FEMTO_AMD_DOCPOS_THEN, FEMTO_AMD_DOCPOS_WITHIN, FEMTO_AMD_DOCPOS_OR}) && s.job_dist == V32({3, 2, 0}));
  CHECK(s.calls[0][1].n == 0 && s.calls[0][2].n == 0);             // the OR of pairs is positional
  CHECK(s.calls[1][1].n == 2 && s.calls[1][1].bound == 14 && s.calls[1][1].pair_at == 14 && s.calls[1][2].n == 1 && s.calls[1][2].pair_at == 28);
  CHECK(!s.calls[1][1].to_documents && !s.calls[1][2].to_documents);
  CHECK(s.doc_cap == 14 && s.pair_cap == 42 && s.ncalls == 2 && s.max_jobs == 2);
  return 0;
}

static int case_c() {
  BqTree t;
  CHECK(parse("a", &t));
  BqForest one, none;
  CHECK(one.append(t));
  for (const BqForest* f : {&one, &none}) {
    const V64 ls = starts_of(f == &one ? V64({9}) : V64());
    const BqSchedule s = bq_schedule(*f, ls);
    CHECK(!invariants(*f, ls, s));
    CHECK(f->height == 0 && s.job_node.empty() && s.ncalls == 0 && s.max_jobs == 1 && s.doc_cap == ls.back() && s.pair_cap == ls.back());
  }
  CHECK(one.root == V32({0}) && one.node_of_leaf == V32({0}) && none.nodes.empty() && none.root.empty());
  return 0;
}

static int case_d() {
  BqTree a, b;
  CHECK(parse(kA, &a) && parse(kB, &b));
  BqForest f;
  CHECK(f.append(a) && f.append(b));
  CHECK(f.nodes.size() == 16 && f.height == 3 && f.root == V32({8, 15}) && f.rtype == V32({BQ_DOCUMENTS, BQ_PAIRS}));
  CHECK(f.node_of_leaf == V32({0, 1, 3, 4, 7, 9, 10, 12, 13}));
  CHECK(f.nodes[11].left == 9 && f.nodes[11].right == 10 && f.nodes[9].leaf == 5 && f.nodes[13].leaf == 8 && f.nodes[15].left == 11 && f.nodes[15].right == 14);
  const V64 ls = starts_of({3, 4, 5, 6, 7, 2, 3, 4, 5});
  const BqSchedule s = bq_schedule(f, ls);
  CHECK(!invariants(f, ls, s));
  CHECK(s.job_node == V32({5, 2, 11, 14, 6, 15, 8}));              // equal heights of both trees share one call
  const BqCall& p1 = s.calls[1][1];
  CHECK(s.calls[0][1].n == 1 && s.calls[0][1].doc_at == 39 && p1.n == 3 && p1.bound == 21 && p1.to_documents && p1.pair_at == 39 && p1.doc_at == 50 && p1.tot == 1);
  CHECK(s.calls[0][2].doc_at == 71 && s.calls[0][2].tot == 3 && s.calls[1][2].pair_at == 60 && s.calls[1][2].tot == 4 && s.calls[0][3].doc_at == 78);
  CHECK(s.ncalls == 6 && s.max_jobs == 3 && s.doc_cap == 85 && s.pair_cap == 74);
  return 0;
}

static int case_e() {
  const uint16_t x[] = {7, 8, 9}, y[] = {11};
  const int64_t first[] = {10, 20, 30}, last[] = {12, 25, 30};
  BqRangeTable r;
  r.literal_leaf(x, 3);
  r.automaton_leaf(first, last, 3);
  r.automaton_leaf(nullptr, nullptr, 0);
  r.literal_leaf(y, 1);
  CHECK(r.leaf_range == V64({0, 1, 4, 4, 5}) && r.lit_of == V32({0, -1, -1, -1, 1}) && r.leaf_of == V32({0, 1, 1, 1, 3}));
  CHECK(r.first == V64({0, 10, 20, 30, 0}) && r.last == V64({-1, 12, 25, 30, -1}));
  CHECK(r.lit_plen == V32({3, 1}) && r.lit_starts == V64({0, 3}) && r.lit_syms == std::vector<uint16_t>({7, 8, 9, 11}));
  BqRangeTable none;
  CHECK(none.leaf_range == V64({0}) && none.first.empty());
  return 0;
}

// a random tree of n leaves as query text: left-associative, a right operand that is an operator in parentheses
static std::string random_text(std::mt19937& rng, int n) {
  if (n == 1) return std::string(1, char('a' + rng() % 26));
  static const char* ops[] = {"AND", "OR", "NOT", "THEN 4", "WITHIN 9"};
  const int k = 1 + int(rng() % unsigned(n - 1));
  const std::string op = ops[rng() % 5], l = random_text(rng, k), r = random_text(rng, n - k);
  return l + " " + op + " " + (n - k > 1 ? "(" + r + ")" : r);
}

static int case_f() {
  std::mt19937 rng(20261018);
  std::string chain = "w";                                         // 2 048 leaves, 2 047 levels: the per-tree limit
  static const char* ops[] = {" AND w", " OR w", " NOT w"};
  for (int i = 1; i < (kBqMaxNodes + 1) / 2; i++) chain += ops[i % 3];
  BqTree t;
  CHECK(parse(chain, &t));
  CHECK(t.nodes.size() == size_t(kBqMaxNodes) && t.nodes.back().height == kBqMaxNodes / 2);
  bool te = false;
  CHECK(!parse(chain + " AND w", &t, &te) && !te);                 // one more is refused by the parser
  CHECK(parse(chain, &t));
  BqForest f, all;
  CHECK(f.append(t));
  V64 rows;
  for (size_t l = 0; l < f.node_of_leaf.size(); l++) rows.push_back(int64_t(rng() % 5));
  CHECK(!invariants(f, starts_of(rows), bq_schedule(f, starts_of(rows))));
  rows.clear();
  for (int k = 0; k < 400; k++) {                                  // each tree alone, and all of them as one batch
    bool type_error = true;
    while (type_error) {
      const bool ok = parse(random_text(rng, 1 + int(rng() % 9)), &t, &type_error);
      CHECK(ok || type_error);
    }
    BqForest one;
    CHECK(one.append(t) && all.append(t));
    V64 r1;
    for (size_t l = 0; l < t.leaves.size(); l++) r1.push_back(rng() % 4 ? int64_t(rng() % 300) : 0);
    rows.insert(rows.end(), r1.begin(), r1.end());
    CHECK(!invariants(one, starts_of(r1), bq_schedule(one, starts_of(r1))));
  }
  CHECK(all.root.size() == 400 && all.node_of_leaf.size() == rows.size());
  CHECK(!invariants(all, starts_of(rows), bq_schedule(all, starts_of(rows))));
  return 0;
}

int main() {
  if (case_a() || case_b() || case_c() || case_d() || case_e() || case_f()) return 1;
  std::printf("bquery_plan ok\n");
  return 0;
}
