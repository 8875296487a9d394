// bquery_plan.hpp -- the host plan of a batch of boolean trees (bquery.hip runs it): the FOREST the trees are merged into, the
// RANGE TABLE of its leaves and the level SCHEDULE with every call's place in the two arenas.  Plain C++ over BqTree: no HIP, no
// handle, no error text (a failure is a bool and the caller words it), so tests/bquery_plan_check.cpp checks all of it on the
// CPU.  DESIGN.md "Boolean queries: the level schedule" states the layout this arithmetic keeps.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/femto_amd.h"
#include "bquery_parser.hpp"

namespace femto_amd {

// ---- the batch as one forest: global node and leaf numbers ----------------------------------------------------------------------

struct BqForest {
  struct Node { int op, distance, left, right, leaf, type, height; };
  std::vector<Node> nodes;                      // postfix per tree, the trees in query order
  std::vector<int32_t> node_of_leaf, root, rtype;
  int height = 0;
  // false: the forest would reach 2^30 nodes (nothing is appended)
  bool append(const BqTree& t) {
    const int nbase = int(nodes.size()), lbase = int(node_of_leaf.size());
    if (nodes.size() + t.nodes.size() >= (size_t(1) << 30)) return false;
    for (const BqNode& n : t.nodes) {
      if (n.op == BQ_LEAF) node_of_leaf.push_back(int32_t(nodes.size()));
      height = std::max(height, n.height);
      nodes.push_back({n.op, n.distance, n.left < 0 ? -1 : n.left + nbase, n.right < 0 ? -1 : n.right + nbase, n.leaf < 0 ? -1 : n.leaf + lbase, n.type, n.height});
    }
    root.push_back(int32_t(nodes.size()) - 1);
    rtype.push_back(t.nodes.back().type);
    return true;
  }
};

// ---- the range table: leaf l's ranges are [leaf_range[l], leaf_range[l + 1]) -----------------------------------------------------

struct BqRangeTable {
  std::vector<int64_t> leaf_range{0}, first, last;   // a literal's range is filled in on the device, from the count
  std::vector<int32_t> lit_of, leaf_of;              // per range: its literal (-1: an automaton's range), its leaf
  std::vector<int32_t> lit_plen;                     // the literal batch, in leaf order
  std::vector<int64_t> lit_starts;
  std::vector<uint16_t> lit_syms;
  void literal_leaf(const uint16_t* syms, int64_t n) {
    lit_plen.push_back(int32_t(n));
    lit_starts.push_back(int64_t(lit_syms.size()));
    lit_syms.insert(lit_syms.end(), syms, syms + n);
    range(int32_t(lit_plen.size()) - 1, 0, -1);
    leaf_range.push_back(int64_t(first.size()));
  }
  void automaton_leaf(const int64_t* f, const int64_t* l, int64_t n) {     // its n result ranges
    for (int64_t r = 0; r < n; r++) range(-1, f[r], l[r]);
    leaf_range.push_back(int64_t(first.size()));
  }

 private:
  void range(int32_t lit, int64_t f, int64_t l) {
    lit_of.push_back(lit);
    leaf_of.push_back(int32_t(leaf_range.size()) - 1);
    first.push_back(f);
    last.push_back(l);
  }
};

// ---- the schedule: jobs by height and family, each call's bound and place, the arenas' sizes -------------------------------------

// one (level, family) of the schedule: jobs [begin, begin + n) of the job arrays
struct BqCall {
  int64_t begin = 0, n = 0;
  int64_t bound = 0;          // no more results than this
  bool to_documents = false;  // positional: an AND / NOT above reads some result of this call
  // where it writes.  Family 0: documents at doc_at.  Family 1: pairs at pair_at and, to_documents, their documents at doc_at
  // (slot tot + 1 of the totals array).  Every slice is `bound` long and no two calls share one.
  int64_t doc_at = 0, pair_at = 0, tot = 0;
};

struct BqSchedule {
  std::vector<int32_t> job_node, job_left, job_right, job_op, job_dist;
  std::vector<BqCall> calls[2];                 // [family][height]: 0 AND / OR / NOT of documents, 1 THEN / WITHIN / OR of pairs
  int64_t doc_cap = 0, pair_cap = 0;            // the arenas: the leaves' rows, then the calls' slices in schedule order
  int64_t max_jobs = 1, ncalls = 0;             // ncalls: slots of the totals array in use
};

// leaf l has leaf_starts[l + 1] - leaf_starts[l] rows.  No result holds more entries than the leaves below it have rows (AND: the
// shorter side; NOT: the left side), so every call's slice is known before anything runs.
inline BqSchedule bq_schedule(const BqForest& f, const std::vector<int64_t>& leaf_starts) {
  const size_t G = f.nodes.size();
  std::vector<int64_t> bound(G, 0);
  std::vector<uint8_t> read_as_documents(G, 0);       // a pair-typed node under AND / NOT
  for (size_t g = 0; g < G; g++) {
    const BqForest::Node& n = f.nodes[g];
    if (n.op == BQ_LEAF) bound[g] = leaf_starts[size_t(n.leaf) + 1] - leaf_starts[size_t(n.leaf)];
    else if (n.op == BQ_AND) bound[g] = std::min(bound[size_t(n.left)], bound[size_t(n.right)]);
    else if (n.op == BQ_NOT) bound[g] = bound[size_t(n.left)];
    else bound[g] = bound[size_t(n.left)] + bound[size_t(n.right)];
    if (n.op == BQ_AND || n.op == BQ_NOT)
      for (int c : {n.left, n.right})
        if (f.nodes[size_t(c)].type == BQ_PAIRS) read_as_documents[size_t(c)] = 1;
  }
  auto positional = [](const BqForest::Node& n) { return n.op == BQ_THEN || n.op == BQ_WITHIN || (n.op == BQ_OR && n.type == BQ_PAIRS); };
  std::vector<std::vector<int32_t>> by_level[2];
  by_level[0].resize(size_t(f.height) + 1);
  by_level[1].resize(size_t(f.height) + 1);
  for (size_t g = 0; g < G; g++)
    if (f.nodes[g].op != BQ_LEAF) by_level[positional(f.nodes[g]) ? 1 : 0][size_t(f.nodes[g].height)].push_back(int32_t(g));
  BqSchedule s;
  s.calls[0].resize(size_t(f.height) + 1);
  s.calls[1].resize(size_t(f.height) + 1);
  s.doc_cap = s.pair_cap = leaf_starts[f.node_of_leaf.size()];
  for (int h = 1; h <= f.height; h++)
    for (int fam = 0; fam < 2; fam++) {
      BqCall& c = s.calls[fam][size_t(h)];
      c.begin = int64_t(s.job_node.size());
      for (int32_t g : by_level[fam][size_t(h)]) {
        const BqForest::Node& n = f.nodes[size_t(g)];
        s.job_node.push_back(g);
        s.job_left.push_back(n.left);
        s.job_right.push_back(n.right);
        s.job_op.push_back(fam ? (n.op == BQ_THEN ? FEMTO_AMD_DOCPOS_THEN : n.op == BQ_WITHIN ? FEMTO_AMD_DOCPOS_WITHIN : FEMTO_AMD_DOCPOS_OR)
                               : (n.op == BQ_AND ? FEMTO_AMD_DOCSET_AND : n.op == BQ_NOT ? FEMTO_AMD_DOCSET_NOT : FEMTO_AMD_DOCSET_OR));
        s.job_dist.push_back(n.distance);
        c.bound += bound[size_t(g)];
        if (fam && read_as_documents[size_t(g)]) c.to_documents = true;
      }
      c.n = int64_t(s.job_node.size()) - c.begin;
      if (!c.n) continue;
      s.max_jobs = std::max(s.max_jobs, c.n);
      c.doc_at = s.doc_cap;
      c.pair_at = s.pair_cap;
      c.tot = s.ncalls;
      s.ncalls += fam && c.to_documents ? 2 : 1;
      if (fam) s.pair_cap += c.bound;
      if (!fam || c.to_documents) s.doc_cap += c.bound;
    }
  return s;
}

}  // namespace femto_amd
