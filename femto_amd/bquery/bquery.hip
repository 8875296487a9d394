// bquery.hip -- boolean queries: a query text with AND OR NOT THEN WITHIN compiled to a typed tree (bquery_parser.hpp), and a
// BATCH of such trees evaluated as a few stream-ordered launches.  include/femto_amd.h "boolean queries" states the semantics;
// DESIGN.md "Boolean queries: the level schedule" the layout.
//
// The operators themselves are the library's own device calls (femto_amd_docset_device, femto_amd_docpos_device,
// femto_amd_docpos_documents_device), used as they are.  What is here is what lets ten thousand trees share them:
//   LEAVES.  Every leaf of every tree is one entry of a RANGE TABLE: a literal leaf has one range (all literal leaves are counted
//   by one femto_amd_count_device), an automaton leaf has its result ranges (all automata searched by one
//   femto_amd_nfa_search_batch).  bq_ranges / bq_clamp and two scans turn the table into clamped per-range row counts and
//   starts, and into one segment of rows per leaf; one femto_amd_locate_walk_device walks all of them into one buffer.
//   LISTING.  One femto_amd_doclist_device over the leaf segments gives every leaf's distinct documents and its rows as sorted
//   (document, offset) pairs.  The ranges of an automaton can overlap (APPROX, alternation), so one row can be located twice:
//   bq_unique (flag, scan, scatter, new starts) drops the repeats -- the reference's sort_dedup -- because the positional
//   operators take strictly ascending lists.
//   LEVELS.  Nodes are grouped by height.  All AND / OR / NOT nodes of one height are ONE femto_amd_docset_device call, all
//   THEN / WITHIN / OR-of-pairs nodes ONE femto_amd_docpos_device call.  A node's list is a view (start, n) into one of two
//   arenas (documents; pairs) kept in a device table: bq_bind fills the level's operand arrays from the table, bq_record writes
//   the results' views back, rebased by the arena offset of the level.  The results of a positional level that an AND / NOT
//   above it reads pass through femto_amd_docpos_documents_device, whole.
//   GATHER.  bq_gather copies the root views into the packed output, in query order.
// No result holds more entries than the leaves below it have rows, so once the leaves' row counts are on the host every level's
// place in the arenas is known: the batch costs TWO readbacks that the host waits for before it can go on -- the leaf segment
// starts (the row total) and the result starts -- and none per level.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "bquery_parser.hpp"

struct femto_amd_bquery {
  femto_amd::BqTree tree;
  std::vector<femto_amd_regexp_t*> leaves;     // one per tree.leaves
  std::string echo;
  ~femto_amd_bquery() {
    for (femto_amd_regexp_t* r : leaves) femto_amd_regexp_free(r);
  }
};

namespace femto_amd {
namespace {

// ---- leaves: range table -> clamped counts ------------------------------------------------------------------------------------

// range r of the table: a literal leaf's range comes from the count (lit_of[r] >= 0), an automaton's was uploaded
__global__ __launch_bounds__(256) void bq_ranges_kernel(int64_t nr, const int32_t* __restrict__ lit_of, const int64_t* __restrict__ lit_first,
                                                        const int64_t* __restrict__ lit_last, int64_t* __restrict__ first,
                                                        int64_t* __restrict__ last, int64_t* __restrict__ sizes) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= nr) return;
  const int32_t k = lit_of[r];
  int64_t f = first[r], l = last[r];
  if (k >= 0) {
    f = lit_first[k];
    l = lit_last[k];
  }
  if (l < f || f < 0) {      // the empty range
    f = 0;
    l = -1;
  }
  first[r] = f;
  last[r] = l;
  sizes[r] = l - f + 1;
}

// rows taken of range r: the leaf's ranges in order until max_occs rows are in; a leaf's FIRST range is clamped exactly as
// do_locate_query clamps a pattern (src/main/server.c:4405-4415, `last - first > max_occs`: a range of max_occs + 1 rows is kept whole)
__global__ __launch_bounds__(256) void bq_clamp_kernel(int64_t nr, const int64_t* __restrict__ size_starts, const int32_t* __restrict__ leaf_of,
                                                       const int64_t* __restrict__ leaf_range, int max_occs, int64_t* __restrict__ counts) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= nr) return;
  const int64_t size = size_starts[r + 1] - size_starts[r];
  const int64_t before = size_starts[r] - size_starts[leaf_range[leaf_of[r]]];
  const int64_t room = int64_t(max_occs) - before;
  int64_t n;
  if (size <= 0) n = 0;
  else if (before == 0) n = size - 1 > room ? room : size;
  else n = room <= 0 ? 0 : size < room ? size : room;
  counts[r] = n;
}

// leaf l's segment of the rows buffer starts where its first range does
__global__ __launch_bounds__(256) void bq_leaf_starts_kernel(int64_t nleaves, const int64_t* __restrict__ leaf_range,
                                                             const int64_t* __restrict__ range_starts, int64_t* __restrict__ leaf_starts,
                                                             int64_t* __restrict__ total2) {
  const int64_t l = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (l > nleaves) return;
  const int64_t s = range_starts[leaf_range[l]];
  leaf_starts[l] = s;
  if (l == nleaves) {
    total2[0] = s;
    total2[1] = 0;
  }
}

// ---- segmented adjacent-unique over the sorted pairs of the leaf segments ---------------------------------------------------------

__global__ __launch_bounds__(256) void bq_unique_flag_kernel(int64_t n, int64_t nseg, const int64_t* __restrict__ starts,
                                                             const int64_t* __restrict__ doc, const int64_t* __restrict__ off,
                                                             int64_t* __restrict__ keep) {
  for (int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x; p < n; p += int64_t(gridDim.x) * 256) {
    bool k = true;
    if (p > 0 && doc[p] == doc[p - 1] && off[p] == off[p - 1]) k = starts[last_start_le(starts, nseg, p)] == p;   // equal to its neighbour: kept only as a segment's first
    keep[p] = k ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void bq_unique_scatter_kernel(int64_t n, const int64_t* __restrict__ slot /* n + 1 */,
                                                                const int64_t* __restrict__ doc, const int64_t* __restrict__ off,
                                                                int64_t* __restrict__ out_doc, int64_t* __restrict__ out_off, int64_t capacity) {
  for (int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x; p < n; p += int64_t(gridDim.x) * 256) {
    const int64_t s = slot[p];
    if (slot[p + 1] != s && s >= 0 && s < capacity) {
      out_doc[s] = doc[p];
      out_off[s] = off[p];
    }
  }
}

__global__ __launch_bounds__(256) void bq_unique_starts_kernel(int64_t nseg, const int64_t* __restrict__ starts, const int64_t* __restrict__ slot,
                                                               int64_t* __restrict__ new_starts) {
  const int64_t l = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (l <= nseg) new_starts[l] = slot[starts[l]];
}

// ---- the node table -----------------------------------------------------------------------------------------------------------
// view v of node g is entry 2 * g + v of vstart / vn: v = 0 its documents (documents arena), v = 1 its pairs (pairs arena)

__global__ __launch_bounds__(256) void bq_leaf_views_kernel(int64_t nleaves, const int32_t* __restrict__ node_of_leaf,
                                                            const int64_t* __restrict__ leaf_starts, const int32_t* __restrict__ ndocs,
                                                            const int64_t* __restrict__ pair_starts, int64_t* __restrict__ vstart,
                                                            int32_t* __restrict__ vn) {
  const int64_t l = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (l >= nleaves) return;
  const int64_t g = node_of_leaf[l];
  vstart[2 * g] = leaf_starts[l];
  vn[2 * g] = ndocs[l];
  vstart[2 * g + 1] = pair_starts[l];
  vn[2 * g + 1] = int32_t(pair_starts[l + 1] - pair_starts[l]);
}

__global__ __launch_bounds__(256) void bq_bind_kernel(int64_t njobs, int view, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                      const int64_t* __restrict__ vstart, const int32_t* __restrict__ vn,
                                                      int64_t* __restrict__ a_start, int32_t* __restrict__ a_n, int64_t* __restrict__ b_start,
                                                      int32_t* __restrict__ b_n) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= njobs) return;
  const int64_t a = 2 * int64_t(left[j]) + view, b = 2 * int64_t(right[j]) + view;
  a_start[j] = vstart[a];
  a_n[j] = vn[a];
  b_start[j] = vstart[b];
  b_n[j] = vn[b];
}

// the results of a level stand at `base` of their arena
__global__ __launch_bounds__(256) void bq_record_kernel(int64_t njobs, int view, const int32_t* __restrict__ node, const int64_t* __restrict__ res_starts,
                                                        int64_t base, int64_t* __restrict__ vstart, int32_t* __restrict__ vn) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= njobs) return;
  const int64_t v = 2 * int64_t(node[j]) + view;
  vstart[v] = base + res_starts[j];
  vn[v] = int32_t(res_starts[j + 1] - res_starts[j]);
}

// ---- gather -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void bq_root_sizes_kernel(int64_t nq, const int32_t* __restrict__ root, const int32_t* __restrict__ type,
                                                            const int32_t* __restrict__ vn, int64_t* __restrict__ sizes) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (q < nq) sizes[q] = vn[2 * int64_t(root[q]) + type[q]];
}

// one workgroup per query at a time; the offsets of a document-typed result are 0
__global__ __launch_bounds__(256) void bq_gather_kernel(int64_t nq, const int32_t* __restrict__ root, const int32_t* __restrict__ type,
                                                        const int64_t* __restrict__ vstart, const int64_t* __restrict__ res_starts,
                                                        const int64_t* __restrict__ docs, const int64_t* __restrict__ pair_doc,
                                                        const int64_t* __restrict__ pair_off, int64_t* __restrict__ out_doc,
                                                        int64_t* __restrict__ out_off, int64_t capacity) {
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const int t = type[q];
    const int64_t src = vstart[2 * int64_t(root[q]) + t], dst = res_starts[q], n = res_starts[q + 1] - dst;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      if (dst + i >= capacity) break;
      out_doc[dst + i] = t ? pair_doc[src + i] : docs[src + i];
      out_off[dst + i] = t ? pair_off[src + i] : 0;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

inline dim3 blocks_for(int64_t n) { return dim3(uint32_t((n + 256) / 256)); }      // (one more than ceil: the n + 1-element kernels)

// one (level, family) of the schedule: jobs [begin, begin + n) of the job arrays
struct Call {
  int64_t begin = 0, n = 0;
  int64_t bound = 0;          // no more results than this
  bool to_documents = false;  // positional: an AND / NOT above reads some result of this call
};

int run_batch(femto_amd_index* ix, int64_t nq, const femto_amd_bquery_t* const* queries, int max_occs, int64_t* res_starts, int32_t* res_type,
              int64_t** res_doc, int64_t** res_off, int64_t* total) {
  int rc;
  // ---- the batch as one forest: global node and leaf numbers
  struct GNode { int op, distance, left, right, leaf, type, height; };
  std::vector<GNode> nodes;
  std::vector<const femto_amd_regexp_t*> leaves;
  std::vector<int32_t> node_of_leaf, root(static_cast<size_t>(nq)), rtype(static_cast<size_t>(nq));
  int height = 0;
  for (int64_t q = 0; q < nq; q++) {
    const femto_amd_bquery* b = queries[q];
    if (!b || b->tree.nodes.empty()) return set_err(FEMTO_AMD_ERR_PARAM, "null query in the batch");
    const int nbase = int(nodes.size()), lbase = int(leaves.size());
    if (nodes.size() + b->tree.nodes.size() >= (size_t(1) << 30)) return set_err(FEMTO_AMD_ERR_PARAM, "too many nodes in one call: split the batch");
    for (const BqNode& n : b->tree.nodes) {
      GNode g{n.op, n.distance, n.left < 0 ? -1 : n.left + nbase, n.right < 0 ? -1 : n.right + nbase, n.leaf < 0 ? -1 : n.leaf + lbase, n.type, n.height};
      if (n.op == BQ_LEAF) node_of_leaf.push_back(int32_t(nodes.size()));
      height = std::max(height, n.height);
      nodes.push_back(g);
    }
    for (const femto_amd_regexp_t* r : b->leaves) leaves.push_back(r);
    root[size_t(q)] = int32_t(nodes.size()) - 1;
    rtype[size_t(q)] = res_type[q] = b->tree.nodes.back().type;
  }
  const int64_t G = int64_t(nodes.size()), nleaves = int64_t(leaves.size());

  // ---- the range table: leaf l's ranges are [leaf_range[l], leaf_range[l + 1])
  std::vector<int32_t> lit_plen;
  std::vector<uint16_t> lit_syms;
  std::vector<int64_t> lit_starts;
  std::vector<femto_amd_nfa_t> nfas;
  std::vector<int64_t> nfa_leaf;
  for (int64_t l = 0; l < nleaves; l++) {
    const uint16_t* syms = nullptr;
    int64_t n = 0;
    if (femto_amd_regexp_literal(leaves[size_t(l)], &syms, &n)) continue;
    nfas.push_back(*femto_amd_regexp_nfa(leaves[size_t(l)]));
    nfa_leaf.push_back(l);
  }
  std::vector<int64_t> nfa_rs(nfas.size() + 1, 0), nfa_first, nfa_last;
  if (!nfas.empty()) {                      // all automata of the batch in one search
    std::vector<int32_t> status(nfas.size(), 0);
    int64_t n = 0, cap = 1 << 16;
    for (int attempt = 0; attempt < 2; attempt++) {
      nfa_first.assign(size_t(cap), 0);
      nfa_last.assign(size_t(cap), 0);
      rc = femto_amd_nfa_search_batch(ix, int64_t(nfas.size()), nfas.data(), cap, nfa_rs.data(), nfa_first.data(), nfa_last.data(), nullptr, nullptr,
                                      status.data(), &n);
      if (rc != FEMTO_AMD_ERR_FULL || attempt) break;
      cap = std::max<int64_t>(n, 1);        // the exact number (or an upper bound) to call again with
    }
    if (rc) return rc;
    for (size_t k = 0; k < status.size(); k++)
      if (status[k])
        return set_err(status[k], "boolean query: the regular expression of leaf " + std::to_string(nfa_leaf[k]) + " of the batch " +
                                      (status[k] == FEMTO_AMD_ERR_OVERWORKED ? "takes too much work" : "overflows the search stack"));
  }
  std::vector<int64_t> leaf_range(size_t(nleaves) + 1), h_first, h_last;
  std::vector<int32_t> lit_of, leaf_of;
  bool any_automaton = !nfas.empty();
  {
    size_t a = 0;
    for (int64_t l = 0; l < nleaves; l++) {
      leaf_range[size_t(l)] = int64_t(h_first.size());
      const uint16_t* syms = nullptr;
      int64_t n = 0;
      if (femto_amd_regexp_literal(leaves[size_t(l)], &syms, &n)) {
        lit_of.push_back(int32_t(lit_plen.size()));
        leaf_of.push_back(int32_t(l));
        h_first.push_back(0);
        h_last.push_back(-1);
        lit_plen.push_back(int32_t(n));
        lit_starts.push_back(int64_t(lit_syms.size()));
        lit_syms.insert(lit_syms.end(), syms, syms + n);
      } else {
        for (int64_t r = nfa_rs[a]; r < nfa_rs[a + 1]; r++) {
          lit_of.push_back(-1);
          leaf_of.push_back(int32_t(l));
          h_first.push_back(nfa_first[size_t(r)]);
          h_last.push_back(nfa_last[size_t(r)]);
        }
        a++;
      }
    }
    leaf_range[size_t(nleaves)] = int64_t(h_first.size());
  }
  const int64_t nr = int64_t(h_first.size()), nlit = int64_t(lit_plen.size());
  if (nr >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "too many result ranges in one call: split the batch");

  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  hipStream_t st = nullptr;       // everything is ordered on the null stream, as the device calls used below are given it
  int64_t *d_first, *d_last, *d_sizes, *d_size_starts, *d_counts, *d_range_starts, *d_leaf_range, *d_leaf_starts, *d_tot;
  int32_t *d_lit_of, *d_leaf_of;
  if ((rc = T.put(&d_first, h_first)) || (rc = T.put(&d_last, h_last)) || (rc = T.put(&d_lit_of, lit_of)) || (rc = T.put(&d_leaf_of, leaf_of)) ||
      (rc = T.put(&d_leaf_range, leaf_range)) || (rc = T.get(&d_sizes, size_t(nr))) || (rc = T.get(&d_size_starts, size_t(nr) + 1)) ||
      (rc = T.get(&d_counts, size_t(nr))) || (rc = T.get(&d_range_starts, size_t(nr) + 1)) || (rc = T.get(&d_leaf_starts, size_t(nleaves) + 1)) ||
      (rc = T.get(&d_tot, 2)))
    return rc;
  int64_t *d_lit_first = nullptr, *d_lit_last = nullptr;
  if (nlit) {                               // all literal leaves of the batch in one count
    int32_t* d_plen;
    uint16_t* d_pats;
    int64_t* d_starts;
    const int64_t nsyms = int64_t(lit_syms.size());
    if ((rc = upload_patterns(T, nlit, lit_plen.data(), lit_starts.data(), nsyms, {{lit_syms.data(), nsyms, 0}}, &d_plen, &d_pats, &d_starts)) ||
        (rc = T.get(&d_lit_first, size_t(nlit))) || (rc = T.get(&d_lit_last, size_t(nlit))))
      return rc;
    if ((rc = femto_amd_count_device(ix, nlit, d_plen, d_pats, d_starts, d_lit_first, d_lit_last, st))) return rc;
  }
  if (nr) {
    hipLaunchKernelGGL(bq_ranges_kernel, blocks_for(nr), dim3(256), 0, st, nr, static_cast<const int32_t*>(d_lit_of),
                       static_cast<const int64_t*>(d_lit_first), static_cast<const int64_t*>(d_lit_last), d_first, d_last, d_sizes);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = device_scan(T.scan, nr, d_sizes, d_size_starts, 0, st))) return rc;
  if (nr) {
    hipLaunchKernelGGL(bq_clamp_kernel, blocks_for(nr), dim3(256), 0, st, nr, static_cast<const int64_t*>(d_size_starts),
                       static_cast<const int32_t*>(d_leaf_of), static_cast<const int64_t*>(d_leaf_range), max_occs, d_counts);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = device_scan(T.scan, nr, d_counts, d_range_starts, 0, st))) return rc;
  hipLaunchKernelGGL(bq_leaf_starts_kernel, blocks_for(nleaves + 1), dim3(256), 0, st, nleaves, static_cast<const int64_t*>(d_leaf_range),
                     static_cast<const int64_t*>(d_range_starts), d_leaf_starts, d_tot);
  HIP_TRY(hipGetLastError());
  // READBACK 1: the leaves' segment starts (their last entry is the row total)
  std::vector<int64_t> leaf_starts(size_t(nleaves) + 1);
  HIP_TRY(hipMemcpyAsync(leaf_starts.data(), d_leaf_starts, leaf_starts.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t rows = leaf_starts[size_t(nleaves)];
  if (rows >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "2^31 or more located rows in one call: split the batch or lower max_occs_each");

  // ---- the schedule: jobs by height and family, each call's bound, the arenas' sizes
  std::vector<int64_t> bound(static_cast<size_t>(G), 0);
  for (int64_t g = 0; g < G; g++) {
    const GNode& n = nodes[size_t(g)];
    if (n.op == BQ_LEAF) bound[size_t(g)] = leaf_starts[size_t(n.leaf) + 1] - leaf_starts[size_t(n.leaf)];
    else if (n.op == BQ_AND) bound[size_t(g)] = std::min(bound[size_t(n.left)], bound[size_t(n.right)]);
    else if (n.op == BQ_NOT) bound[size_t(g)] = bound[size_t(n.left)];
    else bound[size_t(g)] = bound[size_t(n.left)] + bound[size_t(n.right)];
  }
  std::vector<uint8_t> read_as_documents(static_cast<size_t>(G), 0);       // a pair-typed node under AND / NOT
  for (const GNode& n : nodes)
    if (n.op == BQ_AND || n.op == BQ_NOT)
      for (int c : {n.left, n.right})
        if (nodes[size_t(c)].type == BQ_PAIRS) read_as_documents[size_t(c)] = 1;
  auto positional = [](const GNode& n) { return n.op == BQ_THEN || n.op == BQ_WITHIN || (n.op == BQ_OR && n.type == BQ_PAIRS); };
  std::vector<std::vector<int32_t>> by_level[2];
  by_level[0].resize(size_t(height) + 1);
  by_level[1].resize(size_t(height) + 1);
  for (int64_t g = 0; g < G; g++)
    if (nodes[size_t(g)].op != BQ_LEAF) by_level[positional(nodes[size_t(g)]) ? 1 : 0][size_t(nodes[size_t(g)].height)].push_back(int32_t(g));
  std::vector<int32_t> job_node, job_left, job_right, job_op, job_dist;
  std::vector<Call> calls[2];
  calls[0].resize(size_t(height) + 1);
  calls[1].resize(size_t(height) + 1);
  int64_t doc_cap = rows, pair_cap = rows, max_jobs = 1, ncalls = 0;
  for (int h = 1; h <= height; h++)
    for (int fam = 0; fam < 2; fam++) {
      Call& c = calls[fam][size_t(h)];
      c.begin = int64_t(job_node.size());
      for (int32_t g : by_level[fam][size_t(h)]) {
        const GNode& n = nodes[size_t(g)];
        job_node.push_back(g);
        job_left.push_back(n.left);
        job_right.push_back(n.right);
        job_op.push_back(fam ? (n.op == BQ_THEN ? FEMTO_AMD_DOCPOS_THEN : n.op == BQ_WITHIN ? FEMTO_AMD_DOCPOS_WITHIN : FEMTO_AMD_DOCPOS_OR)
                             : (n.op == BQ_AND ? FEMTO_AMD_DOCSET_AND : n.op == BQ_NOT ? FEMTO_AMD_DOCSET_NOT : FEMTO_AMD_DOCSET_OR));
        job_dist.push_back(n.distance);
        c.bound += bound[size_t(g)];
        if (fam && read_as_documents[size_t(g)]) c.to_documents = true;
      }
      c.n = int64_t(job_node.size()) - c.begin;
      if (!c.n) continue;
      max_jobs = std::max(max_jobs, c.n);
      ncalls += fam && c.to_documents ? 2 : 1;
      if (fam) {
        pair_cap += c.bound;
        if (c.to_documents) doc_cap += c.bound;
      } else {
        doc_cap += c.bound;
      }
    }

  // ---- locate, list, drop repeated rows
  int64_t *d_offs, *d_docs, *d_pdoc, *d_poff, *d_pair_starts, *d_vstart, *d_tots, *d_rs;
  int32_t *d_ndocs, *d_vn, *d_node_of_leaf, *d_job_node, *d_job_left, *d_job_right, *d_job_op, *d_job_dist, *d_an, *d_bn;
  int64_t *d_as, *d_bs;
  if ((rc = T.get(&d_offs, size_t(rows))) || (rc = T.get(&d_docs, size_t(doc_cap))) || (rc = T.get(&d_pdoc, size_t(pair_cap))) ||
      (rc = T.get(&d_poff, size_t(pair_cap))) || (rc = T.get(&d_ndocs, size_t(nleaves))) || (rc = T.get(&d_vstart, size_t(2 * G))) ||
      (rc = T.get(&d_vn, size_t(2 * G))) || (rc = T.put(&d_node_of_leaf, node_of_leaf)) || (rc = T.put(&d_job_node, job_node)) ||
      (rc = T.put(&d_job_left, job_left)) || (rc = T.put(&d_job_right, job_right)) || (rc = T.put(&d_job_op, job_op)) ||
      (rc = T.put(&d_job_dist, job_dist)) || (rc = T.get(&d_as, size_t(max_jobs))) || (rc = T.get(&d_bs, size_t(max_jobs))) ||
      (rc = T.get(&d_an, size_t(max_jobs))) || (rc = T.get(&d_bn, size_t(max_jobs))) || (rc = T.get(&d_rs, size_t(max_jobs) + 1)) ||
      (rc = T.get(&d_tots, size_t(2 * ncalls) + 2)))
    return rc;
  HIP_TRY(hipMemsetAsync(d_tots, 0, (size_t(2 * ncalls) + 2) * 8, st));
  if (rows && (rc = femto_amd_locate_walk_device(ix, nr, d_first, d_range_starts, rows, d_offs, st))) return rc;
  d_pair_starts = d_leaf_starts;
  if (!any_automaton) {                     // located rows are distinct: the sorted pairs are lists as they stand
    if ((rc = femto_amd_doclist_device(ix, nleaves, d_leaf_starts, d_offs, rows, d_tot, d_ndocs, d_docs, nullptr, nullptr, d_pdoc, d_poff, nullptr,
                                       nullptr, st)))
      return rc;
  } else {
    int64_t *d_rdoc, *d_roff, *d_keep, *d_slot;
    if ((rc = T.get(&d_rdoc, size_t(rows))) || (rc = T.get(&d_roff, size_t(rows))) || (rc = T.get(&d_keep, size_t(rows))) ||
        (rc = T.get(&d_slot, size_t(rows) + 1)) || (rc = T.get(&d_pair_starts, size_t(nleaves) + 1)))
      return rc;
    if ((rc = femto_amd_doclist_device(ix, nleaves, d_leaf_starts, d_offs, rows, d_tot, d_ndocs, d_docs, nullptr, nullptr, d_rdoc, d_roff, nullptr,
                                       nullptr, st)))
      return rc;
    const dim3 row_grid{uint32_t(persistent_grid(ix, (rows + 255) / 256))};
    if (rows) {
      hipLaunchKernelGGL(bq_unique_flag_kernel, row_grid, dim3(256), 0, st, rows, nleaves, static_cast<const int64_t*>(d_leaf_starts),
                         static_cast<const int64_t*>(d_rdoc), static_cast<const int64_t*>(d_roff), d_keep);
      HIP_TRY(hipGetLastError());
    }
    if ((rc = device_scan(T.scan, rows, d_keep, d_slot, 0, st))) return rc;
    if (rows) {
      hipLaunchKernelGGL(bq_unique_scatter_kernel, row_grid, dim3(256), 0, st, rows, static_cast<const int64_t*>(d_slot),
                         static_cast<const int64_t*>(d_rdoc), static_cast<const int64_t*>(d_roff), d_pdoc, d_poff, rows);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(bq_unique_starts_kernel, blocks_for(nleaves + 1), dim3(256), 0, st, nleaves, static_cast<const int64_t*>(d_leaf_starts),
                       static_cast<const int64_t*>(d_slot), d_pair_starts);
    HIP_TRY(hipGetLastError());
  }
  if (nleaves) {
    hipLaunchKernelGGL(bq_leaf_views_kernel, blocks_for(nleaves), dim3(256), 0, st, nleaves, static_cast<const int32_t*>(d_node_of_leaf),
                       static_cast<const int64_t*>(d_leaf_starts), static_cast<const int32_t*>(d_ndocs), static_cast<const int64_t*>(d_pair_starts),
                       d_vstart, d_vn);
    HIP_TRY(hipGetLastError());
  }

  // ---- the levels
  int64_t doc_at = rows, pair_at = rows, call_no = 0;
  for (int h = 1; h <= height; h++)
    for (int fam = 0; fam < 2; fam++) {
      const Call& c = calls[fam][size_t(h)];
      if (!c.n) continue;
      hipLaunchKernelGGL(bq_bind_kernel, blocks_for(c.n), dim3(256), 0, st, c.n, fam, static_cast<const int32_t*>(d_job_left + c.begin),
                         static_cast<const int32_t*>(d_job_right + c.begin), static_cast<const int64_t*>(d_vstart), static_cast<const int32_t*>(d_vn),
                         d_as, d_an, d_bs, d_bn);
      HIP_TRY(hipGetLastError());
      int64_t* tot = d_tots + 2 * call_no++;
      if (fam == 0) {
        if ((rc = femto_amd_docset_device(ix, c.n, d_docs, d_as, d_an, d_docs, d_bs, d_bn, d_job_op + c.begin, d_rs, d_docs + doc_at, c.bound, tot, st)))
          return rc;
      } else {
        if ((rc = femto_amd_docpos_device(ix, c.n, d_pdoc, d_poff, d_as, d_an, d_pdoc, d_poff, d_bs, d_bn, d_job_op + c.begin, d_job_dist + c.begin, d_rs,
                                          d_pdoc + pair_at, d_poff + pair_at, c.bound, tot, st)))
          return rc;
      }
      hipLaunchKernelGGL(bq_record_kernel, blocks_for(c.n), dim3(256), 0, st, c.n, fam, static_cast<const int32_t*>(d_job_node + c.begin),
                         static_cast<const int64_t*>(d_rs), fam ? pair_at : doc_at, d_vstart, d_vn);
      HIP_TRY(hipGetLastError());
      if (fam && c.to_documents) {          // the level's pair lists are consecutive: d_rs is their starts
        int64_t* d_ds;
        if ((rc = T.get(&d_ds, size_t(c.n) + 1))) return rc;
        tot = d_tots + 2 * call_no++;
        if ((rc = femto_amd_docpos_documents_device(ix, c.n, d_rs, d_pdoc + pair_at, d_ds, d_docs + doc_at, c.bound, tot, st))) return rc;
        hipLaunchKernelGGL(bq_record_kernel, blocks_for(c.n), dim3(256), 0, st, c.n, 0, static_cast<const int32_t*>(d_job_node + c.begin),
                           static_cast<const int64_t*>(d_ds), doc_at, d_vstart, d_vn);
        HIP_TRY(hipGetLastError());
        doc_at += c.bound;
      }
      if (fam) pair_at += c.bound; else doc_at += c.bound;
    }

  // ---- gather the roots
  int32_t *d_root, *d_rtype;
  int64_t *d_qsizes, *d_qstarts;
  if ((rc = T.put(&d_root, root)) || (rc = T.put(&d_rtype, rtype)) || (rc = T.get(&d_qsizes, size_t(nq))) || (rc = T.get(&d_qstarts, size_t(nq) + 1)))
    return rc;
  hipLaunchKernelGGL(bq_root_sizes_kernel, blocks_for(nq), dim3(256), 0, st, nq, static_cast<const int32_t*>(d_root), static_cast<const int32_t*>(d_rtype),
                     static_cast<const int32_t*>(d_vn), d_qsizes);
  HIP_TRY(hipGetLastError());
  if ((rc = device_scan(T.scan, nq, d_qsizes, d_qstarts, 0, st))) return rc;
  // READBACK 2: the result starts, with every level's overflow flag
  std::vector<int64_t> tots(size_t(2 * ncalls) + 2);
  HIP_TRY(hipMemcpyAsync(res_starts, d_qstarts, size_t(nq + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(tots.data(), d_tots, tots.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t k = 0; k < ncalls; k++)
    if (tots[size_t(2 * k + 1)]) return set_err(FEMTO_AMD_ERR_INVALID, "internal error: a level of the boolean batch outgrew its bound");
  const int64_t n = res_starts[nq];
  *total = n;
  if (n == 0) return FEMTO_AMD_OK;
  int64_t *d_out_doc, *d_out_off;
  if ((rc = T.get(&d_out_doc, size_t(n))) || (rc = T.get(&d_out_off, size_t(n)))) return rc;
  hipLaunchKernelGGL(bq_gather_kernel, dim3(uint32_t(persistent_grid(ix, nq))), dim3(256), 0, st, nq,
                     static_cast<const int32_t*>(d_root), static_cast<const int32_t*>(d_rtype), static_cast<const int64_t*>(d_vstart),
                     static_cast<const int64_t*>(d_qstarts), static_cast<const int64_t*>(d_docs), static_cast<const int64_t*>(d_pdoc),
                     static_cast<const int64_t*>(d_poff), d_out_doc, d_out_off, n);
  HIP_TRY(hipGetLastError());
  return pairs_to_host(n, d_out_doc, d_out_off, st, res_doc, res_off, total);
}

}  // namespace
}  // namespace femto_amd

using namespace femto_amd;

int femto_amd_bquery_compile(const uint8_t* query, int64_t query_len, int flags, femto_amd_bquery_t** out) {
  API_BEGIN
  if (!out || (query_len && !query) || query_len < 0) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *out = nullptr;
  std::unique_ptr<femto_amd_bquery> b(new femto_amd_bquery());
  std::string perr;
  bool type_error = false;
  BqParser ps(query, query_len);
  if (!ps.parse(&b->tree, &perr, &type_error)) return set_err(FEMTO_AMD_ERR_PARAM, "query: " + perr);
  for (size_t l = 0; l < b->tree.leaves.size(); l++) {
    const std::string& text = b->tree.leaves[l];
    femto_amd_regexp_t* r = nullptr;
    const int rc = femto_amd_query_compile(reinterpret_cast<const uint8_t*>(text.data()), int64_t(text.size()), flags, &r);
    if (rc) return set_err(rc, "term at byte " + std::to_string(b->tree.leaf_at[l]) + ": " + femto_amd_last_error());
    b->leaves.push_back(r);
  }
  const femto_amd_bquery* bp = b.get();
  bq_echo(b->tree, int(b->tree.nodes.size()) - 1, [bp](int l) { return std::string(femto_amd_regexp_echo(bp->leaves[size_t(l)])); }, b->echo);
  *out = b.release();
  return FEMTO_AMD_OK;
  API_END
}

int femto_amd_bquery_info(const femto_amd_bquery_t* q, int* nodes, int* leaves, int* result_type) {
  if (!q) return set_err(FEMTO_AMD_ERR_PARAM, "null query");
  if (nodes) *nodes = int(q->tree.nodes.size());
  if (leaves) *leaves = int(q->leaves.size());
  if (result_type) *result_type = q->tree.nodes.back().type;
  return FEMTO_AMD_OK;
}

int femto_amd_bquery_node(const femto_amd_bquery_t* q, int i, int* op, int* distance, int* left, int* right, const femto_amd_regexp_t** leaf) {
  if (!q || i < 0 || size_t(i) >= q->tree.nodes.size()) return set_err(FEMTO_AMD_ERR_PARAM, "no such node");
  const BqNode& n = q->tree.nodes[size_t(i)];
  if (op) *op = n.op;
  if (distance) *distance = n.distance;
  if (left) *left = n.left;
  if (right) *right = n.right;
  if (leaf) *leaf = n.leaf >= 0 ? q->leaves[size_t(n.leaf)] : nullptr;
  return FEMTO_AMD_OK;
}

const char* femto_amd_bquery_echo(const femto_amd_bquery_t* q) { return q ? q->echo.c_str() : ""; }

void femto_amd_bquery_free(femto_amd_bquery_t* q) { delete q; }

int femto_amd_bquery_run_batch(femto_amd_index_t* ix0, int64_t nq, const femto_amd_bquery_t* const* queries, int max_occs_each, int64_t* res_starts,
                               int32_t* res_type, int64_t** res_doc, int64_t** res_off, int64_t* total) {
  API_BEGIN
  if (!ix0 || nq < 0 || !res_starts || !res_doc || !res_off || !total || (nq && (!queries || !res_type)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *res_doc = *res_off = nullptr;
  *total = 0;
  res_starts[0] = 0;
  if (max_occs_each < 0) return set_err(FEMTO_AMD_ERR_PARAM, "negative max_occs_each");
  if (nq >= (int64_t(1) << 30)) return set_err(FEMTO_AMD_ERR_PARAM, "too many queries in one call: split the batch");
  femto_amd_index* ix = replica0(ix0);
  int rc = check_plain_handle(ix, "boolean queries are");
  if (rc) return rc;
  if (nq == 0) return FEMTO_AMD_OK;
  return run_batch(ix, nq, queries, max_occs_each, res_starts, res_type, res_doc, res_off, total);
  API_END
}
