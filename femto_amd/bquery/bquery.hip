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
// That arithmetic is not here: the forest the trees are merged into, the range table and the schedule, with every call's
// offsets in the arenas and its slot of the totals, are bquery_plan.hpp, plain C++ that tests/bquery_plan_check.cpp checks on
// the CPU.  run_batch makes the plan and then runs the four phases, a function each.  launch(), blocks_for() and the copy back
// are ../common/host_common.hpp's; last_start_le is ../common/ragged.hpp's.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "bquery_plan.hpp"

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

// The device arrays that cross a phase boundary (Temp owns them, as it owns every other): the leaves, LEAVES -> LISTING;
struct LeafArrays {
  int64_t nr = 0, rows = 0;
  int64_t *first, *range_starts;     // per range: its first row; where its clamped rows start
  int64_t *leaf_starts, *tot;        // per leaf: its segment of the rows; {rows, 0}
};
// the two arenas with the node table, LISTING -> LEVELS -> GATHER;
struct Arenas {
  int64_t *docs, *pdoc, *poff;
  int64_t* vstart;
  int32_t* vn;
};
// the schedule's device copy with the operand arrays of one call, for LEVELS (tots: GATHER reads the overflow flags)
struct LevelArrays {
  int32_t *job_node, *job_left, *job_right, *job_op, *job_dist, *an, *bn;
  int64_t *as, *bs, *rs, *tots;
};

// all automata of the batch in one search: automaton k's result ranges are first / last [rs[k], rs[k + 1])
int search_automata(femto_amd_index* ix, const std::vector<femto_amd_nfa_t>& nfas, const std::vector<int64_t>& nfa_leaf, std::vector<int64_t>* rs,
                    std::vector<int64_t>* first, std::vector<int64_t>* last) {
  rs->assign(nfas.size() + 1, 0);
  if (nfas.empty()) return FEMTO_AMD_OK;
  std::vector<int32_t> status(nfas.size(), 0);
  int64_t n = 0, cap = 1 << 16;
  int rc = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    first->assign(size_t(cap), 0);
    last->assign(size_t(cap), 0);
    rc = femto_amd_nfa_search_batch(ix, int64_t(nfas.size()), nfas.data(), cap, rs->data(), first->data(), last->data(), nullptr, nullptr, status.data(),
                                    &n);
    if (rc != FEMTO_AMD_ERR_FULL || attempt) break;
    cap = std::max<int64_t>(n, 1);        // the exact number (or an upper bound) to call again with
  }
  if (rc) return rc;
  for (size_t k = 0; k < status.size(); k++)
    if (status[k])
      return set_err(status[k], "boolean query: the regular expression of leaf " + std::to_string(nfa_leaf[k]) + " of the batch " +
                                    (status[k] == FEMTO_AMD_ERR_OVERWORKED ? "takes too much work" : "overflows the search stack"));
  return FEMTO_AMD_OK;
}

// LEAVES: the range table to clamped row counts and starts per range and one segment per leaf
int leaf_rows(femto_amd_index* ix, Temp& T, hipStream_t st, const BqRangeTable& R, int max_occs, LeafArrays* L, std::vector<int64_t>* leaf_starts) {
  int rc;
  const int64_t nr = int64_t(R.first.size()), nlit = int64_t(R.lit_plen.size()), nleaves = int64_t(R.leaf_range.size()) - 1;
  int64_t *d_last, *d_sizes, *d_size_starts, *d_counts, *d_leaf_range;
  int32_t *d_lit_of, *d_leaf_of;
  if ((rc = T.put(&L->first, R.first)) || (rc = T.put(&d_last, R.last)) || (rc = T.put(&d_lit_of, R.lit_of)) || (rc = T.put(&d_leaf_of, R.leaf_of)) ||
      (rc = T.put(&d_leaf_range, R.leaf_range)) || (rc = T.get(&d_sizes, size_t(nr))) || (rc = T.get(&d_size_starts, size_t(nr) + 1)) ||
      (rc = T.get(&d_counts, size_t(nr))) || (rc = T.get(&L->range_starts, size_t(nr) + 1)) || (rc = T.get(&L->leaf_starts, size_t(nleaves) + 1)) ||
      (rc = T.get(&L->tot, 2)))
    return rc;
  int64_t *d_lit_first = nullptr, *d_lit_last = nullptr;
  if (nlit) {                               // all literal leaves of the batch in one count
    int32_t* d_plen;
    uint16_t* d_pats;
    int64_t* d_starts;
    const int64_t nsyms = int64_t(R.lit_syms.size());
    if ((rc = upload_patterns(T, nlit, R.lit_plen.data(), R.lit_starts.data(), nsyms, {{R.lit_syms.data(), nsyms, 0}}, &d_plen, &d_pats, &d_starts)) ||
        (rc = T.get(&d_lit_first, size_t(nlit))) || (rc = T.get(&d_lit_last, size_t(nlit))))
      return rc;
    if ((rc = femto_amd_count_device(ix, nlit, d_plen, d_pats, d_starts, d_lit_first, d_lit_last, st))) return rc;
  }
  if (nr && (rc = launch(bq_ranges_kernel, blocks_for(nr), st, nr, d_lit_of, d_lit_first, d_lit_last, L->first, d_last, d_sizes))) return rc;
  if ((rc = device_scan(T.scan, nr, d_sizes, d_size_starts, 0, st))) return rc;
  if (nr && (rc = launch(bq_clamp_kernel, blocks_for(nr), st, nr, d_size_starts, d_leaf_of, d_leaf_range, max_occs, d_counts))) return rc;
  if ((rc = device_scan(T.scan, nr, d_counts, L->range_starts, 0, st))) return rc;
  if ((rc = launch(bq_leaf_starts_kernel, blocks_for(nleaves + 1), st, nleaves, d_leaf_range, L->range_starts, L->leaf_starts, L->tot))) return rc;
  // READBACK 1: the leaves' segment starts (their last entry is the row total)
  leaf_starts->resize(size_t(nleaves) + 1);
  HIP_TRY(hipMemcpyAsync(leaf_starts->data(), L->leaf_starts, leaf_starts->size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  L->nr = nr;
  L->rows = leaf_starts->back();
  if (L->rows >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "2^31 or more located rows in one call: split the batch or lower max_occs_each");
  return FEMTO_AMD_OK;
}

// the schedule's job arrays go up before anything of LISTING is enqueued: an upload waits for the stream
int upload_schedule(Temp& T, hipStream_t st, const BqSchedule& S, LevelArrays* J) {
  int rc;
  const size_t max_jobs = size_t(S.max_jobs), ntots = size_t(2 * S.ncalls) + 2;
  if ((rc = T.put(&J->job_node, S.job_node)) || (rc = T.put(&J->job_left, S.job_left)) || (rc = T.put(&J->job_right, S.job_right)) ||
      (rc = T.put(&J->job_op, S.job_op)) || (rc = T.put(&J->job_dist, S.job_dist)) || (rc = T.get(&J->as, max_jobs)) || (rc = T.get(&J->bs, max_jobs)) ||
      (rc = T.get(&J->an, max_jobs)) || (rc = T.get(&J->bn, max_jobs)) || (rc = T.get(&J->rs, max_jobs + 1)) || (rc = T.get(&J->tots, ntots)))
    return rc;
  HIP_TRY(hipMemsetAsync(J->tots, 0, ntots * 8, st));
  return FEMTO_AMD_OK;
}

// LISTING: locate, list, drop repeated rows; the leaves' views open the node table
int listing(femto_amd_index* ix, Temp& T, hipStream_t st, const BqForest& F, const BqSchedule& S, const LeafArrays& L, bool any_automaton, Arenas* A) {
  int rc;
  const int64_t rows = L.rows, nleaves = int64_t(F.node_of_leaf.size()), G = int64_t(F.nodes.size());
  int64_t *d_offs, *d_pair_starts = L.leaf_starts;
  int32_t *d_ndocs, *d_node_of_leaf;
  if ((rc = T.get(&d_offs, size_t(rows))) || (rc = T.get(&A->docs, size_t(S.doc_cap))) || (rc = T.get(&A->pdoc, size_t(S.pair_cap))) ||
      (rc = T.get(&A->poff, size_t(S.pair_cap))) || (rc = T.get(&d_ndocs, size_t(nleaves))) || (rc = T.get(&A->vstart, size_t(2 * G))) ||
      (rc = T.get(&A->vn, size_t(2 * G))) || (rc = T.put(&d_node_of_leaf, F.node_of_leaf)))
    return rc;
  if (rows && (rc = femto_amd_locate_walk_device(ix, L.nr, L.first, L.range_starts, rows, d_offs, st))) return rc;
  if (!any_automaton) {                     // located rows are distinct: the sorted pairs are lists as they stand
    if ((rc = femto_amd_doclist_device(ix, nleaves, L.leaf_starts, d_offs, rows, L.tot, d_ndocs, A->docs, nullptr, nullptr, A->pdoc, A->poff, nullptr,
                                       nullptr, st)))
      return rc;
  } else {
    int64_t *d_rdoc, *d_roff, *d_keep, *d_slot;
    if ((rc = T.get(&d_rdoc, size_t(rows))) || (rc = T.get(&d_roff, size_t(rows))) || (rc = T.get(&d_keep, size_t(rows))) ||
        (rc = T.get(&d_slot, size_t(rows) + 1)) || (rc = T.get(&d_pair_starts, size_t(nleaves) + 1)))
      return rc;
    if ((rc = femto_amd_doclist_device(ix, nleaves, L.leaf_starts, d_offs, rows, L.tot, d_ndocs, A->docs, nullptr, nullptr, d_rdoc, d_roff, nullptr,
                                       nullptr, st)))
      return rc;
    const dim3 row_grid = persistent_grid(ix, (rows + 255) / 256);
    if (rows && (rc = launch(bq_unique_flag_kernel, row_grid, st, rows, nleaves, L.leaf_starts, d_rdoc, d_roff, d_keep))) return rc;
    if ((rc = device_scan(T.scan, rows, d_keep, d_slot, 0, st))) return rc;
    if (rows && (rc = launch(bq_unique_scatter_kernel, row_grid, st, rows, d_slot, d_rdoc, d_roff, A->pdoc, A->poff, rows))) return rc;
    if ((rc = launch(bq_unique_starts_kernel, blocks_for(nleaves + 1), st, nleaves, L.leaf_starts, d_slot, d_pair_starts))) return rc;
  }
  if (nleaves && (rc = launch(bq_leaf_views_kernel, blocks_for(nleaves), st, nleaves, d_node_of_leaf, L.leaf_starts, d_ndocs, d_pair_starts, A->vstart,
                              A->vn)))
    return rc;
  return FEMTO_AMD_OK;
}

// LEVELS: every call of the schedule at the place the schedule gave it
int levels(femto_amd_index* ix, Temp& T, hipStream_t st, const BqSchedule& S, const LevelArrays& J, const Arenas& A) {
  int rc;
  for (size_t h = 1; h < S.calls[0].size(); h++)
    for (int fam = 0; fam < 2; fam++) {
      const BqCall& c = S.calls[fam][h];
      if (!c.n) continue;
      if ((rc = launch(bq_bind_kernel, blocks_for(c.n), st, c.n, fam, J.job_left + c.begin, J.job_right + c.begin, A.vstart, A.vn, J.as, J.an, J.bs, J.bn)))
        return rc;
      int64_t* tot = J.tots + 2 * c.tot;
      if (fam == 0) {
        if ((rc = femto_amd_docset_device(ix, c.n, A.docs, J.as, J.an, A.docs, J.bs, J.bn, J.job_op + c.begin, J.rs, A.docs + c.doc_at, c.bound, tot, st)))
          return rc;
      } else {
        if ((rc = femto_amd_docpos_device(ix, c.n, A.pdoc, A.poff, J.as, J.an, A.pdoc, A.poff, J.bs, J.bn, J.job_op + c.begin, J.job_dist + c.begin, J.rs,
                                          A.pdoc + c.pair_at, A.poff + c.pair_at, c.bound, tot, st)))
          return rc;
      }
      if ((rc = launch(bq_record_kernel, blocks_for(c.n), st, c.n, fam, J.job_node + c.begin, J.rs, fam ? c.pair_at : c.doc_at, A.vstart, A.vn))) return rc;
      if (fam && c.to_documents) {          // the level's pair lists are consecutive: J.rs is their starts
        int64_t* d_ds;
        if ((rc = T.get(&d_ds, size_t(c.n) + 1))) return rc;
        if ((rc = femto_amd_docpos_documents_device(ix, c.n, J.rs, A.pdoc + c.pair_at, d_ds, A.docs + c.doc_at, c.bound, tot + 2, st))) return rc;
        if ((rc = launch(bq_record_kernel, blocks_for(c.n), st, c.n, 0, J.job_node + c.begin, d_ds, c.doc_at, A.vstart, A.vn))) return rc;
      }
    }
  return FEMTO_AMD_OK;
}

// GATHER: the root views packed in query order
int gather(femto_amd_index* ix, Temp& T, hipStream_t st, const BqForest& F, int64_t ncalls, const int64_t* d_tots, const Arenas& A, int64_t* res_starts,
           int64_t** res_doc, int64_t** res_off, int64_t* total) {
  int rc;
  const int64_t nq = int64_t(F.root.size());
  int32_t *d_root, *d_rtype;
  int64_t *d_qsizes, *d_qstarts;
  if ((rc = T.put(&d_root, F.root)) || (rc = T.put(&d_rtype, F.rtype)) || (rc = T.get(&d_qsizes, size_t(nq))) || (rc = T.get(&d_qstarts, size_t(nq) + 1)))
    return rc;
  if ((rc = launch(bq_root_sizes_kernel, blocks_for(nq), st, nq, d_root, d_rtype, A.vn, d_qsizes))) return rc;
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
  if ((rc = launch(bq_gather_kernel, persistent_grid(ix, nq), st, nq, d_root, d_rtype, A.vstart, d_qstarts, A.docs, A.pdoc, A.poff, d_out_doc,
                   d_out_off, n)))
    return rc;
  return pairs_to_host(n, d_out_doc, d_out_off, st, res_doc, res_off, total);
}

// the host plan of the batch (bquery_plan.hpp): the trees as one forest, then the range table of its leaves in leaf order
int plan_leaves(femto_amd_index* ix, int64_t nq, const femto_amd_bquery_t* const* queries, int32_t* res_type, BqForest* F, BqRangeTable* R,
                bool* any_automaton) {
  struct Leaf { const uint16_t* syms; int64_t n; bool literal; };
  std::vector<Leaf> leaves;
  std::vector<femto_amd_nfa_t> nfas;
  std::vector<int64_t> nfa_leaf, nfa_rs, nfa_first, nfa_last;
  for (int64_t q = 0; q < nq; q++) {
    const femto_amd_bquery* b = queries[q];
    if (!b || b->tree.nodes.empty()) return set_err(FEMTO_AMD_ERR_PARAM, "null query in the batch");
    if (!F->append(b->tree)) return set_err(FEMTO_AMD_ERR_PARAM, "too many nodes in one call: split the batch");
    res_type[q] = F->rtype.back();
    for (const femto_amd_regexp_t* r : b->leaves) {
      Leaf l{nullptr, 0, false};
      l.literal = femto_amd_regexp_literal(r, &l.syms, &l.n) != 0;
      if (!l.literal) {
        nfas.push_back(*femto_amd_regexp_nfa(r));
        nfa_leaf.push_back(int64_t(leaves.size()));
      }
      leaves.push_back(l);
    }
  }
  const int rc = search_automata(ix, nfas, nfa_leaf, &nfa_rs, &nfa_first, &nfa_last);
  if (rc) return rc;
  size_t a = 0;
  for (const Leaf& l : leaves)
    if (l.literal) {
      R->literal_leaf(l.syms, l.n);
    } else {
      R->automaton_leaf(nfa_first.data() + nfa_rs[a], nfa_last.data() + nfa_rs[a], nfa_rs[a + 1] - nfa_rs[a]);
      a++;
    }
  if (int64_t(R->first.size()) >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "too many result ranges in one call: split the batch");
  *any_automaton = !nfas.empty();
  return FEMTO_AMD_OK;
}

int run_batch(femto_amd_index* ix, int64_t nq, const femto_amd_bquery_t* const* queries, int max_occs, int64_t* res_starts, int32_t* res_type,
              int64_t** res_doc, int64_t** res_off, int64_t* total) {
  int rc;
  BqForest F;
  BqRangeTable R;
  bool any_automaton = false;
  if ((rc = plan_leaves(ix, nq, queries, res_type, &F, &R, &any_automaton))) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  hipStream_t st = nullptr;       // everything is ordered on the null stream, as the device calls used below are given it
  LeafArrays L;
  std::vector<int64_t> leaf_starts;
  if ((rc = leaf_rows(ix, T, st, R, max_occs, &L, &leaf_starts))) return rc;             // LEAVES, readback 1
  const BqSchedule S = bq_schedule(F, leaf_starts);                                      // the rows are known: every call's place
  LevelArrays J;
  Arenas A;
  if ((rc = upload_schedule(T, st, S, &J))) return rc;
  if ((rc = listing(ix, T, st, F, S, L, any_automaton, &A))) return rc;                  // LISTING
  if ((rc = levels(ix, T, st, S, J, A))) return rc;                                      // LEVELS
  return gather(ix, T, st, F, S.ncalls, J.tots, A, res_starts, res_doc, res_off, total);  // GATHER, readback 2
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
