// similar.hip -- the byte sequences a file shares with the index, the documents that share them and how similar the file is to
// each (src/main/similar_tool.c).  include/femto_amd.h "common sequences" states the contract; DESIGN.md "Common sequences" the
// kernels and what follows from them.
//
// TAKEN FROM THE REFERENCE: the definitions of its header comment (similar_tool.c:49-84: common sequences grown backwards one byte
// at a time, sequences contained in longer ones removed, sequences found in the --not indexes removed), its score
// (accumulate_score / compute_score, :207-253: sum of length * min(occurrences here, occurrences there), divided by
// min(input length, document length)) and its defaults min_match_length = 8 and max_offsets = 100.  NOT TAKEN: femto-similar
// itself is not built and its printout is not restated -- the --too-similar-stop early exit, the rule that a sequence is reported
// only when none of its occurrences extends, and the overlap removal in qsort order are heuristics of the tool, not of the
// question.
//
// MATCHING STATISTICS.  The reference grows all sequences together, one parallel_query of single steps per round with host
// bookkeeping in between.  Here every END position j of the query runs its own backward search q[j], q[j-1], ... until the range
// empties: one lane per position, one kernel per rank policy (P::search_step called as count_tail_kernel's closing loop calls
// it), the last non-empty range kept.  The bytes are fetched in aligned 8-byte words, right to left.  A lane is a chain of
// dependent scattered loads and the lanes of a wavefront retire at different lengths: occupancy hides the latency, so the kernel
// is held to the policy's kDirectWaves wavefronts per SIMD.  Handles in rank modes 0 / 1 with the derived segment lines are
// served by LanePolicy of ../common/lane_policy.hpp (c_plus_occ_lane, the step of regexp_search.hip's WavePolicy).
//
// SEQUENCES.  End position j is selected when len[j] >= min_len and the match ending at j + 1 does not contain it
// (len[j + 1] <= len[j]; len[j + 1] <= len[j] + 1 always holds): flags, the shared exclusive scan, a scatter in ascending j.
// GROUPS.  Two selected sequences are the same string exactly when (len, first) agree -- the ranges of distinct strings of one
// length are disjoint -- so the distinct sequences are the runs of ONE stable 64-bit radix sort (rocPRIM) of the keys
// (65535 - len) << 48 | first: no byte is compared.  The head of a run writes the group (the sort is stable, so the head is the
// occurrence with the smallest start) and finds the run's end by binary search.
// DOCUMENTS.  The kept groups' rows under do_locate_query's clamp -> femto_amd_locate_walk_device -> femto_amd_doclist_device;
// its d_hits is the number of occurrences in each document, accumulated into two dense arrays with ordinary atomicAdd.  The walk
// is sized on the host (femto_amd_locate_walk_device takes its total by value), so the row plan is followed by PAD segments of at
// most total_length rows each, starting at row 0, that take the walk from the device's total up to that size: every row the walk
// reads is a row of the index, and nothing returns to the host.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../common/block.hpp"
#include "../csrc/kernels.hip.hpp"
#include "../csrc/pack_kernels.hip.hpp"
#include "../csrc/ru_kernels.hip.hpp"
#include "../csrc/pack2_kernels.hip.hpp"
#include "../csrc/ind_kernels.hip.hpp"
#include "../csrc/text_kernels.hip.hpp"
#include "../common/lane_policy.hpp"

namespace femto_amd {
namespace {

constexpr int32_t kMaxPattern = 32768;      // MAX_PATTERN_LENGTH: max_len <= 0
constexpr int32_t kMinLen = 8;              // min_match_length (similar_tool.c)
constexpr int kMaxOffsets = 100;            // max_offsets
constexpr int32_t kKeyLen = 65535;          // the sort key holds 16 bits of length
constexpr int64_t kMaxBytes = int64_t(1) << 39;      // query bytes per call: 2^31 workgroups of 256 lanes
constexpr int64_t kMaxSeqs = int64_t(1) << 31;       // sequences per call: the sort carries 32-bit indexes
const char* const kSubject = "common sequences are";

// ---- matching statistics ------------------------------------------------------------------------------------------------------

// One lane per end position.  kSteps: no outputs but steps[0] += search steps taken, steps[1] += those whose range was one row
// (tools/similar_bench.py: what a text compare on single rows would save).
template <class P, bool kSteps>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P::kDirectWaves, P::kDirectWaves))) void match_stats_kernel(
    const DevIndex ix, const int64_t n, const uint8_t* __restrict__ q, const int32_t max_len, int32_t* __restrict__ out_len,
    int64_t* __restrict__ out_first, int64_t* __restrict__ out_last, unsigned long long* __restrict__ steps) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  unsigned long long nsteps = 0, nsingle = 0;
  if (j < n) {
    const int cap = j + 1 < int64_t(max_len) ? int(j + 1) : max_len;
    int len = 0;
    int64_t first = 0, last = ix.total_length - 1;      // the empty pattern's range
    uint64_t word = 0;              // the aligned 8-byte word holding the byte being read: never below the word of q[0]
    uintptr_t word_addr = 0;
    for (int l = 0; l < cap; l++) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(q + (j - l));
      const uintptr_t wa = a & ~uintptr_t(7);
      if (wa != word_addr) {
        word = *reinterpret_cast<const uint64_t*>(wa);
        word_addr = wa;
      }
      const uint32_t ch = (uint32_t(word >> (8 * (a - wa))) & 0xffu) + uint32_t(FEMTO_AMD_CHARACTER_OFFSET);
      const uint32_t code = P::code_of(ix, ch);
      if (code == 0xffffu) break;      // the byte does not occur in the text
      if (kSteps) {
        nsteps++;
        nsingle += first == last && l > 0;
      }
      int64_t nf = first, nl = last;
      P::search_step(ix, l, code, nf, nl);
      if (nf > nl) break;
      first = nf;
      last = nl;
      len = l + 1;
    }
    if (!kSteps) {
      out_len[j] = len;
      if (out_first) out_first[j] = first;
      if (out_last) out_last[j] = last;
    }
  }
  if (kSteps) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      nsteps += __shfl_xor(nsteps, o);
      nsingle += __shfl_xor(nsingle, o);
    }
    if ((threadIdx.x & 63) == 0 && nsteps) {
      atomicAdd(steps, nsteps);
      atomicAdd(steps + 1, nsingle);
    }
  }
}

// ---- sequences ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool seq_selected(const int32_t* __restrict__ len, int64_t n, int64_t j, int32_t min_len) {
  const int32_t l = len[j];
  return l >= min_len && (j == n - 1 || len[j + 1] <= l);
}

__global__ __launch_bounds__(256) void seq_flag_kernel(const int64_t n, const int32_t* __restrict__ len, const int32_t min_len,
                                                       int64_t* __restrict__ flags) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j < n) flags[j] = seq_selected(len, n, j, min_len) ? 1 : 0;
}

__global__ __launch_bounds__(256) void seq_scatter_kernel(const int64_t n, const int32_t* __restrict__ len, const int64_t* __restrict__ first,
                                                          const int64_t* __restrict__ last, const int32_t min_len, const int64_t* __restrict__ cum,
                                                          int64_t* __restrict__ seq_start, int32_t* __restrict__ seq_len,
                                                          int64_t* __restrict__ seq_first, int64_t* __restrict__ seq_last, const int64_t capacity,
                                                          int64_t* __restrict__ d_total) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j == 0) write_total(d_total, cum[n], capacity);
  if (j >= n || !seq_selected(len, n, j, min_len)) return;
  const int64_t k = cum[j];
  if (k >= capacity) return;
  const int32_t l = len[j];
  if (seq_start) seq_start[k] = j - l + 1;
  if (seq_len) seq_len[k] = l;
  if (seq_first) seq_first[k] = first[j];
  if (seq_last) seq_last[k] = last[j];
}

// ---- groups -------------------------------------------------------------------------------------------------------------------

// the sequences a {total, overflow} pair and a capacity leave complete
__device__ __forceinline__ int64_t live_seqs(const int64_t* __restrict__ d_total, int64_t capacity) {
  const int64_t t = d_total[0];
  return t < 0 ? 0 : (t < capacity ? t : capacity);
}

__global__ __launch_bounds__(256) void group_key_kernel(const int64_t capacity, const int64_t* __restrict__ d_total, const int32_t* __restrict__ seq_len,
                                                        const int64_t* __restrict__ seq_first, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k >= capacity) return;
  uint64_t key = ~uint64_t(0);      // behind every live key: a live one has len >= 1
  if (k < live_seqs(d_total, capacity)) {
    const int32_t l = seq_len[k] < kKeyLen ? seq_len[k] : kKeyLen;
    key = (uint64_t(kKeyLen - l) << 48) | (uint64_t(seq_first[k]) & ((uint64_t(1) << 48) - 1));
  }
  keys[k] = key;
  idx[k] = uint32_t(k);
}

__global__ __launch_bounds__(256) void group_head_kernel(const int64_t capacity, const int64_t* __restrict__ d_total, const uint64_t* __restrict__ keys,
                                                         int64_t* __restrict__ flags) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= capacity) return;
  flags[s] = (s < live_seqs(d_total, capacity) && (s == 0 || keys[s] != keys[s - 1])) ? 1 : 0;
}

struct GroupOut {
  int64_t* group_of;
  int32_t* len;
  int64_t *first, *last;
  int32_t* here;
  int64_t *min_start, *ngroups;
};

// heads[s]: the number of run heads before sorted position s (exclusive scan of the flags; heads[capacity] = the groups)
__global__ __launch_bounds__(256) void group_write_kernel(const int64_t capacity, const int64_t* __restrict__ d_total, const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ idx, const int64_t* __restrict__ heads,
                                                          const int64_t* __restrict__ seq_start, const int32_t* __restrict__ seq_len,
                                                          const int64_t* __restrict__ seq_first, const int64_t* __restrict__ seq_last, const GroupOut out) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t live = live_seqs(d_total, capacity);
  if (s == 0) out.ngroups[0] = heads[capacity];
  unsigned long long part = 0;
  if (s < live) {
    const int64_t k = int64_t(idx[s]);
    const bool head = heads[s + 1] != heads[s];
    const int64_t g = head ? heads[s] : heads[s] - 1;
    if (out.group_of) out.group_of[k] = g;
    if (head) {
      const uint64_t key = keys[s];
      int64_t lo = s + 1, hi = live;      // the end of the run: the first position behind s with another key
      while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (keys[m] == key) lo = m + 1; else hi = m;
      }
      const int64_t here = lo - s, there = seq_last[k] - seq_first[k] + 1;
      if (out.len) out.len[g] = seq_len[k];
      if (out.first) out.first[g] = seq_first[k];
      if (out.last) out.last[g] = seq_last[k];
      if (out.here) out.here[g] = int32_t(here);
      if (out.min_start) out.min_start[g] = seq_start[k];
      part = static_cast<unsigned long long>(int64_t(seq_len[k]) * (here < there ? here : there));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if ((threadIdx.x & 63) == 0 && part) atomicAdd(reinterpret_cast<unsigned long long*>(out.ngroups + 1), part);
}

// ---- documents ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t live_groups(const int64_t* __restrict__ d_ngroups, int64_t capacity) {
  const int64_t t = d_ngroups[0];
  return t < 0 ? 0 : (t < capacity ? t : capacity);
}

// the rows do_locate_query returns for every kept group (the clamp as text_kernels.hip.hpp:446-451 states it)
__global__ __launch_bounds__(256) void doc_rows_kernel(const int64_t capacity, const int64_t* __restrict__ d_ngroups, const int64_t* __restrict__ g_first,
                                                       const int64_t* __restrict__ g_last, const uint8_t* __restrict__ keep, const int max_occs,
                                                       int64_t* __restrict__ counts) {
  const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (g >= capacity) return;
  int64_t c = 0;
  if (g < live_groups(d_ngroups, capacity) && (!keep || keep[g])) {
    const int64_t first = g_first[g], last = g_last[g];
    if (first > last) c = 0;
    else if (last - first > int64_t(max_occs)) c = max_occs;
    else c = last - first + 1;
  }
  counts[g] = c;
}

// The row plan the walk takes: segment g < capacity = the group's rows (none at all when they do not fit the caller's buffer),
// then npad PAD segments from row 0, at most N rows each, up to the size `walk` the host launches the walk with.
__global__ __launch_bounds__(256) void doc_plan_kernel(const int64_t capacity, const int64_t npad, const int64_t* __restrict__ cum, const int64_t* __restrict__ g_first,
                                                       const int64_t offsets_capacity, const int64_t walk, const int64_t N,
                                                       int64_t* __restrict__ starts, int64_t* __restrict__ first, int64_t* __restrict__ d_total) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t total = cum[capacity];
  const bool fits = total <= offsets_capacity;
  const int64_t base = fits ? total : 0;
  if (k == 0) write_total(d_total, total, offsets_capacity);
  if (k < capacity) {
    starts[k] = fits ? cum[k] : 0;
    first[k] = g_first[k];
  } else if (k < capacity + npad) {
    const int64_t p = k - capacity, at = base + p * N;
    starts[k] = at < walk ? at : walk;
    first[k] = 0;
  } else if (k == capacity + npad) {
    starts[k] = walk;
  }
}

__global__ __launch_bounds__(256) void doc_zero_kernel(const int64_t ndocs, int64_t* __restrict__ score, int32_t* __restrict__ seqs) {
  const int64_t d = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (d >= ndocs) return;
  score[d] = 0;
  seqs[d] = 0;
}

// one lane per located row slot: the slots [starts[g], starts[g] + ndocs[g]) hold group g's documents and hits
__global__ __launch_bounds__(256) void doc_score_kernel(const int64_t capacity, const int64_t walk, const int64_t* __restrict__ d_total,
                                                        const int64_t* __restrict__ starts, const int32_t* __restrict__ ndocs,
                                                        const int64_t* __restrict__ docs, const int32_t* __restrict__ hits,
                                                        const int32_t* __restrict__ g_len, const int32_t* __restrict__ g_here, const int64_t ndocuments,
                                                        int64_t* __restrict__ score, int32_t* __restrict__ seqs) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= walk || d_total[1] || r >= d_total[0]) return;
  const int64_t g = last_start_le(starts, capacity, r);
  if (r - starts[g] >= int64_t(ndocs[g])) return;
  const int64_t d = docs[r];
  if (d < 0 || d >= ndocuments) return;
  const int64_t here = g_here[g], there = hits[r];
  atomicAdd(reinterpret_cast<unsigned long long*>(score + d), static_cast<unsigned long long>(int64_t(g_len[g]) * (here < there ? here : there)));
  atomicAdd(seqs + d, 1);
}

// ---- stop lists ---------------------------------------------------------------------------------------------------------------

// group g's bytes as a pattern: q[min_start .. min_start + len) + 5 at pats[starts[g] ..)
__global__ __launch_bounds__(256) void stop_gather_kernel(const int64_t ngroups, const int64_t* __restrict__ starts, const int64_t* __restrict__ min_start,
                                                          const uint8_t* __restrict__ q, uint16_t* __restrict__ pats) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= starts[ngroups]) return;
  const int64_t g = last_start_le(starts, ngroups, t);
  pats[t] = uint16_t(q[min_start[g] + (t - starts[g])]) + uint16_t(FEMTO_AMD_CHARACTER_OFFSET);
}

__global__ __launch_bounds__(256) void stop_clear_kernel(const int64_t ngroups, const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                         uint8_t* __restrict__ keep) {
  const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (g < ngroups && first[g] <= last[g]) keep[g] = 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

// steps != NULL: the counting form (no outputs)
int run_match_stats(femto_amd_index* ix, int64_t n, const uint8_t* d_bytes, int32_t max_len, int32_t* d_len, int64_t* d_first, int64_t* d_last,
                    unsigned long long* steps, hipStream_t st) {
  const int32_t ml = max_len <= 0 ? kMaxPattern : max_len;
  auto go = [&](auto tag) {
    using P = typename decltype(tag)::type;
    return with_flag(steps != nullptr, [&](auto counting) {
      return launch(match_stats_kernel<P, decltype(counting)::value>, blocks_of(n), st, ix->dev, n, d_bytes, ml, d_len, d_first, d_last, steps);
    });
  };
  return with_lane_policy(ix, "matching statistics on this handle need", go);
}

int run_sequences(femto_amd_index* ix, int64_t n, const int32_t* d_len, const int64_t* d_first, const int64_t* d_last, int32_t min_len,
                  int64_t* d_seq_start, int32_t* d_seq_len, int64_t* d_seq_first, int64_t* d_seq_last, int64_t capacity, int64_t* d_total,
                  hipStream_t st) {
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  int rc;
  if ((rc = S.noccs64.reserve(size_t(n) * 8)) || (rc = S.out_starts.reserve(size_t(n + 1) * 8))) return rc;
  int64_t *flags = S.noccs64.as<int64_t>(), *cum = S.out_starts.as<int64_t>();
  if ((rc = launch(seq_flag_kernel, blocks_of(n), st, n, d_len, min_len, flags)) || (rc = device_scan(S.scan, n, flags, cum, 0, st))) return rc;
  return launch(seq_scatter_kernel, blocks_of(n), st, n, d_len, d_first, d_last, min_len, cum, d_seq_start, d_seq_len, d_seq_first, d_seq_last, capacity,
                d_total);
}

int run_groups(femto_amd_index* ix, int64_t capacity, const int64_t* d_total, const int64_t* d_seq_start, const int32_t* d_seq_len,
               const int64_t* d_seq_first, const int64_t* d_seq_last, const GroupOut& out, hipStream_t st) {
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  int rc;
  const size_t un = size_t(capacity);
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                    static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), un, 0u, 64u, st));
  if ((rc = S.keys.reserve(un * 8)) || (rc = S.keys2.reserve(un * 8)) || (rc = S.idx.reserve(un * 4)) || (rc = S.idx2.reserve(un * 4)) ||
      (rc = S.sorttmp.reserve(tmp_bytes ? tmp_bytes : 16)) || (rc = S.noccs64.reserve(un * 8)) || (rc = S.out_starts.reserve((un + 1) * 8)))
    return rc;
  uint64_t* keys = S.keys2.as<uint64_t>();
  uint32_t* idx = S.idx2.as<uint32_t>();
  int64_t *flags = S.noccs64.as<int64_t>(), *heads = S.out_starts.as<int64_t>();
  if ((rc = launch(group_key_kernel, blocks_of(capacity), st, capacity, d_total, d_seq_len, d_seq_first, S.keys.as<uint64_t>(), S.idx.as<uint32_t>())))
    return rc;
  HIP_TRY(rocprim::radix_sort_pairs(S.sorttmp.p, tmp_bytes, S.keys.as<uint64_t>(), keys, S.idx.as<uint32_t>(), idx, un, 0u, 64u, st));
  if ((rc = launch(group_head_kernel, blocks_of(capacity), st, capacity, d_total, keys, flags)) || (rc = device_scan(S.scan, capacity, flags, heads, 0, st)))
    return rc;
  HIP_TRY(hipMemsetAsync(out.ngroups, 0, 16, st));
  return launch(group_write_kernel, blocks_of(capacity), st, capacity, d_total, keys, idx, heads, d_seq_start, d_seq_len, d_seq_first, d_seq_last, out);
}

int run_documents(femto_amd_index* ix, int64_t gcap, const int64_t* d_ngroups, const int32_t* d_g_len, const int64_t* d_g_first, const int64_t* d_g_last,
                  const int32_t* d_g_here, const uint8_t* d_g_keep, int max_occs, int64_t* d_offsets, int64_t offsets_capacity, int64_t* d_doc_score,
                  int32_t* d_doc_seqs, int64_t* d_total, hipStream_t st) {
  const int64_t N = ix->host.total_length, ndocuments = int64_t(ix->host.doc_ends.size());
  int rc;
  if ((rc = launch(doc_zero_kernel, blocks_of(std::max<int64_t>(ndocuments, 1)), st, ndocuments, d_doc_score, d_doc_seqs))) return rc;
  if (gcap == 0) {
    HIP_TRY(hipMemsetAsync(d_total, 0, 16, st));
    return 0;
  }
  // the walk's size: no more rows than the clamp allows, no more than the caller's buffer holds
  const int64_t most = gcap > INT64_MAX / (int64_t(max_occs) + 1) ? INT64_MAX : gcap * int64_t(max_occs);
  const int64_t walk = std::min(offsets_capacity, most);
  const int64_t npad = N > 0 ? walk / N + 1 : 1;
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  const size_t ug = size_t(gcap), uw = size_t(walk);
  if ((rc = S.noccs64.reserve(ug * 8)) || (rc = S.out_starts.reserve((ug + 1) * 8)) || (rc = S.starts.reserve(size_t(gcap + npad + 1) * 8)) ||
      (rc = S.first.reserve(size_t(gcap + npad) * 8)) || (rc = S.noccs.reserve(ug * 4)) || (rc = S.keys.reserve(uw * 8 + 16)) ||
      (rc = S.idx.reserve(uw * 4 + 16)))
    return rc;
  int64_t *counts = S.noccs64.as<int64_t>(), *cum = S.out_starts.as<int64_t>(), *starts = S.starts.as<int64_t>(), *first = S.first.as<int64_t>();
  int64_t* docs = S.keys.as<int64_t>();
  int32_t *ndocs = S.noccs.as<int32_t>(), *hits = S.idx.as<int32_t>();
  if ((rc = launch(doc_rows_kernel, blocks_of(gcap), st, gcap, d_ngroups, d_g_first, d_g_last, d_g_keep, max_occs, counts)) ||
      (rc = device_scan(S.scan, gcap, counts, cum, 0, st)) ||
      (rc = launch(doc_plan_kernel, blocks_for(gcap + npad), st, gcap, npad, cum, d_g_first, offsets_capacity, walk, N, starts, first, d_total)))
    return rc;
  if (walk == 0) return 0;
  if ((rc = femto_amd_locate_walk_device(ix, gcap + npad, first, starts, walk, d_offsets, st)) ||
      (rc = femto_amd_doclist_device(ix, gcap, starts, d_offsets, walk, d_total, ndocs, docs, nullptr, hits, nullptr, nullptr, nullptr, nullptr, st)))
    return rc;
  return launch(doc_score_kernel, blocks_of(walk), st, gcap, walk, d_total, starts, ndocs, docs, hits, d_g_len, d_g_here, ndocuments, d_doc_score,
                d_doc_seqs);
}

template <class T>
int to_host(std::vector<T>& h, const T* d_src, size_t count, hipStream_t st) {
  h.resize(count);
  if (count) HIP_TRY(hipMemcpyAsync(h.data(), d_src, count * sizeof(T), hipMemcpyDeviceToHost, st));
  return 0;
}

template <class T>
int give(T** out, const std::vector<T>& v) {
  *out = nullptr;
  if (v.empty()) return 0;
  *out = static_cast<T*>(malloc(v.size() * sizeof(T)));
  if (!*out) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  memcpy(*out, v.data(), v.size() * sizeof(T));
  return 0;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_match_stats_device(femto_amd_index_t* ix, int64_t n, const uint8_t* d_bytes, int32_t max_len, int32_t* d_len, int64_t* d_first,
                                 int64_t* d_last, void* stream) {
  API_BEGIN
  if (!ix || n < 0 || n >= kMaxBytes || (n && (!d_bytes || !d_len)) || (!d_first != !d_last))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^39 bytes; d_first and d_last go together)");
  int rc = check_device_handle(ix, kSubject);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  return run_match_stats(ix, n, d_bytes, max_len, d_len, d_first, d_last, nullptr, static_cast<hipStream_t>(stream));
  API_END
}

int femto_amd_match_stats_steps_device(femto_amd_index_t* ix, int64_t n, const uint8_t* d_bytes, int32_t max_len, int64_t* d_steps, void* stream) {
  API_BEGIN
  if (!ix || n < 0 || n >= kMaxBytes || (n && !d_bytes) || !d_steps) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^39 bytes)");
  int rc = check_device_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(d_steps, 0, 16, st));
  if (n == 0) return FEMTO_AMD_OK;
  return run_match_stats(ix, n, d_bytes, max_len, nullptr, nullptr, nullptr, reinterpret_cast<unsigned long long*>(d_steps), st);
  API_END
}

int femto_amd_common_sequences_device(femto_amd_index_t* ix, int64_t n, const int32_t* d_len, const int64_t* d_first, const int64_t* d_last,
                                      int32_t min_len, int64_t* d_seq_start, int32_t* d_seq_len, int64_t* d_seq_first, int64_t* d_seq_last,
                                      int64_t capacity, int64_t* d_total, void* stream) {
  API_BEGIN
  if (!ix || n < 0 || n >= kMaxBytes || capacity < 0 || !d_total || (n && !d_len) || (n && d_seq_first && !d_first) || (n && d_seq_last && !d_last))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^39 positions)");
  int rc = check_device_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(d_total, 0, 16, st));
    return FEMTO_AMD_OK;
  }
  return run_sequences(ix, n, d_len, d_first, d_last, min_len <= 0 ? kMinLen : min_len, d_seq_start, d_seq_len, d_seq_first, d_seq_last, capacity,
                       d_total, st);
  API_END
}

int femto_amd_common_groups_device(femto_amd_index_t* ix, int64_t capacity, const int64_t* d_total, const int64_t* d_seq_start,
                                   const int32_t* d_seq_len, const int64_t* d_seq_first, const int64_t* d_seq_last, int64_t* d_group_of,
                                   int32_t* d_g_len, int64_t* d_g_first, int64_t* d_g_last, int32_t* d_g_here, int64_t* d_g_min_start,
                                   int64_t* d_ngroups, void* stream) {
  API_BEGIN
  if (!ix || capacity < 0 || capacity >= kMaxSeqs || !d_ngroups || (capacity && (!d_total || !d_seq_start || !d_seq_len || !d_seq_first || !d_seq_last)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= capacity < 2^31 sequences)");
  int rc = check_device_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (capacity == 0) {
    HIP_TRY(hipMemsetAsync(d_ngroups, 0, 16, st));
    return FEMTO_AMD_OK;
  }
  return run_groups(ix, capacity, d_total, d_seq_start, d_seq_len, d_seq_first, d_seq_last,
                    GroupOut{d_group_of, d_g_len, d_g_first, d_g_last, d_g_here, d_g_min_start, d_ngroups}, st);
  API_END
}

int femto_amd_similar_documents_device(femto_amd_index_t* ix, int64_t ngroups_capacity, const int64_t* d_ngroups, const int32_t* d_g_len,
                                       const int64_t* d_g_first, const int64_t* d_g_last, const int32_t* d_g_here, const uint8_t* d_g_keep,
                                       int max_occs_each, int64_t* d_offsets, int64_t offsets_capacity, int64_t* d_doc_score, int32_t* d_doc_seqs,
                                       int64_t* d_total, void* stream) {
  API_BEGIN
  if (!ix || ngroups_capacity < 0 || ngroups_capacity >= kMaxSeqs || offsets_capacity < 0 || !d_doc_score || !d_doc_seqs || !d_total ||
      (offsets_capacity && !d_offsets) || (ngroups_capacity && (!d_ngroups || !d_g_len || !d_g_first || !d_g_last || !d_g_here)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= ngroups_capacity < 2^31 groups)");
  int rc = check_device_handle(ix, kSubject);
  if (rc) return rc;
  if ((rc = ensure_doc_ends(ix))) return rc;
  return run_documents(ix, ngroups_capacity, d_ngroups, d_g_len, d_g_first, d_g_last, d_g_here, d_g_keep, max_occs_each <= 0 ? kMaxOffsets : max_occs_each,
                       d_offsets, offsets_capacity, d_doc_score, d_doc_seqs, d_total, static_cast<hipStream_t>(stream));
  API_END
}

void femto_amd_similar_free(femto_amd_similar_result_t* out) {
  if (!out) return;
  free(out->len);
  free(out->g_len);
  free(out->g_first);
  free(out->g_last);
  free(out->g_here);
  free(out->g_min_start);
  free(out->g_kept);
  free(out->doc);
  free(out->doc_numerator);
  free(out->doc_seqs);
  free(out->doc_score);
  memset(out, 0, sizeof *out);
}

int femto_amd_similar(femto_amd_index_t* ix0, const uint8_t* bytes, int64_t n, int32_t min_len, int32_t max_len, int max_occs_each, int n_not,
                      femto_amd_index_t* const* not_ix, femto_amd_similar_result_t* out) {
  API_BEGIN
  if (!ix0 || !out || n < 0 || n >= kMaxSeqs || (n && !bytes) || n_not < 0 || (n_not && !not_ix))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 bytes)");
  memset(out, 0, sizeof *out);
  if (max_len > kKeyLen) return set_err(FEMTO_AMD_ERR_PARAM, "max_len may not exceed 65535 (the group key holds 16 bits of length)");
  for (int k = 0; k < n_not; k++)
    if (!not_ix[k]) return set_err(FEMTO_AMD_ERR_PARAM, "null stop-list handle");
  femto_amd_index* ix = replica0(ix0);
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  std::vector<femto_amd_index*> stops;
  for (int k = 0; k < n_not; k++) {
    femto_amd_index* s = replica0(not_ix[k]);
    if ((rc = check_plain_handle(s, "stop lists are"))) return rc;
    if (s->device != ix->device) return set_err(FEMTO_AMD_ERR_INVALID, "a stop-list handle must be on the device of the index");
    stops.push_back(s);
  }
  if (n == 0) return FEMTO_AMD_OK;
  if ((rc = ensure_doc_ends(ix))) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  const int mo = max_occs_each <= 0 ? kMaxOffsets : max_occs_each;
  const size_t un = size_t(n);
  hipStream_t st = nullptr;
  Temp T;
  uint8_t *d_buf, *d_keep;
  int32_t *d_len, *d_sl, *d_gl, *d_gh;
  int64_t *d_first, *d_last, *d_ss, *d_sf, *d_slast, *d_tot, *d_gf, *d_glast, *d_gms, *d_ng;
  // the query stands 8 bytes into a zeroed buffer: every aligned word the search reads lies inside it
  if ((rc = T.get(&d_buf, un + 16))) return rc;
  HIP_TRY(hipMemset(d_buf, 0, un + 16));
  HIP_TRY(hipMemcpy(d_buf + 8, bytes, un, hipMemcpyHostToDevice));
  const uint8_t* d_q = d_buf + 8;
  if ((rc = T.get(&d_len, un)) || (rc = T.get(&d_first, un)) || (rc = T.get(&d_last, un)) || (rc = T.get(&d_ss, un)) || (rc = T.get(&d_sl, un)) ||
      (rc = T.get(&d_sf, un)) || (rc = T.get(&d_slast, un)) || (rc = T.get(&d_tot, 2)) || (rc = T.get(&d_gl, un)) || (rc = T.get(&d_gf, un)) ||
      (rc = T.get(&d_glast, un)) || (rc = T.get(&d_gh, un)) || (rc = T.get(&d_gms, un)) || (rc = T.get(&d_ng, 2)))
    return rc;
  if ((rc = run_match_stats(ix, n, d_q, max_len, d_len, d_first, d_last, nullptr, st)) ||
      (rc = run_sequences(ix, n, d_len, d_first, d_last, min_len <= 0 ? kMinLen : min_len, d_ss, d_sl, d_sf, d_slast, n, d_tot, st)) ||
      (rc = run_groups(ix, n, d_tot, d_ss, d_sl, d_sf, d_slast, GroupOut{nullptr, d_gl, d_gf, d_glast, d_gh, d_gms, d_ng}, st)))
    return rc;
  std::vector<int32_t> h_len, g_len, g_here;
  std::vector<int64_t> g_first, g_last, g_ms;
  int64_t ng2[2] = {0, 0};
  if ((rc = to_host(h_len, d_len, un, st))) return rc;
  HIP_TRY(hipMemcpyAsync(ng2, d_ng, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t ng = ng2[0];
  const size_t ug = size_t(ng);
  if ((rc = to_host(g_len, d_gl, ug, st)) || (rc = to_host(g_first, d_gf, ug, st)) || (rc = to_host(g_last, d_glast, ug, st)) ||
      (rc = to_host(g_here, d_gh, ug, st)) || (rc = to_host(g_ms, d_gms, ug, st)))
    return rc;
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<uint8_t> keep(ug, 1);
  if (ng && !stops.empty()) {
    // the groups as patterns (the 16-byte slack femto_amd_count_device asks for), counted on every stop-list handle
    std::vector<int64_t> pstarts(ug + 1, 0);
    for (size_t g = 0; g < ug; g++) pstarts[g + 1] = pstarts[g] + g_len[g];
    const int64_t nsyms = pstarts[ug];
    int64_t *d_ps, *d_cf, *d_cl;
    uint16_t* d_pbuf;
    if ((rc = T.put(&d_ps, pstarts)) || (rc = T.get(&d_pbuf, size_t(nsyms) + 16)) || (rc = T.get(&d_cf, ug)) || (rc = T.get(&d_cl, ug)) ||
        (rc = T.put(&d_keep, keep)))
      return rc;
    HIP_TRY(hipMemset(d_pbuf, 0, (size_t(nsyms) + 16) * 2));
    if ((rc = launch(stop_gather_kernel, blocks_of(nsyms), st, ng, d_ps, d_gms, d_q, d_pbuf + 8))) return rc;
    for (femto_amd_index* s : stops)
      if ((rc = femto_amd_count_device(s, ng, d_gl, d_pbuf + 8, d_ps, d_cf, d_cl, st)) ||
          (rc = launch(stop_clear_kernel, blocks_of(ng), st, ng, d_cf, d_cl, d_keep)))
        return rc;
    HIP_TRY(hipMemcpyAsync(keep.data(), d_keep, ug, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  } else if ((rc = T.put(&d_keep, keep))) {
    return rc;
  }
  // the index score and the rows to locate
  int64_t numerator = 0, rows = 0;
  for (size_t g = 0; g < ug; g++) {
    if (!keep[g]) continue;
    const int64_t there = g_last[g] - g_first[g] + 1;
    numerator += int64_t(g_len[g]) * std::min<int64_t>(g_here[g], there);
    rows += g_last[g] - g_first[g] > int64_t(mo) ? int64_t(mo) : there;
  }
  const int64_t ndocuments = int64_t(ix->host.doc_ends.size());
  std::vector<int64_t> score;
  std::vector<int32_t> seqs;
  if (ng) {
    int64_t *d_offs, *d_score, *d_tot2;
    int32_t* d_seqs;
    if ((rc = T.get(&d_offs, size_t(rows))) || (rc = T.get(&d_score, size_t(ndocuments))) || (rc = T.get(&d_seqs, size_t(ndocuments))) ||
        (rc = T.get(&d_tot2, 2)))
      return rc;
    if ((rc = run_documents(ix, ng, d_ng, d_gl, d_gf, d_glast, d_gh, d_keep, mo, d_offs, rows, d_score, d_seqs, d_tot2, st)) ||
        (rc = to_host(score, d_score, size_t(ndocuments), st)) || (rc = to_host(seqs, d_seqs, size_t(ndocuments), st)))
      return rc;
    HIP_TRY(hipStreamSynchronize(st));
  }
  // documents with a score, best first
  struct Row {
    int64_t doc, num;
    int32_t seqs;
    double score;
  };
  std::vector<Row> docs;
  for (size_t d = 0; d < score.size(); d++) {
    if (!score[d]) continue;
    const int64_t doc_len = ix->host.doc_ends[d] - (d ? ix->host.doc_ends[d - 1] : 0) - 1;      // (without its SEOF: server.c:4176)
    const int64_t use = doc_len > 0 && doc_len < n ? doc_len : n;
    docs.push_back(Row{int64_t(d), score[d], seqs[d], double(score[d]) / double(use)});
  }
  std::sort(docs.begin(), docs.end(), [](const Row& a, const Row& b) { return a.score != b.score ? a.score > b.score : a.doc < b.doc; });
  std::vector<int64_t> o_doc, o_num;
  std::vector<int32_t> o_seqs;
  std::vector<double> o_score;
  for (const Row& r : docs) {
    o_doc.push_back(r.doc);
    o_num.push_back(r.num);
    o_seqs.push_back(r.seqs);
    o_score.push_back(r.score);
  }
  if ((rc = give(&out->len, h_len)) || (rc = give(&out->g_len, g_len)) || (rc = give(&out->g_first, g_first)) || (rc = give(&out->g_last, g_last)) ||
      (rc = give(&out->g_here, g_here)) || (rc = give(&out->g_min_start, g_ms)) || (rc = give(&out->g_kept, keep)) || (rc = give(&out->doc, o_doc)) ||
      (rc = give(&out->doc_numerator, o_num)) || (rc = give(&out->doc_seqs, o_seqs)) || (rc = give(&out->doc_score, o_score))) {
    femto_amd_similar_free(out);
    return rc;
  }
  out->n = n;
  out->ngroups = ng;
  out->ndocs = int64_t(docs.size());
  out->index_numerator = numerator;
  out->index_score = double(numerator) / double(n);
  return FEMTO_AMD_OK;
  API_END
}
