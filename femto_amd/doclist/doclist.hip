// doclist.hip -- which documents match: the located rows of every pattern as a sorted list of distinct documents (with the
// rows per document, and optionally every row as a (document, offset in document) pair), and AND / OR / NOT of such lists.
// The reference's results_create_sort_locations (src/main/results.c:213, order of compare_location_info, :199), the step
// do_range_to_results_query (src/main/server.c:4549) ends with, and intersectResults / unionResults / subtractResults
// (results.c:435 / 497 / 669).  include/femto_amd.h "document listing" states the semantics; DESIGN.md "Document listing"
// the layout.
//
// LISTING.  Input is what femto_amd_locate_device left in HBM: segment i = offsets[out_starts[i] .. out_starts[i + 1]).
// Documents are contiguous in the prepared text, so a segment sorted by text offset is sorted by (document, offset in
// document); an element starts a new document when the element before it lies in front of its document's start, and the
// rows of that document are the elements up to the first one at or beyond the document's end.  Three size classes, binned on
// the device (no host round trip):
//   n <= kWaveMax (64):   one wavefront per segment; bitonic sort across the lanes (__shfl_xor), heads by __ballot.
//   n <= kGroupMax (4096): one 256-thread workgroup per segment; bitonic sort of the keys in LDS (32 KB).  The wave kernel
//                          appends such segments to a list; a persistent grid takes them from it.
//   larger:                the wave kernel appends (begin, end) to a second list and reserves the segment's tiles of 4096 rows;
//                          rocPRIM's segmented radix sort (library sort, as in query_sort.hip) orders them into a scratch copy,
//                          then one workgroup per tile counts its heads, and a second pass writes with the counts of the
//                          tiles in front.  The launches are sized by host bounds (at most capacity / 4097 such segments).
// A segment whose bounds do not lie inside [0, min(total, capacity)] is treated as empty: nothing is addressed through it.
//
// SET OPERATIONS.  One workgroup per pair walks the stable merge of the two lists (a before b on ties) 256 positions at a
// time: a lane finds the element at its merge position by a diagonal binary search (merge path), decides from its neighbour
// in the other list whether the element belongs to the result, and a ballot scan gives its slot.  Count pass, device scan
// over the pairs, write pass.
//
// The searches (doc_of, first_ge, first_gt, merge_path_split) are ../common/ragged.hpp, the block sum, the rank of a flag and
// the two-word total ../common/block.hpp, the launches and the host forms' checks and copies ../common/host_common.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../common/block.hpp"

namespace femto_amd {
namespace {

constexpr int kWaveMax = 64;
constexpr int kGroupMax = 4096;
constexpr int kTile = 4096;

struct DlArgs {
  int64_t npats;
  const int64_t* out_starts;
  const int64_t* offsets;
  int64_t capacity;
  const int64_t* d_total;      // [0] rows, [1] overflow
  const int64_t* doc_ends;
  int64_t ndocs;
  int32_t* out_ndocs;          // never NULL (the scratch's when the caller passes none)
  int64_t* out_docs;           // the rest may be NULL
  int32_t* out_docs32;
  int32_t* out_hits;
  int64_t* out_pair_doc;
  int64_t* out_pair_off;
  int64_t* out_doc_total;
  int32_t* out_status;
  // binning
  unsigned long long* ctr;     // [0] mid segments, [1] big segments, [2] tiles
  int32_t* mid;                // mid_max
  int64_t mid_max;
  int64_t* big_beg;            // big_max each
  int64_t* big_end;
  int64_t* big_seg;
  int64_t* big_tile0;
  int64_t big_max;
  int32_t* tile_big;           // tile_max each
  int32_t* tile_heads;
  int64_t tile_max;
  const int64_t* sorted;       // the scratch copy the big segments are sorted into (indexed like offsets)
};

// rows the lists may address; -1: the input is incomplete (overflow flag, or more rows than the buffer holds)
__device__ __forceinline__ int64_t live_rows(const DlArgs& A) {
  const int64_t t = A.d_total[0];
  if (A.d_total[1] != 0 || t > A.capacity || t < 0) return -1;
  return t;
}

__device__ __forceinline__ bool segment_rows(const DlArgs& A, int64_t i, int64_t live, int64_t* s, int64_t* n) {
  const int64_t a = A.out_starts[i], b = A.out_starts[i + 1];
  *s = a;
  *n = 0;
  if (a < 0 || b < a || b > live) return false;
  *n = b - a;
  return true;
}

__device__ __forceinline__ void write_head(const DlArgs& A, int64_t slot, const Doc& d, int64_t hits) {
  if (A.out_docs) A.out_docs[slot] = d.doc;
  if (A.out_docs32) A.out_docs32[slot] = int32_t(d.doc);
  if (A.out_hits) A.out_hits[slot] = int32_t(hits);
}
__device__ __forceinline__ void write_pair(const DlArgs& A, int64_t slot, const Doc& d, int64_t off) {
  if (A.out_pair_doc) A.out_pair_doc[slot] = d.doc;
  if (A.out_pair_off) A.out_pair_off[slot] = off - d.start;
}

// clears the counters and the big-segment ranges (rocPRIM sorts big_max ranges: the unused ones must be empty), the status word
__global__ __launch_bounds__(256) void doclist_prep_kernel(const DlArgs A) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < A.big_max) A.big_beg[i] = A.big_end[i] = 0;
  if (i == 0) {
    A.ctr[0] = A.ctr[1] = A.ctr[2] = 0;
    const bool ok = live_rows(A) >= 0;
    if (A.out_status) *A.out_status = ok ? 0 : 1;
    if (ok && A.out_doc_total) *A.out_doc_total = 0;
  }
}

// one wavefront per segment: lists the segments of at most kWaveMax rows, bins the others
__global__ __launch_bounds__(256) void doclist_wave_kernel(const DlArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= A.npats) return;
  const int64_t live = live_rows(A);
  if (live < 0) return;
  int64_t s, n;
  segment_rows(A, i, live, &s, &n);
  if (n > kWaveMax) {
    if (lane != 0) return;
    A.out_ndocs[i] = 0;      // (stands when the segment finds no slot below: only with starts that overlap)
    if (n <= kGroupMax) {
      const unsigned long long k = atomicAdd(&A.ctr[0], 1ull);
      if (k < (unsigned long long)A.mid_max) A.mid[k] = int32_t(i);
    } else {
      const unsigned long long tiles = (unsigned long long)((n + kTile - 1) / kTile);
      const unsigned long long k = atomicAdd(&A.ctr[1], 1ull);
      if (k >= (unsigned long long)A.big_max) return;
      const unsigned long long t0 = atomicAdd(&A.ctr[2], tiles);
      if (t0 + tiles > (unsigned long long)A.tile_max) return;     // (the range stays empty)
      A.big_seg[k] = i;
      A.big_tile0[k] = int64_t(t0);
      A.big_beg[k] = s;
      A.big_end[k] = s + n;
    }
    return;
  }
  int64_t v = lane < n ? A.offsets[s + lane] : kPad;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int64_t o = __shfl_xor(v, j);
      const bool up = (lane & k) == 0, lower = (lane & j) == 0;
      v = (lower == up) ? (v < o ? v : o) : (v < o ? o : v);
    }
  }
  const bool valid = lane < n;
  Doc d{};
  if (valid) d = doc_of(A.doc_ends, A.ndocs, v);
  const int64_t prev = __shfl_up(v, 1);
  const bool head = valid && (lane == 0 || prev < d.start);
  const unsigned long long m = __ballot(head);
  if (lane == 0) A.out_ndocs[i] = __popcll(m);
  if (valid) write_pair(A, s + lane, d, v);
  if (head) {
    const unsigned long long above = lane == 63 ? 0ull : (m >> (lane + 1)) << (lane + 1);
    const int64_t next = above ? int64_t(__ffsll((long long)above) - 1) : n;
    write_head(A, s + __popcll(m & ((1ull << lane) - 1ull)), d, next - lane);
  }
}

// persistent grid over the list of mid segments: one workgroup sorts a segment in LDS
__global__ __launch_bounds__(256) void doclist_group_kernel(const DlArgs A) {
  __shared__ int64_t s_key[kGroupMax];
  __shared__ int s_wave[4];
  const int64_t live = live_rows(A);
  if (live < 0) return;
  unsigned long long nmid = A.ctr[0];
  if (nmid > (unsigned long long)A.mid_max) nmid = (unsigned long long)A.mid_max;
  for (int64_t k = blockIdx.x; k < int64_t(nmid); k += gridDim.x) {
    const int64_t i = A.mid[k];
    int64_t s, n64;
    segment_rows(A, i, live, &s, &n64);
    const int n = int(n64);                 // kWaveMax < n <= kGroupMax (the wave kernel's test)
    int npad = 128;
    while (npad < n) npad <<= 1;
    __syncthreads();                        // (the previous segment's keys have been read)
    for (int t = threadIdx.x; t < npad; t += 256) s_key[t] = t < n ? A.offsets[s + t] : kPad;
    __syncthreads();
    for (int kk = 2; kk <= npad; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < (npad >> 1); t += 256) {
          const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
          const int64_t x = s_key[a], y = s_key[b];
          if ((x > y) == ((a & kk) == 0)) {
            s_key[a] = y;
            s_key[b] = x;
          }
        }
        __syncthreads();
      }
    }
    int base = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
      const int t = t0 + threadIdx.x;
      const bool valid = t < n;
      Doc d{};
      int64_t v = 0;
      if (valid) {
        v = s_key[t];
        d = doc_of(A.doc_ends, A.ndocs, v);
        write_pair(A, s + t, d, v);
      }
      const bool head = valid && (t == 0 || s_key[t - 1] < d.start);
      int count;
      const int r = block_rank(head, s_wave, &count);
      if (head) write_head(A, s + base + r, d, first_ge(s_key, t + 1, n, d.end) - t);
      base += count;
    }
    if (threadIdx.x == 0) A.out_ndocs[i] = base;
  }
}

// tile -> its big segment
__global__ __launch_bounds__(256) void doclist_tiles_kernel(const DlArgs A) {
  if (live_rows(A) < 0) return;
  unsigned long long nbig = A.ctr[1];
  if (nbig > (unsigned long long)A.big_max) nbig = (unsigned long long)A.big_max;
  for (int64_t k = blockIdx.x; k < int64_t(nbig); k += gridDim.x) {
    const int64_t n = A.big_end[k] - A.big_beg[k], t0 = A.big_tile0[k];
    const int64_t tiles = (n + kTile - 1) / kTile;      // 0 for a segment that found no tiles
    for (int64_t t = threadIdx.x; t < tiles; t += 256) A.tile_big[t0 + t] = int32_t(k);
  }
}

// one workgroup per tile of a sorted big segment.  kWrite = false: the tile's heads; true: the lists, with the heads in front
template <bool kWrite>
__global__ __launch_bounds__(256) void doclist_tile_kernel(const DlArgs A) {
  __shared__ int s_wave[4];
  __shared__ int64_t s_sum[256];
  if (live_rows(A) < 0) return;
  unsigned long long ntiles = A.ctr[2];
  if (ntiles > (unsigned long long)A.tile_max) return;     // (overlapping starts: no tile map was completed)
  const int64_t tile = blockIdx.x;
  if (tile >= int64_t(ntiles)) return;
  const int64_t k = A.tile_big[tile];
  const int64_t s = A.big_beg[k], e = A.big_end[k], t0 = A.big_tile0[k];
  const int64_t lo = s + (tile - t0) * kTile, hi = lo + kTile < e ? lo + kTile : e;
  int64_t base = 0;
  if (kWrite) {
    int64_t part = 0;
    for (int64_t t = t0 + threadIdx.x; t < tile; t += 256) part += A.tile_heads[t];
    base = block_sum_i64(part, s_sum);
  }
  for (int64_t j0 = lo; j0 < hi; j0 += 256) {
    const int64_t j = j0 + threadIdx.x;
    const bool valid = j < hi;
    Doc d{};
    int64_t v = 0;
    if (valid) {
      v = A.sorted[j];
      d = doc_of(A.doc_ends, A.ndocs, v);
      if (kWrite) write_pair(A, j, d, v);
    }
    const bool head = valid && (j == s || A.sorted[j - 1] < d.start);
    int count;
    const int r = block_rank(head, s_wave, &count);
    if (kWrite && head) write_head(A, s + base + r, d, first_ge(A.sorted, j + 1, e, d.end) - j);
    base += count;
  }
  if (threadIdx.x == 0) {
    if (!kWrite) A.tile_heads[tile] = int32_t(base);
    else if (hi == e) A.out_ndocs[A.big_seg[k]] = int32_t(base);
  }
}

__global__ __launch_bounds__(256) void doclist_total_kernel(const DlArgs A) {
  __shared__ int64_t s_sum[256];
  if (live_rows(A) < 0) return;
  int64_t part = 0;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < A.npats; i += int64_t(gridDim.x) * 256) part += A.out_ndocs[i];
  const int64_t sum = block_sum_i64(part, s_sum);
  if (threadIdx.x == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long*>(A.out_doc_total), (unsigned long long)sum);
}

// ---- set operations -------------------------------------------------------------------------------------------------------

struct DsArgs {
  int64_t npairs;
  const int64_t* docs_a;
  const int64_t* a_start;
  const int32_t* a_n;
  const int64_t* docs_b;
  const int64_t* b_start;
  const int32_t* b_n;
  const int32_t* op;
  int64_t* counts;             // npairs (count pass)
  const int64_t* res_starts;   // npairs + 1 (write pass)
  int64_t* res_docs;
  int64_t res_capacity;
  int64_t* res_total;
};

// kWrite = false: counts[k] = size of pair k's result; true: the results at res_starts[k], and res_total
template <bool kWrite>
__global__ __launch_bounds__(256) void docset_kernel(const DsArgs A) {
  __shared__ int s_wave[4];
  if (kWrite && blockIdx.x == 0 && threadIdx.x == 0) write_total(A.res_total, A.res_starts[A.npairs], A.res_capacity);
  for (int64_t k = blockIdx.x; k < A.npairs; k += gridDim.x) {
    const int64_t na = A.a_n[k] > 0 ? A.a_n[k] : 0, nb = A.b_n[k] > 0 ? A.b_n[k] : 0;
    const int64_t* a = A.docs_a + A.a_start[k];
    const int64_t* b = A.docs_b + A.b_start[k];
    const int op = A.op[k];
    const int64_t out0 = kWrite ? A.res_starts[k] : 0;
    int64_t base = 0;
    for (int64_t p0 = 0; p0 < na + nb; p0 += 256) {
      const int64_t p = p0 + threadIdx.x;
      bool keep = false;
      int64_t v = 0;
      if (p < na + nb) {
        // i = elements of a among the first p of the stable merge (a before b on ties)
        const int64_t i = merge_path_split(p, na, nb, [&](int64_t x, int64_t y) { return a[x] <= b[y]; }), j = p - i;
        const bool from_a = i < na && (j >= nb || a[i] <= b[j]);
        if (from_a) {
          v = a[i];
          const bool in_b = j < nb && b[j] == v;       // b[j]: the first element of b that is >= a[i]
          keep = op == FEMTO_AMD_DOCSET_AND ? in_b : (op == FEMTO_AMD_DOCSET_OR ? true : (op == FEMTO_AMD_DOCSET_NOT ? !in_b : false));
        } else {
          v = b[j];
          keep = op == FEMTO_AMD_DOCSET_OR && !(i > 0 && a[i - 1] == v);   // a[i - 1]: the last element of a that is <= b[j]
        }
      }
      int count;
      const int r = block_rank(keep, s_wave, &count);
      if (kWrite && keep) {
        const int64_t slot = out0 + base + r;
        if (slot >= 0 && slot < A.res_capacity) A.res_docs[slot] = v;
      }
      base += count;
    }
    if (!kWrite && threadIdx.x == 0) A.counts[k] = base;
  }
}

// packs ragged lists: row j of the ragged array (segment i = the last with out_starts[i] <= j) goes to doc_starts[i] + r when
// r = j - out_starts[i] < ndocs[i]
__global__ __launch_bounds__(256) void doclist_pack_kernel(const int64_t npats, const int64_t total, const int64_t* __restrict__ out_starts,
                                                           const int32_t* __restrict__ ndocs, const int64_t* __restrict__ doc_starts,
                                                           const int64_t* __restrict__ docs, const int32_t* __restrict__ hits,
                                                           int64_t* __restrict__ docs_out, int32_t* __restrict__ hits_out) {
  for (int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x; j < total; j += int64_t(gridDim.x) * 256) {
    const int64_t lo = first_gt(out_starts + 1, 0, npats, j);       // first i with out_starts[i + 1] > j
    if (lo >= npats) continue;
    const int64_t r = j - out_starts[lo];
    if (r < 0 || r >= ndocs[lo]) continue;
    docs_out[doc_starts[lo] + r] = docs[j];
    hits_out[doc_starts[lo] + r] = hits[j];
  }
}

__global__ __launch_bounds__(256) void widen_kernel(const int64_t n, const int32_t* __restrict__ in, int64_t* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// ---- host side --------------------------------------------------------------------------------------------------------------

constexpr const char* kSubject = "document listing is";

int sort_bits(int64_t total_length) {
  int b = 1;
  while (b < 63 && (int64_t(1) << b) <= total_length) b++;
  return b;
}

int run_doclist(femto_amd_index* ix, Scratch& S, int64_t npats, const int64_t* d_out_starts, const int64_t* d_offsets, int64_t capacity,
                const int64_t* d_total, int32_t* d_ndocs, int64_t* d_docs, int32_t* d_docs32, int32_t* d_hits, int64_t* d_pair_doc,
                int64_t* d_pair_off, int64_t* d_doc_total, int32_t* d_status, hipStream_t st) {
  int rc;
  if (d_docs32 && ix->host.doc_ends.size() >= (size_t(1) << 31))
    return set_err(FEMTO_AMD_ERR_PARAM, "32-bit document numbers need an index of fewer than 2^31 documents: pass d_docs");
  if (npats >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "too many patterns in one call: split the batch");
  if ((rc = ensure_doc_ends(ix))) return rc;
  DlArgs A{};
  A.npats = npats;
  A.out_starts = d_out_starts;
  A.offsets = d_offsets;
  A.capacity = capacity;
  A.d_total = d_total;
  A.doc_ends = ix->d_doc_ends;
  A.ndocs = int64_t(ix->host.doc_ends.size());
  A.out_docs = d_docs;
  A.out_docs32 = d_docs32;
  A.out_hits = d_hits;
  A.out_pair_doc = d_pair_doc;
  A.out_pair_off = d_pair_off;
  A.out_doc_total = d_doc_total;
  A.out_status = d_status;
  A.mid_max = std::min(npats, capacity / (kWaveMax + 1));
  A.big_max = std::min(npats, capacity / (kGroupMax + 1));
  A.tile_max = A.big_max ? capacity / kTile + A.big_max : 0;
  if (A.big_max && capacity >= (int64_t(1) << 32))
    return set_err(FEMTO_AMD_ERR_PARAM, "segments of more than 4096 rows need a row buffer of fewer than 2^32 rows: split the batch");
  if (A.tile_max >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "too many rows in one call: split the batch");
  if ((rc = S.tail.reserve(64)) || (rc = S.idx.reserve(size_t(A.mid_max) * 4 + 16)) || (rc = S.keys2.reserve(size_t(A.big_max) * 32 + 16)) ||
      (rc = S.idx2.reserve(size_t(A.tile_max) * 8 + 16)))
    return rc;
  if (!d_ndocs) {
    if ((rc = S.noccs.reserve(size_t(npats) * 4))) return rc;
    d_ndocs = S.noccs.as<int32_t>();
  }
  A.out_ndocs = d_ndocs;
  A.ctr = S.tail.as<unsigned long long>();
  A.mid = S.idx.as<int32_t>();
  A.big_beg = S.keys2.as<int64_t>();
  A.big_end = A.big_beg + A.big_max;
  A.big_seg = A.big_end + A.big_max;
  A.big_tile0 = A.big_seg + A.big_max;
  A.tile_big = S.idx2.as<int32_t>();
  A.tile_heads = A.tile_big + A.tile_max;
  size_t tmp_bytes = 0;
  const int bits = sort_bits(ix->host.total_length);
  if (A.big_max) {
    if ((rc = S.keys.reserve(size_t(capacity) * 8))) return rc;
    A.sorted = S.keys.as<int64_t>();
    HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                               size_t(capacity), static_cast<unsigned int>(A.big_max), A.big_beg, A.big_end, 0u, unsigned(bits), st));
    if ((rc = S.sorttmp.reserve(tmp_bytes ? tmp_bytes : 16))) return rc;
  }
  if ((rc = launch(doclist_prep_kernel, blocks_of(std::max<int64_t>(A.big_max, 1)), st, A)) ||
      (rc = launch(doclist_wave_kernel, dim3(uint32_t((npats + 3) / 4)), st, A)))
    return rc;
  if (A.mid_max && (rc = launch(doclist_group_kernel, persistent_grid(ix, A.mid_max), st, A))) return rc;
  if (A.big_max) {
    HIP_TRY(rocprim::segmented_radix_sort_keys(S.sorttmp.p, tmp_bytes, reinterpret_cast<const uint64_t*>(d_offsets), S.keys.as<uint64_t>(),
                                               size_t(capacity), static_cast<unsigned int>(A.big_max), A.big_beg, A.big_end, 0u, unsigned(bits), st));
    if ((rc = launch(doclist_tiles_kernel, persistent_grid(ix, A.big_max), st, A)) ||
        (rc = launch(doclist_tile_kernel<false>, dim3(uint32_t(A.tile_max)), st, A)) ||
        (rc = launch(doclist_tile_kernel<true>, dim3(uint32_t(A.tile_max)), st, A)))
      return rc;
  }
  if (d_doc_total && (rc = launch(doclist_total_kernel, persistent_grid(ix, (npats + 1023) / 1024), st, A))) return rc;
  return 0;
}

int run_docset(femto_amd_index* ix, Scratch& S, int64_t npairs, const int64_t* d_docs_a, const int64_t* d_a_start, const int32_t* d_a_n,
               const int64_t* d_docs_b, const int64_t* d_b_start, const int32_t* d_b_n, const int32_t* d_op, int64_t* d_res_starts,
               int64_t* d_res_docs, int64_t res_capacity, int64_t* d_res_total, hipStream_t st) {
  int rc;
  if ((rc = S.noccs64.reserve(size_t(npairs) * 8))) return rc;
  const DsArgs A{npairs, d_docs_a, d_a_start, d_a_n, d_docs_b, d_b_start, d_b_n, d_op, S.noccs64.as<int64_t>(), d_res_starts, d_res_docs,
                 res_capacity, d_res_total};
  const dim3 grid = persistent_grid(ix, npairs);
  if ((rc = launch(docset_kernel<false>, grid, st, A)) || (rc = device_scan(S.scan, npairs, A.counts, d_res_starts, 0, st))) return rc;
  return launch(docset_kernel<true>, grid, st, A);
}

}  // namespace
}  // namespace femto_amd

int femto_amd_doclist_info(int* wave_max, int* workgroup_max) {
  if (wave_max) *wave_max = kWaveMax;
  if (workgroup_max) *workgroup_max = kGroupMax;
  return FEMTO_AMD_OK;
}

int femto_amd_doclist_device(femto_amd_index_t* ix, int64_t npats, const int64_t* d_out_starts, const int64_t* d_offsets, int64_t capacity,
                             const int64_t* d_total, int32_t* d_ndocs, int64_t* d_docs, int32_t* d_docs32, int32_t* d_hits,
                             int64_t* d_pair_doc, int64_t* d_pair_off, int64_t* d_doc_total, int32_t* d_status, void* stream) {
  API_BEGIN
  if (!ix || npats < 0 || capacity < 0 || (npats && (!d_out_starts || !d_total || (capacity && !d_offsets))))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (!ix->children.empty()) return refuse_multi_device();
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  if (npats == 0) return FEMTO_AMD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Lease L(ix, st);
  if (!L.s) return L.rc;
  return run_doclist(ix, *L.s, npats, d_out_starts, d_offsets, capacity, d_total, d_ndocs, d_docs, d_docs32, d_hits, d_pair_doc, d_pair_off,
                     d_doc_total, d_status, st);
  API_END
}

int femto_amd_docset_device(femto_amd_index_t* ix, int64_t npairs, const int64_t* d_docs_a, const int64_t* d_a_start, const int32_t* d_a_n,
                            const int64_t* d_docs_b, const int64_t* d_b_start, const int32_t* d_b_n, const int32_t* d_op,
                            int64_t* d_res_starts, int64_t* d_res_docs, int64_t res_capacity, int64_t* d_res_total, void* stream) {
  API_BEGIN
  if (!ix || npairs < 0 || res_capacity < 0 || !d_res_starts || !d_res_total || (res_capacity && !d_res_docs) ||
      (npairs && (!d_docs_a || !d_a_start || !d_a_n || !d_docs_b || !d_b_start || !d_b_n || !d_op)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (!ix->children.empty()) return refuse_multi_device();
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npairs == 0) return empty_result_async(d_res_starts, d_res_total, st);
  Lease L(ix, st);
  if (!L.s) return L.rc;
  return run_docset(ix, *L.s, npairs, d_docs_a, d_a_start, d_a_n, d_docs_b, d_b_start, d_b_n, d_op, d_res_starts, d_res_docs, res_capacity,
                    d_res_total, st);
  API_END
}

int femto_amd_doclist(femto_amd_index_t* ix0, int64_t npats, const int32_t* plen, const uint16_t* pats, const int64_t* starts, int max_occs_each,
                      int64_t* doc_starts, int64_t** docs, int32_t** hits, int64_t* total) {
  API_BEGIN
  if (!ix0 || npats < 0 || !doc_starts || !docs || !total || (npats && (!plen || !pats || !starts)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *docs = nullptr;
  if (hits) *hits = nullptr;
  *total = 0;
  doc_starts[0] = 0;
  femto_amd_index* ix = replica0(ix0);
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  if (npats == 0) return FEMTO_AMD_OK;
  int64_t nsyms;
  if ((rc = check_patterns(npats, plen, pats, starts, &nsyms))) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  int32_t *d_plen, *d_ndocs, *d_hits, *d_hits_p;
  uint16_t* d_pats;
  int64_t *d_starts, *d_docs, *d_docs_p, *d_ndocs64, *d_dstarts;
  LocatedRows R;
  if ((rc = upload_patterns(T, npats, plen, starts, nsyms, {{pats, nsyms, 0}}, &d_plen, &d_pats, &d_starts)) ||
      (rc = locate_rows(ix, T, npats, d_plen, d_pats, d_starts, max_occs_each, &R)) || (rc = T.get(&d_docs, size_t(R.rows))) ||
      (rc = T.get(&d_hits, size_t(R.rows))) || (rc = T.get(&d_ndocs, size_t(npats))) || (rc = T.get(&d_ndocs64, size_t(npats))) ||
      (rc = T.get(&d_dstarts, size_t(npats) + 1)))
    return rc;
  const int64_t rows = R.rows;
  HIP_TRY(hipDeviceSynchronize());
  {
    Lease L(ix);
    if (!L.s) return L.rc;
    Scratch& S = *L.s;
    hipStream_t st = S.stream;
    if ((rc = run_doclist(ix, S, npats, R.ostarts, R.offs, rows, R.tot, d_ndocs, d_docs, nullptr, d_hits, nullptr, nullptr, nullptr, nullptr, st)))
      return rc;
    if ((rc = launch(widen_kernel, blocks_of(npats), st, npats, d_ndocs, d_ndocs64)) || (rc = device_scan(S.scan, npats, d_ndocs64, d_dstarts, 0, st)))
      return rc;
    HIP_TRY(hipMemcpyAsync(doc_starts, d_dstarts, size_t(npats + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t nd = doc_starts[npats];
    *total = nd;
    if (nd == 0) return FEMTO_AMD_OK;
    if ((rc = T.get(&d_docs_p, size_t(nd))) || (rc = T.get(&d_hits_p, size_t(nd)))) return rc;
    if ((rc = launch(doclist_pack_kernel, persistent_grid(ix, (rows + 255) / 256), st, npats, rows, R.ostarts, d_ndocs, d_dstarts, d_docs, d_hits,
                     d_docs_p, d_hits_p)) ||
        (rc = list_to_host(nd, d_docs_p, st, "copying the lists back", docs)))
      return rc;
    if (hits && (rc = list_to_host(nd, d_hits_p, st, "copying the lists back", hits))) {
      free(*docs);
      *docs = nullptr;
      return rc;
    }
  }
  return FEMTO_AMD_OK;
  API_END
}

int femto_amd_docset(femto_amd_index_t* ix0, int64_t npairs, const int64_t* docs_a, const int64_t* a_start, const int32_t* a_n,
                     const int64_t* docs_b, const int64_t* b_start, const int32_t* b_n, const int32_t* op, int64_t* res_starts,
                     int64_t** res_docs, int64_t* total) {
  API_BEGIN
  if (!ix0 || npairs < 0 || !res_starts || !res_docs || !total || (npairs && (!docs_a || !a_start || !a_n || !docs_b || !b_start || !b_n || !op)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *res_docs = nullptr;
  *total = 0;
  res_starts[0] = 0;
  femto_amd_index* ix = replica0(ix0);
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  if (npairs == 0) return FEMTO_AMD_OK;
  int64_t la, lb, bound = 0;
  if ((rc = check_list_pairs(npairs, a_start, a_n, b_start, b_n, &la, &lb))) return rc;
  for (int64_t k = 0; k < npairs; k++) {
    if (op[k] != FEMTO_AMD_DOCSET_AND && op[k] != FEMTO_AMD_DOCSET_OR && op[k] != FEMTO_AMD_DOCSET_NOT)
      return set_err(FEMTO_AMD_ERR_PARAM, "unknown set operation");
    bound += op[k] == FEMTO_AMD_DOCSET_OR ? int64_t(a_n[k]) + b_n[k] : int64_t(a_n[k]);
  }
  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  int64_t *d_a, *d_b, *d_as, *d_bs, *d_rs, *d_rd, *d_rt;
  int32_t *d_an, *d_bn, *d_op;
  const size_t np = size_t(npairs);
  if ((rc = T.put(&d_a, docs_a, size_t(la))) || (rc = T.put(&d_b, docs_b, size_t(lb))) || (rc = T.put(&d_as, a_start, np)) ||
      (rc = T.put(&d_bs, b_start, np)) || (rc = T.put(&d_an, a_n, np)) || (rc = T.put(&d_bn, b_n, np)) || (rc = T.put(&d_op, op, np)) ||
      (rc = T.get(&d_rs, np + 1)) || (rc = T.get(&d_rd, size_t(bound))) || (rc = T.get(&d_rt, 2)))
    return rc;
  Lease L(ix);
  if (!L.s) return L.rc;
  hipStream_t st = L.s->stream;
  if ((rc = run_docset(ix, *L.s, npairs, d_a, d_as, d_an, d_b, d_bs, d_bn, d_op, d_rs, d_rd, bound, d_rt, st))) return rc;
  HIP_TRY(hipMemcpyAsync(res_starts, d_rs, size_t(npairs + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t n = res_starts[npairs];
  *total = n;
  if (n == 0) return FEMTO_AMD_OK;
  return list_to_host(n, d_rd, st, "copying the results back", res_docs);
  API_END
}
