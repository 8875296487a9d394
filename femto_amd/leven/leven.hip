// leven.hip -- occurrences within k edits by exact seeds: for every pattern of a batch, the text offsets where a string within
// Levenshtein distance k of it starts, each with the least cost and the shortest length that reaches it.  include/femto_amd.h
// "occurrences within k edits" states the contract; DESIGN.md "Occurrences within k edits" the kernel, its registers and the figures.
//
// THE ROUTE is ../hamming/hamming.hip's with another check.  k edits touch at most k of the k + 1 pieces of a pattern, so one piece
// stands unchanged in the text: the pieces are LOCATED exactly and every located offset o of a piece j = [b0, b1) is extended with
// edits to the right and to the left.  What stands in front of the extension and around it is ../common/seeds.hpp's: the piece
// table, the work area, the one row-free locate call, the candidates, the driver of the check over both paths and the checks and
// the prologue of the two forms.  This file keeps the extension, the records, the order tail and the two passes of the host form.
// EXTEND.  One lane per candidate.  RIGHT: the pattern behind the piece against the text from o + (b1 - b0), anchored at its start:
// cr = the least cost at which all of it is consumed, tr = the fewest text symbols that reach cr.  LEFT: the pattern in front of
// the piece, reversed, against the text backwards from o - 1, with k - cr edits to spend: for every number t of text symbols,
// cl(t) = the least cost at which all of it is consumed.  A RAW RECORD (pattern, o - t, cl(t) + cr, t + (b1 - b0) + tr) is emitted
// for every t with cl(t) + cr <= k.  The least (cost, length) over an offset's raw records is the answer for that offset
// (tests/test_leven_host.py replays this route in numpy against the definition).
// Both extensions are one routine, diagonal-wise and furthest-reaching (Landau-Vishkin): for e = 0 .. budget and the diagonals
// d = -e .. e (text symbols minus pattern symbols consumed) the furthest pattern row that e edits reach, slid along the exact
// matches.  A step that consumes a text symbol (substitution, insertion) checks that it is a byte character inside the text: an
// exact match cannot step over SEOF, because the pattern holds bytes only.  The per-lane row of 2 k + 3 entries is indexed at run
// time, so it lives in LDS (2 bytes an entry, lanes interleaved), sized by k at the launch; one row updated in place, the old
// left neighbour kept in a register.  False candidates die after k + 1 rounds of short slides.
// ORDER AND DE-DUPLICATION.  The stage of ../common/result_order.hpp sorts the raw records by (pattern, offset, cost, length); the
// first of each (pattern, offset) is a result (edit.hip's heads: flags, their scan, a gather); result_start is found in the
// sorted pattern keys.
// SAMPLE PATH.  No text in HBM: the windows [p - k, p + m + k) of a chunk of candidates, clipped to the text, are extracted
// (femto_amd_extract_device) into a buffer of fixed stride and the same extension runs over alpha codes.  This path reads the
// candidate total back and allocates.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../common/block.hpp"
#include "../common/result_order.hpp"
#include "../extract/extractor.hpp"
#include "../common/seeds.hpp"

namespace femto_amd {
namespace {

using namespace seeds;

constexpr int kMaxK = 31;      // the cost in five bits of the sort key, length - (m - k) in six
const char* const kBadK = "k must be 0 .. 31 edits";

// the shared area with the order stage's buffers and, on top of it, the raw records
struct Work : OrderArea {
  DeviceBuffer raw, r_off, r_pat, r_meta;
  ~Work() override { for (DeviceBuffer* b : {&raw, &r_off, &r_pat, &r_meta}) b->release(); }
};

// ---- extend ---------------------------------------------------------------------------------------------------------------------

// the raw records as the lanes emit them (any order); meta = cost << 22 | (length - (m - k)) << 16 | length.  *total counts every
// emit, whether its record found a slot or not
struct Records {
  int64_t* off;
  uint32_t* pat;
  uint32_t* meta;
  unsigned long long* total;
  int64_t npat, capacity;
};

__device__ __forceinline__ void emit(const Records& R, int64_t q, int64_t p, int cost, int length, int shortest) {
  const int64_t slot = int64_t(atomicAdd(R.total, 1ull));
  if (slot >= R.capacity) return;
  R.off[slot] = p;
  R.pat[slot] = uint32_t(q);
  R.meta[slot] = (uint32_t(cost) << 22) | (uint32_t(length - shortest) << 16) | uint32_t(length);
}

// One extension.  pat(i) = the i-th of mp pattern symbols, text(x) = the alpha code of the x-th text symbol in the direction of
// the extension, 0 where the text ends.  row: this lane's 2 k + 3 entries, entry x at row[x * 256]; entry k + 1 + d holds the
// furthest pattern row reached on diagonal d, plus one (0: not reached).  reached(e, d) is called when diagonal d consumes the whole
// pattern with e edits and did not with e - 1 (mp + d text symbols are consumed then); the extension ends when it returns true.
template <class PatAt, class TextAt, class Reached>
__device__ __forceinline__ void extend(uint16_t* __restrict__ row, const int k, const int mp, const int budget, PatAt pat, TextAt text,
                                       Reached reached) {
  const int base = k + 1;
  for (int x = base - budget - 1; x <= base + budget + 1; x++) row[x * 256] = 0;
  int i = 0;
  while (i < mp && pat(i) == text(i)) i++;
  row[base * 256] = uint16_t(i + 1);
  if (i == mp && reached(0, 0)) return;
  for (int e = 1; e <= budget; e++) {
    int left = -1;      // diagonal d - 1 as round e - 1 left it
    for (int d = -e; d <= e; d++) {
      const int cur = int(row[(base + d) * 256]) - 1, right = int(row[(base + d + 1) * 256]) - 1;
      i = cur;
      // every row up to the furthest of a diagonal is reached, so a step that the pattern's or the text's end forbids from the
      // furthest row is taken from the row in front of it
      if (cur >= 0 && cur < mp && text(cur + d) >= kByte0) i = cur + 1;      // a substitution
      if (left > i) {                                                           // a text symbol the pattern lacks
        const int c = text(left + d - 1) >= kByte0 ? left : left - 1;
        if (c > i) i = c;
      }
      if (right >= 0) {                                                         // a pattern symbol the text lacks
        const int c = right < mp ? right + 1 : mp;
        if (c > i && c + d >= 0) i = c;
      }
      left = cur;
      if (i == cur) continue;      // (not reached, or no further than before: the slide from there was taken then)
      while (i < mp && pat(i) == text(i + d)) i++;
      row[(base + d) * 256] = uint16_t(i + 1);
      if (i == mp && reached(e, d)) return;
    }
  }
}

struct TextSrc {
  const uint8_t* txt;        // one dense code per position
  // the alpha code of T[pos], 0 outside the text
  __device__ __forceinline__ auto text(const Seeds& S, const Cand&, int, int64_t, const uint16_t* s_alpha) const {
    const uint8_t* t = txt;
    const int64_t N = S.N;
    return [=](int64_t pos) -> uint32_t { return pos >= 0 && pos < N ? uint32_t(s_alpha[t[pos]]) : 0u; };
  }
};

// the window of a candidate on the sample path: [p - k, p + m + k), clipped to the text
__device__ __forceinline__ void window_of(const Seeds& S, const Cand& C, int k, int64_t* w0, int64_t* w1) {
  *w0 = C.p - k > 0 ? C.p - k : 0;
  *w1 = C.p + C.m + k < S.N ? C.p + C.m + k : S.N;
}

struct CtxSrc {
  const uint16_t* ctx;       // the window of candidate c0 + i at ctx[i * stride]
  int64_t stride;
  __device__ __forceinline__ auto text(const Seeds& S, const Cand& C, int k, int64_t local, const uint16_t*) const {
    int64_t w0, w1;
    window_of(S, C, k, &w0, &w1);
    const uint16_t* t = ctx + local * stride - w0;
    return [=](int64_t pos) -> uint32_t { return pos >= w0 && pos < w1 ? uint32_t(t[pos]) : 0u; };
  }
};

// candidates [c0, c0 + n) of the chain's output, a grid that strides over them.  Dynamic LDS: (2 k + 3) * 256 uint16
template <class Src>
__global__ __launch_bounds__(256) void extend_kernel(const Src src, const Seeds S, const int64_t c0, const int64_t n, const int k,
                                                     const uint16_t* __restrict__ alpha, const Records R) {
  extern __shared__ uint16_t s_rows[];
  __shared__ uint16_t s_alpha[256];
  s_alpha[threadIdx.x] = alpha ? alpha[threadIdx.x] : uint16_t(0);
  __syncthreads();
  if (S.total[1]) return;
  uint16_t* const row = s_rows + threadIdx.x;
  const int64_t live = S.total[0] - c0 < n ? S.total[0] - c0 : n;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < live; i += int64_t(gridDim.x) * 256) {
    Cand C;
    if (!seed_of(S, c0 + i, &C)) continue;
    const int b0 = C.j * C.m / S.kp1, b1 = (C.j + 1) * C.m / S.kp1, mr = C.m - b1;
    const int64_t o = C.p + b0, behind = o + (b1 - b0);
    const uint16_t* __restrict__ const pat = S.syms + C.s;
    const auto text = src.text(S, C, k, i, s_alpha);
    int cr = -1, tr = 0;
    extend(row, k, mr, k, [=](int x) -> uint32_t { return pat[b1 + x]; }, [=](int x) -> uint32_t { return text(behind + x); },
           [&](int e, int d) {
             cr = e;
             tr = mr + d;      // (the diagonals of a round ascend: the first to arrive consumed the fewest text symbols)
             return true;
           });
    if (cr < 0) continue;
    const int fixed = (b1 - b0) + tr, shortest = C.m - k;
    const int64_t q = C.q;
    extend(row, k, b0, k - cr, [=](int x) -> uint32_t { return pat[b0 - 1 - x]; }, [=](int x) -> uint32_t { return text(o - 1 - x); },
           [&](int e, int d) {
             const int t = b0 + d;
             emit(R, q, o - t, e + cr, t + fixed, shortest);
             return false;
           });
  }
}

// sample path: the window of every served candidate, wherever its piece was found
struct LevenWindow {
  __device__ __forceinline__ static bool of(const Seeds& S, int64_t c, int k, int64_t* w0, int64_t* w1) {
    Cand C;
    if (!seed_of(S, c, &C)) return false;
    window_of(S, C, k, w0, w1);
    return true;
  }
};

// ---- order and de-duplication ---------------------------------------------------------------------------------------------------

// the first sort's key of a raw record: offset << 11 | cost << 6 | length - (m - k)
struct OffsetKey {
  const int64_t* off;
  const uint32_t* meta;
  __device__ __forceinline__ uint64_t operator()(int64_t slot) const { return (uint64_t(off[slot]) << 11) | uint64_t(meta[slot] >> 16); }
};

// flags[s] = 1 at the first record of every (pattern, offset) in sorted order: the least cost and, at that cost, the shortest length
__global__ __launch_bounds__(256) void head_kernel(const Records R, const uint32_t* __restrict__ idx, int64_t* __restrict__ flags) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= R.capacity) return;
  bool head = s < live_records(R.total, R.capacity);
  if (head && s > 0) {
    const uint32_t a = idx[s], b = idx[s - 1];
    head = R.pat[a] != R.pat[b] || R.off[a] != R.off[b];
  }
  flags[s] = head ? 1 : 0;
}

struct Out {
  int64_t* offset;
  int32_t *cost, *length;
};

__global__ __launch_bounds__(256) void gather_kernel(const Records R, const uint32_t* __restrict__ idx, const int64_t* __restrict__ scan, const Out out) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= live_records(R.total, R.capacity)) return;
  const int64_t at = scan[s];
  if (scan[s + 1] == at) return;      // no head
  const uint32_t r = idx[s], meta = R.meta[r];
  out.offset[at] = R.off[r];
  out.cost[at] = int32_t(meta >> 22);
  out.length[at] = int32_t(meta & 0xffffu);
}

// result_start[q] = the heads in front of the first sorted record of a pattern >= q; pkeys: the sorted pattern keys of the capacity slots
__global__ __launch_bounds__(256) void result_start_kernel(const Records R, const uint32_t* __restrict__ pkeys, const int64_t* __restrict__ scan,
                                                           int64_t* __restrict__ result_start) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (q > R.npat) return;
  int64_t lo = 0, hi = R.capacity;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (int64_t(pkeys[mid]) < q) lo = mid + 1; else hi = mid;
  }
  result_start[q] = scan[lo];
}

// {distinct results, raw > capacity, raw, candidates, candidates > cand_capacity}; scan = the heads' exclusive scan over the capacity
// slots, NULL for the counting form
__global__ __launch_bounds__(256) void total_kernel(const Records R, const int64_t* __restrict__ scan, const int64_t* __restrict__ seeds_total,
                                                    int64_t* __restrict__ d_total) {
  if (blockIdx.x || threadIdx.x) return;
  const int64_t raw = int64_t(R.total[0]);
  d_total[0] = scan ? scan[R.capacity] : 0;
  d_total[1] = raw > R.capacity ? 1 : 0;
  d_total[2] = raw;
  d_total[3] = seeds_total[0];
  d_total[4] = seeds_total[1];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// a checked launch of 256-thread workgroups with the LDS rows of bound k behind the static LDS
template <class Src>
int launch_extend(dim3 grid, hipStream_t st, const Src& src, const Seeds& S, int64_t c0, int64_t n, int k, const uint16_t* alpha, const Records& R) {
  extend_kernel<Src><<<grid, dim3(256), size_t(2 * k + 3) * 256 * sizeof(uint16_t), st>>>(src, S, c0, n, k, alpha, R);
  HIP_TRY(hipGetLastError());
  return FEMTO_AMD_OK;
}

int run_leven(femto_amd_extractor* ex, Work& W, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
              int64_t cand_capacity, int64_t capacity, int64_t* d_result_start, const Out& out, int64_t* d_total, hipStream_t st) {
  const size_t cap = size_t(capacity);
  Turn turn(W, st);
  int rc = turn.rc;
  if (rc) return rc;
  if ((rc = W.raw.reserve(8)) || (rc = W.r_off.reserve(cap * 8 + 8)) || (rc = W.r_pat.reserve(cap * 4 + 8)) || (rc = W.r_meta.reserve(cap * 4 + 8)))
    return rc;
  const Records R{W.r_off.as<int64_t>(), W.r_pat.as<uint32_t>(), W.r_meta.as<uint32_t>(), W.raw.as<unsigned long long>(), npat, capacity};
  // (the extension compares alpha codes: the piece table makes no dense codes)
  Seeds S;
  if ((rc = locate_seeds(ex, W, npat, nsyms, d_syms, d_starts, k, false, cand_capacity, R.total, 8, st, &S))) return rc;
  const auto on_text = [&](dim3 grid) { return launch_extend(grid, st, TextSrc{ex->ix->d_txt}, S, int64_t(0), cand_capacity, k, ex->d_alpha, R); };
  const auto on_samples = [&](const uint16_t* w_syms, int64_t stride, int64_t c0, int64_t cn) {
    return launch_extend(blocks_of(cn), st, CtxSrc{w_syms, stride}, S, c0, cn, k, static_cast<const uint16_t*>(nullptr), R);
  };
  if ((rc = for_candidates<LevenWindow>(ex, W, S, k, cand_capacity, 2 * k, "FEMTO_AMD_LEVEN_GRID", "FEMTO_AMD_LEVEN_CHUNK", st, on_text, on_samples))) return rc;
  if (capacity == 0) return launch(total_kernel, dim3(1), st, R, static_cast<const int64_t*>(nullptr), S.total, d_total);
  // by (offset, cost, length), then (stable) by pattern; total_length is no result's offset: the slots behind the live ones sort
  // behind every record.  keys and keys2 hold the heads' flags and their scan afterwards, and the scan writes capacity + 1 words:
  // keys2 is reserved for them here, larger than the sort asks for (and keys in front of it, which keeps the order of the allocations)
  if ((rc = W.keys.reserve(cap * 8)) || (rc = W.keys2.reserve(cap * 8 + 8))) return rc;
  Ordered o;
  if ((rc = order_records(W.order(), R.total, capacity, R.pat, npat, OffsetKey{R.off, R.meta}, unsigned(bits_of(S.N)) + 11u, uint64_t(S.N) << 11, st, &o)))
    return rc;
  int64_t *flags = W.keys.as<int64_t>(), *scan = W.keys2.as<int64_t>();
  if ((rc = launch(head_kernel, blocks_of(capacity), st, R, o.idx, flags)) || (rc = device_scan(W.scan, capacity, flags, scan, 0, st)) ||
      (rc = launch(gather_kernel, blocks_of(capacity), st, R, o.idx, scan, out)) ||
      (rc = launch(result_start_kernel, blocks_for(npat), st, R, o.pattern_keys, scan, d_result_start)))
    return rc;
  return launch(total_kernel, dim3(1), st, R, scan, S.total, d_total);
}

}  // namespace
}  // namespace femto_amd

int femto_amd_leven_device(femto_amd_extractor_t* ex, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                           int64_t cand_capacity, int64_t capacity, int64_t* d_result_start, int64_t* d_offset, int32_t* d_cost, int32_t* d_length,
                           int64_t* d_total, void* stream) {
  API_BEGIN
  int rc = check_device_call(ex, npat, nsyms, d_syms, d_starts, k, kMaxK, kBadK, cand_capacity, capacity, d_result_start, d_total,
                             d_offset && d_cost && d_length);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npat == 0) return empty_result_async(d_result_start, d_total, st, 5);
  Work* W;
  if ((rc = work_of(ex, ex->leven, &W))) return rc;
  return run_leven(ex, *W, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, Out{d_offset, d_cost, d_length}, d_total, st);
  API_END
}

void femto_amd_leven_free(femto_amd_leven_result_t* out) {
  if (!out) return;
  free(out->result_start);
  free(out->offset);
  free(out->cost);
  free(out->length);
  memset(out, 0, sizeof *out);
}

int femto_amd_leven(femto_amd_extractor_t* ex, int64_t npat, const int32_t* plen, const uint16_t* syms, int k, femto_amd_leven_result_t* out) {
  API_BEGIN
  if (!out) return set_err(FEMTO_AMD_ERR_PARAM, "null result");
  memset(out, 0, sizeof *out);
  std::vector<int64_t> starts;
  int64_t nsyms;
  int rc = check_host_batch(ex, npat, plen, syms, k, kMaxK, kBadK, &starts, &nsyms);
  if (rc) return rc;
  out->result_start = static_cast<int64_t*>(calloc(size_t(npat) + 1, 8));
  if (!out->result_start) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  out->npat = npat;
  if (npat == 0) return FEMTO_AMD_OK;
  auto fail = [&](int code) {
    femto_amd_leven_free(out);
    return code;
  };
  hipStream_t st = nullptr;
  Work* W;
  Temp T;
  HostBatch B;
  int64_t* d_off;
  int32_t *d_cost, *d_length;
  // the pieces' counts size the candidates, a counting pass sizes the raw records of the filling pass
  if ((rc = upload_host_batch(ex, ex->leven, T, starts, syms, k, false, 5, st, &W, &B))) return fail(rc);
  const Out none{nullptr, nullptr, nullptr};
  int64_t tot[5] = {0, 0, 0, 0, 0};
  if ((rc = run_leven(ex, *W, npat, nsyms, B.d_syms, B.d_starts, k, B.cands, 0, B.d_rs, none, B.d_tot, st))) return fail(rc);
  if ((rc = words_to_host(5, B.d_tot, st, "counting the records failed on the device", tot))) return fail(rc);
  if (tot[4] || tot[3] != B.cands) return fail(set_err(FEMTO_AMD_ERR_INVALID, "internal error: the seeds disagree with the pieces' counts"));
  const int64_t raw = tot[2];
  if (raw >= kMaxCall) return fail(set_err(FEMTO_AMD_ERR_FULL, "2^31 raw records or more: search the patterns in smaller batches"));
  out->candidates = B.cands;
  out->raw = raw;
  if (raw == 0) return FEMTO_AMD_OK;      // (result_start is zeros)
  const size_t ur = size_t(raw);
  if ((rc = T.get(&d_off, ur)) || (rc = T.get(&d_cost, ur)) || (rc = T.get(&d_length, ur)) ||
      (rc = run_leven(ex, *W, npat, nsyms, B.d_syms, B.d_starts, k, B.cands, raw, B.d_rs, Out{d_off, d_cost, d_length}, B.d_tot, st)))
    return fail(rc);
  if ((rc = words_to_host(5, B.d_tot, st, "de-duplicating the records failed on the device", tot))) return fail(rc);
  const int64_t total = tot[0];
  if (tot[1] || tot[2] != raw || total <= 0 || total > raw) return fail(set_err(FEMTO_AMD_ERR_INVALID, "the filling pass disagrees with the counting pass"));
  if ((rc = list_to_host(total, d_off, st, "copying the results back", &out->offset, false)) ||
      (rc = list_to_host(total, d_cost, st, "copying the results back", &out->cost, false)) ||
      (rc = list_to_host(total, d_length, st, "copying the results back", &out->length, false)))
    return fail(rc);
  if ((rc = result_start_to_host(npat, B.d_rs, st, out->result_start))) return fail(rc);
  out->total = total;
  return FEMTO_AMD_OK;
  API_END
}
