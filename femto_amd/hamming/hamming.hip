// hamming.hip -- occurrences within k substitutions by exact seeds: for every pattern of a batch, the text offsets where it occurs
// with at most k characters changed, each with its cost.  include/femto_amd.h "occurrences within k substitutions" states the
// contract; DESIGN.md "Occurrences within k substitutions" the kernels, their registers and the figures.
//
// THE ROUTE.  A pattern of m symbols is cut into k + 1 pieces, piece j = [j m / (k + 1), (j + 1) m / (k + 1)).  A window that
// differs from the pattern at no more than k positions holds one of them unchanged (pigeonhole), so the windows worth a look are
// those the pieces point at: the pieces are LOCATED exactly (the locate chain, row-free form) and each located offset, moved back
// by its piece's start, is compared against the text.  Nothing is enumerated: the cost follows the candidates, not k or the
// alphabet.  ../mismatch/mismatch.hip answers the question for k <= 2 as strings with row ranges; this answers it as offsets.
//
// What stands in front of the verify and around it is ../common/seeds.hpp's, shared with ../leven/leven.hip: the piece table, the
// work area, the locate call, the lookup of a candidate, the driver of the check over both paths (for_candidates) and the checks
// and the prologue of the two forms.  This file keeps the verify, the records, the order tail and the two passes of the host form;
// the PIECE TABLE, the SEEDS (one row-free femto_amd_locate_device_v2 call, no lease held) and the WORK AREA are described there.
// VERIFY.  One lane per candidate (piece, offset): the window p = offset - piece start is dropped outside [0, total_length - m];
// it is compared with the pattern in 8-byte words (two aligned loads and a funnel shift on either side) and left as soon as the
// differing bytes pass k, a differing text byte is no byte character (SEOF: the window runs over a document's end), or an EARLIER
// piece has no difference -- that piece's own candidate is the occurrence's owner, so every occurrence is emitted once.
// EMIT is mismatch.hip's: atomicAdd on the pattern's counter and the total, the record written below the capacity.  ORDER is the
// stage of ../common/result_order.hpp (two stable radix sorts of the records' indexes, by offset, then by pattern) and a gather;
// result_start from the counters.
// SAMPLE PATH.  No text in HBM: the windows of a chunk of candidates are extracted (femto_amd_extract_device) into a buffer of
// fixed stride and the same rules run over alpha codes.  This path reads the candidate total back and allocates.
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

using namespace seeds;      // the work area and a call's turn on it, the piece table, the candidates: ../common/seeds.hpp

constexpr int kMaxK = 255;
const char* const kBadK = "k must be 0 .. 255 substitutions";

// the shared area with the order stage's buffers and, on top of it, the records
struct Work : OrderArea {
  DeviceBuffer counts, r_off, r_pat, r_cost;
  ~Work() override { for (DeviceBuffer* b : {&counts, &r_off, &r_pat, &r_cost}) b->release(); }
};

// ---- verify ---------------------------------------------------------------------------------------------------------------------

// the records as the lanes emit them (any order), and the counters: counts[q] = results of pattern q, counts[npat] = all
struct Records {
  int64_t* off;
  uint32_t* pat;
  int32_t* cost;
  unsigned long long* counts;
  int64_t npat, capacity;
};

__device__ __forceinline__ void emit(const Records& R, int64_t q, int64_t p, int cost) {
  atomicAdd(R.counts + q, 1ull);
  const int64_t slot = int64_t(atomicAdd(R.counts + R.npat, 1ull));
  if (slot >= R.capacity) return;
  R.off[slot] = p;
  R.pat[slot] = uint32_t(q);
  R.cost[slot] = cost;
}

// the compare symbol by symbol: text(i) = the alpha code of T[p + i].  Returns the cost, -1 for a window that is dropped
template <class TextAt>
__device__ __forceinline__ int compare_syms(const Seeds& S, const Cand& C, const int k, TextAt text) {
  int cost = 0, pi = 0, nb = C.m / S.kp1;
  bool acc = false;
  for (int i = 0; i < C.m; i++) {
    if (pi < C.j && i == nb) {
      if (!acc) return -1;      // an earlier piece stands unchanged: its candidate owns this window
      pi++;
      nb = (pi + 1) * C.m / S.kp1;
      acc = false;
    }
    const uint32_t t = text(i);
    if (t != S.syms[C.s + i]) {
      if (t < kByte0 || ++cost > k) return -1;
      acc = true;
    }
  }
  return cost;
}

struct TextSrc {
  const uint8_t* txt;        // one dense code per position, 64 bytes of slack behind the last
  const uint8_t* dense;      // the patterns' dense codes, symbol g of the batch at dense[g]
  const uint16_t* alpha;     // dense code -> alpha code
  __device__ __forceinline__ int compare(const Seeds& S, const Cand& C, const int k, int64_t, const uint8_t* s_isbyte) const {
    if (C.fl & kSlow) {
      const uint8_t* t = txt + C.p;
      const uint16_t* a = alpha;
      return compare_syms(S, C, k, [=](int i) -> uint32_t { return a[t[i]]; });
    }
    const uint64_t* tw = reinterpret_cast<const uint64_t*>(txt + (C.p & ~int64_t(7)));
    const uint64_t* pw = reinterpret_cast<const uint64_t*>(dense + (C.s & ~int64_t(7)));
    const uint32_t tsh = uint32_t(C.p & 7) * 8u, psh = uint32_t(C.s & 7) * 8u;
    uint64_t t0 = tw[0], p0 = pw[0];
    int cost = 0, pi = 0, nb = C.m / S.kp1;
    bool acc = false;
    for (int w = 0; w < C.m; w += 8) {
      const uint64_t t1 = tw[(w >> 3) + 1], p1 = pw[(w >> 3) + 1];      // (slack behind the text and behind the dense codes)
      const uint64_t tx = tsh ? (t0 >> tsh) | (t1 << (64u - tsh)) : t0;
      const uint64_t px = psh ? (p0 >> psh) | (p1 << (64u - psh)) : p0;
      t0 = t1;
      p0 = p1;
      uint64_t x = tx ^ px;
      if (C.m - w < 8) x &= (uint64_t(1) << (8 * (C.m - w))) - 1;
      uint32_t mask = 0;      // bit b: byte b differs
      if (x) {
        uint64_t y = x | (x >> 4);
        y |= y >> 2;
        y |= y >> 1;
        mask = uint32_t(((y & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
        cost += __popc(mask);
        if (cost > k) return -1;
        for (uint32_t mm = mask; mm; mm &= mm - 1)
          if (!s_isbyte[uint32_t(tx >> (8 * (__ffs(int(mm)) - 1))) & 0xffu]) return -1;      // SEOF under a differing position
      }
      uint32_t donemask = 0;      // the bits of this word that belong to pieces already closed
      while (pi < C.j && nb <= w + 8) {
        const uint32_t low = (1u << (nb - w)) - 1u;      // (nb > w: every end <= w was closed a word ago)
        if (!acc && !(mask & low & ~donemask)) return -1;      // an earlier piece stands unchanged
        donemask = low;
        acc = false;
        pi++;
        nb = (pi + 1) * C.m / S.kp1;
      }
      if (pi < C.j && (mask & ~donemask)) acc = true;
    }
    return cost;
  }
};

struct CtxSrc {
  const uint16_t* ctx;       // the window of candidate c0 + i at ctx[i * stride]
  int64_t stride;
  __device__ __forceinline__ int compare(const Seeds& S, const Cand& C, const int k, int64_t local, const uint8_t*) const {
    const uint16_t* t = ctx + local * stride;
    return compare_syms(S, C, k, [=](int i) -> uint32_t { return t[i]; });
  }
};

// candidates [c0, c0 + n) of the chain's output, a grid that strides over them
template <class Src>
__global__ __launch_bounds__(256) void verify_kernel(const Src src, const Seeds S, const int64_t c0, const int64_t n, const int k,
                                                     const uint16_t* __restrict__ alpha, const Records R) {
  __shared__ uint8_t s_isbyte[256];
  {
    const uint32_t a = alpha ? alpha[threadIdx.x] : 0u;
    s_isbyte[threadIdx.x] = uint8_t(a >= kByte0 && a < kAlpha);
  }
  __syncthreads();
  if (S.total[1]) return;
  const int64_t live = S.total[0] - c0 < n ? S.total[0] - c0 : n;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < live; i += int64_t(gridDim.x) * 256) {
    Cand C;
    if (!candidate(S, c0 + i, &C)) continue;
    const int cost = src.compare(S, C, k, i, s_isbyte);
    if (cost >= 0) emit(R, C.q, C.p, cost);
  }
}

// sample path: the window of a candidate is the one the compare reads, [p, p + m) inside the text
struct HammingWindow {
  __device__ __forceinline__ static bool of(const Seeds& S, int64_t c, int, int64_t* w0, int64_t* w1) {
    Cand C;
    if (!candidate(S, c, &C)) return false;
    *w0 = C.p;
    *w1 = C.p + C.m;
    return true;
  }
};

// ---- order ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void total_kernel(const Records R, const int64_t* __restrict__ seeds_total, int64_t* __restrict__ d_total) {
  if (blockIdx.x || threadIdx.x) return;
  write_total(d_total, int64_t(R.counts[R.npat]), R.capacity);
  d_total[2] = seeds_total[0];
  d_total[3] = seeds_total[1];
}

__global__ __launch_bounds__(256) void gather_kernel(const Records R, const uint32_t* __restrict__ idx, int64_t* __restrict__ out_off,
                                                     int32_t* __restrict__ out_cost) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= live_records(R.counts + R.npat, R.capacity)) return;
  const uint32_t r = idx[s];
  out_off[s] = R.off[r];
  out_cost[s] = R.cost[r];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

int run_hamming(femto_amd_extractor* ex, Work& W, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                int64_t cand_capacity, int64_t capacity, int64_t* d_result_start, int64_t* d_offset, int32_t* d_cost, int64_t* d_total,
                hipStream_t st) {
  const size_t cap = size_t(capacity), un = size_t(npat);
  Turn turn(W, st);
  int rc = turn.rc;
  if (rc) return rc;
  if ((rc = W.counts.reserve((un + 1) * 8)) || (rc = W.r_off.reserve(cap * 8 + 8)) || (rc = W.r_pat.reserve(cap * 4 + 8)) ||
      (rc = W.r_cost.reserve(cap * 4 + 8)))
    return rc;
  const Records R{W.r_off.as<int64_t>(), W.r_pat.as<uint32_t>(), W.r_cost.as<int32_t>(), W.counts.as<unsigned long long>(), npat, capacity};
  // the patterns' dense codes are what the text path compares
  Seeds S;
  if ((rc = locate_seeds(ex, W, npat, nsyms, d_syms, d_starts, k, ex->path == FEMTO_AMD_EXTRACT_PATH_TEXT, cand_capacity, R.counts, (un + 1) * 8, st, &S)))
    return rc;
  const auto on_text = [&](dim3 grid) {
    return launch(verify_kernel<TextSrc>, grid, st, TextSrc{ex->ix->d_txt, W.dense.as<uint8_t>(), ex->d_alpha}, S, int64_t(0), cand_capacity, k, ex->d_alpha, R);
  };
  const auto on_samples = [&](const uint16_t* w_syms, int64_t stride, int64_t c0, int64_t cn) {
    return launch(verify_kernel<CtxSrc>, blocks_of(cn), st, CtxSrc{w_syms, stride}, S, c0, cn, k, static_cast<const uint16_t*>(nullptr), R);
  };
  if ((rc = for_candidates<HammingWindow>(ex, W, S, k, cand_capacity, 0, "FEMTO_AMD_HAMMING_GRID", "FEMTO_AMD_HAMMING_CHUNK", st, on_text, on_samples))) return rc;
  if ((rc = device_scan(W.scan, npat, reinterpret_cast<const int64_t*>(R.counts), d_result_start, 0, st)) ||
      (rc = launch(total_kernel, dim3(1), st, R, S.total, d_total)))
    return rc;
  if (capacity == 0) return 0;
  // by offset, then (stable) by pattern; total_length is no window's start: the slots behind the live ones sort behind every offset
  Ordered o;
  if ((rc = order_records(W.order(), R.counts + npat, capacity, R.pat, npat, ColumnKey{R.off}, unsigned(bits_of(S.N)), uint64_t(S.N), st, &o))) return rc;
  return launch(gather_kernel, blocks_of(capacity), st, R, o.idx, d_offset, d_cost);
}

}  // namespace
}  // namespace femto_amd

int femto_amd_hamming_device(femto_amd_extractor_t* ex, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                             int64_t cand_capacity, int64_t capacity, int64_t* d_result_start, int64_t* d_offset, int32_t* d_cost,
                             int64_t* d_total, void* stream) {
  API_BEGIN
  int rc = check_device_call(ex, npat, nsyms, d_syms, d_starts, k, kMaxK, kBadK, cand_capacity, capacity, d_result_start, d_total,
                             d_offset && d_cost);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npat == 0) return empty_result_async(d_result_start, d_total, st, 4);
  Work* W;
  if ((rc = work_of(ex, ex->hamming, &W))) return rc;
  return run_hamming(ex, *W, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, d_offset, d_cost, d_total, st);
  API_END
}

void femto_amd_hamming_free(femto_amd_hamming_result_t* out) {
  if (!out) return;
  free(out->result_start);
  free(out->offset);
  free(out->cost);
  memset(out, 0, sizeof *out);
}

int femto_amd_hamming(femto_amd_extractor_t* ex, int64_t npat, const int32_t* plen, const uint16_t* syms, int k, femto_amd_hamming_result_t* out) {
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
    femto_amd_hamming_free(out);
    return code;
  };
  hipStream_t st = nullptr;
  Work* W;
  Temp T;
  HostBatch B;
  int64_t* d_off;
  int32_t* d_cost;
  // the pieces' counts size the candidates, a counting pass sizes the filling pass
  if ((rc = upload_host_batch(ex, ex->hamming, T, starts, syms, k, ex->path == FEMTO_AMD_EXTRACT_PATH_TEXT, 4, st, &W, &B))) return fail(rc);
  int64_t tot[4] = {0, 0, 0, 0};
  if ((rc = run_hamming(ex, *W, npat, nsyms, B.d_syms, B.d_starts, k, B.cands, 0, B.d_rs, nullptr, nullptr, B.d_tot, st))) return fail(rc);
  if ((rc = words_to_host(4, B.d_tot, st, "counting the results failed on the device", tot))) return fail(rc);
  if (tot[3] || tot[2] != B.cands) return fail(set_err(FEMTO_AMD_ERR_INVALID, "internal error: the seeds disagree with the pieces' counts"));
  const int64_t total = tot[0];
  if (total) {
    const size_t ut = size_t(total);
    if ((rc = T.get(&d_off, ut)) || (rc = T.get(&d_cost, ut)) ||
        (rc = run_hamming(ex, *W, npat, nsyms, B.d_syms, B.d_starts, k, B.cands, total, B.d_rs, d_off, d_cost, B.d_tot, st)) ||
        (rc = list_to_host(int64_t(ut), d_off, st, "copying the results back", &out->offset, false)) ||
        (rc = list_to_host(int64_t(ut), d_cost, st, "copying the results back", &out->cost, false)))
      return fail(rc);
  }
  if ((rc = result_start_to_host(npat, B.d_rs, st, out->result_start))) return fail(rc);
  out->total = total;
  out->candidates = B.cands;
  return FEMTO_AMD_OK;
  API_END
}
