// extract.hip -- the text of the index on the GPU: extract by position, whole documents, and the context of a row or text
// offset (do_context_query, src/main/server.c:2567-2795; do_extract_document_query, :6337-6440).  include/femto_amd.h states
// the semantics; DESIGN.md "Extraction" the two paths.
//
// Every request is first turned into (pos, len, output slot, valid window [vlo, vhi)): a symbol at text position q is
// written when vlo <= q < vhi (q = -1, allowed only as a context's wrap, is T[N - 1] = SEOF), and 0 otherwise.  Plain
// extraction has the window [0, N); a context has the anchor's document plus the SEOF in front of it -- exactly the
// symbols do_back_query / do_forward_query's stop rule lets through.
//
// TEXT PATH (the handle holds d_txt, one dense code per position): a copy.  The output is laid out as one virtual array
// (exclusive prefix sum of the lengths); every thread owns 8 consecutive output symbols, finds its request by binary search
// within the few requests its workgroup covers, and moves the 8 symbols with two aligned 8-byte text loads and one 16-byte
// store when the request and the alignment allow.
//
// SAMPLE PATH (any other handle): a table samp[p >> s] = SA^-1[p] of the sampled positions and the row of every document's
// SEOF, built once when the extractor opens.  A request is split at every multiple of 2^s; one lane per piece walks LF
// back from the sample row at the piece's end (or from the SEOF row of a document that ends inside it) and writes L[row].
// A walk never steps from a row whose L is <= SEOF: inside a document every symbol is a byte + 5.
//
// The request of an output slot or a piece (first_gt), an anchor's document (doc_of) and the live count (live_of) are
// ../common/ragged.hpp; every launch is ../common/host_common.hpp's checked launch().
#include <algorithm>
#include <chrono>
#include <cstring>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../csrc/kernels.hip.hpp"
#include "../csrc/pack_kernels.hip.hpp"
#include "../csrc/ru_kernels.hip.hpp"
#include "../csrc/pack2_kernels.hip.hpp"
#include "../csrc/ind_kernels.hip.hpp"
#include "../csrc/text_kernels.hip.hpp"

#include "extractor.hpp"

namespace femto_amd {
namespace {

constexpr int kSymsPerThread = 8;
constexpr int kTileSyms = 256 * kSymsPerThread;

struct XReqs {
  const int64_t* pos;
  const int32_t* len;
  const int64_t* out_start;    // NULL: packed, request r at cum[r]
  const int64_t* vlo;          // NULL: 0
  const int64_t* vhi;          // NULL: N
  int64_t n;
  const int64_t* d_n;          // NULL or: only min(n, *d_n) requests are live
  const int64_t* cum;          // n + 1 entries: exclusive prefix sum of the live lengths
  const int64_t* pcum;         // sample path: ... of the pieces
};

// [jlo, jhi): the slots of request r whose position lies in [lo, hi) -- without overflow for any pos
__device__ __forceinline__ void slots_in(int64_t pos, int64_t len, int64_t lo, int64_t hi, int64_t* jlo, int64_t* jhi) {
  int64_t a = pos >= lo ? 0 : (pos < lo - len ? len : lo - pos);
  int64_t b = pos >= hi ? 0 : (pos < hi - len ? len : hi - pos);
  *jlo = a;
  *jhi = b > a ? b : a;
}

// lengths of the live requests (negative: 0) and, sample path, their piece counts
__global__ __launch_bounds__(256) void xprep_kernel(const XReqs R, const int64_t N, const int shift, int64_t* __restrict__ lens64,
                                                    int64_t* __restrict__ pieces) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= R.n) return;
  const int64_t live = live_of(R.d_n, R.n);
  int64_t len = i < live ? int64_t(R.len[i]) : 0;
  if (len < 0) len = 0;
  lens64[i] = len;
  if (pieces) {
    const int64_t pos = R.pos[i];
    const int64_t vlo = R.vlo ? R.vlo[i] : 0, vhi = R.vhi ? R.vhi[i] : N;
    int64_t jlo, jhi;
    slots_in(pos, len, vlo > 0 ? vlo : 0, vhi < N ? vhi : N, &jlo, &jhi);
    pieces[i] = jhi > jlo ? (((pos + jhi - 1) >> shift) - ((pos + jlo) >> shift) + 1) : 0;
  }
}

// kText: every slot of the virtual output (the text path); otherwise only the slots the sample walk does not write
// (outside [max(vlo, 0), vhi): 0, or SEOF for a context's wrap to position -1)
template <bool kText>
__global__ __launch_bounds__(256) void xcopy_kernel(const XReqs R, const int64_t N, const uint8_t* __restrict__ txt,
                                                    const uint16_t* __restrict__ alpha, uint16_t* __restrict__ out) {
  __shared__ uint16_t s_alpha[256];
  __shared__ int64_t s_r[2];
  if (kText) s_alpha[threadIdx.x] = alpha[threadIdx.x];
  const int64_t total = R.cum[R.n];
  for (int64_t base = int64_t(blockIdx.x) * kTileSyms; base < total; base += int64_t(gridDim.x) * kTileSyms) {
    __syncthreads();
    if (threadIdx.x < 2) {
      const int64_t v = threadIdx.x == 0 ? base : (base + kTileSyms - 1 < total ? base + kTileSyms - 1 : total - 1);
      s_r[threadIdx.x] = first_gt(R.cum, 0, R.n + 1, v) - 1;
    }
    __syncthreads();
    const int64_t v0 = base + int64_t(threadIdx.x) * kSymsPerThread;
    if (v0 >= total) continue;
    int64_t r = first_gt(R.cum, s_r[0], s_r[1] + 1, v0) - 1;
    int64_t c0 = R.cum[r], c1 = R.cum[r + 1];
    const int64_t vend = v0 + kSymsPerThread < total ? v0 + kSymsPerThread : total;
    // fast path: 8 symbols of one request, all inside its window
    if (vend - v0 == kSymsPerThread && v0 + kSymsPerThread <= c1) {
      const int64_t pos = R.pos[r], len = c1 - c0, j0 = v0 - c0;
      const int64_t vlo = R.vlo ? R.vlo[r] : 0, vhi = R.vhi ? R.vhi[r] : N;
      int64_t jlo, jhi;
      slots_in(pos, len, vlo > 0 ? vlo : 0, vhi < N ? vhi : N, &jlo, &jhi);
      if (j0 >= jlo && j0 + kSymsPerThread <= jhi) {
        if (!kText) continue;      // the walk writes all eight
        const int64_t q0 = pos + j0;
        const uint64_t* w = reinterpret_cast<const uint64_t*>(txt + (q0 & ~int64_t(7)));
        const uint32_t sh = uint32_t(q0 & 7) * 8u;
        const uint64_t lo = w[0];
        const uint64_t bytes = sh ? ((lo >> sh) | (w[1] << (64u - sh))) : lo;   // (d_txt has 64 bytes of slack)
        uint16_t sym[8];
#pragma unroll
        for (int k = 0; k < 8; k++) sym[k] = s_alpha[(bytes >> (8 * k)) & 0xffu];
        uint16_t* dst = out + (R.out_start ? R.out_start[r] : c0) + j0;
        if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
          uint4 pk;
          pk.x = uint32_t(sym[0]) | (uint32_t(sym[1]) << 16);
          pk.y = uint32_t(sym[2]) | (uint32_t(sym[3]) << 16);
          pk.z = uint32_t(sym[4]) | (uint32_t(sym[5]) << 16);
          pk.w = uint32_t(sym[6]) | (uint32_t(sym[7]) << 16);
          *reinterpret_cast<uint4*>(dst) = pk;
        } else {
#pragma unroll
          for (int k = 0; k < 8; k++) dst[k] = sym[k];
        }
        continue;
      }
    }
    for (int64_t v = v0; v < vend; v++) {
      while (v >= c1) {
        r++;
        c0 = c1;
        c1 = R.cum[r + 1];
      }
      const int64_t j = v - c0, q = R.pos[r] + j;     // (q only compared once it is known to be in the window)
      const int64_t vlo = R.vlo ? R.vlo[r] : 0, vhi = R.vhi ? R.vhi[r] : N;
      int64_t jlo, jhi;
      slots_in(R.pos[r], c1 - c0, vlo, vhi, &jlo, &jhi);
      uint16_t sym = 0;
      if (j >= jlo && j < jhi) {
        if (q < 0) sym = uint16_t(kSEOF);
        else if (!kText) continue;
        else sym = s_alpha[txt[q]];
      }
      out[(R.out_start ? R.out_start[r] : c0) + j] = sym;
    }
  }
}

// ---- sample path --------------------------------------------------------------------------------------------------------

struct SampTables {
  const int64_t* doc_ends;
  int64_t ndocs;
  const int64_t* eof;
  const void* samp;
  int samp32;
  int shift;
};

__device__ __forceinline__ int64_t samp_at(const SampTables& T, int64_t k) {
  if (T.samp32) return int64_t(reinterpret_cast<const uint32_t*>(T.samp)[k]);
  return reinterpret_cast<const int64_t*>(T.samp)[k];
}

// One piece: positions [lo, hi) inside sample block [blk_end - 2^s, blk_end) of request r.  The walk writes positions
// q, q - 1, ..., seg_lo from `row` (L[row] = T[q]); the segments are the documents the piece touches, from the top.
struct Walk {
  int64_t row, q, seg_lo, ds, lo, hi, blk_end, dst;   // dst: output slot of position 0 (slot of q = dst + q)
  int32_t live;
};

// the next segment at or below w.hi - 1; false when the piece is done
__device__ __forceinline__ bool walk_begin(Walk& w, const SampTables& T, uint16_t* __restrict__ out) {
  while (w.hi > w.lo) {
    // the document holding position hi - 1 < N.  Not doc_of: its test for a position behind the last document costs the walk
    // kernels two registers each
    const int64_t d = first_gt(T.doc_ends, 0, T.ndocs, w.hi - 1);
    const int64_t ds = d ? T.doc_ends[d - 1] : 0, de1 = T.doc_ends[d];
    w.ds = ds;
    w.seg_lo = w.lo > ds ? w.lo : ds;
    int64_t e;
    if (de1 <= w.blk_end) {          // the document's SEOF (position de1 - 1) lies in this block: the walk starts at its row
      if (de1 - 1 < w.hi) out[w.dst + de1 - 1] = uint16_t(kSEOF);
      e = de1 - 1;
      w.row = T.eof[d];
    } else {
      e = w.blk_end;
      w.row = samp_at(T, w.blk_end >> T.shift);
    }
    w.q = e - 1;
    if (w.q >= w.seg_lo) return true;
    w.hi = ds;
  }
  return false;
}

// one walk step with L[row] = sym and LF(row) = next; false when the piece is done
__device__ __forceinline__ bool walk_step(Walk& w, const SampTables& T, uint16_t sym, int64_t next, uint16_t* __restrict__ out) {
  if (w.q < w.hi) out[w.dst + w.q] = sym;
  if (w.q > w.seg_lo) {
    w.row = next;
    w.q--;
    return true;
  }
  w.hi = w.ds;
  return walk_begin(w, T, out);
}

__device__ __forceinline__ bool walk_init(Walk& w, const XReqs& R, const int64_t N, const SampTables& T, int64_t g, uint16_t* __restrict__ out) {
  const int64_t r = first_gt(R.pcum, 0, R.n + 1, g) - 1;
  const int64_t pos = R.pos[r], len = R.cum[r + 1] - R.cum[r];
  const int64_t vlo = R.vlo ? R.vlo[r] : 0, vhi = R.vhi ? R.vhi[r] : N;
  int64_t jlo, jhi;
  slots_in(pos, len, vlo > 0 ? vlo : 0, vhi < N ? vhi : N, &jlo, &jhi);
  const int64_t a = pos + jlo, b = pos + jhi;
  const int64_t blk = (a >> T.shift) + (g - R.pcum[r]);
  const int64_t b0 = blk << T.shift;
  w.blk_end = b0 + (int64_t(1) << T.shift);
  w.lo = a > b0 ? a : b0;
  w.hi = b < w.blk_end ? b : w.blk_end;
  w.dst = (R.out_start ? R.out_start[r] : R.cum[r]) - pos;
  return walk_begin(w, T, out);
}

template <class P> struct AlphaOf;
template <> struct AlphaOf<PackPolicy> {
  static __device__ __forceinline__ uint16_t get(const DevIndex& ix, uint32_t code) { return code < 8u ? ix.pack_alpha[code] : uint16_t(0); }
};
template <> struct AlphaOf<Pack2Policy> {
  static __device__ __forceinline__ uint16_t get(const DevIndex& ix, uint32_t code) { return code < 256u ? ix.p2_alpha[code] : uint16_t(0); }
};

// packed handles (modes 3 / 4): one lane walks its whole piece, one line per step
template <class P>
__global__ __launch_bounds__(256) void xwalk_kernel(const DevIndex ix, const XReqs R, const SampTables T, uint16_t* __restrict__ out) {
  const int64_t total = R.pcum[R.n];
  for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < total; g += int64_t(gridDim.x) * blockDim.x) {
    Walk w;
    bool more = walk_init(w, R, ix.total_length, T, g, out);
    while (more) {
      uint32_t code;
      bool marked;
      int64_t sa_index, nx;
      P::lf(ix, w.row, code, marked, sa_index, nx);
      more = walk_step(w, T, AlphaOf<P>::get(ix, code), nx, out);
    }
  }
}

// femto's own tables (modes 0 / 1): the walk as a state machine, one step per launch of the leaf kernel
__global__ __launch_bounds__(256) void xwalk_init_kernel(const XReqs R, const int64_t N, const SampTables T, const int64_t npieces,
                                                         Walk* __restrict__ st, int64_t* __restrict__ rows, uint16_t* __restrict__ out) {
  const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= npieces) return;
  Walk w;
  w.live = walk_init(w, R, N, T, g, out) ? 1 : 0;
  st[g] = w;
  rows[g] = w.live ? w.row : 0;      // (a finished lane asks the leaf kernel about row 0 and ignores the answer)
}
__global__ __launch_bounds__(256) void xwalk_leaf_step_kernel(const SampTables T, const int64_t npieces, Walk* __restrict__ st,
                                                              int64_t* __restrict__ rows, const uint16_t* __restrict__ ch,
                                                              const int64_t* __restrict__ occ, uint16_t* __restrict__ out) {
  const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= npieces) return;
  Walk w = st[g];
  if (!w.live) return;
  w.live = walk_step(w, T, ch[g], occ[g] - 1, out) ? 1 : 0;     // LF = C[ch] + Occ(ch, row) - 1 (server.c:2279-2282)
  st[g] = w;
  rows[g] = w.live ? w.row : 0;
}

// build: rows [r0, r0 + n) located to off[]; samp[p >> s] = row for the sampled positions, eof[d] = row for each SEOF
__global__ __launch_bounds__(256) void xsample_scatter_kernel(const int64_t r0, const int64_t n, const int64_t* __restrict__ off, const int64_t N,
                                                              const SampTables T, void* __restrict__ samp, int64_t* __restrict__ eof,
                                                              int* __restrict__ bad) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t row = r0 + i, p = off[i];
  if (p < 0 || p >= N) {
    atomicOr(bad, 1);
    return;
  }
  if ((p & ((int64_t(1) << T.shift) - 1)) == 0) {
    if (T.samp32) reinterpret_cast<uint32_t*>(samp)[p >> T.shift] = uint32_t(row);
    else reinterpret_cast<int64_t*>(samp)[p >> T.shift] = row;
  }
  const Doc D = doc_of(T.doc_ends, T.ndocs, p);
  if (D.end == p + 1) eof[D.doc] = row;
}

// ---- context: anchors -> requests -------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void xrows_sanitize_kernel(const int64_t n, const int64_t* __restrict__ rows, const int64_t N,
                                                             int64_t* __restrict__ safe, int64_t* __restrict__ iota) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i > n) return;
  iota[i] = i;
  if (i == n) return;
  const int64_t r = rows[i];
  safe[i] = (r >= 0 && r < N) ? r : 0;      // (the locate walk never sees a row outside the index)
}

__global__ __launch_bounds__(256) void xcontext_plan_kernel(const int64_t n, const int64_t* __restrict__ d_n, const int64_t* __restrict__ rows,
                                                            const int64_t* __restrict__ anchors, const int64_t N, const int64_t* __restrict__ doc_ends,
                                                            const int64_t ndocs, const int before, const int after, int64_t* __restrict__ pos,
                                                            int32_t* __restrict__ len, int64_t* __restrict__ out_start, int64_t* __restrict__ vlo,
                                                            int64_t* __restrict__ vhi, int64_t* __restrict__ pos_out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t live = live_of(d_n, n);
  const int64_t W = int64_t(before) + int64_t(after);
  out_start[i] = i * W;
  if (i >= live) {
    pos[i] = 0;
    len[i] = 0;
    vlo[i] = vhi[i] = 0;
    return;
  }
  bool ok = true;
  if (rows) {
    const int64_t r = rows[i];
    ok = r >= 0 && r < N;
  }
  const int64_t p = anchors[i];
  ok = ok && p >= 0 && p < N;
  len[i] = int32_t(W);
  if (!ok) {
    pos[i] = 0;
    vlo[i] = vhi[i] = 0;
    if (pos_out) pos_out[i] = -1;
    return;
  }
  const Doc D = doc_of(doc_ends, ndocs, p);
  pos[i] = p - before;
  vlo[i] = D.start - 1;                   // the SEOF in front of the document (position -1: T[N - 1]) ends the backward walk
  vhi[i] = D.doc < ndocs ? D.end : N;     // ... the document's own SEOF the forward walk
  if (pos_out) pos_out[i] = p;
}

SampTables tables_of(const femto_amd_extractor* ex) {
  SampTables T{};
  T.doc_ends = ex->d_doc_ends;
  T.ndocs = int64_t(ex->ix->host.doc_ends.size());
  T.eof = ex->d_eof;
  T.samp = ex->d_samp;
  T.samp32 = ex->samp32;
  T.shift = ex->shift;
  return T;
}

// the requests R (device arrays, R.cum / R.pcum filled here) into `out`; enqueue-only except on the sample path of modes 0 / 1,
// which reads the piece count back (it sizes the leaf kernel's launches)
int run_extract(femto_amd_extractor* ex, Scratch& S, XReqs R, uint16_t* out, hipStream_t st) {
  femto_amd_index* ix = ex->ix;
  const int64_t N = ix->host.total_length, n = R.n;
  int rc;
  if (n == 0) return 0;
  const bool samples = ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES;
  if ((rc = S.noccs64.reserve(size_t(n) * 8)) || (rc = S.out_starts.reserve(size_t(n + 1) * 8))) return rc;
  if (samples && ((rc = S.keys.reserve(size_t(n) * 8)) || (rc = S.keys2.reserve(size_t(n + 1) * 8)))) return rc;
  if ((rc = launch(xprep_kernel, blocks_of(n), st, R, N, ex->shift, S.noccs64.as<int64_t>(), samples ? S.keys.as<int64_t>() : nullptr)) ||
      (rc = device_scan(S.scan, n, S.noccs64.as<int64_t>(), S.out_starts.as<int64_t>(), 0, st)))
    return rc;
  R.cum = S.out_starts.as<int64_t>();
  const dim3 cgrid = persistent_grid(ix, (int64_t(1) << 40) / kTileSyms);   // persistent: the total is read on the device
  if (!samples) return launch(xcopy_kernel<true>, cgrid, st, R, N, ix->d_txt, ex->d_alpha, out);
  if ((rc = device_scan(S.scan, n, S.keys.as<int64_t>(), S.keys2.as<int64_t>(), 0, st))) return rc;
  R.pcum = S.keys2.as<int64_t>();
  if ((rc = launch(xcopy_kernel<false>, cgrid, st, R, N, nullptr, nullptr, out))) return rc;
  const SampTables T = tables_of(ex);
  if (with_policy<PackPolicy, Pack2Policy>(walk_kind(rank_kind(ix->mode, ix->dev)), [&](auto tag) {
        rc = launch(xwalk_kernel<typename decltype(tag)::type>, persistent_grid(ix, (int64_t(1) << 40) / 256), st, ix->dev, R, T, out);
      }))
    return rc;
  // femto's own tables: one leaf request per live piece and step
  if (!ix->host.dir_regular) return set_err(FEMTO_AMD_ERR_INVALID, "extraction on this handle needs the derived segment lines");
  int64_t npieces = 0;
  HIP_TRY(hipMemcpyAsync(&npieces, R.pcum + n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (npieces == 0) return 0;
  if (npieces >= (int64_t(1) << 31)) return set_err(FEMTO_AMD_ERR_PARAM, "too many pieces in one call on this handle: split the batch");
  if ((rc = S.sorttmp.reserve(size_t(npieces) * sizeof(Walk))) || (rc = S.rows.reserve(size_t(npieces) * 8)) ||
      (rc = S.ch.reserve(size_t(npieces) * 2)) || (rc = S.occ.reserve(size_t(npieces) * 8)))
    return rc;
  WaveletLinesUse use(ix);
  if ((rc = use.acquire())) return rc;
  const dim3 pgrid = blocks_of(npieces);
  Walk* stt = S.sorttmp.as<Walk>();
  int64_t* rows = S.rows.as<int64_t>();
  if ((rc = launch(xwalk_init_kernel, pgrid, st, R, N, T, npieces, stt, rows, out))) return rc;
  // every step consumes one position of the piece's sample block: 2^s steps end every walk
  for (int64_t k = 0; k < (int64_t(1) << ex->shift); k++)
    if ((rc = launch(block_request_kernel_lane, pgrid, st, ix->dev, npieces, rows, nullptr, S.ch.as<uint16_t>(), S.occ.as<int64_t>(), nullptr)) ||
        (rc = launch(xwalk_leaf_step_kernel, pgrid, st, T, npieces, stt, rows, S.ch.as<uint16_t>(), S.occ.as<int64_t>(), out)))
      return rc;
  HIP_TRY(hipStreamSynchronize(st));     // (the wavelet lines may leave with `use`)
  return 0;
}

// context: anchors -> the requests (in S.pairs / S.idx / S.idx2 / S.last / S.tail), then run_extract
int run_context(femto_amd_extractor* ex, Scratch& S, int64_t n, const int64_t* d_rows, const int64_t* d_offsets, const int64_t* d_n,
                int before, int after, uint16_t* d_ctx, int64_t* d_pos_out, hipStream_t st) {
  femto_amd_index* ix = ex->ix;
  const int64_t N = ix->host.total_length;
  int rc;
  if (n == 0) return 0;
  const int64_t* anchors = d_offsets;
  if (d_rows) {
    if ((rc = S.first.reserve(size_t(n) * 8)) || (rc = S.starts.reserve(size_t(n + 1) * 8)) || (rc = S.offsets.reserve(size_t(n) * 8))) return rc;
    if ((rc = launch(xrows_sanitize_kernel, blocks_for(n), st, n, d_rows, N, S.first.as<int64_t>(), S.starts.as<int64_t>()))) return rc;
    if ((rc = launch_locate(ix, S, n, S.first.as<int64_t>(), S.starts.as<int64_t>(), n, S.offsets.as<int64_t>(), st))) return rc;
    anchors = S.offsets.as<int64_t>();
  }
  if ((rc = S.pairs.reserve(size_t(n) * 8)) || (rc = S.idx.reserve(size_t(n) * 4)) || (rc = S.idx2.reserve(size_t(n) * 8)) ||
      (rc = S.last.reserve(size_t(n) * 8)) || (rc = S.tail.reserve(size_t(n) * 8)))
    return rc;
  if ((rc = launch(xcontext_plan_kernel, blocks_of(n), st, n, d_n, d_rows, anchors, N, ex->d_doc_ends, int64_t(ix->host.doc_ends.size()), before, after,
                   S.pairs.as<int64_t>(), S.idx.as<int32_t>(), S.idx2.as<int64_t>(), S.last.as<int64_t>(), S.tail.as<int64_t>(), d_pos_out)))
    return rc;
  XReqs R{};
  R.pos = S.pairs.as<int64_t>();
  R.len = S.idx.as<int32_t>();
  R.out_start = S.idx2.as<int64_t>();
  R.vlo = S.last.as<int64_t>();
  R.vhi = S.tail.as<int64_t>();
  R.n = n;
  return run_extract(ex, S, R, d_ctx, st);
}

int build_samples(femto_amd_extractor* ex) {
  femto_amd_index* ix = ex->ix;
  const int64_t N = ix->host.total_length, nd = int64_t(ix->host.doc_ends.size());
  Lease L(ix);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  hipStream_t st = S.stream;
  const int64_t chunk = int64_t(1) << 26;     // (mode 0 walks with 32 lanes per row: 2^31 work-items)
  int rc;
  if ((rc = S.offsets.reserve(size_t(std::min(chunk, N)) * 8)) || (rc = S.first.reserve(16)) || (rc = S.starts.reserve(16))) return rc;
  HIP_TRY(hipMemsetAsync(S.d_flags, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(ex->d_eof, 0xff, size_t(nd) * 8, st));
  const SampTables T = tables_of(ex);
  for (int64_t r0 = 0; r0 < N; r0 += chunk) {
    const int64_t cn = std::min(chunk, N - r0);
    const int64_t hf[2] = {r0, 0}, hs[2] = {0, cn};
    HIP_TRY(hipMemcpyAsync(S.first.p, hf, 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.starts.p, hs, 16, hipMemcpyHostToDevice, st));
    if ((rc = launch_locate(ix, S, 1, S.first.as<int64_t>(), S.starts.as<int64_t>(), cn, S.offsets.as<int64_t>(), st))) return rc;
    if ((rc = launch(xsample_scatter_kernel, blocks_of(cn), st, r0, cn, S.offsets.as<int64_t>(), N, T, ex->d_samp, ex->d_eof, S.d_flags))) return rc;
    HIP_TRY(hipStreamSynchronize(st));     // (the host copies of hf / hs are reused)
  }
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, S.d_flags, sizeof(int), hipMemcpyDeviceToHost, st));
  ex->h_eof.assign(size_t(nd), -1);
  if (nd) HIP_TRY(hipMemcpyAsync(ex->h_eof.data(), ex->d_eof, size_t(nd) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemsetAsync(S.d_flags, 0, sizeof(int), st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) return set_err(FEMTO_AMD_ERR_FORMAT, "a row of the index located outside the text: damaged index");
  for (int64_t v : ex->h_eof)
    if (v < 0) return set_err(FEMTO_AMD_ERR_FORMAT, "a document's SEOF was not found among the located rows: damaged index");
  return 0;
}

void free_extractor(femto_amd_extractor* ex) {
  if (ex->block) {
    (void)hipSetDevice(ex->ix->device);
    (void)hipDeviceSynchronize();      // (enqueue-only calls may still read the tables)
    std::lock_guard<std::mutex> lk(ex->ix->mu);
    big_free(ex->ix, ex->block);
  }
  delete ex;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_extractor_open(femto_amd_index_t* ix0, int sample_shift, int flags, femto_amd_extractor_t** out) {
  API_BEGIN
  if (!ix0 || !out || sample_shift < -1 || sample_shift > 16 || (flags & ~FEMTO_AMD_EXTRACT_FORCE_SAMPLES))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *out = nullptr;
  femto_amd_index* ix = replica0(ix0);
  int rc = check_plain_handle(ix, "extraction is");
  if (rc) return rc;
  const HostIndex& h = ix->host;
  const int64_t N = h.total_length, nd = int64_t(h.doc_ends.size());
  if (nd < 1 || h.doc_ends.back() != N) return set_err(FEMTO_AMD_ERR_FORMAT, "the documents do not end where the text does");
  std::unique_ptr<femto_amd_extractor> ex(new femto_amd_extractor());
  ex->ix = ix;
  ex->multi = ix != ix0;
  ex->path = (ix->d_txt && !(flags & FEMTO_AMD_EXTRACT_FORCE_SAMPLES)) ? FEMTO_AMD_EXTRACT_PATH_TEXT : FEMTO_AMD_EXTRACT_PATH_SAMPLES;
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES && !(ix->mode == 3 || ix->mode == 4) && !h.dir_regular)
    return set_err(FEMTO_AMD_ERR_INVALID, "extraction on this handle needs the derived segment lines");
  ex->shift = sample_shift < 0 ? 6 : sample_shift;
  ex->samp32 = N < int64_t(0xffffffffll) ? 1 : 0;
  const size_t nsamp = size_t((N + (int64_t(1) << ex->shift) - 1) >> ex->shift);
  size_t need = 512 + size_t(nd) * 8;
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES) need += size_t(nd) * 8 + nsamp * (ex->samp32 ? 4 : 8);
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    const size_t free_b = hbm_free(ix);
    if (need > free_b)
      return set_err(FEMTO_AMD_ERR_MEM, "the extractor needs " + std::to_string(need) + " bytes of HBM; the handle may take " +
                                            std::to_string(free_b) + " more (hbm_budget_bytes)");
    HIP_TRY(big_malloc(ix, &ex->block, need));
  }
  ex->bytes = int64_t(need);
  char* b = static_cast<char*>(ex->block);
  ex->d_alpha = reinterpret_cast<uint16_t*>(b);
  ex->d_doc_ends = reinterpret_cast<int64_t*>(b + 512);
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES) {
    ex->d_eof = ex->d_doc_ends + nd;
    ex->d_samp = static_cast<void*>(ex->d_eof + nd);
  }
  auto fail = [&](int code) {
    free_extractor(ex.release());
    return code;
  };
  // dense code of the text -> alpha code (build_text writes the codes of the 3-bit lines when they exist, else the two-level lines')
  std::vector<uint16_t> alpha(256, 0);
  if (ix->dev.pack) {
    for (int c = 0; c < 8; c++) alpha[size_t(c)] = ix->dev.pack_alpha[c] < kAlphaSize ? ix->dev.pack_alpha[c] : 0;
  } else if (ix->d_p2_alpha && ix->d_txt) {
    if (hipMemcpy(alpha.data(), ix->d_p2_alpha, 512, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(set_err(FEMTO_AMD_ERR_INVALID, "hipMemcpy(p2_alpha)"));
    for (auto& a : alpha)
      if (a >= kAlphaSize) a = 0;
  }
  if (hipMemcpy(ex->d_alpha, alpha.data(), 512, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ex->d_doc_ends, h.doc_ends.data(), size_t(nd) * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_err(FEMTO_AMD_ERR_INVALID, "hipMemcpy(extractor tables)"));
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES) {
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = build_samples(ex.get()))) return fail(rc);
    ex->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  *out = ex.release();
  return FEMTO_AMD_OK;
  API_END
}

void femto_amd_extractor_free(femto_amd_extractor_t* ex) {
  if (ex) free_extractor(ex);
}

int femto_amd_extractor_info(const femto_amd_extractor_t* ex, int* path, int* sample_shift, int64_t* bytes, double* build_ms) {
  if (!ex) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (path) *path = ex->path;
  if (sample_shift) *sample_shift = ex->path == FEMTO_AMD_EXTRACT_PATH_SAMPLES ? ex->shift : -1;
  if (bytes) *bytes = ex->bytes;
  if (build_ms) *build_ms = ex->build_ms;
  return FEMTO_AMD_OK;
}

int femto_amd_extractor_eof_rows(const femto_amd_extractor_t* ex, int64_t* rows, int64_t n) {
  if (!ex || n < 0 || (n && !rows)) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (ex->path != FEMTO_AMD_EXTRACT_PATH_SAMPLES) return set_err(FEMTO_AMD_ERR_INVALID, "only the sample path records the SEOF rows");
  if (n != int64_t(ex->h_eof.size())) return set_err(FEMTO_AMD_ERR_PARAM, "n must be the number of documents");
  if (n) memcpy(rows, ex->h_eof.data(), size_t(n) * 8);
  return FEMTO_AMD_OK;
}

int femto_amd_extract_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_pos, const int32_t* d_len, const int64_t* d_out_starts,
                             uint16_t* d_out, void* stream) {
  API_BEGIN
  if (!ex || n < 0 || (n && (!d_pos || !d_len || !d_out_starts || !d_out))) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (ex->multi) return refuse_multi_device();
  int rc = ensure_device(ex->ix);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Lease L(ex->ix, st);
  if (!L.s) return L.rc;
  XReqs R{};
  R.pos = d_pos;
  R.len = d_len;
  R.out_start = d_out_starts;
  R.n = n;
  return run_extract(ex, *L.s, R, d_out, st);
  API_END
}

int femto_amd_context_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_rows, const int64_t* d_offsets, const int64_t* d_n,
                             int before, int after, uint16_t* d_ctx, int64_t* d_pos_out, void* stream) {
  API_BEGIN
  if (!ex || n < 0 || before < 0 || after < 0 || int64_t(before) + after > (int64_t(1) << 30) || (!d_rows == !d_offsets) ||
      (n && int64_t(before) + after > 0 && !d_ctx))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (exactly one of rows and offsets; 0 <= before, after; before + after <= 2^30)");
  if (ex->multi) return refuse_multi_device();
  int rc = ensure_device(ex->ix);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Lease L(ex->ix, st);
  if (!L.s) return L.rc;
  return run_context(ex, *L.s, n, d_rows, d_offsets, d_n, before, after, d_ctx, d_pos_out, st);
  API_END
}

int femto_amd_extract(femto_amd_extractor_t* ex, int64_t n, const int64_t* pos, const int32_t* len, const int64_t* out_starts, uint16_t* out) {
  API_BEGIN
  if (!ex || n < 0 || (n && (!pos || !len || !out))) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (len[i] < 0) return set_err(FEMTO_AMD_ERR_PARAM, "negative length");
    if (out_starts && out_starts[i] < 0) return set_err(FEMTO_AMD_ERR_PARAM, "negative output start");
    total += len[i];
  }
  femto_amd_index* ix = ex->ix;
  int rc = ensure_device(ix);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  Lease L(ix);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  hipStream_t st = S.stream;
  if ((rc = S.pats.reserve(size_t(n) * 8)) || (rc = S.plen.reserve(size_t(n) * 4)) || (rc = S.off.reserve(size_t(total) * 2 + 16))) return rc;
  HIP_TRY(hipMemcpyAsync(S.pats.p, pos, size_t(n) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(S.plen.p, len, size_t(n) * 4, hipMemcpyHostToDevice, st));
  XReqs R{};
  R.pos = S.pats.as<int64_t>();
  R.len = S.plen.as<int32_t>();
  R.n = n;
  if ((rc = run_extract(ex, S, R, S.off.as<uint16_t>(), st))) return rc;      // packed: request i at sum(len[:i])
  if (!out_starts) {
    if (total) HIP_TRY(hipMemcpyAsync(out, S.off.p, size_t(total) * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FEMTO_AMD_OK;
  }
  std::vector<uint16_t> packed(size_t(total) + 1);
  if (total) HIP_TRY(hipMemcpyAsync(packed.data(), S.off.p, size_t(total) * 2, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int64_t at = 0;
  for (int64_t i = 0; i < n; i++) {
    if (len[i]) memcpy(out + out_starts[i], packed.data() + at, size_t(len[i]) * 2);
    at += len[i];
  }
  return FEMTO_AMD_OK;
  API_END
}

int femto_amd_context(femto_amd_extractor_t* ex, int64_t n, const int64_t* rows, const int64_t* offsets, int before, int after, uint16_t* ctx,
                      int64_t* pos_out) {
  API_BEGIN
  if (!ex || n < 0 || before < 0 || after < 0 || int64_t(before) + after > (int64_t(1) << 30) || (!rows == !offsets) ||
      (n && int64_t(before) + after > 0 && !ctx))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (exactly one of rows and offsets; 0 <= before, after; before + after <= 2^30)");
  femto_amd_index* ix = ex->ix;
  int rc = ensure_device(ix);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  const int64_t W = int64_t(before) + after;
  Lease L(ix);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  hipStream_t st = S.stream;
  if ((rc = S.noccs.reserve(size_t(n) * 8)) || (rc = S.pats.reserve(size_t(n) * 8)) || (rc = S.off.reserve(size_t(n * W) * 2 + 16))) return rc;
  HIP_TRY(hipMemcpyAsync(S.noccs.p, rows ? rows : offsets, size_t(n) * 8, hipMemcpyHostToDevice, st));
  const int64_t* anchors = S.noccs.as<int64_t>();
  if ((rc = run_context(ex, S, n, rows ? anchors : nullptr, rows ? nullptr : anchors, nullptr, before, after, S.off.as<uint16_t>(),
                        S.pats.as<int64_t>(), st)))
    return rc;
  if (W) HIP_TRY(hipMemcpyAsync(ctx, S.off.p, size_t(n * W) * 2, hipMemcpyDeviceToHost, st));
  if (pos_out) HIP_TRY(hipMemcpyAsync(pos_out, S.pats.p, size_t(n) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return FEMTO_AMD_OK;
  API_END
}

int femto_amd_extract_document(femto_amd_extractor_t* ex, int64_t doc, uint16_t** content, int64_t* len) {
  API_BEGIN
  if (!ex || !content || !len) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *content = nullptr;
  *len = 0;
  const std::vector<int64_t>& de = ex->ix->host.doc_ends;
  if (doc < 0 || doc >= int64_t(de.size())) return set_err(FEMTO_AMD_ERR_PARAM, "no such document");
  const int64_t ds = doc ? de[size_t(doc) - 1] : 0, dl = de[size_t(doc)] - ds;     // document_length (index.c): bytes + SEOF
  // requests of at most 2^30 symbols
  const int64_t piece = int64_t(1) << 30, np = (dl + piece - 1) / piece;
  std::vector<int64_t> pos(static_cast<size_t>(np));
  std::vector<int32_t> lens(static_cast<size_t>(np));
  for (int64_t k = 0; k < np; k++) {
    pos[size_t(k)] = ds + k * piece;
    lens[size_t(k)] = int32_t(std::min(piece, dl - k * piece));
  }
  uint16_t* buf = static_cast<uint16_t*>(malloc(size_t(dl > 0 ? dl : 1) * 2));
  if (!buf) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  const int rc = femto_amd_extract(ex, np, pos.data(), lens.data(), nullptr, buf);
  if (rc) {
    free(buf);
    return rc;
  }
  *content = buf;
  *len = dl;
  return FEMTO_AMD_OK;
  API_END
}
