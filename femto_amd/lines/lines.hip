// lines.hip -- the line around every hit, served from the index: its bounds, its bytes and the groups of equal lines
// (print_grep / grep_group_add, src/main_cc/search_tool.cc:134-176, 278-351, with the document's bytes as the index holds them in
// place of the file).  include/femto_amd.h "matching lines" states the rule; DESIGN.md "Matching lines" the kernels.
//
// BOUNDS.  16 lanes per anchor, four anchors per wavefront.  A round covers 256 positions behind the anchor and 256 from it on;
// every lane turns its 16 positions into a mask of the terminators (\n, \r, \0) inside the scan's window -- at most 1023 positions
// back, 1024 forward, never outside the document -- and the group takes the nearest one from a ballot of "my mask is not empty"
// and a clz / ctz of that lane's mask.  At most four rounds; a group whose two scans are done idles until its wavefront's other
// groups are.  The positions come from one of two sources: the handle's text (d_txt, dense codes: two or three aligned 8-byte
// loads and a funnel shift per lane) or, on the sample path, the contexts femto_amd_context_device(1023, 1024) wrote to scratch.
//
// BYTES.  The lines packed one after another (exclusive scan of the lengths); a thread owns 16 consecutive output bytes and finds
// its line by binary search within the few lines its workgroup covers.  On the sample path the symbols come from the extractor
// (femto_amd_extract_device on exactly the lines' positions, in pieces of at most 2^26 symbols) and are narrowed to bytes.
//
// GROUPS.  One hash per line (16 lanes per line, a multiply-mix over 8-byte words, the length folded in), a stable radix sort of
// (hash, index), and every element compared BYTE BY BYTE with the head of its run; the elements that differ from their head
// (collisions) scan their run from the head for the first equal line.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../common/block.hpp"
#include "../extract/extractor.hpp"

namespace femto_amd {
namespace {

constexpr int kMaxLine = 1024;                    // MAX_GREP_LINE (search_tool.cc:74)
constexpr int kBefore = kMaxLine - 1, kAfter = kMaxLine, kCtxW = kBefore + kAfter;
constexpr int kRound = 256;                       // positions per direction and round: 16 lanes x 16
constexpr int64_t kChunkAnchors = 65536;          // sample path: 65536 contexts of 2047 symbols are just under 256 MiB
constexpr int64_t kChunkSyms = int64_t(1) << 26;  // ... and the bytes come through 128 MiB of symbols at a time
constexpr uint16_t kNL = '\n' + FEMTO_AMD_CHARACTER_OFFSET, kCR = '\r' + FEMTO_AMD_CHARACTER_OFFSET, kNUL = FEMTO_AMD_CHARACTER_OFFSET;
constexpr uint64_t kExcluded = uint64_t(1) << 63; // sort key of a slot that is not live or not valid (hashes keep 63 bits)
constexpr int64_t kPending = -2;                  // group_first of an element that differs from the head of its run

// bits k of 16 with lo <= q0 + k < hi
__device__ __forceinline__ uint32_t window_mask(int64_t q0, int64_t lo, int64_t hi) {
  const int64_t a = lo - q0 < 0 ? 0 : (lo - q0 > 16 ? 16 : lo - q0);
  const int64_t b = hi - q0 < 0 ? 0 : (hi - q0 > 16 ? 16 : hi - q0);
  return b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
}

// ---- the two sources of a scan: masks() gives, for the positions q0 + k with bit k of `valid` set, the terminators and the \0s

struct TextSrc {
  const uint8_t* txt;        // one dense code per position, 64 bytes of slack behind the last
  const uint16_t* alpha;     // dense code -> alpha code
  int c_nl, c_cr, c_nul;     // the dense codes of the three stop bytes; 256 (no byte's code) for one the alphabet lacks
  // the whole wavefront: alpha inverted for the three bytes
  __device__ __forceinline__ void init() {
    c_nl = c_cr = c_nul = 256;
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < 4; j++) {
      const uint16_t a = alpha[lane + 64 * j];
      unsigned long long m;
      if ((m = __ballot(a == kNL))) c_nl = 64 * j + __ffsll(m) - 1;
      if ((m = __ballot(a == kCR))) c_cr = 64 * j + __ffsll(m) - 1;
      if ((m = __ballot(a == kNUL))) c_nul = 64 * j + __ffsll(m) - 1;
    }
  }
  __device__ __forceinline__ void masks(int64_t, int64_t, int64_t q0, uint32_t valid, uint32_t* term, uint32_t* nul) const {
    *term = *nul = 0;
    if (!valid) return;
    const int64_t qs = q0 < 0 ? 0 : q0;     // (a valid position is >= 0: q0 > -16)
    const int back = int(qs - q0);
    const uint64_t* w = reinterpret_cast<const uint64_t*>(txt + (qs & ~int64_t(7)));
    const uint32_t sh = uint32_t(qs & 7) * 8u;
    const uint64_t w0 = w[0], w1 = w[1];
    uint64_t lo = w0, hi = w1;
    if (sh) {
      const uint64_t w2 = w[2];
      lo = (w0 >> sh) | (w1 << (64u - sh));
      hi = (w1 >> sh) | (w2 << (64u - sh));
    }
    uint32_t t = 0, z = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int b = int(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 0xffu);
      t |= uint32_t(b == c_nl || b == c_cr || b == c_nul) << k;
      z |= uint32_t(b == c_nul) << k;
    }
    *term = (t << back) & valid;
    *nul = (z << back) & valid;
  }
};

struct CtxSrc {
  const uint16_t* ctx;       // slot i's anchor p is ctx[i * kCtxW + kBefore]
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ void masks(int64_t slot, int64_t p, int64_t q0, uint32_t valid, uint32_t* term, uint32_t* nul) const {
    uint32_t t = 0, z = 0;
    const int64_t at = slot * kCtxW + kBefore + (q0 - p);     // (a valid position lies in [p - 1023, p + 1023])
#pragma unroll
    for (int k = 0; k < 16; k++)
      if ((valid >> k) & 1u) {
        const uint16_t a = ctx[at + k];
        t |= uint32_t(a == kNL || a == kCR || a == kNUL) << k;
        z |= uint32_t(a == kNUL) << k;
      }
    *term = t;
    *nul = z;
  }
};

template <class Src>
__global__ __launch_bounds__(256) void lines_bounds_kernel(Src src, const int64_t n, const int64_t* __restrict__ d_n,
                                                           const int64_t* __restrict__ offsets, const int64_t N,
                                                           const int64_t* __restrict__ doc_ends, const int64_t ndocs,
                                                           int64_t* __restrict__ out_doc, int64_t* __restrict__ out_pos,
                                                           int32_t* __restrict__ out_len, uint8_t* __restrict__ out_flags) {
  src.init();
  const int lane = threadIdx.x & 63, gl = lane & 15, gbase = lane & 48;
  const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const bool active = i < live_of(d_n, n);
  const int64_t p = active ? offsets[i] : 0;
  const bool valid_anchor = active && p >= 0 && p < N;
  int64_t doc = -1, ds = 0, de1 = 0;       // de1: the position of the document's SEOF (o == L)
  if (valid_anchor) {
    const Doc D = doc_of(doc_ends, ndocs, p);
    doc = D.doc;
    ds = D.start;
    de1 = D.end - 1;
  }
  const int64_t blo = p - kBefore > ds ? p - kBefore : ds;       // the backward scan sees [blo, p) ...
  const int64_t fhi = p + kAfter < de1 ? p + kAfter : de1;       // ... the forward scan [p, fhi)
  bool bdone = !valid_anchor, fdone = !valid_anchor, binary = false;
  int64_t lstart = p, lend = p;
  for (int r = 0; r < kMaxLine / kRound; r++) {
    if (!__ballot(!bdone || !fdone)) break;
    uint32_t t, z;
    {   // backward: lane 0 holds the 16 positions next to the anchor; the nearest terminator is the highest bit of the first lane
      const int64_t q0 = p - int64_t(kRound) * r - 16 * (gl + 1);
      src.masks(i, p, q0, bdone ? 0u : window_mask(q0, blo, p), &t, &z);
      const uint32_t gf = uint32_t(__ballot(t != 0) >> gbase) & 0xffffu;
      const int first = gf ? __ffs(int(gf)) - 1 : 0;
      const uint32_t tm = __shfl(t, gbase + first), zm = __shfl(z, gbase + first);
      if (!bdone) {
        if (gf) {
          const int k = 31 - __clz(int(tm));
          lstart = p - int64_t(kRound) * r - 16 * (first + 1) + k + 1;
          binary = binary || ((zm >> k) & 1u);
          bdone = true;
        } else if (p - int64_t(kRound) * (r + 1) <= blo) {
          lstart = blo;
          if (p - ds >= kBefore) binary = true;      // the loop ran out: 1023 bytes and no terminator
          bdone = true;
        }
      }
    }
    {   // forward: the lowest bit of the first lane
      const int64_t q0 = p + int64_t(kRound) * r + 16 * gl;
      src.masks(i, p, q0, fdone ? 0u : window_mask(q0, p, fhi), &t, &z);
      const uint32_t gf = uint32_t(__ballot(t != 0) >> gbase) & 0xffffu;
      const int first = gf ? __ffs(int(gf)) - 1 : 0;
      const uint32_t tm = __shfl(t, gbase + first), zm = __shfl(z, gbase + first);
      if (!fdone) {
        if (gf) {
          const int k = __ffs(int(tm)) - 1;
          lend = p + int64_t(kRound) * r + 16 * first + k;
          binary = binary || ((zm >> k) & 1u);
          fdone = true;
        } else if (p + int64_t(kRound) * (r + 1) >= fhi) {
          if (de1 - p >= kAfter) {                   // the loop ran out: 1024 bytes and no terminator
            lend = p + kAfter - 1;
            binary = true;
          } else {
            lend = de1 > p ? de1 - 1 : p;            // the document ends first: line_end is the last byte it looked at
          }
          fdone = true;
        }
      }
    }
  }
  if (!active || gl) return;
  if (out_doc) out_doc[i] = doc;
  if (out_pos) out_pos[i] = valid_anchor ? lstart : -1;
  if (out_len) out_len[i] = valid_anchor ? int32_t(lend - lstart) : 0;
  if (out_flags) out_flags[i] = valid_anchor ? (binary ? FEMTO_AMD_LINE_BINARY : 0) : FEMTO_AMD_LINE_INVALID;
}

// sample path: the live count of every chunk of kChunkAnchors anchors
__global__ __launch_bounds__(256) void lines_chunk_live_kernel(const int64_t n, const int64_t* __restrict__ d_n, const int64_t nchunks,
                                                               int64_t* __restrict__ out) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const int64_t left = live_of(d_n, n) - c * kChunkAnchors;
  out[c] = left < 0 ? 0 : (left < kChunkAnchors ? left : kChunkAnchors);
}

// ---- bytes --------------------------------------------------------------------------------------------------------------------

// the lengths the copy trusts: live, a start inside the text, no further than the text goes
__global__ __launch_bounds__(256) void lines_lens_kernel(const int64_t n, const int64_t* __restrict__ d_n, const int64_t* __restrict__ line_pos,
                                                         const int32_t* __restrict__ line_len, const int64_t N, int64_t* __restrict__ lens64) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t len = 0;
  if (i < live_of(d_n, n)) {
    const int64_t pos = line_pos[i];
    len = line_len[i];
    if (pos < 0 || pos >= N || len < 0) len = 0;
    else if (len > N - pos) len = N - pos;
  }
  lens64[i] = len;
}

constexpr int kBytesPerThread = 16;
constexpr int kTileBytes = 256 * kBytesPerThread;

__global__ __launch_bounds__(256) void lines_copy_kernel(const int64_t n, const int64_t* __restrict__ cum, const int64_t* __restrict__ line_pos,
                                                         const uint8_t* __restrict__ txt, const uint16_t* __restrict__ alpha,
                                                         uint8_t* __restrict__ out, const int64_t capacity, int64_t* __restrict__ d_total) {
  __shared__ uint8_t s_byte[256];
  __shared__ int64_t s_r[2];
  s_byte[threadIdx.x] = uint8_t(alpha[threadIdx.x] - FEMTO_AMD_CHARACTER_OFFSET);
  const int64_t total = cum[n];
  if (blockIdx.x == 0 && threadIdx.x == 0) write_total(d_total, total, capacity);
  const int64_t lim = total < capacity ? total : capacity;
  for (int64_t base = int64_t(blockIdx.x) * kTileBytes; base < lim; base += int64_t(gridDim.x) * kTileBytes) {
    __syncthreads();
    if (threadIdx.x < 2) {
      const int64_t v = threadIdx.x == 0 ? base : (base + kTileBytes - 1 < lim ? base + kTileBytes - 1 : lim - 1);
      s_r[threadIdx.x] = first_gt(cum, 0, n + 1, v) - 1;
    }
    __syncthreads();
    const int64_t v0 = base + int64_t(threadIdx.x) * kBytesPerThread;
    if (v0 >= lim) continue;
    int64_t r = first_gt(cum, s_r[0], s_r[1] + 1, v0) - 1;
    int64_t c0 = cum[r], c1 = cum[r + 1];
    const int64_t vend = v0 + kBytesPerThread < lim ? v0 + kBytesPerThread : lim;
    if (vend - v0 == kBytesPerThread && v0 + kBytesPerThread <= c1) {      // 16 bytes of one line
      const int64_t q0 = line_pos[r] + (v0 - c0);
      const uint64_t* w = reinterpret_cast<const uint64_t*>(txt + (q0 & ~int64_t(7)));
      const uint32_t sh = uint32_t(q0 & 7) * 8u;
      uint64_t lo = w[0], hi = w[1];
      if (sh) {
        const uint64_t w2 = w[2];      // (d_txt has 64 bytes of slack)
        lo = (lo >> sh) | (hi << (64u - sh));
        hi = (hi >> sh) | (w2 << (64u - sh));
      }
      uint32_t pk[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t c = uint32_t((k < 2 ? lo : hi) >> (32 * (k & 1)));
        pk[k] = uint32_t(s_byte[c & 0xffu]) | (uint32_t(s_byte[(c >> 8) & 0xffu]) << 8) | (uint32_t(s_byte[(c >> 16) & 0xffu]) << 16) |
                (uint32_t(s_byte[c >> 24]) << 24);
      }
      uint8_t* dst = out + v0;
      if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) dst[k] = uint8_t(pk[k >> 2] >> (8 * (k & 3)));
      }
      continue;
    }
    for (int64_t v = v0; v < vend; v++) {
      while (v >= c1) {
        r++;
        c0 = c1;
        c1 = cum[r + 1];
      }
      out[v] = s_byte[txt[line_pos[r] + (v - c0)]];
    }
  }
}

// sample path: the part of every line that falls into output bytes [v_lo, v_hi), as a request to the extractor
__global__ __launch_bounds__(256) void lines_piece_kernel(const int64_t n, const int64_t* __restrict__ cum, const int64_t* __restrict__ line_pos,
                                                          const int64_t v_lo, const int64_t v_hi, int64_t* __restrict__ pos,
                                                          int32_t* __restrict__ len, int64_t* __restrict__ out_start) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c0 = cum[i], c1 = cum[i + 1];
  const int64_t a = c0 > v_lo ? c0 : v_lo, b = c1 < v_hi ? c1 : v_hi;
  const bool some = b > a;
  pos[i] = some ? line_pos[i] + (a - c0) : 0;
  len[i] = some ? int32_t(b - a) : 0;
  out_start[i] = some ? a - v_lo : 0;
}

// ... and its symbols narrowed to bytes
__global__ __launch_bounds__(256) void lines_narrow_kernel(const int64_t n, const int64_t* __restrict__ cum, const uint16_t* __restrict__ syms,
                                                           const int64_t v_lo, const int64_t v_hi, uint8_t* __restrict__ out, const int64_t capacity,
                                                           int64_t* __restrict__ d_total) {
  const int64_t total = cum[n];
  if (blockIdx.x == 0 && threadIdx.x == 0 && d_total) write_total(d_total, total, capacity);
  int64_t lim = total < capacity ? total : capacity;
  if (v_hi < lim) lim = v_hi;
  for (int64_t v = v_lo + int64_t(blockIdx.x) * 256 + threadIdx.x; v < lim; v += int64_t(gridDim.x) * 256)
    out[v] = uint8_t(syms[v - v_lo] - FEMTO_AMD_CHARACTER_OFFSET);
}

// ---- groups -------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 32;
  x *= 0xd6e8feb86659fd93ull;
  x ^= x >> 29;
  return x;
}

// 16 lanes per line: lane l takes the 8-byte words l, l + 16, ... of the line
__global__ __launch_bounds__(256) void lines_hash_kernel(const int64_t n, const int64_t* __restrict__ d_n, const int64_t* __restrict__ cum,
                                                         const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ flags, const uint64_t keep,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int gl = threadIdx.x & 15;
  const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const bool in = i < n;
  const bool ok = in && i < live_of(d_n, n) && !(flags && (flags[i] & FEMTO_AMD_LINE_INVALID));
  const int64_t s = ok ? cum[i] : 0, len = ok ? cum[i + 1] - s : 0;
  uint64_t h = 0;
  for (int64_t w = gl; 8 * w < len; w += 16) {
    const uint8_t* at = bytes + s + 8 * w;
    uint64_t x = 0;
    if (8 * w + 8 <= len) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(at);
      const uint64_t* q = reinterpret_cast<const uint64_t*>(a & ~uintptr_t(7));
      const uint32_t sh = uint32_t(a & 7) * 8u;
      x = sh ? ((q[0] >> sh) | (q[1] << (64u - sh))) : q[0];     // (q[1] holds bytes of this word: it starts inside the line)
    } else {
      for (int k = 0; 8 * w + k < len; k++) x |= uint64_t(at[k]) << (8 * k);
    }
    h += mix64((x + uint64_t(w + 1) * 0x9e3779b97f4a7c15ull) * 0xff51afd7ed558ccdull);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) h += __shfl_xor(h, o);
  if (!in || gl) return;
  h = mix64(h + uint64_t(len) * 0xc4ceb9fe1a85ec53ull);
  keys[i] = ok ? (h & keep & ~kExcluded) : kExcluded;
  idx[i] = uint32_t(i);
}

struct PackedLines {
  const int64_t* cum;
  const uint8_t* bytes;
};

__device__ __forceinline__ bool line_equal_serial(const PackedLines& P, int64_t a, int64_t b) {
  const int64_t sa = P.cum[a], sb = P.cum[b], len = P.cum[a + 1] - sa;
  if (P.cum[b + 1] - sb != len) return false;
  for (int64_t k = 0; k < len; k++)
    if (P.bytes[sa + k] != P.bytes[sb + k]) return false;
  return true;
}

// 16 lanes per sorted element: the head of its run is the first element with its key; equal bytes -> the head's index
__global__ __launch_bounds__(256) void lines_heads_kernel(const int64_t n, const int64_t* __restrict__ d_n, const PackedLines P,
                                                          const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                          int64_t* __restrict__ group_first) {
  const int lane = threadIdx.x & 63, gl = lane & 15, gbase = lane & 48;
  const int64_t s = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const bool in = s < n;
  const uint64_t key = in ? keys[s] : kExcluded;
  const bool ok = in && !(key & kExcluded);
  const int64_t i = in ? int64_t(idx[s]) : 0;
  int64_t head = i;
  bool differ = false;
  if (ok) {
    head = int64_t(idx[first_ge(keys, 0, n, int64_t(key))]);      // (keys below 2^63 compare alike signed and unsigned)
    if (head != i) {
      const int64_t sa = P.cum[i], sb = P.cum[head], len = P.cum[i + 1] - sa;
      differ = P.cum[head + 1] - sb != len;
      for (int64_t k = gl; !differ && k < len; k += 16) differ = P.bytes[sa + k] != P.bytes[sb + k];
    }
  }
  const bool any = (uint32_t(__ballot(differ) >> gbase) & 0xffffu) != 0;
  if (!in || gl) return;
  if (ok) group_first[i] = any ? kPending : head;
  else if (i < live_of(d_n, n)) group_first[i] = -1;      // live and INVALID; the slots beyond the live count stay as they are
}

// one thread per collision: the first equal line of its run (stable sort: ascending indexes), else itself
__global__ __launch_bounds__(256) void lines_collide_kernel(const int64_t n, const PackedLines P, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ idx, int64_t* __restrict__ group_first) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= n) return;
  const uint64_t key = keys[s];
  if (key & kExcluded) return;
  const int64_t i = int64_t(idx[s]);
  if (group_first[i] != kPending) return;
  int64_t g = i;
  for (int64_t j = first_ge(keys, 0, n, int64_t(key)) + 1; j < s; j++)      // (the head itself differs)
    if (line_equal_serial(P, i, int64_t(idx[j]))) {
      g = int64_t(idx[j]);
      break;
    }
  group_first[i] = g;
}

__global__ __launch_bounds__(256) void lines_count_kernel(const int64_t n, const int64_t* __restrict__ d_n, const int64_t* __restrict__ group_first,
                                                          unsigned long long* __restrict__ ngroups) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const unsigned long long m = __ballot(i < live_of(d_n, n) && group_first[i] == i);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ngroups, static_cast<unsigned long long>(__popcll(m)));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

inline dim3 groups_of(int64_t n) { return dim3(uint32_t((n + 15) / 16)); }      // 16 lanes per element, 256-thread workgroups

constexpr int64_t kMaxCall = int64_t(1) << 31;

int run_bounds(femto_amd_extractor* ex, int64_t n, const int64_t* d_offsets, const int64_t* d_n, int64_t* d_doc, int64_t* d_line_pos,
               int32_t* d_line_len, uint8_t* d_flags, hipStream_t st) {
  femto_amd_index* ix = ex->ix;
  const int64_t N = ix->host.total_length, nd = int64_t(ix->host.doc_ends.size());
  int rc;
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_TEXT) {
    TextSrc src{ix->d_txt, ex->d_alpha, 256, 256, 256};
    return launch(lines_bounds_kernel<TextSrc>, groups_of(n), st, src, n, d_n, d_offsets, N, ex->d_doc_ends, nd, d_doc, d_line_pos, d_line_len,
                  d_flags);
  }
  // sample path: the contexts of a chunk of anchors into scratch, the same scan over them.  No scratch of the handle is leased
  // across femto_amd_context_device, which leases its own.
  const int64_t nchunks = (n + kChunkAnchors - 1) / kChunkAnchors;
  Temp T;
  uint16_t* ctx;
  int64_t* d_live;
  if ((rc = T.get(&ctx, size_t(std::min(n, kChunkAnchors)) * kCtxW)) || (rc = T.get(&d_live, size_t(nchunks)))) return rc;
  if ((rc = launch(lines_chunk_live_kernel, blocks_of(nchunks), st, n, d_n, nchunks, d_live))) return rc;
  for (int64_t c = 0; c < nchunks; c++) {
    const int64_t c0 = c * kChunkAnchors, cn = std::min(kChunkAnchors, n - c0);
    if ((rc = femto_amd_context_device(ex, cn, nullptr, d_offsets + c0, d_live + c, kBefore, kAfter, ctx, nullptr, st))) return rc;
    if ((rc = launch(lines_bounds_kernel<CtxSrc>, groups_of(cn), st, CtxSrc{ctx}, cn, d_live + c, d_offsets + c0, N, ex->d_doc_ends, nd,
                     d_doc ? d_doc + c0 : nullptr, d_line_pos ? d_line_pos + c0 : nullptr, d_line_len ? d_line_len + c0 : nullptr,
                     d_flags ? d_flags + c0 : nullptr)))
      return rc;
  }
  return 0;      // (~Temp frees the scratch: hipFree waits for the work enqueued above)
}

// capacity 0 and d_bytes NULL: the starts and the total only
int run_bytes(femto_amd_extractor* ex, int64_t n, const int64_t* d_n, const int64_t* d_line_pos, const int32_t* d_line_len, int64_t* d_byte_starts,
              uint8_t* d_bytes, int64_t capacity, int64_t* d_total, hipStream_t st) {
  femto_amd_index* ix = ex->ix;
  const int64_t N = ix->host.total_length;
  int rc;
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_TEXT) {
    Lease L(ix, st);
    if (!L.s) return L.rc;
    Scratch& S = *L.s;
    if ((rc = S.noccs64.reserve(size_t(n) * 8))) return rc;
    if ((rc = launch(lines_lens_kernel, blocks_of(n), st, n, d_n, d_line_pos, d_line_len, N, S.noccs64.as<int64_t>())) ||
        (rc = device_scan(S.scan, n, S.noccs64.as<int64_t>(), d_byte_starts, 0, st)))
      return rc;
    return launch(lines_copy_kernel, persistent_grid(ix, (int64_t(1) << 40) / kTileBytes), st, n, d_byte_starts, d_line_pos, ix->d_txt, ex->d_alpha,
                  d_bytes, capacity, d_total);
  }
  Temp T;
  int64_t *lens64, *pos, *ostart;
  int32_t* len;
  uint16_t* syms;
  const int64_t nchunks = (capacity + kChunkSyms - 1) / kChunkSyms;
  if ((rc = T.get(&lens64, size_t(n))) || (rc = T.get(&pos, size_t(n))) || (rc = T.get(&ostart, size_t(n))) || (rc = T.get(&len, size_t(n))) ||
      (rc = T.get(&syms, size_t(std::min(capacity, kChunkSyms)))))
    return rc;
  if ((rc = launch(lines_lens_kernel, blocks_of(n), st, n, d_n, d_line_pos, d_line_len, N, lens64)) ||
      (rc = device_scan(T.scan, n, lens64, d_byte_starts, 0, st)))
    return rc;
  const dim3 grid = persistent_grid(ix, (int64_t(1) << 40) / 256);
  if (nchunks == 0) return launch(lines_narrow_kernel, dim3(1), st, n, d_byte_starts, syms, int64_t(0), int64_t(0), d_bytes, capacity, d_total);
  for (int64_t c = 0; c < nchunks; c++) {
    const int64_t v_lo = c * kChunkSyms, v_hi = std::min(capacity, v_lo + kChunkSyms);
    if ((rc = launch(lines_piece_kernel, blocks_of(n), st, n, d_byte_starts, d_line_pos, v_lo, v_hi, pos, len, ostart)) ||
        (rc = femto_amd_extract_device(ex, n, pos, len, ostart, syms, st)) ||
        (rc = launch(lines_narrow_kernel, grid, st, n, d_byte_starts, syms, v_lo, v_hi, d_bytes, capacity, c == 0 ? d_total : nullptr)))
      return rc;
  }
  return 0;
}

int run_groups(femto_amd_index* ix, int64_t n, const int64_t* d_n, const int64_t* d_byte_starts, const uint8_t* d_bytes, const uint8_t* d_flags,
               int hash_bits, int64_t* d_group_first, int64_t* d_ngroups, hipStream_t st) {
  int rc;
  HIP_TRY(hipMemsetAsync(d_ngroups, 0, 8, st));
  if (n == 0) return 0;
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                    static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), size_t(n), 0u, 64u, st));
  if ((rc = S.keys.reserve(size_t(n) * 8)) || (rc = S.keys2.reserve(size_t(n) * 8)) || (rc = S.idx.reserve(size_t(n) * 4)) ||
      (rc = S.idx2.reserve(size_t(n) * 4)) || (rc = S.sorttmp.reserve(tmp_bytes ? tmp_bytes : 16)))
    return rc;
  const uint64_t keep = (hash_bits <= 0 || hash_bits >= 64) ? ~uint64_t(0) : (uint64_t(1) << hash_bits) - 1;
  const PackedLines P{d_byte_starts, d_bytes};
  if ((rc = launch(lines_hash_kernel, groups_of(n), st, n, d_n, d_byte_starts, d_bytes, d_flags, keep, S.keys.as<uint64_t>(), S.idx.as<uint32_t>())))
    return rc;
  HIP_TRY(rocprim::radix_sort_pairs(S.sorttmp.p, tmp_bytes, S.keys.as<uint64_t>(), S.keys2.as<uint64_t>(), S.idx.as<uint32_t>(), S.idx2.as<uint32_t>(),
                                    size_t(n), 0u, 64u, st));
  if ((rc = launch(lines_heads_kernel, groups_of(n), st, n, d_n, P, S.keys2.as<uint64_t>(), S.idx2.as<uint32_t>(), d_group_first)) ||
      (rc = launch(lines_collide_kernel, blocks_of(n), st, n, P, S.keys2.as<uint64_t>(), S.idx2.as<uint32_t>(), d_group_first)))
    return rc;
  return launch(lines_count_kernel, blocks_of(n), st, n, d_n, d_group_first, reinterpret_cast<unsigned long long*>(d_ngroups));
}

// what every call checks of its extractor; device forms refuse a multi-device handle
int check_extractor(femto_amd_extractor* ex, bool device_form) {
  if (!ex) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (device_form && ex->multi) return refuse_multi_device();
  return check_plain_handle(ex->ix, "matching lines are");
}

}  // namespace
}  // namespace femto_amd

int femto_amd_lines_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_offsets, const int64_t* d_n, int64_t* d_doc, int64_t* d_line_pos,
                           int32_t* d_line_len, uint8_t* d_flags, void* stream) {
  API_BEGIN
  if (!ex || n < 0 || n >= kMaxCall || (n && !d_offsets)) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 anchors)");
  int rc = check_extractor(ex, true);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  return run_bounds(ex, n, d_offsets, d_n, d_doc, d_line_pos, d_line_len, d_flags, static_cast<hipStream_t>(stream));
  API_END
}

int femto_amd_line_bytes_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_n, const int64_t* d_line_pos, const int32_t* d_line_len,
                                int64_t* d_byte_starts, uint8_t* d_bytes, int64_t capacity, int64_t* d_total, void* stream) {
  API_BEGIN
  if (!ex || n < 0 || n >= kMaxCall || capacity < 0 || !d_byte_starts || !d_total || (capacity && !d_bytes) || (n && (!d_line_pos || !d_line_len)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 lines)");
  int rc = check_extractor(ex, true);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) return empty_result_async(d_byte_starts, d_total, st);
  return run_bytes(ex, n, d_n, d_line_pos, d_line_len, d_byte_starts, d_bytes, capacity, d_total, st);
  API_END
}

int femto_amd_line_groups_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_n, const int64_t* d_byte_starts, const uint8_t* d_bytes,
                                 const uint8_t* d_flags, int hash_bits, int64_t* d_group_first, int64_t* d_ngroups, void* stream) {
  API_BEGIN
  if (!ex || n < 0 || n >= kMaxCall || hash_bits < 0 || hash_bits > 64 || !d_ngroups || (n && (!d_byte_starts || !d_group_first)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 lines, 0 <= hash_bits <= 64)");
  int rc = check_extractor(ex, true);
  if (rc) return rc;
  return run_groups(ex->ix, n, d_n, d_byte_starts, d_bytes, d_flags, hash_bits, d_group_first, d_ngroups, static_cast<hipStream_t>(stream));
  API_END
}

int femto_amd_lines(femto_amd_extractor_t* ex, int64_t n, const int64_t* offsets, int64_t* doc, int64_t* line_pos, int32_t* line_len, uint8_t* flags,
                    int64_t* byte_starts, uint8_t** bytes, int64_t* total) {
  API_BEGIN
  if (!ex || n < 0 || n >= kMaxCall || (n && !offsets) || (!bytes != !byte_starts) || (bytes && !total))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 anchors; byte_starts, bytes and total go together)");
  if (bytes) {
    *bytes = nullptr;
    *total = 0;
    byte_starts[0] = 0;
  }
  int rc = check_extractor(ex, false);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  Temp T;
  int64_t *d_off, *d_doc, *d_pos, *d_starts, *d_tot;
  int32_t* d_len;
  uint8_t *d_fl, *d_by;
  const size_t un = size_t(n);
  if ((rc = T.put(&d_off, offsets, un)) || (rc = T.get(&d_doc, un)) || (rc = T.get(&d_pos, un)) || (rc = T.get(&d_len, un)) || (rc = T.get(&d_fl, un)) ||
      (rc = T.get(&d_starts, un + 1)) || (rc = T.get(&d_tot, 2)))
    return rc;
  hipStream_t st = nullptr;
  if ((rc = run_bounds(ex, n, d_off, nullptr, d_doc, d_pos, d_len, d_fl, st))) return rc;
  if (doc) HIP_TRY(hipMemcpyAsync(doc, d_doc, un * 8, hipMemcpyDeviceToHost, st));
  if (line_pos) HIP_TRY(hipMemcpyAsync(line_pos, d_pos, un * 8, hipMemcpyDeviceToHost, st));
  if (line_len) HIP_TRY(hipMemcpyAsync(line_len, d_len, un * 4, hipMemcpyDeviceToHost, st));
  if (flags) HIP_TRY(hipMemcpyAsync(flags, d_fl, un, hipMemcpyDeviceToHost, st));
  if (!bytes) {
    HIP_TRY(hipStreamSynchronize(st));
    return FEMTO_AMD_OK;
  }
  // the starts and the total, then the bytes into a buffer of exactly that size
  if ((rc = run_bytes(ex, n, nullptr, d_pos, d_len, d_starts, nullptr, 0, d_tot, st))) return rc;
  HIP_TRY(hipMemcpyAsync(byte_starts, d_starts, (un + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t nb = byte_starts[n];
  *total = nb;
  if (nb == 0) return FEMTO_AMD_OK;
  if ((rc = T.get(&d_by, size_t(nb))) || (rc = run_bytes(ex, n, nullptr, d_pos, d_len, d_starts, d_by, nb, d_tot, st)) ||
      (rc = list_to_host(nb, d_by, st, "copying the lines back", bytes)))
    *total = 0;
  return rc;
  API_END
}

int femto_amd_line_groups(femto_amd_extractor_t* ex, int64_t n, const int64_t* byte_starts, const uint8_t* bytes, const uint8_t* flags, int hash_bits,
                          int64_t* group_first, int64_t* ngroups) {
  API_BEGIN
  if (!ex || n < 0 || n >= kMaxCall || hash_bits < 0 || hash_bits > 64 || !ngroups || (n && (!byte_starts || !group_first)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= n < 2^31 lines, 0 <= hash_bits <= 64)");
  *ngroups = 0;
  int rc = check_extractor(ex, false);
  if (rc) return rc;
  if (n == 0) return FEMTO_AMD_OK;
  for (int64_t i = 0; i < n; i++)
    if (byte_starts[i] < 0 || byte_starts[i + 1] < byte_starts[i]) return set_err(FEMTO_AMD_ERR_PARAM, "byte_starts must ascend from a start >= 0");
  if (byte_starts[n] && !bytes) return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  Temp T;
  int64_t *d_starts, *d_gf, *d_ng;
  uint8_t *d_by, *d_fl = nullptr;
  const size_t un = size_t(n);
  if ((rc = T.put(&d_starts, byte_starts, un + 1)) || (rc = T.put(&d_by, bytes, size_t(byte_starts[n]))) || (flags && (rc = T.put(&d_fl, flags, un))) ||
      (rc = T.get(&d_gf, un)) || (rc = T.get(&d_ng, 1)))
    return rc;
  hipStream_t st = nullptr;
  if ((rc = run_groups(ex->ix, n, nullptr, d_starts, d_by, d_fl, hash_bits, d_gf, d_ng, st))) return rc;
  HIP_TRY(hipMemcpyAsync(group_first, d_gf, un * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ngroups, d_ng, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return FEMTO_AMD_OK;
  API_END
}
