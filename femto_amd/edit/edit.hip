// edit.hip -- search within edit distance 2: for every pattern of a batch, the DISTINCT strings that at most k substitutions,
// deletions and insertions make of it and that occur in the index, each with its row range, its length and the fewest
// operations that reach it.  include/femto_amd.h "search within edit distance" states the contract; DESIGN.md "Search within
// edit distance" the kernels, their registers and the figures.
//
// TAKEN FROM THE REFERENCE: the question of APPROX max:subst:delete:insert with costs 1:1:1 (QUERY_FORMAT.txt:129-160) and its
// bound of two edits (:138, compile_regexp.c:683-685).  NOT TAKEN: the automaton, its rule that the last character is never
// substituted (:143), and what its search does with a match that has reached a final state (it is not extended, and ranges that
// lie inside another are dropped: regexp_result_list_sort, server.c:1528-1573): here every string is listed.
//
// SITES.  A pattern of m symbols has m + 1 sites r = 0 .. m: site r is the gap in front of symbol r, site m the gap behind the
// last one.  Pattern q's sites are entries starts[q] + q + r of the site arrays (nsyms + npat in all).
// EXACT PASS.  One lane per pattern walks right to left and leaves rng[site r] = the range of the suffix p[r..] (site m: the
// whole index; empty from the first empty suffix on) and owner[site] = the pattern; a pattern that matches whole is the cost-0
// result.
// EDIT PASS.  One lane per (site, edit), t = site * (2 nsub + 1) + e: insert substitute e in gap r; substitute p[r - 1] by
// substitute e - nsub; delete p[r - 1].  The lanes of one site are neighbours and read one owner and one range.  A lane quits
// after that round of loads when the suffix p[r..] does not occur or its edit is not allowed there; otherwise it applies the edit
// and walks the remaining prefix exactly.  For k = 2 it first tries, at every point of that walk, each second edit followed by
// the exact remainder -- another insertion in the same gap and an insertion in front of the pattern included.  A lane thus owns
// the scripts whose RIGHTMOST edit is its own.  Two kinds of script that only repeat another lane's are not started: the
// insertion of the character that stands to the right of the gap (the insertion one gap further right gives the same string)
// and the deletion of a character equal to its right neighbour (so is the deletion of that neighbour).
// EMIT.  atomicAdd on the raw total; the record (first, last, pattern, length, cost) is written when its slot is below capacity.
// ORDER AND DE-DUPLICATION.  Several scripts reach one string.  The stage of ../common/result_order.hpp (two stable radix sorts
// of the records' indexes), here by first << 5 | (length - m + 2) << 2 | cost and then by pattern, leaves the records of one
// string -- (pattern, first, length) is a unique key -- side by side, the cheapest in front: the head of every run is kept (flags,
// the shared exclusive scan, a scatter), and result_start[q] is the scan at the first sorted record of a pattern >= q (binary
// search in the sorted pattern keys that stage hands back).
#include <algorithm>
#include <cstdlib>
#include <cstring>

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
#include "../common/sub_table.hpp"
#include "../common/result_order.hpp"

namespace femto_amd {
namespace {

constexpr int32_t kMaxPattern = 32768;               // MAX_PATTERN_LENGTH, as mismatch.hip
constexpr int64_t kMaxSyms = int64_t(1) << 31;       // symbols per call
constexpr int64_t kEditChunk = int64_t(1) << 31;     // lanes per launch of the edit pass: a launch carries fewer than 2^32 work-items
constexpr int64_t kMaxRecords = int64_t(1) << 31;    // raw records per call: the sorts carry 32-bit indexes
constexpr uint32_t kNoOwner = 0xffffffffu;           // owner[site] of a site no pattern of this call covers
const char* const kSubject = "search within edit distance is";

// the records as the lanes emit them (any order); meta = length | cost << 16 | (length - m + 2) << 18; total[0] = raw records
struct Records {
  int64_t *first, *last;
  uint32_t *pat, *meta;
  unsigned long long* total;
  int64_t npat, capacity;
};

__device__ __forceinline__ void emit(const Records& R, uint32_t q, int64_t first, int64_t last, int m, int length, int cost) {
  const int64_t slot = int64_t(atomicAdd(R.total, 1ull));
  if (slot >= R.capacity) return;
  R.first[slot] = first;
  R.last[slot] = last;
  R.pat[slot] = q;
  R.meta[slot] = uint32_t(length) | (uint32_t(cost) << 16) | (uint32_t(length - m + 2) << 18);
}

// a step from the whole index is the policies' step 0 (C alone, no rank)
template <class P>
__device__ __forceinline__ void step(const DevIndex& ix, uint32_t code, int64_t& first, int64_t& last) {
  P::search_step(ix, first == 0 && last == ix.total_length - 1 ? 0 : 1, code, first, last);
}

// pattern q as the caller stated it: false when its bounds leave the nsyms symbols or it is longer than a pattern may be
__device__ __forceinline__ bool pattern_of(const int64_t* __restrict__ starts, int64_t q, int64_t nsyms, int64_t* s, int* len) {
  const int64_t s0 = starts[q], len64 = starts[q + 1] - s0;
  if (s0 < 0 || len64 < 0 || s0 + len64 > nsyms || len64 > int64_t(kMaxPattern)) return false;
  *s = s0;
  *len = int(len64);
  return true;
}

// One lane per pattern.  kRanges: rng[site], owner[site] of its len + 1 sites
template <class P, bool kRanges>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P::kDirectWaves, P::kDirectWaves))) void exact_kernel(
    const DevIndex ix, const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms, const int64_t* __restrict__ starts,
    longlong2* __restrict__ rng, uint32_t* __restrict__ owner, const Records R) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (q >= npat) return;
  int64_t s;
  int len;
  if (!pattern_of(starts, q, nsyms, &s, &len)) return;      // nothing of it is read, and it has no sites
  const int64_t site0 = s + q;
  int64_t first = 0, last = ix.total_length - 1;      // the empty suffix's range
  if (kRanges) {
    for (int r = 0; r <= len; r++) owner[site0 + r] = uint32_t(q);
    rng[site0 + len] = make_longlong2(first, last);
  }
  int pos = len - 1;
  for (; pos >= 0; pos--) {
    const uint32_t code = code_or_none<P>(ix, syms[s + pos]);
    if (code == 0xffffu) break;      // the character does not occur in the text
    int64_t nf = first, nl = last;
    P::search_step(ix, len - 1 - pos, code, nf, nl);
    if (nf > nl) break;
    first = nf;
    last = nl;
    if (kRanges) rng[site0 + pos] = make_longlong2(first, last);
  }
  if (kRanges)
    for (int p = pos; p >= 0; p--) rng[site0 + p] = make_longlong2(1, 0);
  if (pos < 0) emit(R, uint32_t(q), first, last, len, len, 0);
}

// k = 2 keeps a second range, its point of the walk and its edit alive across the inner steps.  The rank units have the room at
// eight wavefronts (53 and 56 VGPRs) and the character rank lines at seven (69).  The other layouts' steps fill the budget of
// kDirectWaves already and need 83 VGPRs here: at seven and at six wavefronts they spill into the chain of dependent steps that is
// this kernel's time, so they run k = 2 with five (DESIGN.md "Search within edit distance" has the compiler's table)
template <class P, int K> struct EditWaves { static constexpr int value = K == 2 ? 5 : P::kDirectWaves; };
template <int K> struct EditWaves<RuPolicy, K> { static constexpr int value = RuPolicy::kDirectWaves; };
template <int K> struct EditWaves<RumPolicy, K> { static constexpr int value = RumPolicy::kDirectWaves; };
template <int K> struct EditWaves<IndPolicy, K> { static constexpr int value = IndPolicy::kDirectWaves - (K == 2 ? 1 : 0); };

// edit e of a point with `rem` symbols of the pattern to its left: false when it is not allowed there.  `fresh`: the symbol to
// the right of the point is the pattern's own pat[rem], matched exactly.  *code = 0xffff: no step (a deletion); *left = the
// symbols to the left of the edit; *grow = what it adds to the length
__device__ __forceinline__ bool edit_of(const SubTable* __restrict__ tab, int nsub, int e, const uint16_t* __restrict__ pat, int rem, bool fresh,
                                        uint32_t* code, int* left, int* grow) {
  const uint32_t own = rem > 0 ? uint32_t(pat[rem - 1]) : 0u;
  const uint32_t right = fresh ? uint32_t(pat[rem]) : 0u;
  if (e < nsub) {      // insert in the gap: not behind a code below 5, not the character to the right
    const uint32_t pr = tab->pair[e];
    if ((rem > 0 && own < kByte0) || (pr & 0xffffu) == right) return false;
    *code = pr >> 16;
    *left = rem;
    *grow = 1;
    return (pr >> 16) != 0xffffu;
  }
  if (rem == 0 || own < kByte0 || own >= kAlpha) return false;      // no byte character to substitute or delete
  if (e < 2 * nsub) {
    const uint32_t pr = tab->pair[e - nsub];
    if ((pr & 0xffffu) == own) return false;
    *code = pr >> 16;
    *left = rem - 1;
    *grow = 0;
    return (pr >> 16) != 0xffffu;
  }
  if (own == right) return false;      // inside a run: the deletion of the right neighbour is the same string
  *code = 0xffffu;
  *left = rem - 1;
  *grow = -1;
  return true;
}

// One lane per (site, edit), t0 = the first lane of this launch; K = 1 or 2
template <class P, int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(EditWaves<P, K>::value, EditWaves<P, K>::value))) void edit_kernel(
    const DevIndex ix, const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms, const int64_t* __restrict__ starts,
    const SubTable* __restrict__ tab, const longlong2* __restrict__ rng, const uint32_t* __restrict__ owner, const int64_t t0, const Records R) {
  const int64_t t = t0 + int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int nsub = tab->n;
  if (nsub < 0 || nsub > 256) return;
  const int nedits = 2 * nsub + 1;
  const int64_t site = t / nedits;
  if (site >= nsyms + npat) return;
  const uint32_t q = owner[site];
  const longlong2 r0 = rng[site];
  if (int64_t(q) >= npat || r0.x > r0.y) return;      // no pattern's site, or the suffix to the right does not occur
  int64_t s;
  int len;
  if (!pattern_of(starts, q, nsyms, &s, &len)) return;
  const int64_t r64 = site - s - int64_t(q);
  if (r64 < 0 || r64 > int64_t(len)) return;      // (a stale owner: the site is not this pattern's)
  const int r = int(r64);
  const uint16_t* __restrict__ const pat = syms + s;
  uint32_t code;
  int rem, grow;
  if (!edit_of(tab, nsub, int(t - site * nedits), pat, r, r < len, &code, &rem, &grow)) return;
  int64_t first = r0.x, last = r0.y;
  if (code != 0xffffu) {
    step<P>(ix, code, first, last);
    if (first > last) return;
  }
  const int rem0 = rem, length = len + grow;
  for (;; rem--) {
    const uint32_t c1 = rem > 0 ? code_or_none<P>(ix, pat[rem - 1]) : 0xffffu;
    // k = 2.  Where the exact step keeps every row of the range, every row is preceded by the pattern's own character and no
    // other character steps from it -- so it is on one row, where a long pattern spends its walk: the second edits worth a
    // search are then the insertion of that character and the deletion, not all 2 nsub + 1 (a lane is one chain of dependent
    // steps: 32768 points times 513 edits would be its time).  Only the new first row is kept across the second edits
    int64_t nf = first;
    bool only = false;
    if (K == 2 && c1 != 0xffffu) {
      int64_t nl = last;
      step<P>(ix, c1, nf, nl);
      only = nl - nf == last - first;
    }
    if (K == 2) {
      for (int e2 = only ? nedits - 2 : 0; e2 < nedits; e2++) {      // a second edit here, then the exact remainder
        uint32_t code2;
        int rem2, grow2;
        if (only && e2 == nedits - 2) {
          const uint32_t own = pat[rem - 1];
          if (own < kByte0 || own >= kAlpha || (rem < rem0 && own == uint32_t(pat[rem]))) continue;      // as edit_of's insertion
          code2 = 0xffffu;      // (its step is the exact step above)
          rem2 = rem;
          grow2 = 1;
        } else {      // the deletion: every row is preceded by pat[rem - 1], so a remainder that goes on with another character is empty
          if (only && rem >= 2 && pat[rem - 2] != pat[rem - 1]) continue;
          if (!edit_of(tab, nsub, e2, pat, rem, rem < rem0, &code2, &rem2, &grow2)) continue;
        }
        int64_t f2 = first, l2 = last;
        if (only && e2 == nedits - 2) {
          f2 = nf;
          l2 = nf + (last - first);
        }
        if (code2 != 0xffffu) step<P>(ix, code2, f2, l2);
        for (; f2 <= l2 && rem2 > 0; rem2--) {
          const uint32_t c2 = code_or_none<P>(ix, pat[rem2 - 1]);
          if (c2 == 0xffffu) {
            l2 = f2 - 1;
            break;
          }
          step<P>(ix, c2, f2, l2);
        }
        if (f2 <= l2) emit(R, q, f2, l2, len, length + grow2, 2);
      }
    }
    if (rem == 0) break;
    if (c1 == 0xffffu) return;
    if (only) {
      last = nf + (last - first);
      first = nf;
    } else {
      step<P>(ix, c1, first, last);
      if (first > last) return;
    }
  }
  emit(R, q, first, last, len, length, 1);
}

// ---- order and de-duplication ----------------------------------------------------------------------------------------------------

// {distinct results, raw > capacity, raw}; scan = the heads' exclusive scan over the capacity slots, NULL for the counting form
__global__ __launch_bounds__(256) void total_kernel(const Records R, const int64_t* __restrict__ scan, int64_t* __restrict__ d_total) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t raw = int64_t(R.total[0]);
  d_total[0] = scan ? scan[R.capacity] : 0;
  d_total[1] = raw > R.capacity ? 1 : 0;
  d_total[2] = raw;
}

// the first sort's key of a record: first << 5 | (length - m + 2) << 2 | cost
struct StringKey {
  const int64_t* first;
  const uint32_t* meta;
  __device__ __forceinline__ uint64_t operator()(int64_t slot) const {
    return (uint64_t(first[slot]) << 5) | uint64_t(((meta[slot] >> 18) << 2) | ((meta[slot] >> 16) & 3u));
  }
};

// flags[s] = 1 at the first record of every (pattern, first, length) in sorted order: the cheapest way to that string
__global__ __launch_bounds__(256) void head_kernel(const Records R, const uint32_t* __restrict__ idx, int64_t* __restrict__ flags) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= R.capacity) return;
  bool head = s < live_records(R.total, R.capacity);
  if (head && s > 0) {
    const uint32_t a = idx[s], b = idx[s - 1];
    head = R.pat[a] != R.pat[b] || R.first[a] != R.first[b] || (R.meta[a] & 0xffffu) != (R.meta[b] & 0xffffu);
  }
  flags[s] = head ? 1 : 0;
}

struct Out {
  int64_t *first, *last;
  int32_t *cost, *length;
};

__global__ __launch_bounds__(256) void gather_kernel(const Records R, const uint32_t* __restrict__ idx, const int64_t* __restrict__ scan, const Out out) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= live_records(R.total, R.capacity)) return;
  const int64_t at = scan[s];
  if (scan[s + 1] == at) return;      // no head
  const uint32_t r = idx[s], meta = R.meta[r];
  out.first[at] = R.first[r];
  out.last[at] = R.last[r];
  out.cost[at] = int32_t((meta >> 16) & 3u);
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

// ---- host side ----------------------------------------------------------------------------------------------------------------

template <class P>
int search_all(femto_amd_index* ix, int64_t npat, int64_t nsyms, int nsub, const uint16_t* d_syms, const int64_t* d_starts, int k, SubTable* tab,
               longlong2* rng, uint32_t* owner, const Records& R, hipStream_t st) {
  int rc;
  if (k == 0) return launch(exact_kernel<P, false>, blocks_of(npat), st, ix->dev, npat, nsyms, d_syms, d_starts, rng, owner, R);
  if ((rc = launch(exact_kernel<P, true>, blocks_of(npat), st, ix->dev, npat, nsyms, d_syms, d_starts, rng, owner, R)) ||
      (rc = launch(sub_table_kernel<P>, dim3(1), st, ix->dev, tab)))
    return rc;
  const int64_t lanes = (nsyms + npat) * (2 * int64_t(nsub) + 1), chunk = lane_chunk("FEMTO_AMD_EDIT_CHUNK", kEditChunk);      // (below 2^32 * 513)
  for (int64_t t0 = 0; t0 < lanes; t0 += chunk) {      // whole workgroups per launch: only the last one has lanes behind the last site
    const dim3 grid = blocks_of(std::min(chunk, lanes - t0));
    if ((rc = k == 1 ? launch(edit_kernel<P, 1>, grid, st, ix->dev, npat, nsyms, d_syms, d_starts, tab, rng, owner, t0, R)
                     : launch(edit_kernel<P, 2>, grid, st, ix->dev, npat, nsyms, d_syms, d_starts, tab, rng, owner, t0, R)))
      return rc;
  }
  return 0;
}

int run_edit(femto_amd_index* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k, int64_t capacity,
             int64_t* d_result_start, const Out& out, int64_t* d_total, hipStream_t st) {
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  int rc;
  const size_t cap = size_t(capacity), nsites = size_t(nsyms) + size_t(npat);
  if ((rc = S.tail.reserve(sizeof(SubTable))) || (rc = S.pairs.reserve(nsites * 20 + 16)) || (rc = S.noccs64.reserve(16)) ||
      (rc = S.first.reserve(cap * 8 + 8)) || (rc = S.last.reserve(cap * 8 + 8)) || (rc = S.rows.reserve(cap * 4 + 8)) ||
      (rc = S.ch.reserve(cap * 4 + 8)))
    return rc;
  const Records R{S.first.as<int64_t>(), S.last.as<int64_t>(), S.rows.as<uint32_t>(), S.ch.as<uint32_t>(), S.noccs64.as<unsigned long long>(), npat, capacity};
  HIP_TRY(hipMemsetAsync(R.total, 0, 8, st));
  longlong2* const rng = S.pairs.as<longlong2>();      // the sites' ranges, then their owners
  uint32_t* const owner = reinterpret_cast<uint32_t*>(rng + nsites);
  if (k > 0) HIP_TRY(hipMemsetAsync(owner, 0xff, nsites * 4, st));      // kNoOwner: the sites of a pattern the exact pass refuses
  int nsub = 0;
  for (uint32_t ch = kByte0; ch < kAlpha; ch++) nsub += ix->host.C[ch + 1] > ix->host.C[ch];
  auto go = [&](auto tag) {
    using P = typename decltype(tag)::type;
    return search_all<P>(ix, npat, nsyms, nsub, d_syms, d_starts, k, S.tail.as<SubTable>(), rng, owner, R, st);
  };
  if ((rc = with_lane_policy(ix, "search within edit distance on this handle needs", go))) return rc;
  if (capacity == 0) return launch(total_kernel, dim3(1), st, R, static_cast<const int64_t*>(nullptr), d_total);
  // by (first, length, cost), then (stable) by pattern; total_length is no row: the slots behind the live ones sort behind every
  // row.  keys and keys2 hold the heads' flags and their scan afterwards, and the scan writes capacity + 1 words: keys2 is
  // reserved for them here, larger than the sort asks for (and keys in front of it, which keeps the order of the allocations)
  const int64_t N = ix->host.total_length;
  if ((rc = S.keys.reserve(cap * 8)) || (rc = S.keys2.reserve(cap * 8 + 8))) return rc;
  Ordered o;
  if ((rc = order_records(OrderBuffers{S.keys, S.keys2, S.idx, S.idx2, S.off, S.offsets, S.sorttmp}, R.total, capacity, R.pat, npat,
                          StringKey{R.first, R.meta}, unsigned(bits_of(N)) + 5u, uint64_t(N) << 5, st, &o)))
    return rc;
  // the sort keys are done with: their buffers hold the heads' flags and the scan of them
  int64_t *flags = S.keys.as<int64_t>(), *scan = S.keys2.as<int64_t>();
  if ((rc = launch(head_kernel, blocks_of(capacity), st, R, o.idx, flags)) || (rc = device_scan(S.scan, capacity, flags, scan, 0, st)) ||
      (rc = launch(gather_kernel, blocks_of(capacity), st, R, o.idx, scan, out)) ||
      (rc = launch(result_start_kernel, blocks_for(npat), st, R, o.pattern_keys, scan, d_result_start)))
    return rc;
  return launch(total_kernel, dim3(1), st, R, scan, d_total);
}

int check_args(femto_amd_index* ix, int64_t npat, int64_t nsyms, int k) {
  if (!ix || npat < 0 || npat >= kMaxRecords || nsyms < 0 || nsyms >= kMaxSyms || (npat == 0 && nsyms != 0))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= npat < 2^31 patterns, 0 <= nsyms < 2^31 symbols, no symbols without patterns)");
  if (k < 0 || k > 2) return set_err(FEMTO_AMD_ERR_PARAM, "k must be 0, 1 or 2 edits");
  return FEMTO_AMD_OK;
}

// the answer of the device form to a call without patterns: result_start[0] = 0 and the three-word total {0, 0, 0}
int no_patterns_async(int64_t* d_result_start, int64_t* d_total, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(d_result_start, 0, 8, st));
  HIP_TRY(hipMemsetAsync(d_total, 0, 24, st));
  return FEMTO_AMD_OK;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_edit_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                          int64_t capacity, int64_t* d_result_start, int64_t* d_first, int64_t* d_last, int32_t* d_cost, int32_t* d_length,
                          int64_t* d_total, void* stream) {
  API_BEGIN
  int rc = check_args(ix, npat, nsyms, k);
  if (rc) return rc;
  if (capacity < 0 || capacity >= kMaxRecords || !d_total || (capacity && !d_result_start) || (npat && !d_starts) || (nsyms && !d_syms) ||
      (capacity && (!d_first || !d_last || !d_cost || !d_length)))
    return set_err(FEMTO_AMD_ERR_PARAM, "null argument or bad capacity (0 <= capacity < 2^31 raw records; capacity 0 alone takes no result arrays)");
  if (reinterpret_cast<uintptr_t>(d_syms) & 1u) return set_err(FEMTO_AMD_ERR_PARAM, "d_syms must be 2-byte aligned (uint16 symbols)");
  if ((rc = check_device_handle(ix, kSubject))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npat == 0) {
    if (!d_result_start) return set_err(FEMTO_AMD_ERR_PARAM, "null result_start");
    return no_patterns_async(d_result_start, d_total, st);
  }
  return run_edit(ix, npat, nsyms, d_syms, d_starts, k, capacity, d_result_start, Out{d_first, d_last, d_cost, d_length}, d_total, st);
  API_END
}

void femto_amd_edit_free(femto_amd_edit_result_t* out) {
  if (!out) return;
  free(out->result_start);
  free(out->first);
  free(out->last);
  free(out->cost);
  free(out->length);
  memset(out, 0, sizeof *out);
}

int femto_amd_edit(femto_amd_index_t* ix0, int64_t npat, const int32_t* plen, const uint16_t* syms, int k, femto_amd_edit_result_t* out) {
  API_BEGIN
  if (!out) return set_err(FEMTO_AMD_ERR_PARAM, "null result");
  memset(out, 0, sizeof *out);
  if (!ix0 || npat < 0 || (npat && !plen)) return set_err(FEMTO_AMD_ERR_PARAM, "null argument or negative npat");
  femto_amd_index* ix = replica0(ix0);
  std::vector<int64_t> starts;
  int rc = pattern_starts(npat, plen, 0, kMaxPattern, "a pattern holds 0 .. 32768 symbols", &starts);
  if (rc) return rc;
  const int64_t nsyms = starts[size_t(npat)];
  if ((rc = check_args(ix, npat, nsyms, k))) return rc;
  if (nsyms && !syms) return set_err(FEMTO_AMD_ERR_PARAM, "null symbols");
  for (int64_t j = 0; j < nsyms; j++)
    if (syms[j] >= FEMTO_AMD_ALPHA_SIZE) return set_err(FEMTO_AMD_ERR_PARAM, "character code >= ALPHA_SIZE in a pattern");
  if ((rc = check_plain_handle(ix, kSubject))) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  out->result_start = static_cast<int64_t*>(calloc(size_t(npat) + 1, 8));
  if (!out->result_start) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  out->npat = npat;
  if (npat == 0) return FEMTO_AMD_OK;
  auto fail = [&](int code) {
    femto_amd_edit_free(out);
    return code;
  };
  hipStream_t st = nullptr;
  Temp T;
  uint16_t* d_syms;
  int64_t *d_starts, *d_rs, *d_tot, *d_first, *d_last;
  int32_t *d_cost, *d_length;
  if ((rc = T.put(&d_syms, syms, size_t(nsyms))) || (rc = T.put(&d_starts, starts)) || (rc = T.get(&d_rs, size_t(npat) + 1)) || (rc = T.get(&d_tot, 3)))
    return fail(rc);
  const Out none{nullptr, nullptr, nullptr, nullptr};
  int64_t tot[3] = {0, 0, 0};
  // the counting pass sizes the filling pass by the raw records
  if ((rc = run_edit(ix, npat, nsyms, d_syms, d_starts, k, 0, d_rs, none, d_tot, st))) return fail(rc);
  if ((rc = words_to_host(3, d_tot, st, "counting the records failed on the device", tot))) return fail(rc);
  const int64_t raw = tot[2];
  if (raw >= kMaxRecords) return fail(set_err(FEMTO_AMD_ERR_FULL, "2^31 raw records or more: search the patterns in smaller batches"));
  if (raw == 0) return FEMTO_AMD_OK;      // (result_start is zeros)
  const size_t ur = size_t(raw);
  if ((rc = T.get(&d_first, ur)) || (rc = T.get(&d_last, ur)) || (rc = T.get(&d_cost, ur)) || (rc = T.get(&d_length, ur)) ||
      (rc = run_edit(ix, npat, nsyms, d_syms, d_starts, k, raw, d_rs, Out{d_first, d_last, d_cost, d_length}, d_tot, st)))
    return fail(rc);
  if ((rc = words_to_host(3, d_tot, st, "de-duplicating the records failed on the device", tot))) return fail(rc);
  const int64_t total = tot[0];
  if (tot[1] || tot[2] != raw || total <= 0 || total > raw) return fail(set_err(FEMTO_AMD_ERR_INVALID, "the filling pass disagrees with the counting pass"));
  if ((rc = list_to_host(total, d_first, st, "copying the results back", &out->first, false)) ||
      (rc = list_to_host(total, d_last, st, "copying the results back", &out->last, false)) ||
      (rc = list_to_host(total, d_cost, st, "copying the results back", &out->cost, false)) ||
      (rc = list_to_host(total, d_length, st, "copying the results back", &out->length, false)))
    return fail(rc);
  if ((rc = result_start_to_host(npat, d_rs, st, out->result_start))) return fail(rc);
  out->total = total;
  return FEMTO_AMD_OK;
  API_END
}
