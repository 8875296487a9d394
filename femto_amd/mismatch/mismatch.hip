// mismatch.hip -- search with up to two substitutions: for every pattern of a batch, the strings at Hamming distance <= k from it
// that occur in the index, each with its row range.  include/femto_amd.h "search with substitutions" states the contract;
// DESIGN.md "Search with substitutions" the kernels, their registers and the figures.
//
// TAKEN FROM THE REFERENCE: the question of APPROX max:subst:delete:insert restricted to substitutions (QUERY_FORMAT.txt:129-160),
// its bound of two edits (:138, compile_regexp.c:683-685) and the order of its result list (regexp_result_list_sort,
// server.c:1528: by first row).  NOT TAKEN: the automaton.  A plain string needs none -- the search is the backward search of
// count with, at one or two positions, the other characters of the text tried -- and the reference's rule that the LAST character
// is never substituted (:143) is a property of how it builds that automaton, not of the question: here every byte position is
// substituted alike.  Insertions and deletions are ../edit/edit.hip.
//
// SUBSTITUTE TABLE.  One 256-lane launch: the byte characters of the text (C[ch + 1] > C[ch]) with their codes in the handle's
// rank layout (P::code_of), compacted in character order.
// EXACT PASS.  One lane per pattern walks right to left (P::search_step called as match_stats_kernel of ../similar/similar.hip
// calls it) and leaves the range of EVERY suffix of the pattern, empty from the first empty one on, and beside it the pattern that
// owns the position; a pattern that matches whole is the cost-0 result.
// SUBSTITUTION PASS.  One lane per (symbol g of the flat batch, substitute i), t = g * nsub + i: the lanes of one position are
// neighbours and read one owner and one suffix range.  A lane quits when the suffix to the right of its position does not
// occur, when its substitute is the pattern's own character or when the position holds no byte character -- after one round of
// loads, with no search for its pattern; otherwise it steps with
// its substitute (step 0 from the whole index at the rightmost position) and carries on exactly to the left.  For k = 2 it first
// tries, at every position it passes, each other substitute followed by the exact remainder.  A lane thus owns the variants whose
// RIGHTMOST substitution is its own: every variant has one owner and is emitted once.
// EMIT.  atomicAdd on the pattern's counter and on the total; the record is written when its slot is below the capacity.
// ORDER.  The stage of ../common/result_order.hpp (two stable radix sorts of the records' indexes, by first over the bits of
// total_length, then by pattern over the bits of npat) and a gather; result_start is the exclusive scan of the counters.  The emit
// order is arbitrary and the final order is not: (pattern, first) is a unique key, the ranges of distinct strings of one length being
// disjoint.
// A launch carries fewer than 2^32 work-items and nsyms * nsub can be 2^39: the pass goes out in launches of kSubstChunk lanes,
// each with the number of its first lane.
// A lane is a chain of dependent scattered loads and lanes retire at different depths: occupancy hides the latency, so the
// search kernels are held to the policy's kDirectWaves wavefronts per SIMD.
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

constexpr int32_t kMaxPattern = 32768;               // MAX_PATTERN_LENGTH, as similar.hip: a position fits 15 bits
constexpr int64_t kMaxSyms = int64_t(1) << 31;       // symbols per call: the owner of a position and its flag share 32 bits
constexpr int64_t kSubstChunk = int64_t(1) << 31;    // lanes per launch of the substitution pass: a launch carries fewer than 2^32 work-items
constexpr uint32_t kRightmost = 0x80000000u;         // owner[g]: the pattern of symbol g | kRightmost at the last symbol of a pattern
constexpr int64_t kMaxResults = int64_t(1) << 31;    // results per call: the sorts carry 32-bit indexes
constexpr uint32_t kUnused = 0xffffu;                // a substitution slot nobody used: position 0xffff, symbol 0
const char* const kSubject = "search with substitutions is";

// the records as the lanes emit them (any order), and the counters: counts[q] = results of pattern q, counts[npat] = all
struct Records {
  int64_t *first, *last;
  uint32_t *pat, *m0, *m1;      // m = position | substitute << 16, ascending positions, kUnused behind the used ones
  unsigned long long* counts;
  int64_t npat, capacity;
};

__device__ __forceinline__ void emit(const Records& R, int64_t q, int64_t first, int64_t last, uint32_t m0, uint32_t m1) {
  atomicAdd(R.counts + q, 1ull);
  const int64_t slot = int64_t(atomicAdd(R.counts + R.npat, 1ull));
  if (slot >= R.capacity) return;
  R.first[slot] = first;
  R.last[slot] = last;
  R.pat[slot] = uint32_t(q);
  R.m0[slot] = m0;
  R.m1[slot] = m1;
}

// One lane per pattern.  kRanges: rng[g] = the range of the suffix that starts at symbol g of the flat batch, owner[g] = its pattern
template <class P, bool kRanges>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P::kDirectWaves, P::kDirectWaves))) void exact_kernel(
    const DevIndex ix, const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms, const int64_t* __restrict__ starts,
    longlong2* __restrict__ rng, uint32_t* __restrict__ owner, const Records R) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (q >= npat) return;
  const int64_t s = starts[q], len64 = starts[q + 1] - s;
  if (s < 0 || len64 < 0 || s + len64 > nsyms) return;        // starts that leave the nsyms symbols the caller stated: nothing is read
  if (len64 > int64_t(kMaxPattern)) return;                   // (the host form refuses it; here it has no results)
  const int len = int(len64);
  if (kRanges)
    for (int p = 0; p < len; p++) owner[s + p] = uint32_t(q) | (p == len - 1 ? kRightmost : 0u);
  int64_t first = 0, last = ix.total_length - 1;      // the empty pattern's range
  int pos = len - 1;
  for (; pos >= 0; pos--) {
    const uint32_t code = code_or_none<P>(ix, syms[s + pos]);
    if (code == 0xffffu) break;      // the character does not occur in the text
    int64_t nf = first, nl = last;
    P::search_step(ix, len - 1 - pos, code, nf, nl);
    if (nf > nl) break;
    first = nf;
    last = nl;
    if (kRanges) rng[s + pos] = make_longlong2(first, last);
  }
  if (kRanges)
    for (int p = pos; p >= 0; p--) rng[s + p] = make_longlong2(1, 0);
  if (pos < 0) emit(R, q, first, last, kUnused, kUnused);
}

// k = 2 keeps a second range and its position alive across the inner steps.  The rank units have the room (54 VGPRs at eight
// wavefronts); the other layouts' steps fill their budget already (text_kernels.hip.hpp on kDirectWaves) and would spill up to 52
// bytes per lane into the chain of dependent steps that is this kernel's time: they run k = 2 with one wavefront less.
template <class P, int K> struct SubstWaves { static constexpr int value = P::kDirectWaves - (K == 2 ? 1 : 0); };
template <int K> struct SubstWaves<RuPolicy, K> { static constexpr int value = RuPolicy::kDirectWaves; };
template <int K> struct SubstWaves<RumPolicy, K> { static constexpr int value = RumPolicy::kDirectWaves; };

// One lane per (symbol, substitute), t0 = the first lane of this launch; K = 1 or 2
template <class P, int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SubstWaves<P, K>::value, SubstWaves<P, K>::value))) void subst_kernel(
    const DevIndex ix, const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms, const int64_t* __restrict__ starts,
    const SubTable* __restrict__ tab, const longlong2* __restrict__ rng, const uint32_t* __restrict__ owner, const int64_t t0, const Records R) {
  const int64_t t = t0 + int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int nsub = tab->n;
  if (nsub <= 0) return;
  const int64_t g = t / nsub;
  if (g >= nsyms) return;
  const uint32_t own = syms[g];
  if (own < kByte0 || own >= kAlpha) return;      // not a byte character: never substituted
  const uint32_t pr = tab->pair[int(t - g * nsub)];
  const uint32_t a = pr & 0xffffu, code = pr >> 16;
  if (a == own || code == 0xffffu) return;
  const uint32_t o = owner[g];
  const longlong2 r = rng[g + 1];      // (rng holds nsyms + 1 pairs: the one behind the last symbol is read and not used)
  if (!(o & kRightmost) && r.x > r.y) return;      // the suffix to the right does not occur
  const uint32_t q = o & ~kRightmost;      // (32 bits and one pointer: what stays alive across the steps is registers)
  if (int64_t(q) >= npat) return;      // a position of a pattern the exact pass refused: the scratch holds whatever it held
  const int64_t s = starts[q], len64 = starts[q + 1] - s;
  if (s < 0 || len64 < 0 || s + len64 > nsyms || len64 > int64_t(kMaxPattern) || g < s || g >= s + len64) return;      // as exact_kernel
  const int p = int(g - s), len = int(len64);
  const uint16_t* __restrict__ const pat = syms + s;
  int64_t first = 0, last = ix.total_length - 1;
  if (p < len - 1) {
    first = r.x;
    last = r.y;
    if (first > last) return;
  }
  P::search_step(ix, p == len - 1 ? 0 : 1, code, first, last);
  if (first > last) return;
  const uint32_t mine = uint32_t(p) | (a << 16);
  int pos = p - 1;
  for (; pos >= 0; pos--) {
    const uint32_t ch = pat[pos];
    if (K == 2 && ch >= kByte0 && ch < kAlpha) {
      for (int j = 0; j < nsub; j++) {      // a second substitution here, then the exact remainder
        const uint32_t pr2 = tab->pair[j];
        if ((pr2 & 0xffffu) == ch || (pr2 >> 16) == 0xffffu) continue;
        int64_t f2 = first, l2 = last;
        P::search_step(ix, 1, pr2 >> 16, f2, l2);
        for (int p2 = pos - 1; f2 <= l2 && p2 >= 0; p2--) {
          const uint32_t c2 = code_or_none<P>(ix, pat[p2]);
          if (c2 == 0xffffu) {
            l2 = f2 - 1;
            break;
          }
          P::search_step(ix, 1, c2, f2, l2);
        }
        if (f2 <= l2) emit(R, q, f2, l2, uint32_t(pos) | (pr2 << 16), mine);
      }
    }
    const uint32_t c1 = code_or_none<P>(ix, ch);
    if (c1 == 0xffffu) break;
    P::search_step(ix, 1, c1, first, last);
    if (first > last) break;
  }
  if (pos < 0) emit(R, q, first, last, mine, kUnused);
}

// ---- order --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void total_kernel(const Records R, int64_t* __restrict__ d_total) {
  if (blockIdx.x == 0 && threadIdx.x == 0) write_total(d_total, int64_t(R.counts[R.npat]), R.capacity);
}

struct Out {
  int64_t *first, *last;
  int32_t *cost, *sub_pos;
  uint16_t* sub_sym;
};

__global__ __launch_bounds__(256) void gather_kernel(const Records R, const uint32_t* __restrict__ idx, const Out out) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= live_records(R.counts + R.npat, R.capacity)) return;
  const uint32_t r = idx[s];
  const uint32_t m0 = R.m0[r], m1 = R.m1[r];
  const bool u0 = (m0 & 0xffffu) != kUnused, u1 = (m1 & 0xffffu) != kUnused;
  out.first[s] = R.first[r];
  out.last[s] = R.last[r];
  out.cost[s] = int32_t(u0) + int32_t(u1);
  out.sub_pos[2 * s] = u0 ? int32_t(m0 & 0xffffu) : -1;
  out.sub_pos[2 * s + 1] = u1 ? int32_t(m1 & 0xffffu) : -1;
  out.sub_sym[2 * s] = uint16_t(m0 >> 16);
  out.sub_sym[2 * s + 1] = uint16_t(m1 >> 16);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

template <class P>
int search_all(femto_amd_index* ix, int64_t npat, int64_t nsyms, int nsub, const uint16_t* d_syms, const int64_t* d_starts, int k, SubTable* tab,
               longlong2* rng, uint32_t* owner, const Records& R, hipStream_t st) {
  int rc;
  if (k == 0) return launch(exact_kernel<P, false>, blocks_of(npat), st, ix->dev, npat, nsyms, d_syms, d_starts, rng, owner, R);
  if ((rc = launch(exact_kernel<P, true>, blocks_of(npat), st, ix->dev, npat, nsyms, d_syms, d_starts, rng, owner, R))) return rc;
  if (nsyms == 0 || nsub == 0) return 0;
  if ((rc = launch(sub_table_kernel<P>, dim3(1), st, ix->dev, tab))) return rc;
  const int64_t lanes = nsyms * nsub, chunk = lane_chunk("FEMTO_AMD_MISMATCH_CHUNK", kSubstChunk);      // (below 2^31 * 256)
  for (int64_t t0 = 0; t0 < lanes; t0 += chunk) {      // whole workgroups per launch: only the last one has lanes behind the last symbol
    const dim3 grid = blocks_of(std::min(chunk, lanes - t0));
    if ((rc = k == 1 ? launch(subst_kernel<P, 1>, grid, st, ix->dev, npat, nsyms, d_syms, d_starts, tab, rng, owner, t0, R)
                     : launch(subst_kernel<P, 2>, grid, st, ix->dev, npat, nsyms, d_syms, d_starts, tab, rng, owner, t0, R)))
      return rc;
  }
  return 0;
}

int run_mismatch(femto_amd_index* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k, int64_t capacity,
                 int64_t* d_result_start, const Out& out, int64_t* d_total, hipStream_t st) {
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  int rc;
  const size_t cap = size_t(capacity), un = size_t(npat);
  if ((rc = S.tail.reserve(sizeof(SubTable))) || (rc = S.pairs.reserve((size_t(nsyms) + 1) * 20)) || (rc = S.noccs64.reserve((un + 1) * 8)) ||
      (rc = S.first.reserve(cap * 8 + 8)) || (rc = S.last.reserve(cap * 8 + 8)) || (rc = S.rows.reserve(cap * 4 + 8)) ||
      (rc = S.ch.reserve(cap * 4 + 8)) || (rc = S.occ.reserve(cap * 4 + 8)))
    return rc;
  const Records R{S.first.as<int64_t>(), S.last.as<int64_t>(), S.rows.as<uint32_t>(), S.ch.as<uint32_t>(), S.occ.as<uint32_t>(),
                  S.noccs64.as<unsigned long long>(), npat, capacity};
  HIP_TRY(hipMemsetAsync(R.counts, 0, (un + 1) * 8, st));
  longlong2* const rng = S.pairs.as<longlong2>();      // nsyms + 1 ranges, then the nsyms owners
  uint32_t* const owner = reinterpret_cast<uint32_t*>(rng + nsyms + 1);
  int nsub = 0;
  for (uint32_t ch = kByte0; ch < kAlpha; ch++) nsub += ix->host.C[ch + 1] > ix->host.C[ch];
  auto go = [&](auto tag) {
    using P = typename decltype(tag)::type;
    return search_all<P>(ix, npat, nsyms, nsub, d_syms, d_starts, k, S.tail.as<SubTable>(), rng, owner, R, st);
  };
  if ((rc = with_lane_policy(ix, "search with substitutions on this handle needs", go))) return rc;
  if ((rc = device_scan(S.scan, npat, reinterpret_cast<const int64_t*>(R.counts), d_result_start, 0, st)) ||
      (rc = launch(total_kernel, dim3(1), st, R, d_total)))
    return rc;
  if (capacity == 0) return 0;
  // by first, then (stable) by pattern; total_length is no row: the slots behind the live ones sort behind every row
  const int64_t N = ix->host.total_length;
  Ordered o;
  if ((rc = order_records(OrderBuffers{S.keys, S.keys2, S.idx, S.idx2, S.off, S.offsets, S.sorttmp}, R.counts + npat, capacity, R.pat, npat,
                          ColumnKey{R.first}, unsigned(bits_of(N)), uint64_t(N), st, &o)))
    return rc;
  return launch(gather_kernel, blocks_of(capacity), st, R, o.idx, out);
}

int check_args(femto_amd_index* ix, int64_t npat, int64_t nsyms, int k) {
  if (!ix || npat < 0 || npat >= kMaxResults || nsyms < 0 || nsyms >= kMaxSyms || (npat == 0 && nsyms != 0))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= npat < 2^31 patterns, 0 <= nsyms < 2^31 symbols, no symbols without patterns)");
  if (k < 0 || k > 2) return set_err(FEMTO_AMD_ERR_PARAM, "k must be 0, 1 or 2 substitutions");
  return FEMTO_AMD_OK;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_mismatch_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                              int64_t capacity, int64_t* d_result_start, int64_t* d_first, int64_t* d_last, int32_t* d_cost, int32_t* d_sub_pos,
                              uint16_t* d_sub_sym, int64_t* d_total, void* stream) {
  API_BEGIN
  int rc = check_args(ix, npat, nsyms, k);
  if (rc) return rc;
  if (capacity < 0 || capacity >= kMaxResults || !d_result_start || !d_total || (npat && !d_starts) || (nsyms && !d_syms) ||
      (capacity && (!d_first || !d_last || !d_cost || !d_sub_pos || !d_sub_sym)))
    return set_err(FEMTO_AMD_ERR_PARAM, "null argument or bad capacity (0 <= capacity < 2^31 results; capacity 0 alone takes no result arrays)");
  if (reinterpret_cast<uintptr_t>(d_syms) & 1u) return set_err(FEMTO_AMD_ERR_PARAM, "d_syms must be 2-byte aligned (uint16 symbols)");
  if ((rc = check_device_handle(ix, kSubject))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npat == 0) return empty_result_async(d_result_start, d_total, st);
  return run_mismatch(ix, npat, nsyms, d_syms, d_starts, k, capacity, d_result_start, Out{d_first, d_last, d_cost, d_sub_pos, d_sub_sym}, d_total, st);
  API_END
}

void femto_amd_mismatch_free(femto_amd_mismatch_result_t* out) {
  if (!out) return;
  free(out->result_start);
  free(out->first);
  free(out->last);
  free(out->cost);
  free(out->sub_pos);
  free(out->sub_sym);
  memset(out, 0, sizeof *out);
}

int femto_amd_mismatch(femto_amd_index_t* ix0, int64_t npat, const int32_t* plen, const uint16_t* syms, int k, femto_amd_mismatch_result_t* out) {
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
    femto_amd_mismatch_free(out);
    return code;
  };
  hipStream_t st = nullptr;
  Temp T;
  uint16_t* d_syms;
  int64_t *d_starts, *d_rs, *d_tot, *d_first, *d_last;
  int32_t *d_cost, *d_pos;
  uint16_t* d_sym;
  if ((rc = T.put(&d_syms, syms, size_t(nsyms))) || (rc = T.put(&d_starts, starts)) || (rc = T.get(&d_rs, size_t(npat) + 1)) || (rc = T.get(&d_tot, 2)))
    return fail(rc);
  const Out none{nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t tot[2] = {0, 0};
  // the counting pass sizes the filling pass
  if ((rc = run_mismatch(ix, npat, nsyms, d_syms, d_starts, k, 0, d_rs, none, d_tot, st))) return fail(rc);
  if ((rc = words_to_host(2, d_tot, st, "counting the results failed on the device", tot))) return fail(rc);
  const int64_t total = tot[0];
  if (total >= kMaxResults) return fail(set_err(FEMTO_AMD_ERR_FULL, "2^31 results or more: search the patterns in smaller batches"));
  if (total) {
    const size_t ut = size_t(total);
    if ((rc = T.get(&d_first, ut)) || (rc = T.get(&d_last, ut)) || (rc = T.get(&d_cost, ut)) || (rc = T.get(&d_pos, 2 * ut)) || (rc = T.get(&d_sym, 2 * ut)) ||
        (rc = run_mismatch(ix, npat, nsyms, d_syms, d_starts, k, total, d_rs, Out{d_first, d_last, d_cost, d_pos, d_sym}, d_tot, st)) ||
        (rc = list_to_host(int64_t(ut), d_first, st, "copying the results back", &out->first, false)) ||
        (rc = list_to_host(int64_t(ut), d_last, st, "copying the results back", &out->last, false)) ||
        (rc = list_to_host(int64_t(ut), d_cost, st, "copying the results back", &out->cost, false)) ||
        (rc = list_to_host(int64_t(2 * ut), d_pos, st, "copying the results back", &out->sub_pos, false)) ||
        (rc = list_to_host(int64_t(2 * ut), d_sym, st, "copying the results back", &out->sub_sym, false)))
      return fail(rc);
  }
  if ((rc = result_start_to_host(npat, d_rs, st, out->result_start))) return fail(rc);
  out->total = total;
  return FEMTO_AMD_OK;
  API_END
}
