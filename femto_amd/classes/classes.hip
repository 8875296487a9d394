// classes.hip -- search with a character class per position: for every pattern of a batch, the strings that occur in the index and
// hold, at each position, the pattern's literal or a member of the pattern's class there, each with its row range.
// include/femto_amd.h "search with character classes" states the contract; DESIGN.md "Search with character classes" the kernels,
// the stack and the registers.
//
// TAKEN FROM THE REFERENCE: what a set, a period and --icase mean (set_node_invert ast.c:324, period_range ast.c:33, icase_ast
// ast.c:556: classes of BYTES) and the order of its result list (regexp_result_list_sort, server.c:1528: by first row).  NOT TAKEN:
// the automaton.  A pattern of fixed length needs none -- the search is the backward search of count with, at a class position,
// every member of the class tried.
//
// MEMBER TABLE.  One 256-lane workgroup per class: lane b keeps byte b when the class holds it and the text does
// (C[ch + 1] > C[ch]); the survivors are compacted in character order with their codes in the handle's rank layout -- a SubTable
// (../common/sub_table.hpp) per class.
// SEARCH.  One lane per pattern, depth first from the pattern's last symbol to its first.  A literal is one P::search_step (step 0
// from the whole index, 1 afterwards, as subst_kernel of ../mismatch/mismatch.hip calls it).  At a class position the lane keeps
// the range it arrived with, tries the members one after another and goes on to the left with each that leaves a range.  An empty
// range or a finished string returns to the nearest class position on the right that has members left; the lane stops when none
// has.  Every string is reached once: the counts are exact whatever the capacity.
// THE STACK lives in the handle's scratch, addressed by the symbol's index in the flat batch: per symbol one range (16 bytes) and
// one word = the next member to try | (the class position to the right + 1) << 16, so a return never rescans the pattern and the
// depth is bounded by the pattern's length alone.  An entry is written when a member leaves a range and read when the lane
// comes back: the first member at a position is tried from registers.
// EMIT is that of mismatch.hip: atomicAdd on the pattern's counter and on the total, the record written when its slot is below the
// capacity.  ORDER is the stage of ../common/result_order.hpp (two stable radix sorts of the records' indexes, by first, then by
// pattern) and a gather.
// A lane is a chain of dependent scattered loads and lanes retire at very different depths: the search kernel is held to the
// policy's kDirectWaves wavefronts per SIMD.  ONE LANE OWNS ONE PATTERN: a pattern with an enormous fan-out ("...." over a byte
// text) is searched serially by its lane.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

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
#include "../csrc/query_parser.hpp"

namespace femto_amd {
namespace {

constexpr int32_t kMaxPattern = 32768;               // MAX_PATTERN_LENGTH, as mismatch.hip: a position + 1 fits 16 bits
constexpr int64_t kMaxSyms = int64_t(1) << 31;       // symbols per call
constexpr int64_t kMaxResults = int64_t(1) << 31;    // results per call: the sorts carry 32-bit indexes
constexpr uint32_t kClass = uint32_t(FEMTO_AMD_CLASS_SYMBOL);
constexpr int64_t kMaxClasses = FEMTO_AMD_MAX_CLASSES;
const char* const kSubject = "search with character classes is";

// the records as the lanes emit them (any order), and the counters: counts[q] = results of pattern q, counts[npat] = all
struct Records {
  int64_t *first, *last;
  uint32_t* pat;
  unsigned long long* counts;
  int64_t npat, capacity;
};

__device__ __forceinline__ void emit(const Records& R, int64_t q, int64_t first, int64_t last) {
  atomicAdd(R.counts + q, 1ull);
  const int64_t slot = int64_t(atomicAdd(R.counts + R.npat, 1ull));
  if (slot >= R.capacity) return;
  R.first[slot] = first;
  R.last[slot] = last;
  R.pat[slot] = uint32_t(q);
}

// One workgroup per class: tab[c] = the bytes of class c that occur in the text, in character order
template <class P>
__global__ __launch_bounds__(256) void member_table_kernel(const DevIndex ix, const uint64_t* __restrict__ classes, SubTable* __restrict__ tab) {
  __shared__ int s_wave[4];
  const uint32_t c = blockIdx.x, b = threadIdx.x, ch = b + kByte0;
  const bool in_text = ((classes[4 * size_t(c) + (b >> 6)] >> (b & 63)) & 1u) && ix.C[ch + 1] > ix.C[ch];
  const uint32_t code = in_text ? uint32_t(P::code_of(ix, ch)) & 0xffffu : 0xffffu;
  const bool have = code != 0xffffu;
  int count;
  const int r = block_rank(have, s_wave, &count);
  if (have) tab[c].pair[r] = ch | (code << 16);
  if (b == 0) tab[c].n = count;
}

// One lane per pattern.  rng / word: the stack, one entry per symbol of the flat batch
template <class P>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P::kDirectWaves, P::kDirectWaves))) void classes_kernel(
    const DevIndex ix, const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms, const int64_t* __restrict__ starts,
    const uint32_t nclasses, const SubTable* __restrict__ tab, longlong2* __restrict__ rng, uint32_t* __restrict__ word, const Records R) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (q >= npat) return;
  const int64_t s = starts[q], len64 = starts[q + 1] - s;
  if (s < 0 || len64 < 0 || s + len64 > nsyms) return;        // starts that leave the nsyms symbols the caller stated: nothing is read
  if (len64 > int64_t(kMaxPattern)) return;                   // (the host form refuses it; here it has no results)
  const int len = int(len64);
  const uint16_t* __restrict__ const pat = syms + s;
  longlong2* __restrict__ const prng = rng + s;
  uint32_t* __restrict__ const pword = word + s;
  int64_t first = 0, last = ix.total_length - 1;      // the empty pattern's range
  int pos = len - 1;
  int right = -1;             // the nearest class position on the right that may have members left
  bool fresh = false;         // `right` was reached from the right just now: its entry is (w, r), not yet in memory
  uint32_t w = 0;
  longlong2 r = make_longlong2(0, -1);
  for (;;) {
    // to the left, until a class position, an empty range or the pattern's first symbol
    bool whole = true;
    for (; pos >= 0; pos--) {
      const uint32_t sym = pat[pos];
      if (sym & kClass) {
        whole = false;
        if ((sym & ~kClass) >= nclasses) break;      // no such class: no string of this pattern is ever finished
        r = make_longlong2(first, last);
        w = uint32_t(right + 1) << 16;
        right = pos;
        fresh = true;
        break;
      }
      const uint32_t code = code_or_none<P>(ix, sym);
      if (code == 0xffffu) {      // the character does not occur in the text (or is no alpha code)
        whole = false;
        break;
      }
      P::search_step(ix, pos == len - 1 ? 0 : 1, code, first, last);
      if (first > last) {
        whole = false;
        break;
      }
    }
    if (whole) emit(R, q, first, last);
    // back to the nearest class position with a member that leaves a range
    for (;;) {
      if (!fresh) {
        if (right < 0) return;
        w = pword[right];
        r = prng[right];
      }
      fresh = false;
      // (an entry is this lane's own unless patterns overlap in d_syms, which is not supported: the two checks below only keep
      // such a batch inside the class table and inside its own pattern)
      const uint32_t c = uint32_t(pat[right]) ^ kClass;
      const SubTable* __restrict__ const t = tab + (c < nclasses ? c : 0u);
      const int n = c < nclasses ? t->n : 0;
      int i = int(w & 0xffffu);
      bool found = false;
      for (; i < n; i++) {
        first = r.x;
        last = r.y;
        P::search_step(ix, right == len - 1 ? 0 : 1, t->pair[i] >> 16, first, last);
        if (first <= last) {
          found = true;
          break;
        }
      }
      if (found) {
        prng[right] = r;
        pword[right] = (w & 0xffff0000u) | uint32_t(i + 1);
        pos = right - 1;
        break;
      }
      const int up = int(w >> 16) - 1;
      right = up > right && up < len ? up : -1;
    }
  }
}

// ---- order -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void total_kernel(const Records R, int64_t* __restrict__ d_total) {
  if (blockIdx.x == 0 && threadIdx.x == 0) write_total(d_total, int64_t(R.counts[R.npat]), R.capacity);
}

__global__ __launch_bounds__(256) void gather_kernel(const Records R, const uint32_t* __restrict__ idx, int64_t* __restrict__ out_first,
                                                     int64_t* __restrict__ out_last) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= live_records(R.counts + R.npat, R.capacity)) return;
  const uint32_t r = idx[s];
  out_first[s] = R.first[r];
  out_last[s] = R.last[r];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

template <class P>
int search_all(femto_amd_index* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int64_t nclasses,
               const uint64_t* d_classes, SubTable* tab, longlong2* rng, uint32_t* word, const Records& R, hipStream_t st) {
  int rc;
  if (nclasses && (rc = launch(member_table_kernel<P>, dim3(uint32_t(nclasses)), st, ix->dev, d_classes, tab))) return rc;
  return launch(classes_kernel<P>, blocks_of(npat), st, ix->dev, npat, nsyms, d_syms, d_starts, uint32_t(nclasses), tab, rng, word, R);
}

int run_classes(femto_amd_index* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int64_t nclasses,
                const uint64_t* d_classes, int64_t capacity, int64_t* d_result_start, int64_t* d_first, int64_t* d_last, int64_t* d_total,
                hipStream_t st) {
  Lease L(ix, st);
  if (!L.s) return L.rc;
  Scratch& S = *L.s;
  int rc;
  const size_t cap = size_t(capacity), un = size_t(npat);
  if ((rc = S.tail.reserve(size_t(std::max<int64_t>(nclasses, 1)) * sizeof(SubTable))) || (rc = S.pairs.reserve((size_t(nsyms) + 1) * 20)) ||
      (rc = S.noccs64.reserve((un + 1) * 8)) || (rc = S.first.reserve(cap * 8 + 8)) || (rc = S.last.reserve(cap * 8 + 8)) ||
      (rc = S.rows.reserve(cap * 4 + 8)))
    return rc;
  const Records R{S.first.as<int64_t>(), S.last.as<int64_t>(), S.rows.as<uint32_t>(), S.noccs64.as<unsigned long long>(), npat, capacity};
  HIP_TRY(hipMemsetAsync(R.counts, 0, (un + 1) * 8, st));
  longlong2* const rng = S.pairs.as<longlong2>();      // the stack: nsyms + 1 ranges, then the nsyms words
  uint32_t* const word = reinterpret_cast<uint32_t*>(rng + nsyms + 1);
  auto go = [&](auto tag) {
    using P = typename decltype(tag)::type;
    return search_all<P>(ix, npat, nsyms, d_syms, d_starts, nclasses, d_classes, S.tail.as<SubTable>(), rng, word, R, st);
  };
  if ((rc = with_lane_policy(ix, "search with character classes on this handle needs", go))) return rc;
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
  return launch(gather_kernel, blocks_of(capacity), st, R, o.idx, d_first, d_last);
}

int check_args(femto_amd_index* ix, int64_t npat, int64_t nsyms, int64_t nclasses, const void* classes) {
  if (!ix || npat < 0 || npat >= kMaxResults || nsyms < 0 || nsyms >= kMaxSyms || (npat == 0 && nsyms != 0))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= npat < 2^31 patterns, 0 <= nsyms < 2^31 symbols, no symbols without patterns)");
  if (nclasses < 0 || nclasses > kMaxClasses) return set_err(FEMTO_AMD_ERR_PARAM, "nclasses must be 0 .. 4096");
  if (nclasses && !classes) return set_err(FEMTO_AMD_ERR_PARAM, "null class table with nclasses > 0");
  return FEMTO_AMD_OK;
}

// ---- query text -> class pattern (host only) ----------------------------------------------------------------------------------------

struct ClassPattern {
  std::vector<uint16_t> syms;
  std::vector<uint64_t> classes;                      // four words per class
  std::map<std::vector<uint64_t>, uint16_t> number;   // equal sets share a class
};

// the bytes of a set, or false when it holds a code below the bytes beside other members (classes hold bytes only)
bool append_set(const CharClass& set, ClassPattern* out, std::string* err) {
  int members = 0, only = 0;
  bool low = false;
  for (int c = 0; c < kRegexAlpha; c++)
    if (set.get(c)) {
      members++;
      only = c;
      low = low || c < int(kByte0);
    }
  if (members == 1) {      // a set with one member is a literal
    out->syms.push_back(uint16_t(only));
    return true;
  }
  if (low) {
    *err = "a set that holds a code below the bytes";
    return false;
  }
  std::vector<uint64_t> bits(4, 0);
  for (int b = 0; b < 256; b++)
    if (set.get(b + int(kByte0))) bits[size_t(b >> 6)] |= uint64_t(1) << (b & 63);
  auto it = out->number.find(bits);
  if (it == out->number.end()) {
    if (out->number.size() >= size_t(kMaxClasses)) {
      *err = "more than 4096 different sets";
      return false;
    }
    it = out->number.emplace(bits, uint16_t(out->number.size())).first;
    out->classes.insert(out->classes.end(), bits.begin(), bits.end());
  }
  out->syms.push_back(uint16_t(kClass | it->second));
  return true;
}

// a sequence of characters, strings, sets and (after q_icase) groups of one such sequence, none of them repeated
bool append_sequence(const QRegexp& q, ClassPattern* out, std::string* err) {
  if (q.choices.size() != 1) {
    *err = "an alternative";
    return false;
  }
  for (const QAtom& a : q.choices[0].atoms) {
    if (a.rmin != 1 || a.rmax != 1) {
      *err = "a repeat";
      return false;
    }
    switch (a.kind) {
      case QAtom::CHARACTER: out->syms.push_back(uint16_t(a.ch)); break;
      case QAtom::STRING: out->syms.insert(out->syms.end(), a.str.begin(), a.str.end()); break;
      case QAtom::SET:
        if (!append_set(a.set, out, err)) return false;
        break;
      case QAtom::GROUP:
        if (!append_sequence(a.group[0], out, err)) return false;
        break;
    }
  }
  return true;
}

// what the PARSED query may hold: q_icase wraps strings into groups of its own, so groups are looked for before it runs
bool plain_concatenation(const QRegexp& q, std::string* err) {
  if (q.has_approx) {
    *err = "APPROX";
    return false;
  }
  if (q.choices.size() != 1) {
    *err = "an alternative";
    return false;
  }
  for (const QAtom& a : q.choices[0].atoms) {
    if (a.kind == QAtom::GROUP) {
      *err = "a group";
      return false;
    }
    if (a.rmin != 1 || a.rmax != 1) {
      *err = "a repeat";
      return false;
    }
  }
  return true;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_classes_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts,
                             int64_t nclasses, const uint64_t* d_classes, int64_t capacity, int64_t* d_result_start, int64_t* d_first,
                             int64_t* d_last, int64_t* d_total, void* stream) {
  API_BEGIN
  int rc = check_args(ix, npat, nsyms, nclasses, d_classes);
  if (rc) return rc;
  if (capacity < 0 || capacity >= kMaxResults || !d_result_start || !d_total || (npat && !d_starts) || (nsyms && !d_syms) ||
      (capacity && (!d_first || !d_last)))
    return set_err(FEMTO_AMD_ERR_PARAM, "null argument or bad capacity (0 <= capacity < 2^31 results; capacity 0 alone takes no result arrays)");
  if (reinterpret_cast<uintptr_t>(d_syms) & 1u) return set_err(FEMTO_AMD_ERR_PARAM, "d_syms must be 2-byte aligned (uint16 symbols)");
  if (reinterpret_cast<uintptr_t>(d_classes) & 7u) return set_err(FEMTO_AMD_ERR_PARAM, "d_classes must be 8-byte aligned (uint64 words)");
  if ((rc = check_device_handle(ix, kSubject))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npat == 0) return empty_result_async(d_result_start, d_total, st);
  return run_classes(ix, npat, nsyms, d_syms, d_starts, nclasses, d_classes, capacity, d_result_start, d_first, d_last, d_total, st);
  API_END
}

void femto_amd_classes_free(femto_amd_classes_result_t* out) {
  if (!out) return;
  free(out->result_start);
  free(out->first);
  free(out->last);
  memset(out, 0, sizeof *out);
}

int femto_amd_classes(femto_amd_index_t* ix0, int64_t npat, const int32_t* plen, const uint16_t* syms, int64_t nclasses, const uint64_t* classes,
                      femto_amd_classes_result_t* out) {
  API_BEGIN
  if (!out) return set_err(FEMTO_AMD_ERR_PARAM, "null result");
  memset(out, 0, sizeof *out);
  if (!ix0 || npat < 0 || (npat && !plen)) return set_err(FEMTO_AMD_ERR_PARAM, "null argument or negative npat");
  femto_amd_index* ix = replica0(ix0);
  std::vector<int64_t> starts;
  int rc = pattern_starts(npat, plen, 0, kMaxPattern, "a pattern holds 0 .. 32768 symbols", &starts);
  if (rc) return rc;
  const int64_t nsyms = starts[size_t(npat)];
  if ((rc = check_args(ix, npat, nsyms, nclasses, classes))) return rc;
  if (nsyms && !syms) return set_err(FEMTO_AMD_ERR_PARAM, "null symbols");
  for (int64_t j = 0; j < nsyms; j++) {
    const uint32_t sym = syms[j];
    if (sym >= uint32_t(FEMTO_AMD_ALPHA_SIZE) && (!(sym & kClass) || int64_t(sym & ~kClass) >= nclasses))
      return set_err(FEMTO_AMD_ERR_PARAM, "a symbol that is neither a character code < ALPHA_SIZE nor FEMTO_AMD_CLASS_SYMBOL | a class < nclasses");
  }
  if ((rc = check_plain_handle(ix, kSubject))) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  out->result_start = static_cast<int64_t*>(calloc(size_t(npat) + 1, 8));
  if (!out->result_start) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  out->npat = npat;
  if (npat == 0) return FEMTO_AMD_OK;
  auto fail = [&](int code) {
    femto_amd_classes_free(out);
    return code;
  };
  hipStream_t st = nullptr;
  Temp T;
  uint16_t* d_syms;
  uint64_t* d_classes;
  int64_t *d_starts, *d_rs, *d_tot, *d_first, *d_last;
  if ((rc = T.put(&d_syms, syms, size_t(nsyms))) || (rc = T.put(&d_starts, starts)) || (rc = T.put(&d_classes, classes, size_t(nclasses) * 4)) ||
      (rc = T.get(&d_rs, size_t(npat) + 1)) || (rc = T.get(&d_tot, 2)))
    return fail(rc);
  int64_t tot[2] = {0, 0};
  // the counting pass sizes the filling pass
  if ((rc = run_classes(ix, npat, nsyms, d_syms, d_starts, nclasses, d_classes, 0, d_rs, nullptr, nullptr, d_tot, st))) return fail(rc);
  if ((rc = words_to_host(2, d_tot, st, "counting the results failed on the device", tot))) return fail(rc);
  const int64_t total = tot[0];
  if (total >= kMaxResults) return fail(set_err(FEMTO_AMD_ERR_FULL, "2^31 results or more: search the patterns in smaller batches"));
  if (total) {
    const size_t ut = size_t(total);
    if ((rc = T.get(&d_first, ut)) || (rc = T.get(&d_last, ut)) ||
        (rc = run_classes(ix, npat, nsyms, d_syms, d_starts, nclasses, d_classes, total, d_rs, d_first, d_last, d_tot, st)) ||
        (rc = list_to_host(int64_t(ut), d_first, st, "copying the results back", &out->first, false)) ||
        (rc = list_to_host(int64_t(ut), d_last, st, "copying the results back", &out->last, false)))
      return fail(rc);
  }
  if ((rc = result_start_to_host(npat, d_rs, st, out->result_start))) return fail(rc);
  out->total = total;
  return FEMTO_AMD_OK;
  API_END
}

int femto_amd_class_pattern_compile(const uint8_t* query, int64_t len, int flags, uint16_t* syms, int64_t syms_cap, int64_t* nsyms,
                                    uint64_t* classes, int64_t classes_cap, int64_t* nclasses) {
  API_BEGIN
  if ((len && !query) || len < 0 || !nsyms || !nclasses || syms_cap < 0 || classes_cap < 0 || (syms_cap && !syms) || (classes_cap && !classes))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *nsyms = *nclasses = 0;
  if (len > kRegexMaxLen) return set_err(FEMTO_AMD_ERR_PARAM, "query: pattern text too long");
  std::vector<QTok> toks;
  std::string perr;
  QueryLexer lx(query, len);
  if (!lx.run(&toks, &perr)) return set_err(FEMTO_AMD_ERR_PARAM, "query: " + perr);
  for (const QTok& t : toks)
    if (t.kind == QTok::BOOL) return set_err(FEMTO_AMD_ERR_INVALID, std::string("not a class pattern: it holds a boolean operator (") + t.word + ")");
  QRegexp q;
  QueryParser ps(toks);
  if (!ps.parse(&q, &perr)) return set_err(FEMTO_AMD_ERR_PARAM, "query: " + perr);
  // (streamline_query only trims repeats and simplify_query only joins characters: neither changes a query that passes here)
  if (!plain_concatenation(q, &perr)) return set_err(FEMTO_AMD_ERR_INVALID, "not a class pattern: it holds " + perr);
  if (flags & FEMTO_AMD_QUERY_ICASE) q_icase(q);
  ClassPattern cp;
  if (!append_sequence(q, &cp, &perr)) return set_err(FEMTO_AMD_ERR_INVALID, "not a class pattern: it holds " + perr);
  if (cp.syms.size() > size_t(kMaxPattern)) return set_err(FEMTO_AMD_ERR_PARAM, "a pattern holds 0 .. 32768 symbols");
  *nsyms = int64_t(cp.syms.size());
  *nclasses = int64_t(cp.classes.size() / 4);
  if (*nsyms > syms_cap || *nclasses > classes_cap)
    return set_err(FEMTO_AMD_ERR_FULL, "the pattern needs " + std::to_string(*nsyms) + " symbols and " + std::to_string(*nclasses) + " classes");
  if (*nsyms) memcpy(syms, cp.syms.data(), cp.syms.size() * 2);
  if (*nclasses) memcpy(classes, cp.classes.data(), cp.classes.size() * 8);
  return FEMTO_AMD_OK;
  API_END
}
