// seeds.hpp -- what ../hamming/hamming.hip and ../leven/leven.hip share: the searches by exact seeds.  A pattern of m symbols is cut
// into k + 1 pieces, piece j = [j m / (k + 1), (j + 1) m / (k + 1)); the pieces are located exactly (the locate chain, row-free
// form) and every located offset is a CANDIDATE that the module checks against the text its own way -- a window compare there, an
// extension with edits here.  This header holds the part in front of the check and around it.  In front: the work area kept with
// the extractor and a call's turn on it, the piece table, the sum of the pieces' counts (what sizes the candidate buffer of a host
// form), the one locate call and the lookup of a candidate's pattern and piece.  Around: the driver that takes the module's check
// over the candidates on either path, the checks of a device form and the prologue of a host form.  The check itself, the
// records, the order tail and the two passes of a host form are the module's.
//
// PIECE TABLE.  16 lanes per pattern: the symbols are checked (byte characters only) and, for a module that compares dense codes,
// turned into the dense codes the text is held in (0xff for a character the text lacks); the k + 1 pieces are written as
// (length, start) spans of the CALLER'S symbols.  A refused pattern's pieces are one symbol long and point at a symbol >= 261 of the
// work area: they reach the chain as patterns that match nothing, never as empty patterns (which match every row).
// WORK AREA.  The buffers between the steps belong to the extractor and grow on demand.  A call locks the area while it enqueues,
// makes its stream wait for the event of the call before it and records its own: calls on one work area run one after another
// on the device, whatever their streams; nothing waits on the host once the buffers have their size.
// Device and host; included after ../csrc/api_internal.hpp, host_common.hpp, result_order.hpp and ../extract/extractor.hpp; no
// object of its own.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <memory>
#include <mutex>

namespace femto_amd {
namespace seeds {

constexpr int32_t kMaxPattern = 32768;            // MAX_PATTERN_LENGTH
constexpr int64_t kMaxCall = int64_t(1) << 31;    // pieces, symbols, candidates and results per call: 32-bit indexes
constexpr uint32_t kByte0 = FEMTO_AMD_CHARACTER_OFFSET, kAlpha = FEMTO_AMD_ALPHA_SIZE;
constexpr uint8_t kServed = 1, kSlow = 2;         // flags[q]: the pattern is searched; ... symbol by symbol (see pieces_kernel)
constexpr int64_t kChunkSyms = int64_t(1) << 26;  // sample path: the windows come through 128 MiB of symbols at a time
constexpr int kBadAt = 32;                        // misc: the symbol >= 261 of refused pieces, 16 bytes of its like on either side

// misc (int64 words): [0], [1] the chain's total and overflow flag, [2] the sum of the pieces' counts (host form), [3] the longest
// served pattern (sample path); bytes 64 .. 127 hold 0xffff symbols.  A module derives its own area from this one and releases
// what it adds
struct Area : ExtractorWork {
  std::mutex mu;
  hipEvent_t done = nullptr;
  bool used = false;
  DeviceBuffer misc, plen, starts, dense, flags, noccs, ostarts, offs, first, last, w_pos, w_len, w_ost, w_syms;
  ~Area() override {
    for (DeviceBuffer* b : {&misc, &plen, &starts, &dense, &flags, &noccs, &ostarts, &offs, &first, &last, &w_pos, &w_len, &w_ost, &w_syms}) b->release();
    if (done) (void)hipEventDestroy(done);
  }
};

// ... and on top of it the order stage's buffers and device_scan's tile sums: a module's area derives from this and adds its records
struct OrderArea : Area {
  DeviceBuffer keys, keys2, idx, idx2, pk, pk2, sorttmp, scan[3];
  ~OrderArea() override { for (DeviceBuffer* b : {&keys, &keys2, &idx, &idx2, &pk, &pk2, &sorttmp, &scan[0], &scan[1], &scan[2]}) b->release(); }
  OrderBuffers order() { return OrderBuffers{keys, keys2, idx, idx2, pk, pk2, sorttmp}; }
};

// the module's work area W (derived from Area) in its slot of the extractor, made on first use
template <class W>
int work_of(femto_amd_extractor* ex, std::unique_ptr<ExtractorWork>& slot, W** out) {
  std::lock_guard<std::mutex> lk(ex->work_mu);
  if (!slot) {
    std::unique_ptr<W> w(new W());
    int rc;
    if ((rc = w->misc.reserve(128))) return rc;
    HIP_TRY(hipMemset(w->misc.p, 0, 64));
    HIP_TRY(hipMemset(static_cast<char*>(w->misc.p) + 64, 0xff, 64));
    HIP_TRY(hipEventCreateWithFlags(&w->done, hipEventDisableTiming));
    slot = std::move(w);
  }
  *out = static_cast<W*>(slot.get());
  return 0;
}

// one call's turn on the work area: the lock while it enqueues, its stream behind the call before it
struct Turn {
  Area& W;
  hipStream_t st;
  std::unique_lock<std::mutex> lk;
  int rc = 0;
  Turn(Area& w, hipStream_t s) : W(w), st(s), lk(w.mu) {
    if (W.used && hipStreamWaitEvent(st, W.done, 0) != hipSuccess) rc = set_err(FEMTO_AMD_ERR_INVALID, "hipStreamWaitEvent failed");
  }
  ~Turn() {
    if (hipEventRecord(W.done, st) == hipSuccess) W.used = true;
  }
};

// ---- piece table ----------------------------------------------------------------------------------------------------------------

struct Pieces {
  int32_t* plen;       // npat * (k + 1)
  int64_t* starts;     // ... in symbols from d_syms
  uint8_t* dense;      // nsyms dense codes (kDense), 16 bytes of slack behind them
  uint8_t* flags;      // npat
  int64_t* maxm;       // or NULL
};

// 16 lanes per pattern.  kDense: the handle holds the text, `alpha` maps its dense codes to alpha codes.  A served pattern is
// kSlow when it holds a character the text lacks AND 0xff is a code of the text: the marker would then compare equal to it
template <bool kDense>
inline __global__ __launch_bounds__(256) void pieces_kernel(const int64_t npat, const int64_t nsyms, const uint16_t* __restrict__ syms,
                                                            const int64_t* __restrict__ starts, const int kp1, const uint16_t* __restrict__ alpha,
                                                            const int64_t bad_start, const Pieces T) {
  __shared__ uint8_t s_inv[264];
  if (kDense) {
    for (int i = threadIdx.x; i < 264; i += 256) s_inv[i] = 0xff;
    __syncthreads();
    const uint32_t a = alpha[threadIdx.x];
    if (a >= kByte0 && a < kAlpha) s_inv[a] = uint8_t(threadIdx.x);
    __syncthreads();
  }
  const bool has255 = kDense && alpha[255] != 0;      // (any character of the text, SEOF too)
  const int lane = threadIdx.x & 63, gl = lane & 15, gbase = lane & 48;
  const int64_t q = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const bool in = q < npat;
  const int64_t s = in ? starts[q] : 0, m64 = in ? starts[q + 1] - s : 0;
  const bool ok = in && s >= 0 && m64 >= int64_t(kp1) && s + m64 <= nsyms && m64 <= int64_t(kMaxPattern);
  const int m = ok ? int(m64) : 0;
  bool bad = false, lack = false;
  for (int i = gl; i < m; i += 16) {
    const uint32_t a = syms[s + i];
    const bool b = a < kByte0 || a >= kAlpha;
    bad = bad || b;
    if (kDense) {
      const uint8_t d = b ? uint8_t(0xff) : s_inv[a];
      T.dense[s + i] = d;
      lack = lack || d == 0xff;
    }
  }
  const bool gbad = (uint32_t(__ballot(bad) >> gbase) & 0xffffu) != 0, glack = (uint32_t(__ballot(lack) >> gbase) & 0xffffu) != 0;
  if (!in) return;
  const bool served = ok && !gbad;
  if (gl == 0) {
    T.flags[q] = served ? uint8_t(kServed | (glack && has255 ? kSlow : 0)) : uint8_t(0);
    if (T.maxm && served) atomicMax(reinterpret_cast<unsigned long long*>(T.maxm), static_cast<unsigned long long>(m));
  }
  for (int j = gl; j < kp1; j += 16) {
    const int64_t at = q * kp1 + j;
    const int b0 = j * m / kp1, b1 = (j + 1) * m / kp1;
    T.plen[at] = served ? b1 - b0 : 1;
    T.starts[at] = served ? s + b0 : bad_start;
  }
}

// the sum of last - first + 1 over the pieces (host form: what sizes the candidate buffer)
inline __global__ __launch_bounds__(256) void cand_sum_kernel(const int64_t np, const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                              unsigned long long* __restrict__ sum) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  unsigned long long v = i < np && last[i] >= first[i] ? static_cast<unsigned long long>(last[i] - first[i] + 1) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(sum, v);
}

// ---- candidates -----------------------------------------------------------------------------------------------------------------

struct Seeds {
  const int64_t* ostarts;    // np + 1: piece i's candidates are offs[ostarts[i] .. ostarts[i + 1])
  const int64_t* offs;
  const int64_t* total;      // [0] candidates, [1] 1 = more than the buffer holds: nothing is checked
  const uint8_t* flags;
  const int64_t* starts;     // the caller's d_starts
  const uint16_t* syms;      // ... and d_syms
  int64_t np, N;
  int kp1;
};

// candidate c: its pattern q = syms[s .. s + m), its piece j, and p = the piece's offset moved back by the piece's start
struct Cand {
  int64_t q, s, p;
  int m, j;
  uint8_t fl;
};
// false: the pattern is not served (nothing leads here: a refused pattern has no candidates)
__device__ __forceinline__ bool seed_of(const Seeds& S, int64_t c, Cand* C) {
  const int64_t piece = first_gt(S.ostarts, 1, S.np, c) - 1;      // the last piece whose candidates start at or before c
  C->q = piece / S.kp1;
  C->j = int(piece - C->q * S.kp1);
  C->fl = S.flags[C->q];
  if (!(C->fl & kServed)) return false;
  C->s = S.starts[C->q];
  C->m = int(S.starts[C->q + 1] - C->s);
  C->p = S.offs[c] - C->j * C->m / S.kp1;
  return true;
}
// ... and the window [p, p + m) lies in the text.  false: nothing to compare
__device__ __forceinline__ bool candidate(const Seeds& S, int64_t c, Cand* C) {
  return seed_of(S, c, C) && C->p >= 0 && C->p <= S.N - C->m;
}

// sample path: the windows of candidates [c0, c0 + n) as requests to the extractor, `stride` symbols apart.  Window is the module's
// rule: Window::of(S, c, k, &w0, &w1) = candidate c has the window [w0, w1) of the text (false: nothing to check)
template <class Window>
inline __global__ __launch_bounds__(256) void windows_kernel(const Seeds S, const int64_t c0, const int64_t n, const int k, const int64_t stride,
                                                             int64_t* __restrict__ pos, int32_t* __restrict__ len, int64_t* __restrict__ out_start) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t w0 = 0, w1 = 0;
  if (!S.total[1] && c0 + i < S.total[0] && !Window::of(S, c0 + i, k, &w0, &w1)) w0 = w1 = 0;
  const bool some = w1 > w0 && w1 - w0 <= stride;
  pos[i] = some ? w0 : 0;
  len[i] = some ? int32_t(w1 - w0) : 0;
  out_start[i] = i * stride;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// the piece table of the batch into the work area (the caller holds its turn).  dense: the patterns' dense codes too (text path)
inline int make_pieces(femto_amd_extractor* ex, Area& W, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k, bool dense,
                       bool want_maxm, hipStream_t st) {
  const int kp1 = k + 1;
  const size_t np = size_t(npat) * size_t(kp1);
  int rc;
  if ((rc = W.plen.reserve(np * 4)) || (rc = W.starts.reserve(np * 8)) || (rc = W.flags.reserve(size_t(npat))) ||
      (dense && (rc = W.dense.reserve(size_t(nsyms) + 16))))
    return rc;
  HIP_TRY(hipMemsetAsync(W.misc.p, 0, 32, st));
  const uint16_t* bad = reinterpret_cast<const uint16_t*>(static_cast<const char*>(W.misc.p) + 64) + kBadAt / 2;
  const int64_t bad_start = (reinterpret_cast<intptr_t>(bad) - reinterpret_cast<intptr_t>(d_syms)) / 2;      // (both 2-byte aligned)
  const Pieces T{W.plen.as<int32_t>(), W.starts.as<int64_t>(), W.dense.as<uint8_t>(), W.flags.as<uint8_t>(),
                 want_maxm ? W.misc.as<int64_t>() + 3 : nullptr};
  const dim3 grid(uint32_t((npat + 15) / 16));
  return dense ? launch(pieces_kernel<true>, grid, st, npat, nsyms, d_syms, d_starts, kp1, ex->d_alpha, bad_start, T)
               : launch(pieces_kernel<false>, grid, st, npat, nsyms, d_syms, d_starts, kp1, ex->d_alpha, bad_start, T);
}

// The seeds of a call: the piece table, and the pieces located by ONE row-free call of the chain (it leases the handle's scratch
// itself: no lease is held here), its totals into misc.  The caller holds its turn and has reserved its record buffers, so all of
// the search's are reserved in front of its first kernel; its counters are zeroed here, between the two, where they always were
inline int locate_seeds(femto_amd_extractor* ex, Area& W, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k, bool dense,
                        int64_t cand_capacity, void* counters, size_t counter_bytes, hipStream_t st, Seeds* S) {
  const int64_t np = npat * (k + 1);
  int64_t* const seeds_total = W.misc.as<int64_t>();
  int rc;
  if ((rc = W.noccs.reserve(size_t(np) * 4 + 16)) || (rc = W.ostarts.reserve(size_t(np + 1) * 8 + 16)) || (rc = W.offs.reserve(size_t(cand_capacity) * 8 + 16)) ||
      (rc = make_pieces(ex, W, npat, nsyms, d_syms, d_starts, k, dense, ex->path != FEMTO_AMD_EXTRACT_PATH_TEXT, st)))
    return rc;
  HIP_TRY(hipMemsetAsync(counters, 0, counter_bytes, st));
  if ((rc = femto_amd_locate_device_v2(ex->ix, np, W.plen.as<int32_t>(), d_syms, W.starts.as<int64_t>(), INT_MAX, nullptr, nullptr, W.noccs.as<int32_t>(),
                                       W.ostarts.as<int64_t>(), W.offs.as<int64_t>(), cand_capacity, seeds_total, st)))
    return rc;
  *S = Seeds{W.ostarts.as<int64_t>(), W.offs.as<int64_t>(), seeds_total, W.flags.as<uint8_t>(), d_starts, d_syms, np, ex->ix->host.total_length, k + 1};
  return 0;
}

// The module's check over the candidates.  Text path: one launch whose grid strides over them, enqueue-only; grid_env (tests) bounds
// the grid, so that every lane takes several.  Sample path: the candidate total and the longest served pattern are read back (the
// call's one wait) and the windows, that pattern + pad symbols apart, are extracted and checked chunk by chunk; chunk_env (tests)
// bounds a chunk's symbols
template <class Window, class OnText, class OnSamples>
int for_candidates(femto_amd_extractor* ex, Area& W, const Seeds& S, int k, int64_t cand_capacity, int64_t pad, const char* grid_env,
                   const char* chunk_env, hipStream_t st, OnText on_text, OnSamples on_samples) {
  int rc;
  if (ex->path == FEMTO_AMD_EXTRACT_PATH_TEXT) {
    if (!cand_capacity) return 0;
    const int64_t most = std::max<int64_t>(1, knob(-1, grid_env, int64_t(ex->ix->num_cus) * 64));
    return on_text(dim3(uint32_t(std::max<int64_t>(1, std::min<int64_t>((cand_capacity + 255) / 256, most)))));
  }
  int64_t h[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, S.total, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t ncand = h[1] ? 0 : h[0], stride = std::max<int64_t>(h[3], 1) + pad;
  const int64_t chunk_syms = std::max<int64_t>(1, std::min(kChunkSyms, knob(-1, chunk_env, kChunkSyms)));
  const int64_t chunk = std::max<int64_t>(1, std::min(ncand, chunk_syms / stride));
  if (ncand && ((rc = W.w_pos.reserve(size_t(chunk) * 8)) || (rc = W.w_len.reserve(size_t(chunk) * 4)) || (rc = W.w_ost.reserve(size_t(chunk) * 8)) ||
                (rc = W.w_syms.reserve(size_t(chunk) * size_t(stride) * 2))))
    return rc;
  for (int64_t c0 = 0; c0 < ncand; c0 += chunk) {
    const int64_t cn = std::min(chunk, ncand - c0);
    if ((rc = launch(windows_kernel<Window>, blocks_of(cn), st, S, c0, cn, k, stride, W.w_pos.as<int64_t>(), W.w_len.as<int32_t>(), W.w_ost.as<int64_t>())) ||
        (rc = femto_amd_extract_device(ex, cn, W.w_pos.as<int64_t>(), W.w_len.as<int32_t>(), W.w_ost.as<int64_t>(), W.w_syms.as<uint16_t>(), st)) ||
        (rc = on_samples(W.w_syms.as<uint16_t>(), stride, c0, cn)))
      return rc;
  }
  return 0;
}

// host form: the sum of the pieces' counts, as femto_amd_count_device gives them
inline int count_candidates(femto_amd_extractor* ex, Area& W, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k,
                            bool dense, hipStream_t st, int64_t* out) {
  const int64_t np = npat * (k + 1);
  Turn turn(W, st);
  int rc = turn.rc;
  if (rc) return rc;
  if ((rc = W.first.reserve(size_t(np) * 8)) || (rc = W.last.reserve(size_t(np) * 8)) ||
      (rc = make_pieces(ex, W, npat, nsyms, d_syms, d_starts, k, dense, false, st)) ||
      (rc = femto_amd_count_device(ex->ix, np, W.plen.as<int32_t>(), d_syms, W.starts.as<int64_t>(), W.first.as<int64_t>(), W.last.as<int64_t>(), st)) ||
      (rc = launch(cand_sum_kernel, blocks_of(np), st, np, W.first.as<int64_t>(), W.last.as<int64_t>(), W.misc.as<unsigned long long>() + 2)))
    return rc;
  HIP_TRY(hipMemcpyAsync(out, W.misc.as<int64_t>() + 2, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// the batch and the bound of either form; k_message refuses a k outside 0 .. max_k
inline int check_args(femto_amd_extractor* ex, int64_t npat, int64_t nsyms, int k, int max_k, const char* k_message) {
  if (!ex || npat < 0 || nsyms < 0 || nsyms >= kMaxCall || (npat == 0 && nsyms != 0))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments (0 <= npat, 0 <= nsyms < 2^31 symbols, no symbols without patterns)");
  if (k < 0 || k > max_k) return set_err(FEMTO_AMD_ERR_PARAM, k_message);
  if (npat * (k + 1) >= kMaxCall) return set_err(FEMTO_AMD_ERR_PARAM, "npat * (k + 1) pieces must stay below 2^31: search the patterns in smaller batches");
  return FEMTO_AMD_OK;
}

const char* const kSubject = "search by exact seeds is";      // (check_plain_handle's words)

// what a device form checks before it answers.  arrays: the module's result arrays are all there
inline int check_device_call(femto_amd_extractor* ex, int64_t npat, int64_t nsyms, const uint16_t* d_syms, const int64_t* d_starts, int k, int max_k,
                             const char* k_message, int64_t cand_capacity, int64_t capacity, const void* d_result_start, const void* d_total, bool arrays) {
  int rc = check_args(ex, npat, nsyms, k, max_k, k_message);
  if (rc) return rc;
  if (cand_capacity < 0 || cand_capacity >= kMaxCall || capacity < 0 || capacity >= kMaxCall || !d_result_start || !d_total || (npat && !d_starts) ||
      (nsyms && !d_syms) || (capacity && !arrays))
    return set_err(FEMTO_AMD_ERR_PARAM, "null argument or bad capacity (0 <= cand_capacity, capacity < 2^31; capacity 0 alone takes no result arrays)");
  if (reinterpret_cast<uintptr_t>(d_syms) & 1u) return set_err(FEMTO_AMD_ERR_PARAM, "d_syms must be 2-byte aligned (uint16 symbols)");
  if (ex->multi) return refuse_multi_device();
  return check_plain_handle(ex->ix, kSubject);
}

// The prologue of a host form in two steps, between which the module allocates its result_start and answers npat == 0: the checks ...
inline int check_host_batch(femto_amd_extractor* ex, int64_t npat, const int32_t* plen, const uint16_t* syms, int k, int max_k, const char* k_message,
                            std::vector<int64_t>* starts, int64_t* nsyms) {
  if (!ex || npat < 0 || (npat && !plen)) return set_err(FEMTO_AMD_ERR_PARAM, "null argument or negative npat");
  if (k < 0 || k > max_k) return set_err(FEMTO_AMD_ERR_PARAM, k_message);
  int rc = pattern_starts(npat, plen, k + 1, kMaxPattern, "a pattern holds k + 1 .. 32768 symbols", starts);
  if (rc) return rc;
  *nsyms = (*starts)[size_t(npat)];
  if ((rc = check_args(ex, npat, *nsyms, k, max_k, k_message))) return rc;
  if (*nsyms && !syms) return set_err(FEMTO_AMD_ERR_PARAM, "null symbols");
  for (int64_t j = 0; j < *nsyms; j++)
    if (syms[j] < FEMTO_AMD_CHARACTER_OFFSET || syms[j] >= FEMTO_AMD_ALPHA_SIZE)
      return set_err(FEMTO_AMD_ERR_PARAM, "a pattern holds byte characters only (codes 5 .. 260)");
  if ((rc = check_plain_handle(ex->ix, kSubject))) return rc;     // (replica 0 of a multi-device handle)
  HIP_TRY(hipSetDevice(ex->ix->device));
  return FEMTO_AMD_OK;
}

struct HostBatch {
  const uint16_t* d_syms;      // 8 symbols of slack on either side: "reads around the symbols"
  int64_t *d_starts, *d_rs, *d_tot, cands = 0;
};

// ... and the module's work area, the batch on the device (T frees it) and the pieces' counts, which size the passes
template <class W>
int upload_host_batch(femto_amd_extractor* ex, std::unique_ptr<ExtractorWork>& slot, Temp& T, const std::vector<int64_t>& starts, const uint16_t* syms,
                      int k, bool dense, size_t words, hipStream_t st, W** work, HostBatch* B) {
  const int64_t npat = int64_t(starts.size()) - 1, nsyms = starts.back();
  int rc;
  uint16_t* buf;
  if ((rc = work_of(ex, slot, work)) || (rc = T.get(&buf, size_t(nsyms) + 16))) return rc;
  if (hipMemset(buf, 0, (size_t(nsyms) + 16) * 2) != hipSuccess || hipMemcpy(buf + 8, syms, size_t(nsyms) * 2, hipMemcpyHostToDevice) != hipSuccess)
    return set_err(FEMTO_AMD_ERR_INVALID, "uploading the patterns failed");
  B->d_syms = buf + 8;
  if ((rc = T.put(&B->d_starts, starts)) || (rc = T.get(&B->d_rs, size_t(npat) + 1)) || (rc = T.get(&B->d_tot, words)) ||
      (rc = count_candidates(ex, **work, npat, nsyms, B->d_syms, B->d_starts, k, dense, st, &B->cands)))
    return rc;
  if (B->cands >= kMaxCall) return set_err(FEMTO_AMD_ERR_FULL, "2^31 candidates or more: search the patterns in smaller batches");
  return FEMTO_AMD_OK;
}

}  // namespace seeds
}  // namespace femto_amd
