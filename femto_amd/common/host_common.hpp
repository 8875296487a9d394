// host_common.hpp -- the host plumbing that doclist.hip, docpos.hip, bquery.hip, extract.hip and the launch layer in ../csrc share: the handle checks, the
// checks of a pattern batch and of a batch of list pairs, the checked kernel launch and the size of a persistent grid, the
// device memory of a blocking host form, the upload of a pattern batch and the rows it locates, the copy of a result back to
// the host -- and what the host forms of mismatch.hip, edit.hip, classes.hip and hamming.hip share on top of that: the handle
// check of a device form, the layout of a batch given by its lengths, the lanes of a chunked pass, the way back of the total words
// and of result_start.  Included after ../csrc/api_internal.hpp; everything is inline or a template (no object of its own).  The
// searches that host and device share are ragged.hpp (included here), the workgroup-wide device steps block.hpp, the order stage
// of the four approximate searches result_order.hpp.  DESIGN.md "Shared host plumbing" says what belongs where.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

#include "ragged.hpp"

namespace femto_amd {

// ---- handles --------------------------------------------------------------------------------------------------------------------

// `what` is the subject with its verb: "document listing is", "positional operators are"
inline int check_plain_handle(femto_amd_index* ix, const char* what) {
  if (ix->split_parts > 0) return set_err(FEMTO_AMD_ERR_INVALID, std::string(what) + " not available on a range-split part");
  if (!ix->striped.empty() || ix->borrowed || ix->imported)
    return set_err(FEMTO_AMD_ERR_INVALID, std::string(what) + " not available on a striped handle");
  return ensure_device(ix);
}

// host forms of a multi-device handle run on replica 0 ...
inline femto_amd_index* replica0(femto_amd_index* ix0) { return ix0->children.empty() ? ix0 : ix0->children[0]; }
// ... device forms refuse it
inline int refuse_multi_device() {
  return set_err(FEMTO_AMD_ERR_INVALID, "device-pointer calls are not available on a multi-device handle");
}
// the handle of a device form: one device, and plain
inline int check_device_handle(femto_amd_index* ix, const char* what) {
  if (!ix->children.empty()) return refuse_multi_device();
  return check_plain_handle(ix, what);
}

// the handle's device copy of doc_ends, made on first use (resolve.hip, doclist.hip).  The fast path takes no lock --
// femto_amd_resolve_device is an enqueue-only call issued every step: the pointer is published with release order once the
// table is complete
inline int ensure_doc_ends(femto_amd_index* ix) {
  if (__atomic_load_n(&ix->d_doc_ends, __ATOMIC_ACQUIRE)) return 0;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->d_doc_ends) return 0;
  const size_t n = ix->host.doc_ends.size();
  int64_t* p = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * 8));
  if (n) {
    const hipError_t e = hipMemcpy(p, ix->host.doc_ends.data(), n * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return set_err(FEMTO_AMD_ERR_INVALID, std::string("hipMemcpy(doc_ends): ") + hipGetErrorString(e));
    }
  }
  __atomic_store_n(&ix->d_doc_ends, p, __ATOMIC_RELEASE);
  ix->table_bytes += int64_t(n * 8);
  ix->hbm_held += int64_t(n * 8);
  return 0;
}

// ---- arguments of a host form -----------------------------------------------------------------------------------------------------

// n patterns, pattern i = pats[starts[i] .. starts[i] + plen[i]): *nsyms = the extent of the symbols they address
inline int check_patterns(int64_t n, const int32_t* plen, const uint16_t* pats, const int64_t* starts, int64_t* nsyms) {
  *nsyms = 0;
  for (int64_t i = 0; i < n; i++) {
    if (plen[i] < 0 || starts[i] < 0) return set_err(FEMTO_AMD_ERR_PARAM, "negative pattern length or start");
    for (int32_t j = 0; j < plen[i]; j++)
      if (pats[starts[i] + j] >= FEMTO_AMD_ALPHA_SIZE) return set_err(FEMTO_AMD_ERR_PARAM, "character code >= ALPHA_SIZE in a pattern");
    *nsyms = std::max(*nsyms, starts[i] + plen[i]);
  }
  return FEMTO_AMD_OK;
}

// npat patterns given by their lengths alone, one behind the other: (*starts)[i] = the first symbol of pattern i, (*starts)[npat] =
// the symbols in all.  `message` refuses a length outside min_len .. max_len
inline int pattern_starts(int64_t npat, const int32_t* plen, int32_t min_len, int32_t max_len, const char* message, std::vector<int64_t>* starts) {
  starts->assign(size_t(npat) + 1, 0);
  for (int64_t i = 0; i < npat; i++) {
    if (plen[i] < min_len || plen[i] > max_len) return set_err(FEMTO_AMD_ERR_PARAM, message);
    (*starts)[size_t(i) + 1] = (*starts)[size_t(i)] + plen[i];
  }
  return FEMTO_AMD_OK;
}

// n pairs of lists, a = [a_start[k], a_start[k] + a_n[k]) and b likewise: *la, *lb = the extents of the two element arrays
inline int check_list_pairs(int64_t n, const int64_t* a_start, const int32_t* a_n, const int64_t* b_start, const int32_t* b_n, int64_t* la,
                            int64_t* lb) {
  *la = *lb = 0;
  for (int64_t k = 0; k < n; k++) {
    if (a_start[k] < 0 || b_start[k] < 0 || a_n[k] < 0 || b_n[k] < 0) return set_err(FEMTO_AMD_ERR_PARAM, "negative list start or length");
    *la = std::max(*la, a_start[k] + a_n[k]);
    *lb = std::max(*lb, b_start[k] + b_n[k]);
  }
  return FEMTO_AMD_OK;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------

// one checked launch of 256-thread workgroups; the call itself converts T* to the kernel's const T*
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, hipStream_t st, A... args) {
  kernel<<<grid, dim3(256), 0, st>>>(args...);
  HIP_TRY(hipGetLastError());
  return FEMTO_AMD_OK;
}

// the grid of a kernel with one thread per element: ceil(n / 256) workgroups for n elements ...
inline dim3 blocks_of(int64_t n) { return dim3(uint32_t((n + 255) / 256)); }
// ... and (one more than ceil) for the kernels that write n + 1
inline dim3 blocks_for(int64_t n) { return dim3(uint32_t((n + 256) / 256)); }

// blocks of a grid that strides over `items` units of work: at most eight per CU, at least one
inline dim3 persistent_grid(const femto_amd_index* ix, int64_t items) {
  return dim3(uint32_t(std::max<int64_t>(1, std::min(items, int64_t(ix->num_cus) * 8))));
}

// lanes per launch of a pass that may need more than the 2^32 work-items of one launch: `cap`, a multiple of the 256 of a workgroup,
// or what the environment says (test hook: more than one launch on small batches), rounded down to whole workgroups
inline int64_t lane_chunk(const char* env_name, int64_t cap) {
  if (const char* e = getenv(env_name)) return std::max<int64_t>(256, std::min<int64_t>(cap, atoll(e)) & ~int64_t(255));
  return cap;
}

// the answer of a device form to a call with no jobs: res_starts[0] = 0 and the total words zero -- two, {0, 0}, where the caller
// has no more (hamming.hip has four, leven.hip five)
inline int empty_result_async(int64_t* d_starts, int64_t* d_total, hipStream_t st, int words = 2) {
  HIP_TRY(hipMemsetAsync(d_starts, 0, 8, st));
  HIP_TRY(hipMemsetAsync(d_total, 0, size_t(words) * 8, st));
  return FEMTO_AMD_OK;
}

// ---- device memory of a blocking host form, freed on every exit path ------------------------------------------------------------

struct Temp {
  std::vector<void*> ptrs;
  DeviceBuffer scan[3];        // device_scan's tile sums
  ~Temp() {
    for (void* p : ptrs) (void)hipFree(p);
    for (DeviceBuffer& b : scan) b.release();
  }
  template <class T> int get(T** out, size_t count) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, (count ? count : 1) * sizeof(T)));
    ptrs.push_back(p);
    *out = static_cast<T*>(p);
    return 0;
  }
  // get() and the upload of `count` elements
  template <class T> int put(T** out, const T* host, size_t count) {
    int rc = get(out, count);
    if (rc) return rc;
    if (count) HIP_TRY(hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  template <class T> int put(T** out, const std::vector<T>& v) { return put(out, v.data(), v.size()); }
};

// ---- patterns -> rows -----------------------------------------------------------------------------------------------------------

// `count` symbols from `src` to symbol `at` of the batch's symbol array
struct SymRun {
  const uint16_t* src;
  int64_t count, at;
};

// The device copies of a batch of n patterns.  *d_pats addresses an array of nsyms symbols filled from `runs`; it stands 8
// symbols into a zeroed buffer of nsyms + 16, so that the count kernels may read 16 bytes on either side of any pattern.
inline int upload_patterns(Temp& T, int64_t n, const int32_t* plen, const int64_t* starts, int64_t nsyms, std::initializer_list<SymRun> runs,
                           int32_t** d_plen, uint16_t** d_pats, int64_t** d_starts) {
  int rc;
  uint16_t* buf;
  if ((rc = T.put(d_plen, plen, size_t(n))) || (rc = T.get(&buf, size_t(nsyms) + 16))) return rc;
  HIP_TRY(hipMemset(buf, 0, (size_t(nsyms) + 16) * 2));
  for (const SymRun& r : runs)
    if (r.count) HIP_TRY(hipMemcpy(buf + 8 + r.at, r.src, size_t(r.count) * 2, hipMemcpyHostToDevice));
  *d_pats = buf + 8;
  return T.put(d_starts, starts, size_t(n));
}

// what locate_rows leaves on the device: pattern i's rows are offs[ostarts[i] .. ostarts[i + 1]); tot = {rows, 0}
struct LocatedRows {
  int64_t *first, *last, *ostarts, *offs, *tot;
  int32_t* noccs;
  int64_t rows;
};

// The rows parallel_locate returns for np uploaded patterns (femto_amd_locate_plan_device + _walk_device on the null stream): the
// row total is read back to size the buffer.  The last copy is a blocking one; the walk may still be running when this returns.
inline int locate_rows(femto_amd_index* ix, Temp& T, int64_t np, const int32_t* d_plen, const uint16_t* d_pats, const int64_t* d_starts,
                       int max_occs_each, LocatedRows* R) {
  int rc;
  if ((rc = T.get(&R->first, size_t(np))) || (rc = T.get(&R->last, size_t(np))) || (rc = T.get(&R->noccs, size_t(np))) ||
      (rc = T.get(&R->ostarts, size_t(np) + 1)) || (rc = T.get(&R->tot, 2)))
    return rc;
  if ((rc = femto_amd_locate_plan_device(ix, np, d_plen, d_pats, d_starts, max_occs_each, R->first, R->last, R->noccs, R->ostarts, nullptr)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  R->rows = 0;
  HIP_TRY(hipMemcpy(&R->rows, R->ostarts + np, 8, hipMemcpyDeviceToHost));
  if ((rc = T.get(&R->offs, size_t(R->rows)))) return rc;
  if (R->rows && (rc = femto_amd_locate_walk_device(ix, np, R->first, R->ostarts, R->rows, R->offs, nullptr))) return rc;
  const int64_t tot2[2] = {R->rows, 0};
  HIP_TRY(hipMemcpy(R->tot, tot2, 16, hipMemcpyHostToDevice));
  return 0;
}

// ---- results -> host ------------------------------------------------------------------------------------------------------------

// one malloc()ed array of n > 0 elements from a device array of a finished run on `st`; `what` opens the message of a failed copy.
// wait = false only enqueues the copy: the next wait on `st` completes it, and the caller frees *out should that wait fail
template <class T>
int list_to_host(int64_t n, const T* d_src, hipStream_t st, const char* what, T** out, bool wait = true) {
  T* h = static_cast<T*>(malloc(size_t(n) * sizeof(T)));
  if (!h) return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  hipError_t e = hipMemcpyAsync(h, d_src, size_t(n) * sizeof(T), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && wait) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    free(h);
    return set_err(FEMTO_AMD_ERR_INVALID, std::string(what) + ": " + hipGetErrorString(e));
  }
  *out = h;
  return FEMTO_AMD_OK;
}

// n int64 words of a finished run on `st` (the total words of a device form) into `host`, waited for; `message` is the failure's
inline int words_to_host(int64_t n, const int64_t* d_src, hipStream_t st, const char* message, int64_t* host) {
  if (hipMemcpyAsync(host, d_src, size_t(n) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return set_err(FEMTO_AMD_ERR_INVALID, message);
  return FEMTO_AMD_OK;
}

// the npat + 1 words of result_start into the host form's array; the wait completes the copies enqueued before it (list_to_host)
inline int result_start_to_host(int64_t npat, const int64_t* d_result_start, hipStream_t st, int64_t* result_start) {
  return words_to_host(npat + 1, d_result_start, st, "copying the results back failed", result_start);
}

// the two malloc()ed arrays of a result of n > 0 (document, offset) pairs, with one wait for both copies; on failure nothing is
// handed out and *total is reset
inline int pairs_to_host(int64_t n, const int64_t* d_rd, const int64_t* d_ro, hipStream_t st, int64_t** res_doc, int64_t** res_off,
                         int64_t* total) {
  int rc = list_to_host(n, d_rd, st, "copying the results back", res_doc, false);
  if (rc == FEMTO_AMD_OK && (rc = list_to_host(n, d_ro, st, "copying the results back", res_off))) {
    free(*res_doc);
    *res_doc = nullptr;
  }
  if (rc) *total = 0;
  return rc;
}

// res_starts, *total and the result arrays of a host form
inline int copy_pairs_back(int64_t npairs, const int64_t* d_rs, const int64_t* d_rd, const int64_t* d_ro, hipStream_t st, int64_t* res_starts,
                           int64_t** res_doc, int64_t** res_off, int64_t* total) {
  HIP_TRY(hipMemcpyAsync(res_starts, d_rs, size_t(npairs + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t n = res_starts[npairs];
  *total = n;
  if (n == 0) return FEMTO_AMD_OK;
  return pairs_to_host(n, d_rd, d_ro, st, res_doc, res_off, total);
}

}  // namespace femto_amd
