// host_common.hpp -- the host plumbing that doclist.hip, docpos.hip, bquery.hip and extract.hip share: the handle checks, the
// device memory of a blocking host form, the upload of a pattern batch and the rows it locates, the copy of a pairs result back
// to the host, the size of a persistent grid.  Included after ../csrc/api_internal.hpp; everything is inline or a template
// (no object of its own).  DESIGN.md "Shared host plumbing" says what belongs here.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

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

// the handle's device copy of doc_ends.  Mirrors the static ensure_doc_ends of ../csrc/resolve.hip: the same table, lock and
// publication, so whichever call comes first makes it (one of the two can go once resolve.hip may include this header)
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

// ---- launches -------------------------------------------------------------------------------------------------------------------

// blocks of a grid that strides over `items` units of work: at most eight per CU, at least one
inline int64_t persistent_grid(const femto_amd_index* ix, int64_t items) {
  return std::max<int64_t>(1, std::min(items, int64_t(ix->num_cus) * 8));
}

// the answer of a device form to a call with no jobs: res_starts[0] = 0 and the two-word total {0, 0}
inline int empty_result_async(int64_t* d_starts, int64_t* d_total, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(d_starts, 0, 8, st));
  HIP_TRY(hipMemsetAsync(d_total, 0, 16, st));
  return FEMTO_AMD_OK;
}

#ifdef __HIPCC__
// the last k in [0, n) with starts[k] <= p   (0 <= p < starts[n]): the segment of a ragged array that element p belongs to
__device__ __forceinline__ int64_t last_start_le(const int64_t* __restrict__ starts, int64_t n, int64_t p) {
  int64_t lo = 1, hi = n;      // the first index with starts[index] > p lies in [1, n]
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (starts[m] <= p) lo = m + 1; else hi = m;
  }
  return lo - 1;
}
#endif

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

// the two malloc()ed arrays of a result of n > 0 (document, offset) pairs, from the device arrays of a finished run on `st`;
// on failure nothing is handed out and *total is reset
inline int pairs_to_host(int64_t n, const int64_t* d_rd, const int64_t* d_ro, hipStream_t st, int64_t** res_doc, int64_t** res_off,
                         int64_t* total) {
  int64_t* hd = static_cast<int64_t*>(malloc(size_t(n) * 8));
  int64_t* ho = static_cast<int64_t*>(malloc(size_t(n) * 8));
  hipError_t e = hipSuccess;
  if (hd && ho) {
    e = hipMemcpyAsync(hd, d_rd, size_t(n) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ho, d_ro, size_t(n) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (!hd || !ho || e != hipSuccess) {
    free(hd);
    free(ho);
    *total = 0;
    if (e != hipSuccess) return set_err(FEMTO_AMD_ERR_INVALID, std::string("copying the results back: ") + hipGetErrorString(e));
    return set_err(FEMTO_AMD_ERR_MEM, "out of memory");
  }
  *res_doc = hd;
  *res_off = ho;
  return FEMTO_AMD_OK;
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
