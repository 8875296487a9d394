// result_order.hpp -- the order stage that ../mismatch/mismatch.hip, ../edit/edit.hip, ../classes/classes.hip,
// ../hamming/hamming.hip and ../leven/leven.hip share.  Their lanes emit records in any order, into the slots below a capacity; the
// answer lists them by pattern and, within a pattern, by a key of the record (its first row, its offset; for edit.hip
// first << 5 | length and cost, for leven.hip offset << 11 | cost and length).
// Two stable radix sorts (rocPRIM) of the records' INDEXES do it: by the record's key, then by pattern.  The slots behind the live
// records take part in both sorts with a key that sorts behind every record: the caller's `dead` key in the first, npat in the
// second -- which is why the pattern keys are sorted over the bits of npat, one more than the largest pattern number needs when
// npat is a power of two.  What the caller does with the sorted indexes (its gather, edit.hip's heads) is its own.
// Device and host; included after host_common.hpp (launch, blocks_of) and block.hpp; no object of its own.
#pragma once
#include <algorithm>
#include <cstdint>

#include <rocprim/rocprim.hpp>

namespace femto_amd {

inline int bits_of(int64_t v) {      // bits that hold every value in [0, v]
  int b = 1;
  while (b < 63 && (int64_t(1) << b) <= v) b++;
  return b;
}

// the slots that hold a record: *total_word counts every emit, whether its record found a slot or not
__device__ __forceinline__ int64_t live_records(const unsigned long long* total_word, int64_t capacity) {
  const int64_t t = int64_t(*total_word);
  return t < capacity ? t : capacity;
}

// the key of a record that is one int64 column of it (a row, an offset: never negative)
struct ColumnKey {
  const int64_t* column;
  __device__ __forceinline__ uint64_t operator()(int64_t slot) const { return uint64_t(column[slot]); }
};

// keys[s] = key(s) and idx[s] = s; slots behind the live ones sort behind every record
template <class Key>
inline __global__ __launch_bounds__(256) void first_key_kernel(const Key key, const unsigned long long* __restrict__ total_word, const int64_t capacity,
                                                               const uint64_t dead, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= capacity) return;
  keys[s] = s < live_records(total_word, capacity) ? key(s) : dead;
  idx[s] = uint32_t(s);
}

// ... and behind every pattern
inline __global__ __launch_bounds__(256) void pattern_key_kernel(const uint32_t* __restrict__ pat, const int64_t npat,
                                                                 const unsigned long long* __restrict__ total_word, const int64_t capacity,
                                                                 const uint32_t* __restrict__ idx, uint32_t* __restrict__ keys) {
  const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (s >= capacity) return;
  keys[s] = s < live_records(total_word, capacity) ? pat[idx[s]] : uint32_t(npat);
}

// the buffers of the two sorts: Scratch's (api_internal.hpp) or a work area's of the caller
struct OrderBuffers {
  DeviceBuffer &keys, &keys2, &idx, &idx2, &pk, &pk2, &sorttmp;
};

// what order_records leaves: idx[s] = the slot of the s-th record in the final order, pattern_keys[s] = its pattern (npat behind the
// live records); both `capacity` long
struct Ordered {
  const uint32_t* idx;
  const uint32_t* pattern_keys;
};

// The records of slots [0, capacity), capacity > 0, by (pat, key), enqueued on `st`.  key_bits: the bits that hold every key and
// `dead`.  The buffers are reserved HERE, behind the search kernels the caller has enqueued, and the caller's record buffers in
// front of them: DeviceBuffer::reserve frees before it allocates and hipFree waits for the device, so a buffer that grows here
// waits while the search runs, not in front of it.  A caller that wants a buffer larger than a sort needs (edit.hip's keys2)
// reserves it just before the call; the reserve below is then a no-op.
template <class Key>
int order_records(const OrderBuffers& B, const unsigned long long* total_word, int64_t capacity, const uint32_t* pat, int64_t npat, Key key,
                  unsigned key_bits, uint64_t dead, hipStream_t st, Ordered* out) {
  const size_t cap = size_t(capacity);
  const unsigned pat_bits = unsigned(std::min(32, bits_of(npat)));
  int rc;
  size_t tmp1 = 0, tmp2 = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp1, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                    static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), cap, 0u, key_bits, st));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp2, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                    static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), cap, 0u, pat_bits, st));
  const size_t tmp = std::max(tmp1, tmp2);
  if ((rc = B.keys.reserve(cap * 8)) || (rc = B.keys2.reserve(cap * 8)) || (rc = B.idx.reserve(cap * 4)) || (rc = B.idx2.reserve(cap * 4)) ||
      (rc = B.pk.reserve(cap * 4)) || (rc = B.pk2.reserve(cap * 4)) || (rc = B.sorttmp.reserve(tmp ? tmp : 16)))
    return rc;
  uint32_t *idx = B.idx.as<uint32_t>(), *idx2 = B.idx2.as<uint32_t>(), *pk = B.pk.as<uint32_t>(), *pk2 = B.pk2.as<uint32_t>();
  // by key, then (stable) by pattern
  if ((rc = launch(first_key_kernel<Key>, blocks_of(capacity), st, key, total_word, capacity, dead, B.keys.as<uint64_t>(), idx))) return rc;
  HIP_TRY(rocprim::radix_sort_pairs(B.sorttmp.p, tmp1, B.keys.as<uint64_t>(), B.keys2.as<uint64_t>(), idx, idx2, cap, 0u, key_bits, st));
  if ((rc = launch(pattern_key_kernel, blocks_of(capacity), st, pat, npat, total_word, capacity, idx2, pk))) return rc;
  HIP_TRY(rocprim::radix_sort_pairs(B.sorttmp.p, tmp2, pk, pk2, idx2, idx, cap, 0u, pat_bits, st));
  *out = Ordered{idx, pk2};
  return FEMTO_AMD_OK;
}

}  // namespace femto_amd
