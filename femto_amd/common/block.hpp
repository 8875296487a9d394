// block.hpp -- the workgroup-wide steps that the kernels of doclist.hip and docpos.hip share; device only, for workgroups of 256
// threads (four wavefronts).  DESIGN.md "Shared host plumbing" says what belongs here.
#pragma once
#include <cstdint>

namespace femto_amd {

// the sum of `part` over the block's 256 threads, in every thread; s_sum: 256 words of LDS, free again after the next barrier
__device__ __forceinline__ int64_t block_sum_i64(int64_t part, int64_t* s_sum) {
  s_sum[threadIdx.x] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    __syncthreads();
  }
  return s_sum[0];
}

// exclusive rank of `flag` among the block's threads (thread order) and the block's count; s_wave: 4 words; two barriers
__device__ __forceinline__ int block_rank(bool flag, int* s_wave, int* count) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  __syncthreads();        // (s_wave of the previous round has been read)
  if (lane == 0) s_wave[w] = __popcll(m);
  __syncthreads();
  int base = 0, all = 0;
  for (int k = 0; k < 4; k++) {
    const int c = s_wave[k];
    if (k < w) base += c;
    all += c;
  }
  *count = all;
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

// the two-word answer of a device form: {total, total > capacity}
__device__ __forceinline__ void write_total(int64_t* res_total, int64_t total, int64_t capacity) {
  res_total[0] = total;
  res_total[1] = total > capacity ? 1 : 0;
}

}  // namespace femto_amd
