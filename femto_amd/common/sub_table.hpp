// sub_table.hpp -- what ../mismatch/mismatch.hip, ../edit/edit.hip and ../classes/classes.hip share: the table of the byte characters
// of the text that a substitution or an insertion may use (classes.hip keeps one of its shape per class: the members that occur), the
// code of a pattern symbol in the handle's rank layout, and the bounds of the byte characters (kByte0, kAlpha).  (The bits of a sort key
// stand with the sorts, in result_order.hpp.)
// Device and host; included after ../csrc/kernels.hip.hpp (DevIndex) and block.hpp (block_rank).
#pragma once
#include <cstdint>

namespace femto_amd {

constexpr uint32_t kAlpha = uint32_t(FEMTO_AMD_ALPHA_SIZE), kByte0 = uint32_t(FEMTO_AMD_CHARACTER_OFFSET);

// the byte characters of the text in character order: alpha code | code in the rank layout << 16
struct SubTable {
  uint32_t pair[256];
  int32_t n;
};

template <class P>
__device__ __forceinline__ uint32_t code_or_none(const DevIndex& ix, uint32_t ch) {
  return ch < kAlpha ? P::code_of(ix, ch) : 0xffffu;
}

template <class P>
__global__ __launch_bounds__(256) void sub_table_kernel(const DevIndex ix, SubTable* __restrict__ tab) {
  __shared__ int s_wave[4];
  const uint32_t ch = threadIdx.x + kByte0;
  const bool have = ix.C[ch + 1] > ix.C[ch];
  const uint32_t code = have ? uint32_t(P::code_of(ix, ch)) & 0xffffu : 0xffffu;
  int count;
  const int r = block_rank(have, s_wave, &count);
  if (have) tab->pair[r] = ch | (code << 16);
  if (threadIdx.x == 0) tab->n = count;
}

}  // namespace femto_amd
