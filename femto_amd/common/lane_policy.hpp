// lane_policy.hpp -- the rank policy of handles in rank modes 0 / 1 for kernels that give every search ONE lane
// (../similar/similar.hip, ../mismatch/mismatch.hip): femto's own wavelet tree over the derived segment lines, the step of
// regexp_search.hip's WavePolicy.  Device only; included after ../csrc/kernels.hip.hpp (c_plus_occ_lane, DevIndex).  It has no
// KindOf: with_policy<...> serves the five derived layouts, and the caller launches this one when none of them applies and the
// handle has the derived segment lines (host.dir_regular).
#pragma once
#include <cstdint>

namespace femto_amd {

struct LanePolicy {
  static constexpr int kDirectWaves = 7;      // 67 VGPRs
  static __device__ __forceinline__ void search_step(const DevIndex& ix, int, uint32_t ch, int64_t& f, int64_t& l) {
    const int64_t nf = f == 0 ? ix.C[ch] : c_plus_occ_lane(ix, ch, f - 1);
    const int64_t nl = c_plus_occ_lane(ix, ch, l) - 1;
    f = nf;
    l = nl;
  }
  static __device__ __forceinline__ uint32_t code_of(const DevIndex& ix, uint32_t ch) { return ix.C[ch + 1] > ix.C[ch] ? ch : 0xffffu; }
};

}  // namespace femto_amd
