// lane_policy.hpp -- the rank policy of handles in rank modes 0 / 1 for kernels that give every search ONE lane
// (../similar/similar.hip, ../mismatch/mismatch.hip, ../edit/edit.hip, ../classes/classes.hip): femto's own wavelet tree over the
// derived segment lines, the step of regexp_search.hip's WavePolicy -- and with_lane_policy, the dispatch of such a kernel over the
// policy of a handle.  Included after ../csrc/api_internal.hpp and the kernel headers of the five derived layouts
// (c_plus_occ_lane, DevIndex, the policy structs).  LanePolicy has no KindOf: with_policy<...> serves the five derived layouts, and
// this one is launched when none of them applies and the handle has the derived segment lines (host.dir_regular).
#pragma once
#include <cstdint>
#include <string>

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

// go(Tag<P>{}) for the rank policy P of `ix`, and what it returns.  `what_needs` opens the refusal of a handle that has neither a
// derived layout nor the derived segment lines: "matching statistics on this handle need"
template <class F>
int with_lane_policy(femto_amd_index* ix, const char* what_needs, F&& go) {
  int rc = FEMTO_AMD_OK;
  auto call = [&](auto tag) { rc = go(tag); };
  if (with_policy<RumPolicy, RuPolicy, PackPolicy, IndPolicy, Pack2Policy>(rank_kind(ix->mode, ix->dev), call)) return rc;
  if (!ix->host.dir_regular) return set_err(FEMTO_AMD_ERR_INVALID, std::string(what_needs) + " the derived segment lines");
  call(Tag<LanePolicy>{});
  return rc;
}

}  // namespace femto_amd
