// plan_span.hpp -- which 256-pattern tiles a wavefront of plan_stream_kernel owns, and how many workgroups the launch has.
// Plain arithmetic, callable from the host and the device: tests/plan_span_check.cpp runs it on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLAN_SPAN_FN __host__ __device__ inline
#else
#define PLAN_SPAN_FN inline
#endif

namespace femto_amd {

constexpr int kPlanTile = 256;           // patterns per tile = count_direct_kernel's block: PlanSums::sums[] has one word per tile
constexpr int kPlanWavesPerGroup = 4;    // 256 threads
constexpr int kPlanGroupsPerCu = 8;      // W: the automatic grid is num_cus x W workgroups (profiles/plan_stream_stats.txt)

struct PlanSpan {
  int64_t t0, t1;      // tiles [t0, t1); t0 == t1: the wavefront owns none
};

PLAN_SPAN_FN int64_t plan_tiles(int64_t npats) { return npats <= 0 ? 0 : (npats + kPlanTile - 1) / kPlanTile; }

// Every wavefront owns ONE contiguous run of ceil(ntiles / nwaves) tiles (the last owner's run may be shorter, the wavefronts
// after it own nothing): the running row count is carried in a register from tile to tile, and only a run's first tile
// needs the sums of the tiles before it.
PLAN_SPAN_FN PlanSpan plan_span_of(int64_t ntiles, int64_t nwaves, int64_t wave) {
  if (ntiles <= 0 || nwaves <= 0 || wave < 0 || wave >= nwaves) return PlanSpan{0, 0};
  const int64_t per = (ntiles + nwaves - 1) / nwaves;
  // wave * per cannot overflow: wave < nwaves and per <= ntiles / nwaves + 1, so the product is below ntiles + nwaves
  const int64_t t0 = wave * per;
  if (t0 >= ntiles) return PlanSpan{ntiles, ntiles};
  const int64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
  return PlanSpan{t0, t1};
}

// the wavefront that owns the last tile (it publishes the total)
PLAN_SPAN_FN int64_t plan_last_owner(int64_t ntiles, int64_t nwaves) {
  if (ntiles <= 0 || nwaves <= 0) return -1;
  const int64_t per = (ntiles + nwaves - 1) / nwaves;
  return (ntiles - 1) / per;
}

// workgroups of the launch: one per tile until the device is full (num_cus x kPlanGroupsPerCu), then the wavefronts loop.
// `forced` > 0 (FEMTO_AMD_PLAN_STREAM_GRID, tests): that many, still at most one per tile.
PLAN_SPAN_FN int64_t plan_stream_groups(int64_t ntiles, int64_t num_cus, int64_t forced) {
  if (ntiles <= 0) return 0;
  int64_t g = forced > 0 ? forced : (num_cus > 0 ? num_cus : 1) * kPlanGroupsPerCu;
  if (g > ntiles) g = ntiles;
  if (g > 0x7fffffffLL) g = 0x7fffffffLL;
  return g;
}

}  // namespace femto_amd
