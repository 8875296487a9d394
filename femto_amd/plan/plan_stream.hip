// plan_stream.hip -- femto_amd_locate_device_v2: the one-call device chain with a STREAMING row plan.
//
// After count_direct_kernel the chain needs out_starts[] (the exclusive prefix sum of noccs[]) and the located offsets.
// plan_rows_kernel<kRowsSa> (csrc/direct_kernels.hip.hpp) does that with one four-wave workgroup per 256 patterns: 39 063
// short workgroups for the headline's 10 M patterns, each a chain of dependent steps (three sum loads, a wave reduction,
// LDS, a barrier, a second scan, LDS, a second barrier) around 1 KB in and 2 KB out.  It ran at about a third of the rate
// its 120 MB can be streamed at, and the idle plan_big_rows_kernel behind it cost a third launch per step.
//
// plan_stream_kernel is a persistent grid instead.  Every WAVEFRONT owns a contiguous run of 256-pattern tiles
// (plan_span.hpp), computes the rows before its first tile once from the PlanSums the count kernel left (final when this
// kernel starts: nothing is waited for across wavefronts or workgroups), and then carries the running base in a register:
// per tile one 16-byte load of four noccs per lane, a 4-element local prefix, one wave scan, two 16-byte stores of four
// out_starts -- with the loads of the next two tiles in flight.  There is no __syncthreads; the LDS of the row expansion is
// private to the wavefront.  Rows are expanded only in tiles that hold any, cooperatively over the tile's 256 patterns:
// consecutive lanes write consecutive slots and read consecutive suffix-array entries, as plan_rows_kernel does over 64.
// Every output is bit-identical to plan_rows_kernel<kRowsSa>'s (tests/test_gpu_plan_stream.py).
//
// Ranges longer than kExpandSerialMax can only exist when max_occs allows them; only then does the kernel test for them
// (kLong) and is plan_big_rows_kernel launched behind it.  With max_occs <= kExpandSerialMax the step is two launches.
//
// The old entry point and its kernels stay as they are (the round-6 profiles describe them); the next profile round may
// fold this launch into csrc.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "../csrc/api_internal.hpp"
#include "../csrc/kernels.hip.hpp"
#include "../csrc/pack_kernels.hip.hpp"
#include "../csrc/ru_kernels.hip.hpp"
#include "../csrc/pack2_kernels.hip.hpp"
#include "../csrc/ind_kernels.hip.hpp"
#include "../csrc/text_kernels.hip.hpp"
#include "../csrc/ctx_kernels.hip.hpp"
#include "../csrc/direct_kernels.hip.hpp"
#include "plan_span.hpp"

namespace femto_amd {
namespace {

struct alignas(16) I64x2 { int64_t x, y; };

// LDS writes of this wavefront become visible to its other lanes (and reads are done before the next tile's writes)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// four consecutive noccs of tile t for this lane (patterns t * 256 + 4 * lane ..); 0 beyond npats or beyond the run
__device__ __forceinline__ int4 load_counts(const int32_t* __restrict__ noccs, int64_t npats, int64_t t, int64_t t1, int lane) {
  int4 v = make_int4(0, 0, 0, 0);
  if (t >= t1) return v;
  const int64_t q0 = t * kPlanTile + 4 * lane;
  if (q0 + 4 <= npats) {
    v = *reinterpret_cast<const int4*>(noccs + q0);      // noccs is 16-byte aligned (the entry point checks)
  } else {
    if (q0 < npats) v.x = noccs[q0];
    if (q0 + 1 < npats) v.y = noccs[q0 + 1];
    if (q0 + 2 < npats) v.z = noccs[q0 + 2];
  }
  return v;
}

// a[q0 .. q0 + 3] where need[j]; as two 16-byte loads when the quad is whole and `a` is 16-byte aligned (entries that are
// not needed are then read and ignored: they lie inside the array)
__device__ __forceinline__ void load_quad(const int64_t* __restrict__ a, bool vec, int64_t q0, const bool need[4], int64_t out[4]) {
  if (vec) {
    const I64x2 lo = *reinterpret_cast<const I64x2*>(a + q0), hi = *reinterpret_cast<const I64x2*>(a + q0 + 2);
    out[0] = lo.x; out[1] = lo.y; out[2] = hi.x; out[3] = hi.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = need[j] ? a[q0 + j] : 0;
  }
}

// kLong: max_occs > kExpandSerialMax, a range may be too long for the cooperative expansion (plan_big_rows_kernel's work)
// Occupancy: eight waves per SIMD (64 VGPRs) -- the suffix-array gathers of dense batches live on memory-level parallelism;
// the kLong form needs a few registers more and is allowed down to six rather than spill.
template <bool kLong>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kLong ? 6 : 8, 8))) void plan_stream_kernel(
    const int64_t npats, const int32_t* __restrict__ noccs, const int64_t* __restrict__ first, const PlanSums ps,
    int64_t* __restrict__ out_starts, int64_t* __restrict__ offsets, const int64_t capacity, int* __restrict__ big_flag,
    const DevIndex ix, int64_t* __restrict__ total_out, int64_t* __restrict__ total_user, const int64_t* __restrict__ sa_known) {
  // wave-private LDS of the row expansion: inclusive row counts of the tile's patterns (long ranges count 0), what each
  // pattern's rows start from (a row, or ~position), and -- kLong only -- where its slots start relative to the tile
  __shared__ uint32_t s_incl[kPlanWavesPerGroup][kPlanTile];
  __shared__ int64_t s_first[kPlanWavesPerGroup][kPlanTile];
  __shared__ int64_t s_lrel[kLong ? kPlanWavesPerGroup : 1][kLong ? kPlanTile : 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nwaves = int64_t(gridDim.x) * kPlanWavesPerGroup, wave = int64_t(blockIdx.x) * kPlanWavesPerGroup + wv;
  // the set of group sums the NEXT launch accumulates into starts at zero
  for (int64_t k = wave * 64 + lane; k < ps.next_words; k += nwaves * 64) ps.next_super[k] = 0;
  const PlanSpan span = plan_span_of(ps.nblocks, nwaves, wave);
  if (span.t0 >= span.t1) return;
  int4 cur = load_counts(noccs, npats, span.t0, span.t1, lane);
  int4 nx1 = load_counts(noccs, npats, span.t0 + 1, span.t1, lane);
  // rows before the run: the groups before its first tile's group + the tiles before it inside the group (plan_rows_kernel's sum)
  int64_t base;
  {
    const int64_t b = span.t0, g = b >> 6;
    uint64_t acc = lane < int(b & 63) ? uint64_t(ps.sums[(b & ~int64_t(63)) + lane]) : 0;
    if (lane < int(g & 63)) acc += uint64_t(ps.super[(g & ~int64_t(63)) + lane]);
    for (int64_t k = lane; k < (g >> 6); k += 64) acc += uint64_t(ps.super2[k]);
    const uint64_t part = wave_sum_u64(acc);      // valid in lane 0
    const uint32_t lo = uint32_t(__shfl(int(uint32_t(part)), 0, 64)), hi = uint32_t(__shfl(int(uint32_t(part >> 32)), 0, 64));
    base = int64_t((uint64_t(hi) << 32) | lo);
  }
  const bool first_vec = (reinterpret_cast<uintptr_t>(first) & 15u) == 0, known_vec = (reinterpret_cast<uintptr_t>(sa_known) & 15u) == 0;
  for (int64_t t = span.t0; t < span.t1; t++) {
    const int4 nx2 = load_counts(noccs, npats, t + 2, span.t1, lane);      // two tiles ahead, in flight across this tile's scan
    const int64_t q0 = t * kPlanTile + 4 * lane;
    const int64_t n[4] = {int64_t(cur.x), int64_t(cur.y), int64_t(cur.z), int64_t(cur.w)};
    // exclusive prefix inside the lane, inclusive scan of the lane sums over the wavefront
    // (kLong: a tile's rows are <= 256 * (2^31 - 1): 64 bits; otherwise <= 256 * kExpandSerialMax = 2^20)
    const int64_t lsum = n[0] + n[1] + n[2] + n[3];
    int64_t incl = lsum;
    if (kLong) {
      uint64_t v = uint64_t(lsum);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64)), hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
        if (lane >= d) v += (uint64_t(hi) << 32) | lo;
      }
      incl = int64_t(v);
    } else {
      uint32_t v = uint32_t(lsum);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = uint32_t(__shfl_up(int(v), d, 64));
        if (lane >= d) v += y;
      }
      incl = int64_t(v);
    }
    int64_t tile_rows;
    if (kLong) {
      const uint32_t lo = uint32_t(__shfl(int(uint32_t(uint64_t(incl))), 63, 64)), hi = uint32_t(__shfl(int(uint32_t(uint64_t(incl) >> 32)), 63, 64));
      tile_rows = int64_t((uint64_t(hi) << 32) | lo);
    } else {
      tile_rows = int64_t(uint32_t(__shfl(int(uint32_t(incl)), 63, 64)));
    }
    const int64_t rel0 = incl - lsum;      // rows of the tile before this lane's four patterns
    const int64_t s0 = base + rel0, s1 = s0 + n[0], s2 = s1 + n[1], s3 = s2 + n[2];
    if (q0 + 4 <= npats) {
      *reinterpret_cast<I64x2*>(out_starts + q0) = I64x2{s0, s1};      // out_starts is 16-byte aligned (the entry point checks)
      *reinterpret_cast<I64x2*>(out_starts + q0 + 2) = I64x2{s2, s3};
    } else {
      if (q0 < npats) out_starts[q0] = s0;
      if (q0 + 1 < npats) out_starts[q0 + 1] = s1;
      if (q0 + 2 < npats) out_starts[q0 + 2] = s2;
    }
    if (offsets && tile_rows > 0) {      // (wave-uniform) this tile holds rows: expand them
      bool live[4], big[4];
      bool any_big = false;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        big[j] = kLong && n[j] > kExpandSerialMax;
        any_big |= big[j];
        live[j] = q0 + j < npats && !big[j] && n[j] > 0;      // rows this pattern contributes to the cooperative part
      }
      if (kLong && any_big) atomicOr(big_flag, 1);
      // inclusive counts of the cooperative part, per pattern, relative to the tile
      uint32_t mine[4], linc[4], lsum2 = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        mine[j] = live[j] ? uint32_t(n[j]) : 0u;
        lsum2 += mine[j];
        linc[j] = lsum2;
      }
      uint32_t before = uint32_t(rel0);      // without long ranges the cooperative part is everything
      if (kLong) {
        uint32_t v = lsum2;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = uint32_t(__shfl_up(int(v), d, 64));
          if (lane >= d) v += y;
        }
        before = v - lsum2;
      }
      *reinterpret_cast<uint4*>(&s_incl[wv][4 * lane]) = make_uint4(before + linc[0], before + linc[1], before + linc[2], before + linc[3]);
      const uint32_t total = uint32_t(__shfl(int(before + lsum2), 63, 64));
      // what the rows start from: the position the count kernel already knows for a one-row pattern (~position < 0), else the first row
      bool need_known[4], need_first[4], want_known = false, want_first = false;
      int64_t known[4] = {-1, -1, -1, -1}, f[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        need_known[j] = sa_known && mine[j] == 1u;
        want_known |= need_known[j];
      }
      const bool whole = q0 + 4 <= npats;
      if (want_known) load_quad(sa_known, whole && known_vec, q0, need_known, known);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        need_first[j] = mine[j] && !(need_known[j] && known[j] >= 0);      // (only ranges with rows: most of first[] is never touched on a random batch)
        want_first |= need_first[j];
      }
      if (want_first) load_quad(first, whole && first_vec, q0, need_first, f);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!need_first[j]) f[j] = (need_known[j] && known[j] >= 0) ? ~known[j] : 0;
      }
      *reinterpret_cast<I64x2*>(&s_first[wv][4 * lane]) = I64x2{f[0], f[1]};
      *reinterpret_cast<I64x2*>(&s_first[wv][4 * lane + 2]) = I64x2{f[2], f[3]};
      if (kLong) {      // slots are addressed per pattern: a long range keeps its slots but is not written here
        *reinterpret_cast<I64x2*>(&s_lrel[wv][4 * lane]) = I64x2{rel0, rel0 + n[0]};
        *reinterpret_cast<I64x2*>(&s_lrel[wv][4 * lane + 2]) = I64x2{rel0 + n[0] + n[1], rel0 + n[0] + n[1] + n[2]};
      }
      wave_lds_sync();
      for (uint32_t r0 = 0; r0 < total; r0 += 64) {
        const uint32_t sidx = r0 + uint32_t(lane);
        if (sidx < total) {
          int lo = 0, hi = kPlanTile - 1;      // first pattern of the tile whose inclusive count exceeds sidx
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_incl[wv][mid] > sidx) hi = mid; else lo = mid + 1;
          }
          const uint32_t bef = lo ? s_incl[wv][lo - 1] : 0u;
          const int64_t k = int64_t(sidx - bef);
          const int64_t slot = base + (kLong ? s_lrel[wv][lo] : int64_t(bef)) + k;
          if (slot < capacity) {
            const int64_t fr = s_first[wv][lo], row = fr + k;
            if (fr < 0) {
              offsets[slot] = ~fr;
            } else {
              offsets[slot] = sa_at(ix, row);
              trace_touch(ix, kTraceSa, sa_line_of(ix, row));
            }
          }
        }
      }
      wave_lds_sync();
    }
    base += tile_rows;
    cur = nx1;
    nx1 = nx2;
  }
  if (span.t1 == ps.nblocks && lane == 0) {      // the owner of the last tile knows the total
    total_out[0] = base;
    total_out[1] = base > capacity ? 1 : 0;
    if (total_user) {
      total_user[0] = base;
      total_user[1] = base > capacity ? 1 : 0;
    }
    out_starts[npats] = base;
  }
}

// process-wide counters of femto_amd_plan_stream_stats
std::atomic<int64_t> g_streamed{0}, g_fell_back{0}, g_big_launches{0}, g_last_groups{0};

// direct pipeline, after launch_count_plan, kRowsSa: what launch_plan_rows does, with plan_stream_kernel
int launch_plan_stream(femto_amd_index* ix, Scratch& S, int64_t npats, const int32_t* d_noccs, const int64_t* d_first, int64_t* d_out_starts,
                       int64_t* d_offsets, int64_t capacity, hipStream_t stream, const int64_t* d_sa_known, int max_occs, int64_t forced_groups) {
  int* big_flag = S.d_flags + 1;      // cleared by the count kernel
  const int64_t ntiles = plan_tiles(npats);
  const PlanSums ps = plan_sums_at(S.bsums.p, ntiles, false, S.bsums_parity);
  S.bsums_clean = true;
  const dim3 grid{uint32_t(plan_stream_groups(ntiles, ix->num_cus, forced_groups))}, block{uint32_t(kBlockThreads)};
  // noccs <= max_occs: without a clamp above kExpandSerialMax no range is long, the kernel does not look and nothing runs behind it
  const bool may_be_long = int64_t(max_occs) > kExpandSerialMax;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  timer_begin(ix, ix->t_locate, stream, &e0, &e1);
  if (may_be_long) {
    hipLaunchKernelGGL(plan_stream_kernel<true>, grid, block, 0, stream, npats, d_noccs, d_first, ps, d_out_starts, d_offsets, capacity,
                       big_flag, ix->dev, S.d_total, S.total_user, d_sa_known);
    const dim3 bgrid{uint32_t(std::min<int64_t>(ntiles, int64_t(ix->num_cus) * 8))};
    hipLaunchKernelGGL((plan_big_rows_kernel<kRowsSa, PackPolicy>), bgrid, block, 0, stream, npats, d_first, static_cast<const int2*>(nullptr),
                       static_cast<const int64_t*>(d_out_starts), static_cast<const int64_t*>(S.d_total), capacity, d_offsets,
                       static_cast<const int*>(big_flag), ix->dev);
    g_big_launches++;
  } else {
    hipLaunchKernelGGL(plan_stream_kernel<false>, grid, block, 0, stream, npats, d_noccs, d_first, ps, d_out_starts, d_offsets, capacity,
                       big_flag, ix->dev, S.d_total, S.total_user, d_sa_known);
  }
  HIP_TRY(hipGetLastError());
  timer_end(ix, ix->t_locate, stream, e0, e1);
  g_streamed++;
  g_last_groups = int64_t(grid.x);
  return 0;
}

}  // namespace
}  // namespace femto_amd

int femto_amd_locate_device_v2(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen, const uint16_t* d_pats,
                               const int64_t* d_starts, int max_occs_each, int64_t* d_first, int64_t* d_last,
                               int32_t* d_noccs, int64_t* d_out_starts, int64_t* d_offsets, int64_t offsets_capacity,
                               int64_t* d_total, void* stream_) {
  API_BEGIN
  bool direct = false;
  const int rc = locate_chain(
      ix, npats, d_plen, d_pats, d_starts, max_occs_each, d_first, d_last, d_noccs, d_out_starts, d_offsets, offsets_capacity, d_total, stream_,
      [&](Scratch& S, const int64_t* first, const Plan& plan, hipStream_t stream) {
        // The two switches are read from the environment on every call (through knob(), no option field): the handle lives in
        // csrc and has neither a field for them nor a hook at close that would keep a table keyed by the handle from going stale.
        const bool aligned = ((reinterpret_cast<uintptr_t>(d_noccs) | reinterpret_cast<uintptr_t>(d_out_starts)) & 15u) == 0;
        const bool streamed = d_offsets && ix->dev.sa_full && aligned && npats > 0 && knob(-1, "FEMTO_AMD_PLAN_STREAM", 1) != 0;
        if (streamed)
          return launch_plan_stream(ix, S, npats, d_noccs, first, d_out_starts, d_offsets, offsets_capacity, stream, plan.sa_known, max_occs_each,
                                    knob(-1, "FEMTO_AMD_PLAN_STREAM_GRID", 0));
        // handles that walk to marks, no offsets buffer, pointers that are not 16-byte aligned, the switch: the old row plan
        const int r = launch_plan_rows(ix, S, npats, d_noccs, first, d_out_starts, d_offsets, offsets_capacity, stream, nullptr, /*fuse_walk=*/true, plan.sa_known);
        if (!r) g_fell_back++;
        return r;
      },
      &direct);
  if (!rc && !direct) g_fell_back++;      // other kernel families size the walk on the host
  return rc;
  API_END
}

void femto_amd_plan_stream_stats(int64_t out[4]) {
  out[0] = g_streamed.load();
  out[1] = g_fell_back.load();
  out[2] = g_big_launches.load();
  out[3] = g_last_groups.load();
}
