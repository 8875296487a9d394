// trace_kernels.hip -- the query kernels of the direct pipeline compiled a SECOND time with the line trace switched on.
//
// bench.py's roofline needs the COMPULSORY bytes of a launch: 128 B for every distinct line of a derived array the
// kernels load.  That is counted on the GPU by running the batch once through traced twins of the very same kernel
// sources: this translation unit includes the kernel headers with FEMTO_AMD_TRACE defined (trace_touch() then sets one
// bit per loaded line, pack_kernels.hip.hpp) and with the namespace renamed, so the twins do not collide with the
// production kernels -- which contain no trace code at all.  The launches are direct_launch.hpp's, the ones production runs: the
// twins only say what a trace does differently (it always plans, and it raises errors in its own flag word).
#define FEMTO_AMD_TRACE 1
#define femto_amd femto_amd_traced
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernels.hip.hpp"
#include "pack_kernels.hip.hpp"
#include "ru_kernels.hip.hpp"
#include "pack2_kernels.hip.hpp"
#include "ind_kernels.hip.hpp"
#include "text_kernels.hip.hpp"
#include "ctx_kernels.hip.hpp"
#include "direct_kernels.hip.hpp"
#include "direct_launch.hpp"
#undef femto_amd

#include "trace_api.hpp"

namespace femto_amd_trace_api {

using namespace femto_amd_traced;

size_t traced_dev_index_bytes() { return sizeof(DevIndex); }

static DevIndex make_dev(const TraceArgs& a) {
  DevIndex d;
  memcpy(&d, a.dev, sizeof d);
  d.trace = a.bitmap;
  d.trace_reads = a.reads;
  for (int r = 0; r < kTraceRegions; r++) d.trace_off[r] = a.trace_off[r];
  d.tail_items = a.tail_items;
  d.tail_count = a.flags + 2;
  d.tail_min = a.tail_min;
  d.row_free = a.row_free;
  if (!a.tail_items && !inline_tail_applies(d, a.row_free != 0)) d.txt = nullptr;
  return d;
}

// count_direct_kernel + count_tail_kernel (+ plan_super_kernel) + plan_rows_kernel (out_starts only)
hipError_t traced_count_plan(const TraceArgs& a) {
  const DevIndex d = make_dev(a);
  const int64_t nblocks = direct_blocks(a.npats);
  hipError_t e = hipMemsetAsync(a.flags, 0, 4 * sizeof(int), a.stream);
  if (e != hipSuccess) return e;
  const DirectDecision dec = direct_decision(a.mode, d, /*plan=*/true, a.row_free != 0);
  const PlanSums ps = plan_sums_at(a.bsums, nblocks, !dec.tail, a.parity);
  const CountArgs c{a.npats, a.plen, a.pats, a.starts, a.first, a.last, a.flags, a.max_occs, a.noccs, ps, a.flags + 1, dec.wants_sa_out ? a.sa_known : nullptr,
                    a.num_cus, a.stream};
  if ((e = enqueue_count_direct<true>(rank_kind(a.mode, d), dec, d, c)) != hipSuccess) return e;
  if (dec.tail && (e = enqueue_plan_super(ps, a.stream)) != hipSuccess) return e;
  enqueue_plan_rows<kRowsOnly, PackPolicy>(d, RowsArgs{a.npats, a.noccs, a.first, nullptr, ps, a.out_starts, nullptr, INT64_MAX, a.flags + 1, a.total, nullptr, nullptr,
                                                       a.num_cus, a.stream});
  return hipGetLastError();
}

// the row plan that writes the offsets, as femto_amd_locate_device launches it: from the resident suffix array, or -- sampled
// marks -- by the walk inside the row expansion
hipError_t traced_walk(const TraceArgs& a, int64_t* offsets, int64_t capacity) {
  const DevIndex d = make_dev(a);
  hipError_t e = hipMemsetAsync(a.flags + 1, 0, sizeof(int), a.stream);
  if (e != hipSuccess) return e;
  // the count twin left its hints in a.sa_known
  const bool known = d.sa_full || spots_marks(a.mode, d.ru, d.ru_marks, d.pack, d.pack_sa) || (a.row_free && a.tail_items);
  return enqueue_plan_offsets(rank_kind(a.mode, d), d,
                              RowsArgs{a.npats, a.noccs, a.first, nullptr, plan_sums_at(a.bsums, direct_blocks(a.npats), false, a.parity), a.out_starts, offsets,
                                       capacity, a.flags + 1, a.total, nullptr, known ? a.sa_known : nullptr, a.num_cus, a.stream});
}

hipError_t traced_popcount(const uint32_t* bitmap, int64_t w0, int64_t w1, unsigned long long* out, hipStream_t stream) {
  hipLaunchKernelGGL(trace_popcount_kernel, dim3(1024), dim3(256), 0, stream, bitmap, w0, w1, out);
  return hipGetLastError();
}

}  // namespace femto_amd_trace_api
