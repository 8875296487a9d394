// direct_launch.hpp -- the launch sequence of the direct pipeline (modes 3 / 4, direct_kernels.hip.hpp), once: what a count
// launch decides and the enqueue functions of its kernels, over plain arguments (no handle, no scratch).  femto_amd_api.hip wraps
// them in its scratch reservations and timer brackets; trace_kernels.hip includes this header under its renamed namespace, so the
// traced twins are launched by the very same code.
//
// The decision is plain C++ (tests/policy_check.cpp compiles it with g++); the rest follows the kernel headers.
#pragma once
#include "policy_dispatch.hpp"

namespace femto_amd {

// dense: full suffix array + inverse suffix array resident -- the text tail is compared inline, after the wavefront's stepping
//   loop (count_direct_kernel<.., kDense = true>; a row-free launch needs no way back from a position to a row: inline_tail_applies).
// tail: the handle holds text but only the sampled arrays -- the pattern is handed over to count_tail_kernel instead.
// spot: a handle WITHOUT the inline tail whose rank units carry the rows' mark bits (ru_kernels.hip.hpp) and that walks to
//   sampled marks: the search reports a marked row it stood on and plan_rows_kernel starts from it ("mark spotting").
// wants_sa_out: the count leaves what it knows of one-row patterns for plan_rows_kernel -- the text position (dense: the text
//   tail's, the wide context table's; row-free hand-over: the position count_tail_kernel found the pattern at) or the spotted row.
struct DirectDecision { bool dense, tail, spot, wants_sa_out; };
constexpr bool spots_marks(int mode, bool has_ru, bool has_ru_marks, bool has_pack, bool has_pack_sa) {
  return mode == 3 && has_ru && has_ru_marks && has_pack && has_pack_sa;
}
constexpr DirectDecision direct_decision(bool inline_tail, bool has_text, bool plan, bool row_free, bool spots) {
  const bool tail = has_text && !inline_tail, spot = plan && !inline_tail && spots;
  return {inline_tail, tail, spot, plan && (inline_tail || spot || (row_free && tail))};
}

}  // namespace femto_amd

#ifdef __HIPCC__
#include <algorithm>

namespace femto_amd {

inline DirectDecision direct_decision(int mode, const DevIndex& d, bool plan, bool row_free) {
  return direct_decision(inline_tail_applies(d, plan && row_free), d.txt != nullptr, plan, row_free,
                         spots_marks(mode, d.ru != nullptr, d.ru_marks != 0, d.pack != nullptr, d.pack_sa != nullptr));
}

// what the kernels of a count launch take besides the index (whose tail_* and row_free fields the caller has set)
struct CountArgs {
  int64_t npats;
  const int32_t* plen;  const uint16_t* pats;  const int64_t* starts;
  int64_t *first, *last;  int* err;
  int max_occs;          // with a plan: its clamp, noccs[], block sums and flag of long ranges
  int32_t* noccs;  PlanSums ps;  int* big_flag;
  int64_t* sa_out;       // or NULL (DirectDecision::wants_sa_out)
  int num_cus;  hipStream_t stream;
};

inline int64_t direct_blocks(int64_t npats) { return (npats + 255) / 256; }
inline dim3 direct_persistent_grid(int64_t npats, int num_cus) { return dim3(uint32_t(std::min<int64_t>(direct_blocks(npats), int64_t(num_cus) * 8))); }

// count_direct_kernel of the handle's layout and, for a hand-over tail, count_tail_kernel on its persistent grid (the number of
// handed-over patterns is only known on the device); with the full suffix array resident the tail's row position is one read
template <bool kPlan>
hipError_t enqueue_count_direct(RankKind kind, const DirectDecision& dec, const DevIndex& d, const CountArgs& c) {
  const dim3 grid{uint32_t(direct_blocks(c.npats))}, block{256};
  bool known = with_policy<RumPolicy, RuPolicy, PackPolicy, IndPolicy, Pack2Policy>(kind, [&](auto tag) {
    using P = typename decltype(tag)::type;
    with_flag(dec.dense, [&](auto dense) {
      hipLaunchKernelGGL((count_direct_kernel<P, kPlan, decltype(dense)::value>), grid, block, 0, c.stream, d, c.npats, c.plen, c.pats, c.starts,
                         c.first, c.last, c.err, c.max_occs, c.noccs, c.ps, c.big_flag, c.sa_out);
    });
  });
  hipError_t e = known ? hipGetLastError() : hipErrorInvalidDeviceFunction;
  if (e != hipSuccess || !dec.tail) return e;
  const TailOut out{nullptr, c.first, c.last, c.noccs, c.ps.sums, c.max_occs, c.sa_out, d.row_free};
  known = with_policy<RumPolicy, RuPolicy, PackPolicy, Pack2Policy>(tail_kind(kind), [&](auto tag) {
    using P = typename decltype(tag)::type;
    with_flag(d.sa_full != nullptr, [&](auto sa_full) {
      // (no permutation, no keys: those are the sorted batches')
      hipLaunchKernelGGL((count_tail_kernel<P, decltype(sa_full)::value>), direct_persistent_grid(c.npats, c.num_cus), block, 0, c.stream, d,
                         static_cast<const TailItem*>(d.tail_items), d.tail_count, c.plen, c.pats, c.starts, nullptr, nullptr, 1, 0, out, c.err);
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidDeviceFunction;
}

// a hand-over tail made the block sums final in count_tail_kernel: the group sums in a launch of their own
inline hipError_t enqueue_plan_super(const PlanSums& ps, hipStream_t stream) {
  hipLaunchKernelGGL(plan_super_kernel, dim3(uint32_t(((ps.nblocks + 63) / 64 + 3) / 4)), dim3(256), 0, stream, ps);
  return hipGetLastError();
}

// what the row plan takes besides the index
struct RowsArgs {
  int64_t npats;
  const int32_t* noccs;  const int64_t* first;
  const int2* first32;         // or NULL: (first, last) pairs instead of first[]
  PlanSums ps;  int64_t* out_starts;
  int64_t* offsets;            // or NULL: out_starts[] only
  int64_t capacity;
  int* big_flag;               // cleared by the count kernel
  int64_t *total, *total_user;
  const int64_t* sa_known;     // or NULL: the count's sa_out
  int num_cus;  hipStream_t stream;
};

template <int kMode, class P>
void enqueue_plan_rows(const DevIndex& d, const RowsArgs& r) {
  hipLaunchKernelGGL((plan_rows_kernel<kMode, P>), dim3(uint32_t(direct_blocks(r.npats))), dim3(256), 0, r.stream, r.npats, r.noccs, r.first, r.first32,
                     r.ps, r.out_starts, r.offsets, r.capacity, r.big_flag, d, r.total, r.total_user, r.sa_known);
}
// ... and, when there is an offsets buffer, plan_big_rows_kernel for the long ranges it left over
template <int kMode, class P>
void enqueue_plan_rows_big(const DevIndex& d, const RowsArgs& r) {
  enqueue_plan_rows<kMode, P>(d, r);
  if (!r.offsets) return;
  hipLaunchKernelGGL((plan_big_rows_kernel<kMode, P>), direct_persistent_grid(r.npats, r.num_cus), dim3(256), 0, r.stream, r.npats, r.first, r.first32,
                     r.out_starts, r.total, r.capacity, r.offsets, r.big_flag, d);
}

// The row plan that writes the offsets themselves (r.offsets is given): from the resident suffix array, or by a walk per row
// inside the expansion.  The policy only matters to the walk.
inline hipError_t enqueue_plan_offsets(RankKind kind, const DevIndex& d, const RowsArgs& r) {
  bool known = true;
  if (d.sa_full) enqueue_plan_rows_big<kRowsSa, PackPolicy>(d, r);
  else known = with_policy<PackPolicy, Pack2Policy>(walk_kind(kind), [&](auto tag) { enqueue_plan_rows_big<kRowsWalk, typename decltype(tag)::type>(d, r); });
  return known ? hipGetLastError() : hipErrorInvalidDeviceFunction;
}

}  // namespace femto_amd
#endif
