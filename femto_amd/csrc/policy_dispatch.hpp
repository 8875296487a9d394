// policy_dispatch.hpp -- which rank policy a handle runs, stated once, and the dispatcher that turns that answer into a
// template argument.  Every kernel family that is templated on a policy struct (text_kernels.hip.hpp; WavePolicy of
// regexp_search.hip) is launched through with_policy<the policies it exists for>(kind, f).
//
// The first part is plain C++ (no HIP): tests/policy_check.cpp compiles it with g++.  The second part names the policy structs
// and DevIndex and is included after the kernel headers -- inside trace_kernels.hip's renamed namespace too.
#pragma once
#include <type_traits>

namespace femto_amd {

enum class RankKind { Rum, Ru, Pack, Ind, Pack2, Wave };

// mode 3 (packed lines of small alphabets): the rank units when the handle has them -- the marked ones when they carry the rows'
// mark bits; mode 4 (two-level lines of byte alphabets): the per-character rank lines when the handle has them; modes 0 / 1:
// femto's own wavelet tree
constexpr RankKind rank_kind(int mode, bool has_ru, bool has_ru_marks, bool has_ind) {
  if (mode == 3) return has_ru ? (has_ru_marks ? RankKind::Rum : RankKind::Ru) : RankKind::Pack;
  if (mode == 4) return has_ind ? RankKind::Ind : RankKind::Pack2;
  return RankKind::Wave;
}

// the text tail (count_tail_kernel) steps a single row a few times: the rank lines' one-line-per-range-end step buys it nothing,
// and the kernel is not built for them
constexpr RankKind tail_kind(RankKind k) { return k == RankKind::Ind ? RankKind::Pack2 : k; }

// a walk to a mark (walk_row, lf_steps_kernel, xwalk_kernel) is LF steps of single rows over the layout's base lines: the rank
// units and rank lines only speed up range ends
constexpr RankKind walk_kind(RankKind k) {
  return (k == RankKind::Rum || k == RankKind::Ru) ? RankKind::Pack : (k == RankKind::Ind ? RankKind::Pack2 : k);
}

template <class P> struct Tag { using type = P; };
template <class P> struct KindOf;      // KindOf<P>::value: the kind policy struct P serves

// f(Tag<P>{}) for the policy of `kind`; f is instantiated for the policies in Allowed only.  false: `kind` is none of them
// (nothing was called)
template <class... Allowed, class F>
bool with_policy(RankKind kind, F&& f) {
  return ((KindOf<Allowed>::value == kind && (f(Tag<Allowed>{}), true)) || ...);
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
auto with_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace femto_amd

#ifdef __HIPCC__
namespace femto_amd {

struct RumPolicy; struct RuPolicy; struct PackPolicy; struct IndPolicy; struct Pack2Policy; struct WavePolicy;
template <> struct KindOf<RumPolicy> { static constexpr RankKind value = RankKind::Rum; };
template <> struct KindOf<RuPolicy> { static constexpr RankKind value = RankKind::Ru; };
template <> struct KindOf<PackPolicy> { static constexpr RankKind value = RankKind::Pack; };
template <> struct KindOf<IndPolicy> { static constexpr RankKind value = RankKind::Ind; };
template <> struct KindOf<Pack2Policy> { static constexpr RankKind value = RankKind::Pack2; };
template <> struct KindOf<WavePolicy> { static constexpr RankKind value = RankKind::Wave; };

inline RankKind rank_kind(int mode, const DevIndex& d) { return rank_kind(mode, d.ru != nullptr, d.ru_marks != 0, d.ind != nullptr); }

}  // namespace femto_amd
#endif
