// policy_check.cpp -- the rank-policy rule and the decision of a direct count launch on the CPU: a stand-alone program over
// the plain-C++ parts of femto_amd/csrc/policy_dispatch.hpp and direct_launch.hpp (tests/test_policy_rule.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer and runs it once).  Every expectation is a literal table written down from the
// if / else-if ladders the launch layer held before there was one rule; none is computed by the functions under test.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../femto_amd/csrc/direct_launch.hpp"

using namespace femto_amd;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

namespace {

constexpr RankKind Rum = RankKind::Rum, Ru = RankKind::Ru, Pack = RankKind::Pack, Ind = RankKind::Ind, Pack2 = RankKind::Pack2, Wave = RankKind::Wave;

// mode, rank units, marked rank units, rank lines -> the policy of the search.  The ladder of the automaton search (mode 3 && ru
// && marks / mode 3 && ru / mode 3 / mode 4 && ind / mode 4 / else) and the ladder of the count launch (the same, but `ind` without
// `mode == 4`: it only ever runs in modes 3 / 4) agree on every row a handle can have.  Rows no handle has: the rank lines (ind) are
// derived for byte alphabets, the rank units for small ones, so ind with mode 3 and ru with mode 4 only meet on a handle whose rank
// mode was forced; marks without units never; and in modes 0 / 1 the count ladder does not run (its own answer there, ind -> Ind,
// else Pack2, is the one place the two disagree: the table records the automaton search's, the only one that runs).
struct KindRow {
  int mode, ru, marks, ind;
  RankKind want;
};
const KindRow kKinds[] = {
    {3, 0, 0, 0, Pack}, {3, 0, 0, 1, Pack}, {3, 0, 1, 0, Pack}, {3, 0, 1, 1, Pack}, {3, 1, 0, 0, Ru},    {3, 1, 0, 1, Ru},  {3, 1, 1, 0, Rum},   {3, 1, 1, 1, Rum},
    {4, 0, 0, 0, Pack2}, {4, 0, 0, 1, Ind}, {4, 0, 1, 0, Pack2}, {4, 0, 1, 1, Ind}, {4, 1, 0, 0, Pack2}, {4, 1, 0, 1, Ind}, {4, 1, 1, 0, Pack2}, {4, 1, 1, 1, Ind},
    {0, 0, 0, 0, Wave}, {0, 0, 0, 1, Wave}, {0, 0, 1, 0, Wave}, {0, 0, 1, 1, Wave}, {0, 1, 0, 0, Wave},  {0, 1, 0, 1, Wave}, {0, 1, 1, 0, Wave}, {0, 1, 1, 1, Wave},
    {1, 0, 0, 0, Wave}, {1, 0, 0, 1, Wave}, {1, 0, 1, 0, Wave}, {1, 0, 1, 1, Wave}, {1, 1, 0, 0, Wave},  {1, 1, 0, 1, Wave}, {1, 1, 1, 0, Wave}, {1, 1, 1, 1, Wave},
};

// the text tail's ladder (Rum / Ru / Pack, else Pack2: a handle with rank lines takes Pack2Policy) and the walks' (mode 3: Pack,
// else Pack2 -- the device-sized walk, the LF steps, extraction's walk); neither exists for the wavelet tree
struct NarrowRow {
  RankKind kind, tail, walk;
};
const NarrowRow kNarrow[] = {{Rum, Rum, Pack}, {Ru, Ru, Pack}, {Pack, Pack, Pack}, {Ind, Pack2, Pack2}, {Pack2, Pack2, Pack2}, {Wave, Wave, Wave}};

// inline tail applies, the handle holds text, a plan is wanted, the plan is row-free, the layout spots marks -> dense, tail, spot,
// wants_sa_out: the count launch's  dense = inline;  tail = text && !inline;  spot = plan && !dense && layout;
// sa_out = plan && (dense || spot || (row_free && tail)).  (inline without text cannot happen: the inline tail reads the text.)
struct DecisionRow {
  int inline_tail, text, plan, row_free, spots, dense, tail, spot, wants;
};
const DecisionRow kDecisions[] = {
    {0, 0, 0, 0, 0,   0, 0, 0, 0}, {0, 0, 0, 0, 1,   0, 0, 0, 0}, {0, 0, 0, 1, 0,   0, 0, 0, 0}, {0, 0, 0, 1, 1,   0, 0, 0, 0},
    {0, 0, 1, 0, 0,   0, 0, 0, 0}, {0, 0, 1, 0, 1,   0, 0, 1, 1}, {0, 0, 1, 1, 0,   0, 0, 0, 0}, {0, 0, 1, 1, 1,   0, 0, 1, 1},
    {0, 1, 0, 0, 0,   0, 1, 0, 0}, {0, 1, 0, 0, 1,   0, 1, 0, 0}, {0, 1, 0, 1, 0,   0, 1, 0, 0}, {0, 1, 0, 1, 1,   0, 1, 0, 0},
    {0, 1, 1, 0, 0,   0, 1, 0, 0}, {0, 1, 1, 0, 1,   0, 1, 1, 1}, {0, 1, 1, 1, 0,   0, 1, 0, 1}, {0, 1, 1, 1, 1,   0, 1, 1, 1},
    {1, 0, 0, 0, 0,   1, 0, 0, 0}, {1, 0, 0, 0, 1,   1, 0, 0, 0}, {1, 0, 0, 1, 0,   1, 0, 0, 0}, {1, 0, 0, 1, 1,   1, 0, 0, 0},
    {1, 0, 1, 0, 0,   1, 0, 0, 1}, {1, 0, 1, 0, 1,   1, 0, 0, 1}, {1, 0, 1, 1, 0,   1, 0, 0, 1}, {1, 0, 1, 1, 1,   1, 0, 0, 1},
    {1, 1, 0, 0, 0,   1, 0, 0, 0}, {1, 1, 0, 0, 1,   1, 0, 0, 0}, {1, 1, 0, 1, 0,   1, 0, 0, 0}, {1, 1, 0, 1, 1,   1, 0, 0, 0},
    {1, 1, 1, 0, 0,   1, 0, 0, 1}, {1, 1, 1, 0, 1,   1, 0, 0, 1}, {1, 1, 1, 1, 0,   1, 0, 0, 1}, {1, 1, 1, 1, 1,   1, 0, 0, 1},
};

// six policy structs of the check's own
struct ARum { static constexpr int id = 11; };
struct ARu { static constexpr int id = 12; };
struct APack { static constexpr int id = 13; };
struct AInd { static constexpr int id = 14; };
struct APack2 { static constexpr int id = 15; };
struct AWave { static constexpr int id = 16; };

}  // namespace

namespace femto_amd {
template <> struct KindOf<ARum> { static constexpr RankKind value = RankKind::Rum; };
template <> struct KindOf<ARu> { static constexpr RankKind value = RankKind::Ru; };
template <> struct KindOf<APack> { static constexpr RankKind value = RankKind::Pack; };
template <> struct KindOf<AInd> { static constexpr RankKind value = RankKind::Ind; };
template <> struct KindOf<APack2> { static constexpr RankKind value = RankKind::Pack2; };
template <> struct KindOf<AWave> { static constexpr RankKind value = RankKind::Wave; };
}  // namespace femto_amd

int main() {
  // ---- rank_kind: all 4 x 2 x 2 x 2 combinations, each once
  CHECK(sizeof kKinds / sizeof kKinds[0] == 32);
  std::vector<int> seen(4 * 8, 0);
  for (const KindRow& r : kKinds) {
    CHECK(rank_kind(r.mode, r.ru != 0, r.marks != 0, r.ind != 0) == r.want);
    seen[size_t((r.mode == 3 ? 0 : r.mode == 4 ? 1 : r.mode == 0 ? 2 : 3) * 8 + r.ru * 4 + r.marks * 2 + r.ind)]++;
  }
  for (int s : seen) CHECK(s == 1);

  // ---- the two narrowings
  for (const NarrowRow& r : kNarrow) {
    CHECK(tail_kind(r.kind) == r.tail);
    CHECK(walk_kind(r.kind) == r.walk);
  }

  // ---- mark spotting: of the 4 x 16 layouts exactly one -- mode 3, marked rank units, packed lines and their sampled marks
  int spotting = 0;
  for (int mode : {0, 1, 3, 4})
    for (int m = 0; m < 16; m++) spotting += spots_marks(mode, (m & 8) != 0, (m & 4) != 0, (m & 2) != 0, (m & 1) != 0) ? 1 : 0;
  CHECK(spotting == 1);
  CHECK(spots_marks(3, true, true, true, true));

  // ---- the decision of a direct count launch: all 2^5 combinations, each once
  CHECK(sizeof kDecisions / sizeof kDecisions[0] == 32);
  std::vector<int> dseen(32, 0);
  for (const DecisionRow& r : kDecisions) {
    const DirectDecision d = direct_decision(r.inline_tail != 0, r.text != 0, r.plan != 0, r.row_free != 0, r.spots != 0);
    CHECK(d.dense == (r.dense != 0));
    CHECK(d.tail == (r.tail != 0));
    CHECK(d.spot == (r.spot != 0));
    CHECK(d.wants_sa_out == (r.wants != 0));
    CHECK(!(d.tail && d.dense));
    CHECK(d.wants_sa_out == (r.plan && (d.dense || d.spot || (r.row_free && d.tail))));
    dseen[size_t(r.inline_tail * 16 + r.text * 8 + r.plan * 4 + r.row_free * 2 + r.spots)]++;
  }
  for (int s : dseen) CHECK(s == 1);

  // ---- the dispatcher: every kind reaches its own policy, once ...
  const RankKind all[] = {Rum, Ru, Pack, Ind, Pack2, Wave};
  const int ids[] = {11, 12, 13, 14, 15, 16};
  for (int k = 0; k < 6; k++) {
    std::vector<int> got;
    CHECK((with_policy<ARum, ARu, APack, AInd, APack2, AWave>(all[k], [&](auto tag) { got.push_back(decltype(tag)::type::id); })));
    CHECK(got.size() == 1 && got[0] == ids[k]);
  }
  // ... and a kind outside the allowed policies is reported, nothing is called in its place
  for (int k = 0; k < 6; k++) {
    int calls = 0, id = 0;
    const bool hit = with_policy<APack, APack2>(all[k], [&](auto tag) { calls++; id = decltype(tag)::type::id; });
    const bool allowed = all[k] == Pack || all[k] == Pack2;
    CHECK(hit == allowed && calls == (allowed ? 1 : 0));
    if (allowed) CHECK(id == (all[k] == Pack ? 13 : 15));
    // narrowed first, the walk's two policies serve every derived layout; the wavelet tree stays reported
    int wid = 0;
    CHECK((with_policy<APack, APack2>(walk_kind(all[k]), [&](auto tag) { wid = decltype(tag)::type::id; })) == (all[k] != Wave));
    CHECK(wid == (all[k] == Wave ? 0 : (all[k] == Ind || all[k] == Pack2) ? 15 : 13));
  }
  // with_flag hands the flag on as a type
  CHECK(with_flag(true, [](auto f) { return int(decltype(f)::value) + 10; }) == 11);
  CHECK(with_flag(false, [](auto f) { return int(decltype(f)::value) + 10; }) == 10);
  std::printf("policy ok\n");
  return 0;
}
