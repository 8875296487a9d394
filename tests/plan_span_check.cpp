// plan_span_check.cpp -- femto_amd/plan/plan_span.hpp on the CPU (tests/test_plan_span.py builds this with
// -fsanitize=address,undefined and runs it): the runs of all wavefronts tile [0, ntiles) exactly once, in order, the owner of
// the last tile is the one plan_last_owner names, and the grid never exceeds one workgroup per tile.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../femto_amd/plan/plan_span.hpp"

using namespace femto_amd;

static int check(int64_t ntiles, int64_t nwaves) {
  std::vector<int> seen(size_t(ntiles), 0);
  int64_t at = 0, last_owner = -1, longest = 0;
  for (int64_t w = 0; w < nwaves; w++) {
    const PlanSpan s = plan_span_of(ntiles, nwaves, w);
    if (s.t0 > s.t1 || s.t0 < 0 || s.t1 > ntiles) return std::printf("bad span %lld %lld w %lld\n", (long long)s.t0, (long long)s.t1, (long long)w), 1;
    if (s.t0 == s.t1) continue;
    if (s.t0 != at) return std::printf("gap before wave %lld (%lld tiles, %lld waves)\n", (long long)w, (long long)ntiles, (long long)nwaves), 1;
    for (int64_t t = s.t0; t < s.t1; t++) seen[size_t(t)]++;
    at = s.t1;
    last_owner = w;
    if (s.t1 - s.t0 > longest) longest = s.t1 - s.t0;
  }
  if (at != ntiles) return std::printf("%lld of %lld tiles covered\n", (long long)at, (long long)ntiles), 1;
  for (int v : seen) if (v != 1) return std::printf("a tile owned %d times\n", v), 1;
  if (last_owner != plan_last_owner(ntiles, nwaves)) return std::printf("last owner %lld != %lld\n", (long long)last_owner, (long long)plan_last_owner(ntiles, nwaves)), 1;
  if (ntiles > 0 && longest != (ntiles + nwaves - 1) / nwaves) return std::printf("longest run %lld\n", (long long)longest), 1;
  return 0;
}

int main() {
  for (int64_t ntiles = 0; ntiles <= 300; ntiles++)
    for (int64_t nwaves = 1; nwaves <= 70; nwaves++)
      if (check(ntiles, nwaves)) return 1;
  const int64_t cases[][2] = {{79, 4}, {79, 8}, {79, 12}, {39063, 8192}, {39063, 2048}, {1 << 18, 8192}, {(int64_t(1) << 31) / 256, 8192}};
  for (auto& c : cases)
    if (check(c[0], c[1])) return 1;
  // spans outside the grid and degenerate arguments own nothing; the extreme sizes do not overflow
  if (plan_span_of(10, 4, 4).t0 != plan_span_of(10, 4, 4).t1 || plan_span_of(10, 4, -1).t1 != 0 || plan_span_of(0, 4, 0).t1 != 0) return std::printf("degenerate\n"), 1;
  const PlanSpan big = plan_span_of(INT64_MAX / 512, 4, 3);
  if (big.t1 != INT64_MAX / 512 || big.t0 >= big.t1) return std::printf("large\n"), 1;
  if (plan_tiles(0) != 0 || plan_tiles(1) != 1 || plan_tiles(256) != 1 || plan_tiles(257) != 2 || plan_tiles(10000000) != 39063) return std::printf("tiles\n"), 1;
  if (plan_stream_groups(39063, 256, 0) != 256 * kPlanGroupsPerCu || plan_stream_groups(79, 256, 0) != 79 || plan_stream_groups(79, 256, 3) != 3 ||
      plan_stream_groups(2, 256, 3) != 2 || plan_stream_groups(0, 256, 0) != 0 || plan_stream_groups(int64_t(1) << 40, 1 << 30, 0) != 0x7fffffffLL)
    return std::printf("groups\n"), 1;
  std::printf("plan_span ok\n");
  return 0;
}
