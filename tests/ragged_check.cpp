// ragged_check.cpp -- femto_amd/common/ragged.hpp on the CPU (tests/test_ragged.py builds this with -fsanitize=address,undefined
// and runs it): both binary searches against a linear scan on every small ascending array, sub-range and value; last_start_le on
// every ragged array with empty segments; doc_of at the documents' edges; merge_path_split against an explicit stable merge, for
// plain values and for (document, offset) pairs, with the calls of the comparator counted and their indexes checked; live_of.
// The arrays are heap vectors of their exact size, so the sanitizer sees every index outside them.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <utility>
#include <vector>

#include "../femto_amd/common/ragged.hpp"

using namespace femto_amd;
typedef std::vector<int64_t> Vec;

#define FAIL(...) return std::printf(__VA_ARGS__), std::printf("\n"), 1

// every ascending array of length n over 0..vmax, repeats included
static void ascending(int n, int64_t vmax, Vec& cur, const std::function<void(const Vec&)>& f) {
  if (int(cur.size()) == n) return f(cur);
  for (int64_t v = cur.empty() ? 0 : cur.back(); v <= vmax; v++) {
    cur.push_back(v);
    ascending(n, vmax, cur, f);
    cur.pop_back();
  }
}
static std::vector<Vec> all_ascending(int nmax, int64_t vmax) {
  std::vector<Vec> all;
  for (int n = 0; n <= nmax; n++) {
    Vec cur;
    ascending(n, vmax, cur, [&](const Vec& a) { all.push_back(a); });
  }
  return all;
}

static int check_searches() {
  for (const Vec& a : all_ascending(6, 3)) {
    const int64_t n = int64_t(a.size());
    for (int64_t lo = 0; lo <= n; lo++)
      for (int64_t hi = lo; hi <= n; hi++)
        for (int64_t v = -1; v <= 4; v++) {
          int64_t gt = lo, ge = lo;
          while (gt < hi && a[size_t(gt)] <= v) gt++;
          while (ge < hi && a[size_t(ge)] < v) ge++;
          if (first_gt(a.data(), lo, hi, v) != gt) FAIL("first_gt n %lld [%lld, %lld) v %lld", (long long)n, (long long)lo, (long long)hi, (long long)v);
          if (first_ge(a.data(), lo, hi, v) != ge) FAIL("first_ge n %lld [%lld, %lld) v %lld", (long long)n, (long long)lo, (long long)hi, (long long)v);
          // the accessor may be ptr + 1 (doclist's pack kernel)
          if (lo >= 1 && first_gt(a.data() + 1, lo - 1, hi - 1, v) != gt - 1) FAIL("first_gt on ptr + 1");
        }
  }
  return 0;
}

// starts[0] = 0 <= ... <= starts[n]: repeated starts are empty segments; every p < starts[n] lies in exactly one segment
static int check_last_start_le() {
  int64_t with_empty = 0;
  for (const Vec& tail : all_ascending(6, 3)) {
    if (tail.empty()) continue;
    Vec starts(1, 0);
    starts.insert(starts.end(), tail.begin(), tail.end());
    const int64_t n = int64_t(starts.size()) - 1;
    for (int64_t k = 0; k < n; k++) with_empty += starts[size_t(k)] == starts[size_t(k + 1)];
    for (int64_t p = 0; p < starts[size_t(n)]; p++) {
      const int64_t k = last_start_le(starts.data(), n, p);
      if (k < 0 || k >= n || starts[size_t(k)] > p || starts[size_t(k + 1)] <= p) FAIL("last_start_le n %lld p %lld -> %lld", (long long)n, (long long)p, (long long)k);
    }
  }
  if (!with_empty) FAIL("no empty segment was tried");
  return 0;
}

// document d = [ends[d - 1], ends[d]); lengths 1..3, so one-symbol documents occur at every place
static int check_doc_of() {
  for (int nd = 1; nd <= 4; nd++) {
    int combos = 1;
    for (int i = 0; i < nd; i++) combos *= 3;
    for (int c = 0; c < combos; c++) {
      Vec ends;
      int64_t at = 0;
      for (int i = 0, x = c; i < nd; i++, x /= 3) ends.push_back(at += 1 + x % 3);
      Vec ts(1, 0);
      for (int64_t e : ends) {
        ts.push_back(e - 1);
        ts.push_back(e);
      }
      ts.push_back(at + 5);      // behind the last document
      for (int64_t t : ts) {
        const Doc d = doc_of(ends.data(), nd, t);
        int64_t want = 0;
        while (want < nd && ends[size_t(want)] <= t) want++;
        const int64_t start = want ? ends[size_t(want - 1)] : 0, end = want < nd ? ends[size_t(want)] : kPad;
        if (d.doc != want || d.start != start || d.end != end || t < d.start || t >= d.end) FAIL("doc_of nd %d combo %d t %lld", nd, c, (long long)t);
      }
    }
  }
  const Doc none = doc_of(nullptr, 0, 7);      // no documents: nothing is read
  if (none.doc != 0 || none.start != 0 || none.end != kPad) FAIL("doc_of without documents");
  return 0;
}

// the count of a's elements among the first p of the stable merge (a before b on ties), from the merge itself
template <class Le>
static int64_t merged_from_a(int64_t p, int64_t na, int64_t nb, Le le) {
  int64_t i = 0, j = 0;
  while (i + j < p) {
    if (i < na && (j >= nb || le(i, j))) i++; else j++;
  }
  return i;
}

// docpos' comparator
static bool pair_le(int64_t ad, int64_t ao, int64_t bd, int64_t bo) { return ad < bd || (ad == bd && ao <= bo); }

static int check_merge_path() {
  const std::vector<Vec> lists = all_ascending(5, 3);
  int64_t calls = 0, silent = 0;
  for (const Vec& a : lists)
    for (const Vec& b : lists) {
      const int64_t na = int64_t(a.size()), nb = int64_t(b.size());
      // the same lists as pairs: value v is (document v / 2, offset v % 2)
      Vec ad, ao, bd, bo;
      for (int64_t v : a) ad.push_back(v / 2), ao.push_back(v % 2);
      for (int64_t v : b) bd.push_back(v / 2), bo.push_back(v % 2);
      for (int64_t p = 0; p <= na + nb; p++) {
        const int64_t want = merged_from_a(p, na, nb, [&](int64_t i, int64_t j) { return a[size_t(i)] <= b[size_t(j)]; });
        int64_t asked = 0;
        bool outside = false;
        auto seen = [&](int64_t i, int64_t j) {
          asked++;
          if (i < 0 || i >= na || j < 0 || j >= nb) outside = true;
        };
        // (the raw pointers: an index outside the lists is the sanitizer's to see)
        const int64_t *pa = a.data(), *pb = b.data(), *pad = ad.data(), *pao = ao.data(), *pbd = bd.data(), *pbo = bo.data();
        const int64_t got = merge_path_split(p, na, nb, [&](int64_t i, int64_t j) { return seen(i, j), pa[i] <= pb[j]; });
        const int64_t got2 = merge_path_split(p, na, nb, [&](int64_t i, int64_t j) { return seen(i, j), pair_le(pad[i], pao[i], pbd[j], pbo[j]); });
        const int got3 = merge_path_split(int(p), int(na), int(nb), [&](int i, int j) { return seen(i, j), pa[i] <= pb[j]; });      // a tile in LDS
        if (got != want || got2 != want || got3 != want) FAIL("merge_path_split na %lld nb %lld p %lld: %lld %lld %d, want %lld", (long long)na, (long long)nb, (long long)p, (long long)got, (long long)got2, got3, (long long)want);
        if (outside) FAIL("le asked outside the lists: na %lld nb %lld p %lld", (long long)na, (long long)nb, (long long)p);
        if (p == 0 || p == na + nb || na == 0 || nb == 0) {
          if (asked) FAIL("le asked %lld times for na %lld nb %lld p %lld", (long long)asked, (long long)na, (long long)nb, (long long)p);
          silent++;
        }
        calls += asked;
      }
    }
  if (!calls || !silent) FAIL("merge path: nothing was searched");
  return 0;
}

static int check_live_of() {
  const int64_t n = 5, vals[] = {-3, 0, 4, 5, 6, INT64_MAX}, want[] = {0, 0, 4, 5, 5, 5};
  if (live_of(nullptr, n) != n || live_of(nullptr, 0) != 0) FAIL("live_of without a count");
  for (int i = 0; i < 6; i++)
    if (live_of(&vals[i], n) != want[i]) FAIL("live_of %lld", (long long)vals[i]);
  return 0;
}

int main() {
  if (check_searches() || check_last_start_le() || check_doc_of() || check_merge_path() || check_live_of()) return 1;
  std::printf("ragged ok\n");
  return 0;
}
