// ragged.hpp -- the searches that doclist.hip, docpos.hip, bquery.hip and extract.hip share: the two binary searches over an
// ascending array, the segment of a ragged array an element belongs to, the document that holds a text position, the split of a
// merge path, the live count of a batch.  Plain arithmetic, callable from the host and the device: tests/ragged_check.cpp runs it
// on the CPU.  DESIGN.md "Shared host plumbing" says what belongs here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAGGED_FN __host__ __device__ __forceinline__
#else
#define RAGGED_FN inline
#endif

namespace femto_amd {

// `a` is anything ascending with operator[]: a global pointer, an LDS array, ptr + 1.  Every caller gives its own bounds.

// first index in [lo, hi) with a[i] > v (hi when there is none)
template <class A>
RAGGED_FN int64_t first_gt(A a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (a[m] <= v) lo = m + 1; else hi = m;
  }
  return lo;
}

// first index in [lo, hi) with a[i] >= v (hi when there is none)
template <class A>
RAGGED_FN int64_t first_ge(A a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (a[m] < v) lo = m + 1; else hi = m;
  }
  return lo;
}

// the last k in [0, n) with starts[k] <= p   (0 <= p < starts[n]): the segment of a ragged array that element p belongs to.
// The first index with starts[index] > p lies in [1, n]: starts[0] and starts[n] are not read.
RAGGED_FN int64_t last_start_le(const int64_t* __restrict__ starts, int64_t n, int64_t p) { return first_gt(starts, 1, n, p) - 1; }

constexpr int64_t kPad = INT64_MAX;      // sorts behind every text position

struct Doc {
  int64_t doc, start, end;     // end = kPad for the "document" behind the last one
};

// the document that holds text position t: the number of document ends <= t (resolve_location, src/main/index.c:1587)
RAGGED_FN Doc doc_of(const int64_t* __restrict__ doc_ends, int64_t ndocs, int64_t t) {
  const int64_t d = first_gt(doc_ends, 0, ndocs, t);
  Doc r;
  r.doc = d;
  r.start = d ? doc_ends[d - 1] : 0;
  r.end = d < ndocs ? doc_ends[d] : kPad;
  return r;
}

// Merge path: the number of elements of a among the first p of the stable merge of a (na elements) and b (nb elements), a before
// b on ties: the least i with i == hi or a[i] > b[p - i - 1].  le(i, j) says a[i] <= b[j]; it is asked only for i < na and j < nb,
// and not at all when p = 0, p = na + nb, na = 0 or nb = 0 (they leave lo == hi).  I: int64_t, or int for a tile staged in LDS.
template <class I, class Le>
RAGGED_FN I merge_path_split(I p, I na, I nb, Le le) {
  I lo = p > nb ? p - nb : 0, hi = p < na ? p : na;
  while (lo < hi) {
    const I m = (lo + hi) >> 1;
    if (le(m, p - m - 1)) lo = m + 1; else hi = m;
  }
  return lo;
}

// how many of a batch's n entries are live: all of them, or min(n, *d_n) when the caller passes a count (negative: none)
RAGGED_FN int64_t live_of(const int64_t* d_n, int64_t n) {
  if (!d_n) return n;
  const int64_t v = *d_n;
  return v < 0 ? 0 : (v < n ? v : n);
}

}  // namespace femto_amd
