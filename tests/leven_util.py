"""The question of include/femto_amd.h "occurrences within k edits, by exact seeds", restated in plain numpy over a fixture's
documents, and the pattern sets the tests of it share (tests/test_leven_host.py pins both to a plain double loop, to
tests/hamming_util.py and to tests/edit_util.py; tests/test_gpu_leven.py and tests/test_gpu_leven_edges.py run them).

THE RULE.  Over the PREPARED TEXT -- every document's bytes + 5 followed by SEOF, not cyclic -- offset p is an occurrence of the
pattern (byte characters only) when some substring T[p .. e), p < e, of byte characters only has Levenshtein distance <= k to it.
Its result is (p, c, L): c the smallest distance over all e, L the smallest e - p that reaches c.

THE YARDSTICK.  Text and pattern are reversed, so that the free end becomes a free START: Sellers' recurrence, row by row over the
pattern, with key = cost * M + length (M = 2^20) in every cell, so the lexicographic minimum travels with the cost.  The dependency
along the text (a text symbol the pattern lacks: key + M + 1 from the left neighbour) is resolved per row with
np.minimum.accumulate on key - j (M + 1).  A symbol that is no byte character starts the table afresh behind it: its column is the
column of the empty text, and the accumulate is kept from crossing it by an offset per run that dwarfs every key."""
import zlib

import numpy as np

from hamming_util import ALPHA, MAX_PATTERN, OFFSET, SEOF, codes, pieces, prepared          # noqa: F401  (the tests import them from here)

M = 1 << 20
_RUN = 1 << 42          # per run of byte characters: |key - j (M + 1)| stays below 2^39 for texts below 2^17 symbols, and 2^17 runs fit an int64
KS = (0, 1, 2, 3, 5)
CUTS = ((9, 8), (24, 8), (64, 8), (100, 8), (300, 2))          # (length, how many); and eight of k + 1


def occurrences(text, pattern, k):
    """(offsets int64[] ascending, costs int32[], lengths int32[]) of `pattern` (alpha codes of bytes) in `text` (prepared)"""
    p = np.asarray(pattern, dtype=np.int64)[::-1]
    m, n = len(p), len(text)
    assert 0 <= k < m and n < (1 << 17)
    rr = np.asarray(text, dtype=np.int64)[::-1]
    fresh = np.concatenate([[True], rr < OFFSET])          # column j = j reversed symbols consumed; 0 and the columns of non-bytes start afresh
    shift = np.arange(n + 1, dtype=np.int64) * (M + 1) + (np.cumsum(fresh) - 1) * _RUN
    row = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, m + 1):
        a = row + M                                                     # the pattern symbol has no partner
        np.minimum(a[1:], row[:-1] + (rr != p[i - 1]) * M + 1, out=a[1:])          # ... stands opposite the text symbol
        a[fresh] = i * M
        row = np.minimum.accumulate(a - shift) + shift                  # ... the text symbol has no partner
    cost, length = row // M, row % M
    at = np.nonzero((cost <= k) & ~fresh)[0][::-1]
    assert (length[at] >= 1).all()
    return (n - at).astype(np.int64), cost[at].astype(np.int32), length[at].astype(np.int32)


def expected(text, patterns, k):
    """the call's answer: (result_start int64[n + 1], offset int64[], cost int32[], length int32[])"""
    start, cols = [0], ([], [], [])
    for p in patterns:
        r = occurrences(text, p, k)
        for col, v in zip(cols, r):
            col.append(v)
        start.append(start[-1] + len(r[0]))
    cat = lambda col, dtype: np.concatenate(col).astype(dtype) if col else np.zeros(0, dtype=dtype)          # noqa: E731
    return np.array(start, dtype=np.int64), cat(cols[0], np.int64), cat(cols[1], np.int32), cat(cols[2], np.int32)


def around(text, p, k, at):
    """occurrences() over the part of the text that can hold a result near `at`: (offsets in the whole text, costs, lengths) of the
    slice [at - 2 k - 8, at + len(p) + 2 k + 8) -- for patterns too long to slide over a whole text in a test"""
    lo, hi = max(0, at - 2 * k - 8), min(len(text), at + len(p) + 2 * k + 8)
    o, c, length = _banded(text[lo:hi], p, k)
    return o + lo, c, length


def _banded(text, pattern, k):
    """occurrences() for a text little longer than the pattern, row i over the columns i - k - 1 .. i + (n - m) + 2 k + 1 alone: an
    alignment of cost <= k that starts at column s and ends inside the text has consumed between i - k and i + k symbols at row i,
    and s <= n - m + k, so it never leaves the band; a cell outside it counts as unreachable"""
    p = np.asarray(pattern, dtype=np.int64)[::-1]
    m, n = len(p), len(text)
    far = 1 << 50
    rr = np.asarray(text, dtype=np.int64)[::-1]
    fresh = np.concatenate([[True], rr < OFFSET])
    shift = np.arange(n + 1, dtype=np.int64) * (M + 1) + (np.cumsum(fresh) - 1) * _RUN
    row = np.full(n + 1, far, dtype=np.int64)
    width = max(n - m, 0) + 2 * k + 1
    row[:min(n, width) + 1] = 0
    for i in range(1, m + 1):
        lo, hi = max(0, i - k - 1), min(n, i + width)
        a = row[lo:hi + 1] + M
        d0 = max(lo, 1)
        np.minimum(a[d0 - lo:], row[d0 - 1:hi] + (rr[d0 - 1:hi] != p[i - 1]) * M + 1, out=a[d0 - lo:])
        a[fresh[lo:hi + 1]] = i * M
        row[lo:hi + 1] = np.minimum.accumulate(a - shift[lo:hi + 1]) + shift[lo:hi + 1]
        if lo:
            row[lo - 1] = far
    cost, length = row // M, row % M
    at = np.nonzero((cost <= k) & ~fresh)[0][::-1]
    return (n - at).astype(np.int64), cost[at].astype(np.int32), length[at].astype(np.int32)


# ---- planting edits ---------------------------------------------------------------------------------------------------------------

KINDS = ("sub", "del", "ins", "mix")


def plant(rng, p, nedits, kind, have, k, lack=None):
    """p with `nedits` edits: substitutions by another byte of `have`, deletions, insertions of a byte of `have`, or a mix.  Never
    shorter than k + 1.  lack: the first edit is a substitution by that alpha code (a character the text lacks)"""
    p = list(int(v) for v in p)
    for n in range(nedits):
        what = kind if kind != "mix" else KINDS[int(rng.integers(0, 3))]
        if lack is not None and n == 0:
            p[int(rng.integers(0, len(p)))] = lack
            continue
        if what == "del" and len(p) - 1 <= k:
            what = "sub"
        i = int(rng.integers(0, len(p)))
        if what == "sub":
            c = have[have != p[i] - OFFSET]
            if len(c):
                p[i] = int(rng.choice(c)) + OFFSET
        elif what == "del":
            del p[i]
        else:
            p.insert(i, int(rng.choice(have)) + OFFSET)
    return np.array(p[:MAX_PATTERN], dtype=np.uint16)


def pattern_set(docs, name, k):
    """[(tag, uint16 alpha codes)]: patterns of more than k symbols for bound k.  Cuts of the text of k + 1, 9, 24, 64, 100 (eight
    each) and 300 symbols (two) with 0 .. k edits planted -- substitutions, deletions, insertions and mixes in turn; every fourth
    planted cut with a character the text lacks, where it lacks one -- tagged "cut..."; then the named cases.  Deterministic per
    fixture name and k."""
    rng = np.random.default_rng(zlib.crc32(("leven %s %d" % (name, k)).encode()))
    docs = [np.asarray(d, dtype=np.uint8) for d in docs]
    total = sum(len(d) + 1 for d in docs)
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    longest = max(docs, key=len)
    out = []

    def add(tag, p):
        assert k < len(p) <= MAX_PATTERN
        out.append((tag, np.asarray(p, dtype=np.uint16)))

    def cut(length, doc=None, at=None):
        d = longest if doc is None else doc
        at = int(rng.integers(0, len(d) - length + 1)) if at is None else at
        return d[at:at + length].astype(np.uint16) + OFFSET

    n = 0
    for m, count in sorted({(k + 1, 8)} | set(CUTS)):
        if not k < m <= len(longest):
            continue
        for r in range(count):
            nedits = r % (k + 1)
            lack = int(lacks[0]) + OFFSET if n % 4 == 3 and nedits and len(lacks) else None
            add("cut%d_%d_%s" % (m, nedits, KINDS[n % 4]), plant(rng, cut(m), nedits, KINDS[n % 4], have, k, lack))
            n += 1
    m = min(24, len(docs[0]))
    if m > k:
        add("from_offset_0", cut(m, docs[0], 0))
        add("from_offset_0_planted", plant(rng, cut(m, docs[0], 0), min(k, 1), "ins", have, k))
    for d in docs[:3]:
        m = min(24, len(d))
        if m > k:
            add("to_last_byte", cut(m, d, len(d) - m))
            add("to_last_byte_planted", plant(rng, cut(m, d, len(d) - m), min(k, 2), "mix", have, k))
    if len(docs) > 1 and min(len(docs[0]), len(docs[1])) >= 12:
        add("straddle", np.concatenate([docs[0][-12:], docs[1][:12]]).astype(np.uint16) + OFFSET)
    if total + 1 <= MAX_PATTERN:          # (acgt48k's text is longer than a pattern may be)
        add("longer_than_the_text", rng.choice(have, size=total + 1).astype(np.uint16) + OFFSET)
    for m in (3 * (k + 1) + 1, 7 * (k + 1) + k):          # lengths that k + 1 does not divide (k > 0)
        if m <= len(longest):
            add("ragged%d" % m, plant(rng, cut(m), k, "mix", have, k))
    if len(lacks) and len(longest) >= 24 + k:
        p = cut(24 + k)
        p[rng.choice(len(p), size=k + 1, replace=False)] = int(lacks[-1]) + OFFSET          # k + 1 lacking characters: no result
        add("lacks_too_many", p)
    for _ in range(6):
        add("random", rng.choice(have, size=max(k + 1, int(rng.integers(4, 30)))).astype(np.uint16) + OFFSET)
    return out


# ---- the builders of tests/test_gpu_leven_edges.py, on hamming_util's small corpora -------------------------------------------------

import hamming_util as hu          # noqa: E402

GEOMETRY_KS = (1, 2, 3, 7)
GEOMETRY_MS = (7, 8, 9, 15, 16, 17, 63, 64, 65)          # and k + 1


def _rng(*what):
    return np.random.default_rng(zlib.crc32(" ".join(str(w) for w in ("leven edges",) + what).encode()))


def edit_at(rng, p, op, i, have):
    """p with one edit at position i: "sub" another letter there, "del" the symbol removed, "ins" a letter put in front of it"""
    p = [int(v) for v in p]
    i = min(i, len(p) - 1)
    if op == "sub":
        p[i] = int(rng.choice(have[have != p[i] - OFFSET])) + OFFSET
    elif op == "del":
        del p[i]
    else:
        p.insert(i, int(rng.choice(have)) + OFFSET)
    return p


def geometry_plants(m, k):
    """[(tag, [(op, position)])] for a cut of m symbols, the positions descending so that an edit does not move the ones behind it:
    none; an insertion, a deletion and a substitution at 0, 7, 8 and m - 1; on either side of every piece seam; one edit in each of
    pieces 0 .. j - 1 for every j; an edit in every piece"""
    b = pieces(m, k)
    ops = ("ins", "del", "sub")
    out = [("exact", [])]
    for i in sorted({0, 7, 8, m - 1}):
        if i < m:
            out += [("%s_at%d" % (op, i), [(op, i)]) for op in ops]
    for j in range(1, k + 1):
        out += [("seam%d_%s" % (j, side), [(ops[(j + n) % 3], at)]) for n, (side, at) in enumerate((("left", b[j][0] - 1), ("right", b[j][0])))]
    for j in range(1, k + 1):
        out.append(("owner%d" % j, [(ops[i % 3], b[i][0] if i % 2 == 0 else b[i][1] - 1) for i in reversed(range(j))]))
    out.append(("every_piece", [(ops[i % 3], b[i][0]) for i in reversed(range(k + 1))]))
    return out


def geometry_batch(docs, k):
    """[(tag, codes)]: for every m, 64 cuts -- text offsets of every residue modulo 8, each at every residue of its first symbol in
    the batch (fillers of k + 1 .. k + 8 symbols, cuts themselves, move it there) -- with geometry_plants(m, k) in turn.  A planted
    pattern keeps more than k symbols"""
    docs = hu._as_arrays(docs)
    rng = _rng("geometry", k)
    bases = [0, len(docs[0]) + 1]
    out, total = [], 0
    for m in sorted({k + 1} | set(GEOMETRY_MS)):
        if m <= k:
            continue
        plants = geometry_plants(m, k)
        n = 0
        for r in range(8):
            for a in range(8):
                f = (a - total) & 7
                if f:
                    length = k + 1 + ((f - k - 1) & 7)
                    d = docs[n % 2]
                    at = hu._cut_at(rng, d, length)
                    out.append(("filler%d" % length, codes(d[at:at + length])))
                    total += length
                tag, edits = plants[n % len(plants)]
                d = docs[(n // len(plants)) % 2]
                at = hu._cut_at(rng, d, m, r, bases[(n // len(plants)) % 2])
                p = codes(d[at:at + m])
                for op, i in edits:
                    if op != "del" or len(p) - 1 > k:
                        p = edit_at(rng, p, op, i, hu.ACGT)
                p = np.asarray(p, dtype=np.uint16)
                out.append(("m%d_%s_r%d_a%d" % (m, tag, r, a), p))
                total += len(p)
                n += 1
    return out


def bounds_patterns(docs, k, m=24):
    """[(tag, codes, offset, cost at most)] on letters of acgt: the pattern's front hangs off the text's start by f = 1 and k symbols
    (a later piece is found at the text's first letters; offset 0 is a result when the front can be deleted within k, and is not
    with k + 1 hanging); its back hangs over the last document's end likewise; the first and the last window themselves"""
    docs = hu._as_arrays(docs)
    text = prepared(docs)
    n = len(text)
    rng = _rng("bounds", k)
    letters = lambda count: codes(hu.ACGT[rng.integers(0, 4, count)])          # noqa: E731
    out = []
    for f in sorted({1, k, k + 1}):
        out.append(("front_hangs_%d" % f, np.concatenate([letters(f), text[:m - f]]), 0, f if f <= k else None))
        out.append(("back_hangs_%d" % f, np.concatenate([text[n - 1 - (m - f):n - 1], letters(f)]), n - 1 - (m - f), f if f <= k else None))
    out.append(("window_0", text[:m].copy(), 0, 0))
    out.append(("window_last", text[n - 1 - m:n - 1].copy(), n - 1 - m, 0))
    return out


LARGE_KS = (15, 16, 30, 31)


def large_k_batch(docs, k):
    """[(tag, codes)]: cuts of k + 1, k + 2, 2k + 1 and 300 letters with 0, 1, k and k + 1 edits planted, and a pattern of a letter
    the text lacks"""
    docs = hu._as_arrays(docs)
    rng = _rng("large k", k)
    out = []
    for m in sorted({k + 1, k + 2, 2 * k + 1, 300}):
        for nedits in (0, 1, k, k + 1):
            at = hu._cut_at(rng, docs[0], m)
            out.append(("cut%d_%d" % (m, nedits), plant(rng, codes(docs[0][at:at + m]), nedits, "mix", hu.ACGT, k)))
    out.append(("lacking", codes(b"n" * (k + 4))))
    return out


def long_batch(doc, k=31, m=MAX_PATTERN, at=200):
    """cuts of the longest pattern with 0, k and k + 1 other letters planted, and one deletion with k - 1 (doc: letters of acgt)"""
    rng = _rng("long", k, m)
    have = np.unique(doc)
    p = codes(doc[at:at + m])
    out = [("long_%d" % nsub, hu._differ(rng, p, rng.choice(m, size=nsub, replace=False), have)) for nsub in (0, k, k + 1)]
    q = np.concatenate([p[:m // 3], p[m // 3 + 1:], codes(doc[at + m:at + m + 1])])          # one symbol removed, the next of the text appended
    out.append(("long_deletion", hu._differ(rng, q, rng.choice(m // 4, size=k - 1, replace=False), have)))
    return out


def lacking_opposite(docs, k, m=24):
    """[(tag, codes)] on an alphabet corpus: the lacking byte opposite every distinct byte of the text in turn, and twice"""
    docs = hu._as_arrays(docs)
    rng = _rng("lacking", k)
    have = np.unique(np.concatenate(docs))
    lack = int(np.setdiff1d(np.arange(256), have)[0]) + OFFSET
    out = []
    for n, c in enumerate(have):
        i = n % m
        for d in docs:
            at = np.nonzero(d == c)[0]
            at = at[(at >= i) & (at - i + m <= len(d))]
            if len(at):
                p = codes(d[at[0] - i:at[0] - i + m])
                p[i] = lack
                out.append(("opposite_%d_%d" % (c, i), p))
                break
    at = hu._cut_at(rng, docs[0], m)
    p = codes(docs[0][at:at + m])
    p[[3, 17]] = lack
    out.append(("two_lacking", p))
    return out


# ---- the route of femto_amd/leven/leven.hip, in Python ------------------------------------------------------------------------------

def extend(k, mp, budget, pat, text, reached):
    """One extension, statement for statement the kernel's: diagonal-wise and furthest-reaching over one row of 2 k + 3 entries
    updated in place (entry k + 1 + d: the furthest pattern row on diagonal d, plus one; 0 = not reached).  pat(i): the i-th of mp
    pattern symbols; text(x): the x-th text symbol in the direction of the extension, 0 where the text ends; reached(e, d) -> stop"""
    base = k + 1
    row = [0] * (2 * k + 3)
    i = 0
    while i < mp and pat(i) == text(i):
        i += 1
    row[base] = i + 1
    if i == mp and reached(0, 0):
        return
    for e in range(1, budget + 1):
        left = -1
        for d in range(-e, e + 1):
            cur, right = row[base + d] - 1, row[base + d + 1] - 1
            i = cur
            if 0 <= cur < mp and text(cur + d) >= OFFSET:
                i = cur + 1
            if left > i:
                c = left if text(left + d - 1) >= OFFSET else left - 1
                if c > i:
                    i = c
            if right >= 0:
                c = right + 1 if right < mp else mp
                if c > i and c + d >= 0:
                    i = c
            left = cur
            if i == cur:
                continue
            while i < mp and pat(i) == text(i + d):
                i += 1
            row[base + d] = i + 1
            if i == mp and reached(e, d):
                return


def route(text, pattern, k):
    """the seeds-and-two-extensions route: (raw records [(offset, cost, length)], candidates).  Every occurrence of every piece is a
    seed; the right extension gives cr and tr, the left one a record for every t with cl(t) + cr <= k"""
    p = [int(v) for v in pattern]
    t = [int(v) for v in text]
    m, n = len(p), len(t)
    at = lambda pos: t[pos] if 0 <= pos < n else 0          # noqa: E731
    raw, cands = [], 0
    for b0, b1 in pieces(m, k):
        piece = np.asarray(p[b0:b1], dtype=text.dtype)
        hits = np.nonzero((np.lib.stride_tricks.sliding_window_view(text, b1 - b0) == piece).all(axis=1))[0] if b1 - b0 <= n else []
        for o in (int(h) for h in hits):
            cands += 1
            right = []

            def arrived(e, d):
                right.append((e, m - b1 + d))
                return True
            extend(k, m - b1, k, lambda i: p[b1 + i], lambda x: at(o + b1 - b0 + x), arrived)
            if not right:
                continue
            cr, tr = right[0]

            def record(e, d):
                raw.append((o - (b0 + d), e + cr, b0 + d + (b1 - b0) + tr))
                return False
            extend(k, b0, k - cr, lambda i: p[b0 - 1 - i], lambda x: at(o - 1 - x), record)
    return raw, cands


def route_answer(text, pattern, k):
    """the least (cost, length) of every offset's raw records, as occurrences() lists them"""
    raw, _ = route(text, pattern, k)
    best = {}
    for o, c, length in raw:
        assert 0 <= c <= k and len(pattern) - k <= length <= len(pattern) + k
        best[o] = min(best.get(o, (c, length)), (c, length))
    offs = sorted(best)
    return (np.array(offs, dtype=np.int64), np.array([best[o][0] for o in offs], dtype=np.int32),
            np.array([best[o][1] for o in offs], dtype=np.int32))
