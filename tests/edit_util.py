"""The question of include/femto_amd.h "search within edit distance", restated in plain numpy over a fixture's documents, and the
pattern set the tests of it share (tests/test_edit_host.py pins both to a plain dynamic programme and to the CPU oracle,
tests/test_gpu_edit.py runs them).

THE RULE.  The pattern p of m symbols is aligned against every window of the PREPARED TEXT (mismatch_util.prepared: every
document's bytes + 5 followed by SEOF, not cyclic) that starts at s: D[i][j] = the fewest operations that turn p[:i] into
text[s:s + j], where
  * a match costs 0,
  * a substitution costs 1 and needs both codes to be bytes (codes in [5, 261)),
  * a deletion (of p[i - 1]) costs 1 and needs a byte pattern symbol,
  * an insertion (of text[s + j - 1] behind p[:i]) costs 1 and needs a byte text symbol and i == 0 or p[i - 1] >= 5.
Behind its end the text is padded with a code that matches nothing.  Only the band |i - j| <= k matters; a start is dropped once
the column's minimum exceeds k, and the prefix of length j is kept whenever D[m][j] <= k.  Equal strings are merged: their cost
(it depends on the string alone) and the number of their windows, which is last - first + 1.  The strings are ordered
lexicographically with a prefix in front of its extensions: the order of (first, length), without knowing a row.  Computed with
k = 2 a cost <= 2 is exact, so the answer for a smaller bound is the strings of at most that cost."""
import zlib
from collections import namedtuple

import numpy as np

import mismatch_util as mu
from mismatch_util import ALPHA, OFFSET, SEOF, prepared      # noqa: F401 (prepared: for the tests that import it from here)

Variant = namedtuple("Variant", "symbols rows cost")      # uint16[length], windows, fewest operations
PAD, INF = 0xFFFF, 99


def _is_byte(a):
    return (a >= OFFSET) & (a < ALPHA)


def variants(text, pattern, k=2):
    """[Variant] of `pattern` (alpha codes) in `text` (prepared) within k operations, in lexicographic order, a prefix first"""
    p = np.asarray(pattern, dtype=np.int64)
    m, n = len(p), len(text)
    padded = np.concatenate([np.asarray(text, dtype=np.int64), np.full(m + k + 1, PAD, dtype=np.int64)])
    pbyte = _is_byte(p)
    may_insert = np.ones(m + 1, dtype=bool)      # behind p[:i]
    may_insert[1:] = p >= OFFSET
    width = 2 * k + 1      # band cell b of column j is row i = j + b - k
    cand = np.arange(n)
    col = np.full((n, width), INF, dtype=np.int64)
    for b in range(width):      # column 0: p[:i] deleted whole
        i = b - k
        if 0 <= i <= m and pbyte[:i].all():
            col[:, b] = i
    found = []      # (length, starts, costs)
    if m <= k and col[0, m + k] <= k:
        found.append((0, cand, col[:, m + k]))
    for j in range(1, m + k + 1):
        t = padded[cand + j - 1]
        tbyte = _is_byte(t)
        new = np.full((len(cand), width), INF, dtype=np.int64)
        for b in range(width):
            i = j + b - k
            if i < 0 or i > m:
                continue
            best = np.full(len(cand), INF, dtype=np.int64)
            if i >= 1:      # match or substitution
                step = np.where(t == p[i - 1], 0, np.where(tbyte & pbyte[i - 1], 1, INF))
                best = np.minimum(best, col[:, b] + step)
            if b + 1 < width and may_insert[i]:      # insertion of t behind p[:i]
                best = np.minimum(best, np.where(tbyte, col[:, b + 1] + 1, INF))
            if i >= 1 and b >= 1 and pbyte[i - 1]:      # deletion of p[i - 1]
                best = np.minimum(best, new[:, b - 1] + 1)
            new[:, b] = np.minimum(best, INF)
        keep = new.min(axis=1) <= k
        cand, col = cand[keep], new[keep]
        if len(cand) == 0:
            break
        bm = m - j + k
        if 0 <= bm < width:
            hit = col[:, bm] <= k
            if hit.any():
                found.append((j, cand[hit], col[hit, bm]))
    out = []
    for length, starts, costs in found:
        if length == 0:
            out.append(Variant(np.zeros(0, dtype=np.uint16), n, int(costs[0])))
            continue
        win = padded[starts[:, None] + np.arange(length)]
        uniq, index, rows = np.unique(win, axis=0, return_index=True, return_counts=True)
        out += [Variant(v.astype(np.uint16), int(c), int(costs[i])) for v, i, c in zip(uniq, index, rows)]
    out.sort(key=lambda v: tuple(v.symbols.tolist()))
    return out


def expected(all_variants, k):
    """the call's answer but for the rows, from variants(.., 2) of every pattern: (result_start, the variants in result order,
    cost int32[], length int32[])"""
    start, flat = [0], []
    for vs in all_variants:
        flat += [v for v in vs if v.cost <= k]
        start.append(len(flat))
    return (np.array(start, dtype=np.int64), flat, np.array([v.cost for v in flat], dtype=np.int32),
            np.array([len(v.symbols) for v in flat], dtype=np.int32))


def plain_distance(p, w):
    """the rule as a plain dynamic programme over one pattern and one string (no band, no numpy)"""
    p, w = [int(c) for c in p], [int(c) for c in w]
    byte = lambda c: OFFSET <= c < ALPHA
    m, n = len(p), len(w)
    D = [[INF] * (n + 1) for _ in range(m + 1)]
    D[0][0] = 0
    for i in range(m + 1):
        for j in range(n + 1):
            if i and j and (p[i - 1] == w[j - 1] or (byte(p[i - 1]) and byte(w[j - 1]))):
                D[i][j] = min(D[i][j], D[i - 1][j - 1] + (p[i - 1] != w[j - 1]))
            if i and byte(p[i - 1]):
                D[i][j] = min(D[i][j], D[i - 1][j] + 1)
            if j and byte(w[j - 1]) and (i == 0 or p[i - 1] >= OFFSET):
                D[i][j] = min(D[i][j], D[i][j - 1] + 1)
    return D[m][n]


def plain_variants(text, pattern, k):
    """[(symbols tuple, windows, cost)] in result order, from plain_distance over every distinct substring of the text"""
    t = [int(c) for c in text]
    m = len(pattern)
    count = {}
    for length in range(max(0, m - k), m + k + 1):
        for s in range(len(t) - length + 1 if length else len(t)):
            w = tuple(t[s:s + length])
            count[w] = count.get(w, 0) + 1
    out = []
    for w, c in count.items():
        d = plain_distance(pattern, w)
        if d <= k:
            out.append((w, c, d))
    return sorted(out)


def tiny_patterns(longest=4):
    """every string over a, b and c of 1 .. `longest` symbols, bare and with SEOF behind it, and the empty pattern"""
    abc = np.frombuffer(b"abc", dtype=np.uint8).astype(np.uint16) + OFFSET
    bare = []
    for m in range(1, longest + 1):
        for i in range(3 ** m):
            bare.append(abc[[(i // 3 ** j) % 3 for j in range(m)]])
    return bare + [np.concatenate([p, [SEOF]]).astype(np.uint16) for p in bare] + [np.zeros(0, dtype=np.uint16)]


KEPT_TAGS = ("empty", "len", "long", "straddle", "seof_end", "lacks_", "random", "twice")


def pattern_set(docs, name):
    """[(tag, uint16 alpha codes)]: about 120 patterns -- the cases of mismatch_util.pattern_set that the header names (but for SEOF
    inside a pattern, which an insertion or a deletion can bring to where the yardstick and parallel_count disagree), then cuts
    of the text of 3 .. 40 symbols with a deletion, an insertion, both, two deletions, two insertions in one gap, an edit at the
    first and at the last symbol planted -- the cut itself occurs, so every one of them has a result -- and a cut from inside the
    longest run of one character.  Deterministic per fixture name."""
    rng = np.random.default_rng(zlib.crc32(("edit " + name).encode()))
    docs = [np.asarray(d, dtype=np.uint8) for d in docs]
    have = np.unique(np.concatenate(docs))
    longest = max(docs, key=len)
    out, randoms = [], 0
    for tag, p in mu.pattern_set(docs, name):
        if tag.startswith("cut") or tag.startswith("planted") or tag == "seof_inside" or not tag.startswith(KEPT_TAGS):
            continue
        if tag == "random":
            randoms += 1
            if randoms > 8:
                continue
        out.append((tag, p))

    def add(tag, p):
        out.append((tag, np.asarray(p, dtype=np.uint16)))

    def cut(length):
        length = min(length, len(longest))
        at = int(rng.integers(0, len(longest) - length + 1))
        return longest[at:at + length].astype(np.uint16) + OFFSET

    def some():
        return int(rng.choice(have)) + OFFSET

    def deleted(p, i):      # the text holds p: the pattern lacks p[i], an insertion away
        return np.delete(p, i)

    def inserted(p, i, n=1):      # the pattern holds n characters more in gap i: n deletions away
        return np.insert(p, i, [some() for _ in range(n)])

    # the run first: many scripts reach one string
    best_len, best = 0, None
    for d in docs:
        if len(d) == 0:
            continue
        edges = np.flatnonzero(np.diff(d) != 0)
        bounds = np.concatenate([[-1], edges, [len(d) - 1]])
        runs = np.diff(bounds)
        r = int(np.argmax(runs))
        if runs[r] > best_len:
            best_len, best = int(runs[r]), np.full(min(int(runs[r]), 6), int(d[bounds[r] + 1]), dtype=np.uint16) + OFFSET
    add("run", best)
    add("run_less", best[:max(1, len(best) - 1)])
    base = cut(12)
    add("edit_first_del", deleted(base, 0))
    add("edit_first_ins", inserted(base, 0))
    add("edit_last_del", deleted(base, len(base) - 1))
    add("edit_last_ins", inserted(base, len(base)))
    add("edit_last_sub", np.concatenate([base[:-1], [some()]]))
    kinds = ("del", "ins", "del_ins", "del_del", "ins_ins_gap", "sub_del", "none")
    at = 0
    while len(out) < 120:
        p = cut(int(rng.integers(3, 41)))
        kind = kinds[at % len(kinds)]
        at += 1
        i = int(rng.integers(0, len(p)))
        if kind == "del":
            p = deleted(p, i)
        elif kind == "ins":
            p = inserted(p, i)
        elif kind == "del_ins":
            p = inserted(deleted(p, i), int(rng.integers(0, len(p))))
        elif kind == "del_del":
            p = deleted(deleted(p, i), int(rng.integers(0, len(p) - 1)))
        elif kind == "ins_ins_gap":
            p = inserted(p, i, 2)
        elif kind == "sub_del":
            p[i] = some()
            p = deleted(p, int(rng.integers(0, len(p))))
        add("cut_" + kind, p)
    return out


# ---- past the fixtures: what tests/test_gpu_edit_edges.py and the full-size case run, and tests/test_edit_host.py pins ----------

PASSAGES = (2, 3, 4, 5)          # P3 .. P6 of corpus_util's "library": they stand in 64, 65, 150 and 300 documents
NOISE = 6                        # the symbols of group (d) that belong to one document alone


def _codes(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).astype(np.uint16) + OFFSET


def passage_patterns(lib):
    """[(tag, pattern)] of at most 60 symbols over the passages P3 .. P6 of `lib` (corpus_util.library_docs()); a tag is
    "P<n>_<group>_<what>".  The groups:
      a  the passage, a cut of 20 symbols from its middle and a seeded one;
      b  the two cuts and the passage's first 58 symbols with a deletion, an insertion, a substitution, del + ins, del + del, two
         insertions in one gap and sub + del planted at least 8 symbols from either end (as pattern_set plants them: `deleted` takes
         a symbol of the text's string out of the pattern, `inserted` puts a foreign one in);
      c  the middle cut with a deletion, an insertion and a substitution at its first and at its last symbol;
      d  NOISE symbols that stand in front of the passage in one document, then the passage's first 14: bare, with an edit to the
         right of that point, to the left of it, on both sides, and at the two symbols that meet there;
      e  the first 58 symbols with one character doubled, with two, and -- where the passage holds a run xx -- with the run
         shortened, alone and beside a doubled character;
      f  P3 and P5 whole with SEOF behind them (documents that are the passage and nothing else end them).
    Deterministic."""
    rng = np.random.default_rng(zlib.crc32(b"edit passages"))
    letters = np.unique(np.concatenate([_codes(d) for d in lib.docs]))
    out = []

    def add(tag, p):
        p = np.asarray(p, dtype=np.uint16)
        assert len(p) <= 60, tag
        out.append((tag, p))

    def other(c):
        return int(rng.choice(letters[letters != int(c)]))

    def planted(p, kind, lo, hi):
        """`kind` planted in p at seeded positions of [lo, hi)"""
        i = int(rng.integers(lo, hi))
        if kind == "del":
            return np.delete(p, i)
        if kind == "ins":
            return np.insert(p, i, other(p[i]))
        if kind == "sub":
            q = p.copy()
            q[i] = other(p[i])
            return q
        if kind == "del_ins":
            q = np.delete(p, i)
            j = int(rng.integers(lo, hi - 1))
            return np.insert(q, j, other(q[j]))
        if kind == "del_del":
            return np.delete(np.delete(p, i), int(rng.integers(lo, hi - 1)))
        if kind == "ins_ins_gap":
            return np.insert(p, i, [other(p[i]), other(p[i - 1])])
        assert kind == "sub_del"
        q = p.copy()
        q[i] = other(p[i])
        return np.delete(q, int(rng.integers(lo, hi)))

    for k in PASSAGES:
        name = "P%d" % (k + 1)
        whole = _codes(lib.passages[k])
        n = len(whole)
        mid = whole[(n - 20) // 2:(n - 20) // 2 + 20]
        at = int(rng.integers(0, n - 20 + 1))
        cut = whole[at:at + 20]
        head = whole[:58]
        add(name + "_a_whole", whole)
        add(name + "_a_mid", mid)
        add(name + "_a_cut", cut)
        for what, base in (("mid", mid), ("cut", cut), ("head", head)):
            for kind in ("del", "ins", "sub", "del_ins", "del_del", "ins_ins_gap", "sub_del"):
                add("%s_b_%s_%s" % (name, what, kind), planted(base, kind, 8, len(base) - 8))
        for kind in ("del", "ins", "sub"):
            add("%s_c_first_%s" % (name, kind), planted(mid, kind, 0, 1))
            add("%s_c_last_%s" % (name, kind), planted(mid, kind, 19, 20))
        add(name + "_c_ins_behind", np.concatenate([mid, [other(0)]]))
        # d: the first document that holds the passage once, NOISE bytes or more from its start
        d = next(b for b in lib.docs if bytes(b).count(lib.passages[k]) == 1 and bytes(b).find(lib.passages[k]) >= NOISE)
        s = bytes(d).find(lib.passages[k])
        fall = np.concatenate([_codes(bytes(d)[s - NOISE:s]), whole[:14]])
        add(name + "_d_bare", fall)
        add(name + "_d_right_del", np.delete(fall, NOISE + 6))
        add(name + "_d_right_ins", np.insert(fall, NOISE + 6, other(fall[NOISE + 6])))
        add(name + "_d_left_sub", np.concatenate([fall[:2], [other(fall[2])], fall[3:]]))
        add(name + "_d_left_del", np.delete(fall, 2))
        add(name + "_d_both", np.delete(np.insert(fall, NOISE + 6, other(fall[NOISE + 6])), 2))
        add(name + "_d_at_del", np.delete(fall, NOISE - 1))
        add(name + "_d_at_del_del", np.delete(fall, [NOISE - 1, NOISE]))
        # e: runs
        i, j = int(rng.integers(8, len(head) // 2 - 2)), int(rng.integers(len(head) // 2 + 2, len(head) - 8))
        add(name + "_e_doubled", np.insert(head, i, head[i]))
        add(name + "_e_doubled_twice", np.insert(np.insert(head, j, head[j]), i, head[i]))
        runs = np.flatnonzero(head[1:] == head[:-1])
        if len(runs):
            r = int(runs[len(runs) // 2])
            add(name + "_e_shortened", np.delete(head, r))
            far = j if abs(j - r) > 3 else i
            add(name + "_e_shortened_doubled", np.delete(np.insert(head, far, head[far]), r + (far < r)))
    for k in (2, 4):
        add("P%d_f_seof" % (k + 1), np.concatenate([_codes(lib.passages[k]), [SEOF]]))
    return out


def corpus_pattern_set(docs, name):
    """pattern_set of a built corpus, then mismatch_util's SEOF family (patterns that END in SEOF, whole tiny documents with SEOF
    behind them, SEOF alone: none with SEOF inside) and, for "library", passage_patterns"""
    out = pattern_set(mu.as_arrays(docs), name) + mu.seof_family(docs, name)
    if name == "library":
        import corpus_util as cu
        out += passage_patterns(cu.library_docs())
    return out


def repeated(nbase, npat, seed):
    """int64[npat]: seeded permutations of range(nbase) one after another, so that a boundary every 256 patterns does not land on
    the same base pattern each time"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(nbase) for _ in range(-(-npat // nbase))])[:npat].astype(np.int64)


def cap_patterns(doc):
    """[(tag, pattern)] at the cap, from `doc` (uint8, longer than 32770): a 32768-symbol cut with one deletion and one insertion
    planted far apart (so still 32768 long), the cut untouched -- with text on either side, so that insertions in front of and
    behind it give strings of 32769 and 32770 symbols -- and a 32767-symbol cut"""
    doc = np.asarray(doc, dtype=np.uint8)
    assert len(doc) > mu.MAX_PATTERN + 40
    have = np.unique(doc)
    cut = doc[20:20 + mu.MAX_PATTERN].astype(np.uint16) + OFFSET
    foreign = int(have[have != int(cut[24000]) - OFFSET][0]) + OFFSET
    planted = np.insert(np.delete(cut, 8000), 24000, foreign)
    assert len(planted) == mu.MAX_PATTERN and not np.array_equal(planted, cut)
    return [("cap_planted", planted), ("cap_untouched", cut), ("cap_less_one", doc[31:31 + mu.MAX_PATTERN - 1].astype(np.uint16) + OFFSET)]


# The front of the full-size case.  On a text of 256 byte characters a site has 2 * 256 + 1 = 513 lanes, and lane 2^31 =
# 513 * 4 186 127 + 497 is lane 497 of site 4 186 127: the substitution by substitute 497 - 256 = 241.  A pattern of m symbols has
# m + 1 sites, so 127 patterns of 32768 random bytes and one of 24447 are FRONT_SITES = 4 186 111 sites, and the lane stands in site
# FRONT_BEHIND = 16 behind them.
EDIT_LANES = 513
FRONT_LENS = (mu.MAX_PATTERN,) * 127 + (24447,)
FRONT_SITES = sum(FRONT_LENS) + len(FRONT_LENS)
FRONT_BEHIND, FRONT_EDIT = divmod(1 << 31, EDIT_LANES)[0] - FRONT_SITES, (1 << 31) % EDIT_LANES


def fullsize_front():
    rng = np.random.default_rng((1 << 31) + 513)
    return [rng.integers(0, 256, size=n).astype(np.uint16) + OFFSET for n in FRONT_LENS]
