"""The question of include/femto_amd.h "search with substitutions", restated in plain numpy over a fixture's documents, and the
pattern set the tests of it share (tests/test_mismatch_host.py pins both to the CPU oracle, tests/test_gpu_mismatch.py runs them).

THE RULE.  The pattern slides over the PREPARED TEXT -- every document's bytes + 5 followed by SEOF (Fixture.prepared_text), not
cyclic -- and a window is kept when
  * at every position of the pattern that is not substitutable (a code outside [5, 261)) the window holds the pattern's code,
  * at every substitutable position the window holds the pattern's code or another BYTE code (SEOF is no substitute: a window
    that runs over a document's end survives only where the pattern itself holds SEOF there), and
  * at most k positions differ.
The distinct kept windows are the variants with a non-empty range; a window's multiplicity is last - first + 1.  A pattern of
bytes alone therefore never matches across a document end, and a pattern that ENDS in SEOF matches where documents end -- as it
does for parallel_count.  (The index orders the documents' SEOF rows by document, not by what follows them, so a backward search
THROUGH a SEOF does not land on the text that precedes it in the prepared text: parallel_count itself does not find the end of one
document joined to the start of the next.  The pattern set therefore holds SEOF at a pattern's end, and inside a pattern only
where the yardstick and parallel_count agree that nothing matches.)  The variants of one pattern have one length, so their order by `first` is the lexicographic order of
their alpha codes: the yardstick orders them so, without knowing a row."""
import zlib
from collections import namedtuple

import numpy as np

SEOF, OFFSET, ALPHA, MAX_PATTERN = 2, 5, 261, 32768
Variant = namedtuple("Variant", "symbols rows subs")      # uint16[m], windows, ((position, substitute), ...) ascending


def prepared(docs):
    parts = []
    for d in docs:
        b = np.frombuffer(d, dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else np.asarray(d, dtype=np.uint8)
        parts += [b.astype(np.uint16) + OFFSET, np.array([SEOF], dtype=np.uint16)]
    return np.concatenate(parts)


def variants(text, pattern, k=2):
    """[Variant] of `pattern` (alpha codes) in `text` (prepared) with at most k substitutions, in lexicographic order"""
    p = np.asarray(pattern, dtype=np.uint16)
    m, n = len(p), len(text)
    if m == 0:
        return [Variant(p, n, ())]
    if m > n:
        return []
    sub = (p >= OFFSET) & (p < ALPHA)
    cand = np.arange(n - m + 1)
    diff = np.zeros(len(cand), dtype=np.int64)
    for j in range(m):          # column by column: the candidates thin out after a few
        col = text[cand + j]
        neq = col != p[j]
        diff = diff + neq
        keep = (diff <= k) & (~neq | (col >= OFFSET)) if sub[j] else ~neq
        cand, diff = cand[keep], diff[keep]
        if len(cand) == 0:
            return []
    uniq, rows = np.unique(text[cand[:, None] + np.arange(m)], axis=0, return_counts=True)
    return [Variant(v, int(c), tuple((int(i), int(v[i])) for i in np.nonzero(v != p)[0])) for v, c in zip(uniq, rows)]


def expected(all_variants, k):
    """the call's answer but for the rows, from variants(.., 2) of every pattern: (result_start, the variants in result order,
    cost int32[], sub_pos int32[total, 2], sub_sym uint16[total, 2])"""
    start, flat = [0], []
    for vs in all_variants:
        flat += [v for v in vs if len(v.subs) <= k]
        start.append(len(flat))
    t = len(flat)
    cost = np.array([len(v.subs) for v in flat], dtype=np.int32)
    pos, sym = np.full((t, 2), -1, dtype=np.int32), np.zeros((t, 2), dtype=np.uint16)
    for r, v in enumerate(flat):
        for s, (i, c) in enumerate(v.subs):
            pos[r, s], sym[r, s] = i, c
    return np.array(start, dtype=np.int64), flat, cost, pos, sym


def pattern_set(docs, name):
    """[(tag, uint16 alpha codes)]: about 300 patterns of mixed lengths -- the cases the header names, then cuts of the text with
    0..2 substitutions planted.  Deterministic per fixture name."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    docs = [np.asarray(d, dtype=np.uint8) for d in docs]
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    longest = max(docs, key=len)
    shortest = min(len(d) for d in docs)
    out = []

    def add(tag, p):
        out.append((tag, np.asarray(p, dtype=np.uint16)))

    def cut(length, doc=None):
        """`length` consecutive bytes of a document as alpha codes; random characters of the text when no document is that long"""
        d = longest if doc is None else doc
        if len(d) < length:
            return rng.choice(have, size=length).astype(np.uint16) + OFFSET
        at = int(rng.integers(0, len(d) - length + 1))
        return d[at:at + length].astype(np.uint16) + OFFSET

    def other(sym):
        """a character of the text other than `sym` (alpha codes)"""
        c = have[have != int(sym) - OFFSET] if OFFSET <= int(sym) < ALPHA else have
        return int(rng.choice(c)) + OFFSET if len(c) else int(sym)

    def planted(p, at):
        p = p.copy()
        for i in at:
            p[i] = other(p[i])
        return p

    add("empty", [])
    for length in (1, 2, 20, 64, 65):
        add("len%d" % length, cut(length))
    if shortest + 1 <= MAX_PATTERN:      # longer than the shortest document: no window inside it (acgt48k's one document is longer than a pattern may be)
        add("long", cut(shortest + 1) if len(longest) > shortest else np.concatenate([cut(shortest), cut(1)]))
    m = min(20, len(longest))
    base = cut(m)
    first, mid, last = 0, m // 2, m - 1
    add("cut", base)
    for tag, at in (("first", [first]), ("mid", [mid]), ("last", [last]), ("first_last", [first, last]), ("first_mid", [first, mid]),
                    ("mid_last", [mid, last])):
        add("planted_" + tag, planted(base, at))
    if len(docs) > 1:
        add("straddle", np.concatenate([docs[0][-6:], docs[1][:6]]).astype(np.uint16) + OFFSET)
        add("seof_end", np.concatenate([docs[0][-5:].astype(np.uint16) + OFFSET, [SEOF]]))
    add("seof_end", np.concatenate([longest[-8:].astype(np.uint16) + OFFSET, [SEOF]]))
    for _ in range(200):      # SEOF inside: in front of bytes that no document starts with, not even with three of them changed
        tail = cut(min(10, len(longest)))
        if all(len(d) < len(tail) or int((d[:len(tail)].astype(np.uint16) + OFFSET != tail).sum()) >= 3 for d in docs):
            add("seof_inside", np.concatenate([base[:m // 2], [SEOF], tail]))
            break
    if len(lacks):          # (bytes256 holds every byte)
        n1 = int(lacks[0]) + OFFSET
        n2 = int(lacks[-1]) + OFFSET
        for tag, at in (("first", [first]), ("mid", [mid]), ("last", [last]), ("two", [first, last]), ("three", [first, mid, last])):
            p = cut(m)
            for i, c in zip(at, (n1, n2, n1)):
                p[i] = c
            add("lacks_" + tag, p)
    for r in range(20):
        add("random", rng.integers(0, 256, size=int(rng.integers(1, 25))).astype(np.uint16) + OFFSET)
    add("twice", out[8][1])
    add("twice", out[8][1])
    while len(out) < 300:
        p = cut(int(rng.integers(3, 41)))
        nsub = int(rng.integers(0, 3))
        add("cut%d" % nsub, planted(p, rng.choice(len(p), size=min(nsub, len(p)), replace=False)))
    return out


# ---- past the fixtures: what tests/test_gpu_mismatch_edges.py and the full-size case run, and tests/test_mismatch_host.py pins ----

def as_arrays(docs):
    """the documents as uint8 arrays (a corpus of tests/corpus_util.py holds bytes or arrays)"""
    return [np.frombuffer(bytes(d), dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else np.asarray(d, dtype=np.uint8) for d in docs]


def _other(rng, have, sym):
    c = have[have != int(sym) - OFFSET]
    return int(rng.choice(c)) + OFFSET if len(c) else int(sym)


def seof_family(docs, name):
    """[(tag, pattern)] that END in SEOF (never hold it elsewhere: the module's docstring): SEOF alone, [c, SEOF] for every byte
    character c of the text and one it lacks, the last 1, 2, 5 and 12 bytes of ten documents as they are and with 1 and 2
    substitutions planted, three whole tiny documents"""
    rng = np.random.default_rng(zlib.crc32(("seof " + name).encode()))
    docs = as_arrays(docs)
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    end = np.array([SEOF], dtype=np.uint16)
    out = [("seof_alone", end)]
    for c in list(have) + [int(lacks[0])]:
        out.append(("seof_after_%d" % c, np.array([int(c) + OFFSET, SEOF], dtype=np.uint16)))
    ten = rng.choice([i for i, d in enumerate(docs) if len(d) >= 12], 10, replace=False)
    for i in ten:
        for n in (1, 2, 5, 12):
            tail = docs[i][-n:].astype(np.uint16) + OFFSET
            for nsub in (0, 1, 2):
                p = tail.copy()
                for at in rng.choice(n, size=min(nsub, n), replace=False):
                    p[at] = _other(rng, have, p[at])
                out.append(("seof_tail%d_%d" % (n, nsub), np.concatenate([p, end])))
    tiny = [i for i, d in enumerate(docs) if 1 <= len(d) <= 3]
    for i in (tiny + [int(np.argmin([len(d) if len(d) else 1 << 30 for d in docs]))] * 3)[:3]:
        out.append(("seof_whole", np.concatenate([docs[i].astype(np.uint16) + OFFSET, end])))
    return out


def corpus_pattern_set(docs, name):
    """pattern_set of a built corpus, then its SEOF family"""
    return pattern_set(as_arrays(docs), name) + seof_family(docs, name)


# two texts of one and of two byte characters (the second with an empty document), and every string over a, b and c -- which
# neither holds -- of 1 .. 5 symbols, bare and with SEOF behind it, and the empty pattern
TINY_TEXTS = {"one": [b"aaaaaaa", b"aaa"], "two": [b"abba", b"", b"ab", b"bbbb"]}
TINY_MAX = 5


def tiny_patterns():
    abc = np.frombuffer(b"abc", dtype=np.uint8).astype(np.uint16) + OFFSET
    bare = []
    for m in range(1, TINY_MAX + 1):
        for i in range(3 ** m):
            bare.append(abc[[(i // 3 ** j) % 3 for j in range(m)]])
    return bare + [np.concatenate([p, [SEOF]]).astype(np.uint16) for p in bare] + [np.zeros(0, dtype=np.uint16)]


LONG_CUTS = (MAX_PATTERN, MAX_PATTERN - 1, 4097)


def long_patterns(doc):
    """[(tag, pattern, planted positions)]: cuts of `doc` (uint8, longer than MAX_PATTERN) of 32768, 32767 and 4097 symbols with
    other byte characters of the document planted at {last}, {0}, {0, last}, {last - 1, last} and, where the cut is that long,
    {16383, 16384}; then one untouched cut of 32768 symbols"""
    rng = np.random.default_rng(32768)
    doc = np.asarray(doc, dtype=np.uint8)
    have = np.unique(doc)
    out = []
    for m in LONG_CUTS:
        last = m - 1
        for at in ((last,), (0,), (0, last), (last - 1, last), (16383, 16384)):
            if at[-1] > last:
                continue
            s = int(rng.integers(0, len(doc) - m + 1))
            p = doc[s:s + m].astype(np.uint16) + OFFSET
            for i in at:
                p[i] = _other(rng, have, p[i])
            out.append(("long%d_%s" % (m, "_".join(map(str, at))), p, at))
    s = int(rng.integers(0, len(doc) - MAX_PATTERN + 1))
    out.append(("long%d_untouched" % MAX_PATTERN, doc[s:s + MAX_PATTERN].astype(np.uint16) + OFFSET, ()))
    return out


# the front of the full-size case: 255 patterns of 32768 random bytes and one of 32765.  Over a text of 256 byte characters they
# are 2^31 - 768 lanes of the substitution pass (one per symbol and substitute), so lane 2^31 = 256 * (FRONT_SYMS + 3) is the first
# lane of the FOURTH symbol behind them.
FRONT_PATTERNS, FRONT_SHORT_BY = 256, 3
FRONT_SYMS = FRONT_PATTERNS * MAX_PATTERN - FRONT_SHORT_BY


def fullsize_front():
    rng = np.random.default_rng(1 << 31)
    lens = [MAX_PATTERN] * (FRONT_PATTERNS - 1) + [MAX_PATTERN - FRONT_SHORT_BY]
    return [rng.integers(0, 256, size=n).astype(np.uint16) + OFFSET for n in lens]
