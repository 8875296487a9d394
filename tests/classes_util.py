"""The question of include/femto_amd.h "search with character classes", restated in plain numpy over a fixture's documents, and the
pattern set the tests of it share (tests/test_classes_host.py pins both to the committed reference results and to the CPU oracle,
tests/test_gpu_classes.py runs them).

THE RULE.  The pattern slides over the PREPARED TEXT -- every document's bytes + 5 followed by SEOF (mismatch_util.prepared), not
cyclic -- and a window is kept when at every literal position it holds the pattern's code and at every class position a byte code
whose byte the class holds.  Classes hold bytes alone, so a window that runs over a document's end survives only where the pattern
itself holds SEOF there, and that is at a pattern's END alone (mismatch_util's docstring says why).  The distinct kept windows are
the results; a window's multiplicity is last - first + 1.  The strings of one pattern have one length, so their order by `first` is
the lexicographic order of their codes: the yardstick orders them so, without knowing a row."""
import zlib
from collections import namedtuple

import numpy as np

from mismatch_util import prepared

SEOF, OFFSET, ALPHA, MAX_PATTERN, CLASS, MAX_CLASSES = 2, 5, 261, 32768, 0x8000, 4096
Found = namedtuple("Found", "symbols rows")      # uint16[m] alpha codes, windows

# (fixture, regular expression, the reference's result count): the class patterns among tests/golden/<fixture>_regexp.npz
GOLDEN = [("acgt48k", b"G[AC]T[^A]GG", 6), ("acgt48k", b"TTT.TTT", 3), ("acgt48k", b"[AC][AC][GT][GT]ACG", 16), ("eng2doc", b"q.", 10),
          ("eng2doc", b"\\n.", 32), ("eng2doc", b"[^a-z ]", 66), ("bytes256", b"\\x00.", 46), ("bytes256", b"[\\x80-\\xff][\\x00-\\x10]", 364),
          ("bytes256", b"[\\x00-\\xff]\\x7f", 36), ("runs3doc", b"b.b", 2)]


def golden_case(name, regex):
    """the reference's (first, last, match_len) lists for `regex` on fixture `name`: the entry with from_regex = 1 and approx[0] = 0"""
    from regexp_util import load_regexp_golden
    hits = [c for c in load_regexp_golden(name) if c[1] == regex and c[2][0] == 0]
    assert len(hits) == 1, (name, regex, len(hits))
    err, first, last, mlen, cost = hits[0][3]
    assert err == 0 and not cost.any()
    return first, last, mlen


def class_words(members):
    """uint64[4]: bit b of word w says that byte 64 w + b belongs to the class"""
    w = [0, 0, 0, 0]
    for b in members:
        w[int(b) >> 6] |= 1 << (int(b) & 63)
    return np.array(w, dtype=np.uint64)


def members_of(words):
    return [b for b in range(256) if (int(words[b >> 6]) >> (b & 63)) & 1]


def allowed(pattern, classes):
    """bool[m, 261]: the alpha codes each position takes; None for a pattern that holds a symbol that is neither a literal nor a
    class of the table"""
    p = np.asarray(pattern, dtype=np.uint16)
    ok = np.zeros((len(p), ALPHA), dtype=bool)
    for j, s in enumerate(p):
        s = int(s)
        if s < ALPHA:
            ok[j, s] = True
        elif s & CLASS and (s & ~CLASS) < len(classes):
            ok[j, [b + OFFSET for b in members_of(classes[s & ~CLASS])]] = True
        else:
            return None
    return ok


def strings(text, pattern, classes):
    """[Found] of `pattern` (symbols) in `text` (prepared), in lexicographic order"""
    p = np.asarray(pattern, dtype=np.uint16)
    m, n = len(p), len(text)
    if m == 0:
        return [Found(p, n)]
    ok = allowed(p, classes)
    if ok is None or m > n or m > MAX_PATTERN:
        return []
    cand = np.arange(n - m + 1)
    for j in np.argsort(ok.sum(axis=1), kind="stable"):          # the narrowest positions first: the candidates thin out quickly
        cand = cand[ok[j][text[cand + j]]]
        if len(cand) == 0:
            return []
    uniq, rows = np.unique(text[cand[:, None] + np.arange(m)], axis=0, return_counts=True)
    return [Found(v, int(c)) for v, c in zip(uniq, rows)]


def automaton_may_differ(text, pattern, classes):
    """Can the automaton route (do_regexp_query) list fewer strings than the question has?  It keeps its pending entries BY RANGE: a
    string w of k symbols that matches the pattern's last k symbols and a string u of j < k symbols that matches the last j are
    merged into one entry when their ranges are equal, and an entry with a final state alive is a result that is never extended.
    Equal ranges of different lengths mean w = u t with every occurrence of u followed by t, so where no such pair exists the two
    routes give the same list; where one exists, the automaton's list is a sub-list.  (eng2doc: every ' is followed by s, so for
    `..` the entry of "'" is merged with "'s", reported, and the nineteen strings "x'" are never reached.)"""
    p = np.asarray(pattern, dtype=np.uint16)
    shorter = {}
    for k in range(1, len(p) + 1):
        mine = {f.symbols.tobytes(): f.rows for f in strings(text, p[len(p) - k:], classes)}
        for w, rows in mine.items():
            for j in range(1, k):
                if shorter[j].get(w[:2 * j]) == rows:
                    return True
        shorter[k] = mine
    return False


def expected(per_pattern):
    """(result_start, the strings in result order) from strings() of every pattern"""
    start, flat = [0], []
    for fs in per_pattern:
        flat += fs
        start.append(len(flat))
    return np.array(start, dtype=np.int64), flat


class Table:
    """the class table of a pattern set: equal sets share a number"""

    def __init__(self):
        self.number, self.words = {}, []

    def sym(self, members):
        key = tuple(sorted({int(b) for b in members}))
        if key not in self.number:
            self.number[key] = len(self.words)
            self.words.append(class_words(key))
        return CLASS | self.number[key]

    def array(self):
        return np.stack(self.words) if self.words else np.zeros((0, 4), dtype=np.uint64)


def icase_symbols(codes, table):
    """icase_ast of a string of byte codes: a letter becomes the class of its two cases, anything else stays a literal"""
    out = []
    for c in codes:
        b = int(c) - OFFSET
        if 65 <= b <= 90 or 97 <= b <= 122:
            out.append(table.sym([b | 32, b & ~32]))
        else:
            out.append(int(c))
    return np.array(out, dtype=np.uint16)


def regex_of(pattern, classes):
    """the pattern in the query language, or None where it has no such text (an empty class)"""
    out = b""
    for s in np.asarray(pattern, dtype=np.uint16):
        s = int(s)
        if s < OFFSET:
            out += b"\\x-%02x" % (OFFSET - s)
        elif s < ALPHA:
            out += b"\\x%02x" % (s - OFFSET)
        else:
            mem = members_of(classes[s & ~CLASS])
            if not mem:
                return None
            out += b"." if len(mem) == 256 else b"[" + b"".join(b"\\x%02x" % b for b in mem) + b"]"
    return out


def pattern_set(docs, name):
    """([(tag, uint16 symbols)], classes uint64[n, 4]): about 200 patterns -- the cases tests/test_gpu_classes.py names, then cuts of
    the text with up to three positions turned into random classes.  Deterministic per fixture name."""
    rng = np.random.default_rng(zlib.crc32(("classes " + name).encode()))
    docs = [np.asarray(d, dtype=np.uint8) for d in docs]
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    longest = max(docs, key=len)
    T = Table()
    out = []

    def add(tag, p):
        out.append((tag, np.asarray(p, dtype=np.uint16)))

    def cut(length):
        if len(longest) < length:
            return rng.choice(have, size=length).astype(np.uint16) + OFFSET
        at = int(rng.integers(0, len(longest) - length + 1))
        return longest[at:at + length].astype(np.uint16) + OFFSET

    def widened(sym, extra):
        """the class of the byte of `sym` and `extra` other bytes of the text (fewer where the text has fewer)"""
        own = int(sym) - OFFSET
        rest = have[have != own]
        return T.sym([own] + list(rng.choice(rest, size=min(extra, len(rest)), replace=False)))

    def classed(p, at, extra=2):
        p = p.copy()
        for i in at:
            p[i] = widened(p[i], extra)
        return p

    period = T.sym(range(256))
    add("empty", [])
    for length in (1, 2, 20, 64):
        add("literal%d" % length, cut(length))
    m = min(20, len(longest))
    base = cut(m)
    first, mid, last = 0, m // 2, m - 1
    for tag, at in (("first", [first]), ("mid", [mid]), ("last", [last]), ("all_three", [first, mid, last])):
        add("class_" + tag, classed(base, at))
    for length in (1, 2, 20):
        add("every%d" % length, classed(cut(length), range(length), 1))
    deep = min(300, len(longest))
    add("deep", classed(cut(deep), range(deep), 1))
    add("period1", [period])
    add("period2", [period, period])
    for length in (3, 8, 20, 40):
        add("icase", icase_symbols(cut(length), T))
    nobody = T.sym(lacks[:3])          # (bytes256 holds every byte: the empty class)
    for tag, at in (("first", first), ("mid", mid), ("last", last)):
        p = cut(m)
        p[at] = nobody
        add("nobody_" + tag, p)
    add("nobody_alone", [nobody])
    add("empty_class", [T.sym([]), base[last]])
    add("period_mid", np.concatenate([base[:3], [period], base[4:8]]))
    add("period_ends", np.concatenate([[period], base[1:6], [period]]))
    lacking = int(lacks[0]) + OFFSET if len(lacks) else 1          # (code 1: below SEOF, in no text)
    for at in (first, mid, last):
        p = classed(cut(m), [first, last])
        p[at] = lacking
        add("lacks", p)
    tail = longest[-6:].astype(np.uint16) + OFFSET
    add("seof_end", np.concatenate([tail, [SEOF]]))
    add("seof_end_class", np.concatenate([classed(tail, [len(tail) - 1, 0]), [SEOF]]))
    add("seof_after_period", [period, SEOF])
    add("seof_alone", [SEOF])
    add("twice", out[8][1])
    add("twice", out[8][1])
    shared = widened(base[mid], 3)
    for _ in range(2):
        p = cut(m)
        p[mid] = shared
        add("shared", p)
    add("shared", [shared, shared])
    for at in (first, last):          # literals alone that do not occur
        p = cut(m)
        p[at] = lacking
        add("absent", p)
    # short and wide: many strings per pattern.  (A lane tries up to 12 + 12^2 + 12^3 members: the slowest rank policy, a walk of
    # femto's wavelet tree per step, stays within a second on it)
    for _ in range(30):
        p = []
        for _ in range(int(rng.integers(2, 4))):
            k = int(rng.integers(2, min(12, len(have)) + 1))
            p.append(T.sym(rng.choice(have, size=k, replace=False)) if rng.random() < 0.8 else int(rng.choice(have)) + OFFSET)
        add("wide", p)
    while len(out) < 200:
        p = cut(int(rng.integers(3, 33)))
        n = int(rng.integers(0, 4))
        at = rng.choice(len(p), size=min(n, len(p)), replace=False)
        add("cut%d" % n, classed(p, at, int(rng.integers(1, 6))))
    return out, T.array()


# ---- past the fixtures: what tests/test_gpu_classes_edges.py runs and tests/test_classes_host.py pins ---------------------------

def table_of(classes):
    """a Table that holds `classes` (distinct sets) under their numbers, to be extended"""
    T = Table()
    for w in classes:
        T.sym(members_of(w))
    assert len(T.words) == len(classes)
    return T


def corpus_pattern_set(docs, name):
    """([(tag, symbols)], classes) of a built corpus: pattern_set, then mismatch_util's SEOF family (patterns that END in SEOF) --
    each member as it is and with one and with two of its byte positions turned into the class of its byte and two others --, then
    [period, SEOF], [period, period, SEOF] and the class {a, b, \\n} in front of SEOF"""
    import mismatch_util as mu
    docs = mu.as_arrays(docs)
    rng = np.random.default_rng(zlib.crc32(("classes corpus " + name).encode()))
    have = np.unique(np.concatenate(docs))
    out, cls = pattern_set(docs, name)
    T = table_of(cls)

    def classed(p, at):
        p = p.copy()
        for i in at:
            own = int(p[i]) - OFFSET
            rest = have[have != own]
            p[i] = T.sym([own] + list(rng.choice(rest, size=min(2, len(rest)), replace=False)))
        return p

    for tag, p in mu.seof_family(docs, name):
        out.append((tag, p))
        nbytes = len(p) - 1          # (SEOF stands last)
        for n in (1, 2):
            if nbytes >= n:
                out.append(("%s_classed%d" % (tag, n), classed(p, rng.choice(nbytes, size=n, replace=False))))
    period = T.sym(range(256))
    out.append(("seof_after_period", np.array([period, SEOF], dtype=np.uint16)))
    out.append(("seof_after_period2", np.array([period, period, SEOF], dtype=np.uint16)))
    out.append(("seof_after_abn", np.array([T.sym(b"ab\n"), SEOF], dtype=np.uint16)))
    return out, T.array()


def tiny_patterns():
    """(patterns, classes): every pattern of 1 .. 3 of the symbols a, b, c, [ab], [abc], [bc], [c] (a class of one member, which the
    tiny texts lack), the period and the empty class, bare and with SEOF behind it, and the empty pattern: 2 * (9 + 81 + 729) + 1"""
    T = Table()
    a, b, c = (ord(x) + OFFSET for x in "abc")
    alphabet = [a, b, c, T.sym(b"ab"), T.sym(b"abc"), T.sym(b"bc"), T.sym(b"c"), T.sym(range(256)), T.sym([])]
    bare = []
    for m in (1, 2, 3):
        for i in range(9 ** m):
            bare.append(np.array([alphabet[(i // 9 ** j) % 9] for j in range(m)], dtype=np.uint16))
    return bare + [np.concatenate([p, [SEOF]]).astype(np.uint16) for p in bare] + [np.zeros(0, dtype=np.uint16)], T.array()


def plain_strings(docs, pattern, classes):
    """the rule as a plain triple loop over the documents (bytes), the window starts and the pattern's positions; no numpy"""
    text = []
    for d in docs:
        text += [int(x) + OFFSET for x in bytes(d)] + [SEOF]
    p = [int(s) for s in pattern]
    if not p:
        return [((), len(text))]
    sets = [set(x + OFFSET for x in members_of(classes[s & ~CLASS])) if s & CLASS else {s} for s in p]
    count = {}
    for s in range(len(text) - len(p) + 1):
        for j in range(len(p)):
            if text[s + j] not in sets[j]:
                break
        else:
            w = tuple(text[s:s + len(p)])
            count[w] = count.get(w, 0) + 1
    return sorted(count.items())


LONG_CUTS = (MAX_PATTERN, MAX_PATTERN - 1)
DEEP_CUT = 4097


def long_patterns(doc):
    """([(tag, symbols)], classes): cuts of `doc` (uint8, longer than MAX_PATTERN) of 32768 and of 32767 symbols with the class
    {own byte, one other byte of the document} at {32767}, {0}, {0, 32767}, {32766, 32767} and {16383, 16384} (the last position is
    the cut's last where the cut is shorter), then one cut of each length and one of 4097 symbols with such a class at EVERY
    position"""
    rng = np.random.default_rng(32768 + 0x8000)
    doc = np.asarray(doc, dtype=np.uint8)
    have = np.unique(doc)
    T = Table()
    out = []

    def classed(p, at):
        p = p.copy()
        for i in at:
            own = int(p[i]) - OFFSET
            p[i] = T.sym([own, int(rng.choice(have[have != own]))])
        return p

    def cut(m):
        s = int(rng.integers(0, len(doc) - m + 1))
        return doc[s:s + m].astype(np.uint16) + OFFSET

    for m in LONG_CUTS:
        last = m - 1
        for at in ((last,), (0,), (0, last), (last - 1, last), (16383, 16384)):
            out.append(("long%d_%s" % (m, "_".join(map(str, at))), classed(cut(m), at)))
    for m in LONG_CUTS + (DEEP_CUT,):
        out.append(("every%d" % m, classed(cut(m), range(m))))
    return out, T.array()


SUBSETS = [s for s in ([b"ACGT"[i] for i in range(4) if m >> i & 1] for m in range(16)) if len(s) >= 2]          # the 11 of two or more
MARKERS = list(range(128, 137))          # nine bytes a text over A, C, G and T lacks: 2^9 > 4096 / 11


def table_4096(doc):
    """([(tag, symbols)], classes uint64[4096, 4]): 4096 DISTINCT classes -- class i is SUBSETS[i % 11] and the markers of the bits
    of i // 11 -- and 4096 patterns, pattern i a 12-symbol cut of `doc` whose position i % 12 holds a byte of class i and is turned
    into CLASS | i"""
    rng = np.random.default_rng(4096)
    doc = np.asarray(doc, dtype=np.uint8)
    assert set(np.unique(doc).tolist()) == set(b"ACGT")
    classes = np.stack([class_words(SUBSETS[i % 11] + [m for b, m in enumerate(MARKERS) if (i // 11) >> b & 1]) for i in range(MAX_CLASSES)])
    assert len({w.tobytes() for w in classes}) == MAX_CLASSES
    out = []
    for i in range(MAX_CLASSES):
        j = i % 12
        while True:
            s = int(rng.integers(0, len(doc) - 12 + 1))
            if int(doc[s + j]) in SUBSETS[i % 11]:
                break
        p = doc[s:s + 12].astype(np.uint16) + OFFSET
        p[j] = CLASS | i
        out.append(("class%d" % i, p))
    return out, classes
