"""The question of include/femto_amd.h "occurrences within k substitutions, by exact seeds", restated in plain numpy over a
fixture's documents, and the pattern sets the tests of it share (tests/test_hamming_host.py pins both to tests/mismatch_util.py and
to the CPU oracle, tests/test_gpu_hamming.py runs them); below them the corpora and batches of tests/test_gpu_hamming_edges.py.

THE RULE.  The pattern (byte characters only) slides over the PREPARED TEXT -- every document's bytes + 5 followed by SEOF, not
cyclic -- and a window p is an occurrence of cost c when it differs from the pattern at exactly c <= k positions and holds a byte
character at each of them.  SEOF is no substitute, so no window runs over a document's end.  This is mismatch_util.variants for a
pattern of bytes, asked for the windows themselves rather than for the distinct strings they hold, and for any k.

THE PIECES.  Piece j of m symbols under k is [j m // (k + 1), (j + 1) m // (k + 1)), j = 0 .. k: part of the contract, because the
call reports how many candidates the pieces gave it."""
import zlib

import numpy as np

SEOF, OFFSET, ALPHA, MAX_PATTERN = 2, 5, 261, 32768
KS = (0, 1, 2, 3, 5, 8)
LENGTHS = (9, 24, 64, 100, 300)          # and k + 1


def prepared(docs):
    parts = []
    for d in docs:
        b = np.frombuffer(d, dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else np.asarray(d, dtype=np.uint8)
        parts += [b.astype(np.uint16) + OFFSET, np.array([SEOF], dtype=np.uint16)]
    return np.concatenate(parts)


def occurrences(text, pattern, k):
    """(offsets int64[] ascending, costs int32[]) of `pattern` (alpha codes of bytes) in `text` (prepared)"""
    p = np.asarray(pattern, dtype=np.uint16)
    m, n = len(p), len(text)
    none = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    if m == 0 or m > n:
        return none
    cand = np.arange(n - m + 1, dtype=np.int64)
    diff = np.zeros(len(cand), dtype=np.int32)
    for j in range(m):          # column by column: the candidates thin out after a few
        col = text[cand + j]
        neq = col != p[j]
        diff = diff + neq
        keep = (diff <= k) & (~neq | (col >= OFFSET))
        cand, diff = cand[keep], diff[keep]
        if len(cand) == 0:
            return none
    return cand, diff.astype(np.int32)


def pieces(m, k):
    """[(start, end)] of the k + 1 pieces of a pattern of m symbols"""
    return [(j * m // (k + 1), (j + 1) * m // (k + 1)) for j in range(k + 1)]


def expected(text, patterns, k):
    """the call's answer: (result_start int64[n + 1], offset int64[], cost int32[])"""
    start, offs, costs = [0], [], []
    for p in patterns:
        o, c = occurrences(text, p, k)
        offs.append(o)
        costs.append(c)
        start.append(start[-1] + len(o))
    return (np.array(start, dtype=np.int64), np.concatenate(offs) if offs else np.zeros(0, dtype=np.int64),
            np.concatenate(costs) if costs else np.zeros(0, dtype=np.int32))


def pattern_set(docs, name, k):
    """[(tag, uint16 alpha codes)]: about 120 patterns of more than k symbols for bound k.  Cuts of the text of k + 1, 9, 24, 64, 100
    and 300 symbols with 0 .. k substitutions planted (every fourth planted cut with a character the text lacks, where it lacks
    one), then the named cases.  Deterministic per fixture name and k."""
    rng = np.random.default_rng(zlib.crc32(("hamming %s %d" % (name, k)).encode()))
    docs = [np.asarray(d, dtype=np.uint8) for d in docs]
    total = sum(len(d) + 1 for d in docs)
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    longest = max(docs, key=len)
    out = []

    def add(tag, p):
        assert len(p) > k
        out.append((tag, np.asarray(p, dtype=np.uint16)))

    def cut(length, doc=None, at=None):
        d = longest if doc is None else doc
        at = int(rng.integers(0, len(d) - length + 1)) if at is None else at
        return d[at:at + length].astype(np.uint16) + OFFSET

    def planted(p, nsub, lacking=False):
        p = p.copy()
        at = rng.choice(len(p), size=min(nsub, len(p)), replace=False)
        for n, i in enumerate(at):
            c = have[have != int(p[i]) - OFFSET]
            if lacking and n == 0 and len(lacks):
                p[i] = int(lacks[0]) + OFFSET
            elif len(c):
                p[i] = int(rng.choice(c)) + OFFSET
        return p

    lengths = [m for m in sorted({k + 1} | set(LENGTHS)) if k < m <= len(longest)]
    n = 0
    for m in lengths:
        for r in range(16):
            nsub = r % (k + 1)
            add("cut%d_%d" % (m, nsub), planted(cut(m), nsub, lacking=n % 4 == 3))
            n += 1
    m = min(24, len(docs[0]))
    if m > k:
        add("from_offset_0", cut(m, docs[0], 0))
        add("from_offset_0_planted", planted(cut(m, docs[0], 0), min(k, 1)))
    for d in docs[:3]:
        m = min(24, len(d))
        if m > k:
            add("to_last_byte", cut(m, d, len(d) - m))
            add("to_last_byte_planted", planted(cut(m, d, len(d) - m), min(k, 2)))
    if len(docs) > 1 and min(len(docs[0]), len(docs[1])) >= 12:
        add("straddle", np.concatenate([docs[0][-12:], docs[1][:12]]).astype(np.uint16) + OFFSET)
    if total + 1 <= MAX_PATTERN:          # (acgt48k's text is longer than a pattern may be)
        add("longer_than_the_text", rng.choice(have, size=total + 1).astype(np.uint16) + OFFSET)
    for m in (3 * (k + 1) + 1, 7 * (k + 1) + k):          # lengths that k + 1 does not divide (k > 0)
        if m <= len(longest):
            add("ragged%d" % m, planted(cut(m), k))
    if len(lacks) and len(longest) >= 24 + k:
        p = cut(24 + k)
        p[rng.choice(len(p), size=k + 1, replace=False)] = int(lacks[-1]) + OFFSET          # k + 1 lacking characters: no result
        add("lacks_too_many", p)
    for _ in range(6):
        add("random", rng.choice(have, size=max(k + 1, int(rng.integers(4, 30)))).astype(np.uint16) + OFFSET)
    return out


# ---- the builders of tests/test_gpu_hamming_edges.py (plain numpy; tests/test_hamming_host.py asserts what they must hold) ------

def codes(b):
    """alpha codes of bytes"""
    return (np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, dtype=np.uint8)).astype(np.uint16) + OFFSET


def _rng(*what):
    return np.random.default_rng(zlib.crc32(" ".join(str(w) for w in ("hamming edges",) + what).encode()))


def _as_arrays(docs):
    return [np.frombuffer(bytes(d), dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else np.asarray(d, dtype=np.uint8) for d in docs]


def _cut_at(rng, d, m, residue=None, base=0):
    """a start in d for a cut of m bytes; with `residue`, one whose text offset base + start is that modulo 8"""
    if residue is None:
        return int(rng.integers(0, len(d) - m + 1))
    first = (residue - base) & 7
    return first + 8 * int(rng.integers(0, (len(d) - m - first) // 8 + 1))


def _differ(rng, p, positions, have):
    """p with another character of `have` (bytes) at every position"""
    p = p.copy()
    for i in positions:
        p[i] = int(rng.choice(have[have != int(p[i]) - OFFSET])) + OFFSET
    return p


# -- 1. alphabets of 256 and of 255 codes -----------------------------------------------------------------------------------------
ALPHABET_LACKS = {256: (0x4e,), 255: (0x4e, 0xfe)}          # the bytes the corpus of that many codes (SEOF among them) lacks
ALPHABET_M = 24


def alphabet_docs(ncodes):
    """three documents, 4086 bytes, of every byte value but ALPHABET_LACKS[ncodes]; a permutation of them all stands in two of the
    documents, so every character has 24 symbols of room on either side somewhere"""
    rng = _rng("alphabet", ncodes)
    have = np.setdiff1d(np.arange(256), ALPHABET_LACKS[ncodes]).astype(np.uint8)
    docs = [have[rng.integers(0, len(have), n)] for n in (1400, 1290, 1396)]
    docs[0][100:100 + len(have)] = rng.permutation(have)
    docs[1][500:500 + len(have)] = rng.permutation(have)
    return docs


def alphabet_patterns(docs, k):
    """[(tag, codes)] for k >= 1.  "opposite_<c>_<i>": a 24-symbol cut with the lacking byte at position i, where the text holds
    byte c -- one for every distinct c, i going round the pattern; then the lacking byte twice, in every piece in turn, in pieces
    0 .. j - 1 for every owner j (and in all: no result), next to a true difference across a piece's end, over a document's end
    (opposite SEOF, and anywhere in a cut laid over the two documents), in lengths that k + 1 does not divide, and cuts without it"""
    docs = _as_arrays(docs)
    rng = _rng("alphabet patterns", len(np.unique(np.concatenate(docs))), k)
    have = np.unique(np.concatenate(docs))
    lacks = np.setdiff1d(np.arange(256), have)
    lack, lack2 = int(lacks[0]) + OFFSET, int(lacks[-1]) + OFFSET
    m = ALPHABET_M
    b = pieces(m, k)
    out = []

    def cut(length=m, doc=0):
        at = _cut_at(rng, docs[doc], length)
        return codes(docs[doc][at:at + length])

    def lacking(p, positions, code=lack):
        p = p.copy()
        p[list(positions)] = code
        return p

    for n, c in enumerate(have):
        i = n % m
        for d in docs:
            at = np.nonzero(d == c)[0]
            at = at[(at >= i) & (at - i + m <= len(d))]
            if len(at):
                out.append(("opposite_%d_%d" % (c, i), lacking(codes(d[at[0] - i:at[0] - i + m]), [i])))
                break
    out.append(("two_lacking", lacking(lacking(cut(), [3]), [17], lack2)))
    for j, (b0, b1) in enumerate(b):
        out.append(("lack_in_piece%d" % j, lacking(cut(doc=j % 3), [(b0 + b1) // 2])))
    for j in range(1, k + 2):          # owner j: pieces 0 .. j - 1 each hold it, at their first and last symbols in turn; j = k + 1: all do
        out.append(("lack_owner%d" % j, lacking(cut(doc=j % 3), [b[i][0] if i % 2 == 0 else b[i][1] - 1 for i in range(j)])))
    for j in range(1, k + 1):          # the last symbol of piece j - 1 lacking, the first of piece j another character of the text
        out.append(("lack_seam%d" % j, _differ(rng, lacking(cut(), [b[j][0] - 1]), [b[j][0]], have)))
    a, c = docs[0], docs[1]
    out.append(("lack_opposite_seof", np.concatenate([codes(a[-12:]), [lack], codes(c[:11])]).astype(np.uint16)))
    out.append(("lack_over_the_end", lacking(np.concatenate([codes(a[-12:]), codes(c[:12])]), [5])))
    for length in (3 * (k + 1) + 1, 7 * (k + 1) + k):
        p = cut(length)
        at = rng.choice(length, size=k, replace=False)
        out.append(("lack_ragged%d" % length, _differ(rng, lacking(p, at[:1]), at[1:], have)))
    for n in range(8):
        p = cut(doc=n % 3)
        out.append(("plain%d" % n, _differ(rng, p, rng.choice(m, size=n % (k + 1), replace=False), have)))
    return out


# -- 2. the word compare's geometry on a text of four letters ----------------------------------------------------------------------
ACGT = np.frombuffer(b"acgt", dtype=np.uint8)
GEOMETRY_KS = (1, 2, 3, 7)
GEOMETRY_MS = (7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65)          # and k + 1


def acgt_docs():
    """two documents of 2100 and 1990 letters of acgt"""
    rng = _rng("acgt")
    return [ACGT[rng.integers(0, 4, n)] for n in (2100, 1990)]


def geometry_plants(m, k):
    """[(tag, positions that get another letter)] for a cut of m symbols: none; byte 0, 7, 8 and m - 1; the last byte of piece
    j - 1 with the first of piece j; one in each of pieces 0 .. j - 1 (owner j), at their first and last bytes in turn; one in
    every piece; and the last k + 1 bytes, which leave piece 0 standing where m > k + 1"""
    b = pieces(m, k)
    out = [("exact", [])]
    for i in sorted({0, 7, 8, m - 1}):
        if i < m:
            out.append(("at%d" % i, [i]))
    for j in range(1, k + 1):
        out.append(("seam%d" % j, [b[j][0] - 1, b[j][0]]))
    for j in range(1, k + 1):
        out.append(("owner%d" % j, [b[i][0] if i % 2 == 0 else b[i][1] - 1 for i in range(j)]))
    out.append(("every_piece", [b0 for b0, _ in b]))
    if m > k + 1:
        out.append(("too_many", list(range(m - k - 1, m))))
    return out


def geometry_batch(docs, k):
    """[(tag, codes)]: for every m, 64 cuts -- text offsets of every residue modulo 8, each at every residue of its first symbol
    in the batch (fillers of k + 1 .. k + 8 symbols, cuts themselves, move it there) -- with geometry_plants(m, k) in turn"""
    docs = _as_arrays(docs)
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
                    at = _cut_at(rng, d, length)
                    out.append(("filler%d" % length, codes(d[at:at + length])))
                    total += length
                tag, positions = plants[n % len(plants)]
                d = docs[(n // len(plants)) % 2]
                at = _cut_at(rng, d, m, r, bases[(n // len(plants)) % 2])
                out.append(("m%d_%s_r%d_a%d" % (m, tag, r, a), _differ(rng, codes(d[at:at + m]), positions, ACGT)))
                total += m
                n += 1
    return out


def owners(text, p, k, offsets):
    """for every result window of p: the leftmost piece without a difference (the piece whose candidate emits it)"""
    m = len(p)
    neq = text[np.asarray(offsets, dtype=np.int64)[:, None] + np.arange(m)] != p
    clean = np.stack([~neq[:, b0:b1].any(axis=1) for b0, b1 in pieces(m, k)], axis=1)
    assert clean.any(axis=1).all()
    return clean.argmax(axis=1)


RUN_TEXTS = {"one": [b"a" * 300], "two": [b"a" * 37 + b"b" * 5 + b"a" * 64 + b"b" + b"a" * 9 + b"bb" + b"a" * 17, b"b" * 80 + b"a" * 3 + b"b" * 82]}
RUN_KS = (0, 2, 8)


def run_patterns(k):
    """patterns of one character: every piece occurs wherever that character runs"""
    return [("%s%d" % (ch, m), codes(ch.encode() * m)) for ch in "ab" for m in sorted({k + 1, 9, 16, 24, 65}) if m > k]


# -- 3. large k ---------------------------------------------------------------------------------------------------------------------
LARGE_KS = (15, 16, 17, 31, 64, 255)


def large_k_batch(docs, k):
    """[(tag, codes)]: cuts of k + 1, k + 2, 2k + 1 and 300 letters with 0, 1, k and k + 1 other letters planted, and a pattern of
    a letter the text lacks"""
    docs = _as_arrays(docs)
    rng = _rng("large k", k)
    out = []
    for m in sorted({k + 1, k + 2, 2 * k + 1} | ({300} if 300 > k else set())):
        for nsub in (0, 1, k, k + 1):
            at = _cut_at(rng, docs[0], m)
            out.append(("cut%d_%d" % (m, nsub), _differ(rng, codes(docs[0][at:at + m]), rng.choice(m, size=nsub, replace=False), ACGT)))
    out.append(("lacking", codes(b"n" * (k + 4))))
    return out


def long_batch(doc, k=255, m=MAX_PATTERN):
    """cuts of the longest pattern with 0, k and k + 1 other letters planted (doc: letters of acgt, longer than m)"""
    rng = _rng("long", k, m)
    have = np.unique(doc)
    p = codes(doc[200:200 + m])
    return [("long_%d" % nsub, _differ(rng, p, rng.choice(m, size=nsub, replace=False), have)) for nsub in (0, k, k + 1)]


# -- 4. the bounds of the window -----------------------------------------------------------------------------------------------------
BOUNDS_M = 24


def bounds_patterns(docs, k):
    """[(tag, codes, piece, offset)] on letters of acgt: `piece` of the pattern occurs at `offset` of the prepared text (None:
    the whole pattern is the case).  A later piece at the text's start with all that follows it (the window starts in front of
    the text); piece 0 at the text's last letters, and one symbol too far right to fit; the first and the last window themselves"""
    docs = _as_arrays(docs)
    text = prepared(docs)
    n, m = len(text), BOUNDS_M
    rng = _rng("bounds", k)
    b = pieces(m, k)
    letters = lambda count: codes(ACGT[rng.integers(0, 4, count)])
    out = []
    for j in sorted({1, k}):
        b0 = b[j][0]
        out.append(("piece%d_at_the_start" % j, np.concatenate([letters(b0), text[:m - b0]]), j, 0))
    l0 = b[0][1]
    out.append(("piece0_at_the_end", np.concatenate([text[n - 1 - l0:n - 1], letters(m - l0)]), 0, n - 1 - l0))
    out.append(("one_symbol_too_far", np.concatenate([text[n - m + 1:n - 1], letters(2)]), 0, n - m + 1))
    first, last = text[:m].copy(), text[n - 1 - m:n - 1].copy()
    out.append(("window_0", first, None, 0))
    out.append(("window_0_owner1", _differ(rng, first, [b[0][0]], ACGT), None, 0))
    out.append(("window_last", last, None, n - 1 - m))
    out.append(("window_last_owner%d" % k, _differ(rng, last, [b[i][1] - 1 for i in range(k)], ACGT), None, n - 1 - m))
    return out


# -- 5. many documents -----------------------------------------------------------------------------------------------------------------
MANY_KS = (1, 2, 5)
STRADDLE_MS = (9, 24)


def many_docs_patterns(docs, name, k):
    """[(tag, codes)] on a corpus of hundreds of documents.  "straddle<m>_<i>_<e>": the last i bytes of a document, any byte, and
    the first m - i - 1 of the next, e further bytes changed: the window over the two has SEOF under one difference and is no
    result, whatever k -- every i = 1 .. m - 1, over pairs of neighbours taken in turn.  Then cuts to the last and from the first
    byte, documents with k + 1 lacking bytes behind them (longer than the document, never an occurrence), the bytes on either side
    of an empty document, and the most frequent 24-byte strings of the corpus, bare and with k bytes changed"""
    docs = _as_arrays(docs)
    rng = _rng("many", name, k)
    have = np.unique(np.concatenate(docs))
    lack = int(np.setdiff1d(np.arange(256), have)[0]) + OFFSET
    lens = np.array([len(d) for d in docs])
    out = []
    any_byte = lambda: np.array([int(rng.choice(have)) + OFFSET], dtype=np.uint16)
    for m in STRADDLE_MS:
        if m <= k:
            continue
        for i in range(1, m):
            pairs = np.nonzero((lens[:-1] >= i) & (lens[1:] >= m - i - 1))[0]
            d = int(pairs[(7 * i + 3 * m) % len(pairs)])
            p = np.concatenate([codes(docs[d][lens[d] - i:]), any_byte(), codes(docs[d + 1][:m - i - 1])]).astype(np.uint16)
            for extra in sorted({0, k - 1}):
                at = rng.choice(np.delete(np.arange(m), i), size=extra, replace=False)
                out.append(("straddle%d_%d_%d" % (m, i, extra), _differ(rng, p, at, have)))
    whole = np.nonzero(lens >= 9)[0]
    for d in whole[:: max(1, len(whole) // 8)][:8]:
        out.append(("to_last_byte", codes(docs[d][-9:])))
        out.append(("from_first_byte", codes(docs[d][:9])))
        out.append(("to_last_byte_planted", _differ(rng, codes(docs[d][-9:]), [int(rng.integers(0, 9))], have)))
    short = np.nonzero(lens >= 1)[0]
    short = short[np.argsort(lens[short], kind="stable")]
    nth = [int(short[min(np.searchsorted(lens[short], length), len(short) - 1)]) for length in range(1, 9)]
    for d in dict.fromkeys(nth + [int(d) for d in short[:3]]):          # (documents of 1 .. 8 bytes where there are such, and the shortest)
        out.append(("longer_than_its_document", np.concatenate([codes(docs[d]), np.full(k + 1, lack)]).astype(np.uint16)))
    empty = [d for d in range(1, len(docs) - 1) if lens[d] == 0 and lens[d - 1] >= 4 and lens[d + 1] >= 1][:6]
    for d in empty:          # ...xxxx S S yyy...: two symbols of the pattern lie opposite the two SEOFs
        out.append(("across_an_empty_document", np.concatenate([codes(docs[d - 1][-4:]), any_byte(), any_byte(), codes(docs[d + 1][:3])]).astype(np.uint16)))
    text = prepared(docs)
    win = np.lib.stride_tricks.sliding_window_view(text, 24)
    win = win[(win >= OFFSET).all(axis=1)]
    uniq, count = np.unique(win, axis=0, return_counts=True)
    for n, row in enumerate(np.argsort(-count, kind="stable")[:6]):
        out.append(("frequent%d" % n, uniq[row].astype(np.uint16)))
        if k:
            out.append(("frequent%d_planted" % n, _differ(rng, uniq[row].astype(np.uint16), rng.choice(24, size=k, replace=False), have)))
    return out


# -- 6. the work area ----------------------------------------------------------------------------------------------------------------

def pool(docs, k, size=48):
    """cuts of k + 1 + 6 .. k + 1 + 30 letters of acgt, every third with up to k other letters planted"""
    docs = _as_arrays(docs)
    rng = _rng("pool", k, size)
    out = []
    for i in range(size):
        m = k + 7 + int(rng.integers(0, 25))
        d = docs[i % 2]
        at = _cut_at(rng, d, m)
        p = codes(d[at:at + m])
        out.append(_differ(rng, p, rng.choice(m, size=int(rng.integers(1, k + 1)), replace=False), ACGT) if i % 3 == 1 and k else p)
    return out
