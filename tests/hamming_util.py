"""The question of include/femto_amd.h "occurrences within k substitutions, by exact seeds", restated in plain numpy over a
fixture's documents, and the pattern sets the tests of it share (tests/test_hamming_host.py pins both to tests/mismatch_util.py and
to the CPU oracle, tests/test_gpu_hamming.py runs them).

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
