"""What the level table (ktab2) and the context tables (ctx / ctxm / ctx2) owe for EVERY entry, from the reference's goldens alone
(pure numpy, no device code): the batches that ask for every entry, the expected (first, last) of every level-table entry, and a
comparer that names the first offending entry."""
from collections import namedtuple

import numpy as np

SEOF = 2
# one flat pattern batch; heap[i] = the level-table heap position pattern i asks for (-1: not a string of table characters)
Batch = namedtuple("Batch", "plen flat starts heap")
# the reference's answers for a batch: count's (first, last), and locate's (noccs, offsets) at one clamp
Answers = namedtuple("Answers", "first last max_occs noccs offs")


def table_chars(symbols):
    """the table characters of a text (or of its L): the symbols above SEOF, ascending -- digit(c) = index of c"""
    u = np.unique(np.asarray(symbols))
    return u[u > SEOF].astype(np.uint16)


def level_offsets(t, K):
    """lo[m] = heap position of level m's first entry, m = 0 .. K + 1 (lo[K + 1] = entries of a table whose deepest level is K)"""
    lo = [0]
    for m in range(K + 1):
        lo.append(lo[-1] + t ** m)
    return lo


def strings_at(chars, m, idx):
    """rows `idx` of all_strings(chars, m), as a (len(idx), m) uint16 array"""
    chars, idx = np.asarray(chars, dtype=np.uint16), np.asarray(idx, dtype=np.int64)
    t = len(chars)
    out = np.zeros((len(idx), m), dtype=np.uint16)
    for j in range(m):              # the pattern's LAST symbol is searched first: it is the most significant digit
        out[:, j] = chars[(idx // t ** j) % t]
    return out


def all_strings(chars, m):
    """Every string of m table characters, in the heap order of the level table within level m: pos(s.c) = pos(s) * t + 1 +
    digit(c), where the digit searched first is the pattern's last symbol -- so row i holds the pattern whose j-th symbol is
    chars[(i // t^j) % t], and row i of level m sits at heap position level_offsets(t, m)[m] + i."""
    return strings_at(chars, m, np.arange(len(chars) ** m, dtype=np.int64))


def level_answers(L, chars, K):
    """(first, last) of every entry of levels 0 .. K in heap order, from the reference's L alone: C[c] = #(L < c), Occ(c, i) =
    #(L[:i] == c); a live range steps to first' = C[c] + Occ(c, first), last' = C[c] + Occ(c, last + 1) - 1; an entry whose
    parent is dead keeps the parent's values (the reference stops at the step that emptied the range)."""
    L = np.asarray(L)
    n, t = len(L), len(chars)
    C = [int((L < c).sum()) for c in chars]
    occ = [np.concatenate([[0], np.cumsum(L == c, dtype=np.int64)]) for c in chars]
    f, l = np.array([0], dtype=np.int64), np.array([n - 1], dtype=np.int64)
    firsts, lasts = [f], [l]
    for _ in range(K):
        live = f <= l
        nf, nl = np.empty((len(f), t), dtype=np.int64), np.empty((len(f), t), dtype=np.int64)
        fi, li = np.clip(f, 0, n), np.clip(l + 1, 0, n)
        for d in range(t):
            nf[:, d] = np.where(live, C[d] + occ[d][fi], f)
            nl[:, d] = np.where(live, C[d] + occ[d][li] - 1, l)
        f, l = nf.reshape(-1), nl.reshape(-1)
        firsts.append(f)
        lasts.append(l)
    return np.concatenate(firsts), np.concatenate(lasts)


def _batch(blocks):
    """blocks: [(patterns as an (M, m) array, heap positions or None)] -> Batch"""
    plen = np.concatenate([np.full(len(p), p.shape[1], dtype=np.int32) for p, _ in blocks])
    heap = np.concatenate([np.full(len(p), -1, dtype=np.int64) if h is None else np.asarray(h, dtype=np.int64) for p, h in blocks])
    flat = np.ascontiguousarray(np.concatenate([p.reshape(-1) for p, _ in blocks]).astype(np.uint16))
    starts = np.zeros(len(plen), dtype=np.int64)
    starts[1:] = np.cumsum(plen[:-1], dtype=np.int64)
    return Batch(plen, flat, starts, heap)


def outside_characters(chars):
    """what a pattern may hold that the table does not: SEOF, the codes 3 and 4 (no text has them), a byte + 5 the text lacks
    and 260 (the last code that is not a parameter error)"""
    have = set(int(c) for c in chars)
    lacking = next(c for c in range(5 + 0x41, 260) if c not in have)
    out = [SEOF, 3, 4, lacking, 260]
    assert not have & set(out)
    return np.array(out, dtype=np.uint16)


def level_batch(chars, K, seed, all_next_up_to=300_000, next_sample=100_000, spoilt=20_000):
    """One batch that asks a level table of depth K for everything: every string of 0 .. K table characters in heap order (pattern
    i asks for heap position i); every string of K + 1 where there are at most `all_next_up_to` of them, else a seeded sample of
    `next_sample` (the hand-over from the table to the stepping code); and a seeded `spoilt` strings of 1 .. K + 1 characters
    with one symbol replaced by a character outside the table.  Returns (Batch, entries = the number of table strings)."""
    t = len(chars)
    lo = level_offsets(t, K)
    rng = np.random.Generator(np.random.PCG64(seed))
    blocks = [(all_strings(chars, m), lo[m] + np.arange(t ** m, dtype=np.int64)) for m in range(K + 1)]
    nxt = t ** (K + 1)
    idx = np.arange(nxt, dtype=np.int64) if nxt <= all_next_up_to else np.sort(rng.choice(nxt, next_sample, replace=False))
    blocks.append((strings_at(chars, K + 1, idx), None))
    out = outside_characters(chars)
    per = -(-spoilt // (K + 1))
    left = spoilt
    for m in range(1, K + 2):        # the same share of every length, so that the table is left at every level
        k = min(per, left)
        left -= k
        s = strings_at(chars, m, rng.integers(0, t ** m, k))
        s[np.arange(k), rng.integers(0, m, k)] = out[rng.integers(0, len(out), k)]
        blocks.append((s, None))
    return _batch(blocks), lo[K + 1]


def text_windows(prepared, lengths, seed):
    """For every length in `lengths` (ascending) and every position of the prepared text the window fits at -- windows that hold
    SEOF included -- the window as a pattern, and after each window the same window with one symbol, at a seeded position,
    replaced by ANOTHER table character (most of these miss).  One flat batch in that interleaved order; returns (Batch,
    replaced) with replaced[i] true for the spoilt copies."""
    prepared = np.asarray(prepared, dtype=np.uint16)
    chars = table_chars(prepared)
    t, n = len(chars), len(prepared)
    assert t >= 2
    rng = np.random.Generator(np.random.PCG64(seed))
    blocks = []
    for ln in sorted(set(int(x) for x in lengths if 0 < x <= n)):
        m = n - ln + 1
        w = prepared[np.arange(m, dtype=np.int64)[:, None] + np.arange(ln, dtype=np.int64)[None, :]]
        at = rng.integers(0, ln, m)
        old = w[np.arange(m), at]
        rank = np.searchsorted(chars, old)
        is_char = (rank < t) & (chars[np.minimum(rank, t - 1)] == old)
        pick = np.where(is_char, rng.integers(0, t - 1, m), rng.integers(0, t, m))
        pick = pick + (is_char & (pick >= rank))           # skip the symbol that stands there
        both = np.repeat(w, 2, axis=0)
        both[2 * np.arange(m) + 1, at] = chars[pick]
        blocks.append((both, None))
    b = _batch(blocks)
    replaced = (np.arange(len(b.plen)) & 1).astype(bool)
    return b, replaced


def oracle_answers(oracle, batch, max_occs=3, threads=16):
    """Answers of an oracle.pyoracle.Oracle for a batch"""
    first, last = oracle.count_flat(batch.plen, batch.flat, batch.starts, threads=threads)
    noccs, offs = oracle.locate_flat(batch.plen, batch.flat, batch.starts, max_occs, threads=threads)
    return Answers(first, last, max_occs, noccs, offs)


def pattern_of(batch, i):
    return [int(c) for c in batch.flat[batch.starts[i]:batch.starts[i] + batch.plen[i]]]


def compare_entries(fixture, batch, want, *, count=None, chain=None, capacity=None, upto=None, what=()):
    """The one comparison behind the table tests (pure numpy).  count = (first, last) for the first `upto` patterns of the batch
    (all of them by default) against want.first / want.last; chain = a gpu_common.Chain (anything with first / last / noccs /
    out_starts / offsets / total / overflow; first = last = None in the row-free form) whose offset buffer held `capacity`,
    against want.noccs / want.offs.  The error names the first offending entry: fixture, level (= the pattern's length), heap
    position (-1: not a table string), the string itself, got and want."""
    what = what if isinstance(what, tuple) else (what,)

    def check(field, got, exp, to_pattern=None):
        got, exp = np.asarray(got), np.asarray(exp)
        if len(got) != len(exp):
            raise AssertionError((field, "length", len(got), "want", len(exp), "fixture", fixture) + what)
        bad = np.flatnonzero(got != exp)
        if len(bad):
            k = int(bad[0])
            i = k if to_pattern is None else int(to_pattern(k))
            raise AssertionError((field, "fixture", fixture, "pattern", i, "level", int(batch.plen[i]), "heap position", int(batch.heap[i]),
                                  "string", pattern_of(batch, i), "got", int(got[k]), "want", int(exp[k])) + what)

    if count is not None:
        cut = slice(None) if upto is None else slice(0, upto)
        check("first", count[0][cut], want.first[cut])
        check("last", count[1][cut], want.last[cut])
    if chain is not None:
        if chain.first is not None:
            check("chain first", chain.first, want.first)
            check("chain last", chain.last, want.last)
        check("noccs", chain.noccs, want.noccs)
        ostarts = np.concatenate([[0], np.cumsum(want.noccs, dtype=np.int64)])
        check("out_starts", chain.out_starts[:-1], ostarts[:-1])
        cap = len(want.offs) if capacity is None else capacity
        check("offset", chain.offsets, want.offs[:cap], lambda k: np.searchsorted(ostarts, k, side="right") - 1)
        if (int(chain.out_starts[-1]), chain.total, chain.overflow) != (len(want.offs), len(want.offs), int(len(want.offs) > cap)):
            raise AssertionError(("total", int(chain.out_starts[-1]), chain.total, chain.overflow, "want", len(want.offs), "fixture", fixture) + what)


# ---- an index with "too many rows" under one H-gram -----------------------------------------------------------------------------
CTX_BIG = 0xffffff          # the rows field of a context-table value that says "too many" (ctx_kernels.hip.hpp)
PERIODIC_M = CTX_BIG + 7    # (ab)^M: the 16-gram abab..ab then has exactly 0xffffff rows, baba..ba 0xfffffe -- the field's two ends
PERIODIC_NARROW_M = CTX_BIG + 5      # ... and with this M the 12-grams (the narrow table's longest key over eleven characters)


def periodic_text(M, tail_len, seed):
    """(ab)^M followed by `tail_len` seeded symbols over the nine characters c .. k: eleven characters in all (a byte alphabet:
    two-level lines and context tables), and every string of a's and b's alternating occurs about M times"""
    rng = np.random.Generator(np.random.PCG64(seed))
    tail = rng.integers(ord("c"), ord("c") + 9, tail_len).astype(np.uint8)
    return np.concatenate([np.tile(np.array([ord("a"), ord("b")], dtype=np.uint8), M), tail])


def periodic_sa(text, M, suffix_array):
    """Suffix array of the prepared periodic_text (bytes + 5, then SEOF) in closed form: SEOF first; then the suffixes that
    start with a, then those that start with b, each in text order (of two such suffixes the later one meets the tail first,
    and every tail character is above a and b); then the tail's own suffixes, sorted by `suffix_array` (tests/sa_util.py)."""
    n = len(text)
    tail = np.concatenate([text[2 * M:].astype(np.uint16) + 5, [SEOF]])
    tsa = suffix_array(tail)
    assert tsa[0] == len(tail) - 1 and (text[2 * M:] > ord("b")).all()
    ev = np.arange(0, 2 * M, 2, dtype=np.int64)
    return np.concatenate([[n], ev, ev + 1, tsa[1:] + 2 * M]).astype(np.int64)


def periodic_rows(M, ln, phase):
    """occurrences of the alternating string of ln symbols that starts with a (phase 0) or b (phase 1) in (ab)^M + tail"""
    return max(0, (2 * M - ln - phase) // 2 + 1)


def periodic_batch(text, M, lengths, seed):
    """What asks an index of periodic_text for its big ranges: the alternating strings of 1 .. 48, 100 and 1000 symbols in both
    phases, each followed by a copy with one symbol replaced by the other of a / b (never found beyond one symbol); then
    text_windows of the text's end -- 48 periodic symbols, the junction, the tail -- at `lengths`.  Returns (Batch, expected
    rows of the
    alternating strings in closed form and -1 elsewhere, the number of patterns before the windows)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ab = np.array([ord("a") + 5, ord("b") + 5], dtype=np.uint16)
    blocks, rows = [], []
    for ln in list(range(1, 49)) + [100, 1000]:
        for phase in (0, 1):
            p = ab[(np.arange(ln) + phase) & 1]
            s = p.copy()
            at = int(rng.integers(0, ln))
            s[at] = ab[0] + ab[1] - s[at]
            blocks.append((np.stack([p, s]), None))
            rows += [periodic_rows(M, ln, phase), -1 if ln > 1 else periodic_rows(M, 1, 1 - phase)]
    prepared_end = np.concatenate([text[2 * M - 48:].astype(np.uint16) + 5, [SEOF]])
    w, _ = text_windows(prepared_end, lengths, seed + 1)
    k = len(rows)
    b = _batch(blocks)
    plen = np.concatenate([b.plen, w.plen])
    flat = np.ascontiguousarray(np.concatenate([b.flat, w.flat]))
    starts = np.zeros(len(plen), dtype=np.int64)
    starts[1:] = np.cumsum(plen[:-1], dtype=np.int64)
    return Batch(plen, flat, starts, np.full(len(plen), -1, dtype=np.int64)), np.concatenate([rows, np.full(len(w.plen), -1)]).astype(np.int64), k
