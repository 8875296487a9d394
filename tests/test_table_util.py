"""table_util, the expected values behind tests/test_gpu_tables.py, checked without a GPU: the level recurrence on the golden L
equals the oracle for every entry, the batches hold what they claim, and the comparer fails on each single corruption."""
from collections import namedtuple

import numpy as np
import pytest

import femto_amd

from oracle import pyoracle as po
from sa_util import suffix_array
from table_util import (CTX_BIG, PERIODIC_M, PERIODIC_NARROW_M, SEOF, Answers, all_strings, compare_entries, level_answers, level_batch, level_offsets, oracle_answers,
                        outside_characters, pattern_of, periodic_batch, periodic_rows, periodic_sa, periodic_text, strings_at, table_chars,
                        text_windows)

# fixture, K, entries of levels 0 .. K, dead entries at level K, one-row entries at level K
LEVEL_CASES = [("acgt48k", 8, 87_381, 31_076, 23_104), ("runs3doc", 8, 87_381, 65_495, None), ("b1000", 6, 55_987, 39_918, None),
               ("chunks2doc", 5, 111_111, 94_638, None), ("eng2doc", 2, 8_743, 6_650, None)]
FakeChain = namedtuple("FakeChain", "first last noccs out_starts offsets total overflow")


def test_all_strings_are_in_heap_order():
    chars = np.array([70, 72, 76, 89], dtype=np.uint16)
    assert all_strings(chars, 0).shape == (1, 0)
    assert all_strings(chars, 1)[:, 0].tolist() == [70, 72, 76, 89]
    # pos(s.c) = pos(s) * t + 1 + digit(c), the digit searched first being the pattern's LAST symbol: walk the heap by hand
    t, lo = 4, level_offsets(4, 3)
    assert lo == [0, 1, 5, 21, 85]
    for m in (2, 3):
        s = all_strings(chars, m)
        assert s.shape == (t ** m, m) and len(np.unique(s, axis=0)) == t ** m
        for i in (0, 1, 5, 7, t ** m - 1):
            pos = 0
            for c in s[i][::-1]:                       # searched from the end
                pos = pos * t + 1 + int(np.searchsorted(chars, c))
            assert pos == lo[m] + i, (m, i)
    assert np.array_equal(strings_at(chars, 3, [5, 63]), all_strings(chars, 3)[[5, 63]])


@pytest.mark.parametrize("name,K,entries,dead,one_row", LEVEL_CASES)
def test_level_recurrence_equals_the_oracle_for_every_entry(fixtures, name, K, entries, dead, one_row):
    """level_answers -- Occ as cumulative counts of the golden L, nothing else -- against Oracle.count_flat for every string of
    0 .. K table characters: no mismatch, and the numbers of entries / dead entries the GPU tests rely on."""
    fx = fixtures(name)
    chars = table_chars(fx.prepared_text())
    assert np.array_equal(chars, table_chars(fx.gold["L"]))
    first, last = level_answers(fx.gold["L"], chars, K)
    lo = level_offsets(len(chars), K)
    assert len(first) == len(last) == lo[K + 1] == entries
    batch, n_entries = level_batch(chars, K, seed=1, next_sample=1000, spoilt=100)
    assert n_entries == entries and np.array_equal(batch.heap[:entries], np.arange(entries)) and (batch.heap[entries:] == -1).all()
    o = po.Oracle(fx.index)
    of, ol = o.count_flat(batch.plen[:entries], batch.flat, batch.starts[:entries], threads=16)
    o.close()
    compare_entries(name, batch, Answers(first, last, None, None, None), count=(of, ol), upto=entries, what="oracle vs recurrence")
    rows = (last - first + 1)[lo[K]:]
    assert int((rows <= 0).sum()) == dead and (rows >= 0).all()
    if one_row is not None:
        assert int((rows == 1).sum()) == one_row


def test_level_batch_holds_what_it_claims(fixtures):
    for name, K, all_next in (("acgt48k", 2, True), ("eng2doc", 2, False)):
        fx = fixtures(name)
        chars = table_chars(fx.prepared_text())
        t = len(chars)
        lo = level_offsets(t, K)
        batch, entries = level_batch(chars, K, seed=7)
        again, _ = level_batch(chars, K, seed=7)
        assert all(np.array_equal(a, b) for a, b in zip(batch, again))           # seeded
        n_next = t ** (K + 1) if all_next else 100_000
        assert entries == lo[K + 1] and len(batch.plen) == entries + n_next + 20_000
        assert int(batch.plen.sum()) == len(batch.flat) and batch.plen.max() == K + 1
        nxt = batch.flat[batch.starts[entries]:batch.starts[entries + n_next]].reshape(n_next, K + 1)
        assert np.isin(nxt, chars).all() and len(np.unique(nxt, axis=0)) == n_next
        out = outside_characters(chars)
        assert out[:3].tolist() == [SEOF, 3, 4] and out[4] == 260 and out[3] - 5 not in set(np.concatenate(fx.docs).tolist())
        seen, lengths = set(), set()
        for i in range(entries + n_next, len(batch.plen)):
            p = np.array(pattern_of(batch, i))
            foreign = p[~np.isin(p, chars)]
            assert len(foreign) == 1 and foreign[0] in out, (i, p)
            seen.add(int(foreign[0]))
            lengths.add(len(p))
        assert seen == set(out.tolist()) and lengths == set(range(1, K + 2))


def test_text_windows_interleave_every_window_with_a_spoilt_copy(fixtures):
    fx = fixtures("chunks2doc")
    prepared = fx.prepared_text()
    chars = table_chars(prepared)
    n = len(prepared)
    batch, replaced = text_windows(prepared, {3, 4, 4, 0, n + 1}, seed=5)
    assert len(batch.plen) == 2 * ((n - 2) + (n - 3)) and not replaced[0] and replaced[1] and replaced.sum() * 2 == len(replaced)
    assert (batch.heap == -1).all()
    with_seof = 0
    for i in list(range(0, 400, 2)) + [2 * (n - 2) - 2, 2 * (n - 2), len(batch.plen) - 2]:
        ln = 3 if i < 2 * (n - 2) else 4
        p0 = (i - (0 if ln == 3 else 2 * (n - 2))) // 2
        w, s = np.array(pattern_of(batch, i)), np.array(pattern_of(batch, i + 1))
        assert np.array_equal(w, prepared[p0:p0 + ln]), i
        diff = np.flatnonzero(w != s)
        assert len(diff) == 1 and s[diff[0]] in chars, (i, w, s)          # exactly one symbol, now another table character
    flat2 = batch.flat.reshape(-1)
    for ln, base, m in ((3, 0, n - 2), (4, 2 * (n - 2) * 3, n - 3)):
        w = flat2[base:base + 2 * m * ln].reshape(m, 2, ln)
        assert ((w[:, 0] != w[:, 1]).sum(axis=1) == 1).all()
        with_seof += int((w[:, 0] == SEOF).any(axis=1).sum())
    assert with_seof > 0                                                   # windows over a document end are part of the batch
    again, _ = text_windows(prepared, [4, 3], seed=5)
    assert np.array_equal(again.flat, batch.flat)
    other, _ = text_windows(prepared, [4, 3], seed=6)
    assert not np.array_equal(other.flat, batch.flat)


def test_compare_entries_catches_every_single_corruption(fixtures):
    """A correct answer passes; one value flipped -- first, last, noccs, one offset, and the chain's bookkeeping -- raises, and
    the message names the entry: fixture, level, heap position, string, got and want."""
    fx = fixtures("acgt48k")
    chars = table_chars(fx.prepared_text())
    K = 3
    batch, entries = level_batch(chars, K, seed=3, spoilt=50)
    o = po.Oracle(fx.index)
    want = oracle_answers(o, batch, 3, threads=16)
    o.close()
    lf, ll = level_answers(fx.gold["L"], chars, K)
    level_want = Answers(lf, ll, None, None, None)
    cap = len(want.offs) + 16
    ostarts = np.concatenate([[0], np.cumsum(want.noccs, dtype=np.int64)])
    chain = FakeChain(want.first.copy(), want.last.copy(), want.noccs.copy(), ostarts, want.offs.copy(), len(want.offs), 0)
    compare_entries("acgt48k", batch, want, count=(want.first, want.last), chain=chain, capacity=cap)
    compare_entries("acgt48k", batch, level_want, count=(want.first, want.last), upto=entries)
    compare_entries("acgt48k", batch, want, chain=chain._replace(first=None, last=None), capacity=cap)            # the row-free form
    compare_entries("acgt48k", batch, want, chain=chain._replace(offsets=want.offs[:5], overflow=1), capacity=5)  # a buffer cut short

    def bump(a, i, by=1):
        a = a.copy()
        a[i] += by
        return a

    lo = level_offsets(len(chars), K)
    e = lo[K] + 37                                   # an entry of the deepest level
    hit = int(np.flatnonzero(want.noccs)[5])         # a pattern with offsets, and its first offset
    for field, bad, at in (("first", bump(want.first, e), e), ("last", bump(want.last, e, -1), e), ("first", bump(want.first, 0), 0),
                           ("last", bump(want.last, len(batch.plen) - 1), len(batch.plen) - 1)):
        for w, upto in ((want, None), (level_want, entries)):
            if upto is not None and at >= upto:
                continue
            with pytest.raises(AssertionError) as ei:
                compare_entries("acgt48k", batch, w, count=(bad, want.last) if field == "first" else (want.first, bad), upto=upto)
            msg = ei.value.args[0]
            assert msg[0] == field and msg[msg.index("fixture") + 1] == "acgt48k" and msg[msg.index("level") + 1] == batch.plen[at]
            assert msg[msg.index("heap position") + 1] == batch.heap[at] and msg[msg.index("string") + 1] == pattern_of(batch, at)
            got, exp = msg[msg.index("got") + 1], msg[msg.index("want") + 1]
            assert (got, exp) == (int(bad[at]), int((want.first if field == "first" else want.last)[at]))
        with pytest.raises(AssertionError):
            compare_entries("acgt48k", batch, want, chain=chain._replace(**{field: bad}), capacity=cap)
    for field, bad, at in (("noccs", bump(want.noccs, hit), hit), ("offsets", bump(want.offs, int(ostarts[hit])), hit),
                           ("offsets", bump(want.offs, len(want.offs) - 1), None), ("offsets", want.offs[:-1], None),
                           ("out_starts", bump(ostarts, hit), hit), ("total", chain.total + 1, None), ("overflow", 1, None)):
        for rows in (True, False):
            c = chain if rows else chain._replace(first=None, last=None)
            with pytest.raises(AssertionError) as ei:
                compare_entries("acgt48k", batch, want, chain=c._replace(**{field: bad}), capacity=cap, what=("rows", rows))
            msg = ei.value.args[0]
            assert msg[-2:] == ("rows", rows)
            if at is not None:
                assert msg[msg.index("pattern") + 1] == at and msg[msg.index("string") + 1] == pattern_of(batch, at), msg
    # the offset check knows which pattern an offset belongs to
    with pytest.raises(AssertionError) as ei:
        compare_entries("acgt48k", batch, want, chain=chain._replace(offsets=bump(want.offs, len(want.offs) - 1)), capacity=cap)
    last_hit = int(np.flatnonzero(want.noccs)[-1])
    assert ei.value.args[0][ei.value.args[0].index("pattern") + 1] == last_hit


def test_periodic_suffix_array_in_closed_form():
    """periodic_sa against prefix doubling, and periodic_rows against counting by hand, at sizes where both can be done"""
    for M in (7, 500):
        text = periodic_text(M, 300, seed=1)
        prepared = np.concatenate([text.astype(np.uint16) + 5, [SEOF]])
        assert np.array_equal(periodic_sa(text, M, suffix_array), suffix_array(prepared))
        s = bytes(text)
        for ln in (1, 2, 3, 8, 9, 13, 2 * M, 2 * M + 1):
            for phase in (0, 1):
                p = bytes(b"ab"[(i + phase) & 1] for i in range(ln))
                assert sum(s[i:i + ln] == p for i in range(len(s) - ln + 1)) == periodic_rows(M, ln, phase), (M, ln, phase)
    # the size the GPU test uses puts the 16-grams at the two ends of the 24-bit rows field
    assert (periodic_rows(PERIODIC_M, 16, 0), periodic_rows(PERIODIC_M, 16, 1)) == (CTX_BIG, CTX_BIG - 1)
    assert all(periodic_rows(PERIODIC_M, ln, ph) >= CTX_BIG for ln in range(1, 16) for ph in (0, 1))
    assert (periodic_rows(PERIODIC_NARROW_M, 12, 0), periodic_rows(PERIODIC_NARROW_M, 12, 1)) == (CTX_BIG, CTX_BIG - 1)
    assert all(periodic_rows(PERIODIC_NARROW_M, ln, ph) < CTX_BIG for ln in range(13, 18) for ph in (0, 1))


def test_periodic_index_has_too_many_rows_under_one_gram(tmp_path):
    """The index tests/test_gpu_tables.py opens for the "too many rows" answer of the context tables, written from the closed-form
    suffix array on the CPU: the oracle's counts of the alternating strings are the closed-form ones (16.7 M rows and more),
    their first offsets 0, 2, 4 / 1, 3, 5, and spoilt copies are not found."""
    text = periodic_text(PERIODIC_M, 3000, seed=1)
    path = str(tmp_path / "periodic")
    femto_amd.build_index_from_sa(path, [text], periodic_sa(text, PERIODIC_M, suffix_array), params=None, infos=["periodic"])
    batch, rows, k = periodic_batch(text, PERIODIC_M, (15, 16, 17), seed=9)
    o = po.Oracle(path)
    want = oracle_answers(o, batch, 3, threads=16)
    o.close()
    assert o.total_length == len(text) + 1
    got = want.last - want.first + 1
    known = rows >= 0
    assert known[:k:2].all() and np.array_equal(got[known], rows[known])
    assert (got[1:k:2][batch.plen[1:k:2] > 1] == 0).all()                      # aab / abb never occur
    ostarts = np.concatenate([[0], np.cumsum(want.noccs)])
    for i in (4 * 15, 4 * 15 + 2):                                             # the two 16-grams
        assert batch.plen[i] == 16 and want.noccs[i] == 3
        assert want.offs[ostarts[i]:ostarts[i + 1]].tolist() == ([0, 2, 4] if i == 60 else [1, 3, 5])
    assert (got[k::2] >= 1).all()                                             # every window of the text's end is found
