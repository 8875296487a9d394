"""`-m gpu`: search with substitutions (femto_amd/mismatch/mismatch.hip) where the golden fixtures do not reach: SEOF ranges of
hundreds of rows on the two corpora of tests/corpus_util.py, texts of one and of two byte characters, patterns as long as the cap,
what the device form is handed (symbols and starts the host form would refuse, stale owners and ranges in the leased scratch),
other users of that scratch in between, a batch of one pattern, and a batch of 256 with slots behind its results.  Every
expectation is the yardstick of tests/mismatch_util.py (variants / expected) with its rows from ix.count on every variant and from
the CPU oracle on the same index; the preconditions that keep these cases from going hollow are asserted without a GPU in
tests/test_mismatch_host.py.  (The case that needs 2^31 lanes stands in tests/test_gpu_fullsize.py.)"""
import numpy as np
import pytest

import corpus_util as cu
import edit_util as eu
import femto_amd
import mismatch_util as mu
from mismatch_util import OFFSET, SEOF, expected, pattern_set, prepared, variants
from oracle import pyoracle
from regexp_util import KINDS, open_kind
from test_gpu_mismatch import _device_run, _expected, _patterns, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _count(ix, flat):
    if not flat:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    first, last = ix.count([v.symbols for v in flat])
    assert np.array_equal(last - first + 1, np.array([v.rows for v in flat], dtype=np.int64))
    return first, last


def _answer(ix, per, k):
    """(result_start, first, last, cost, sub_pos, sub_sym) the call owes for patterns whose variants(.., 2) are `per`"""
    start, flat, cost, pos, sym = expected(per, k)
    first, last = _count(ix, flat)
    for q in range(len(per)):
        assert (np.diff(first[start[q]:start[q + 1]]) > 0).all()
    return start, first, last, cost, pos, sym


def _oracle_agrees(ix, index, per, nth=1):
    """the rows of every nth variant from the CPU oracle on the same index"""
    flat = [v for vs in per for v in vs][::nth]
    first, last = _count(ix, flat)
    o = pyoracle.Oracle(index)
    try:
        f, l = o.count([v.symbols for v in flat])
    finally:
        o.close()
    assert np.array_equal(f, first) and np.array_equal(l, last)


def _of(r, total=None):
    t = slice(None) if total is None else slice(0, total)
    return (r["start"], r["first"][t], r["last"][t], r["cost"][t], r["pos"][t], r["sym"][t])


class Built:
    """an index built here: docs (uint8 arrays), index (its path), text (prepared), pats, per (variants(.., 2) of every pattern),
    want[k] (the answer, filled by the first handle that opens it)"""

    def __init__(self, tmp_path_factory, name, docs, pats):
        self.name, self.docs, self.pats = name, mu.as_arrays(docs), pats
        self.index = str(tmp_path_factory.mktemp(name) / "index")
        femto_amd.build_index(self.index, self.docs, params=None, infos=["%s%d" % (name, i) for i in range(len(self.docs))], device=0)
        self.text = prepared(self.docs)
        self.per = [variants(self.text, p, 2) for p in pats]
        self.want = None

    def answers(self, ix):
        if self.want is None:
            assert ix.info.number_of_documents == len(self.docs) and ix.info.total_length == len(self.text)
            self.want = {k: _answer(ix, self.per, k) for k in (0, 1, 2)}
            _oracle_agrees(ix, self.index, self.per)
        return self.want


def _run_kind(B, kind):
    ix = open_kind(B.index, kind)
    try:
        want = B.answers(ix)
        got = {k: ix.mismatch(B.pats, k) for k in (0, 1, 2)}
        for k in (0, 1, 2):
            _same(got[k], want[k], (B.name, kind, k))
        return got
    finally:
        ix.close()


# ---- 1. many documents ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["edges", "library"])
def corpus(request, tmp_path_factory, gpu_ok):
    name = request.param
    docs = cu.edges_docs() if name == "edges" else cu.library_docs().docs
    return Built(tmp_path_factory, name, docs, [p for _, p in mu.corpus_pattern_set(docs, name)])


@pytest.mark.parametrize("kind", ["ind", "pack2", "wave"])
def test_many_documents(corpus, kind):
    """a pattern that ends in SEOF starts its exact pass on one row per document (816 on "edges", 17 of them of empty documents;
    507 on "library") and every substitution lane left of it steps from a range that wide; a pattern of three symbols has more
    than a thousand variants to emit and to sort"""
    B = corpus
    got = _run_kind(B, kind)
    start, first, last, cost, pos, sym = got[2]
    assert max(len(vs) for vs in B.per) > 1000 and int(np.diff(start).max()) > 1000
    behind = np.array([len(p) > 0 and p[-1] == SEOF for p in B.pats])
    assert behind.sum() >= 1 + 20 + 120 + 3          # SEOF alone, behind every character, behind the tails, behind three documents
    of_pattern = np.repeat(np.arange(len(B.pats)), np.diff(start))
    nonempty = np.array([len(p) > 0 for p in B.pats])
    assert ((last - first + 1 > 256) & nonempty[of_pattern]).any() and len(B.docs) > 256
    # the lanes of the byte in front of a final SEOF step from the SEOF range itself, one row per document
    before = np.array([len(p) - 2 for p in B.pats])[of_pattern]
    through = behind[of_pattern] & (cost >= 1) & ((pos[:, 0] == before) | (pos[:, 1] == before))
    assert through.sum() > 100 and (through & (cost == 2)).sum() > 50 and (last - first + 1)[through].max() > 16
    alone = [q for q, p in enumerate(B.pats) if len(p) == 1 and p[0] == SEOF]
    assert all(last[start[q]] - first[start[q]] + 1 == len(B.docs) and start[q + 1] - start[q] == 1 for q in alone) and alone


# ---- 2. tiny alphabets, exhaustively --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["one", "two"])
def tiny(request, tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, request.param, mu.TINY_TEXTS[request.param], mu.tiny_patterns())


@pytest.mark.parametrize("kind", ["ru", "rum", "pack", "wave"])
def test_tiny_alphabets(tiny, kind):
    """nsub = 1 and nsub = 2 in `g = t / nsub`, `pair[t - g * nsub]`: every string over a, b and a character neither text holds,
    1 to 5 symbols, bare and with SEOF behind it.  With one character in the text, every lane whose pattern character is that
    character quits, and only c is ever substituted"""
    B = tiny
    got = _run_kind(B, kind)
    a = ord("a") + OFFSET
    if B.name == "one":
        for k in (1, 2):
            start, first, last, cost, pos, sym = got[k]
            assert len(first) > 40 and (sym[pos >= 0] == a).all()
            for q, p in enumerate(B.pats):
                if len(p) and (p[:len(p) - (p[-1] == SEOF)] == a).all():          # a alone: the k = 0 result and no other
                    assert np.array_equal(cost[start[q]:start[q + 1]], got[0][3][got[0][0][q]:got[0][0][q + 1]]), (k, q)
                    assert start[q + 1] - start[q] <= 1


# ---- 3. patterns as long as the cap ---------------------------------------------------------------------------------------------

_long = {}


def _long_patterns(fixtures):
    if not _long:
        fx = fixtures("acgt48k")
        longs = mu.long_patterns(fx.docs[0])
        _long["pats"] = [p for _, p, _ in longs]
        _long["per"] = [variants(prepared(fx.docs), p, 2) for p in _long["pats"]]
        assert all(len(vs) == 1 for vs in _long["per"])
    return _long


@pytest.mark.parametrize("kind", ["ru", "rum", "pack", "wave"])
def test_patterns_as_long_as_the_cap(fixtures, gpu_ok, kind):
    """positions share 16 bits with kUnused = 0xffff: cuts of acgt48k's document of 32768, 32767 and 4097 symbols with other
    characters planted at the last, the first, both, the last two and the two middle positions.  The lane that owns position
    32767 walks the whole pattern; under k = 2 it tries every other character at every position on the way"""
    fx = fixtures("acgt48k")
    L = _long_patterns(fixtures)
    ix = open_kind(fx.index, kind)
    try:
        if "want" not in L:
            L["want"] = {k: _answer(ix, L["per"], k) for k in (1, 2)}
            _oracle_agrees(ix, fx.index, L["per"])
        for k in (1, 2):
            got = ix.mismatch(L["pats"], k)
            _same(got, L["want"][k], (kind, k))
            pos = got[4]
            assert ((pos[:, 0] == 32767) & (pos[:, 1] == -1)).any()
            assert ((pos[:, 0] == 0) & (pos[:, 1] == 32767)).any() == (k == 2)
            assert ((pos[:, 0] == 32766) & (pos[:, 1] == 32767)).any() == (k == 2) and (got[3] == 0).sum() == 1
    finally:
        ix.close()


# ---- 4. what the device form is handed ------------------------------------------------------------------------------------------

class _Handed:
    pass


@pytest.fixture(scope="module")
def handed(fixtures, gpu_ok):
    """eng2doc's pattern set with one of its patterns of 7 .. 12 symbols in front (pattern 0 has five symbols to lose), each
    pattern's variants alone"""
    fx = fixtures("eng2doc")
    H = _Handed()
    ps = [p for _, p in pattern_set(fx.docs, "eng2doc")]
    q0 = next(q for q, p in enumerate(ps) if 7 <= len(p) <= 12)
    H.fx, H.text = fx, prepared(fx.docs)
    H.pats = [ps[q0]] + ps[:q0] + ps[q0 + 1:]
    H.per = [variants(H.text, p, 2) for p in H.pats]
    H.nsyms = sum(len(p) for p in H.pats)
    return H


def _prime(ix, H, k, st):
    """the full set first: the leased scratch then holds its owners and ranges"""
    total = int(expected(H.per, k)[0][-1])
    r = _device_run(ix, H.pats, k, total, st)
    assert r["total"].tolist() == [total, 0]


def test_device_form_symbols_the_host_form_refuses(handed):
    """261, 0x7fff and 0xffff at the first, a middle and the last position of cuts that match without them: matched by nothing,
    substituted by nothing (code_or_none, and `own >= kAlpha` in subst_kernel), and the patterns around them keep their results"""
    import torch
    H = handed
    doc = H.fx.docs[0].astype(np.uint16) + OFFSET
    bad = []
    for n, code in enumerate((261, 0x7fff, 0xffff)):
        for m, at in enumerate((0, 9, 19)):
            s = 40 + 50 * (3 * n + m)
            p = doc[s:s + 20].copy()
            assert len(variants(H.text, p, 0)) == 1
            p[at] = code
            bad.append(p)
    rich = [q for q, vs in enumerate(H.per) if len(vs) > 1]          # the neighbours: 30 patterns with several results, then 30 others
    near = [H.pats[q] for q in rich[:30] + [q for q in range(len(H.pats)) if q not in rich[:30]][:30]]
    near = [near[(7 * i) % 60] for i in range(60)]          # (mixed: 7 and 60 share no factor)
    pats = []
    for i, p in enumerate(bad):
        pats += near[4 * i:4 * i + 4] + [p]
    pats += near[4 * len(bad):]
    per = [variants(H.text, p, 2) for p in pats]
    assert all(per[5 * i + 4] == [] for i in range(len(bad))) and sum(len(vs) > 1 for vs in per) > 20
    ix = femto_amd.Index(H.fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        _oracle_agrees(ix, H.fx.index, per)
        for k in (0, 1, 2):
            want = _answer(ix, per, k)
            total = len(want[1])
            _prime(ix, H, k, st)
            r = _device_run(ix, pats, k, total + 6, st)
            assert r["total"].tolist() == [total, 0]
            _same(_of(r, total), want, (k,))
            assert (r["first"][total:] == -3).all() and (r["pos"][total:] == -3).all() and (r["sym"][total:] == 7).all()
            with pytest.raises(femto_amd.FemtoAmdError) as e:          # (the host form refuses what it can: 261 and above)
                ix.mismatch(pats, k)
            assert e.value.code == 3
    finally:
        ix.close()


def _starts_cases(H):
    """(name, edit, per): the inputs with one thing wrong, and what every pattern then owes"""
    npat, nsyms = len(H.pats), H.nsyms
    j = next(j for j in range(100, npat - 1) if len(H.per[j - 1]) > 1 and len(H.per[j]) > 1)          # both have results to lose
    assert 2 <= j <= npat - 2
    lost = [vs if q not in (j - 1, j) else [] for q, vs in enumerate(H.per)]

    def entry(q, value):
        def edit(starts, flat, n):
            starts[q] = value
            return starts, flat, n
        return edit

    def longer(starts, flat, n):          # seven symbols behind the last pattern: a cut that occurs, owned by nobody
        return starts, np.concatenate([flat[:n], H.pats[0][:7]]), n + 7

    shorter = [variants(H.text, H.pats[0][5:], 2)] + H.per[1:]
    assert len(shorter[0]) > len(H.per[0]) and all(len(v.symbols) == len(H.pats[0]) - 5 for v in shorter[0])
    return [("start -4", entry(j, -4), lost), ("start nsyms + 9", entry(j, nsyms + 9), lost), ("starts[0] = 5", entry(0, 5), shorter),
            ("nsyms + 7", longer, H.per)]


def test_device_form_starts_that_leave_the_symbols(handed):
    """d_starts is never read on the host.  One entry at -4 or at nsyms + 9: the two patterns it bounds have no results
    (exact_kernel's and subst_kernel's test of s, len and s + len) although owner[] and rng[] still hold them from the call
    before; d_starts[0] = 5: pattern 0 is what follows its first five symbols, and those five belong to nobody (`g < s`); nsyms stated 7
    above d_starts[npat]: seven symbols nobody owns, whose owner[] is whatever the scratch held.  Every other pattern has
    exactly the results it has alone, d_total is their sum and nothing is written behind them"""
    import torch
    H = handed
    ix = femto_amd.Index(H.fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        _oracle_agrees(ix, H.fx.index, H.per, nth=3)
        for name, edit, per in _starts_cases(H):
            for k in (0, 1, 2):
                want = _answer(ix, per, k)
                total = len(want[1])
                _prime(ix, H, k, st)
                r = _device_run(ix, H.pats, k, total + 9, st, edit=edit)
                assert r["total"].tolist() == [total, 0], (name, k)
                _same(_of(r, total), want, (name, k))
                assert (r["first"][total:] == -3).all() and (r["last"][total:] == -3).all() and (r["cost"][total:] == -3).all(), (name, k)
                assert (r["pos"][total:] == -3).all() and (r["sym"][total:] == 7).all(), (name, k)
                c0 = _device_run(ix, H.pats, k, 0, st, arrays=False, edit=edit)
                assert c0["total"].tolist() == [total, int(total > 0)] and np.array_equal(c0["start"], want[0]), (name, k)
    finally:
        ix.close()


LOW_CASES = [(name, kind) for name, nchars in (("eng2doc", 94), ("acgt48k", 5)) for kind, v in KINDS.items() if v.applies(nchars)]


@pytest.mark.parametrize("name,kind", LOW_CASES)
def test_codes_below_the_byte_characters(fixtures, gpu_ok, name, kind):
    """0, 1, 3 and 4 are no byte characters and not SEOF; only the host form can pass them.  P::code_of of every policy leaves them
    empty: at the first, a middle and the last position of cuts that match, they match nothing and are never substituted"""
    fx = fixtures(name)
    text = prepared(fx.docs)
    doc = fx.docs[0].astype(np.uint16) + OFFSET
    pats = []
    for n, code in enumerate((0, 1, 3, 4)):
        for m, at in enumerate((0, 7, 15)):
            s = 30 + 40 * (3 * n + m)
            p = doc[s:s + 16].copy()
            pats.append(p.copy())
            p[at] = code
            pats.append(p)
    per = [variants(text, p, 2) for p in pats]
    assert all(per[2 * i + 1] == [] and any(not v.subs for v in per[2 * i]) for i in range(12))
    ix = open_kind(fx.index, kind)
    try:
        _oracle_agrees(ix, fx.index, per)
        for k in (0, 1, 2):
            got = ix.mismatch(pats, k)
            _same(got, _answer(ix, per, k), (name, kind, k))
            assert (np.diff(got[0])[1::2] == 0).all() and (np.diff(got[0])[0::2] >= 1).all()
    finally:
        ix.close()


# ---- 5. other users of the scratch in between -----------------------------------------------------------------------------------

def test_other_users_of_the_scratch_in_between(fixtures, gpu_ok):
    """count, an automaton search, matching lines and common sequences lease the same scratch between two searches; the second
    search is a smaller batch, so rng and owner stand at other offsets of the scratch, and the first batch follows once more"""
    fx = fixtures("chunks2doc")
    pats = [p for _, p in pattern_set(fx.docs, "chunks2doc")]
    fewer = pats[40:190]
    assert sum(len(p) for p in fewer) < sum(len(p) for p in pats) // 2
    text = prepared(fx.docs)
    per = [variants(text, p, 2) for p in pats]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, per, 2)
        want_fewer = _answer(ix, per[40:190], 2)
        _same(ix.mismatch(pats, 2), want, ("before",))
        first, last = ix.count(pats)
        assert (first <= last).any()
        p = next(p for p in pats if len(p) == 20)
        f, l, m, c = ix.regexp_search(b"".join(b"\\x%02x" % (int(ch) - OFFSET) for ch in p), approx=(1, 1, 2, 2))
        assert len(f) >= 1
        ex = ix.extractor()
        doc, pos, lens, flags, starts, data = ex.lines(np.arange(0, len(text), 7, dtype=np.int64))
        assert len(data) > 0
        ex.free()
        r = ix.similar(fx.docs[0][:400])
        assert r.n == 400
        _same(ix.mismatch(fewer, 2), want_fewer, ("after, the smaller batch",))
        _same(ix.mismatch(pats, 2), want, ("after",))
    finally:
        ix.close()


# ---- 6. one pattern ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,length", [("acgt48k", 8), ("bytes256", 2)])
def test_one_pattern_at_every_capacity(fixtures, gpu_ok, name, length):
    """npat = 1: the pattern keys are one bit wide and the dead slots' key is 1"""
    import torch
    fx = fixtures(name)
    p = fx.docs[0][1000:1000 + length].astype(np.uint16) + OFFSET
    per = [variants(prepared(fx.docs), p, 2)]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, per, 2)
        if name == "acgt48k":
            _oracle_agrees(ix, fx.index, per)
        start, first, last, cost, pos, sym = want
        total = len(first)
        assert total > 40 and start.tolist() == [0, total]
        st = torch.cuda.Stream(device=DEV)
        c0 = _device_run(ix, [p], 2, 0, st, arrays=False)
        assert c0["total"].tolist() == [total, 1] and np.array_equal(c0["start"], start)
        for cap in (1, total - 1):
            short = _device_run(ix, [p], 2, cap, st)
            assert short["total"].tolist() == [total, 1] and np.array_equal(short["start"], start)
        full = _device_run(ix, [p], 2, total, st)
        assert full["total"].tolist() == [total, 0]
        _same(_of(full), want, (name, "capacity = total"))
        more = _device_run(ix, [p], 2, total + 5, st)          # slots behind the results are not written
        assert more["total"].tolist() == [total, 0]
        _same(_of(more, total), want, (name, "capacity = total + 5"))
        assert (more["first"][total:] == -3).all() and (more["last"][total:] == -3).all() and (more["cost"][total:] == -3).all()
        assert (more["pos"][total:] == -3).all() and (more["sym"][total:] == 7).all()
    finally:
        ix.close()


# ---- 7. a power of two of patterns with slots behind the results ----------------------------------------------------------------

def test_power_of_two_patterns_with_slots_behind_the_results(fixtures, gpu_ok):
    """npat = 256 and capacity = total + 300: the 300 slots behind the live records carry the pattern key 256, which needs
    bits_of(256) = 9 bits where the largest pattern number, 255, needs 8 -- sorted over 8 bits they would stand among pattern 0's
    results.  The batch is acgt48k's pattern set under seeded permutations (edit_util.repeated), so the answer is each base
    pattern's, laid out by the permutation"""
    import torch
    base = _patterns(fixtures, "acgt48k")
    npat, k = 256, 1
    order = eu.repeated(len(base), npat, npat)
    pats = [base[o] for o in order]
    ix = femto_amd.Index(fixtures("acgt48k").index, device=0)
    try:
        want = _expected(fixtures, "acgt48k", ix)[k]
        start = want[0]
        n = np.diff(start)[order]
        begin = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        idx = np.repeat(start[order] - begin[:-1], n) + np.arange(begin[-1])
        laid_out = (begin,) + tuple(a[idx] for a in want[1:])
        total = int(begin[-1])
        assert total > 0 and (n[1:] > 0).any()          # results of a pattern other than 0: the ones a key of 0 would stand in front of
        r = _device_run(ix, pats, k, total + 300, torch.cuda.Stream(device=DEV))
        assert r["total"].tolist() == [total, 0]
        _same(_of(r, total), laid_out, (npat, k))
        assert (r["first"][total:] == -3).all() and (r["last"][total:] == -3).all() and (r["cost"][total:] == -3).all()
        assert (r["pos"][total:] == -3).all() and (r["sym"][total:] == 7).all()
    finally:
        ix.close()
