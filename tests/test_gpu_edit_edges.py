"""`-m gpu`: search within edit distance (femto_amd/edit/edit.hip) where the golden fixtures do not reach: SEOF ranges of hundreds of
rows on the two corpora of tests/corpus_util.py, ranges of hundreds of rows that stay whole for dozens of steps and then split (the
`only` shortcut of edit_kernel<P, 2>), batches of more than one workgroup of patterns and pattern keys of 17 bits, patterns as long
as the cap and one symbol past it, and other users of the leased scratch in between.  Every expectation is the yardstick of
tests/edit_util.py with its rows from ix.count on every listed string and from the CPU oracle on the same index; the preconditions
that keep these cases from going hollow are asserted without a GPU in tests/test_edit_host.py.  (The case at the shipped launch
size of 2^31 lanes stands in tests/test_gpu_fullsize.py.)"""
import numpy as np
import pytest

import classes_util as xu
import corpus_util as cu
import edit_util as eu
import femto_amd
import mismatch_util as mu
from edit_util import variants
from mismatch_util import OFFSET, SEOF, prepared
from oracle import pyoracle
from regexp_util import KINDS, open_kind
from test_gpu_edit import Built, _answer, _device_answer, _expected, _patterns, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _oracle_agrees(ix, index, per, nth=1):
    """the rows of every nth listed string from the CPU oracle on the same index"""
    flat = [v for vs in per for v in vs][::nth]
    first, last = ix.count([v.symbols for v in flat])
    assert np.array_equal(last - first + 1, np.array([v.rows for v in flat], dtype=np.int64))
    o = pyoracle.Oracle(index)
    try:
        f, l = o.count([v.symbols for v in flat])
    finally:
        o.close()
    assert np.array_equal(f, first) and np.array_equal(l, last)


def _answers(B, ix, nth):
    """Built.answers, with the oracle's word on every nth string the first time"""
    fresh = B.want is None
    want = B.answers(ix)
    if fresh:
        _oracle_agrees(ix, B.index, B.per, nth)
    return want


# ---- 1. many documents ----------------------------------------------------------------------------------------------------------

_corpora = {}


def _corpus(tmp_path_factory, name):
    if name not in _corpora:
        docs = cu.edges_docs() if name == "edges" else cu.library_docs().docs
        tagged = eu.corpus_pattern_set(docs, name)
        B = Built(tmp_path_factory, name, docs, [p for _, p in tagged])
        B.tags = [t for t, _ in tagged]
        _corpora[name] = B
    return _corpora[name]


@pytest.fixture(scope="module", params=["edges", "library"])
def corpus(request, tmp_path_factory, gpu_ok):
    return _corpus(tmp_path_factory, request.param)


@pytest.fixture(scope="module")
def library(tmp_path_factory, gpu_ok):
    return _corpus(tmp_path_factory, "library")


def _is_what_it_claims(B, want2):
    start, first, last, cost, length = want2
    of_pattern = np.repeat(np.arange(len(B.pats)), np.diff(start))
    behind = np.array([len(p) > 0 and p[-1] == SEOF for p in B.pats])
    assert behind.sum() >= 1 + 20 + 120 + 3          # SEOF alone, behind every character, behind the tails, behind three documents
    assert len(B.docs) > 256 and (behind[of_pattern] & (cost == 1) & (last - first + 1 >= 100)).any()
    if B.name == "edges":          # the string of SEOF alone, reached from [c, SEOF] by the deletion of c: one row per document
        empty = sum(len(d) == 0 for d in B.docs)
        alone = behind[of_pattern] & (length == 1) & (cost >= 1) & (last - first + 1 == len(B.docs))
        assert empty == 17 and alone.sum() > 20 and (length == 0).any()


@pytest.mark.parametrize("kind", ["ind", "pack2", "wave"])
def test_many_documents(corpus, kind):
    """a pattern that ends in SEOF starts from one row per document (816 on "edges", 17 of them of empty documents; 507 on
    "library"): its site behind the last byte holds that range, every insertion in front of SEOF steps from it ("no insertion
    behind a code below 5" keeps SEOF's own gap shut), and the deletion of the one byte of [c, SEOF] leaves SEOF alone"""
    B = corpus
    ix = open_kind(B.index, kind)
    try:
        want = _answers(B, ix, 5)
        for k in (0, 1, 2):
            _same(ix.edit(B.pats, k), want[k], (B.name, kind, k))
        _is_what_it_claims(B, want[2])
    finally:
        ix.close()


def test_many_documents_device_form(corpus):
    import torch
    B = corpus
    ix = femto_amd.Index(B.index, device=0)
    try:
        want = _answers(B, ix, 5)
        st = torch.cuda.Stream(device=DEV)
        for k in (0, 1, 2):
            got, raw = _device_answer(ix, B.pats, k, st)          # the counting form, then the filling form
            _same(got, want[k], (B.name, k, "device"))
            assert raw >= len(want[k][1])
    finally:
        ix.close()


# ---- 2. wide ranges that stay whole ---------------------------------------------------------------------------------------------

LIBRARY_KINDS = [kind for kind, v in KINDS.items() if v.applies(len(cu.ALPHABET20) + 1)]


@pytest.mark.parametrize("kind", LIBRARY_KINDS)
def test_wide_ranges_that_stay_whole(library, kind):
    """the passage patterns alone, as a batch of their own: the exact step keeps all of 64 .. 305 rows for dozens of steps -- the
    `only` shortcut carries the range on as nf .. nf + (last - first) and searches two second edits -- and then the range splits
    (the passage's first symbol, the noise of group d).  tests/test_edit_host.py shows from the text alone that every pattern of
    the groups a, b, c and e has a string in as many windows as its passage has documents"""
    B = library
    sel = [q for q, t in enumerate(B.tags) if t.startswith("P")]
    assert len(sel) > 150 and len(LIBRARY_KINDS) >= 3
    pats, per = [B.pats[q] for q in sel], [B.per[q] for q in sel]
    ix = open_kind(B.index, kind)
    try:
        _answers(B, ix, 5)
        for k in (1, 2):
            want = _answer(ix, per, k)
            _same(ix.edit(pats, k), want, ("passages", kind, k))
        start, first, last, cost, length = want
        for i, q in enumerate(sel):
            tag = B.tags[q]
            rows = (last - first + 1)[start[i]:start[i + 1]]
            if tag[3] in "abce":
                assert rows.max() >= cu.PASSAGE_DOCS[int(tag[1]) - 1], tag
            elif tag[3] == "f":          # the documents that are the passage and nothing else
                assert rows[cost[start[i]:start[i + 1]] == 0].tolist() == [cu.PURE.count(int(tag[1]) - 1)], tag
        assert ((cost == 2) & (last - first + 1 >= 64)).sum() > 100
    finally:
        ix.close()


# ---- 3. batches past one workgroup ----------------------------------------------------------------------------------------------

BATCHES = (255, 256, 257, 513, 70001)


_base = {}


def _batches(fixtures, ix):
    """acgt48k's pattern set without its patterns of more than 100 symbols, each pattern's answer once"""
    if not _base:
        ps = _patterns(fixtures, "acgt48k")
        _base["keep"] = np.array([q for q, p in enumerate(ps) if len(p) <= 100], dtype=np.int64)          # (on acgt48k: all of them)
        _base["pats"] = [ps[q] for q in _base["keep"]]
        assert 100 < len(_base["keep"]) < 255
    _base["want"] = _expected(fixtures, "acgt48k", ix)
    return _base


def _laid_out(want, keep, order):
    """the answer of the batch keep[order] from the whole set's answer `want`"""
    start = want[0]
    n = np.diff(start)[keep][order]
    begin = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    idx = np.repeat(start[keep][order] - begin[:-1], n) + np.arange(begin[-1])
    return (begin,) + tuple(a[idx] for a in want[1:])


@pytest.mark.parametrize("npat", BATCHES)
def test_batches_past_one_workgroup(fixtures, gpu_ok, npat):
    """exact_kernel and result_start_kernel take one lane per pattern: 255, 256, 257 and 513 patterns put the batch's end on either
    side of a workgroup's, 70 001 make the pattern keys of the second sort 17 bits wide.  The batch is the base under seeded
    permutations, so the answer is each base pattern's, laid out by the permutation.  Raw records at 70 001 patterns, from the
    counting form: see test_batches_past_one_workgroup_device_form"""
    ix = femto_amd.Index(fixtures("acgt48k").index, device=0)
    try:
        b = _batches(fixtures, ix)
        order = eu.repeated(len(b["keep"]), npat, npat)
        pats = [b["pats"][o] for o in order]
        for k in (1, 2):
            _same(ix.edit(pats, k), _laid_out(b["want"][k], b["keep"], order), (npat, k))
    finally:
        ix.close()


@pytest.mark.parametrize("npat", [256, 257, 70001])
def test_batches_past_one_workgroup_device_form(fixtures, gpu_ok, npat):
    """result_start has npat + 1 entries, written by a grid of blocks_for(npat) workgroups -- one more than the patterns need at
    npat = 256 --: every one is written over the -3 it held, and the last is the total.  70 001 patterns leave 541 304 raw records at k = 1 and 9 759 607 at k = 2 (7 163 874 distinct results), far below the 2^31 a call may
    hold"""
    import torch
    ix = femto_amd.Index(fixtures("acgt48k").index, device=0)
    try:
        b = _batches(fixtures, ix)
        order = eu.repeated(len(b["keep"]), npat, npat)
        pats = [b["pats"][o] for o in order]
        st = torch.cuda.Stream(device=DEV)
        for k in (1, 2):
            want = _laid_out(b["want"][k], b["keep"], order)
            got, raw = _device_answer(ix, pats, k, st)
            print("npat %d k %d: %d raw records, %d results" % (npat, k, raw, len(want[1])))
            assert raw < 50_000_000
            assert len(got[0]) == npat + 1 and (got[0] >= 0).all() and got[0][-1] == len(want[1])
            _same(got, want, (npat, k, "device"))
    finally:
        ix.close()


# ---- 4. at the cap --------------------------------------------------------------------------------------------------------------

_cap = {}


def _cap_patterns(fixtures):
    if not _cap:
        fx = fixtures("acgt48k")
        _cap["pats"] = [p for _, p in eu.cap_patterns(fx.docs[0])]
        _cap["per"] = [variants(prepared(fx.docs), p, 2) for p in _cap["pats"]]          # (seconds each: once for the module)
    return _cap


@pytest.mark.parametrize("kind", ["ru", "rum", "pack"])
def test_at_the_cap(fixtures, gpu_ok, kind):
    """meta packs the length into 16 bits: a 32768-symbol cut of acgt48k's document with a deletion and an insertion planted far
    apart, the cut untouched and a 32767-symbol cut.  An insertion in front of or behind the untouched cut gives a string of 32769
    symbols, two give 32770.  (Not under the lane policy: its steps take 60 us each)"""
    fx = fixtures("acgt48k")
    L = _cap_patterns(fixtures)
    ix = open_kind(fx.index, kind)
    try:
        if "want" not in L:
            L["want"] = {k: _answer(ix, L["per"], k) for k in (1, 2)}
            _oracle_agrees(ix, fx.index, L["per"])
        for k in (1, 2):
            got = ix.edit(L["pats"], k)
            _same(got, L["want"][k], (kind, k))
            start, first, last, cost, length = got
            assert (length == 32769).any() and (length == 32770).any() == (k == 2) and (length == 32768).sum() >= 1 + (k == 2)
            assert (start[1] - start[0] >= 1) == (k == 2) and (cost[start[0]:start[1]] == 2).all()          # the planted one needs both
    finally:
        ix.close()


def test_one_symbol_past_the_cap_in_the_device_form(fixtures, gpu_ok):
    """a pattern of 32769 symbols in the middle and one at the end of a batch of short patterns: the exact pass refuses them, they
    have no results and every neighbour has the results it has alone.  The call before has the same layout with 32768 of those
    symbols in their place, which occur: it leaves their owner and non-empty ranges in the sites"""
    import torch
    fx = fixtures("acgt48k")
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    long = doc[100:100 + 32769].astype(np.uint16) + OFFSET
    ps = _patterns(fixtures, "acgt48k")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        whole = _expected(fixtures, "acgt48k", ix)          # the yardstick's answer for the fixture's set, pattern by pattern
        have = np.diff(whole[1][0]) > 0
        near = np.array([q for q, p in enumerate(ps) if 0 < len(p) <= 40 and have[q]][:24], dtype=np.int64)          # the neighbours have results
        assert len(near) == 24 and (np.diff(whole[1][0])[near] > 1).sum() > 12
        short = [ps[q] for q in near]
        batch = short[:12] + [long] + short[12:] + [long]
        before = short[:12] + [long[:32768]] + short[12:] + [long[:32768]]
        st = torch.cuda.Stream(device=DEV)
        for k in (1, 2):
            start, first, last, cost, length = _laid_out(whole[k], near, np.arange(24))
            want = (np.concatenate([start[:13], start[12:], start[-1:]]), first, last, cost, length)
            r, _ = _device_answer(ix, before, k, st)
            assert r[0][13] - r[0][12] >= 1 and r[0][-1] - r[0][-2] >= 1
            got, _ = _device_answer(ix, batch, k, st)
            _same(got, want, (k,))
            assert got[0][12] == got[0][13] and got[0][-2] == got[0][-1] and len(got[0]) == 27
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.edit(batch, 1)
        assert e.value.code == 3
    finally:
        ix.close()


# ---- 5. other users of the scratch in between -----------------------------------------------------------------------------------

def test_other_users_of_the_scratch_in_between(fixtures, gpu_ok):
    """count, an automaton search, a search with substitutions, one with classes, matching lines and common sequences lease the same
    scratch between two searches; the second search is a smaller batch, so rng and owner stand at other offsets of the scratch,
    and the first batch follows once more"""
    fx = fixtures("chunks2doc")
    pats = _patterns(fixtures, "chunks2doc")
    fewer = pats[30:90]
    assert sum(len(p) for p in fewer) < sum(len(p) for p in pats) // 2
    text = prepared(fx.docs)
    per = [variants(text, p, 2) for p in pats]
    cpats, cls = xu.pattern_set(fx.docs, "chunks2doc")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, per, 2)
        want_fewer = _answer(ix, per[30:90], 2)
        _same(ix.edit(pats, 2), want, ("before",))
        first, last = ix.count(pats)
        assert (first <= last).any()
        p = next(p for p in pats if len(p) == 20)
        rs, rf, rl, rlen, rcost, status = ix.regexp_search_batch([b"".join(b"\\x%02x" % (int(ch) - OFFSET) for ch in p)])
        assert not status.any() and len(rf) >= 1
        assert len(ix.mismatch([q for _, q in mu.pattern_set(fx.docs, "chunks2doc")][:100], 2)[1]) > 100
        assert len(ix.classes([q for _, q in cpats], cls)[1]) > len(cpats)
        ex = ix.extractor()
        doc, pos, lens, flags, starts, data = ex.lines(np.arange(0, len(text), 7, dtype=np.int64))
        assert len(data) > 0
        ex.free()
        r = ix.similar(fx.docs[0][:400])
        assert r.n == 400
        _same(ix.edit(fewer, 2), want_fewer, ("after, the smaller batch",))
        _same(ix.edit(pats, 2), want, ("after",))
    finally:
        ix.close()
