"""`-m gpu`: search with character classes (femto_amd/classes/classes.hip) where the golden fixtures do not reach: SEOF ranges of
hundreds of rows on the two corpora of tests/corpus_util.py, texts of one and of two byte characters exhaustively, batches of more
than one workgroup of patterns and pattern keys of 17 bits, a stack as deep as the cap (the link 0x8000 in the stack word), a class
table of 4096 classes and the symbols just outside it, and other users of the leased scratch in between.  Every expectation is the
yardstick of tests/classes_util.py with its rows from ix.count on every listed string and from the CPU oracle on the same index;
tests/test_classes_host.py pins the yardstick on these inputs without a GPU."""
import numpy as np
import pytest

import classes_util as xu
import corpus_util as cu
import edit_util as eu
import femto_amd
import mismatch_util as mu
from classes_util import CLASS, OFFSET, expected, strings
from mismatch_util import prepared
from oracle import pyoracle
from regexp_util import open_kind
from test_gpu_classes import _device_run, _same, _set

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _answer(ix, per):
    """(result_start, first, last) the call owes for patterns whose strings() are `per`"""
    start, flat = expected(per)
    if flat:
        first, last = ix.count([f.symbols for f in flat])
        assert np.array_equal(last - first + 1, np.array([f.rows for f in flat], dtype=np.int64))
    else:
        first, last = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    for q in range(len(per)):
        assert (np.diff(first[start[q]:start[q + 1]]) > 0).all()
    return start, first, last


def _oracle_agrees(ix, index, per, nth=1):
    """the rows of every nth listed string from the CPU oracle on the same index"""
    flat = [f for fs in per for f in fs][::nth]
    first, last = ix.count([f.symbols for f in flat])
    o = pyoracle.Oracle(index)
    try:
        f, l = o.count([x.symbols for x in flat])
    finally:
        o.close()
    assert np.array_equal(f, first) and np.array_equal(l, last)
    assert np.array_equal(last - first + 1, np.array([x.rows for x in flat], dtype=np.int64))


class Built:
    """an index built here: docs (uint8 arrays), index (its path), text (prepared), pats and cls, per (strings() of every pattern),
    want (the answer, filled by the first handle that opens it, with the oracle's word on every nth string)"""

    def __init__(self, tmp_path_factory, name, docs, pats, cls):
        self.name, self.docs, self.pats, self.cls = name, mu.as_arrays(docs), pats, cls
        self.index = str(tmp_path_factory.mktemp("classes_" + name) / "index")
        femto_amd.build_index(self.index, self.docs, params=None, infos=["%s%d" % (name, i) for i in range(len(self.docs))], device=0)
        self.text = prepared(self.docs)
        self.per = [strings(self.text, p, cls) for p in pats]
        self.want = None

    def answers(self, ix, nth=1):
        if self.want is None:
            assert ix.info.number_of_documents == len(self.docs) and ix.info.total_length == len(self.text)
            self.want = _answer(ix, self.per)
            _oracle_agrees(ix, self.index, self.per, nth)
        return self.want


def _full(ix, pats, cls, want, what):
    """the device form with capacity = total"""
    import torch
    total = len(want[1])
    r = _device_run(ix, pats, cls, total, torch.cuda.Stream(device=DEV))
    assert r["total"].tolist() == [total, 0], what
    _same((r["start"], r["first"][:total], r["last"][:total]), want, what)


# ---- 1. many documents ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["edges", "library"])
def corpus(request, tmp_path_factory, gpu_ok):
    name = request.param
    docs = cu.edges_docs() if name == "edges" else cu.library_docs().docs
    tagged, cls = xu.corpus_pattern_set(docs, name)
    B = Built(tmp_path_factory, name, docs, [p for _, p in tagged], cls)
    B.tags = [t for t, _ in tagged]
    return B


def _is_what_it_claims(B, want):
    start, first, last = want
    n = np.diff(start)
    q1, q2, q3 = (B.tags.index(t) for t in ("seof_after_period", "seof_after_period2", "seof_after_abn"))
    ends = {int(d[-1]) for d in B.docs if len(d)}
    assert n[q1] == len(ends) and n[q2] > n[q1] and 1 <= n[q3] <= 3 and len(B.docs) > 500
    assert (last - first + 1)[start[q1]:start[q1 + 1]].sum() == sum(len(d) > 0 for d in B.docs)          # every document that has an end
    classed = [q for q, t in enumerate(B.tags) if "_classed" in t]
    assert len(classed) > 200 and sum(n[q] > 1 for q in classed) > 30 and len(B.pats) > 512
    alone = B.tags.index("seof_alone", 200)          # (the family's, behind pattern_set's own)
    assert n[alone] == 1 and last[start[alone]] - first[start[alone]] + 1 == len(B.docs)


@pytest.mark.parametrize("kind", ["ind", "pack2", "wave"])
def test_many_documents(corpus, kind):
    """a pattern that ends in SEOF starts from one row per document (816 on "edges", 17 of them of empty documents; 507 on
    "library") and a class in front of it fans out from that range: "a class holds bytes alone" keeps the empty documents' rows
    out of every member's step.  (The patterns of two periods stay under the lane policy: some thirty characters, not 256)"""
    B = corpus
    ix = open_kind(B.index, kind)
    try:
        want = B.answers(ix, 2)
        _same(ix.classes(B.pats, B.cls), want, (B.name, kind))
        _is_what_it_claims(B, want)
    finally:
        ix.close()


def test_many_documents_device_form(corpus):
    B = corpus
    ix = femto_amd.Index(B.index, device=0)
    try:
        _full(ix, B.pats, B.cls, B.answers(ix, 2), (B.name, "device"))
    finally:
        ix.close()


# ---- 2. tiny texts, exhaustively ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["one", "two"])
def tiny(request, tmp_path_factory, gpu_ok):
    pats, cls = xu.tiny_patterns()
    return Built(tmp_path_factory, request.param, mu.TINY_TEXTS[request.param], pats, cls)


@pytest.mark.parametrize("kind", ["ru", "rum", "pack", "wave"])
def test_tiny_texts(tiny, kind):
    """member tables of n = 0, 1 and 2: every pattern of 1 to 3 symbols over a, b, c, [ab], [abc], [bc], [c], the period and the
    empty class, bare and with SEOF behind it -- 1639 patterns, seven workgroups.  On "one" the class [bc] and the class [c] keep
    no member and [ab], [abc] and the period keep the text's only character"""
    B = tiny
    ix = open_kind(B.index, kind)
    try:
        want = B.answers(ix)
        assert len(B.pats) == 1639
        _same(ix.classes(B.pats, B.cls), want, (B.name, kind))
        n = np.diff(want[0])
        assert n.max() == (1 if B.name == "one" else 3) and (n == 0).sum() > 400 and (n > 0).sum() > (100 if B.name == "one" else 400)
    finally:
        ix.close()


# ---- 3. batches past one workgroup ----------------------------------------------------------------------------------------------

BATCHES = (255, 256, 257, 70001)
_base = {}


def _batches(fixtures, ix):
    """acgt48k's pattern set without "deep" and "period2", each pattern's answer once"""
    if not _base:
        fx = fixtures("acgt48k")
        tagged, cls = xu.pattern_set(fx.docs, "acgt48k")
        pats = [p for t, p in tagged if t not in ("deep", "period2")]
        assert len(pats) == 198
        per = [strings(prepared(fx.docs), p, cls) for p in pats]
        _base.update(pats=pats, cls=cls, per=per, want=_answer(ix, per))
        _oracle_agrees(ix, fx.index, per)
    return _base


def _laid_out(want, order):
    start, first, last = want
    n = np.diff(start)[order]
    begin = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    idx = np.repeat(start[order] - begin[:-1], n) + np.arange(begin[-1])
    return begin, first[idx], last[idx]


@pytest.mark.parametrize("npat", BATCHES)
def test_batches_past_one_workgroup(fixtures, gpu_ok, npat):
    """classes_kernel takes one lane per pattern, q = blockIdx.x * 256 + threadIdx.x: 255, 256 and 257 patterns put the batch's end
    on either side of a workgroup's, 70 001 make the pattern keys of the second sort 17 bits wide.  The batch is the base under
    seeded permutations, so the answer is each base pattern's, laid out by the permutation"""
    import torch
    ix = femto_amd.Index(fixtures("acgt48k").index, device=0)
    try:
        b = _batches(fixtures, ix)
        order = eu.repeated(len(b["pats"]), npat, npat)
        pats = [b["pats"][o] for o in order]
        want = _laid_out(b["want"], order)
        total = len(want[1])
        assert total > npat
        _same(ix.classes(pats, b["cls"]), want, (npat, "host"))
        if npat in (257, 70001):
            _full(ix, pats, b["cls"], want, (npat, "capacity = total"))
            short = _device_run(ix, pats, b["cls"], total - 1, torch.cuda.Stream(device=DEV))          # the counts do not depend on the capacity
            assert short["total"].tolist() == [total, 1] and np.array_equal(short["start"], want[0])
    finally:
        ix.close()


# ---- 4. at the cap --------------------------------------------------------------------------------------------------------------

_long = {}


def _long_patterns(fixtures):
    if not _long:
        fx = fixtures("acgt48k")
        tagged, cls = xu.long_patterns(fx.docs[0])
        pats = [p for _, p in tagged]
        _long.update(tags=[t for t, _ in tagged], pats=pats, cls=cls, per=[strings(prepared(fx.docs), p, cls) for p in pats])
    return _long


@pytest.mark.parametrize("kind", ["ru", "rum", "pack"])
def test_at_the_cap(fixtures, gpu_ok, kind):
    """the stack word is (right + 1) << 16 | next member: with classes at positions 32766 and 32767 the link is 0x8000, and the cut
    with a class at EVERY one of its 32768 positions makes the stack 32768 entries deep and the return walk the whole chain.
    The same at 32767 symbols, and 4097 symbols all classes.  (Not under the lane policy: its steps take 60 us each)"""
    fx = fixtures("acgt48k")
    L = _long_patterns(fixtures)
    ix = open_kind(fx.index, kind)
    try:
        if "want" not in L:
            L["want"] = _answer(ix, L["per"])
            _oracle_agrees(ix, fx.index, L["per"])
        _same(ix.classes(L["pats"], L["cls"]), L["want"], (kind,))
        n = np.diff(L["want"][0])
        assert (n >= 1).all() and len(n) == 13 and (L["pats"][L["tags"].index("every32768")] & CLASS).all()
    finally:
        ix.close()


# ---- 5. the class table at its size ---------------------------------------------------------------------------------------------

_table = {}


def _table_4096(fixtures):
    if not _table:
        fx = fixtures("acgt48k")
        tagged, cls = xu.table_4096(fx.docs[0])
        pats = [p for _, p in tagged]
        text = prepared(fx.docs)
        _table.update(pats=pats, cls=cls, text=text, per=[strings(text, p, cls) for p in pats])
    return _table


def test_class_table_of_4096(fixtures, gpu_ok):
    """S.tail holds 4096 SubTables, member_table_kernel runs a grid of 4096 and `tab + c` reaches 4095: 4096 distinct classes, pattern
    i with class i at position i % 12"""
    fx = fixtures("acgt48k")
    T = _table_4096(fixtures)
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, T["per"])
        _oracle_agrees(ix, fx.index, T["per"], nth=4)
        n = np.diff(want[0])
        assert len(T["cls"]) == 4096 and (n >= 1).all() and (n > 1).sum() >= 10 and int(T["pats"][4095][4095 % 12]) == CLASS | 4095
        _same(ix.classes(T["pats"], T["cls"]), want, ("host",))
        _full(ix, T["pats"], T["cls"], want, ("device",))
    finally:
        ix.close()


def _spoilt(T, doc, sym, klass_members):
    """three 12-symbol cuts with `sym` at the first, a middle and the last position, over a byte that `klass_members` holds: with
    the class number masked they would have results"""
    out = []
    for at in (0, 5, 11):
        s = next(s for s in range(1000 + 100 * at, len(doc)) if int(doc[s + at]) in klass_members)
        p = doc[s:s + 12].astype(np.uint16) + OFFSET
        p[at] = sym
        out.append(p)
    return out


@pytest.mark.parametrize("what", ["nclasses", "a bit of 0x7000"])
def test_symbols_just_outside_the_class_table(fixtures, gpu_ok, what):
    """CLASS | 4096 beside a table of 4096 classes, and CLASS | 0x1000 | c for a valid class c beside a table of six:
    `(sym & ~kClass) >= nclasses` refuses both, a mask of twelve bits would search class 0 and class c.  Each at a first, a middle
    and a last position: the spoilt pattern has no results, its neighbours keep theirs, and the host form refuses the batch"""
    import torch
    fx = fixtures("acgt48k")
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    T = _table_4096(fixtures)
    if what == "nclasses":
        cls, near, near_per = T["cls"], T["pats"][4096 - 12:], T["per"][4096 - 12:]
        bad = _spoilt(T, doc, CLASS | 4096, xu.SUBSETS[0])
        masked = [np.where(p == (CLASS | 4096), CLASS | 0, p).astype(np.uint16) for p in bad]
    else:
        c = 3
        cls, near, near_per = T["cls"][:6], T["pats"][:6] * 2, T["per"][:6] * 2
        bad = _spoilt(T, doc, CLASS | 0x1000 | c, xu.SUBSETS[c])
        masked = [np.where(p == (CLASS | 0x1000 | c), CLASS | c, p).astype(np.uint16) for p in bad]
    assert all(len(strings(T["text"], p, cls)) >= 1 for p in masked) and all(strings(T["text"], p, cls) == [] for p in bad)
    batch, per = [], []
    for i, p in enumerate(bad):
        batch += near[4 * i:4 * i + 2] + [p] + near[4 * i + 2:4 * i + 4]
        per += near_per[4 * i:4 * i + 2] + [[]] + near_per[4 * i + 2:4 * i + 4]
    assert all(len(per[5 * i + j]) >= 1 for i in range(3) for j in (0, 1, 3, 4))
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, per)
        total = len(want[1])
        st = torch.cuda.Stream(device=DEV)
        r = _device_run(ix, batch, cls, total + 5, st)
        assert r["total"].tolist() == [total, 0]
        _same((r["start"], r["first"][:total], r["last"][:total]), want, (what,))
        assert (r["first"][total:] == -3).all() and (r["last"][total:] == -3).all()
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.classes(batch, cls)
        assert e.value.code == 3
    finally:
        ix.close()


# ---- 6. other users of the scratch in between -----------------------------------------------------------------------------------

def test_other_users_of_the_scratch_in_between(fixtures, gpu_ok):
    """count, an automaton search, a search with substitutions, one within edit distance, matching lines and common sequences lease
    the same scratch between two searches; the second search is a smaller batch whose stack lies at other offsets -- a lane that
    read a stack entry it had not written would pick up the first batch's -- and the first batch follows once more"""
    fx = fixtures("chunks2doc")
    pats, cls = _set(fixtures, "chunks2doc")
    fewer = pats[40:150]
    assert sum(len(p) for p in fewer) < sum(len(p) for p in pats) // 2 and sum((p & CLASS).any() for p in fewer) > 50
    text = prepared(fx.docs)
    per = [strings(text, p, cls) for p in pats]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        want = _answer(ix, per)
        want_fewer = _answer(ix, per[40:150])
        _same(ix.classes(pats, cls), want, ("before",))
        plain = [p for _, p in mu.pattern_set(fx.docs, "chunks2doc")]
        first, last = ix.count(plain)
        assert (first <= last).any()
        p = next(p for p in plain if len(p) == 20)
        rs, rf, rl, rlen, rcost, status = ix.regexp_search_batch([b"".join(b"\\x%02x" % (int(ch) - OFFSET) for ch in p)])
        assert not status.any() and len(rf) >= 1
        assert len(ix.mismatch(plain[:100], 2)[1]) > 100
        assert len(ix.edit([q for _, q in eu.pattern_set(fx.docs, "chunks2doc")], 2)[1]) > 100
        ex = ix.extractor()
        doc, pos, lens, flags, starts, data = ex.lines(np.arange(0, len(text), 7, dtype=np.int64))
        assert len(data) > 0
        ex.free()
        r = ix.similar(fx.docs[0][:400])
        assert r.n == 400
        _same(ix.classes(fewer, cls), want_fewer, ("after, the smaller batch",))
        _same(ix.classes(pats, cls), want, ("after",))
    finally:
        ix.close()
