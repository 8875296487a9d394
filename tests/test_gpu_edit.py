"""`-m gpu`: search within edit distance (include/femto_amd.h "search within edit distance", femto_amd/edit/edit.hip) against the
yardstick of tests/edit_util.py, which tests/test_edit_host.py pins to a plain dynamic programme and to the CPU oracle: every
fixture with k = 0, 1, 2 in the host and the device form, every rank policy, the edit pass in several launches, the automaton route
on the same handle, tiny texts exhaustively, the capacities, what the device form is handed, and one long pattern.  The rows come
from ix.count on every string the yardstick lists."""
import numpy as np
import pytest

import femto_amd
import mismatch_util as mu
from edit_util import expected, pattern_set, tiny_patterns, variants
from mismatch_util import OFFSET, prepared
from regexp_util import KINDS, open_kind, text_chars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NCHARS = {"acgt48k": 5, "b1000": 7, "bytes256": 257, "eng2doc": 94, "chunks2doc": 11, "runs3doc": 5, "counter400_small": 7, "construct_kat": 11}
FIXTURES = list(NCHARS)
KIND_CASES = [(name, kind) for name in ("acgt48k", "eng2doc", "bytes256") for kind, v in KINDS.items() if v.applies(NCHARS[name])]
FIELDS = ("result_start", "first", "last", "cost", "length")
_want = {}


def _patterns(fixtures, name):
    return [p for _, p in pattern_set(fixtures(name).docs, name)]


def _answer(ix, per, k):
    """(result_start, first, last, cost, length) the call owes for patterns whose variants(.., 2) are `per`"""
    start, flat, cost, length = expected(per, k)
    if flat:
        first, last = ix.count([v.symbols for v in flat])
        assert np.array_equal(last - first + 1, np.array([v.rows for v in flat], dtype=np.int64))
    else:
        first, last = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    for q in range(len(per)):          # the yardstick's order is the order of (first, length)
        f, n = first[start[q]:start[q + 1]], length[start[q]:start[q + 1]]
        assert ((np.diff(f) > 0) | ((np.diff(f) == 0) & (np.diff(n) > 0))).all()
    return start, first, last, cost, length


def _expected(fixtures, name, ix):
    """{k: the answer for the fixture's pattern set}, computed once"""
    if name not in _want:
        fx = fixtures(name)
        assert len(text_chars(fx.docs)) == NCHARS[name]
        text = prepared(fx.docs)
        per = [variants(text, p, 2) for p in _patterns(fixtures, name)]
        _want[name] = {k: _answer(ix, per, k) for k in (0, 1, 2)}
    return _want[name]


def _same(got, want, what):
    for g, w, field in zip(got, want, FIELDS):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what + (field, np.nonzero(g != w)[0][:8] if g.shape == w.shape else g.shape)


def _device_run(ix, pats, k, capacity, stream, arrays=True, edit=None):
    """femto_amd_edit_device on `stream`, chained after the upload on that stream with no synchronisation in between.
    edit(starts, flat, nsyms) -> (starts, flat, nsyms): what the call is handed in place of the well-formed inputs"""
    import torch
    plen, flat, starts = femto_amd.flatten(pats)
    nsyms = int(plen.sum())
    starts = np.concatenate([starts, [nsyms]]).astype(np.int64)
    if edit is not None:
        starts, flat, nsyms = edit(starts.copy(), flat.copy(), nsyms)
    if len(flat) == 0:
        flat = np.zeros(1, dtype=np.uint16)
    with torch.cuda.stream(stream):
        d_syms = torch.from_numpy(flat.view(np.int16)).to(DEV, non_blocking=True)
        d_starts = torch.from_numpy(starts).to(DEV, non_blocking=True)
        cap = max(capacity, 1)
        o = dict(start=torch.full((len(pats) + 1,), -3, dtype=torch.int64, device=DEV), first=torch.full((cap,), -3, dtype=torch.int64, device=DEV),
                 last=torch.full((cap,), -3, dtype=torch.int64, device=DEV), cost=torch.full((cap,), -3, dtype=torch.int32, device=DEV),
                 length=torch.full((cap,), -3, dtype=torch.int32, device=DEV), total=torch.full((3,), -3, dtype=torch.int64, device=DEV))
        a = (o["start"], o["first"], o["last"], o["cost"], o["length"]) if arrays else (None,) * 5
        ix.edit_device(len(pats), nsyms, d_syms, d_starts, k, capacity, *a, o["total"], stream=stream.cuda_stream)
    stream.synchronize()
    return {key: v.cpu().numpy() for key, v in o.items()}


def _of(r):
    t = int(r["total"][0])
    return (r["start"], r["first"][:t], r["last"][:t], r["cost"][:t], r["length"][:t])


def _device_answer(ix, pats, k, stream, edit=None):
    """the counting form sizes the filling call, as the header prescribes; nothing is written behind the distinct results"""
    c0 = _device_run(ix, pats, k, 0, stream, arrays=False, edit=edit)
    raw = int(c0["total"][2])
    assert c0["total"][1] == int(raw > 0) and (c0["start"] == -3).all()
    r = _device_run(ix, pats, k, raw + 3, stream, edit=edit)
    total = int(r["total"][0])
    assert r["total"].tolist() == [total, 0, raw] and 0 <= total <= raw
    assert all((r[key][total:] == -3).all() for key in ("first", "last", "cost", "length"))
    return _of(r), raw


# ---- 5. the yardstick, bit for bit ------------------------------------------------------------------------------------------------

def _check_handle(ix, pats, want, what, modes, device_form=True):
    import torch
    st = torch.cuda.Stream(device=DEV)
    for mode in modes:
        ix.set_rank_mode(mode)
        for k in ((0, 1, 2) if mode else (1,)):
            _same(ix.edit(pats, k), want[k], what + (mode, k, "host"))
            if device_form:
                got, raw = _device_answer(ix, pats, k, st)
                _same(got, want[k], what + (mode, k, "device"))
                assert raw >= len(want[k][1])


@pytest.mark.parametrize("name", FIXTURES)
def test_equals_the_yardstick(fixtures, gpu_ok, name):
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        want = _expected(fixtures, name, ix)
        _check_handle(ix, pats, want, (name,), [ix.rank_mode])
        cost, length = want[2][3], want[2][4]
        m = np.repeat(np.array([len(p) for p in pats]), np.diff(want[2][0]))
        assert all((cost == c).sum() > 0 for c in (0, 1, 2)) and set((length - m).tolist()) == {-2, -1, 0, 1, 2}
    finally:
        ix.close()


@pytest.mark.parametrize("name,kind", KIND_CASES)
def test_every_rank_policy(fixtures, gpu_ok, name, kind):
    pats = _patterns(fixtures, name)
    ix = open_kind(fixtures(name).index, kind)
    try:
        want = _expected(fixtures, name, ix)
        # the host form, which is the device form twice (test_equals_the_yardstick runs both on every fixture); mode 0 with the
        # derived lines is the same lane policy
        _check_handle(ix, pats, want, (name, kind), [ix.rank_mode] + ([0] if kind == "wave" else []), device_form=False)
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "bytes256"])
def test_edit_pass_in_several_launches(fixtures, gpu_ok, monkeypatch, name):
    """a launch carries fewer than 2^32 lanes and a batch may need 2^41: the pass goes out in launches of whole workgroups, each
    told its first lane.  FEMTO_AMD_EDIT_CHUNK (lanes per launch) makes that happen at these sizes: five launches or so, cut
    inside a site's edits wherever 256 is no multiple of their number, and one workgroup per launch"""
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        want = _expected(fixtures, name, ix)
        nedits = 2 * (NCHARS[name] - 1) + 1
        lanes = (sum(len(p) for p in pats) + len(pats)) * nedits
        for k in (1, 2):
            monkeypatch.setenv("FEMTO_AMD_EDIT_CHUNK", str(lanes // 5))
            _same(ix.edit(pats, k), want[k], (name, k, lanes // 5))
        few = [p for p in pats if len(p) <= 24][:12]
        monkeypatch.delenv("FEMTO_AMD_EDIT_CHUNK")
        whole = ix.edit(few, 2)
        assert len(whole[1]) > len(few)
        monkeypatch.setenv("FEMTO_AMD_EDIT_CHUNK", "1")         # below a workgroup: one workgroup of 256 lanes per launch
        _same(ix.edit(few, 2), whole, (name, 2, 256))
    finally:
        ix.close()


# ---- 6. the automaton route on the same handle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_contains_what_the_automaton_route_finds(fixtures, gpu_ok, name):
    """every result (first, last, length, cost) of APPROX k:1:1:1 is in the list under (first, length) with the same last and a
    cost no higher (the reference pays 2 for a change of the last character).  Not the converse: the reference never extends a
    match that has reached a final state and drops nested ranges.  Left out: automaton results whose string holds a code below 5,
    which the definition excludes -- read through the extractor, and no more than 5 % of what is seen"""
    tagged = pattern_set(fixtures(name).docs, name)
    some = [p for t, p in tagged if 8 <= len(p) <= 24 and (p >= OFFSET).all()][:20]
    assert len(some) == 20
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        seen, excluded = 0, 0
        for k in (1, 2):
            start, first, last, cost, length = ix.edit(some, k)
            for q, p in enumerate(some):
                rx = b"".join(b"\\x%02x" % (int(c) - OFFSET) for c in p)
                f, l, m, c = ix.regexp_search(rx, approx=(k, 1, 1, 1))
                s, e = int(start[q]), int(start[q + 1])
                mine = {(int(a), int(n)): (int(b), int(d)) for a, b, n, d in zip(first[s:e], last[s:e], length[s:e], cost[s:e])}
                for a, b, n, d in zip(f, l, m, c):
                    seen += 1
                    hit = mine.get((int(a), int(n)))
                    if hit is None:
                        ctx, _ = ix.context(rows=[int(a)], before=0, after=int(n))
                        assert (ctx[0] < OFFSET).any(), (name, k, q, int(a), int(b), int(n), int(d), ctx[0].tolist())
                        excluded += 1
                        continue
                    assert hit[0] == int(b) and hit[1] <= int(d), (name, k, q, int(a), int(b), int(n), int(d), hit)
        print("automaton results seen %d, left out for a code below 5: %d" % (seen, excluded))
        assert seen >= 20 and excluded * 20 <= seen
        if name == "acgt48k":          # one document, patterns from its interior
            assert excluded == 0
    finally:
        ix.close()


# ---- 7. tiny texts, exhaustively ---------------------------------------------------------------------------------------------------

class Built:
    """an index built here: docs (uint8 arrays), index (its path), text (prepared), pats, per (variants(.., 2) of every pattern)"""

    def __init__(self, tmp_path_factory, name, docs, pats):
        self.name, self.docs, self.pats = name, mu.as_arrays(docs), pats
        self.index = str(tmp_path_factory.mktemp("edit_" + name) / "index")
        femto_amd.build_index(self.index, self.docs, params=None, infos=["%s%d" % (name, i) for i in range(len(self.docs))], device=0)
        self.text = prepared(self.docs)
        self.per = [variants(self.text, p, 2) for p in pats]
        self.want = None

    def answers(self, ix):
        if self.want is None:
            assert ix.info.number_of_documents == len(self.docs) and ix.info.total_length == len(self.text)
            self.want = {k: _answer(ix, self.per, k) for k in (0, 1, 2)}
        return self.want


@pytest.fixture(scope="module", params=["one", "two"])
def tiny(request, tmp_path_factory, gpu_ok):
    return Built(tmp_path_factory, request.param, mu.TINY_TEXTS[request.param], tiny_patterns())


@pytest.mark.parametrize("kind", ["ru", "rum", "pack", "wave"])
def test_tiny_texts(tiny, kind):
    """one and two byte characters in the text (2 nsub + 1 = 3 and 5 edits per site): every string over a, b and a character neither
    text holds, 1 to 4 symbols, bare and with SEOF behind it, and the empty pattern.  Runs, where many scripts reach one string,
    and patterns shorter than k, whose results include the empty string"""
    B = tiny
    ix = open_kind(B.index, kind)
    try:
        want = B.answers(ix)
        for k in (0, 1, 2):
            got = ix.edit(B.pats, k)
            _same(got, want[k], (B.name, kind, k))
        start, first, last, cost, length = want[2]
        assert (length == 0).sum() >= 3 + 9 and ((length == 0) & (last - first + 1 == len(B.text))).sum() == (length == 0).sum()
    finally:
        ix.close()


# ---- 8. capacity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "bytes256"])
def test_capacities(fixtures, gpu_ok, name):
    import torch
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        want = _expected(fixtures, name, ix)
        st = torch.cuda.Stream(device=DEV)
        for k in (1, 2):
            total = len(want[k][1])
            c0 = _device_run(ix, pats, k, 0, st, arrays=False)          # the counting form, with NULL arrays
            raw = int(c0["total"][2])
            assert raw >= total and c0["total"][1] == 1
            short = _device_run(ix, pats, k, raw - 1, st)
            assert short["total"][1:].tolist() == [1, raw]
            full = _device_run(ix, pats, k, raw, st)
            assert full["total"].tolist() == [total, 0, raw]
            _same(_of(full), want[k], (name, k, "capacity = raw"))
            more = _device_run(ix, pats, k, raw + 300, st)          # slots behind the results are not written
            assert more["total"].tolist() == [total, 0, raw]
            _same(_of(more), want[k], (name, k, "capacity = raw + 300"))
            assert all((more[key][total:] == -3).all() for key in ("first", "last", "cost", "length"))
        none = _device_run(ix, [], 1, 0, st)
        assert none["total"].tolist() == [0, 0, 0] and none["start"].tolist() == [0]
        # one pattern of one symbol: the pattern keys are one bit wide
        p = [pats[[len(q) for q in pats].index(1)]]
        one = _answer(ix, [variants(prepared(fixtures(name).docs), p[0], 2)], 2)
        got, raw = _device_answer(ix, p, 2, st)
        _same(got, one, (name, "one pattern"))
        _same(ix.edit(p, 2), one, (name, "one pattern, host"))
        assert one[0].tolist() == [0, len(one[1])] and len(one[1]) > 4 and one[4].min() == 0
    finally:
        ix.close()


def test_device_form_on_its_own_stream_and_bad_arguments(fixtures, gpu_ok):
    import torch
    name = "chunks2doc"
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    try:
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        for k in (0, 1, 2):
            host = ix.edit(pats, k)
            a, _ = _device_answer(ix, pats, k, st)
            b, _ = _device_answer(ix, pats, k, st)
            _same(a, host, (k, "first"))
            _same(b, host, (k, "second"))
        bad = [lambda: ix.edit_device(1, 2, z, z, 3, 0, z, None, None, None, None, z), lambda: ix.edit_device(1, 2, z, z, -1, 0, z, None, None, None, None, z),
               lambda: ix.edit_device(1, 2, None, z, 1, 0, z, None, None, None, None, z), lambda: ix.edit_device(1, 2, z, None, 1, 0, z, None, None, None, None, z),
               lambda: ix.edit_device(1, 2, z, z, 1, 0, z, None, None, None, None, None), lambda: ix.edit_device(1, 2, z, z, 1, 8, z, z, z, z, None, z),
               lambda: ix.edit_device(0, 2, z, z, 1, 0, z, None, None, None, None, z), lambda: ix.edit_device(1, 1 << 31, z, z, 1, 0, z, None, None, None, None, z),
               lambda: ix.edit_device(1 << 31, 2, z, z, 1, 0, z, None, None, None, None, z), lambda: ix.edit_device(1, 2, z, z, 1, 1 << 31, z, z, z, z, z, z),
               lambda: ix.edit([np.full(32769, 70, dtype=np.uint16)], 1), lambda: ix.edit([np.array([70], dtype=np.uint16)], 3)]
        for call in bad:
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 3
        torch.cuda.synchronize()
        assert not z.any()          # nothing was written
    finally:
        ix.close()
    multi = femto_amd.Index(fixtures(name).index, devices=[0, 0])
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            multi.edit_device(1, 2, z, z, 1, 0, z, None, None, None, None, z)
        assert e.value.code == 6 and "multi-device" in str(e.value)
        few = pats[:30]
        single = femto_amd.Index(fixtures(name).index, device=0)
        try:
            _same(multi.edit(few, 2), single.edit(few, 2), ("replica 0",))
        finally:
            single.close()
    finally:
        multi.close()


# ---- 9. what the device form is handed ---------------------------------------------------------------------------------------------

class _Handed:
    pass


@pytest.fixture(scope="module")
def handed(fixtures, gpu_ok):
    """eng2doc's pattern set with one of its patterns of 9 .. 14 symbols in front (pattern 0 has five symbols to lose), each
    pattern's variants alone"""
    fx = fixtures("eng2doc")
    H = _Handed()
    ps = [p for p in _patterns(fixtures, "eng2doc") if len(p) <= 100]          # (the long pattern has its own test)
    q0 = next(q for q, p in enumerate(ps) if 9 <= len(p) <= 14 and (p >= OFFSET).all())
    H.fx, H.text = fx, prepared(fx.docs)
    H.pats = [ps[q0]] + ps[:q0] + ps[q0 + 1:]
    H.per = [variants(H.text, p, 2) for p in H.pats]
    H.nsyms = sum(len(p) for p in H.pats)
    return H


def test_device_form_symbols_the_host_form_refuses(handed):
    """261, 0x7fff and 0xffff at the first, a middle and the last position of cuts that match without them: matched by nothing,
    never substituted or deleted, and the patterns around them keep their results"""
    import torch
    H = handed
    doc = H.fx.docs[0].astype(np.uint16) + OFFSET
    bad = []
    for n, code in enumerate((261, 0x7fff, 0xffff)):
        for m, at in enumerate((0, 9, 19)):
            s = 40 + 50 * (3 * n + m)
            p = doc[s:s + 20].copy()
            assert any(v.cost == 0 for v in variants(H.text, p, 0))
            p[at] = code
            bad.append(p)
    rich = [q for q, vs in enumerate(H.per) if len(vs) > 1]          # the neighbours: 30 patterns with several results, then 10 others
    near = [H.pats[q] for q in rich[:30] + [q for q in range(len(H.pats)) if q not in rich[:30]][:10]]
    near = [near[(7 * i) % 40] for i in range(40)]          # (mixed: 7 and 40 share no factor)
    pats = []
    for i, p in enumerate(bad):
        pats += near[4 * i:4 * i + 4] + [p]
    pats += near[4 * len(bad):]
    per = [variants(H.text, p, 2) if not (p >= 261).any() else [] for p in pats]
    assert sum(len(vs) > 1 for vs in per) > 20
    ix = femto_amd.Index(H.fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        for k in (0, 1, 2):
            want = _answer(ix, per, k)
            _device_answer(ix, H.pats, k, st)          # the full set first: the leased scratch then holds its owners and ranges
            got, _ = _device_answer(ix, pats, k, st)
            _same(got, want, (k,))
            assert all(got[0][5 * i + 4] == got[0][5 * i + 5] for i in range(len(bad)))
            with pytest.raises(femto_amd.FemtoAmdError) as e:          # (the host form refuses what it can: 261 and above)
                ix.edit(pats, k)
            assert e.value.code == 3
    finally:
        ix.close()


def test_device_form_starts_that_leave_the_symbols(handed):
    """d_starts is never read on the host.  One entry at -4 or at nsyms + 9: the two patterns it bounds have no results although the
    scratch still holds their owners and ranges from the call before; d_starts[0] = 5: pattern 0 is what follows its first five
    symbols; nsyms stated 7 above d_starts[npat]: seven symbols nobody owns.  Every other pattern has exactly the results it has
    alone.  A mismatch_device call and a count stand between the calls: they lease the same scratch"""
    import torch
    H = handed
    npat, nsyms = len(H.pats), H.nsyms
    j = next(j for j in range(60, npat - 1) if len(H.per[j - 1]) > 1 and len(H.per[j]) > 1)
    lost = [vs if q not in (j - 1, j) else [] for q, vs in enumerate(H.per)]

    def entry(q, value):
        def edit(starts, flat, n):
            starts[q] = value
            return starts, flat, n
        return edit

    def longer(starts, flat, n):
        return starts, np.concatenate([flat[:n], H.pats[0][:7]]), n + 7

    shorter = [variants(H.text, H.pats[0][5:], 2)] + H.per[1:]
    cases = [("start -4", entry(j, -4), lost), ("start nsyms + 9", entry(j, nsyms + 9), lost), ("starts[0] = 5", entry(0, 5), shorter),
             ("nsyms + 7", longer, H.per)]
    ix = femto_amd.Index(H.fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        for what, edit, per in cases:
            for k in (0, 1, 2):
                want = _answer(ix, per, k)
                _device_answer(ix, H.pats, k, st)
                ix.mismatch(H.pats[:50], 2)
                f, l = ix.count(H.pats)
                assert (f <= l).any()
                got, _ = _device_answer(ix, H.pats, k, st, edit=edit)
                _same(got, want, (what, k))
    finally:
        ix.close()


# ---- 10. one long pattern ----------------------------------------------------------------------------------------------------------

def test_one_long_pattern(tmp_path_factory, gpu_ok):
    """4097 symbols cut from a random document, with one deletion and one insertion planted, beside the same cut untouched and
    short patterns: the lanes of its sites walk up to 4097 exact steps, and under k = 2 try every second edit on the way"""
    rng = np.random.default_rng(4097)
    doc = rng.integers(0, 4, size=20000).astype(np.uint8) + ord("A")
    cut = doc[5000:5000 + 4097].astype(np.uint16) + OFFSET
    planted = np.insert(np.delete(cut, 1000), 3000, ord("C") + OFFSET)
    assert len(planted) == 4097 and not np.array_equal(planted, cut)
    short = [doc[s:s + n].astype(np.uint16) + OFFSET for s, n in ((10, 8), (300, 12), (7000, 5), (15000, 20))]
    B = Built(tmp_path_factory, "long", [doc, doc[:50]], [short[0], planted, short[1], cut, short[2], short[3]])
    assert any(v.cost == 2 and len(v.symbols) == 4097 for v in B.per[1]) and any(v.cost == 0 for v in B.per[3])
    ix = femto_amd.Index(B.index, device=0)
    try:
        want = B.answers(ix)
        for k in (1, 2):
            _same(ix.edit(B.pats, k), want[k], ("long", k))
        start = want[2][0]
        assert start[2] - start[1] >= 1 and start[4] - start[3] >= 1
    finally:
        ix.close()
