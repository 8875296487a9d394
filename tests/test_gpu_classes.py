"""`-m gpu`: search with character classes (include/femto_amd.h "search with character classes", femto_amd/classes/classes.hip)
against the committed reference results and against the yardstick of tests/classes_util.py, which tests/test_classes_host.py pins to
both: the five fixtures under every rank policy that applies to them and the lane fallback, the capacities, the device form on a
stream of its own with a growing scratch, malformed input to the device form, the automaton route on the same handle, refusals."""
import numpy as np
import pytest

import femto_amd
from classes_util import CLASS, GOLDEN, OFFSET, automaton_may_differ, expected, golden_case, members_of, pattern_set, regex_of, strings
from mismatch_util import prepared
from regexp_util import KINDS, open_kind, text_chars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# characters of the fixtures' texts, SEOF included (checked against the documents below): what decides the policies that apply
NCHARS = {"acgt48k": 5, "eng2doc": 94, "bytes256": 257, "runs3doc": 5, "chunks2doc": 11}
FIXTURES = list(NCHARS)
CASES = [(name, kind) for name in FIXTURES for kind, v in KINDS.items() if v.applies(NCHARS[name])]
_want = {}


def _set(fixtures, name):
    tagged, cls = pattern_set(fixtures(name).docs, name)
    return [p for _, p in tagged], cls


def _expected(fixtures, name, ix):
    """(result_start, first, last) for the fixture's pattern set, computed once: the strings and their order from the yardstick,
    their rows from ix.count (femto_amd_count_device's host form) on each string"""
    if name not in _want:
        fx = fixtures(name)
        assert len(text_chars(fx.docs)) == NCHARS[name]
        pats, cls = _set(fixtures, name)
        text = prepared(fx.docs)
        per = [strings(text, p, cls) for p in pats]
        start, flat = expected(per)
        first, last = ix.count([f.symbols for f in flat])
        assert np.array_equal(last - first + 1, np.array([f.rows for f in flat], dtype=np.int64))
        for q in range(len(per)):
            assert (np.diff(first[start[q]:start[q + 1]]) > 0).all()
        _want[name] = (start, first, last)
    return _want[name]


def _same(got, want, what):
    for g, w, field in zip(got, want, ("result_start", "first", "last")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what + (field, np.nonzero(g != w)[0][:8] if g.shape == w.shape else g.shape)


def _device_run(ix, pats, cls, capacity, stream, arrays=True, edit=None, nclasses=None):
    """femto_amd_classes_device on `stream`, chained after the upload on that stream with no synchronisation in between.
    edit(starts, flat, nsyms) -> (starts, flat, nsyms): what the call is handed in place of the well-formed inputs"""
    import torch
    plen, flat, starts = femto_amd.flatten(pats)
    nsyms = int(plen.sum())
    starts = np.concatenate([starts, [nsyms]]).astype(np.int64)
    if edit is not None:
        starts, flat, nsyms = edit(starts.copy(), flat.copy(), nsyms)
    table = np.ascontiguousarray(cls, dtype=np.uint64).reshape(-1, 4)
    with torch.cuda.stream(stream):
        d_syms = torch.from_numpy(flat.view(np.int16)).to(DEV, non_blocking=True)
        d_starts = torch.from_numpy(starts).to(DEV, non_blocking=True)
        d_cls = torch.from_numpy(np.concatenate([table, np.zeros((1, 4), dtype=np.uint64)]).view(np.int64)).to(DEV, non_blocking=True)
        cap = max(capacity, 1)
        o = dict(start=torch.full((len(pats) + 1,), -3, dtype=torch.int64, device=DEV), first=torch.full((cap,), -3, dtype=torch.int64, device=DEV),
                 last=torch.full((cap,), -3, dtype=torch.int64, device=DEV), total=torch.full((2,), -3, dtype=torch.int64, device=DEV))
        a = (o["first"], o["last"]) if arrays else (None, None)
        ix.classes_device(len(pats), nsyms, d_syms, d_starts, len(table) if nclasses is None else nclasses, d_cls, capacity, o["start"], *a,
                          o["total"], stream=stream.cuda_stream)
    stream.synchronize()
    return {key: v.cpu().numpy() for key, v in o.items()}


# ---- 1. the reference's result lists ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted({g[0] for g in GOLDEN}))
def test_parity_with_the_reference(fixtures, gpu_ok, name):
    import torch
    mine = [(rx, n) for fx, rx, n in GOLDEN if fx == name]
    pats, cls = femto_amd.class_patterns([rx for rx, _ in mine])
    want = [golden_case(name, rx) for rx, _ in mine]
    start = np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).astype(np.int64)
    first, last = np.concatenate([w[0] for w in want]).astype(np.int64), np.concatenate([w[1] for w in want]).astype(np.int64)
    assert [len(w[0]) for w in want] == [n for _, n in mine]
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        r = _device_run(ix, pats, cls, len(first), torch.cuda.Stream(device=DEV))
        assert r["total"].tolist() == [len(first), 0]
        _same((r["start"], r["first"], r["last"]), (start, first, last), (name, "device form"))
        _same(ix.classes(pats, cls), (start, first, last), (name, "host form"))
    finally:
        ix.close()


# ---- 2. the yardstick, bit for bit, under every rank policy ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", CASES)
def test_equals_the_yardstick(fixtures, gpu_ok, name, kind):
    pats, cls = _set(fixtures, name)
    ix = open_kind(fixtures(name).index, kind)
    try:
        want = _expected(fixtures, name, ix)
        _same(ix.classes(pats, cls), want, (name, kind, ix.rank_mode))
        assert int(np.diff(want[0]).max()) > 1 and len(want[1]) > len(pats)
        if kind == "wave":      # mode 0 with the derived lines: the same lane policy.  Without the two periods: on a byte text their
            ix.set_rank_mode(0)          # lane takes 65 792 steps through femto's wavelet tree, seconds that mode 1 has spent already
            start, first, last = want
            keep = [q for q, (tag, _) in enumerate(pattern_set(fixtures(name).docs, name)[0]) if tag != "period2"]
            sub = (np.concatenate([[0], np.cumsum([start[q + 1] - start[q] for q in keep])]).astype(np.int64),
                   np.concatenate([first[start[q]:start[q + 1]] for q in keep]), np.concatenate([last[start[q]:start[q + 1]] for q in keep]))
            _same(ix.classes([pats[q] for q in keep], cls), sub, (name, kind, 0))
    finally:
        ix.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_literal_patterns_are_count(fixtures, gpu_ok, name):
    tagged, cls = pattern_set(fixtures(name).docs, name)
    pats = [p for t, p in tagged if not (p & CLASS).any()]
    assert len(pats) >= 8 and any(len(p) == 0 for p in pats)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        first, last = ix.count(pats)
        start, f, l = ix.classes(pats, np.zeros((0, 4), dtype=np.uint64))
        occurs = first <= last
        assert np.array_equal(np.diff(start), occurs.astype(np.int64)) and occurs.any() and not occurs.all()
        assert np.array_equal(f, first[occurs]) and np.array_equal(l, last[occurs])
        empty = [i for i, p in enumerate(pats) if len(p) == 0]
        assert all(first[i] == 0 and last[i] == ix.info.total_length - 1 for i in empty)
    finally:
        ix.close()


# ---- 3. the automaton route on the same handle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_automaton_route_gives_the_same_lists(fixtures, gpu_ok, name):
    """regexp_search_batch on the same handle, for the first 64 patterns of the set that have a text in the query language: the same
    lists -- but for the patterns where classes_util.automaton_may_differ shows, from the text alone, that do_regexp_query merges
    two of its entries by range and so never reaches some strings: there its list is a sub-list of this call's, in order."""
    fx = fixtures(name)
    tagged, cls = pattern_set(fx.docs, name)
    some = [p for t, p in tagged if 0 < len(p) <= 40 and (p & CLASS).any() and (p >= OFFSET).all() and regex_of(p, cls) is not None]
    # (at most 10 000 combinations of members: bytes256's two periods are 65 536, seconds of one lane on femto's wavelet tree that
    # test_equals_the_yardstick spends once; eng2doc's two periods, the case where the routes differ, stay)
    some = [p for p in some if np.prod([len(members_of(cls[int(s) & ~CLASS])) for s in p if s & CLASS], dtype=np.float64) <= 10000][:64]
    assert len(some) >= 40
    text = prepared(fx.docs)
    merges = [automaton_may_differ(text, p, cls) for p in some]
    assert sum(merges) < len(some) // 2, (name, sum(merges))
    ix = femto_amd.Index(fx.index, device=0)
    try:
        start, first, last = ix.classes(some, cls)
        rs, rf, rl, rlen, rcost, status = ix.regexp_search_batch([regex_of(p, cls) for p in some])
        assert not status.any() and not rcost.any() and len(first) > len(some)
        for q, p in enumerate(some):
            mine = list(zip(first[start[q]:start[q + 1]].tolist(), last[start[q]:start[q + 1]].tolist()))
            theirs = list(zip(rf[rs[q]:rs[q + 1]].tolist(), rl[rs[q]:rs[q + 1]].tolist()))
            if merges[q]:
                assert set(theirs) <= set(mine) and theirs == sorted(theirs), (name, q, len(theirs), len(mine))
            else:
                assert theirs == mine and (rlen[rs[q]:rs[q + 1]] == len(p)).all(), (name, q, len(theirs), len(mine))
    finally:
        ix.close()


# ---- 4. capacities, streams, a growing scratch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "chunks2doc"])
def test_capacities(fixtures, gpu_ok, name):
    import torch
    pats, cls = _set(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        start, first, last = _expected(fixtures, name, ix)
        total = len(first)
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        c0 = _device_run(ix, pats, cls, 0, st, arrays=False)
        assert c0["total"].tolist() == [total, 1] and np.array_equal(c0["start"], start)
        short = _device_run(ix, pats, cls, total - 1, st)
        assert short["total"].tolist() == [total, 1] and np.array_equal(short["start"], start)
        full = _device_run(ix, pats, cls, total, st)
        assert full["total"].tolist() == [total, 0]
        _same((full["start"], full["first"], full["last"]), (start, first, last), (name, "capacity = total"))
        more = _device_run(ix, pats, cls, total + 300, st)          # slots behind the results are not written
        assert more["total"].tolist() == [total, 0] and np.array_equal(more["first"][:total], first) and (more["first"][total:] == -3).all()
        assert np.array_equal(more["last"][:total], last) and (more["last"][total:] == -3).all()
        none = _device_run(ix, [], cls, 0, st, arrays=False)
        assert none["total"].tolist() == [0, 0] and none["start"].tolist() == [0]
    finally:
        ix.close()


@pytest.mark.parametrize("kw", [None, dict(text=0, dense_arrays=0), dict(rank_mode=1)])
def test_scratch_grows_between_calls_on_a_stream_of_their_own(fixtures, gpu_ok, kw):
    import torch
    name = "chunks2doc"
    pats, cls = _set(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0, options=kw) if kw else femto_amd.Index(fixtures(name).index, device=0)
    try:
        start, first, last = _expected(fixtures, name, ix)
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        few = 12          # the first call sizes the scratch for 12 patterns, the second needs it for 200 and their 300-deep stack
        a = _device_run(ix, pats[:few], cls, int(start[few]), st)
        assert a["total"].tolist() == [int(start[few]), 0]
        _same((a["start"], a["first"], a["last"]), (start[:few + 1], first[:start[few]], last[:start[few]]), (kw, "small"))
        for _ in range(2):
            b = _device_run(ix, pats, cls, len(first), st)
            assert b["total"].tolist() == [len(first), 0]
            _same((b["start"], b["first"], b["last"]), (start, first, last), (kw, "large"))
    finally:
        ix.close()


# ---- 5. what the device form is handed ------------------------------------------------------------------------------------------------

def test_malformed_patterns_have_no_results_and_their_neighbours_keep_theirs(fixtures, gpu_ok):
    """the device form never reads d_starts or d_syms on the host.  Every case spoils ONE pattern q of a batch whose other patterns
    are left as they are: the spoilt one has no results, every other pattern has the results it has alone."""
    import torch
    name = "acgt48k"
    fx = fixtures(name)
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    assert len(doc) > 32769
    pats, cls = _set(fixtures, name)
    pats = pats[:60]
    long = doc[100:100 + 32769].astype(np.uint16) + OFFSET
    ix = femto_amd.Index(fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        start, first, last = ix.classes(pats, cls)
        per = [(first[start[q]:start[q + 1]], last[start[q]:start[q + 1]]) for q in range(len(pats))]
        assert ix.classes([long[:32768]], cls)[0].tolist() == [0, 1]          # at the limit it is searched, and found

        def check(batch, spoilt, what, edit=None, nclasses=None, keep=None):
            keep = per if keep is None else keep
            want_n = [0 if q in spoilt else len(keep[q][0]) for q in range(len(batch))]
            ws = np.concatenate([[0], np.cumsum(want_n)]).astype(np.int64)
            total = int(ws[-1])
            r = _device_run(ix, batch, cls, total + 5, st, edit=edit, nclasses=nclasses)
            assert r["total"].tolist() == [total, 0], what
            wf = np.concatenate([keep[q][0] for q in range(len(batch)) if q not in spoilt])
            wl = np.concatenate([keep[q][1] for q in range(len(batch)) if q not in spoilt])
            _same((r["start"], r["first"][:total], r["last"][:total]), (ws, wf, wl), (what,))
            assert (r["first"][total:] == -3).all() and (r["last"][total:] == -3).all(), what

        q = 9          # "every1", one class position: patterns with results on either side
        assert len(per[q][0]) and len(per[q - 1][0]) and len(per[q + 1][0]) and len(pats[q]) > 0

        def below(starts, flat, nsyms):          # d_starts[0] < 0: pattern 0 leaves the symbols
            starts[0] = -4
            return starts, flat, nsyms
        check(pats, {0}, "a start below 0", edit=below)

        def above(starts, flat, nsyms):          # the last entry above nsyms: the last pattern leaves the symbols
            starts[-1] = nsyms + 3
            return starts, flat, nsyms
        check(pats, {len(pats) - 1}, "a start above nsyms", edit=above)

        # a descending pair where it leaves no two well-formed patterns sharing symbols (overlap is not supported): at either end
        def descending_last(starts, flat, nsyms):          # the last pattern has a negative length; nsyms stays what it is
            starts[-1] = starts[-2] - 3
            return starts, flat, nsyms
        assert len(per[len(pats) - 1][0])
        check(pats, {len(pats) - 1}, "a descending pair at the end", edit=descending_last)

        def descending_first(starts, flat, nsyms):          # the first pattern has a negative length
            starts[0] = starts[1] + 2
            return starts, flat, nsyms
        check([pats[q]] + pats[1:], {0}, "a descending pair in front", edit=descending_first, keep=[per[q]] + per[1:])

        def no_such_class(starts, flat, nsyms):
            at = int(starts[q]) + int(np.nonzero(flat[starts[q]:starts[q + 1]] & CLASS)[0][0])
            flat[at] = CLASS | len(cls)
            return starts, flat, nsyms
        assert (pats[q] & CLASS).any()
        check(pats, {q}, "a class number equal to nclasses", edit=no_such_class)

        def not_a_code(starts, flat, nsyms):
            flat[starts[q]] = 261
            return starts, flat, nsyms
        check(pats, {q}, "a symbol 261", edit=not_a_code)

        batch = pats[:7] + [long] + pats[7:] + [long]
        keep7 = per[:7] + [None] + per[7:] + [None]
        check(batch, {7, len(batch) - 1}, "a pattern of 32769 symbols", keep=keep7)
    finally:
        ix.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused(fixtures, gpu_ok):
    import torch
    fx = fixtures("eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    one = np.zeros((1, 4), dtype=np.uint64)
    try:
        bad = [lambda: ix.classes_device(1, 2, None, z, 1, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 2, z, None, 1, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 2, z, z, 1, z, 0, None, None, None, z),
               lambda: ix.classes_device(1, 2, z, z, 1, z, 0, z, None, None, None),
               lambda: ix.classes_device(1, 2, z, z, 1, z, 8, z, z, None, z),
               lambda: ix.classes_device(0, 2, z, z, 1, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 1 << 31, z, z, 1, z, 0, z, None, None, z),         # the bounds the header states
               lambda: ix.classes_device(1 << 31, 2, z, z, 1, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 2, z, z, 1, z, 1 << 31, z, z, z, z),
               lambda: ix.classes_device(1, 2, z, z, 4097, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 2, z, z, -1, z, 0, z, None, None, z),
               lambda: ix.classes_device(1, 2, z, z, 1, None, 0, z, None, None, z),            # a NULL class table with nclasses > 0
               lambda: ix.classes([np.full(32769, 70, dtype=np.uint16)], one),
               lambda: ix.classes([np.array([70, CLASS], dtype=np.uint16)], np.zeros((0, 4), dtype=np.uint64)),      # the class flag when nclasses = 0
               lambda: ix.classes([np.array([70, CLASS | 1], dtype=np.uint16)], one),
               lambda: ix.classes([np.array([70, 261], dtype=np.uint16)], one),
               lambda: ix.classes([np.array([70], dtype=np.uint16)], np.zeros((4097, 4), dtype=np.uint64))]
        for i, call in enumerate(bad):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 3, i
        torch.cuda.synchronize()
        assert not z.any()          # nothing was written
    finally:
        ix.close()
    multi = femto_amd.Index(fx.index, devices=[0, 0])
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            multi.classes_device(1, 2, z, z, 1, z, 0, z, None, None, z)
        assert e.value.code == 6 and "multi-device" in str(e.value)
        pats, cls = femto_amd.class_patterns([b"q."])          # the host form runs on replica 0
        assert multi.classes(pats, cls)[0].tolist() == [0, 10]
    finally:
        multi.close()
    a = femto_amd.Index(fx.index, device=0, part=0, nparts=2)
    b = femto_amd.Index(fx.index, device=0, part=1, nparts=2)
    try:
        a.split_attach_local(b)
        b.split_attach_local(a)
        a.split_commit()
        b.split_commit()
        for call in (lambda: a.classes_device(1, 2, z, z, 1, z, 0, z, None, None, z), lambda: a.classes([np.array([70, CLASS], dtype=np.uint16)], one)):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 6 and "range-split part" in str(e.value)
    finally:
        a.close()
        b.close()
