"""`-m gpu`: search with substitutions (include/femto_amd.h "search with substitutions") against the yardstick of
tests/mismatch_util.py, which tests/test_mismatch_host.py pins to the CPU oracle: every fixture under every rank policy that
applies to it, k = 0, 1, 2, the capacities, the device form on a stream of its own, the automaton route on the same handle."""
import numpy as np
import pytest

import femto_amd
from mismatch_util import expected, pattern_set, prepared, variants
from oracle import pyoracle
from regexp_util import KINDS, open_kind, text_chars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# characters of the fixtures' texts, SEOF included (checked against the documents below): what decides the policies that apply
NCHARS = {"acgt48k": 5, "b1000": 7, "bytes256": 257, "eng2doc": 94, "chunks2doc": 11, "runs3doc": 5, "counter400_small": 7, "construct_kat": 11}
FIXTURES = list(NCHARS)
CASES = [(name, kind) for name in FIXTURES for kind, v in KINDS.items() if v.applies(NCHARS[name])]
_want = {}


def _patterns(fixtures, name):
    return [p for _, p in pattern_set(fixtures(name).docs, name)]


def _expected(fixtures, name, ix):
    """{k: (result_start, first, last, cost, sub_pos, sub_sym)} for the fixture's pattern set, computed once: the variants and
    their order from the yardstick, their rows from ix.count on each variant -- and, where the CPU oracle is quick, from it too"""
    if name not in _want:
        fx = fixtures(name)
        assert len(text_chars(fx.docs)) == NCHARS[name]
        text = prepared(fx.docs)
        per = [variants(text, p, 2) for p in _patterns(fixtures, name)]
        _want[name] = {}
        for k in (0, 1, 2):
            start, flat, cost, pos, sym = expected(per, k)
            first, last = ix.count([v.symbols for v in flat])
            assert np.array_equal(last - first + 1, np.array([v.rows for v in flat], dtype=np.int64))
            if name in ("acgt48k", "eng2doc"):
                o = pyoracle.Oracle(fx.index)
                try:
                    f, l = o.count([v.symbols for v in flat])
                finally:
                    o.close()
                assert np.array_equal(f, first) and np.array_equal(l, last)
            for q in range(len(per)):
                assert (np.diff(first[start[q]:start[q + 1]]) > 0).all()
            _want[name][k] = (start, first, last, cost, pos, sym)
    return _want[name]


def _same(got, want, what):
    for g, w, field in zip(got, want, ("result_start", "first", "last", "cost", "sub_pos", "sub_sym")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what + (field, np.nonzero(g != w)[0][:8] if g.shape == w.shape else g.shape)


# ---- 1. the yardstick, bit for bit ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", CASES)
def test_equals_the_yardstick(fixtures, gpu_ok, name, kind):
    fx = fixtures(name)
    pats = _patterns(fixtures, name)
    ix = open_kind(fx.index, kind)
    try:
        want = _expected(fixtures, name, ix)
        for mode in [ix.rank_mode] + ([0] if kind == "wave" else []):      # mode 0 with the derived lines: the same lane policy
            ix.set_rank_mode(mode)
            for k in ((0, 1, 2) if mode else (1,)):
                got = ix.mismatch(pats, k)
                _same(got, want[k], (name, kind, mode, k))
                pos = got[4]
                assert ((pos[:, 1] == -1) | (pos[:, 0] < pos[:, 1])).all() and ((pos[:, 0] >= 0) | (pos[:, 1] == -1)).all()
                assert np.array_equal((pos >= 0).sum(axis=1), got[3]) and (got[5][pos < 0] == 0).all()
        assert int((want[2][3] == 2).sum()) > 0 and int((want[1][3] == 1).sum()) > 0
    finally:
        ix.close()


# ---- 2. k = 0 is count ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_k0_is_count(fixtures, gpu_ok, name):
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        first, last = ix.count(pats)
        start, f, l, cost, pos, sym = ix.mismatch(pats, 0)
        occurs = first <= last
        assert np.array_equal(np.diff(start), occurs.astype(np.int64)) and occurs.any() and not occurs.all()
        assert np.array_equal(f, first[occurs]) and np.array_equal(l, last[occurs]) and not cost.any() and (pos == -1).all() and not sym.any()
        empty = [i for i, p in enumerate(pats) if len(p) == 0]
        assert empty and all(first[i] == 0 and last[i] == ix.info.total_length - 1 for i in empty)
    finally:
        ix.close()


# ---- 3, 4. the device form --------------------------------------------------------------------------------------------------------

def _device_run(ix, pats, k, capacity, stream, arrays=True, edit=None):
    """femto_amd_mismatch_device on `stream`, chained after the upload on that stream with no synchronisation in between.
    edit(starts, flat, nsyms) -> (starts, flat, nsyms): what the call is handed in place of the well-formed inputs"""
    import torch
    plen, flat, starts = femto_amd.flatten(pats)
    nsyms = int(plen.sum())
    starts = np.concatenate([starts, [nsyms]]).astype(np.int64)
    if edit is not None:
        starts, flat, nsyms = edit(starts.copy(), flat.copy(), nsyms)
    with torch.cuda.stream(stream):
        d_syms = torch.from_numpy(flat.view(np.int16)).to(DEV, non_blocking=True)
        d_starts = torch.from_numpy(starts).to(DEV, non_blocking=True)
        cap = max(capacity, 1)
        o = dict(start=torch.full((len(pats) + 1,), -3, dtype=torch.int64, device=DEV), first=torch.full((cap,), -3, dtype=torch.int64, device=DEV),
                 last=torch.full((cap,), -3, dtype=torch.int64, device=DEV), cost=torch.full((cap,), -3, dtype=torch.int32, device=DEV),
                 pos=torch.full((cap, 2), -3, dtype=torch.int32, device=DEV), sym=torch.full((cap, 2), 7, dtype=torch.int16, device=DEV),
                 total=torch.full((2,), -3, dtype=torch.int64, device=DEV))
        a = (o["first"], o["last"], o["cost"], o["pos"], o["sym"]) if arrays else (None,) * 5
        ix.mismatch_device(len(pats), nsyms, d_syms, d_starts, k, capacity, o["start"], *a, o["total"], stream=stream.cuda_stream)
    stream.synchronize()
    r = {key: v.cpu().numpy() for key, v in o.items()}
    r["sym"] = r["sym"].view(np.uint16)
    return r


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "bytes256"])
def test_capacities(fixtures, gpu_ok, name):
    import torch
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        want = _expected(fixtures, name, ix)
        st = torch.cuda.Stream(device=DEV)
        for k in (1, 2):
            start, first, last, cost, pos, sym = want[k]
            total = len(first)
            c0 = _device_run(ix, pats, k, 0, st, arrays=False)
            assert c0["total"].tolist() == [total, 1] and np.array_equal(c0["start"], start)
            short = _device_run(ix, pats, k, total - 1, st)
            assert short["total"].tolist() == [total, 1] and np.array_equal(short["start"], start)
            full = _device_run(ix, pats, k, total, st)
            assert full["total"].tolist() == [total, 0]
            _same((full["start"], full["first"], full["last"], full["cost"], full["pos"], full["sym"]), want[k], (name, k, "capacity = total"))
            more = _device_run(ix, pats, k, total + 300, st)          # slots behind the results are not written
            assert more["total"].tolist() == [total, 0] and np.array_equal(more["first"][:total], first) and (more["first"][total:] == -3).all()
            assert (more["pos"][total:] == -3).all() and (more["sym"][total:] == 7).all() and np.array_equal(more["pos"][:total], pos)
        none = _device_run(ix, [], 1, 0, st, arrays=False)
        assert none["total"].tolist() == [0, 0] and none["start"].tolist() == [0]
    finally:
        ix.close()


@pytest.mark.parametrize("kw", [None, dict(text=0, dense_arrays=0), dict(rank_mode=1)])
def test_device_form_on_its_own_stream_equals_the_host_form(fixtures, gpu_ok, kw):
    import torch
    name = "chunks2doc"
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0, options=kw) if kw else femto_amd.Index(fixtures(name).index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        for k in (0, 1, 2):
            host = ix.mismatch(pats, k)
            total = len(host[1])
            a = _device_run(ix, pats, k, total, st)
            b = _device_run(ix, pats, k, total, st)
            for r in (a, b):
                _same((r["start"], r["first"], r["last"], r["cost"], r["pos"], r["sym"]), host, (kw, k))
            assert a["total"].tolist() == b["total"].tolist() == [total, 0]
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "bytes256"])
def test_substitution_pass_in_several_launches(fixtures, gpu_ok, monkeypatch, name):
    """a launch carries fewer than 2^32 lanes and a batch may need 2^39: the pass goes out in launches of whole workgroups, each
    told its first lane.  FEMTO_AMD_MISMATCH_CHUNK (lanes per launch) makes that happen at these sizes: five launches or so, cut
    inside a position's substitutes wherever 256 is no multiple of their number (93 on eng2doc), and one workgroup per launch."""
    pats = _patterns(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        want = _expected(fixtures, name, ix)
        nsub = NCHARS[name] - 1
        lanes = sum(len(p) for p in pats) * nsub
        for k in (1, 2):
            monkeypatch.setenv("FEMTO_AMD_MISMATCH_CHUNK", str(lanes // 5))
            _same(ix.mismatch(pats, k), want[k], (name, k, lanes // 5))
        few = [p for p in pats if len(p) <= 24][:12]
        monkeypatch.delenv("FEMTO_AMD_MISMATCH_CHUNK")
        whole = ix.mismatch(few, 2)
        assert len(whole[1]) > len(few)
        monkeypatch.setenv("FEMTO_AMD_MISMATCH_CHUNK", "1")         # below a workgroup: one workgroup per launch
        _same(ix.mismatch(few, 2), whole, (name, 2, 256))
    finally:
        ix.close()


def test_device_form_gives_a_pattern_past_the_limit_no_results(fixtures, gpu_ok):
    """the device form never reads d_starts on the host: a pattern of 32769 symbols -- a cut of acgt48k's one document, which
    would match whole -- has no results, and the patterns around it have theirs.  The positions it covers held other patterns'
    ranges and owners in the call before."""
    import torch
    name = "acgt48k"
    fx = fixtures(name)
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    assert len(doc) > 32769
    long = doc[100:100 + 32769].astype(np.uint16) + 5
    pats = _patterns(fixtures, name)[:60]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        assert ix.mismatch([long[:32768]], 0)[0].tolist() == [0, 1]          # at the limit it is searched, and found
        st = torch.cuda.Stream(device=DEV)
        for k in (0, 1, 2):
            start, f, l, cost, pos, sym = ix.mismatch(pats, k)
            start = np.append(np.insert(start, 7, start[7]), start[-1])
            total = len(f)
            r = _device_run(ix, pats[:7] + [long] + pats[7:] + [long], k, total + 4, st)
            assert r["total"].tolist() == [total, 0]
            _same((r["start"], r["first"][:total], r["last"][:total], r["cost"][:total], r["pos"][:total], r["sym"][:total]),
                  (start, f, l, cost, pos, sym), (k,))
            assert (r["first"][total:] == -3).all()
    finally:
        ix.close()


# ---- 5. the automaton route on the same handle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_contains_what_the_automaton_route_finds(fixtures, gpu_ok, name):
    """every result of APPROX k:1:k+1:k+1 (substitutions only) is in the list, with its rows and cost.  Not the converse: the
    reference never substitutes the last character (QUERY_FORMAT.txt:143)"""
    tagged = pattern_set(fixtures(name).docs, name)
    some = [p for t, p in tagged if t.startswith(("planted", "cut", "len20", "lacks")) and 8 <= len(p) <= 24][:20]
    assert len(some) == 20
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        seen = 0
        for k in (1, 2):
            start, first, last, cost, pos, sym = ix.mismatch(some, k)
            for q, p in enumerate(some):
                rx = b"".join(b"\\x%02x" % (int(c) - 5) for c in p)
                f, l, m, c = ix.regexp_search(rx, approx=(k, 1, k + 1, k + 1))
                mine = {(int(a), int(b)): int(d) for a, b, d in zip(first[start[q]:start[q + 1]], last[start[q]:start[q + 1]], cost[start[q]:start[q + 1]])}
                for a, b, n, d in zip(f, l, m, c):
                    assert n == len(p) and mine.get((int(a), int(b))) == int(d), (name, k, q, int(a), int(b), int(d))
                seen += len(f)
        assert seen > 20
    finally:
        ix.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused(fixtures, gpu_ok):
    import torch
    fx = fixtures("eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    try:
        bad = [lambda: ix.mismatch_device(1, 2, z, z, 3, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, z, z, -1, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, None, z, 1, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, z, None, 1, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, z, z, 1, 0, None, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, z, z, 1, 0, z, None, None, None, None, None, None),
               lambda: ix.mismatch_device(1, 2, z, z, 1, 8, z, z, z, z, z, None, z),
               lambda: ix.mismatch_device(0, 2, z, z, 1, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 1 << 31, z, z, 1, 0, z, None, None, None, None, None, z),         # the bounds the header states
               lambda: ix.mismatch_device(1 << 31, 2, z, z, 1, 0, z, None, None, None, None, None, z),
               lambda: ix.mismatch_device(1, 2, z, z, 1, 1 << 31, z, z, z, z, z, z, z),
               lambda: ix.mismatch([np.full(32769, 70, dtype=np.uint16)], 1), lambda: ix.mismatch([np.array([70], dtype=np.uint16)], 3),
               lambda: ix.mismatch([np.array([70], dtype=np.uint16)], -1)]
        for call in bad:
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 3
        torch.cuda.synchronize()
        assert not z.any()          # nothing was written
    finally:
        ix.close()
    multi = femto_amd.Index(fx.index, devices=[0, 0])
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            multi.mismatch_device(1, 2, z, z, 1, 0, z, None, None, None, None, None, z)
        assert e.value.code == 6 and "multi-device" in str(e.value)
    finally:
        multi.close()
    a = femto_amd.Index(fx.index, device=0, part=0, nparts=2)
    b = femto_amd.Index(fx.index, device=0, part=1, nparts=2)
    try:
        a.split_attach_local(b)
        b.split_attach_local(a)
        a.split_commit()
        b.split_commit()
        for call in (lambda: a.mismatch_device(1, 2, z, z, 1, 0, z, None, None, None, None, None, z), lambda: a.mismatch([np.array([70, 71], dtype=np.uint16)], 1)):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 6 and "range-split part" in str(e.value)
    finally:
        a.close()
        b.close()
