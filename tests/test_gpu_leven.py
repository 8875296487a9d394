"""`-m gpu`: occurrences within k edits by exact seeds (include/femto_amd.h) against the yardstick of tests/leven_util.py, which
tests/test_leven_host.py pins to a double loop over the definition, to tests/hamming_util.py and to tests/edit_util.py: every
fixture under every rank policy that applies to it, k = 0, 1, 2, 3, 5, the candidate count, the three relations the header states
(k = 0 and locate, containment of femto_amd_hamming, femto_amd_edit + locate for k <= 2), the sample path, the device form on a
stream of its own with its capacities, what the device form is handed, the refusals, batches of more than one workgroup and more
than one grid of candidates, and a batch of 256 with slots behind its results."""
import numpy as np
import pytest

import femto_amd
from leven_util import KS, OFFSET, expected, occurrences, pattern_set, pieces, prepared
from regexp_util import KINDS, open_kind, text_chars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NCHARS = {"acgt48k": 5, "b1000": 7, "bytes256": 257, "eng2doc": 94, "chunks2doc": 11, "runs3doc": 5, "counter400_small": 7, "construct_kat": 11}
FIXTURES = list(NCHARS)
CASES = [(name, kind) for name in FIXTURES for kind, v in KINDS.items() if v.applies(NCHARS[name])]
HOLDS_TEXT = ("ru", "pack", "ind", "pack2")          # the kinds whose handle keeps the text: their extractor extends against it
FIELDS = ("result_start", "offset", "cost", "length")
_want = {}


def _tagged(fixtures, name, k):
    return pattern_set(fixtures(name).docs, name, k)


def _patterns(fixtures, name, k):
    return [p for _, p in _tagged(fixtures, name, k)]


def _expected(fixtures, name, k):
    """(result_start, offset, cost, length) of the fixture's pattern set for k, computed once"""
    if (name, k) not in _want:
        fx = fixtures(name)
        assert len(text_chars(fx.docs)) == NCHARS[name]
        _want[name, k] = expected(prepared(fx.docs), _patterns(fixtures, name, k), k)
    return _want[name, k]


def _piece_candidates(ix, pats, k):
    """the sum of ix.count over the pieces of every pattern"""
    cut = [p[b0:b1] for p in pats for b0, b1 in pieces(len(p), k)]
    if not cut:
        return 0
    first, last = ix.count(cut)
    return int(np.maximum(last - first + 1, 0).sum())


def _same(got, want, what):
    for g, w, field in zip(got, want, FIELDS):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what + (field, np.nonzero(g != w)[0][:8] if g.shape == w.shape else g.shape)


# ---- 1. the yardstick, bit for bit, and the candidates --------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", CASES)
def test_equals_the_yardstick(fixtures, gpu_ok, name, kind):
    ix = open_kind(fixtures(name).index, kind)
    try:
        path = ix.extractor().info()["path"]          # (a "wave" handle keeps the text where the packed layouts exist beside it)
        assert path == femto_amd.Extractor.PATH_TEXT if kind in HOLDS_TEXT else kind == "wave" or path == femto_amd.Extractor.PATH_SAMPLES
        assert name != "bytes256" or path == femto_amd.Extractor.PATH_SAMPLES
        results = 0
        for k in KS:
            tagged = _tagged(fixtures, name, k)
            pats = [p for _, p in tagged]
            want = _expected(fixtures, name, k)
            start, off, cost, length, cands, raw = ix.leven(pats, k)
            _same((start, off, cost, length), want, (name, kind, k))
            assert cands == _piece_candidates(ix, pats, k) and raw >= len(off)
            for q, (tag, _) in enumerate(tagged):          # at least one result per planted cut
                assert not tag.startswith("cut") or start[q + 1] > start[q], (name, kind, k, tag)
            results += len(off)
        assert results > 100
    finally:
        ix.close()


# ---- 2. the relations the header states ---------------------------------------------------------------------------------------------

RELATED = ["acgt48k", "eng2doc", "chunks2doc"]


@pytest.mark.parametrize("name", RELATED)
def test_k_0_gives_the_offsets_of_locate(fixtures, gpu_ok, name):
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        pats = _patterns(fixtures, name, 0)
        start, off, cost, length, _, raw = ix.leven(pats, 0)
        noccs, located = ix.locate(pats, 1 << 30)
        assert np.array_equal(np.diff(start), noccs) and raw == len(off) > 50
        at = np.concatenate([[0], np.cumsum(noccs)])
        for q, p in enumerate(pats):
            assert np.array_equal(off[start[q]:start[q + 1]], np.sort(located[at[q]:at[q + 1]])), (name, q)
            assert not cost[start[q]:start[q + 1]].any() and (length[start[q]:start[q + 1]] == len(p)).all()
    finally:
        ix.close()


@pytest.mark.parametrize("name", RELATED)
def test_holds_every_occurrence_within_k_substitutions(fixtures, gpu_ok, name):
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        seen = 0
        for k in (1, 3):
            pats = _patterns(fixtures, name, k)
            start, off, cost, length, _, _ = ix.leven(pats, k)
            hstart, hoff, hcost, _ = ix.hamming(pats, k)
            for q in range(len(pats)):
                mine = dict(zip(off[start[q]:start[q + 1]].tolist(), cost[start[q]:start[q + 1]].tolist()))
                for w, c in zip(hoff[hstart[q]:hstart[q + 1]].tolist(), hcost[hstart[q]:hstart[q + 1]].tolist()):
                    assert w in mine and mine[w] <= c, (name, k, q, w)
            seen += len(hoff)
        assert seen > 100
    finally:
        ix.close()


@pytest.mark.parametrize("name", RELATED)
def test_results_are_the_located_strings_of_search_within_edit_distance(fixtures, gpu_ok, name):
    """k <= 2, both ways: T[p .. p + L) is one of ix.edit's strings for the pattern, with cost c (a row of that string of that
    length and cost is located at p); every located offset of an ix.edit string of cost c is a result with cost <= c"""
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        seen = 0
        for k in (1, 2):
            pats = [p for p in _patterns(fixtures, name, k) if 9 <= len(p) <= 100]
            start, off, cost, length, _, _ = ix.leven(pats, k)
            estart, first, last, ecost, elen = ix.edit(pats, k)
            nrows = last - first + 1
            rows = np.concatenate([np.arange(f, la + 1) for f, la in zip(first, last)]) if len(first) else np.zeros(0, dtype=np.int64)
            _, where = ix.extractor().context(rows=rows)          # SA[row]: the locate of the strings' ranges
            at = np.concatenate([[0], np.cumsum(nrows)])
            for q in range(len(pats)):
                o, c, ln = off[start[q]:start[q + 1]], cost[start[q]:start[q + 1]], length[start[q]:start[q + 1]]
                r0, r1 = int(estart[q]), int(estart[q + 1])
                w = where[at[r0]:at[r1]]
                wc, wl = np.repeat(ecost[r0:r1], nrows[r0:r1]).astype(np.int64), np.repeat(elen[r0:r1], nrows[r0:r1]).astype(np.int64)
                assert np.isin((o << 20 | ln.astype(np.int64)) << 2 | c, (w << 20 | wl) << 2 | wc).all(), (name, k, q)
                idx = np.searchsorted(o, w)
                assert len(w) == 0 or (idx < len(o)).all() and (o[np.minimum(idx, len(o) - 1)] == w).all() and (c[idx] <= wc).all(), (name, k, q)
                seen += len(o)
        assert seen > 100
    finally:
        ix.close()


# ---- 3. the sample path ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_forced_samples_equal_the_text_path(fixtures, gpu_ok, monkeypatch, name):
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        assert ix.extractor().info()["path"] == femto_amd.Extractor.PATH_TEXT
        assert ix.extractor(-1, True).info()["path"] == femto_amd.Extractor.PATH_SAMPLES
        for k in (1, 3):
            pats = _patterns(fixtures, name, k)
            text = ix.leven(pats, k)
            _same(text[:4], _expected(fixtures, name, k), (name, k))
            samples = ix.leven(pats, k, force_samples=True)
            _same(samples[:4], text[:4], (name, k, "samples"))
            assert samples[4:] == text[4:]
        # the windows in several chunks: 300-symbol patterns make the stride 306, so 4096 symbols hold 13 windows
        monkeypatch.setenv("FEMTO_AMD_LEVEN_CHUNK", "4096")
        pats = [p for p in _patterns(fixtures, name, 3) if len(p) >= 24]
        assert 297 <= max(len(p) for p in pats) <= 303
        want = expected(prepared(fixtures(name).docs), pats, 3)
        got = ix.leven(pats, 3, force_samples=True)
        _same(got[:4], want, (name, "chunks"))
        assert got[4] > 100
    finally:
        ix.close()


# ---- 4. the device form ---------------------------------------------------------------------------------------------------------

def _device_run(ix, pats, k, cand_capacity, capacity, stream, arrays=True, edit=None, wait=True, **kw):
    """femto_amd_leven_device on `stream`, chained after the upload on that stream with no synchronisation in between.
    edit(starts, flat, nsyms) -> (starts, flat, nsyms): what the call is handed in place of the well-formed inputs"""
    import torch
    plen, flat, starts = femto_amd.flatten(pats)
    nsyms = int(plen.sum())
    starts = np.concatenate([starts, [nsyms]]).astype(np.int64)
    if edit is not None:
        starts, flat, nsyms = edit(starts.copy(), flat.copy(), nsyms)
    with torch.cuda.stream(stream):
        buf = torch.zeros(len(flat) + 16, dtype=torch.int16, device=DEV)          # (8 symbols of slack on either side)
        buf[8:8 + len(flat)] = torch.from_numpy(flat.view(np.int16)).to(DEV, non_blocking=True)
        d_starts = torch.from_numpy(starts).to(DEV, non_blocking=True)
        cap = max(capacity, 1)
        o = dict(start=torch.full((len(pats) + 1,), -3, dtype=torch.int64, device=DEV), offset=torch.full((cap,), -3, dtype=torch.int64, device=DEV),
                 cost=torch.full((cap,), -3, dtype=torch.int32, device=DEV), length=torch.full((cap,), -3, dtype=torch.int32, device=DEV),
                 total=torch.full((5,), -3, dtype=torch.int64, device=DEV))
        a = (o["offset"], o["cost"], o["length"]) if arrays else (None, None, None)
        ix.leven_device(len(pats), nsyms, buf.data_ptr() + 16, d_starts, k, cand_capacity, capacity, o["start"], *a, o["total"],
                        stream=stream.cuda_stream, **kw)
    if not wait:
        return o, (buf, d_starts)
    stream.synchronize()
    return {key: v.cpu().numpy() for key, v in o.items()}


def _got(r, total=None):
    return (r["start"],) + tuple(r[f] if total is None else r[f][:total] for f in FIELDS[1:])


@pytest.mark.parametrize("name,kw", [("acgt48k", {}), ("eng2doc", {}), ("bytes256", {}), ("eng2doc", dict(force_samples=True))])
def test_capacities_on_a_stream_of_its_own(fixtures, gpu_ok, name, kw):
    import torch
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        for k in (1, 5):
            pats = _patterns(fixtures, name, k)
            want = _expected(fixtures, name, k)
            total, cands, raw = len(want[1]), _piece_candidates(ix, pats, k), ix.leven(pats, k, **kw)[5]
            assert total > 2 and cands > 2 and raw > total
            c0 = _device_run(ix, pats, k, cands, 0, st, arrays=False, **kw)          # the counting form: result_start is left as it is
            assert c0["total"][1:].tolist() == [1, raw, cands, 0] and (c0["start"] == -3).all()
            short = _device_run(ix, pats, k, cands, raw - 1, st, **kw)
            assert short["total"][1:].tolist() == [1, raw, cands, 0]
            full = _device_run(ix, pats, k, cands, raw, st, **kw)
            assert full["total"].tolist() == [total, 0, raw, cands, 0]
            _same(_got(full, total), want, (name, k, "capacity = raw"))
            for f in FIELDS[1:]:          # the raw records behind the distinct results are not the caller's
                assert (full[f][total:] == -3).all()
            more = _device_run(ix, pats, k, cands + 77, raw + 300, st, **kw)          # slots behind the results are not written
            assert more["total"].tolist() == [total, 0, raw, cands, 0]
            _same(_got(more, total), want, (name, k, "capacity > raw"))
            for f in FIELDS[1:]:
                assert (more[f][total:] == -3).all()
            few = _device_run(ix, pats, k, cands - 1, raw, st, **kw)          # one candidate short: only the candidate words are defined
            assert few["total"][3:].tolist() == [cands, 1]
            again = _device_run(ix, pats, k, cands, raw, st, **kw)          # ... and the call after it is whole
            _same(_got(again, total), want, (name, k, "again"))
        none = _device_run(ix, [], 1, 0, 0, st, arrays=False, **kw)
        assert none["total"].tolist() == [0, 0, 0, 0, 0] and none["start"].tolist() == [0]
    finally:
        ix.close()


@pytest.mark.parametrize("kw", [None, dict(text=0, dense_arrays=0), dict(rank_mode=1)])
def test_device_form_equals_the_host_form_on_other_handles(fixtures, gpu_ok, kw):
    import torch
    name = "chunks2doc"
    ix = femto_amd.Index(fixtures(name).index, device=0, options=kw) if kw else femto_amd.Index(fixtures(name).index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        for k in (0, 2, 5):
            pats = _patterns(fixtures, name, k)
            host = ix.leven(pats, k)
            _same(host[:4], _expected(fixtures, name, k), (kw, k))
            total = len(host[1])
            a = _device_run(ix, pats, k, host[4], host[5], st)
            b = _device_run(ix, pats, k, host[4], host[5], st)
            for r in (a, b):
                _same(_got(r, total), host[:4], (kw, k))
            assert a["total"].tolist() == b["total"].tolist() == [total, 0, host[5], host[4], 0]
    finally:
        ix.close()


# ---- 5. what the device form is handed ------------------------------------------------------------------------------------------

def _handed(fixtures, ix, st, pats, k, refused, edit, what, **kw):
    """the patterns `refused` have no results and no candidates; the others keep theirs.  kw: the extractor's (force_samples)"""
    text = prepared(fixtures("acgt48k").docs)
    kept = [p if q not in refused else None for q, p in enumerate(pats)]
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    per = [_occurrences(text, p, k) if p is not None else none for p in kept]
    want = (np.concatenate([[0], np.cumsum([len(r[0]) for r in per])]).astype(np.int64),) + tuple(np.concatenate([r[i] for r in per]) for i in range(3))
    served = [p for p in kept if p is not None]
    cands, raw = _piece_candidates(ix, served, k), ix.leven(served, k, **kw)[5]
    total = len(want[1])
    assert total > 10
    r = _device_run(ix, pats, k, cands + 5, raw + 5, st, edit=edit, **kw)
    assert r["total"].tolist() == [total, 0, raw, cands, 0], what
    _same(_got(r, total), want, (what,))
    assert (r["offset"][total:] == -3).all()


_seen = {}


def _occurrences(text, p, k):
    """the yardstick's answer for one pattern, kept: the batches of this section share their patterns"""
    key = (p.tobytes(), k)
    if key not in _seen:
        _seen[key] = occurrences(text, p, k)
    return _seen[key]


def test_device_form_refuses_patterns_and_keeps_their_neighbours(fixtures, gpu_ok):
    import torch
    name, k = "acgt48k", 2
    fx = fixtures(name)
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    base = [p for p in _patterns(fixtures, name, k) if 9 <= len(p) <= 100][:24]
    ix = femto_amd.Index(fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)

        def starts_negative(starts, flat, nsyms):
            starts[5] = -4          # pattern 4 has a negative length, pattern 5 starts in front of the symbols
            return starts, flat, nsyms

        def starts_beyond(starts, flat, nsyms):
            starts[7] = nsyms + 10          # pattern 6 ends behind the symbols, pattern 7 has a negative length
            return starts, flat, nsyms

        def nsyms_short(starts, flat, nsyms):
            return starts, flat, nsyms - 3          # the last pattern leaves [0, nsyms]

        def code(at, value):
            def edit(starts, flat, nsyms):
                flat[starts[at] + 1] = value
                return starts, flat, nsyms
            return edit

        _handed(fixtures, ix, st, base, k, {4, 5}, starts_negative, "negative start")
        _handed(fixtures, ix, st, base, k, {6, 7}, starts_beyond, "start behind the symbols")
        _handed(fixtures, ix, st, base, k, {len(base) - 1}, nsyms_short, "nsyms short of the last pattern")
        _handed(fixtures, ix, st, base, k, {3}, code(3, 2), "SEOF in a pattern")
        _handed(fixtures, ix, st, base, k, {3}, code(3, 4), "code 4")
        _handed(fixtures, ix, st, base, k, {8}, code(8, 261), "code 261")
        _handed(fixtures, ix, st, base, k, {9}, code(9, 0xffff), "code 0xffff")
        short = [doc[10:10 + k].astype(np.uint16) + OFFSET, doc[30:31].astype(np.uint16) + OFFSET]          # m = k and m = 1: both occur
        _handed(fixtures, ix, st, base[:7] + short + base[7:], k, {7, 8}, None, "m <= k")
        long = doc[100:100 + 32769].astype(np.uint16) + OFFSET          # would match whole; at the limit it is searched, and found
        at_limit = ix.leven([long[:32768]], k)
        assert at_limit[0].tolist() == [0, 5] and at_limit[1].tolist() == [98, 99, 100, 101, 102] and at_limit[2].tolist() == [2, 1, 0, 1, 2]
        assert at_limit[3].tolist() == [32770, 32769, 32768, 32767, 32766]
        _handed(fixtures, ix, st, base[:7] + [long] + base[7:] + [long], k, {7, len(base) + 1}, None, "m = 32769")
        _handed(fixtures, ix, st, base, k, set(), None, "nothing refused")
    finally:
        ix.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused(fixtures, gpu_ok):
    import torch
    fx = fixtures("eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    ok = np.array([70, 71, 72], dtype=np.uint16)
    try:
        bad = [lambda: ix.leven_device(1, 3, z, z, 32, 0, 0, z, None, None, None, z),
               lambda: ix.leven_device(1, 3, z, z, -1, 0, 0, z, None, None, None, z),
               lambda: ix.leven_device(1, 3, None, z, 1, 0, 0, z, None, None, None, z),
               lambda: ix.leven_device(1, 3, z, None, 1, 0, 0, z, None, None, None, z),
               lambda: ix.leven_device(1, 3, z, z, 1, 0, 0, None, None, None, None, z),
               lambda: ix.leven_device(1, 3, z, z, 1, 0, 0, z, None, None, None, None),
               lambda: ix.leven_device(1, 3, z, z, 1, 8, 8, z, z, None, z, z),          # a capacity without its arrays
               lambda: ix.leven_device(1, 3, z, z, 1, 8, 8, z, z, z, None, z),
               lambda: ix.leven_device(0, 3, z, z, 1, 0, 0, z, None, None, None, z),          # symbols without patterns
               lambda: ix.leven_device(1, 1 << 31, z, z, 1, 0, 0, z, None, None, None, z),          # the bounds the header states
               lambda: ix.leven_device(1 << 30, 3, z, z, 1, 0, 0, z, None, None, None, z),          # npat * (k + 1) = 2^31
               lambda: ix.leven_device(1, 3, z, z, 1, 1 << 31, 0, z, None, None, None, z),
               lambda: ix.leven_device(1, 3, z, z, 1, 0, 1 << 31, z, z, z, z, z),
               lambda: ix.leven_device(1, 3, z.data_ptr() + 1, z, 1, 0, 0, z, None, None, None, z),          # d_syms not 2-byte aligned
               lambda: ix.leven([ok], 32), lambda: ix.leven([ok], -1),
               lambda: ix.leven([ok], 3), lambda: ix.leven([ok, ok[:1]], 1),          # m <= k
               lambda: ix.leven([np.full(32769, 70, dtype=np.uint16)], 1),
               lambda: ix.leven([np.array([70, 4, 71], dtype=np.uint16)], 1),          # a code below 5
               lambda: ix.leven([np.array([70, 261, 71], dtype=np.uint16)], 1)]
        for n, call in enumerate(bad):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 3, n
        torch.cuda.synchronize()
        assert not z.any()          # nothing was written
        assert ix.leven([], 1)[0].tolist() == [0] and ix.leven([ok], 2)[4] >= 0
        # k = 31 is served: 40 symbols of the text with 31 edits to spend
        p = np.asarray(fx.docs[0][200:240], dtype=np.uint8).astype(np.uint16) + OFFSET
        got = ix.leven([p], 31)
        _same(got[:4], expected(prepared(fx.docs), [p], 31), ("k = 31",))
        at = got[1].tolist().index(200)
        assert got[2][at] == 0 and got[3][at] == 40 and got[4] > 1000
    finally:
        ix.close()
    multi = femto_amd.Index(fx.index, devices=[0, 0])
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            multi.leven_device(1, 3, z, z, 1, 0, 0, z, None, None, None, z)
        assert e.value.code == 6 and "multi-device" in str(e.value)
        pats = _patterns(fixtures, "eng2doc", 1)[:30]          # the host form runs on replica 0
        _same(multi.leven(pats, 1)[:4], expected(prepared(fx.docs), pats, 1), ("multi",))
    finally:
        multi.close()


# ---- 7. more than one workgroup, more than one grid of candidates ----------------------------------------------------------------

def _pool(fx, rng):
    """64 ten-mers of acgt48k's document, every third with one character changed, removed or added"""
    doc = np.asarray(fx.docs[0], dtype=np.uint8)
    have = np.unique(doc)
    pool = []
    for i in range(64):
        at = int(rng.integers(0, len(doc) - 11))
        p = doc[at:at + 10].astype(np.uint16) + OFFSET
        if i % 3 == 1:
            j = int(rng.integers(0, 10))
            if i % 9 == 1:
                p[j] = int(rng.choice(have[have != int(p[j]) - OFFSET])) + OFFSET
            elif i % 9 == 4:
                p = np.concatenate([p[:j], p[j + 1:], doc[at + 10:at + 11].astype(np.uint16) + OFFSET])
            else:
                p = np.concatenate([p[:j], [int(rng.choice(have)) + OFFSET], p[j:9]]).astype(np.uint16)
        assert len(p) == 10
        pool.append(p)
    return pool


def _picked(per, pick):
    """the answer of the batch pool[pick] from each pool pattern's (offsets, costs, lengths) `per`"""
    return (np.concatenate([[0], np.cumsum([len(per[i][0]) for i in pick])]).astype(np.int64),) + tuple(np.concatenate([per[i][c] for i in pick]) for c in range(3))


@pytest.mark.parametrize("npat,grid", [(257, "1"), (70001, None)])
def test_large_batches(fixtures, gpu_ok, monkeypatch, npat, grid):
    """257 patterns are more than one workgroup of the piece table (16 per workgroup) and, with FEMTO_AMD_LEVEN_GRID=1, hundreds
    of candidates per lane of the extend kernel; 70 001 ten-mers under k = 1 have pieces of five symbols -- some 48 candidates each
    on this text, millions in all: more than the lanes of the extend kernel's largest grid (64 workgroups per CU)"""
    name, k = "acgt48k", 1
    fx = fixtures(name)
    text = prepared(fx.docs)
    rng = np.random.default_rng(npat)
    pool = _pool(fx, rng)
    per = [occurrences(text, p, k) for p in pool]
    pick = rng.integers(0, len(pool), size=npat)
    pats = [pool[i] for i in pick]
    want = _picked(per, pick)
    if grid:
        monkeypatch.setenv("FEMTO_AMD_LEVEN_GRID", grid)
    ix = femto_amd.Index(fx.index, device=0)
    try:
        start, off, cost, length, cands, raw = ix.leven(pats, k)
        _same((start, off, cost, length), want, (npat,))
        assert cands == _piece_candidates(ix, pats, k)
        assert len(off) >= npat and raw > len(off) and cands > (256 * 64 * 256 if not grid else 256 * 16)
    finally:
        ix.close()


def test_power_of_two_patterns_with_slots_behind_the_results(fixtures, gpu_ok):
    """npat = 256 and capacity = raw + 300: the slots behind the live records carry the pattern key 256, which needs
    bits_of(256) = 9 bits where the largest pattern number, 255, needs 8 -- sorted over 8 bits they would stand among pattern 0's
    results.  256 picks of test_large_batches' pool through the device form, the candidates sized by the pieces' counts"""
    import torch
    name, k, npat = "acgt48k", 1, 256
    fx = fixtures(name)
    text = prepared(fx.docs)
    rng = np.random.default_rng(npat)
    pool = _pool(fx, rng)
    per = [occurrences(text, p, k) for p in pool]
    pick = rng.integers(0, len(pool), size=npat)
    pats = [pool[i] for i in pick]
    want = _picked(per, pick)
    total = len(want[1])
    assert total > 0 and want[0][1] < total          # results of a pattern other than 0: the ones a key of 0 would stand in front of
    ix = femto_amd.Index(fx.index, device=0)
    try:
        cands, raw = _piece_candidates(ix, pats, k), ix.leven(pats, k)[5]
        r = _device_run(ix, pats, k, cands, raw + 300, torch.cuda.Stream(device=DEV))
        assert r["total"].tolist() == [total, 0, raw, cands, 0]
        _same(_got(r, total), want, (npat, k))
        for f in FIELDS[1:]:
            assert (r[f][total:] == -3).all()
    finally:
        ix.close()


