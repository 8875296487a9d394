"""`-m gpu`: common sequences (include/femto_amd.h "common sequences") against the restatement of tests/similar_util.py: the
matching statistics of every fixture and every rank policy, the selected sequences, the groups and the scores, stop lists, and
the device calls chained on one stream."""
import zlib

import numpy as np
import pytest

import femto_amd
from oracle import pyoracle
from regexp_util import KINDS
from similar_util import Text, document_scores, groups_of, index_numerator, match_lengths, ranked

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXTURES = ["acgt48k", "b1000", "bytes256", "eng2doc", "chunks2doc", "runs3doc", "counter400_small", "construct_kat"]
_texts, _lens = {}, {}


def _T(fixtures, name):
    if name not in _texts:
        _texts[name] = Text(fixtures(name).docs)
    return _texts[name]


def _want_lens(fixtures, name, tag, q, max_len=0):
    """the restatement's answer, computed once per (fixture, query, max_len)"""
    key = (name, tag, max_len)
    if key not in _lens:
        _lens[key] = match_lengths(_T(fixtures, name), q, max_len)
    return _lens[key]


def _substituted(fx, n=2048, at=None):
    allb = np.concatenate(fx.docs)
    at = len(allb) // 3 if at is None else at
    q = allb[at:at + n].copy()
    q[::37] ^= 0x55
    return q


def _queries(fx, name):
    """(tag, bytes): the fixture's text with a substitution every 37 bytes; the end of one document joined to the start of the
    next; a whole short document (its first 1024 bytes when it is longer); uniform random bytes"""
    out = [("subst", _substituted(fx))]
    if len(fx.docs) > 1:
        out.append(("joint", np.concatenate([fx.docs[0][-700:], fx.docs[1][:700]])))
    out.append(("whole", min(fx.docs, key=lambda d: (len(d) < 9, len(d)))[:1024].copy()))
    out.append(("random", np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, 1500).astype(np.uint8)))
    return out


def _check_stats(ix, q, max_len, want, what):
    lens, first, last = ix.match_stats(q, max_len=max_len)
    assert np.array_equal(lens, want), (what, np.nonzero(lens != want)[0][:8])
    n = len(q)
    if n == 0:
        return
    cap = 32768 if max_len <= 0 else max_len
    sym = np.asarray(q, dtype=np.uint8).astype(np.uint16) + 5
    f, l = ix.count([sym[j - lens[j] + 1:j + 1] for j in range(n)])
    assert np.array_equal(first, f) and np.array_equal(last, l), what
    assert (first <= last).all()
    longer = [sym[j - lens[j]:j + 1] for j in range(n) if j - lens[j] >= 0 and lens[j] < cap]
    if longer:
        f, l = ix.count(longer)
        assert (f > l).all(), what
    only = ix.match_stats(q, max_len=max_len, ranges=False)
    assert np.array_equal(only, want), what


# ---- 1. matching statistics -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_match_stats_equal_the_restatement(fixtures, gpu_ok, name):
    fx = fixtures(name)
    ix = femto_amd.Index(fx.index, device=0)
    try:
        for tag, q in _queries(fx, name):
            for max_len in (1, 7, 0):
                want = _want_lens(fixtures, name, tag, q, max_len)
                _check_stats(ix, q, max_len, want, (name, tag, max_len))
            full = _want_lens(fixtures, name, tag, q, 0)
            if tag == "whole":          # lengths run into the start of the file
                assert (full == np.arange(len(q)) + 1).all()
            if tag == "random":
                assert (full <= 3).mean() > 0.9
            if tag == "joint" and len(q) == 1400:          # the first document's tail is found whole; the restatement stops at the boundary
                assert full[699] == 700
    finally:
        ix.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096])
def test_match_stats_sizes(fixtures, gpu_ok, n):
    fx = fixtures("eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        q = _substituted(fx, n, at=1000)
        for max_len in (1, 7, 0):
            _check_stats(ix, q, max_len, _want_lens(fixtures, "eng2doc", "size%d" % n, q, max_len), (n, max_len))
    finally:
        ix.close()


def test_match_stats_unaligned_bytes_and_untouched_slots(fixtures, gpu_ok):
    """d_bytes at every offset of an 8-byte word; nothing is written beyond n"""
    import torch
    fx = fixtures("chunks2doc")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        q = _substituted(fx, 300)
        want = _want_lens(fixtures, "chunks2doc", "s300", q)
        for off in range(8):
            buf = torch.zeros(400, dtype=torch.uint8, device=DEV)
            buf[8 + off:8 + off + 300] = torch.from_numpy(q).to(DEV)
            d_len = torch.full((310,), -7, dtype=torch.int32, device=DEV)
            ix.match_stats_device(300, buf.data_ptr() + 8 + off, d_len)
            torch.cuda.synchronize()
            got = d_len.cpu().numpy()
            assert np.array_equal(got[:300], want) and (got[300:] == -7).all(), off
    finally:
        ix.close()


# ---- 2. every rank policy -------------------------------------------------------------------------------------------------------

OPTION_SETS = [None, dict(rank_units=0), dict(char_rank_lines=0), dict(hbm_budget_bytes=400_000), dict(text=0, dense_arrays=0),
               dict(rank_units=3, dense_arrays=0, text=0), dict(rank_mode=1)]


def _open_set(fx, kw):
    """(handle, the one rank policy its layout proves: regexp_util.KINDS)"""
    ix = femto_amd.Index(fx.index, device=0, options=kw) if kw else femto_amd.Index(fx.index, device=0)
    kinds = [k for k, v in KINDS.items() if v.proves(ix)]
    assert len(kinds) == 1, (kw, ix.rank_mode, ix.pack_info())
    return ix, kinds[0]


def test_option_sets_reach_every_policy(fixtures, gpu_ok):
    """the five derived kinds and the mode-1 path are each reached by the sets test_every_rank_policy runs"""
    reached = set()
    for name in ("acgt48k", "eng2doc"):
        for kw in OPTION_SETS:
            ix, kind = _open_set(fixtures(name), kw)
            ix.close()
            reached.add(kind)
    assert reached == {"ru", "rum", "pack", "ind", "pack2", "wave"}, reached


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_every_rank_policy(fixtures, gpu_ok, name):
    fx = fixtures(name)
    qs = _queries(fx, name)
    base = femto_amd.Index(fx.index, device=0)
    try:
        want = {(tag, ml): base.match_stats(q, max_len=ml) for tag, q in qs for ml in (7, 0)}
        for tag, q in qs:
            assert np.array_equal(want[(tag, 0)][0], _want_lens(fixtures, name, tag, q, 0))
    finally:
        base.close()
    for kw in OPTION_SETS:
        ix, kind = _open_set(fx, kw)
        try:
            modes = [ix.rank_mode] + ([0] if kw == dict(rank_mode=1) else [])      # mode 0 with the derived lines: the same lane policy
            for mode in modes:
                ix.set_rank_mode(mode)
                for tag, q in qs:
                    for ml in (7, 0):
                        got = ix.match_stats(q, max_len=ml)
                        for a, b in zip(got, want[(tag, ml)]):
                            assert np.array_equal(a, b), (name, kw, kind, mode, tag, ml)
        finally:
            ix.close()


def test_range_split_part_refuses(fixtures, gpu_ok):
    import torch
    fx = fixtures("eng2doc")
    a = femto_amd.Index(fx.index, device=0, part=0, nparts=2)
    b = femto_amd.Index(fx.index, device=0, part=1, nparts=2)
    try:
        a.split_attach_local(b)
        b.split_attach_local(a)
        a.split_commit()
        b.split_commit()
        z = torch.zeros(64, dtype=torch.int64, device=DEV)
        for call in (lambda: a.match_stats_device(8, z, z), lambda: a.common_sequences_device(8, z, z, z, z, z, z, z, 8, z),
                     lambda: a.common_groups_device(8, z, z, z, z, z, z, z, z, z, z, z, z),
                     lambda: a.similar_documents_device(8, z, z, z, z, z, z, 8, z, z, z), lambda: a.similar(b"abcdefgh")):
            with pytest.raises(femto_amd.FemtoAmdError) as e:
                call()
            assert e.value.code == 6 and "range-split part" in str(e.value)
    finally:
        a.close()
        b.close()


# ---- 3. sequences, groups, documents --------------------------------------------------------------------------------------------

def _group_query(fx, name):
    if name == "counter400_small":
        d = fx.docs[0]
        return np.concatenate([d[10:130], d[10:130], d[200:330], np.frombuffer(b"#", dtype=np.uint8), d[10:130]])
    q = _substituted(fx, 1500)
    return np.concatenate([q, q[100:400], q[:64]])          # repeated sequences: here > 1


def _hits_of(ix, t, mo):
    """the located occurrences per document of a group: brute force, or -- under the clamp -- what the document listing's host form
    lists for the group's pattern"""
    def f(g):
        occ = t.occurrences(g.bytes)
        if len(occ) <= mo + 1:
            return t.hits(g.bytes)
        starts, docs, hits = ix.documents([g.pattern], mo)
        return {int(d): int(h) for d, h in zip(docs, hits)}
    return f


@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc", "runs3doc", "counter400_small"])
def test_groups_and_scores(fixtures, gpu_ok, name):
    fx, t = fixtures(name), _T(fixtures, name)
    q = _group_query(fx, name)
    n = len(q)
    lens = _want_lens(fixtures, name, "groups", q)
    seqs, groups, group_of = groups_of(q, lens)
    assert len(groups) >= 3 and max(g.here for g in groups) > 1
    there = [len(t.occurrences(g.bytes)) for g in groups]
    if name == "runs3doc":
        assert max(there) > 101          # a range the default clamp cuts
    ix = femto_amd.Index(fx.index, device=0)
    try:
        first, last = ix.count([g.pattern for g in groups])
        assert (last - first + 1).tolist() == there
        for mo in (1, 3, 100):
            r = ix.similar(q, max_occs=mo)
            assert np.array_equal(r.len, lens) and r.n == n
            assert r.g_len.tolist() == [g.len for g in groups] and r.g_here.tolist() == [g.here for g in groups]
            assert r.g_min_start.tolist() == [g.min_start for g in groups]
            assert np.array_equal(r.g_first, first) and np.array_equal(r.g_last, last) and r.g_kept.all()
            assert r.index_numerator == index_numerator(t, groups) and r.index_score == r.index_numerator / n
            score, nseq = document_scores(len(t.docs), groups, _hits_of(ix, t, mo))
            want = ranked(t, n, score, nseq)
            got = list(zip(r.doc.tolist(), r.doc_numerator.tolist(), r.doc_seqs.tolist(), r.doc_score.tolist()))
            assert got == want, (name, mo)
        assert ix.similar(b"").n == 0 and ix.similar(b"").ngroups == 0 and ix.similar(q[:7]).ngroups == 0
        r4 = ix.similar(q, min_len=12, max_len=20)
        l4 = _want_lens(fixtures, name, "groups", q, 20)
        assert np.array_equal(r4.len, l4) and r4.g_len.tolist() == [g.len for g in groups_of(q, l4, 12)[1]]
    finally:
        ix.close()


def _chain(ix, q, stream, min_len=0, max_occs=0, seq_cap=None, off_cap=None, keep=None):
    """the device calls back to back on `stream`; returns the tensors"""
    import torch
    n = len(q)
    with torch.cuda.stream(stream):
        buf = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
        buf[8:8 + n] = torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
        i64 = lambda k, v=-3: torch.full((max(k, 1),), v, dtype=torch.int64, device=DEV)
        i32 = lambda k, v=-3: torch.full((max(k, 1),), v, dtype=torch.int32, device=DEV)
        cap = n if seq_cap is None else seq_cap
        ocap = 20000 if off_cap is None else off_cap
        o = dict(len=i32(n), first=i64(n), last=i64(n), s_start=i64(cap), s_len=i32(cap), s_first=i64(cap), s_last=i64(cap), s_tot=i64(2),
                 group_of=i64(cap), g_len=i32(cap), g_first=i64(cap), g_last=i64(cap), g_here=i32(cap), g_ms=i64(cap), ng=i64(2),
                 offs=i64(ocap), score=i64(ix.info.number_of_documents, 99), seqs=i32(ix.info.number_of_documents, 99), tot=i64(2), steps=i64(2))
        s = stream.cuda_stream
        ix.match_stats_device(n, buf.data_ptr() + 8, o["len"], o["first"], o["last"], stream=s)
        ix.match_stats_steps_device(n, buf.data_ptr() + 8, o["steps"], stream=s)
        ix.common_sequences_device(n, o["len"], o["first"], o["last"], o["s_start"], o["s_len"], o["s_first"], o["s_last"], cap, o["s_tot"],
                                   min_len=min_len, stream=s)
        ix.common_groups_device(cap, o["s_tot"], o["s_start"], o["s_len"], o["s_first"], o["s_last"], o["group_of"], o["g_len"], o["g_first"],
                                o["g_last"], o["g_here"], o["g_ms"], o["ng"], stream=s)
        ix.similar_documents_device(cap, o["ng"], o["g_len"], o["g_first"], o["g_last"], o["g_here"], o["offs"], ocap, o["score"], o["seqs"],
                                    o["tot"], d_g_keep=keep, max_occs=max_occs, stream=s)
    stream.synchronize()
    o["buf"] = buf
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", ["eng2doc", "runs3doc"])
def test_device_forms_and_capacities(fixtures, gpu_ok, name):
    import torch
    fx, t = fixtures(name), _T(fixtures, name)
    q = _group_query(fx, name)
    lens = _want_lens(fixtures, name, "groups", q)
    seqs, groups, group_of = groups_of(q, lens)
    ns, ng = len(seqs), len(groups)
    ix = femto_amd.Index(fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        o = _chain(ix, q, st)
        assert o["s_tot"].tolist() == [ns, 0] and o["ng"][0] == ng and o["ng"][1] == index_numerator(t, groups)
        assert list(zip(o["s_start"][:ns].tolist(), o["s_len"][:ns].tolist())) == seqs and (o["s_start"][ns:] == -3).all()
        assert o["group_of"][:ns].tolist() == group_of and (o["group_of"][ns:] == -3).all()
        assert o["g_len"][:ng].tolist() == [g.len for g in groups] and (o["g_len"][ng:] == -3).all()
        j = np.array([s + l - 1 for s, l in seqs])
        assert np.array_equal(o["s_first"][:ns], o["first"][j]) and np.array_equal(o["s_last"][:ns], o["last"][j])
        score, nseq = document_scores(len(t.docs), groups, _hits_of(ix, t, 100))
        assert np.array_equal(o["score"], score) and np.array_equal(o["seqs"], nseq) and o["tot"][1] == 0
        rows = int(o["tot"][0])
        want_rows = sum(min(c, 100) if c > 101 else c for c in (len(t.occurrences(g.bytes)) for g in groups))
        assert rows == want_rows
        located = np.sort(o["offs"][:rows])
        if max(len(t.occurrences(g.bytes)) for g in groups) <= 101:      # no clamp: every occurrence's text position
            wantpos = np.sort([int(t.doc_starts[d]) + off for g in groups for d, off in t.occurrences(g.bytes)])
            assert np.array_equal(located, wantpos)
        steps = o["steps"].tolist()
        assert steps[0] >= int(lens.sum()) and steps[0] <= int(lens.sum()) + len(q) and 0 <= steps[1] <= steps[0]
        # a keep mask: only the kept groups count
        keep = np.zeros(len(q), dtype=np.uint8)
        keep[:ng:2] = 1
        ok = _chain(ix, q, st, keep=torch.from_numpy(keep).to(DEV))
        score, nseq = document_scores(len(t.docs), groups, _hits_of(ix, t, 100), kept=keep)
        assert np.array_equal(ok["score"], score) and np.array_equal(ok["seqs"], nseq)
        # capacities one short: the flag is set and the total stays exact
        o1 = _chain(ix, q, st, seq_cap=ns - 1)
        assert o1["s_tot"].tolist() == [ns, 1] and list(zip(o1["s_start"].tolist(), o1["s_len"].tolist())) == seqs[:ns - 1]
        o2 = _chain(ix, q, st, off_cap=rows - 1)
        assert o2["tot"].tolist() == [rows, 1] and not o2["score"].any() and not o2["seqs"].any()
        o3 = _chain(ix, q, st, off_cap=rows)
        assert o3["tot"].tolist() == [rows, 0] and np.array_equal(o3["score"], o["score"])
    finally:
        ix.close()


# ---- 4. stop lists --------------------------------------------------------------------------------------------------------------

def test_the_index_as_its_own_stop_list(fixtures, gpu_ok):
    fx = fixtures("eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        q = _group_query(fx, "eng2doc")
        r = ix.similar(q, not_indexes=[ix])
        plain = ix.similar(q)
        assert r.ngroups == plain.ngroups > 0 and not r.g_kept.any() and r.index_numerator == 0 and r.index_score == 0 and r.ndocs == 0
        assert np.array_equal(r.g_len, plain.g_len) and np.array_equal(r.g_first, plain.g_first) and plain.ndocs > 0
    finally:
        ix.close()


def test_stop_list_of_another_index(fixtures, gpu_ok):
    eng, acgt = fixtures("eng2doc"), fixtures("acgt48k")
    t = _T(fixtures, "eng2doc")
    allb, a = np.concatenate(eng.docs), np.concatenate(acgt.docs)
    parts = []
    for k in range(12):
        parts += [allb[3000 + k * 700:3090 + k * 700], a[100 + k * 977:117 + k * 977 + k]]
    q = np.concatenate(parts)
    lens = _want_lens(fixtures, "eng2doc", "spliced", q)
    seqs, groups, group_of = groups_of(q, lens, 2)
    o = pyoracle.Oracle(acgt.index)
    try:
        f, l = o.count([g.pattern for g in groups])
    finally:
        o.close()
    kept = (f > l).astype(np.uint8)
    assert kept.any() and not kept.all()
    ix, stop = femto_amd.Index(eng.index, device=0), femto_amd.Index(acgt.index, device=0)
    try:
        r = ix.similar(q, min_len=2, not_indexes=[stop])
        assert r.g_len.tolist() == [g.len for g in groups] and np.array_equal(r.g_kept, kept)
        assert r.index_numerator == index_numerator(t, groups, kept)
        score, nseq = document_scores(len(t.docs), groups, _hits_of(ix, t, 100), kept=kept)
        assert list(zip(r.doc.tolist(), r.doc_numerator.tolist(), r.doc_seqs.tolist(), r.doc_score.tolist())) == ranked(t, len(q), score, nseq)
        two = ix.similar(q, min_len=2, not_indexes=[stop, stop])
        assert np.array_equal(two.g_kept, kept)
    finally:
        ix.close()
        stop.close()


# ---- 5. one stream --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [None, dict(text=0, dense_arrays=0), dict(rank_mode=1)])
def test_chain_on_one_stream_equals_the_host_form(fixtures, gpu_ok, kw):
    import torch
    fx = fixtures("chunks2doc")
    q = _group_query(fx, "chunks2doc")
    ix = femto_amd.Index(fx.index, device=0, options=kw) if kw else femto_amd.Index(fx.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        o = _chain(ix, q, st, min_len=6, max_occs=3)
        r = ix.similar(q, min_len=6, max_occs=3)
        ng = r.ngroups
        assert ng > 0 and o["ng"][0] == ng and np.array_equal(o["len"], r.len)
        for dev, host in (("g_len", r.g_len), ("g_first", r.g_first), ("g_last", r.g_last), ("g_here", r.g_here), ("g_ms", r.g_min_start)):
            assert np.array_equal(o[dev][:ng], host), dev
        assert o["ng"][1] == r.index_numerator
        assert sorted(np.nonzero(o["score"])[0].tolist()) == sorted(r.doc.tolist()) and r.ndocs > 0
        assert o["score"][r.doc].tolist() == r.doc_numerator.tolist() and o["seqs"][r.doc].tolist() == r.doc_seqs.tolist()
    finally:
        ix.close()
