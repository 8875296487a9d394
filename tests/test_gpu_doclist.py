"""Document listing on the GPU (femto_amd_doclist_device / femto_amd_docset_device and their host forms) against the numpy
restatement of tests/doclist_util.py: the golden fixtures through the locate chain on one stream, synthetic segments that straddle
the size classes, the persistent loops taken more than once, a search end to end against a brute-force scan, liveness, the set
operations, refusals.

One departure from the letter of the plan, forced by arithmetic: the synthetic index (700 documents of 1..90 bytes) has about
32 000 text positions, so its 200 000-row segment cannot hold DISTINCT offsets.  That segment holds every position of the text at
least once and random repeats; every other segment holds distinct offsets.  The restatement counts a repeated offset as another
row of its document, which is what the kernels owe."""
import numpy as np
import pytest

import femto_amd
import doclist_util as du
from gpu_common import _open

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -77


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Lists:
    """output buffers of one femto_amd_doclist_device call, pre-filled with a sentinel"""

    def __init__(self, npats, capacity):
        import torch
        f = lambda n, dt: torch.full((max(n, 1),), SENT, dtype=dt, device=DEV)
        self.ndocs, self.docs, self.docs32, self.hits = f(npats, torch.int32), f(capacity, torch.int64), f(capacity, torch.int32), f(capacity, torch.int32)
        self.pair_doc, self.pair_off, self.doc_total, self.status = f(capacity, torch.int64), f(capacity, torch.int64), f(1, torch.int64), f(1, torch.int32)
        self.npats = npats

    def call(self, ix, d_ostarts, d_offs, capacity, d_total, stream=0):
        ix.doclist_device(self.npats, d_ostarts.data_ptr(), d_offs.data_ptr(), capacity, d_total.data_ptr(), self.ndocs.data_ptr(),
                          self.docs.data_ptr(), self.docs32.data_ptr(), self.hits.data_ptr(), self.pair_doc.data_ptr(), self.pair_off.data_ptr(),
                          self.doc_total.data_ptr(), self.status.data_ptr(), stream)

    def untouched(self, but_status=True):
        outs = [self.ndocs, self.docs, self.docs32, self.hits, self.pair_doc, self.pair_off, self.doc_total] + ([] if but_status else [self.status])
        return all(bool((o == SENT).all()) for o in outs)

    def check(self, want, out_starts, what=()):
        rows = int(out_starts[-1])
        n = self.npats
        assert int(self.status[0]) == 0, what
        assert np.array_equal(self.ndocs.cpu().numpy()[:n], want.ndocs), ("ndocs",) + what
        assert int(self.doc_total[0]) == int(want.ndocs.sum()), ("doc_total",) + what
        lv = want.live
        assert np.array_equal(self.docs.cpu().numpy()[:rows][lv], want.docs[lv]), ("docs",) + what
        assert np.array_equal(self.docs32.cpu().numpy()[:rows][lv], want.docs[lv].astype(np.int32)), ("docs32",) + what
        assert np.array_equal(self.hits.cpu().numpy()[:rows][lv], want.hits[lv]), ("hits",) + what
        assert np.array_equal(self.pair_doc.cpu().numpy()[:rows], want.pair_doc), ("pair_doc",) + what
        assert np.array_equal(self.pair_off.cpu().numpy()[:rows], want.pair_off), ("pair_off",) + what
        # nothing behind the rows
        for o in (self.docs, self.docs32, self.hits, self.pair_doc, self.pair_off):
            assert bool((o[rows:] == SENT).all()), ("wrote behind the rows",) + what


def _chain_then_list(ix, plen, flat, starts, max_occs, cap):
    """locate_device -> doclist_device on ONE non-default stream, no synchronise between; returns (Lists, out_starts, offsets, noccs)"""
    import torch
    n = len(plen)
    d_plen, d_flat, d_starts = _t(plen), _t(flat.view(np.int16)), _t(starts)
    d_noccs = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_ost = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    d_off = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    d_tot = torch.zeros(2, dtype=torch.int64, device=DEV)
    L = Lists(n, cap)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ix.locate_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), max_occs, 0, 0, d_noccs.data_ptr(), d_ost.data_ptr(),
                         d_off.data_ptr(), cap, d_tot.data_ptr(), stream=s.cuda_stream)
        L.call(ix, d_ost, d_off, cap, d_tot, stream=s.cuda_stream)
    s.synchronize()
    tot, over = d_tot.cpu().tolist()
    assert over == 0 and tot <= cap
    return L, d_ost.cpu().numpy(), d_off.cpu().numpy()[:tot], d_noccs.cpu().numpy()


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc", "runs3doc", "acgt48k"])
def test_goldens(fixtures, gpu_ok, name):
    fx = fixtures(name)
    ends = du.doc_ends(fx.docs)
    plen, flat, starts = fx.patterns
    ix = _open(fx.index)
    try:
        assert np.array_equal(ends, np.cumsum([len(d) + 1 for d in fx.docs]))
        for mo, noccs, offs in fx.locate_cases():
            out_starts = np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)])
            want = du.listing(ends, offs, out_starts)
            L, got_starts, got_offs, got_noccs = _chain_then_list(ix, plen, flat, starts, mo, len(offs) + 16)
            assert np.array_equal(got_starts, out_starts) and np.array_equal(got_offs, offs), (name, mo)
            L.check(want, out_starts, (name, mo))
            if len(fx.docs) == 1:      # one document: every non-empty list is [0] with hits = noccs
                nz = noccs > 0
                assert np.array_equal(L.ndocs.cpu().numpy(), nz.astype(np.int32))
                assert not L.docs.cpu().numpy()[out_starts[:-1][nz]].any()
                assert np.array_equal(L.hits.cpu().numpy()[out_starts[:-1][nz]], noccs[nz])
            pats = [flat[starts[i]:starts[i] + plen[i]] for i in range(len(plen))]
            ds, docs, hits = ix.documents(pats, mo)
            wds, wdocs, whits = du.packed(want, out_starts)
            assert np.array_equal(ds, wds) and np.array_equal(docs, wdocs) and np.array_equal(hits, whits), (name, mo, "documents()")
    finally:
        ix.close()


# ---- the synthetic index of cases 2, 3 and 5 -----------------------------------------------------------------------------------

class Synth:
    pass


@pytest.fixture(scope="module")
def synth(tmp_path_factory, gpu_ok):
    rng = np.random.default_rng(20240607)
    S = Synth()
    S.docs = [rng.integers(ord("a"), ord("b") + 1, int(rng.integers(1, 91))).astype(np.uint8) for _ in range(700)]
    S.path = str(tmp_path_factory.mktemp("doclist") / "index")
    femto_amd.build_index(S.path, S.docs, params=None, infos=["d%d" % i for i in range(700)], device=0)
    S.ends = du.doc_ends(S.docs)
    S.N = int(S.ends[-1])
    S.text = np.concatenate([np.concatenate([d, [0]]) for d in S.docs]).astype(np.uint8)    # 0 where the SEOF stands
    S.ix = _open(S.path)
    assert S.ix.info.total_length == S.N and S.ix.info.number_of_documents == 700
    yield S
    S.ix.close()


def _grams():
    pats = []
    for k in (1, 2, 3):
        for v in range(2 ** k):
            pats.append(bytes(ord("a") + ((v >> (k - 1 - j)) & 1) for j in range(k)))
    return pats + [b"c", b"abz"]


@pytest.fixture(scope="module")
def searched(synth):
    """case 3's chains, shared with case 5: {max_occs: (Lists, out_starts, offsets, noccs)}"""
    S = synth
    pats = [np.frombuffer(p, dtype=np.uint8).astype(np.uint16) + 5 for p in _grams()]
    plen, flat, starts = femto_amd.flatten(pats)
    S.pats = pats
    return {mo: _chain_then_list(S.ix, plen, flat, starts, mo, 14 * S.N + 16) for mo in (1 << 20, 5)}


# ---- 2. synthetic segments ----------------------------------------------------------------------------------------------------

def test_synthetic_segments(synth):
    import torch
    S = synth
    w, g = femto_amd.doclist_info()
    rng = np.random.default_rng(5)
    N, ends = S.N, S.ends
    firsts = np.concatenate([[0], ends[:-1]])
    longest = int(np.argmax(ends - firsts))
    assert ends[longest] - firsts[longest] >= w - 1

    def draw(n, must=()):
        must = np.unique(np.asarray(must, dtype=np.int64))
        rest = np.setdiff1d(np.arange(N, dtype=np.int64), must)
        return rng.permutation(np.concatenate([must, rng.choice(rest, n - len(must), replace=False)]))

    every_doc = np.concatenate([firsts, ends - 1])                    # each document's first position and its SEOF
    big = np.concatenate([np.arange(N, dtype=np.int64), rng.integers(0, N, 200000 - N)])
    segs = [[], [], [0], [0, N - 1],
            rng.permutation(np.arange(firsts[longest], firsts[longest] + w - 1)),     # w - 1 rows, all in one document
            draw(w, [0, N - 1]), [], draw(w + 1, [ends[3] - 1, ends[3]]),
            rng.permutation(every_doc),                                                # touches every document
            draw(g - 1, every_doc), draw(g, [0]), [], [], draw(g + 1, [N - 1]), draw(4 * g + 3, every_doc),
            rng.permutation(big), []]
    sizes = [len(s) for s in segs]
    assert set([0, 1, 2, w - 1, w, w + 1, g - 1, g, g + 1, 4 * g + 3, 200000]) <= set(sizes)
    for s in segs[:-2]:
        assert len(np.unique(s)) == len(s)
    out_starts = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    offs = np.concatenate([np.asarray(s, dtype=np.int64) for s in segs])
    want = du.listing(ends, offs, out_starts)
    assert want.ndocs[8] == 700 and want.ndocs[4] == 1 and want.ndocs[-2] == 700
    rows = len(offs)
    for cap in (rows, rows + 1000):
        L = Lists(len(segs), cap)
        L.call(S.ix, _t(out_starts), _t(np.concatenate([offs, np.full(cap - rows, -5, dtype=np.int64)])), cap, _t(np.array([rows, 0], dtype=np.int64)))
        torch.cuda.synchronize()
        L.check(want, out_starts, ("synthetic", cap))


# ---- 2b. the persistent loops taken more than once -----------------------------------------------------------------------------
# persistent_grid gives a kernel at most eight workgroups per CU; the cases below are sized from the device's CU count so that a
# workgroup goes round its loop at least twice, and each asserts that from its own inputs before it calls.

GUARD = 256


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _distinct(rng, N, n, must=()):
    """n distinct text positions in random order, those of `must` among them"""
    must = np.unique(np.asarray(must, dtype=np.int64))
    pick = rng.choice(N, n, replace=False).astype(np.int64)
    return rng.permutation(np.concatenate([must, pick[~np.isin(pick, must)][:n - len(must)]]))


def _list_segments(S, segs, what):
    """one femto_amd_doclist_device call with capacity == rows over buffers that hold GUARD entries more, checked against the
    restatement, which is returned"""
    import torch
    out_starts = np.concatenate([[0], np.cumsum([len(s) for s in segs], dtype=np.int64)])
    offs = np.concatenate([np.asarray(s, dtype=np.int64) for s in segs])
    rows = len(offs)
    want = du.listing(S.ends, offs, out_starts)
    L = Lists(len(segs), rows + GUARD)
    L.call(S.ix, _t(out_starts), _t(offs), rows, _t(np.array([rows, 0], dtype=np.int64)))
    torch.cuda.synchronize()
    L.check(want, out_starts, what)
    return want


def test_more_mid_segments_than_workgroups(synth):
    """More workgroup-class segments than doclist_group_kernel has workgroups: a workgroup sorts a second and a third segment,
    of another padded size, in the LDS the one before used; more than 1024 segments, so doclist_total_kernel adds from several
    workgroups.  A segment of at least 700 rows touches every document: all 1400 first and last positions where it has the room,
    the 700 first positions otherwise.
    Not run: a capacity at which mid_max clips the list.  mid_max is capacity / (wave_max + 1), the call lists nothing unless all
    rows fit the capacity, and every listed segment has more than wave_max rows: segments that do not overlap cannot outnumber
    mid_max, and doclist_util.listing has no notion of segments that overlap."""
    S = synth
    w, g = femto_amd.doclist_info()
    C = _cus()
    rng = np.random.default_rng(6)
    firsts = np.concatenate([[0], S.ends[:-1]])
    every_doc = np.concatenate([firsts, S.ends - 1])
    edges = [w + 1, 127, 128, 129, 255, 256, 257, 1000, g - 1, g]
    segs, touches_all = [], []
    for k in range(2 * 8 * C + 301):
        n = int(rng.choice(edges)) if k % 2 == 0 else int(rng.integers(w + 1, 401))
        if n >= 700:
            touches_all.append(len(segs))
        segs.append(_distinct(rng, S.N, n, () if n < 700 else every_doc if n >= len(every_doc) else firsts))
        if k % 20 == 7:
            segs.append([])
        if k % 20 == 17:
            segs.append(_distinct(rng, S.N, int(rng.integers(1, w + 1))))
    sizes = np.array([len(s) for s in segs])
    assert ((sizes > w) & (sizes <= g)).sum() > 2 * 8 * C and not (sizes > g).any()
    assert (sizes == 0).sum() > 100 and ((sizes > 0) & (sizes <= w)).sum() > 100 and set(edges) <= set(sizes.tolist())
    assert len(segs) > 2 * 1024
    want = _list_segments(S, segs, ("mid segments",))
    assert (want.ndocs[touches_all] == 700).all() and len(touches_all) > 100


def test_big_segment_of_more_than_256_tiles(synth):
    """A segment of more than 256 tiles (a tile is workgroup_max rows): the workgroups of its last tiles add the heads of the
    tiles in front in more than one trip, and doclist_tiles_kernel maps its tiles in more than one; a second segment of several
    tiles beside it, so that one of the two does not start at tile 0.  The large one holds every text position at least once
    and random repeats (the file's docstring)."""
    S = synth
    w, g = femto_amd.doclist_info()
    rng = np.random.default_rng(16)
    N = S.N
    n1, n2 = 257 * g + 5, 3 * g + 1
    firsts = np.concatenate([[0], S.ends[:-1]])
    big1 = rng.permutation(np.concatenate([np.arange(N, dtype=np.int64), rng.integers(0, N, n1 - N)]))
    big2 = rng.permutation(np.concatenate([firsts, rng.integers(0, N, n2 - len(firsts))]))
    segs = [_distinct(rng, N, 5), [], big1, [0], big2, _distinct(rng, N, w + 1), []]
    assert len(big1) == n1 and len(big2) == n2 and -(-n1 // g) > 257
    d = du.resolve(S.ends, np.sort(big1))[0]
    heads = np.concatenate([[True], d[1:] != d[:-1]])
    assert heads[256 * g:257 * g].any() and heads[:g].any()          # the 257th tile has heads for the 258th to add in a second trip
    want = _list_segments(S, segs, ("more than 256 tiles",))
    assert want.ndocs[2] == 700 and want.ndocs[4] == 700


def test_documents_host_form_beyond_one_pass(synth):
    """femto_amd_doclist (the host form) over more located rows than two passes of doclist_pack_kernel's grid hold"""
    S = synth
    grams = _grams()
    occ = [_occurrences(S.text, p) for p in grams]
    need = 2 * 256 * 8 * _cus()
    reps = need // sum(len(o) for o in occ) + 1
    out_starts = np.concatenate([[0], np.cumsum([len(o) for o in occ] * reps, dtype=np.int64)])
    assert out_starts[-1] > need
    want = du.listing(S.ends, np.concatenate(occ * reps), out_starts)
    pats = [np.frombuffer(p, dtype=np.uint8).astype(np.uint16) + 5 for p in grams] * reps
    ds, docs, hits = S.ix.documents(pats, 1 << 20)
    wds, wdocs, whits = du.packed(want, out_starts)
    assert wds[-1] > 700 * reps
    assert np.array_equal(ds, wds) and np.array_equal(docs, wdocs) and np.array_equal(hits, whits)


# ---- 3. search end to end -----------------------------------------------------------------------------------------------------

def _occurrences(text, pat):
    """every text position where the byte string pat stands (it never holds the SEOF's 0: a match stays inside a document)"""
    p = np.frombuffer(pat, dtype=np.uint8)
    ok = np.ones(len(text) - len(p) + 1, dtype=bool)
    for j, c in enumerate(p):
        ok &= text[j:j + len(ok)] == c
    return np.flatnonzero(ok).astype(np.int64)


@pytest.mark.parametrize("mo", [1 << 20, 5])
def test_search_end_to_end(synth, searched, mo):
    S = synth
    L, out_starts, offs, noccs = searched[mo]
    grams = _grams()
    located = []
    for i, p in enumerate(grams):
        occ = _occurrences(S.text, p)
        got = np.sort(offs[out_starts[i]:out_starts[i + 1]])
        if len(occ) - 1 > mo:                       # the reference's clamp (server.c:4411): exactly mo rows of the range
            assert len(got) == mo and np.isin(got, occ).all(), (p, mo)
        else:
            assert np.array_equal(got, occ), (p, mo)
        located.append(got)
    assert not len(located[-1]) and not len(located[-2])
    # brute force, restricted to the located rows: the documents holding them, and how many each holds
    want_starts = np.concatenate([[0], np.cumsum([len(x) for x in located], dtype=np.int64)])
    assert np.array_equal(want_starts, out_starts)
    want = du.listing(S.ends, np.concatenate(located), out_starts)
    if mo == 1 << 20:
        for i, p in enumerate(grams):               # the scan document by document, without doc_ends
            holds = np.array([d.tobytes().count(p) if len(p) == 1 else sum(d.tobytes().startswith(p, k) for k in range(len(d))) for d in S.docs])
            s = int(out_starts[i])
            assert np.array_equal(want.docs[s:s + want.ndocs[i]], np.flatnonzero(holds)), p
            assert np.array_equal(want.hits[s:s + want.ndocs[i]], holds[holds > 0]), p
    L.check(want, out_starts, ("search", mo))
    ds, docs, hits = S.ix.documents(S.pats, mo)
    wds, wdocs, whits = du.packed(want, out_starts)
    assert np.array_equal(ds, wds) and np.array_equal(docs, wdocs) and np.array_equal(hits, whits)


# ---- 4. liveness ----------------------------------------------------------------------------------------------------------------

def test_liveness(synth):
    import torch
    S = synth
    out_starts = np.array([0, 3, 3, 100, 5000], dtype=np.int64)
    offs = np.random.default_rng(1).integers(0, S.N, 5000)
    for total in ([5000, 1], [5001, 0], [9000, 1]):         # flagged as overflow; more rows than the buffer holds; both
        L = Lists(4, 5000)
        L.call(S.ix, _t(out_starts), _t(offs), 5000, _t(np.array(total, dtype=np.int64)))
        torch.cuda.synchronize()
        assert L.untouched(), total
        assert int(L.status[0]) == 1, total
    L = Lists(0, 5000)
    L.call(S.ix, _t(out_starts[:1]), _t(offs), 5000, _t(np.array([0, 0], dtype=np.int64)))
    torch.cuda.synchronize()
    assert L.untouched(but_status=False)
    # and alive again: the same buffers, the flag cleared
    L = Lists(4, 5000)
    L.call(S.ix, _t(out_starts), _t(offs), 5000, _t(np.array([5000, 0], dtype=np.int64)))
    torch.cuda.synchronize()
    L.check(du.listing(S.ends, offs, out_starts), out_starts, ("alive",))


# ---- 5. set operations ----------------------------------------------------------------------------------------------------------

def _run_docset(ix, flat, a_start, a_n, b_start, b_n, ops, cap, guard=0):
    """one femto_amd_docset_device call: (res_starts, res_docs, res_total); res_docs holds `guard` entries behind cap"""
    import torch
    n = len(ops)
    d_flat = _t(flat)
    rs = torch.full((n + 1,), SENT, dtype=torch.int64, device=DEV)
    rd = torch.full((max(cap + guard, 1),), SENT, dtype=torch.int64, device=DEV)
    rt = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
    d_as, d_an, d_bs, d_bn, d_op = _t(a_start), _t(a_n), _t(b_start), _t(b_n), _t(ops)      # (alive until the synchronise)
    ix.docset_device(n, d_flat.data_ptr(), d_as.data_ptr(), d_an.data_ptr(), d_flat.data_ptr(), d_bs.data_ptr(), d_bn.data_ptr(),
                     d_op.data_ptr(), rs.data_ptr(), rd.data_ptr() if cap else 0, cap, rt.data_ptr())
    torch.cuda.synchronize()
    return rs.cpu().numpy(), rd.cpu().numpy(), rt.cpu().tolist()


def test_set_operations(synth, searched):
    S = synth
    w, g = femto_amd.doclist_info()
    rng = np.random.default_rng(11)
    L, out_starts, _, _ = searched[1 << 20]
    ndocs, docs = L.ndocs.cpu().numpy(), L.docs.cpu().numpy()
    lists = [docs[out_starts[i]:out_starts[i] + ndocs[i]] for i in range(len(ndocs))]                # case 3's lists (two of them empty)
    uni = 400000

    def rand(n):
        return np.sort(rng.choice(uni, n, replace=False)).astype(np.int64)

    for n in (0, 1, w - 1, w + 1, g - 1, g + 1, 50000):
        lists.append(rand(n))
    base = len(lists) - 7
    big = lists[-1]
    lists += [big[::2].copy(), big[1::2].copy(), big[1000:3000].copy(), big + uni, lists[base + 4][::3].copy(),      # interleaved halves, nested, disjoint
              np.setdiff1d(np.arange(2 * g, dtype=np.int64), lists[base + 4])]
    # the named shapes first, then random pairs up to 2000
    ia, ib = [], []
    k = len(lists)
    for x in range(base, k):
        ia += [x, x, base, x]                           # identical; with the empty list on either side; with the single-element list
        ib += [x, base, x, base + 1]
    nested = [(k - 6, k - 7), (k - 7, k - 6), (k - 5, k - 7), (k - 7, k - 5), (k - 4, k - 7), (k - 7, k - 4), (k - 6, k - 5), (k - 7, k - 3), (k - 2, base + 4), (base + 4, k - 2),
              (base + 4, k - 1), (k - 1, base + 4)]
    ia += [p[0] for p in nested]
    ib += [p[1] for p in nested]
    more = 2000 - len(ia)
    small = np.concatenate([np.arange(base), np.arange(base, base + 6)])      # (the 50 000-element lists only in the named pairs)
    ia += rng.choice(small, more).tolist()
    ib += rng.choice(small, more).tolist()
    ia, ib = np.array(ia), np.array(ib)
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    lstart = np.concatenate([[0], np.cumsum(lens)])[:-1]
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])
    a_start, b_start = lstart[ia], lstart[ib]
    a_n, b_n = lens[ia].astype(np.int32), lens[ib].astype(np.int32)
    for op in (du.AND, du.OR, du.NOT, None):
        ops = np.full(len(ia), op, dtype=np.int32) if op is not None else rng.integers(0, 3, len(ia)).astype(np.int32)
        ws, wd = du.setops([lists[x] for x in ia], [lists[x] for x in ib], ops)
        tot = int(ws[-1])
        rs, rd, rt = _run_docset(S.ix, flat, a_start, a_n, b_start, b_n, ops, tot + 8)
        assert rt == [tot, 0], op
        assert np.array_equal(rs, ws), op
        assert np.array_equal(rd[:tot], wd), op
        assert (rd[tot:] == SENT).all(), op
        # one short: the flag, the needed size, complete starts, nothing behind the buffer
        rs, rd, rt = _run_docset(S.ix, flat, a_start, a_n, b_start, b_n, ops, tot - 1)
        assert rt == [tot, 1] and np.array_equal(rs, ws), op
        assert np.array_equal(rd[:tot - 1], wd[:tot - 1]), op
        if op is None:
            hs, hd = S.ix.docset([lists[x] for x in ia], [lists[x] for x in ib], ops)
            assert np.array_equal(hs, ws) and np.array_equal(hd, wd)
    hs, hd = S.ix.docset([], [], [])
    assert hs.tolist() == [0] and len(hd) == 0


def test_more_pairs_than_workgroups(synth):
    """more pairs than docset_kernel has workgroups: every workgroup takes a second pair, some a third"""
    S = synth
    C = _cus()
    rng = np.random.default_rng(17)
    npairs = 2 * 8 * C + 37
    assert npairs > 2 * 8 * C
    lens = [int(rng.choice([0, 1, 255, 256, 257, 600])) if k % 2 else int(rng.integers(0, 301)) for k in range(300)]
    assert set([0, 1, 255, 256, 257, 600]) <= set(lens)
    lists = [np.sort(rng.choice(1500, n, replace=False)).astype(np.int64) for n in lens]
    ia, ib = rng.integers(0, 300, npairs), rng.integers(0, 300, npairs)
    ops = rng.integers(0, 3, npairs).astype(np.int32)
    lens = np.array(lens, dtype=np.int64)
    lstart = np.concatenate([[0], np.cumsum(lens)])[:-1]
    flat = np.concatenate(lists)
    a_start, b_start = lstart[ia], lstart[ib]
    a_n, b_n = lens[ia].astype(np.int32), lens[ib].astype(np.int32)
    ws, wd = du.setops([lists[x] for x in ia], [lists[x] for x in ib], ops)
    tot = int(ws[-1])
    sizes = np.diff(ws)
    assert all((sizes[ops == op] > 0).sum() > 100 for op in (du.AND, du.OR, du.NOT))
    rs, rd, rt = _run_docset(S.ix, flat, a_start, a_n, b_start, b_n, ops, tot + 8)
    assert rt == [tot, 0]
    assert np.array_equal(rs, ws)
    assert np.array_equal(rd[:tot], wd)
    assert (rd[tot:] == SENT).all()
    # one short: the flag, the needed size, complete starts, nothing behind the buffer
    rs, rd, rt = _run_docset(S.ix, flat, a_start, a_n, b_start, b_n, ops, tot - 1, GUARD)
    assert rt == [tot, 1] and np.array_equal(rs, ws)
    assert np.array_equal(rd[:tot - 1], wd[:tot - 1]) and (rd[tot - 1:] == SENT).all()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------

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
        L = Lists(1, 8)
        z = torch.zeros(8, dtype=torch.int64, device=DEV)
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            L.call(a, z, z, 8, z)
        assert e.value.code == 6
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            a.docset_device(1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                            z.data_ptr(), 8, z.data_ptr())
        assert e.value.code == 6
        assert L.untouched(but_status=False)
    finally:
        a.close()
        b.close()
