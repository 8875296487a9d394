"""`-m gpu`: extraction (femto_amd/extract/extract.hip) where the golden fixtures do not reach: on two corpora of hundreds of tiny
and empty documents built here (tests/corpus_util.py: "edges", two-level lines, and "dna", packed 3-bit lines), at both ends of the
sample-shift range, on femto's own tables (the leaf state machine) with many documents, with thousands of requests in one tile of
the copy, with both persistent loops taken more than twice, and through the device forms with odd slots, guards and every edge of
d_n.  Every expectation comes from extract_util.TextRestated (numpy over the prepared text and its suffix array); the
preconditions that keep these cases from going hollow are asserted without a GPU in tests/test_extract_host.py."""
import numpy as np
import pytest

import corpus_util as cu
import femto_amd
from extract_util import TextRestated, all_empty_requests, crowded_requests, long_requests, random_requests

pytestmark = pytest.mark.gpu

# what extract.hip does not export, restated once
TILE_SYMS = 2048               # kTileSyms: the output symbols one workgroup of xcopy_kernel covers per turn
WORKGROUPS_PER_CU = 8          # host_common.hpp persistent_grid
WALK_LANES = 256               # the pieces one workgroup of xwalk_kernel covers per turn

DEV = "cuda:0"
GUARD = 0x0909

EDGES_KINDS = ["default", "samples0", "samples1", "samples3", "samples6", "samples16", "no_text", "wave0", "wave6"]
DNA_KINDS = ["default", "samples0", "samples3", "samples6", "samples16", "no_text"]
ALL_KINDS = [("edges", k) for k in EDGES_KINDS] + [("dna", k) for k in DNA_KINDS]
MODE = {"edges": 4, "dna": 3}


def _ids(pairs):
    return ["%s-%s" % p for p in pairs]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the two indexes and their expectations, once ---------------------------------------------------------------------------

class _Built:
    pass


@pytest.fixture(scope="module")
def corpora(tmp_path_factory, gpu_ok):
    out = {}
    for name, docs in (("edges", cu.edges_docs()), ("dna", cu.dna_docs())):
        C = _Built()
        C.name, C.docs = name, docs
        C.index = str(tmp_path_factory.mktemp(name) / "index")
        femto_amd.build_index(C.index, docs, params=None, infos=["%s%d" % (name[0], i) for i in range(len(docs))], device=0)
        C.R = TextRestated(docs)
        C.cache = {}
        out[name] = C
    return out


def _windows(C, before, after):
    """context_window of EVERY position, computed once per corpus and pair and left unchanged"""
    key = ("win", before, after)
    if key not in C.cache:
        w = C.R.context_window(np.arange(C.R.N, dtype=np.int64), before, after)
        w.setflags(write=False)
        C.cache[key] = w
    return C.cache[key]


def _batches(C):
    """the four request batches and TextRestated.extract of them"""
    if "batches" not in C.cache:
        N = C.R.N
        made = {"random": random_requests(N, 41), "crowded": crowded_requests(N, 42), "all_empty": all_empty_requests(N, 43),
                "long": long_requests(N, 44)}
        C.cache["batches"] = {k: (pos, lens, C.R.extract(pos, lens)) for k, (pos, lens) in made.items()}
    return C.cache["batches"]


def _open(C, kind):
    """(ix, ex) of one kind; the rank mode, the path and the shift are asserted here for every test"""
    options = dict(text=0) if kind == "no_text" else (dict(rank_mode=1) if kind.startswith("wave") else None)
    ix = femto_amd.Index(C.index, device=0, options=options) if options else femto_amd.Index(C.index, device=0)
    try:
        forced = kind.startswith("samples") or kind.startswith("wave")
        shift = int("".join(c for c in kind if c.isdigit())) if forced else -1
        assert ix.rank_mode == (1 if kind.startswith("wave") else MODE[C.name]), (C.name, kind, ix.rank_mode)
        assert ix.info.number_of_documents == len(C.docs) and ix.info.total_length == C.R.N          # the empty documents are there
        ex = ix.extractor(shift, forced)
        info = ex.info()
        assert info["path"] == (ex.PATH_TEXT if kind == "default" else ex.PATH_SAMPLES), (C.name, kind, info)
        if forced:
            assert info["sample_shift"] == shift, (C.name, kind, info)
        elif kind == "no_text":
            assert info["sample_shift"] == 6, (C.name, kind, info)
    except BaseException:
        ix.close()
        raise
    return ix, ex


def _same(got, want, *what):
    """equal arrays, or the failure names `what` and the first differing indexes"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what + (got.shape, want.shape)
    if not np.array_equal(got, want):
        raise AssertionError(what + (np.argwhere(got != want)[:6].tolist(),))


# ---- documents and SEOF rows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus,kind", ALL_KINDS, ids=_ids(ALL_KINDS))
def test_every_document_and_eof_row(corpora, corpus, kind):
    """xsample_scatter_kernel's eof[D.doc] = row for hundreds of documents, empty ones among them (two SEOFs in neighbouring
    positions); every document by extract_document, an empty one being its SEOF alone"""
    C = corpora[corpus]
    R = C.R
    ix, ex = _open(C, kind)
    try:
        if kind != "default":
            _same(ex.eof_rows(), R.eof_rows, corpus, kind, "eof_rows")
        for d in range(len(C.docs)):
            doc = ex.extract_document(d)
            assert len(doc) == len(C.docs[d]) + 1, (corpus, kind, d, len(doc))
            _same(doc, R.document(d), corpus, kind, "document", d)
    finally:
        ix.close()


# ---- requests -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus,kind", ALL_KINDS, ids=_ids(ALL_KINDS))
def test_requests(corpora, corpus, kind):
    """xcopy_kernel's s_r[0..1] and first_gt with thousands of requests of 0, 1 or 2 symbols in one tile and runs of hundreds of
    empty ones ("crowded"), a total of 0 ("all_empty"), requests of dozens of tiles ("long"); walk_begin through every document
    end of the text in one request"""
    C = corpora[corpus]
    ix, ex = _open(C, kind)
    try:
        for name, (pos, lens, want) in _batches(C).items():
            got = ex.extract(pos, lens)
            _same(got, want, corpus, kind, name, "packed")
            if name == "all_empty":
                assert len(got) == 0
            starts = np.cumsum(np.concatenate([[3], lens[:-1].astype(np.int64) + 5]))
            got = ex.extract(pos, lens, out_starts=starts)
            slots = np.zeros_like(got)
            for s, w in zip(starts, np.split(want, np.cumsum(lens.astype(np.int64))[:-1])):
                slots[s:s + len(w)] = w
            _same(got, slots, corpus, kind, name, "out_starts")
    finally:
        ix.close()


# ---- contexts -----------------------------------------------------------------------------------------------------------------

def _near_ends(R):
    """the 2 000 positions nearest a document's SEOF and 1 000 seeded ones"""
    p = np.arange(R.N, dtype=np.int64)
    eof = R.doc_ends - 1
    k = np.searchsorted(eof, p)          # eof[k] >= p: the anchor's own SEOF; eof[k - 1]: the one in front of its document
    dist = np.minimum(eof[k] - p, np.where(k > 0, p - eof[np.maximum(k - 1, 0)], R.N))
    near = np.argsort(dist, kind="stable")[:2000]
    return np.unique(np.concatenate([near, np.random.default_rng(20250716).integers(0, R.N, 1000)])).astype(np.int64)


@pytest.mark.parametrize("corpus,kind", ALL_KINDS, ids=_ids(ALL_KINDS))
def test_context_every_position(corpora, corpus, kind):
    """xcontext_plan_kernel's window for an anchor in every document and on every SEOF, xcopy_kernel's fast and slow path
    alternating within a request (the windows are mostly outside [vlo, vhi)), the walk of every row's context"""
    C = corpora[corpus]
    R = C.R
    ix, ex = _open(C, kind)
    try:
        rows = np.arange(R.N, dtype=np.int64)
        p = R.sa
        for before, after in ((0, 0), (0, 1), (1, 0), (7, 7), (3, 200), (64, 1)):
            want = _windows(C, before, after)[p]
            ctx, pos = ex.context(rows=rows, before=before, after=after)
            _same(pos, p, corpus, kind, (before, after), "rows form: pos_out")
            _same(ctx, want, corpus, kind, (before, after), "rows form")
            ctx, pos = ex.context(offsets=p, before=before, after=after)
            _same(pos, p, corpus, kind, (before, after), "offsets form: pos_out")
            _same(ctx, want, corpus, kind, (before, after), "offsets form")
        a = _near_ends(R)
        if "far" not in C.cache:
            C.cache["far"] = R.context_window(a, 2047, 2047)
        ctx, pos = ex.context(offsets=a, before=2047, after=2047)
        _same(pos, a, corpus, kind, (2047, 2047), "offsets form: pos_out")
        _same(ctx, C.cache["far"], corpus, kind, (2047, 2047), "offsets form")
        ctx, pos = ex.context(rows=R.isa[a], before=2047, after=2047)
        _same(pos, a, corpus, kind, (2047, 2047), "rows form: pos_out")
        _same(ctx, C.cache["far"], corpus, kind, (2047, 2047), "rows form")
        # out of range: pos_out = -1 and zeros; the anchors around them are served
        bad = np.array([5, -1, R.N, 1 << 62, -(1 << 62), R.N - 1], dtype=np.int64)
        for form in ("rows", "offsets"):
            ctx, pos = ex.context(before=7, after=7, **{form: bad})
            at = bad[[0, 5]] if form == "offsets" else R.sa[bad[[0, 5]]]
            _same(pos, [at[0], -1, -1, -1, -1, at[1]], corpus, kind, form, "out of range: pos_out")
            assert not ctx[1:5].any(), (corpus, kind, form)
            _same(ctx[[0, 5]], _windows(C, 7, 7)[at], corpus, kind, form, "beside the anchors out of range")
    finally:
        ix.close()


def _pieces(R, before, after, shift):
    """the pieces of every position's context on the sample path: the blocks of 2^shift that [p - before, p + after), clamped to
    the anchor's document (the SEOF in front of it is the copy's, not the walk's, when it is position -1), spans"""
    p = np.arange(R.N, dtype=np.int64)
    d = np.searchsorted(R.doc_ends, p, side="right")
    ds = np.where(d > 0, R.doc_ends[np.maximum(d - 1, 0)], 0)
    lo = np.maximum(np.maximum(p - before, ds - 1), 0)
    hi = np.minimum(p + after, R.doc_ends[d])
    return int(np.where(hi > lo, ((hi - 1) >> shift) - (lo >> shift) + 1, 0).sum())


@pytest.mark.parametrize("kind", ["default", "samples3"])
def test_persistent_loops_go_round_twice(corpora, kind):
    """xcopy_kernel's loop over 8 x CUs workgroups of 2048 symbols and xwalk_kernel's over 8 x CUs x 256 pieces, each taken more
    than twice by one call: the context of every row"""
    import torch
    C = corpora["edges"]
    R = C.R
    grid = WORKGROUPS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    W = 160
    while R.N * W <= 2 * grid * TILE_SYMS or (kind == "samples3" and _pieces(R, W // 2, W // 2, 3) <= 2 * grid * WALK_LANES):
        W += 32
        assert W <= 4094, (grid, W)
    before = after = W // 2
    assert R.N * W > 2 * grid * TILE_SYMS
    if kind == "samples3":
        assert _pieces(R, before, after, 3) > 2 * grid * WALK_LANES
    ix, ex = _open(C, kind)
    try:
        want = _windows(C, before, after)[R.sa]
        ctx, pos = ex.context(rows=np.arange(R.N, dtype=np.int64), before=before, after=after)
        _same(pos, R.sa, kind, (before, after), "pos_out")
        _same(ctx, want, kind, (before, after), "rows form")
    finally:
        ix.close()


# ---- the device forms ---------------------------------------------------------------------------------------------------------

DEVICE_KINDS = [("edges", "default"), ("edges", "samples3"), ("edges", "wave6"), ("dna", "default"), ("dna", "samples3")]


@pytest.mark.parametrize("corpus,kind", DEVICE_KINDS, ids=_ids(DEVICE_KINDS))
def test_device_forms(corpora, corpus, kind):
    """femto_amd_extract_device into slots with 3-symbol gaps that begin at odd and even symbols of a 16-byte aligned buffer and of
    that buffer + 1 symbol (xcopy_kernel's scalar branch beside the uint4 store), negative lengths (xprep_kernel: 0);
    femto_amd_context_device with d_n = 0, 1, n - 1, n, n + 5 and -1 in both forms: exact inside, the guard everywhere else"""
    import torch
    C = corpora[corpus]
    R = C.R
    ix, ex = _open(C, kind)
    try:
        # extract_device
        pos, lens = random_requests(R.N, seed=45, n=300)
        lens = lens.copy()
        lens[[2, 4, 90, 200, len(lens) - 1]] = (-3, -1, -7, -(1 << 31), -1)
        live = lens.clip(0)
        starts = 1 + np.concatenate([[0], np.cumsum(live[:-1].astype(np.int64) + 3)])
        end = int(starts[-1] + live[-1])
        assert starts[0] % 2 == 1 and live[0] >= 16 and (starts % 2 == 0).any() and (starts % 8 == 0).any() and (live >= 16).sum() > 100
        pieces = np.split(R.extract(pos, live), np.cumsum(live.astype(np.int64))[:-1])
        d_pos, d_len, d_st = _t(pos), _t(lens), _t(starts)
        for shifted in (0, 1):
            base = torch.full((end + 32,), GUARD, dtype=torch.int16, device=DEV)
            assert base.data_ptr() % 16 == 0
            ex.extract_device(len(pos), d_pos.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), base.data_ptr() + 2 * shifted)
            torch.cuda.synchronize()
            want = np.full(end + 32, GUARD, dtype=np.uint16)
            for s, w in zip(starts, pieces):
                want[shifted + s:shifted + s + len(w)] = w
            _same(base.cpu().numpy().view(np.uint16), want, corpus, kind, "extract_device", "d_out + %d" % shifted)
        # context_device
        rng = np.random.default_rng(46)
        a = np.concatenate([rng.integers(0, R.N, 600), R.doc_ends[:90] - 1, [0, R.N - 1]]).astype(np.int64)
        a = a[rng.permutation(len(a))]
        a[[3, 300]] = (-1, R.N)
        n, before, after = len(a), 5, 9
        ok = (a >= 0) & (a < R.N)
        for form in ("offsets", "rows"):
            p = np.where(ok, a if form == "offsets" else R.sa[np.where(ok, a, 0)], -1)
            want_ctx = np.where(ok[:, None], _windows(C, before, after)[np.where(ok, p, 0)], 0).astype(np.uint16)
            d_a = _t(a)
            for live_n in (0, 1, n - 1, n, n + 5, -1):
                m = min(n, max(live_n, 0))
                d_n = torch.tensor([live_n], dtype=torch.int64, device=DEV)
                d_ctx = torch.full((n + 3, before + after), GUARD, dtype=torch.int16, device=DEV)
                d_out = torch.full((n + 3,), -5, dtype=torch.int64, device=DEV)
                ex.context_device(n, d_n=d_n.data_ptr(), before=before, after=after, d_ctx=d_ctx.data_ptr(), d_pos_out=d_out.data_ptr(),
                                  **{"d_" + form: d_a.data_ptr()})
                torch.cuda.synchronize()
                got, got_pos = d_ctx.cpu().numpy().view(np.uint16), d_out.cpu().numpy()
                _same(got[:m], want_ctx[:m], corpus, kind, form, "d_n = %d" % live_n, "ctx")
                _same(got_pos[:m], p[:m], corpus, kind, form, "d_n = %d" % live_n, "pos_out")
                assert (got[m:] == GUARD).all(), (corpus, kind, form, live_n, m + np.argwhere(got[m:] != GUARD)[:6])
                assert (got_pos[m:] == -5).all(), (corpus, kind, form, live_n, m + np.nonzero(got_pos[m:] != -5)[0][:6])
    finally:
        ix.close()


# ---- the wrap to T[N - 1] and empty neighbours ----------------------------------------------------------------------------------

def _hand_listed(C):
    R = C.R
    eof = R.doc_ends - 1
    first = eof[:-1][np.diff(eof) == 1]          # the first SEOF of every pair of neighbours
    ends = [0, 1, 2] if C.name == "edges" else [R.N - 3, R.N - 2, R.N - 1]
    a = np.unique(np.concatenate([ends, first, first + 1, first + 2])).astype(np.int64)
    return a[a < R.N]


@pytest.mark.parametrize("corpus,kind", ALL_KINDS, ids=_ids(ALL_KINDS))
def test_wrap_and_empty_neighbours(corpora, corpus, kind):
    """vlo = D.start - 1 where it is the SEOF of an empty document, where it is -1 (T[N - 1]) and where the anchor IS the SEOF of an
    empty document: against the stepping restatement, not the window"""
    C = corpora[corpus]
    R = C.R
    a = _hand_listed(C)
    assert len(a) >= 30
    if corpus == "edges":
        assert len(C.docs[0]) == 0 and R.T[0] == 2 and a[:3].tolist() == [0, 1, 2]
    else:
        assert len(C.docs[-1]) == 0 and R.T[-1] == 2 and R.T[-2] == 2 and a[-3:].tolist() == [R.N - 3, R.N - 2, R.N - 1]
    ix, ex = _open(C, kind)
    try:
        for before, after in ((1, 1), (2, 2), (9, 9)):
            want = np.stack([R.context_text(int(p), before, after) for p in a])
            ctx, pos = ex.context(offsets=a, before=before, after=after)
            _same(pos, a, corpus, kind, (before, after), "offsets form: pos_out")
            _same(ctx, want, corpus, kind, (before, after), "offsets form")
            ctx, pos = ex.context(rows=R.isa[a], before=before, after=after)
            _same(pos, a, corpus, kind, (before, after), "rows form: pos_out")
            _same(ctx, want, corpus, kind, (before, after), "rows form")
    finally:
        ix.close()
