"""`-m gpu`: matching lines (femto_amd/lines/lines.hip) and common sequences (femto_amd/similar/similar.hip) where the golden
fixtures do not reach: on two corpora of hundreds of documents built here (tests/corpus_util.py: "edges" and "library"), past one
chunk and one piece of the sample path's host loops, into an unaligned destination, and on matches as long as the cap.  Every
expectation comes from tests/lines_util.py, tests/similar_util.py, the CPU oracle or a closed form stated at the test; the
preconditions that keep these cases from going hollow are asserted without a GPU in tests/test_lines_host.py and
tests/test_similar_host.py.  (The one case that needs 2^26 bytes of lines stands in tests/test_gpu_fullsize.py.)"""
import numpy as np
import pytest

import corpus_util as cu
import femto_amd
from lines_util import BINARY, INVALID, Lines, group_first
from oracle import pyoracle
from similar_util import Text, document_scores, groups_of, index_numerator, match_lengths, ranked
from test_gpu_lines import KINDS, _open as _open_kind
from test_gpu_similar import OPTION_SETS, _chain, _open_set

pytestmark = pytest.mark.gpu

# what lines.hip does not export, restated once
CHUNK_ANCHORS = 65536          # lines.hip:36 kChunkAnchors: the anchors of one round of run_bounds' loop on the sample path
PIECE_SYMS = 1 << 26           # lines.hip:37 kChunkSyms: the symbols of one round of run_bytes' loop on the sample path
ROUND = 256                    # lines.hip:35 kRound: the positions a group of lanes looks at per direction and round
GROUP_LANES = 16               # lines.hip:5, :406 (groups_of): the lanes of one anchor, and lines.hip:213 the bytes of one thread
TILE_BYTES = 4096              # lines.hip:214 kTileBytes: the output bytes one workgroup of lines_copy_kernel covers per turn
MAX_PATTERN = 32768            # similar.hip:51 kMaxPattern

DEV = "cuda:0"


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the two indexes ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edges(tmp_path_factory, gpu_ok):
    docs = cu.edges_docs()
    E = cu.Corpus(docs, str(tmp_path_factory.mktemp("edges") / "index"))
    femto_amd.build_index(E.index, docs, params=None, infos=["e%d" % i for i in range(len(docs))], device=0)
    E.L = L = Lines(E)
    E.flags = L.binary.astype(np.uint8) * BINARY
    E.starts, E.data = L.packed(L.pos, L.len)                 # every anchor's line, computed once and left unchanged
    E.group_first, E.ngroups = group_first(E.starts, E.data, E.flags)
    return E


@pytest.fixture(scope="module")
def library(tmp_path_factory, gpu_ok):
    lib = cu.library_docs()
    lib.index = str(tmp_path_factory.mktemp("library") / "index")
    femto_amd.build_index(lib.index, lib.docs, params=None, infos=["l%d" % i for i in range(len(lib.docs))], device=0)
    lib.text = t = Text(lib.docs)
    lib.q = np.frombuffer(cu.library_query(lib), dtype=np.uint8)
    lib.lens = match_lengths(t, lib.q)
    lib.seqs, lib.groups, lib.group_of = groups_of(lib.q, lib.lens)
    lib.hits_of = lambda g: t.hits(g.bytes)
    lib.rows = sum(len(t.occurrences(g.bytes)) for g in lib.groups)
    return lib


# ---- 2. lines on "edges" --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_every_anchor_of_edges(edges, kind):
    """lines_bounds_kernel (both sources) where doc_of searches 816 documents, a group's 16 lanes, a round of 256 positions and
    the 2047-symbol contexts hold dozens of documents and SEOFs, documents are empty or one byte, and a terminator (\\n, \\r, \\0)
    stands exactly 255 .. 1024 positions from the anchor; lines_copy_kernel / lines_piece_kernel over 38 MB of such lines; the
    groups of all of them with the full hash and with 3 bits of it (lines_heads_kernel, lines_collide_kernel)"""
    L = edges.L
    ix, ex = _open_kind(edges, kind)
    try:
        assert ix.info.number_of_documents == len(edges.docs) and ix.info.total_length == L.N          # the empty documents are there
        assert ex.info()["path"] == (ex.PATH_TEXT if kind == "default" else ex.PATH_SAMPLES)
        assert L.N < CHUNK_ANCHORS          # (one chunk: the chunk loop is test_anchors_past_one_chunk's)
        doc, pos, lens, flags, starts, data = ex.lines(np.arange(L.N, dtype=np.int64))
        for name, got, want in (("doc", doc, L.doc), ("pos", pos, L.pos), ("len", lens, L.len), ("flags", flags, edges.flags),
                                ("byte_starts", starts, edges.starts)):
            assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
        assert np.array_equal(data, edges.data)
        for bits in (0, 3):
            gf, ng = ex.line_groups(starts, data, flags, hash_bits=bits)
            assert np.array_equal(gf, edges.group_first) and ng == edges.ngroups, bits
    finally:
        ix.close()


def _sample_of_lines(edges, n, seed):
    L = edges.L
    a = np.random.default_rng(seed).integers(0, L.N, n).astype(np.int64)
    wdoc, wpos, wlen, wflags = L.answer(a)
    wstarts, wdata = L.packed(wpos, wlen)
    return a, wpos, wlen, wflags, wstarts, wdata


@pytest.mark.parametrize("kind,offsets,grouped", [("default", range(16), (0, 1, 7, 8, 15)), ("samples3", (1, 8), (1, 8))])
def test_unaligned_destination(edges, kind, offsets, grouped):
    """lines_copy_kernel's second branch: 16 single bytes where `out + v0` is not 16-byte aligned (the text path; every fresh
    allocation takes the uint4 store); lines_narrow_kernel on the sample path; lines_hash_kernel's words rounded down from an
    address whose BASE is unaligned.  d_bytes = base + k: the bytes are exact and nothing outside [k, k + total) is written."""
    import torch
    a, wpos, wlen, wflags, wstarts, wdata = _sample_of_lines(edges, 3000, 31)
    n, total = len(a), int(wstarts[-1])
    assert total > 4 * TILE_BYTES and (wlen < GROUP_LANES).any() and (wlen > ROUND).any()
    wgf, wng = group_first(wstarts, wdata, wflags)
    assert wng < n          # equal lines at different places of the buffer
    ix, ex = _open_kind(edges, kind)
    try:
        d_pos, d_len, d_fl = _t(wpos), _t(wlen), _t(wflags)
        for k in offsets:
            base = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=DEV)
            assert base.data_ptr() % 16 == 0
            d_st = torch.full((n + 1,), -3, dtype=torch.int64, device=DEV)
            d_tot = torch.full((2,), -3, dtype=torch.int64, device=DEV)
            ex.line_bytes_device(n, d_pos.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), base.data_ptr() + k, total, d_tot.data_ptr())
            torch.cuda.synchronize()
            got = base.cpu().numpy()
            assert d_tot.cpu().tolist() == [total, 0] and np.array_equal(d_st.cpu().numpy(), wstarts), k
            assert np.array_equal(got[k:k + total], wdata), (k, np.nonzero(got[k:k + total] != wdata)[0][:8])
            assert (got[:k] == 0xEE).all() and (got[k + total:] == 0xEE).all(), k
            if k in grouped:
                d_gf = torch.full((n,), -9, dtype=torch.int64, device=DEV)
                d_ng = torch.full((1,), -9, dtype=torch.int64, device=DEV)
                ex.line_groups_device(n, d_st.data_ptr(), base.data_ptr() + k, d_gf.data_ptr(), d_ng.data_ptr(), d_flags=d_fl.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(d_gf.cpu().numpy(), wgf) and int(d_ng[0]) == wng, k
    finally:
        ix.close()


# ---- 3. the chunk and piece loops of the sample path ----------------------------------------------------------------------------

def test_anchors_past_one_chunk(edges):
    """run_bounds' loop over chunks of 65536 anchors taken three times: d_offsets and every output re-based by c0, the live count
    of chunk c from lines_chunk_live_kernel with the caller's count ending inside chunk 0, exactly at its end, one into chunk 1,
    exactly at the end of chunk 1, and at 0; an absent output stays absent in every chunk"""
    import torch
    L = edges.L
    n = 2 * CHUNK_ANCHORS + 17
    a = np.random.default_rng(77).integers(0, L.N, n).astype(np.int64)
    a[9], a[CHUNK_ANCHORS + 5], a[CHUNK_ANCHORS + 40000] = 1 << 62, -1, L.N           # out of range in every chunk
    a[2 * CHUNK_ANCHORS + 3], a[2 * CHUNK_ANCHORS + 16] = L.N + 7, -(1 << 40)
    wdoc, wpos, wlen, wflags = L.answer(a)
    assert int((wflags == INVALID).sum()) == 5
    for c in range(3):          # the three chunks hold different anchors and different answers
        assert not np.array_equal(wpos[c * CHUNK_ANCHORS:][:17], wpos[(c + 1) % 3 * CHUNK_ANCHORS:][:17])
    ix = femto_amd.Index(edges.index, device=0)
    try:
        ex = ix.extractor(3, True)
        assert ex.info()["path"] == ex.PATH_SAMPLES
        d_a = _t(a)
        for live in (None, CHUNK_ANCHORS - 1, CHUNK_ANCHORS, CHUNK_ANCHORS + 1, 2 * CHUNK_ANCHORS, 0):
            d_n = None if live is None else torch.tensor([live], dtype=torch.int64, device=DEV)
            d_doc, d_pos = torch.full((n,), -7, dtype=torch.int64, device=DEV), torch.full((n,), -7, dtype=torch.int64, device=DEV)
            d_len, d_fl = torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((n,), 77, dtype=torch.uint8, device=DEV)
            ex.lines_device(n, d_a.data_ptr(), 0 if live is None else d_n.data_ptr(), d_doc.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(),
                            d_fl.data_ptr())
            torch.cuda.synchronize()
            m = n if live is None else live
            for name, got, want, guard in (("doc", d_doc, wdoc, -7), ("pos", d_pos, wpos, -7), ("len", d_len, wlen, -7), ("flags", d_fl, wflags, 77)):
                got = got.cpu().numpy()
                assert np.array_equal(got[:m], want[:m]), (live, name, np.nonzero(got[:m] != want[:m])[0][:8])
                assert (got[m:] == guard).all(), (live, name, m + np.nonzero(got[m:] != guard)[0][:8])
        # two of the four outputs only
        d_pos, d_len = torch.full((n,), -7, dtype=torch.int64, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
        ex.lines_device(n, d_a.data_ptr(), d_line_pos=d_pos.data_ptr(), d_line_len=d_len.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_pos.cpu().numpy(), wpos) and np.array_equal(d_len.cpu().numpy(), wlen)
    finally:
        ix.close()


def test_capacity_past_one_piece(edges):
    """run_bytes' loop over pieces of 2^26 symbols runs by the CAPACITY: with 2^26 + 5 bytes of room and a few hundred lines the
    second piece is empty (lines_piece_kernel asks for nothing, lines_narrow_kernel stops at the total)"""
    import torch
    a, wpos, wlen, wflags, wstarts, wdata = _sample_of_lines(edges, 300, 32)
    n, total, cap = len(a), int(wstarts[-1]), PIECE_SYMS + 5
    assert 0 < total < PIECE_SYMS
    ix = femto_amd.Index(edges.index, device=0)
    try:
        ex = ix.extractor(3, True)
        assert ex.info()["path"] == ex.PATH_SAMPLES
        d_pos, d_len = _t(wpos), _t(wlen)
        d_by = torch.full((cap,), 0xEE, dtype=torch.uint8, device=DEV)
        d_st = torch.full((n + 1,), -3, dtype=torch.int64, device=DEV)
        d_tot = torch.full((2,), -3, dtype=torch.int64, device=DEV)
        ex.line_bytes_device(n, d_pos.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), d_by.data_ptr(), cap, d_tot.data_ptr())
        torch.cuda.synchronize()
        assert d_tot.cpu().tolist() == [total, 0] and np.array_equal(d_st.cpu().numpy(), wstarts)
        assert np.array_equal(d_by[:total].cpu().numpy(), wdata)
        assert bool((d_by[total:] == 0xEE).all())
    finally:
        ix.close()


# ---- 4. common sequences on "library" -------------------------------------------------------------------------------------------

def test_similar_on_many_documents(library):
    """femto_amd_similar where one sequence's hits are spread over up to 300 documents and a document collects up to a dozen
    sequences (doc_score_kernel's atomics on hundreds of slots), the ranking's ties fall to the smaller document, and every
    divisor is min(n, document length) = the document's length.  max_occs = 1000: no range reaches the clamp"""
    lib, t, q, groups = library, library.text, library.q, library.groups
    n = len(q)
    o = pyoracle.Oracle(lib.index)
    try:
        first, last = o.count([g.pattern for g in groups])
    finally:
        o.close()
    assert (last - first + 1).tolist() == [len(t.occurrences(g.bytes)) for g in groups]
    score, nseq = document_scores(len(t.docs), groups, lib.hits_of)
    want = ranked(t, n, score, nseq)
    ix = femto_amd.Index(lib.index, device=0)
    try:
        assert ix.info.number_of_documents == len(t.docs) and ix.info.total_length == t.total_length
        r = ix.similar(q, max_occs=1000)
        assert r.n == n and np.array_equal(r.len, lib.lens)
        assert r.g_len.tolist() == [g.len for g in groups] and r.g_here.tolist() == [g.here for g in groups]
        assert r.g_min_start.tolist() == [g.min_start for g in groups]
        assert np.array_equal(r.g_first, first) and np.array_equal(r.g_last, last) and r.g_kept.all()
        assert r.index_numerator == index_numerator(t, groups) and r.index_score == r.index_numerator / n
        got = list(zip(r.doc.tolist(), r.doc_numerator.tolist(), r.doc_seqs.tolist(), r.doc_score.tolist()))
        assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:4]
    finally:
        ix.close()


def test_similar_device_chain_on_many_documents(library):
    """the device calls back to back on a side stream: doc_plan_kernel with the offsets' capacity exact and one short (nothing is
    located, nothing scored, the total stays exact), doc_rows_kernel's keep mask"""
    import torch
    lib, t, q, groups = library, library.text, library.q, library.groups
    ns, ng, rows = len(lib.seqs), len(groups), lib.rows
    score, nseq = document_scores(len(t.docs), groups, lib.hits_of)
    ix = femto_amd.Index(lib.index, device=0)
    try:
        st = torch.cuda.Stream(device=DEV)
        assert st.cuda_stream != 0
        o = _chain(ix, q, st, max_occs=1000, off_cap=rows)
        assert np.array_equal(o["len"], lib.lens) and o["s_tot"].tolist() == [ns, 0]
        assert list(zip(o["s_start"][:ns].tolist(), o["s_len"][:ns].tolist())) == lib.seqs and o["group_of"][:ns].tolist() == lib.group_of
        assert o["ng"].tolist() == [ng, index_numerator(t, groups)]
        assert o["g_len"][:ng].tolist() == [g.len for g in groups] and o["g_here"][:ng].tolist() == [g.here for g in groups]
        assert o["tot"].tolist() == [rows, 0]
        assert np.array_equal(o["score"], score) and np.array_equal(o["seqs"], nseq)
        wantpos = np.sort([int(t.doc_starts[d]) + off for g in groups for d, off in t.occurrences(g.bytes)])
        assert np.array_equal(np.sort(o["offs"][:rows]), wantpos)          # every occurrence's text position
        o1 = _chain(ix, q, st, max_occs=1000, off_cap=rows - 1)
        assert o1["tot"].tolist() == [rows, 1] and not o1["score"].any() and not o1["seqs"].any()
        keep = np.zeros(len(q), dtype=np.uint8)
        keep[:ng:2] = 1
        ok = _chain(ix, q, st, max_occs=1000, keep=torch.from_numpy(keep).to(DEV))
        kscore, kseq = document_scores(len(t.docs), groups, lib.hits_of, kept=keep)
        assert kscore.any() and not np.array_equal(kscore, score)
        assert np.array_equal(ok["score"], kscore) and np.array_equal(ok["seqs"], kseq)
    finally:
        ix.close()


# ---- 5. long matches ------------------------------------------------------------------------------------------------------------

class Whole:
    pass


@pytest.fixture(scope="module")
def whole(fixtures, gpu_ok):
    """acgt48k's one document as the query: the query IS the text and no match is longer than its prefix, so
    len[j] = min(j + 1, cap); the ranges of 200 seeded end positions from the oracle, once"""
    fx = fixtures("acgt48k")
    W = Whole()
    W.fx, W.q = fx, fx.docs[0]
    W.n = n = len(W.q)
    assert n == 49152 and len(fx.docs) == 1
    W.j = np.unique(np.concatenate([[0, 7, MAX_PATTERN - 2, MAX_PATTERN - 1, MAX_PATTERN, 39999, 40000, n - 1],
                                    np.random.default_rng(50).integers(0, n, 192)]))
    W.lens = {cap: np.minimum(np.arange(n) + 1, cap).astype(np.int32) for cap in (MAX_PATTERN, 40000)}
    sym = W.q.astype(np.uint16) + 5
    o = pyoracle.Oracle(fx.index)
    try:
        W.ranges = {cap: o.count([sym[j - lens[j] + 1:j + 1] for j in W.j], threads=16) for cap, lens in W.lens.items()}
    finally:
        o.close()
    for f, l in W.ranges.values():
        assert (f <= l).all()
    return W


def test_matches_as_long_as_the_cap(whole):
    """match_stats_kernel's lanes stop at `cap` and nowhere else: 32768 steps by default, 40000 with max_len on the device form
    (above kMaxPattern); the counting form takes exactly len.sum() steps, none of them failing"""
    import torch
    W = whole
    ix = femto_amd.Index(W.fx.index, device=0)
    try:
        lens, first, last = ix.match_stats(W.q)
        want = W.lens[MAX_PATTERN]
        assert np.array_equal(lens, want), np.nonzero(lens != want)[0][:8]
        assert np.array_equal(first[W.j], W.ranges[MAX_PATTERN][0]) and np.array_equal(last[W.j], W.ranges[MAX_PATTERN][1])
        buf = torch.zeros(W.n + 16, dtype=torch.uint8, device=DEV)
        buf[8:8 + W.n] = _t(W.q)
        d_len = torch.full((W.n + 8,), -7, dtype=torch.int32, device=DEV)
        d_first, d_last = torch.full((W.n,), -7, dtype=torch.int64, device=DEV), torch.full((W.n,), -7, dtype=torch.int64, device=DEV)
        ix.match_stats_device(W.n, buf.data_ptr() + 8, d_len, d_first, d_last, max_len=40000)
        d_steps = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        ix.match_stats_steps_device(W.n, buf.data_ptr() + 8, d_steps)
        torch.cuda.synchronize()
        got = d_len.cpu().numpy()
        assert np.array_equal(got[:W.n], W.lens[40000]) and (got[W.n:] == -7).all()
        assert np.array_equal(d_first.cpu().numpy()[W.j], W.ranges[40000][0]) and np.array_equal(d_last.cpu().numpy()[W.j], W.ranges[40000][1])
        steps = d_steps.cpu().tolist()
        assert steps[0] == int(want.astype(np.int64).sum()) and 0 <= steps[1] <= steps[0], steps
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.similar(W.q, max_len=65536)
        assert e.value.code == 3 and "65535" in str(e.value)
    finally:
        ix.close()


@pytest.mark.parametrize("kw", OPTION_SETS, ids=[str(i) for i in range(len(OPTION_SETS))])
def test_long_matches_under_every_rank_policy(whole, kw):
    """the same 32768-step lanes through the search_step of every policy the option sets reach on this fixture (RuPolicy,
    RumPolicy, PackPolicy and, in rank modes 1 and 0, LanePolicy: the kinds "ru", "rum", "pack" and "wave" of
    regexp_util.KINDS; "ind" and "pack2" need eng2doc, whose documents are shorter than the cap): one handle open at a time"""
    W = whole
    ix, kind = _open_set(W.fx, kw)
    try:
        for mode in [ix.rank_mode] + ([0] if kw == dict(rank_mode=1) else []):
            ix.set_rank_mode(mode)
            lens, first, last = ix.match_stats(W.q)
            assert np.array_equal(lens, W.lens[MAX_PATTERN]), (kind, mode, np.nonzero(lens != W.lens[MAX_PATTERN])[0][:8])
            assert np.array_equal(first[W.j], W.ranges[MAX_PATTERN][0]) and np.array_equal(last[W.j], W.ranges[MAX_PATTERN][1]), (kind, mode)
    finally:
        ix.close()
