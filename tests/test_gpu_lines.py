"""`-m gpu`: matching lines (include/femto_amd.h "matching lines") on every fixture and on the three kinds of extractor -- the
text path, the sample path forced (shift 3), a handle without the text -- against the restatement of tests/lines_util.py; the
edge cases of the device forms; the locate -> lines -> bytes -> groups chain on one stream; groups under forced collisions."""
import zlib

import numpy as np
import pytest

import femto_amd
from lines_util import BINARY, FIXTURES, INVALID, Lines, group_first

pytestmark = pytest.mark.gpu

KINDS = ["default", "samples3", "no_text"]
_lines = {}


def _L(fixtures, name):
    if name not in _lines:
        _lines[name] = Lines(fixtures(name))
    return _lines[name]


def _open(fx, kind):
    ix = femto_amd.Index(fx.index, device=0, options=dict(text=0)) if kind == "no_text" else femto_amd.Index(fx.index, device=0)
    return ix, (ix.extractor(3, True) if kind == "samples3" else ix.extractor())


def _anchors(L, name, text_path):
    """the text path: every anchor; a sample path above 20 000 anchors: 5 000 seeded ones and every anchor within 1030 bytes of
    a document's start or end"""
    if text_path or L.N <= 20000:
        return np.arange(L.N, dtype=np.int64)
    picks = [np.random.default_rng(zlib.crc32(name.encode())).choice(L.N, 5000, replace=False)]
    for s, e in zip(L.doc_starts, L.doc_ends):
        picks += [np.arange(s, min(s + 1031, e)), np.arange(max(e - 1031, s), e)]
    return np.unique(np.concatenate(picks)).astype(np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_lines_equal_the_restatement(fixtures, gpu_ok, name, kind):
    L = _L(fixtures, name)
    ix, ex = _open(fixtures(name), kind)
    try:
        path = ex.info()["path"]
        if kind != "default" or name == "bytes256":       # (bytes256: no derived lines, no text)
            assert path == ex.PATH_SAMPLES
        a = _anchors(L, name, path == ex.PATH_TEXT)
        doc, pos, lens, flags, starts, data = ex.lines(a)
        wdoc, wpos, wlen, wflags = L.answer(a)
        assert np.array_equal(doc, wdoc) and np.array_equal(pos, wpos)
        assert np.array_equal(lens, wlen) and np.array_equal(flags, wflags)
        wstarts, wdata = L.packed(wpos, wlen)
        assert np.array_equal(starts, wstarts) and np.array_equal(data, wdata)
        d2, p2, l2, f2 = ex.lines(a[:100], with_bytes=False)
        assert np.array_equal(p2, wpos[:100]) and np.array_equal(l2, wlen[:100]) and np.array_equal(f2, wflags[:100]) and np.array_equal(d2, wdoc[:100])
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["default", "samples3"])
def test_anchors_out_of_range(fixtures, gpu_ok, kind):
    L = _L(fixtures, "chunks2doc")
    ix, ex = _open(fixtures("chunks2doc"), kind)
    try:
        a = np.array([7, -1, L.N, L.N + 5, 1 << 62, -(1 << 62), L.N - 1, 0], dtype=np.int64)
        doc, pos, lens, flags, starts, data = ex.lines(a)
        wdoc, wpos, wlen, wflags = L.answer(a)
        assert list(wflags[1:6]) == [INVALID] * 5 and not (wflags[[0, 6, 7]] & INVALID).any()
        assert np.array_equal(doc, wdoc) and np.array_equal(pos, wpos) and np.array_equal(lens, wlen) and np.array_equal(flags, wflags)
        wstarts, wdata = L.packed(np.maximum(wpos, 0), wlen)
        assert np.array_equal(starts, wstarts) and np.array_equal(data, wdata)      # nothing is written for the five
        assert (np.diff(starts)[1:6] == 0).all()
        gf, ng = ex.line_groups(starts, data, flags)
        wgf, wng = group_first(wstarts, wdata, wflags)
        assert np.array_equal(gf, wgf) and ng == wng and (gf[1:6] == -1).all()
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["default", "samples3"])
def test_live_count_and_capacity(fixtures, gpu_ok, kind):
    """a d_n smaller than n leaves the other slots as they were; a byte capacity one short sets d_total[1] with complete starts"""
    import torch
    L = _L(fixtures, "chunks2doc")
    ix, ex = _open(fixtures("chunks2doc"), kind)
    try:
        dev = "cuda:0"
        a = np.random.default_rng(5).integers(0, L.N, 300).astype(np.int64)
        n, live = len(a), 211
        wdoc, wpos, wlen, wflags = L.answer(a[:live])
        wstarts, wdata = L.packed(wpos, wlen)
        total = int(wstarts[-1])
        d_a, d_n = torch.from_numpy(a).to(dev), torch.tensor([live], dtype=torch.int64, device=dev)
        d_doc, d_pos = torch.full((n,), -7, dtype=torch.int64, device=dev), torch.full((n,), -7, dtype=torch.int64, device=dev)
        d_len, d_fl = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), 77, dtype=torch.uint8, device=dev)
        ex.lines_device(n, d_a.data_ptr(), d_n.data_ptr(), d_doc.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), d_fl.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_doc.cpu().numpy()[:live], wdoc) and (d_doc.cpu().numpy()[live:] == -7).all()
        assert np.array_equal(d_pos.cpu().numpy()[:live], wpos) and (d_pos.cpu().numpy()[live:] == -7).all()
        assert np.array_equal(d_len.cpu().numpy()[:live], wlen) and (d_len.cpu().numpy()[live:] == -7).all()
        assert np.array_equal(d_fl.cpu().numpy()[:live], wflags) and (d_fl.cpu().numpy()[live:] == 77).all()
        for cap in (total + 16, total, total - 1, 0):
            d_st = torch.full((n + 1,), -3, dtype=torch.int64, device=dev)
            d_by = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=dev)
            d_tot = torch.full((2,), -3, dtype=torch.int64, device=dev)
            ex.line_bytes_device(n, d_pos.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), d_by.data_ptr(), cap, d_tot.data_ptr(), d_n=d_n.data_ptr())
            torch.cuda.synchronize()
            assert d_tot.cpu().tolist() == [total, 1 if cap < total else 0], cap
            st = d_st.cpu().numpy()
            assert np.array_equal(st[:live + 1], wstarts) and (st[live + 1:] == total).all()      # complete, and flat beyond the live count
            got = d_by.cpu().numpy()
            k = min(cap, total)
            assert np.array_equal(got[:k], wdata[:k]) and (got[k:] == 0xEE).all(), cap
    finally:
        ix.close()


@pytest.mark.parametrize("name,force", [("eng2doc", False), ("eng2doc", True), ("bytes256", False)])
def test_locate_lines_chain(fixtures, gpu_ok, name, force):
    """locate_device -> lines_device -> line_bytes_device -> line_groups_device on one stream, d_total as d_n, no synchronise
    between: equal to the host forms on the located offsets"""
    import torch
    fx = fixtures(name)
    L = _L(fixtures, name)
    ix = femto_amd.Index(fx.index, device=0)
    try:
        ex = ix.extractor(-1, force)
        plen, flat, starts = fx.patterns
        n = len(plen)
        dev = "cuda:0"
        d_plen, d_flat, d_starts = (torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(starts).to(dev))
        noccs, offs = ix.locate_flat(plen, flat, starts, 7)
        assert len(offs) > 50
        cap = len(offs) + 64
        hdoc, hpos, hlen, hflags, hstarts, hdata = ex.lines(offs)
        bcap = len(hdata) + 32
        d_nocc, d_st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_off, d_tot = torch.full((cap,), -1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        d_doc, d_pos = torch.full((cap,), -7, dtype=torch.int64, device=dev), torch.full((cap,), -7, dtype=torch.int64, device=dev)
        d_len, d_fl = torch.full((cap,), -7, dtype=torch.int32, device=dev), torch.full((cap,), 77, dtype=torch.uint8, device=dev)
        d_bst, d_by = torch.zeros(cap + 1, dtype=torch.int64, device=dev), torch.full((bcap,), 0xEE, dtype=torch.uint8, device=dev)
        d_bt, d_gf = torch.zeros(2, dtype=torch.int64, device=dev), torch.full((cap,), -9, dtype=torch.int64, device=dev)
        d_ng = torch.full((1,), -9, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ix.locate_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), 7, 0, 0, d_nocc.data_ptr(), d_st.data_ptr(),
                             d_off.data_ptr(), cap, d_tot.data_ptr(), stream=s.cuda_stream)
            ex.lines_device(cap, d_off.data_ptr(), d_tot.data_ptr(), d_doc.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), d_fl.data_ptr(),
                            stream=s.cuda_stream)
            ex.line_bytes_device(cap, d_pos.data_ptr(), d_len.data_ptr(), d_bst.data_ptr(), d_by.data_ptr(), bcap, d_bt.data_ptr(),
                                 d_n=d_tot.data_ptr(), stream=s.cuda_stream)
            ex.line_groups_device(cap, d_bst.data_ptr(), d_by.data_ptr(), d_gf.data_ptr(), d_ng.data_ptr(), d_flags=d_fl.data_ptr(),
                                  d_n=d_tot.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        tot = int(d_tot[0])
        assert tot == len(offs) and np.array_equal(d_off.cpu().numpy()[:tot], offs)
        assert np.array_equal(d_doc.cpu().numpy()[:tot], hdoc) and np.array_equal(d_pos.cpu().numpy()[:tot], hpos)
        assert np.array_equal(d_len.cpu().numpy()[:tot], hlen) and np.array_equal(d_fl.cpu().numpy()[:tot], hflags)
        assert (d_pos.cpu().numpy()[tot:] == -7).all() and (d_fl.cpu().numpy()[tot:] == 77).all()
        assert d_bt.cpu().tolist() == [len(hdata), 0] and np.array_equal(d_bst.cpu().numpy()[:tot + 1], hstarts)
        assert np.array_equal(d_by.cpu().numpy()[:len(hdata)], hdata) and (d_by.cpu().numpy()[len(hdata):] == 0xEE).all()
        hgf, hng = ex.line_groups(hstarts, hdata, hflags)
        wgf, wng = group_first(hstarts, hdata, hflags)
        assert np.array_equal(hgf, wgf) and hng == wng
        assert np.array_equal(d_gf.cpu().numpy()[:tot], hgf) and (d_gf.cpu().numpy()[tot:] == -9).all() and int(d_ng[0]) == hng
        # ... and the host forms are the restatement's
        wdoc, wpos, wlen, wflags = L.answer(offs)
        assert np.array_equal(hdoc, wdoc) and np.array_equal(hpos, wpos) and np.array_equal(hlen, wlen) and np.array_equal(hflags, wflags)
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc", "bytes256"])
def test_groups_with_and_without_collisions(fixtures, gpu_ok, name):
    """the groups of EVERY anchor's line equal the numpy grouping with the full hash and, identically, with 3 bits of it: at most
    8 runs for more than a hundred distinct lines, so the byte comparison and the scan of a colliding run decide"""
    L = _L(fixtures, name)
    ix = femto_amd.Index(fixtures(name).index, device=0)
    try:
        ex = ix.extractor()
        flags = (L.binary.astype(np.uint8) * BINARY)
        starts, data = L.packed(L.pos, L.len)
        wgf, wng = group_first(starts, data, flags)
        assert wng > 100
        for bits in (0, 3, 64, 1):
            gf, ng = ex.line_groups(starts, data, flags, hash_bits=bits)
            assert np.array_equal(gf, wgf) and ng == wng, bits
        gf, ng = ex.line_groups(starts, data, None, hash_bits=3)
        assert np.array_equal(gf, wgf) and ng == wng
    finally:
        ix.close()
