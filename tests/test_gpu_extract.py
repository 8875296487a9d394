"""`-m gpu`: extraction (include/femto_amd.h "extraction") on every fixture and every kind of handle -- the text path, the
sample path on packed lines (forced, shifts 3 and 6), on a handle without the text, and on femto's own tables (bytes256:
one leaf launch per step) -- against the two restatements of tests/extract_util.py; the locate -> context chain on one
stream; the HBM accounting; concurrent callers; one full-size 1 GiB handle without the text."""
import threading
import zlib

import numpy as np
import pytest

import femto_amd
from extract_util import FIXTURES, Restated, random_requests

pytestmark = pytest.mark.gpu

KINDS = ["default", "samples3", "samples6", "no_text", "budget64k"]
_restated = {}


def _R(fixtures, name):
    if name not in _restated:
        _restated[name] = Restated(fixtures(name))
    return _restated[name]


def _open_kind(fx, kind):
    if kind == "no_text":
        ix = femto_amd.Index(fx.index, device=0, options=dict(text=0))
    elif kind == "budget64k":
        ix = femto_amd.Index(fx.index, device=0, options=dict(hbm_budget_bytes=1 << 16))
    else:
        ix = femto_amd.Index(fx.index, device=0)
    shift, force = {"samples3": (3, True), "samples6": (6, True)}.get(kind, (-1, False))
    return ix, shift, force


def _context_window(R, p, before, after):
    return R.context_window(p, before, after)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_extract_documents_context(fixtures, gpu_ok, name, kind):
    fx = fixtures(name)
    R = _R(fixtures, name)
    ix, shift, force = _open_kind(fx, kind)
    try:
        before_alloc = ix.structures()["hbm_allocated"]
        try:
            ex = ix.extractor(shift, force)
        except femto_amd.FemtoAmdError as e:
            # a budget that cannot hold the table: ERR_MEM naming the bytes, and the handle still answers as before
            assert kind == "budget64k" and e.code == 1 and "bytes" in str(e), (kind, e)
            assert ix.structures()["hbm_allocated"] == before_alloc
            plen, flat, starts = fx.patterns
            first, last = ix.count_flat(plen, flat, starts)
            assert np.array_equal(first, fx.gold["count_first"]) and np.array_equal(last, fx.gold["count_last"])
            return
        info = ex.info()
        if force or kind == "no_text" or name == "bytes256":      # (bytes256: 257 symbols, no derived lines, no text)
            assert info["path"] == ex.PATH_SAMPLES
        if force:
            assert info["sample_shift"] == shift
        assert ix.structures()["hbm_allocated"] == before_alloc + info["bytes"]
        # extract by position
        pos, lens = random_requests(R.N, seed=zlib.crc32(name.encode()))
        assert np.array_equal(ex.extract(pos, lens), R.extract(pos, lens))
        # ... into caller-chosen slots (gaps stay 0)
        starts = np.cumsum(np.concatenate([[3], lens[:-1].astype(np.int64) + 5]))
        got = ex.extract(pos, lens, out_starts=starts)
        want = np.zeros_like(got)
        for s, w in zip(starts, np.split(R.extract(pos, lens), np.cumsum(lens.astype(np.int64))[:-1])):
            want[s:s + len(w)] = w
        assert np.array_equal(got, want)
        # documents; their SEOF rows against the header's
        for d in range(len(R.doc_ends)):
            assert np.array_equal(ex.extract_document(d), R.document(d)), d
        if info["path"] == ex.PATH_SAMPLES:
            assert np.array_equal(ex.eof_rows(), R.eof_rows_gold)
        # context: rows form on every row of the small fixtures (a sample of the large), offsets form, out-of-range rows
        rows = np.arange(R.N) if R.N <= 20000 else np.random.default_rng(3).integers(0, R.N, 20000)
        for before, after in ((0, 0), (1, 1), (7, 7), (64, 64), (0, 7), (64, 1)):
            ctx, p = ex.context(rows=rows, before=before, after=after)
            assert np.array_equal(p, R.sa[rows])
            assert np.array_equal(ctx, _context_window(R, R.sa[rows], before, after)), (before, after)
            ctx2, _ = ex.context(offsets=R.sa[rows], before=before, after=after)
            assert np.array_equal(ctx2, ctx)
        ctx, p = ex.context(rows=np.array([-1, R.N, 0], dtype=np.int64), before=7, after=7)
        assert np.array_equal(p[:2], [-1, -1]) and not ctx[:2].any()
        assert np.array_equal(ctx[2], R.context_rows(0, 7, 7))
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["acgt48k", "eng2doc", "bytes256"])
def test_locate_context_chain(fixtures, gpu_ok, name):
    """locate_device -> context_device(d_offsets = located offsets, d_n = d_total) on one stream, no synchronise between"""
    import torch
    fx = fixtures(name)
    R = _R(fixtures, name)
    for force in (False, True):
        ix = femto_amd.Index(fx.index, device=0)
        try:
            ex = ix.extractor(-1, force)
            plen, flat, starts = fx.patterns
            n = len(plen)
            dev = "cuda:0"
            d_plen, d_flat, d_starts = (torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev),
                                        torch.from_numpy(starts).to(dev))
            noccs, offs = ix.locate_flat(plen, flat, starts, 7)
            cap = len(offs) + 64
            d_n, d_st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_off, d_tot = torch.full((cap,), -1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
            before, after = 16, 16
            d_ctx = torch.full((cap, before + after), 7, dtype=torch.int16, device=dev)
            d_pos = torch.full((cap,), -5, dtype=torch.int64, device=dev)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                ix.locate_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), 7, 0, 0, d_n.data_ptr(), d_st.data_ptr(),
                                 d_off.data_ptr(), cap, d_tot.data_ptr(), stream=s.cuda_stream)
                ex.context_device(cap, d_offsets=d_off.data_ptr(), d_n=d_tot.data_ptr(), before=before, after=after,
                                  d_ctx=d_ctx.data_ptr(), d_pos_out=d_pos.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            tot = int(d_tot[0])
            assert tot == len(offs)
            want, _ = ex.context(offsets=offs, before=before, after=after)
            got = d_ctx.cpu().numpy().view(np.uint16)
            assert np.array_equal(got[:tot], want) and np.array_equal(want, _context_window(R, offs, before, after))
            assert (got[tot:] == 7).all() and (d_pos.cpu().numpy()[tot:] == -5).all()      # anchors beyond d_n untouched
            assert np.array_equal(d_pos.cpu().numpy()[:tot], offs)
        finally:
            ix.close()


def test_device_extract_and_accounting(fixtures, gpu_ok):
    import torch
    fx = fixtures("eng2doc")
    R = _R(fixtures, "eng2doc")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        a0 = ix.structures()["hbm_allocated"]
        ex = ix.extractor(4, True)
        b = ex.info()["bytes"]
        assert b > (R.N >> 4) * 4 and ix.structures()["hbm_allocated"] == a0 + b
        pos, lens = random_requests(R.N, seed=11, n=3000)
        out_starts = np.zeros(len(lens), dtype=np.int64)
        out_starts[1:] = np.cumsum(lens[:-1].astype(np.int64))
        total = int(lens.astype(np.int64).sum())
        for e in (ex, ix.extractor()):
            d_out = torch.full((total + 8,), 9, dtype=torch.int16, device="cuda:0")
            t = [torch.from_numpy(a).to("cuda:0") for a in (pos, lens, out_starts)]
            e.extract_device(len(pos), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d_out.data_ptr())
            torch.cuda.synchronize()
            o = d_out.cpu().numpy().view(np.uint16)
            assert np.array_equal(o[:total], R.extract(pos, lens)) and (o[total:] == 9).all()
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ex.extract(np.array([0], dtype=np.int64), np.array([-1], dtype=np.int32))
        assert e.value.code == 3
        ex.free()
        ix._extractors.pop((4, True))
        ix.extractor().free()
        ix._extractors.clear()
        assert ix.structures()["hbm_allocated"] == a0
    finally:
        ix.close()


def test_concurrent_callers(fixtures, gpu_ok):
    """two threads extract while a third counts on the same handle: every result equals the serial run"""
    fx = fixtures("acgt48k")
    R = _R(fixtures, "acgt48k")
    ix = femto_amd.Index(fx.index, device=0)
    try:
        exs = [ix.extractor(), ix.extractor(5, True)]
        plen, flat, starts = fx.patterns
        reqs = [random_requests(R.N, seed=100 + k, n=5000) for k in range(2)]
        want = [R.extract(*r) for r in reqs]
        errors = []

        def work(k):
            try:
                for _ in range(20):
                    assert np.array_equal(exs[k].extract(*reqs[k]), want[k])
            except Exception as e:      # noqa: BLE001 -- reported below
                errors.append(e)

        def counter():
            try:
                for _ in range(20):
                    first, last = ix.count_flat(plen, flat, starts)
                    assert np.array_equal(first, fx.gold["count_first"]) and np.array_equal(last, fx.gold["count_last"])
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(0,)), threading.Thread(target=work, args=(1,)), threading.Thread(target=counter)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
    finally:
        ix.close()


def test_full_size_1gib_text_free_handle(tmp_path, gpu_ok):
    """1 GiB ACGT under hbm_budget_bytes = 4 x text, without the text: the sample table, 1 M random 64-symbol windows and the
    whole document against the text regenerated on the host"""
    import shutil
    from femto_amd import textgen as tg
    n = 1 << 30
    text = tg.t_acgt(n, 515151)
    path = str(tmp_path / "acgt1g")
    femto_amd.build_index(path, [text], params=None, infos=["full"], device=0)
    ix = femto_amd.Index(path, device=0, options=dict(hbm_budget_bytes=4 * n, text=0))
    try:
        a0 = ix.structures()["hbm_allocated"]
        ex = ix.extractor()
        info = ex.info()
        assert info["path"] == ex.PATH_SAMPLES and info["sample_shift"] == 6 and info["bytes"] >= (n >> 6) * 4
        assert ix.structures()["hbm_allocated"] == a0 + info["bytes"] <= 4 * n
        T = text.astype(np.uint16) + 5
        rng = np.random.default_rng(9)
        pos = rng.integers(0, n + 1, 1 << 20).astype(np.int64)
        lens = np.full(len(pos), 64, dtype=np.int32)
        got = ex.extract(pos, lens).reshape(-1, 64)
        q = pos[:, None] + np.arange(64)[None, :]
        want = np.where(q < n, T[np.minimum(q, n - 1)], np.where(q == n, 2, 0)).astype(np.uint16)
        assert np.array_equal(got, want)
        doc = ex.extract_document(0)
        assert len(doc) == n + 1 and doc[-1] == 2 and np.array_equal(doc[:-1], T)
    finally:
        ix.close()
        shutil.rmtree(path, ignore_errors=True)
