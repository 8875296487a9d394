"""`-m gpu`: femto_amd_locate_device_v2's streaming row plan (femto_amd/plan/plan_stream.hip) against the old chain.

The reference in every case is plan_rows_kernel on a SECOND handle, reached through the same entry point with
FEMTO_AMD_PLAN_STREAM=0 (the switch is read on every call: it is set while the reference handle is opened and called, and
removed before the handle under test runs).  "Equal" is noccs, all npats + 1 out_starts, both words of d_total and
offsets[:min(total, capacity)], bit for bit; where the batch is a fixture's own pattern list the goldens are a second
reference through gpu_common.compare.  femto_amd_plan_stream_stats says which path a call took.

Patterns are the fixtures' golden patterns, repeated and cut to length: absent, one-row and many-row patterns mixed."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
from gpu_common import Chain, _open, assert_row_free_equals, compare, device_chain, want_from_golden

pytestmark = pytest.mark.gpu

OFF, GRID = "FEMTO_AMD_PLAN_STREAM", "FEMTO_AMD_PLAN_STREAM_GRID"
CANARY = -7


def _stats():
    """(calls that streamed, calls that did not, long-range launches behind a streaming kernel, workgroups of the last streaming launch)"""
    out = (C.c_int64 * 4)()
    femto_amd.lib().femto_amd_plan_stream_stats(out)
    return tuple(out)


def _batch(fx, npats, shift=0, extra=None):
    """npats patterns: the fixture's golden patterns from number `shift` on, repeated; `extra` (a list of symbols) replaces pattern 1"""
    plen, flat, starts = fx.patterns
    pats = [flat[starts[i]:starts[i] + plen[i]] for i in range(len(plen))]
    pick = [pats[(i + shift) % len(pats)] for i in range(npats)]
    if extra is not None:
        pick[min(1, npats - 1)] = np.asarray(extra, dtype=np.uint16)
    pl = np.array([len(p) for p in pick], dtype=np.int32)
    st = np.zeros(npats, dtype=np.int64)
    st[1:] = np.cumsum(pl[:-1])
    fl = np.concatenate(pick).astype(np.uint16) if pl.sum() else np.zeros(1, dtype=np.uint16)
    return pl, fl, st


def _chain(ix, plen, flat, starts, max_occs, capacity, slack=0, skew=0, row_free=False):
    """one femto_amd_locate_device_v2 call as a Chain + the `slack` entries behind `capacity` of the offsets buffer; skew = 1
    hands d_noccs and d_out_starts over one element into their allocations (not 16-byte aligned)"""
    import torch
    dev = "cuda:0"
    n = len(plen)
    d_plen, d_flat, d_starts = torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(starts).to(dev)
    f, l = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    noccs = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    ostarts = torch.full((n + 9,), CANARY, dtype=torch.int64, device=dev)
    offs = torch.full((capacity + slack + 1,), CANARY, dtype=torch.int64, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    assert noccs.data_ptr() % 16 == 0 and ostarts.data_ptr() % 16 == 0
    ix.locate_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), max_occs, 0 if row_free else f.data_ptr(),
                     0 if row_free else l.data_ptr(), noccs.data_ptr() + 4 * skew, ostarts.data_ptr() + 8 * skew, offs.data_ptr(), capacity,
                     total.data_ptr())
    torch.cuda.synchronize()
    tot, over = total.cpu().tolist()
    no, os_ = noccs.cpu().numpy(), ostarts.cpu().numpy()
    assert (no[:skew] == CANARY).all() and (no[skew + n:] == CANARY).all(), "noccs written outside [0, npats)"
    assert (os_[:skew] == CANARY).all() and (os_[skew + n + 1:] == CANARY).all(), "out_starts written outside [0, npats]"
    o = offs.cpu().numpy()
    return Chain(None if row_free else f.cpu().numpy(), None if row_free else l.cpu().numpy(), no[skew:skew + n], os_[skew:skew + n + 1],
                 o[:min(tot, capacity)], tot, over), o[capacity:]


def _same(a, b, what):
    for name, x, y in zip(Chain._fields, a, b):
        if x is None or y is None:
            assert x is None and y is None, (name,) + what
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name,) + what
        else:
            assert x == y, (name, x, y) + what


class Pair:
    """the handle under test and the reference handle (the old row plan) on one fixture"""

    def __init__(self, monkeypatch, path, mode, options=None):
        self.mp = monkeypatch
        monkeypatch.setenv(OFF, "0")
        self.ref = _open(path, mode) if options is None else femto_amd.Index(path, device=0, options=options)
        monkeypatch.delenv(OFF)
        self.ix = _open(path, mode) if options is None else femto_amd.Index(path, device=0, options=options)

    def reference(self, fn):
        self.mp.setenv(OFF, "0")
        s0 = _stats()
        try:
            out = fn(self.ref)
        finally:
            self.mp.delenv(OFF)
        s1 = _stats()
        assert s1[0] == s0[0] and s1[1] > s0[1], "the reference must run the old row plan"
        return out

    def streamed(self, fn, calls=1, long_launches=0, grid=None):
        """fn on the handle under test: every call must take the streaming kernel, `long_launches` of them with plan_big_rows_kernel behind it"""
        if grid is not None:
            self.mp.setenv(GRID, str(grid))
        s0 = _stats()
        try:
            out = fn(self.ix)
        finally:
            if grid is not None:
                self.mp.delenv(GRID)
        s1 = _stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (calls, 0, long_launches), (s0, s1)
        if grid is not None:
            assert s1[3] == grid
        return out

    def close(self):
        self.ix.close()
        self.ref.close()


@pytest.mark.parametrize("npats", [1, 3, 4, 5, 255, 256, 257, 1023, 1025])
@pytest.mark.parametrize("name,mode", [("acgt48k", 3), ("eng2doc", 4)])
def test_edges_of_the_vector_width_and_the_tile(fixtures, gpu_ok, monkeypatch, name, mode, npats):
    fx = fixtures(name)
    p = Pair(monkeypatch, fx.index, mode)
    assert p.ix.pack_info()["sa_full"]
    b = _batch(fx, npats)
    for mo in (1, 7, 100):
        want = p.reference(lambda ix: device_chain(ix, *b, mo, 1 << 17))
        got = p.streamed(lambda ix: device_chain(ix, *b, mo, 1 << 17))
        _same(got, want, (name, npats, mo))
        assert got.out_starts[-1] == got.total == int(got.noccs.sum())
    p.close()


def test_fixture_batches_equal_the_goldens(fixtures, gpu_ok, monkeypatch):
    """the fixtures' own pattern lists through the streaming kernel: the reference's golden noccs / offsets for every clamp"""
    for name, mode in (("acgt48k", 3), ("eng2doc", 4)):
        fx = fixtures(name)
        p = Pair(monkeypatch, fx.index, mode)
        want = want_from_golden(fx.gold)
        for k, (mo, _, offs) in enumerate(want.locate):
            cap = len(offs) + 16
            got = p.streamed(lambda ix: device_chain(ix, *fx.patterns, mo, cap), long_launches=int(mo > 4096))
            compare(want, (name, "streamed"), k, chain=got, capacity=cap)
            _same(got, p.reference(lambda ix: device_chain(ix, *fx.patterns, mo, cap)), (name, mo))
        p.close()


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_waves_that_loop(fixtures, gpu_ok, monkeypatch, grid):
    """20 011 patterns = 79 tiles on 4, 8 and 12 wavefronts: several tiles per wavefront, a ragged last tile, a last run
    shorter than the others (12 wavefronts: eleven runs of 7 tiles and one of 2)"""
    for name, mode in (("acgt48k", 3), ("eng2doc", 4)):
        fx = fixtures(name)
        p = Pair(monkeypatch, fx.index, mode)
        b = _batch(fx, 20011, shift=grid)
        want = p.reference(lambda ix: device_chain(ix, *b, 100, 1 << 21))
        assert want.total > 0 and not want.overflow
        _same(p.streamed(lambda ix: device_chain(ix, *b, 100, 1 << 21), grid=grid), want, (name, grid))
        _same(p.streamed(lambda ix: device_chain(ix, *b, 100, 1 << 21, row_free=True), grid=grid)._replace(first=want.first, last=want.last), want,
              (name, grid, "row-free"))
        p.close()


def test_capacity(fixtures, gpu_ok, monkeypatch):
    """capacity = total - 1, total and 0: the overflow word, the offsets that fit, and nothing written behind the capacity"""
    fx = fixtures("acgt48k")
    p = Pair(monkeypatch, fx.index, 3)
    b = _batch(fx, 3001)
    total = p.reference(lambda ix: device_chain(ix, *b, 100, 1 << 20)).total
    assert total > 1
    for cap in (total - 1, total, 0):
        want, wtail = p.reference(lambda ix: _chain(ix, *b, 100, cap, slack=4096))
        got, tail = p.streamed(lambda ix: _chain(ix, *b, 100, cap, slack=4096), grid=2)
        _same(got, want, ("capacity", cap))
        assert (got.total, got.overflow) == (total, int(total > cap))
        assert len(got.offsets) == min(total, cap)
        assert (tail == CANARY).all() and (wtail == CANARY).all(), ("written behind the capacity", cap)
    p.close()


def test_long_ranges(fixtures, gpu_ok, monkeypatch):
    """a one-symbol pattern has thousands of rows: max_occs = 100 000 makes it a long range (plan_big_rows_kernel behind the
    streaming kernel); 4096 and 100 clamp it below the limit, and nothing is launched behind the streaming kernel"""
    fx = fixtures("acgt48k")
    plen, flat, starts = fx.patterns
    hit = int(np.flatnonzero(fx.gold["count_last"] >= fx.gold["count_first"])[0])
    sym = int(flat[starts[hit] + plen[hit] - 1])
    p = Pair(monkeypatch, fx.index, 3)
    b = _batch(fx, 1500, extra=[sym])
    for mo, long_launches in ((100000, 1), (4096, 0), (100, 0)):
        want = p.reference(lambda ix: device_chain(ix, *b, mo, 1 << 20))
        if mo == 100000:
            assert want.noccs.max() > 4096, "the one-symbol pattern must be a long range"
        else:
            assert want.noccs.max() == mo
        _same(p.streamed(lambda ix: device_chain(ix, *b, mo, 1 << 20), long_launches=long_launches, grid=2), want, ("long ranges", mo))
        _same(p.streamed(lambda ix: device_chain(ix, *b, mo, 1 << 20), long_launches=long_launches), want, ("long ranges", mo, "default grid"))
    p.close()


def test_alternating_sum_sets(fixtures, gpu_ok, monkeypatch):
    """five calls back to back on one handle and stream: a missed clear of the next launch's group sums, or a wrong
    bsums_clean, shows in the call after"""
    for name, mode in (("acgt48k", 3), ("eng2doc", 4)):
        fx = fixtures(name)
        p = Pair(monkeypatch, fx.index, mode)
        batches = [_batch(fx, n, shift=s) for n, s in ((5000, 0), (5000, 3), (5000, 11), (777, 5), (5000, 7))]
        want = p.reference(lambda ix: [device_chain(ix, *b, 100, 1 << 18) for b in batches])
        got = p.streamed(lambda ix: [device_chain(ix, *b, 100, 1 << 18) for b in batches], calls=5, grid=3)
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, (name, "call", k))
        p.close()


def test_row_free_form(fixtures, gpu_ok, monkeypatch):
    for name, mode in (("acgt48k", 3), ("eng2doc", 4)):
        fx = fixtures(name)
        p = Pair(monkeypatch, fx.index, mode)
        want = want_from_golden(fx.gold)
        s0 = _stats()
        for mo, noccs, offs in want.locate:
            assert_row_free_equals(p.ix, *fx.patterns, mo, noccs, offs, what=(name, "streamed"))
        s1 = _stats()
        assert s1[0] - s0[0] == len(want.locate) and s1[1] == s0[1]
        b = _batch(fx, 2049, shift=2)
        ref = p.reference(lambda ix: device_chain(ix, *b, 100, 1 << 18))
        got = p.streamed(lambda ix: device_chain(ix, *b, 100, 1 << 18, row_free=True))
        _same(got._replace(first=ref.first, last=ref.last), ref, (name, "row-free against the form with rows"))
        p.close()


def test_fallbacks(fixtures, gpu_ok, monkeypatch):
    """d_noccs / d_out_starts that are not 16-byte aligned, and a handle without the dense suffix array, take the old row plan"""
    fx = fixtures("acgt48k")
    p = Pair(monkeypatch, fx.index, 3)
    b = _batch(fx, 1025)
    want = p.reference(lambda ix: _chain(ix, *b, 100, 1 << 16)[0])
    _same(p.streamed(lambda ix: _chain(ix, *b, 100, 1 << 16)[0]), want, ("aligned",))
    s0 = _stats()
    _same(_chain(p.ix, *b, 100, 1 << 16, skew=1)[0], want, ("one element in",))
    s1 = _stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1)
    p.close()
    kw = dict(two_level_lines=1, hbm_budget_bytes=150_000)
    probe = femto_amd.Index(fx.index, device=0, options=kw)
    if probe.pack_info()["sa_full"]:      # the budget still pays for this fixture's suffix array: decline it outright
        kw["dense_arrays"] = 0
    probe.close()
    p = Pair(monkeypatch, fx.index, None, options=kw)
    assert not p.ix.pack_info()["sa_full"] and p.ix.rank_mode in (3, 4)
    want = p.reference(lambda ix: device_chain(ix, *b, 100, 1 << 16))
    s0 = _stats()
    _same(device_chain(p.ix, *b, 100, 1 << 16), want, ("walks to marks",))
    s1 = _stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1)
    compare(want_from_golden(fx.gold, clamps=(7,)), ("walks to marks",), 0, chain=device_chain(p.ix, *fx.patterns, 7, 1 << 16), capacity=1 << 16)
    p.close()


def test_one_locate_sample_per_call(fixtures, gpu_ok, monkeypatch):
    fx = fixtures("acgt48k")
    p = Pair(monkeypatch, fx.index, 3)
    b = _batch(fx, 1025)
    for mo in (100, 100000):      # with and without the long-range kernel inside the bracket
        p.ix.kernel_time_reset()
        p.ix.kernel_time_enable(True)
        p.streamed(lambda ix: device_chain(ix, *b, mo, 1 << 16), long_launches=int(mo > 4096))
        p.ix.kernel_time_enable(False)
        ms, n = p.ix.kernel_time("locate")
        assert n == 1 and ms > 0
        assert p.ix.kernel_time("count")[1] == 1
    p.close()
