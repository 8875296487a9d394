"""gpu_common.compare, the one check behind every GPU parity test, and gpu_common.compare_lf_step, the one behind every check of
femto_amd_lf_steps_device: a fixture's goldens pass, and each single corruption fails."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from extract_util import Restated
from gpu_common import SEOF, Chain, compare, compare_lf_step, owner_changes, stray_rows, want_from_golden, want_lf_step

_restated = {}


def _R(fixtures, name):
    if name not in _restated:
        _restated[name] = Restated(fixtures(name))
    return _restated[name]


def test_compare_catches_every_single_corruption():
    want = want_from_golden(np.load(os.path.join(GOLDEN, "eng2doc.npz")))
    k = [mo for mo, _, _ in want.locate].index(7)
    _, noccs, offs = want.locate[k]
    cap = len(offs) + 16
    chain = Chain(want.first.copy(), want.last.copy(), noccs.copy(), np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)]),
                  offs.copy(), len(offs), 0)
    leaves = {key: v.copy() for key, v in want.leaves.items()}

    def bump(a, i=3):
        a = a.copy()
        a[i] += 1
        return a

    compare(want, ("unit",), k, count=(want.first, want.last), located=(noccs, offs), chain=chain, capacity=cap, leaves=leaves)
    compare(want, k=k, chain=chain._replace(offsets=offs[:5], overflow=1), capacity=5)        # a buffer that cuts the output short
    nz = int(np.flatnonzero(noccs)[0])
    for field, bad in (("first", bump(chain.first)), ("last", bump(chain.last)), ("noccs", bump(noccs, nz)), ("offsets", bump(offs, 0)),
                       ("offsets", offs[:-1]), ("out_starts", bump(chain.out_starts)), ("total", chain.total + 1), ("overflow", 1)):
        with pytest.raises(AssertionError):
            compare(want, k=k, chain=chain._replace(**{field: bad}), capacity=cap)
        if field in ("first", "last"):       # ... and through the host forms
            with pytest.raises(AssertionError):
                compare(want, count=(bad, want.last) if field == "first" else (want.first, bad))
        elif field in ("noccs", "offsets"):
            with pytest.raises(AssertionError):
                compare(want, k=k, located=(bad, offs) if field == "noccs" else (noccs, bad))
    for key in ("L", "occ", "off"):
        with pytest.raises(AssertionError):
            compare(want, leaves=dict(leaves, **{key: bump(leaves[key])}))


@pytest.mark.parametrize("name", ["eng2doc", "counter400_small"])
def test_compare_lf_step_catches_every_single_corruption(fixtures, name):
    """The answers one LF step owes for every row, built from the reference alone (golden off / L, LF as the inverse of the
    golden fwd_row, SA of the prepared text) in both forms -- femto's marks only (modes 0 / 1, range-split parts) and with
    every third unmarked row carrying a derived mark (modes 3 / 4) -- pass; each single corruption raises."""
    fx, R = fixtures(name), _R(fixtures, name)
    want = want_lf_step(R, fx.gold)
    n = len(want.L)
    assert n == R.N
    rows = np.concatenate([np.arange(n, dtype=np.int64), stray_rows(n)])
    fm = want.off >= 0
    stop = want.L <= SEOF
    assert fm[stop].all() and 1 <= stop.sum() <= 3           # the stop branch only ever shows as "marked, next = -1" here
    assert (want.off[fm] == want.sa[fm]).all()
    for derived in (False, True):
        off = np.concatenate([want.off, np.full(6, -1)])
        if derived:
            extra = np.flatnonzero(~fm)[::3]
            off[extra] = want.sa[extra]
        nxt = np.concatenate([np.where((off[:n] >= 0) | stop, -1, want.lf), np.full(6, -1)])
        plain = np.flatnonzero((off[:n] < 0) & ~stop)           # rows whose step is LF
        assert len(plain) > n // 2 and (nxt[plain] >= 0).all()
        compare_lf_step(rows, nxt, off, want, not derived, n, ("unit", name))
        compare_lf_step(rows[:n][::-1], nxt[:n][::-1], off[:n][::-1], want, not derived, n)      # any order, any subset
        if derived:                                              # ... and the derived form accepts femto's marks alone
            compare_lf_step(rows, np.concatenate([np.where(fm | stop, -1, want.lf), np.full(6, -1)]),
                            np.concatenate([want.off, np.full(6, -1)]), want, False, n)

        def put(a, i, v):
            a = a.copy()
            a[i] = v
            return a

        u, m, s = int(plain[len(plain) // 2]), int(np.flatnonzero(fm & ~stop)[1]), int(np.flatnonzero(stop)[0])
        bad = [("next off by one at an unmarked row", put(nxt, u, nxt[u] + 1), off),
               ("next one short at an unmarked row", put(nxt, u, nxt[u] - 1), off),
               ("next = LF at a marked row", put(nxt, m, want.lf[m]), off),
               ("no offset at a row femto marks", nxt, put(off, m, -1)),
               ("a wrong offset at a row femto marks", nxt, put(off, m, off[m] + 1)),
               ("a stop row with a next row", put(nxt, s, 0), off),
               ("a stop row with a next row and no offset", put(nxt, s, 0), put(off, s, -1))]
        # an offset at a row nobody need mark: SA[row] + 1 is wrong in either form, SA[row] itself only on femto's marks
        bad.append(("a derived mark that is not SA[row]", put(nxt, u, -1), put(off, u, want.sa[u] + 1)))
        if not derived:
            bad.append(("a mark femto does not have", put(nxt, u, -1), put(off, u, want.sa[u])))
        else:
            compare_lf_step(rows, put(nxt, u, -1), put(off, u, want.sa[u]), want, False, n)
        for k in range(6):                                       # an out-of-range slot left at 0, in next or in off
            bad.append(("out of range, next = 0", put(nxt, n + k, 0), off))
            bad.append(("out of range, off = 0", nxt, put(off, n + k, 0)))
        for why, bn, bo in bad:
            with pytest.raises(AssertionError) as ei:
                compare_lf_step(rows, bn, bo, want, not derived, n, ("unit", name))
            assert "row" in ei.value.args[0] and ("femto marks only", "derived marks")[derived] in ei.value.args[0], why
    with pytest.raises(AssertionError):
        compare_lf_step(rows, nxt[:-1], off, want, False, n)


def test_owner_changes_counts_of_the_reference_walk(fixtures):
    """gpu_common.owner_changes (what the range-split tests expect of the walker exchange) on the reference alone: with one
    owner nothing moves; the first step's changes under the block ranges of femto_amd_open_split"""
    import torch
    from femto_amd import parallel
    from oracle import pyoracle as po
    for name, nparts, first_step, live_rows in (("acgt48k", 2, 15669, 46694), ("acgt48k", 3, 23605, 46694), ("chunks2doc", 3, 3182, 4950),
                                                ("counter400_small", 8, 325, 380), ("eng2doc", 2, 10700, None), ("runs3doc", 3, 6, None),
                                                ("b1000", 3, 0, None)):
        fx, R = fixtures(name), _R(fixtures, name)
        want = want_lf_step(R, fx.gold)
        o = po.Oracle(fx.index)
        n = len(want.L)
        owner = parallel.owner_of_rows(torch.arange(n), o.block_size, parallel.split_bounds(o.num_blocks, nparts)).numpy()
        changes, rounds, live = owner_changes(want, owner)
        assert owner_changes(want, np.zeros(n, dtype=np.int64)) == (0, rounds, live)
        assert 1 <= rounds <= o.mark_period + 2 and (live_rows is None or live == live_rows), (name, rounds, live)
        go = np.flatnonzero((want.off < 0) & (want.L > SEOF))
        assert int((owner[want.lf[go]] != owner[go]).sum()) == first_step, (name, nparts)
        assert changes >= first_step
