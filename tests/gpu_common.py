"""helpers shared by the `-m gpu` test modules"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import femto_amd

# 3: packed small-alphabet lines (default when the index has <= 8 characters); 4: two-level 16-ary lines (default for
# 9..256 characters); 1: lane per query on femto's wavelet tree (default otherwise); 0: wavefront-per-query raw walk
MODES = [3, 4, 1, 0]


def _torchrun(nproc, script_and_args, env, cwd=None, attempts=2):
    """python -m torch.distributed.run on 127.0.0.1 with a free port; one retry (a port can be taken between probing and use)"""
    import socket
    import subprocess
    import sys
    out = None
    for _ in range(attempts):
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
                              "--master-addr", "127.0.0.1", "--master-port", str(port)] + script_and_args,
                             env=env, capture_output=True, text=True, timeout=600, cwd=cwd)
        if out.returncode == 0:
            break
    return out


def _open(path, mode=None):
    """open on GPU 0; mode 4 is built for small alphabets too (two_level_lines=1) so that every fixture exercises it"""
    ix = femto_amd.Index(path, device=0, options=dict(two_level_lines=1))
    if mode is not None:
        _set_mode(ix, mode)
    return ix


def _set_mode(ix, mode):
    if mode == 3 and not ix.pack_info()["available"]:
        ix.close()
        pytest.skip("more than 8 distinct characters: no packed lines for this index")
    if mode == 4 and not ix.pack_info()["available2"]:
        ix.close()
        pytest.skip("more than 256 distinct characters: no two-level lines for this index")
    ix.set_rank_mode(mode)
    assert ix.rank_mode == mode


# the answers a handle owes for one batch: (first, last), [(max_occs, noccs, offsets)] per clamp, {name: array} of leaf answers
Want = namedtuple("Want", "first last locate leaves")
# what femto_amd_locate_device returned: first / last are None in the row-free form; offsets are cut to min(total, capacity)
Chain = namedtuple("Chain", "first last noccs out_starts offsets total overflow")


def patterns_of(g):
    """plen / flat / starts of a fixture's npz (conftest.Fixture.patterns, for the torchrun workers)"""
    plen = g["pat_len"].astype(np.int32)
    starts = np.zeros(len(plen), dtype=np.int64)
    starts[1:] = np.cumsum(plen[:-1])
    return plen, g["pat_flat"].astype(np.uint16), starts


def want_from_golden(g, clamps=None, occs_ch=False):
    """the reference's answers in a fixture's npz: every clamp in Fixture.locate_cases() order (only those in `clamps` when
    given), the leaves L / occ / off, and with occs_ch every OCCS answer for a given character (occs_ch<c>)"""
    locate = [(int(k[3:-6]), g[k], g[k[:-6] + "_offs"]) for k in g.files if k.startswith("loc") and k.endswith("_noccs")]
    leaves = {k: g[k] for k in g.files if k in ("L", "occ", "off") or (occs_ch and k.startswith("occs_ch"))}
    return Want(g["count_first"], g["count_last"], [c for c in locate if clamps is None or c[0] in clamps], leaves)


def compare(want, what=(), k=None, count=None, located=None, chain=None, capacity=None, leaves=None):
    """The one comparison behind assert_answers (pure numpy): count = (first, last); for clamp k of want.locate, located =
    (noccs, offsets) and a Chain whose offset buffer held `capacity`; leaves = {name: array} for names of want.leaves."""
    if count is not None:
        assert np.array_equal(count[0], want.first), ("first",) + what
        assert np.array_equal(count[1], want.last), ("last",) + what
    if k is not None:
        mo, noccs, offs = want.locate[k]
        what = what + ("max_occs", mo)
    if located is not None:
        assert np.array_equal(located[0], noccs), ("noccs",) + what
        assert np.array_equal(located[1], offs), ("offsets",) + what
    if chain is not None:
        if chain.first is not None:
            compare(want, ("chain",) + what, count=(chain.first, chain.last))
        assert (chain.total, chain.overflow) == (len(offs), int(len(offs) > capacity)), ("total", chain.total, chain.overflow) + what
        assert np.array_equal(chain.noccs, noccs), ("chain noccs",) + what
        assert np.array_equal(chain.out_starts, np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)])), ("out_starts",) + what
        assert np.array_equal(chain.offsets, offs[:capacity]), ("chain offsets",) + what
    for key, got in (leaves or {}).items():
        assert np.array_equal(got, want.leaves[key]), (key,) + what


SEOF = 2
# what one step of the locate walk owes per row, from the reference alone: femto's mark offsets (golden `off`, -1 where femto
# has no mark), the suffix array of the prepared text, LF (the inverse of the golden fwd_row) and L
LfWant = namedtuple("LfWant", "off sa lf L")


def stray_rows(n):
    """rows outside an index of n rows, for the handles that check the range on the device (modes 3 / 4)"""
    return np.array([-1, n, n + 1, -2**63, 2**63 - 1, 1 << 40], dtype=np.int64)


def want_lf_step(R, g):
    """LfWant of a fixture: R an extract_util.Restated, g its npz"""
    return LfWant(g["off"].astype(np.int64), R.sa, R.lf, R.L)


def compare_lf_step(rows, nxt, off, want, femto_marks_only, n, what=()):
    """The one comparison behind every check of femto_amd_lf_steps_device (pure numpy): nxt / off are what a launch over `rows`
    returned on an index of n rows.  femto_marks_only: the handle steps on femto's own tables (modes 0 / 1, range-split parts),
    whose marks are exactly the golden ones; otherwise (modes 3 / 4) a row femto does not mark may carry a derived mark, and
    then reports SA[row].  Every message names the first offending row and the form.
    (Every row of the fixtures with L[row] <= SEOF is marked by femto, so the stop-character branch shows as "marked, next =
    -1": the L <= SEOF clause below is never the only reason for a -1 here.)"""
    rows, nxt, off = (np.asarray(a, dtype=np.int64) for a in (rows, nxt, off))
    what = (("femto marks only" if femto_marks_only else "derived marks"),) + (what if isinstance(what, tuple) else (what,))

    def check(bad, msg, sel):
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError((msg, "row", int(rows[sel][i]), "next", int(nxt[sel][i]), "off", int(off[sel][i])) + what)

    assert len(nxt) == len(rows) and len(off) == len(rows), ("lengths", len(rows), len(nxt), len(off)) + what
    inr = (rows >= 0) & (rows < n)
    check((nxt[~inr] != -1) | (off[~inr] != -1), "a row outside the index must give next = off = -1", ~inr)
    r, nx, of = rows[inr], nxt[inr], off[inr]
    fm = want.off[r] >= 0
    check(fm & (of != want.off[r]), "femto's mark offset", inr)
    if femto_marks_only:
        check(~fm & (of != -1), "an offset at a row femto does not mark", inr)
    else:
        check(~fm & (of != -1) & (of != want.sa[r]), "a derived mark's offset is not SA[row]", inr)
    check((of >= 0) & (nx != -1), "a marked row has no next row", inr)
    check((want.L[r] <= SEOF) & (nx != -1), "a stop character ends the walk", inr)
    check((of < 0) & (want.L[r] > SEOF) & (nx != want.lf[r]), "next row is not LF(row)", inr)


def lf_step_all_rows(ix, want, what=(), stray=None):
    """one femto_amd_lf_steps_device launch over every row of `ix` -- followed, in the same launch, by the rows outside the
    index where the handle checks the range on the device (modes 3 / 4; `stray` overrides) -- through compare_lf_step"""
    import torch
    n = int(ix.info.total_length)
    femto_marks_only = ix.rank_mode in (0, 1)
    # modes 0 / 1 index femto's bucket table with row / block_size unchecked: a row outside the index would be an
    # out-of-bounds read on the device there, so those handles are only ever given rows of the index
    stray = (not femto_marks_only) if stray is None else stray
    rows = np.concatenate([np.arange(n, dtype=np.int64), stray_rows(n)]) if stray else np.arange(n, dtype=np.int64)
    d = torch.from_numpy(rows).to("cuda:0")
    nxt, off = torch.full_like(d, -7), torch.full_like(d, -7)
    ix.lf_steps_device(d.numel(), d.data_ptr(), nxt.data_ptr(), off.data_ptr())
    torch.cuda.synchronize()
    compare_lf_step(rows, nxt.cpu().numpy(), off.cpu().numpy(), want, femto_marks_only, n, what)
    return nxt.cpu().numpy()[:n], off.cpu().numpy()[:n]


def walk_all_rows(ix):
    """Every row of `ix` stepped with femto_amd_lf_steps_device, all rows at once, until its walk ends: offset + steps at the
    marked row it reaches (-1 for a walk that stopped without one).  Every walk must have ended after 4 * mark_period + 16 steps."""
    import torch
    n = int(ix.info.total_length)
    dev = "cuda:0"
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    cur, steps, res = rows.clone(), torch.zeros_like(rows), torch.full_like(rows, -1)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    for _ in range(4 * int(ix.info.mark_period) + 16):
        idx = torch.nonzero(alive).flatten()
        if idx.numel() == 0:
            break
        r = cur[idx].contiguous()
        a, b = torch.empty_like(r), torch.empty_like(r)
        ix.lf_steps_device(r.numel(), r.data_ptr(), a.data_ptr(), b.data_ptr())
        torch.cuda.synchronize()
        done = b >= 0
        res[idx[done]] = b[done] + steps[idx[done]]
        dead = (~done) & (a < 0)
        alive[idx[done | dead]] = False
        go = idx[~(done | dead)]
        cur[go] = a[~(done | dead)]
        steps[go] += 1
    assert not bool(alive.any())
    return res.cpu().numpy()


def owner_changes(want, owner):
    """From the reference alone: every row walks row -> LF(row) until it stands on a row femto marks; `owner` (numpy, per row)
    is the part a row belongs to.  Returns (changes, rounds, live): the steps, over all walks, that took a walker to a row of
    another owner, the launches the longest walk needs, and the rows that are not marked themselves."""
    n = len(want.off)
    cur = np.arange(n, dtype=np.int64)
    go = lambda c: (want.off[c] < 0) & (want.L[c] > SEOF)
    cur = cur[go(cur)]
    live, changes, rounds = len(cur), 0, 1
    while len(cur):
        nx = want.lf[cur]
        assert (nx >= 0).all()
        changes += int((owner[nx] != owner[cur]).sum())
        cur = nx[go(nx)]
        rounds += 1
    return changes, rounds, live


def exchange_in_process(parts, block_size, nblocks, want):
    """The walker exchange of femto_amd/parallel.py without torch.distributed, on the parts of a range-split index opened in
    this process: every row of the index is a walker (row, steps); each round the walkers are grouped by the part that owns
    their row (parallel.owner_of_rows) and part p steps ITS group only.  Returns (offsets per row, rounds, walkers that
    changed owner between two consecutive rounds)."""
    import torch
    from femto_amd import parallel
    dev = "cuda:0"
    n = int(parts[0].info.total_length)
    bounds = parallel.split_bounds(nblocks, len(parts))
    slot = torch.arange(n, dtype=torch.int64, device=dev)
    cur, steps = slot.clone(), torch.zeros_like(slot)
    res = torch.full_like(slot, -1)
    rounds = moved = 0
    while slot.numel():
        assert rounds < 4 * int(parts[0].info.mark_period) + 16, "the in-process exchange does not end"
        rounds += 1
        own = parallel.owner_of_rows(cur, block_size, bounds)
        nxt, off = torch.full_like(cur, -7), torch.full_like(cur, -7)
        for p, ix in enumerate(parts):
            sel = torch.nonzero(own == p).flatten()
            if sel.numel() == 0:
                continue
            r = cur[sel].contiguous()
            a, b = torch.empty_like(r), torch.empty_like(r)
            ix.lf_steps_device(r.numel(), r.data_ptr(), a.data_ptr(), b.data_ptr())
            torch.cuda.synchronize()
            nxt[sel], off[sel] = a, b
        compare_lf_step(cur.cpu().numpy(), nxt.cpu().numpy(), off.cpu().numpy(), want, True, n, ("exchange round", rounds))
        done = off >= 0
        res[slot[done]] = off[done] + steps[done]
        go = ~done & (nxt >= 0)
        moved += int((parallel.owner_of_rows(nxt[go], block_size, bounds) != own[go]).sum())
        slot, cur, steps = slot[go], nxt[go], steps[go] + 1
    return res.cpu().numpy(), rounds, moved


def pointer_array(plen, flat, starts):
    """the alpha_t** of femto_amd_parallel_count / _locate, and the arrays it points into (keep them alive)"""
    pats = [np.ascontiguousarray(flat[starts[i]:starts[i] + plen[i]]) for i in range(len(plen))]
    return (C.c_void_p * len(pats))(*[p.ctypes.data if len(p) else None for p in pats]), pats


def assert_answers(ix, plen, flat, starts, want, *, host=True, two_call=False, pointers=False, chain=False, row_free=False,
                   leaves=False, what=()):
    """Ask `ix` for the answers of `want` in every form the flags name and compare them; `what` goes into every message.
    Order: leaves (block_requests), count_flat, then per clamp locate_flat / locate_flat_two_call / the device chain with rows /
    its row-free form (offset buffers of total + 16), then the reference's pointer-array forms (callee-malloc'd offsets[i])."""
    what = what if isinstance(what, tuple) else (what,)
    if leaves:
        rows = np.arange(ix.info.total_length, dtype=np.int64)
        got = dict(zip(("L", "occ", "off"), ix.block_requests(rows)))
        for key in want.leaves:
            if key.startswith("occs_ch"):
                got[key] = ix.block_requests(rows, np.full(len(rows), int(key[7:]), dtype=np.uint16))[1]
        compare(want, what, leaves=got)
    if host:
        compare(want, what, count=ix.count_flat(plen, flat, starts))
    for k, (mo, _, offs) in enumerate(want.locate):
        if host:
            compare(want, what, k, located=ix.locate_flat(plen, flat, starts, mo))
        if two_call:
            compare(want, ("two-call",) + what, k, located=ix.locate_flat_two_call(plen, flat, starts, mo))
        for rf in [False] * chain + [True] * row_free:
            cap = len(offs) + 16
            compare(want, ("row-free" if rf else "chain",) + what, k, chain=device_chain(ix, plen, flat, starts, mo, cap, row_free=rf), capacity=cap)
    if pointers:
        n, lib = len(plen), femto_amd.lib()
        parr, _pats = pointer_array(plen, flat, starts)
        pl = plen.astype(np.int32)
        first, last = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        assert lib.femto_amd_parallel_count(ix.handle, n, pl.ctypes.data, parr, first.ctypes.data, last.ctypes.data) == 0, what
        compare(want, ("pointers",) + what, count=(first, last))
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        for k, (mo, _, _) in enumerate(want.locate):
            noccs, offs = np.zeros(n, dtype=np.int32), (C.POINTER(C.c_int64) * n)()
            assert lib.femto_amd_parallel_locate(ix.handle, n, pl.ctypes.data, parr, mo, noccs.ctypes.data, offs) == 0, what
            got = []
            for i in range(n):
                if noccs[i]:
                    got.extend(offs[i][j] for j in range(noccs[i]))
                    libc.free(offs[i])
                else:
                    assert not offs[i], ("pointers", i) + what
            compare(want, ("pointers",) + what, k, located=(noccs, np.array(got, dtype=np.int64)))


def device_chain(ix, plen, flat, starts, max_occs, capacity, row_free=False, stream=0, reps=1):
    """femto_amd_locate_device (the one-call device chain: count -> plan_rows with the walk inside) on host arrays, as a Chain.
    row_free: the form without row arrays (d_first = d_last = NULL: parallel_locate's own results).  reps > 1 launches again
    into the same buffers; every launch must return what the last one did."""
    import torch
    dev = "cuda:0"
    n = len(plen)
    d_plen, d_flat, d_starts = torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(starts).to(dev)
    f, l = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    noccs = torch.zeros(n, dtype=torch.int32, device=dev)
    ostarts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offs = torch.full((capacity,), -7, dtype=torch.int64, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    outs = []
    for _ in range(reps):
        ix.locate_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), max_occs, 0 if row_free else f.data_ptr(),
                         0 if row_free else l.data_ptr(), noccs.data_ptr(), ostarts.data_ptr(), offs.data_ptr(), capacity, total.data_ptr(), stream)
        torch.cuda.synchronize()
        tot, over = total.cpu().tolist()
        if row_free:
            assert not f.any() and not l.any()
        outs.append(Chain(None if row_free else f.cpu().numpy(), None if row_free else l.cpu().numpy(), noccs.cpu().numpy(),
                          ostarts.cpu().numpy(), offs[:min(tot, capacity)].cpu().numpy(), tot, over))
    for rep, o in enumerate(outs[:-1]):
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[-1])), ("launch", rep, "differs from the last")
    return outs[-1]


# tools/soak.py unpacks the first six fields of a Chain and calls assert_row_free_equals
def device_locate(ix, plen, flat, starts, max_occs, capacity, row_free=False):
    return device_chain(ix, plen, flat, starts, max_occs, capacity, row_free)[:6]


def assert_row_free_equals(ix, plen, flat, starts, max_occs, noccs, offs, what=""):
    assert_answers(ix, plen, flat, starts, Want(None, None, [(max_occs, noccs, offs)], {}), host=False, row_free=True, what=what)
