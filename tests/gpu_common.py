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
