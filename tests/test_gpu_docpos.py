"""The positional operators on the GPU (femto_amd_docpos_device, femto_amd_docpos_documents_device, femto_amd_proximity) against the
restatements of tests/docpos_util.py: the reference's known answers, jobs that straddle the tile, many small jobs beside one
large one, more tiles than the call has chunks, the overflow protocol, aliasing and chaining, and pattern pairs end to end on the
multi-document fixtures."""
import numpy as np
import pytest

import femto_amd
import doclist_util as du
import docpos_util as dp
from gpu_common import _open

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -77
GUARD = 256


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def ix(fixtures, gpu_ok):
    h = _open(fixtures("eng2doc").index)
    yield h
    h.close()


class Views:
    """jobs as views into ONE pair of arrays holding `lists` one after another: job k = lists[ia[k]] op lists[ib[k]]"""

    def __init__(self, lists, ia, ib, ops, ds):
        self.lists = [dp.pairs(x) for x in lists]
        lens = np.array([len(x) for x in self.lists], dtype=np.int64)
        lstart = np.concatenate([[0], np.cumsum(lens)])[:-1]
        flat = np.concatenate(self.lists + [np.zeros((1, 2), dtype=np.int64)])
        self.doc, self.off = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
        self.ia, self.ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
        self.a_start, self.b_start = lstart[self.ia], lstart[self.ib]
        self.a_n, self.b_n = lens[self.ia].astype(np.int32), lens[self.ib].astype(np.int32)
        self.ops, self.ds = np.asarray(ops, dtype=np.int32), np.asarray(ds, dtype=np.int32)

    def want(self, f=dp.loop):
        return dp.batch([self.lists[x] for x in self.ia], [self.lists[x] for x in self.ib], self.ops, self.ds, f)

    def run(self, ix, cap):
        return _run(ix, self.doc, self.off, self.a_start, self.a_n, self.doc, self.off, self.b_start, self.b_n, self.ops, self.ds, cap)


def _run(ix, a_doc, a_off, a_start, a_n, b_doc, b_off, b_start, b_n, ops, ds, cap):
    """one femto_amd_docpos_device call: (res_starts, res_doc, res_off, res_total); the pair arrays hold GUARD entries behind cap"""
    import torch
    n = len(ops)
    rs = torch.full((n + 1,), SENT, dtype=torch.int64, device=DEV)
    rd = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device=DEV)
    ro = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device=DEV)
    rt = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
    same = a_doc is b_doc
    d_ad, d_ao = _t(a_doc), _t(a_off)
    d_bd, d_bo = (d_ad, d_ao) if same else (_t(b_doc), _t(b_off))
    keep = [_t(x) for x in (a_start, a_n, b_start, b_n, ops, ds)]            # (alive until the synchronise)
    ix.docpos_device(n, d_ad.data_ptr(), d_ao.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), d_bd.data_ptr(), d_bo.data_ptr(),
                     keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), rs.data_ptr(), rd.data_ptr(), ro.data_ptr(),
                     cap, rt.data_ptr())
    torch.cuda.synchronize()
    return rs.cpu().numpy(), rd.cpu().numpy(), ro.cpu().numpy(), rt.cpu().tolist()


def _check(got, want, cap, what=()):
    rs, rd, ro, rt = got
    ws, wd, wo = want
    tot = int(ws[-1])
    assert rt == [tot, int(tot > cap)], ("res_total", rt, tot) + what
    assert np.array_equal(rs, ws), ("res_starts",) + what
    m = min(tot, cap)
    if tot <= cap:
        assert np.array_equal(rd[:m], wd[:m]) and np.array_equal(ro[:m], wo[:m]), ("pairs",) + what
    assert (rd[cap:] == SENT).all() and (ro[cap:] == SENT).all(), ("wrote at or behind res_capacity",) + what
    if tot <= cap:
        assert (rd[tot:] == SENT).all() and (ro[tot:] == SENT).all(), ("wrote behind the results",) + what


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------

def test_known_answers_on_the_device(ix):
    a_lists, b_lists = [dp.pairs(k[0]) for k in dp.KATS], [dp.pairs(k[1]) for k in dp.KATS]
    ops, ds = np.array([k[2] for k in dp.KATS], dtype=np.int32), np.array([k[3] for k in dp.KATS], dtype=np.int32)

    def flat(lists):
        lens = np.array([len(x) for x in lists], dtype=np.int64)
        f = np.concatenate(lists + [np.zeros((1, 2), dtype=np.int64)])
        return np.ascontiguousarray(f[:, 0]), np.ascontiguousarray(f[:, 1]), np.concatenate([[0], np.cumsum(lens)])[:-1], lens.astype(np.int32)

    ad, ao, sa, na = flat(a_lists)
    bd, bo, sb, nb = flat(b_lists)
    got = _run(ix, ad, ao, sa, na, bd, bo, sb, nb, ops, ds, 64)
    want = [dp.pairs(k[4]) for k in dp.KATS]
    ws = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    allw = np.concatenate(want)
    _check(got, (ws, allw[:, 0], allw[:, 1]), 64, ("KATs",))
    hs, hd, ho = ix.docpos(a_lists, b_lists, ops, ds)
    assert np.array_equal(hs, ws) and np.array_equal(hd, allw[:, 0]) and np.array_equal(ho, allw[:, 1])
    # an operator the call does not know yields the empty result
    got = _run(ix, ad, ao, sa, na, bd, bo, sb, nb, np.full(len(ops), 9, dtype=np.int32), ds, 64)
    _check(got, (np.zeros(len(ops) + 1, dtype=np.int64), allw[:0, 0], allw[:0, 1]), 64, ("unknown op",))
    hs, hd, ho = ix.docpos([], [], [], [])
    assert hs.tolist() == [0] and len(hd) == 0 and len(ho) == 0


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------------------

def _split(rng, n, ndocs, span):
    """a random list of n pairs dealt at random to two lists, a tenth of the pairs to both"""
    x = dp.random_list(rng, n, ndocs, span)
    side = rng.integers(0, 10, len(x))
    return x[side <= 5], x[side >= 5]


def _alternating(n, first_b):
    """one document, offsets 0, 10, 20, ..: merged position p belongs to b when p is even (first_b) or odd"""
    x = np.stack([np.zeros(n, dtype=np.int64), 10 * np.arange(n, dtype=np.int64)], axis=1)
    even = np.arange(n) % 2 == 0
    return (x[~even], x[even]) if first_b else (x[even], x[~even])


def test_tile_edges(ix):
    T = femto_amd.docpos_info()
    rng = np.random.default_rng(7)
    lists, ja, jb = [], [], []

    def job(a, b):
        lists.extend([dp.pairs(a), dp.pairs(b)])
        ja.append(len(lists) - 2)
        jb.append(len(lists) - 1)

    for n in (0, 1, T - 1, T, T + 1, 2 * T, 3 * T + 5):          # a_n + b_n on either side of the tile
        x = dp.random_list(rng, n, 3, 4 * T)
        side = rng.integers(0, 2, len(x)).astype(bool)
        job(x[side], x[~side])
        assert len(lists[-1]) + len(lists[-2]) == n
    lo, hi = dp.random_list(rng, T + 3, 1, 8 * T), dp.random_list(rng, T + 3, 1, 8 * T) + [1, 0]
    job(lo, hi)                                                    # all of a before all of b: the split sits at a corner
    job(hi, lo)
    d0 = dp.random_list(rng, T, 1, 4 * T)                          # a document change exactly at the tile boundary
    d1 = dp.random_list(rng, T // 2 + 7, 1, 4 * T) + [1, 0]
    sd = rng.integers(0, 2, T).astype(bool)
    s1 = rng.integers(0, 2, len(d1)).astype(bool)
    job(np.concatenate([d0[sd], d1[s1]]), np.concatenate([d0[~sd], d1[~s1]]))
    job(*_alternating(2 * T, True))                                # a at T - 1 whose partner b is the first element of the next tile
    job(*_alternating(2 * T, False))                               # b at T - 1 whose partner a is
    base = np.stack([np.zeros(T, dtype=np.int64), 3 * np.arange(1, T + 1, dtype=np.int64)], axis=1)
    job(np.concatenate([[[0, 0]], base]), base)                    # a position of both lists on either side of the boundary
    job(dp.random_list(rng, T + 1, 2, 2 * T), [])                  # b_n = 0
    job([], dp.random_list(rng, T + 1, 2, 2 * T))                  # a_n = 0
    job(*_split(rng, 700, 2, 400))
    job(*_split(rng, 300, 1, 200))
    assert len(ja) == 17
    combos = [(op, d) for op in (dp.THEN, dp.WITHIN, dp.OR) for d in (-3, 0, 2, 1000)]
    order = rng.permutation(len(ja) * len(combos))               # one call: every shape with every (op, d), as views of the same lists
    ia = np.array([ja[x % len(ja)] for x in order])
    ib = np.array([jb[x % len(ja)] for x in order])
    ops = np.array([combos[x // len(ja)][0] for x in order])
    ds = np.array([combos[x // len(ja)][1] for x in order])
    V = Views(lists, ia, ib, ops, ds)
    want = V.want()
    cap = int(want[0][-1]) + 5
    _check(V.run(ix, cap), want, cap, ("tile edges",))


# ---- 3. many small and one large ---------------------------------------------------------------------------------------------------

def test_many_small_and_one_large(ix):
    rng = np.random.default_rng(8)
    lists, ia, ib = [], [], []
    for k in range(20000):
        a, b = _split(rng, int(rng.integers(0, 41)), int(rng.choice([1, 2, 3])), int(rng.choice([16, 64])))
        lists += [a, b]
    big = dp.random_list(rng, 540000, 50, 20000)
    side = rng.integers(0, 10, len(big))
    lists += [big[side <= 5][:300000], big[side >= 4][:300000]]
    assert len(lists[-1]) == 300000 and len(lists[-2]) == 300000
    order = rng.permutation(20001)
    ia, ib = 2 * order, 2 * order + 1
    ops = rng.integers(0, 3, 20001)
    ds = rng.choice([-1000, -3, -1, 0, 1, 2, 5, 1000], 20001)
    V = Views(lists, ia, ib, ops, ds)
    res = []
    for a, b, op, d in zip(ia, ib, ops, ds):
        res.append((dp.closed if a == 40000 else dp.loop)(lists[a], lists[b], int(op), int(d)))      # (the large job through the closed form)
    ws = np.concatenate([[0], np.cumsum([len(r) for r in res])]).astype(np.int64)
    allr = np.concatenate(res)
    cap = int(ws[-1])
    _check(V.run(ix, cap), (ws, allr[:, 0], allr[:, 1]), cap, ("many small and one large",))


# ---- 3b. more tiles than chunks ----------------------------------------------------------------------------------------------------
# While a call has at most docpos_chunks() tiles a chunk is one tile.  Beyond that a workgroup walks several tiles per chunk: it
# moves from job to job inside the chunk, carries the running slot from tile to tile, notes for every job that starts inside the
# chunk how many outputs of the chunk stand in front of it, and the last chunks of the call are partial or empty.

def _split_exact(rng, n, ndocs, span):
    """as _split, with len(a) + len(b) == n exactly: n // 11 of the positions stand in both lists"""
    s = n // 11
    x = dp.random_list(rng, n - s, ndocs, span)
    assert len(x) == n - s
    side = rng.permutation(np.concatenate([np.full(s, 5), rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 9], n - 2 * s)]))
    return x[side <= 5], x[side >= 5]


def _scattered(rng, njobs, nruns, nlarge):
    """(empty, large): job numbers of runs of consecutive empty jobs -- one at the very start and one at the very end of the
    call -- and of nlarge other jobs scattered through the order.  Job njobs - 6, the last one in front of the empty run at the
    end, is in neither: the caller empties it when the tile count would otherwise fill the last chunk in use."""
    empty = np.zeros(njobs, dtype=bool)
    empty[:7] = empty[-5:] = True
    for at in rng.integers(8, njobs - 20, nruns):
        empty[at:at + int(rng.integers(1, 9))] = True
    free = np.flatnonzero(~empty)
    return empty, rng.choice(free[free != njobs - 6], nlarge, replace=False)


def _chunk_walk(tile_counts, K):
    """(ntiles, per, tile_starts, job of every tile) of a call: `per` consecutive tiles make a chunk, as docpos.hip deals them"""
    ts = np.concatenate([[0], np.cumsum(tile_counts, dtype=np.int64)])
    ntiles = int(ts[-1])
    per = -(-ntiles // K) if ntiles > K else 1
    return ntiles, per, ts, np.repeat(np.arange(len(tile_counts)), tile_counts)


def _fills_last_chunk(sizes, T, K):
    """whether jobs of these sizes make a tile count that leaves no partial chunk"""
    ntiles, per = _chunk_walk(-(-np.asarray(sizes, dtype=np.int64) // T), K)[:2]
    return ntiles % per == 0 or ntiles % K == 0


def test_more_tiles_than_chunks(ix):
    K, T = femto_amd.docpos_chunks(), femto_amd.docpos_info()
    rng = np.random.default_rng(14)
    njobs = 12 * K // 5
    empty, large = _scattered(rng, njobs, 40, 20)
    sizes = ([T + 1, 2 * T, 3 * T + 5] * 7)[:19] + [40 * T]
    size_of = dict(zip(large.tolist(), sizes))
    ns, nds, spans = rng.integers(0, 41, njobs), rng.choice([1, 2, 3], njobs), rng.choice([16, 64], njobs)
    ns[njobs - 6] = 30
    lists = []
    for k in range(njobs):
        if empty[k]:
            lists += [dp.pairs([]), dp.pairs([])]
        elif k in size_of:
            n = size_of[k]
            lists += list(_split_exact(rng, n, 50 if n > 4 * T else 3, 20000 if n > 4 * T else 4 * T))
        else:
            lists += list(_split(rng, int(ns[k]), int(nds[k]), int(spans[k])))
    assert len(lists[2 * njobs - 12]) + len(lists[2 * njobs - 11]) >= 30
    if _fills_last_chunk([len(lists[2 * k]) + len(lists[2 * k + 1]) for k in range(njobs)], T, K):
        lists[2 * njobs - 12] = lists[2 * njobs - 11] = dp.pairs([])
    ia, ib = 2 * np.arange(njobs), 2 * np.arange(njobs) + 1
    ops = rng.integers(0, 3, njobs)
    ds = rng.choice([-1000, -3, -1, 0, 1, 2, 5, 1000], njobs)
    V = Views(lists, ia, ib, ops, ds)
    # the regime, from the inputs alone
    tile_counts = -(-(V.a_n.astype(np.int64) + V.b_n) // T)
    assert [int(tile_counts[k]) for k in large] == [-(-n // T) for n in sizes] and not tile_counts[empty].any()
    assert not tile_counts[0] and not tile_counts[-1]
    ntiles, per, ts, tile_job = _chunk_walk(tile_counts, K)
    assert 2 * K < ntiles < 3 * K and ntiles % K != 0 and per == 3, (ntiles, K)
    used = -(-ntiles // per)
    assert ntiles % per != 0 and used < K                          # the last chunk in use is partial, those behind it are empty
    whole = tile_job[:ntiles // per * per].reshape(-1, per)
    assert ((whole[:, 0] < whole[:, 1]) & (whole[:, 1] < whole[:, 2])).any()       # a chunk with tiles of three jobs
    multi = np.flatnonzero(tile_counts > 1)
    assert (ts[multi] // per != (ts[multi + 1] - 1) // per).any()                   # a multi-tile job across a chunk boundary
    res = []
    for a, b, op, d in zip(ia, ib, ops, ds):
        res.append((dp.closed if len(lists[a]) + len(lists[b]) > T else dp.loop)(lists[a], lists[b], int(op), int(d)))
    nres = np.array([len(r) for r in res], dtype=np.int64)
    # job_local: a job whose first tile is not its chunk's first, behind whole single-tile jobs of the chunk that have outputs
    local = 0
    for k in np.flatnonzero((tile_counts > 0) & (ts[:-1] % per != 0)):
        front = tile_job[ts[k] - ts[k] % per:ts[k]]
        if (tile_counts[front] == 1).all():
            local += int(nres[front].sum() > 0)
    assert local > 100
    ws = np.concatenate([[0], np.cumsum(nres)]).astype(np.int64)
    allr = np.concatenate(res)
    tot = int(ws[-1])
    assert tot > ntiles
    for cap in (tot, tot + 5, tot - 1):
        _check(V.run(ix, cap), (ws, allr[:, 0], allr[:, 1]), cap, ("more tiles than chunks", cap))


def test_documents_of_more_tiles_than_chunks(ix):
    """the same regime through femto_amd_docpos_documents_device.  A list of no pairs has no tile and one list in six is drawn
    empty, so 2.8 * K lists give the 2.3 * K tiles that 2.4 * K non-empty lists would."""
    import torch
    K, T = femto_amd.docpos_chunks(), femto_amd.docpos_info()
    rng = np.random.default_rng(15)
    nlists = 14 * K // 5
    empty, large = _scattered(rng, nlists, 40, 6)
    lens = rng.integers(0, 6, nlists)
    lens[empty] = 0
    lens[large] = [T + 1, 9 * T + 11] * 3
    lens[nlists - 6] = 3
    if _fills_last_chunk(lens, T, K):
        lens[nlists - 6] = 0
    starts = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    seg = np.repeat(np.arange(nlists), lens)
    doc = np.sort(seg * 4 + rng.integers(0, 4, len(seg))) % 4       # 0 to 5 pairs of four documents, ascending within the list
    for k, nd in zip(large, [T, 700] * 3):
        doc[starts[k]:starts[k + 1]] = dp.random_list(rng, int(lens[k]), nd, 4 * T)[:, 0]
    off = np.arange(len(seg)) - starts[seg]                         # (the offsets: ascending; the call does not read them)
    flat = np.stack([doc, off], axis=1).astype(np.int64)
    lists = np.split(flat, starts[1:-1])
    tile_counts = -(-lens.astype(np.int64) // T)
    ntiles, per, ts, tile_job = _chunk_walk(tile_counts, K)
    assert 2 * K < ntiles < 3 * K and ntiles % K != 0 and ntiles % per != 0 and per == 3, (ntiles, K)
    assert not lens[0] and not lens[-1]
    multi = np.flatnonzero(tile_counts > 1)
    assert (ts[multi] // per != (ts[multi + 1] - 1) // per).any()
    ws, wd = dp.documents(lists)
    td = int(ws[-1])
    assert td > ntiles
    d_starts, d_doc = _t(starts), _t(flat[:, 0])
    for cap in (td, td - 1):
        ds_ = torch.full((nlists + 1,), SENT, dtype=torch.int64, device=DEV)
        dd_ = torch.full((td + GUARD,), SENT, dtype=torch.int64, device=DEV)
        dt_ = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
        ix.docpos_documents_device(nlists, d_starts.data_ptr(), d_doc.data_ptr(), ds_.data_ptr(), dd_.data_ptr(), cap, dt_.data_ptr())
        torch.cuda.synchronize()
        assert dt_.cpu().tolist() == [td, int(td > cap)], cap
        assert np.array_equal(ds_.cpu().numpy(), ws), cap
        if cap == td:
            assert np.array_equal(dd_.cpu().numpy()[:td], wd)
        assert bool((dd_[cap:] == SENT).all()), ("wrote at or behind doc_capacity", cap)


# ---- 4. overflow -------------------------------------------------------------------------------------------------------------------

def test_overflow_protocol(ix):
    T = femto_amd.docpos_info()
    rng = np.random.default_rng(9)
    lists = []
    for n in (T + 100, 50, 0, 3 * T, 7):
        lists += list(_split(rng, n, 2, 2 * T))
    V = Views(lists, [0, 2, 4, 6, 8], [1, 3, 5, 7, 9], [dp.OR, dp.WITHIN, dp.OR, dp.WITHIN, dp.OR], [0, 5, 0, 2000, 0])
    want = V.want()
    tot = int(want[0][-1])
    assert tot > T
    for cap in (tot - 1, 10, 0):
        rs, rd, ro, rt = V.run(ix, cap)
        _check((rs, rd, ro, rt), want, cap, ("overflow", cap))
        assert rt == [tot, 1]
    _check(V.run(ix, rt[0]), want, tot, ("second call",))


# ---- 5. aliasing and chaining --------------------------------------------------------------------------------------------------------

def test_aliasing_and_chaining(ix):
    import torch
    rng = np.random.default_rng(10)
    n = 60
    A = [dp.random_list(rng, int(rng.integers(0, 3000)), 6, 900) for _ in range(n)]
    B = [dp.random_list(rng, int(rng.integers(0, 3000)), 6, 900) for _ in range(n)]
    Cl = [dp.random_list(rng, int(rng.integers(0, 3000)), 6, 900) for _ in range(n)]
    V = Views(A + B + Cl, np.arange(n), n + np.arange(n), np.full(n, dp.THEN), np.full(n, 3))          # a and b: views into the same arrays
    w1 = V.want()
    cap1 = int(w1[0][-1]) + 3
    d_doc, d_off = _t(V.doc), _t(V.off)
    mk = lambda shape, dt=torch.int64: torch.full((shape,), SENT, dtype=dt, device=DEV)
    rs1, rd1, ro1, rt1 = mk(n + 1), mk(cap1), mk(cap1), mk(2)
    k1 = [_t(x) for x in (V.a_start, V.a_n, V.b_start, V.b_n, V.ops, V.ds)]
    ix.docpos_device(n, d_doc.data_ptr(), d_off.data_ptr(), k1[0].data_ptr(), k1[1].data_ptr(), d_doc.data_ptr(), d_off.data_ptr(), k1[2].data_ptr(),
                     k1[3].data_ptr(), k1[4].data_ptr(), k1[5].data_ptr(), rs1.data_ptr(), rd1.data_ptr(), ro1.data_ptr(), cap1, rt1.data_ptr())
    # (A THEN 3 B) WITHIN 10 C: the result as the left operand, without leaving the device
    r1 = [np.stack([w1[1][w1[0][k]:w1[0][k + 1]], w1[2][w1[0][k]:w1[0][k + 1]]], axis=1) for k in range(n)]
    w2 = dp.batch(r1, Cl, np.full(n, dp.WITHIN), np.full(n, 10))
    cap2 = int(w2[0][-1]) + 3
    n1 = (rs1[1:] - rs1[:-1]).to(torch.int32)
    c_start = _t(np.concatenate([[0], np.cumsum([len(x) for x in A + B + Cl])])[2 * n:3 * n].astype(np.int64))
    c_n = _t(np.array([len(x) for x in Cl], dtype=np.int32))
    op2, di2 = _t(np.full(n, dp.WITHIN, dtype=np.int32)), _t(np.full(n, 10, dtype=np.int32))
    rs2, rd2, ro2, rt2 = mk(n + 1), mk(cap2), mk(cap2), mk(2)
    ix.docpos_device(n, rd1.data_ptr(), ro1.data_ptr(), rs1.data_ptr(), n1.data_ptr(), d_doc.data_ptr(), d_off.data_ptr(), c_start.data_ptr(),
                     c_n.data_ptr(), op2.data_ptr(), di2.data_ptr(), rs2.data_ptr(), rd2.data_ptr(), ro2.data_ptr(), cap2, rt2.data_ptr())
    # the documents of that result AND a plain document list
    plain = [np.sort(rng.choice(7, int(rng.integers(0, 7)), replace=False)).astype(np.int64) for _ in range(n)]
    r2 = [np.stack([w2[1][w2[0][k]:w2[0][k + 1]], w2[2][w2[0][k]:w2[0][k + 1]]], axis=1) for k in range(n)]
    wd_starts, wd_docs = dp.documents(r2)
    capd = int(wd_starts[-1]) + 3
    ds_, dd_, dt_ = mk(n + 1), mk(capd), mk(2)
    ix.docpos_documents_device(n, rs2.data_ptr(), rd2.data_ptr(), ds_.data_ptr(), dd_.data_ptr(), capd, dt_.data_ptr())
    nd = (ds_[1:] - ds_[:-1]).to(torch.int32)
    p_flat = _t(np.concatenate(plain + [np.zeros(1, dtype=np.int64)]))
    p_start = _t(np.concatenate([[0], np.cumsum([len(x) for x in plain])])[:-1].astype(np.int64))
    p_n = _t(np.array([len(x) for x in plain], dtype=np.int32))
    op3 = _t(np.full(n, du.AND, dtype=np.int32))
    w3 = du.setops([wd_docs[wd_starts[k]:wd_starts[k + 1]] for k in range(n)], plain, np.full(n, du.AND))
    cap3 = int(w3[0][-1]) + 3
    rs3, rd3, rt3 = mk(n + 1), mk(cap3), mk(2)
    ix.docset_device(n, dd_.data_ptr(), ds_.data_ptr(), nd.data_ptr(), p_flat.data_ptr(), p_start.data_ptr(), p_n.data_ptr(), op3.data_ptr(),
                     rs3.data_ptr(), rd3.data_ptr(), cap3, rt3.data_ptr())
    torch.cuda.synchronize()
    for name, (rs, rd, ro, rt), w in (("A THEN 3 B", (rs1, rd1, ro1, rt1), w1), ("WITHIN 10 C", (rs2, rd2, ro2, rt2), w2)):
        tot = int(w[0][-1])
        assert rt.cpu().tolist() == [tot, 0], name
        assert np.array_equal(rs.cpu().numpy(), w[0]), name
        assert np.array_equal(rd.cpu().numpy()[:tot], w[1]) and np.array_equal(ro.cpu().numpy()[:tot], w[2]), name
        assert bool((rd[tot:] == SENT).all()) and bool((ro[tot:] == SENT).all()), name
    assert int(w1[0][-1]) > 0 and int(w2[0][-1]) > 0 and int(w3[0][-1]) > 0
    td = int(wd_starts[-1])
    assert dt_.cpu().tolist() == [td, 0]
    assert np.array_equal(ds_.cpu().numpy(), wd_starts) and np.array_equal(dd_.cpu().numpy()[:td], wd_docs) and bool((dd_[td:] == SENT).all())
    t3 = int(w3[0][-1])
    assert rt3.cpu().tolist() == [t3, 0]
    assert np.array_equal(rs3.cpu().numpy(), w3[0]) and np.array_equal(rd3.cpu().numpy()[:t3], w3[1])
    # the documents under the overflow protocol: one short, complete starts, nothing at or behind the capacity
    ds_, dd_, dt_ = mk(n + 1), mk(td + GUARD), mk(2)
    ix.docpos_documents_device(n, rs2.data_ptr(), rd2.data_ptr(), ds_.data_ptr(), dd_.data_ptr(), td - 1, dt_.data_ptr())
    torch.cuda.synchronize()
    assert dt_.cpu().tolist() == [td, 1] and np.array_equal(ds_.cpu().numpy(), wd_starts) and bool((dd_[td - 1:] == SENT).all())


def test_documents_of_long_lists(ix):
    """lists on either side of the tile, and one of many tiles, through femto_amd_docpos_documents_device"""
    import torch
    T = femto_amd.docpos_info()
    rng = np.random.default_rng(12)
    lists = [dp.random_list(rng, n, nd, 4 * T) for n, nd in ((0, 1), (1, 1), (T - 1, 40), (T, 1), (T + 1, T), (0, 1), (9 * T + 11, 700), (5, 5))]
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.concatenate(lists)
    ws, wd = dp.documents(lists)
    td = int(ws[-1])
    ds_ = torch.full((len(lists) + 1,), SENT, dtype=torch.int64, device=DEV)
    dd_ = torch.full((td + GUARD,), SENT, dtype=torch.int64, device=DEV)
    dt_ = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
    d_starts, d_doc = _t(starts), _t(flat[:, 0])
    ix.docpos_documents_device(len(lists), d_starts.data_ptr(), d_doc.data_ptr(), ds_.data_ptr(), dd_.data_ptr(), td, dt_.data_ptr())
    torch.cuda.synchronize()
    assert dt_.cpu().tolist() == [td, 0]
    assert np.array_equal(ds_.cpu().numpy(), ws) and np.array_equal(dd_.cpu().numpy()[:td], wd) and bool((dd_[td:] == SENT).all())


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------

def _occurrences(docs, pat):
    """(document, offset) of every occurrence of the byte string pat, document by document"""
    out = []
    for k, d in enumerate(docs):
        s, at = d.tobytes(), -1
        while True:
            at = s.find(pat, at + 1)
            if at < 0:
                break
            out.append((k, at))
    return dp.pairs(out)


@pytest.mark.parametrize("name", ["eng2doc", "runs3doc", "chunks2doc"])
def test_proximity_end_to_end(fixtures, gpu_ok, name):
    fx = fixtures(name)
    rng = np.random.default_rng(13)
    ends = du.doc_ends(fx.docs)

    def sample():
        d = fx.docs[int(rng.integers(0, len(fx.docs)))]
        n = int(rng.integers(1, 5))
        at = int(rng.integers(0, max(len(d) - n, 1)))
        return d[at:at + n].tobytes()

    lefts, rights = [sample() for _ in range(50)], [sample() for _ in range(50)]
    rights[:5] = lefts[:5]                                          # the same pattern on both sides: every position in both lists
    combos = [(dp.THEN, 3), (dp.THEN, -6), (dp.WITHIN, 2), (dp.WITHIN, 40), (dp.OR, 0)]
    L, R = lefts * len(combos), rights * len(combos)
    ops = np.repeat([c[0] for c in combos], 50)
    ds = np.repeat([c[1] for c in combos], 50)
    enc = lambda s: np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + 5
    ix = _open(fx.index)
    try:
        occ = {p: _occurrences(fx.docs, p) for p in set(lefts + rights)}
        assert all(len(v) for v in occ.values())
        want = dp.batch([occ[p] for p in L], [occ[p] for p in R], ops, ds)
        got = ix.proximity([enc(p) for p in L], [enc(p) for p in R], ops, ds, 1 << 24)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, "unclamped")
        assert len(want[1])
        # clamped: the operators applied to the rows that were located
        pats = sorted(occ)
        plen, flat, starts = femto_amd.flatten([enc(p) for p in pats])
        noccs, offs = ix.locate_flat(plen, flat, starts, 5)
        ost = np.concatenate([[0], np.cumsum(noccs)])
        clamped = {}
        for k, p in enumerate(pats):
            d, o = du.resolve(ends, np.sort(offs[ost[k]:ost[k + 1]]))
            clamped[p] = np.stack([d, o], axis=1)
        assert any(len(clamped[p]) < len(occ[p]) for p in pats)
        want = dp.batch([clamped[p] for p in L], [clamped[p] for p in R], ops, ds)
        got = ix.proximity([enc(p) for p in L], [enc(p) for p in R], ops, ds, 5)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, "clamped")
    finally:
        ix.close()


def test_more_concurrent_callers_than_scratches(fixtures, gpu_ok):
    """A handle may be used from several host threads at once, and its pool of per-call scratches is bounded (8): 12 threads
    inside femto_amd_proximity together must all return, with the answer a lone caller gets -- no call may hold one scratch while
    it waits for a second one."""
    import threading
    fx = fixtures("eng2doc")
    enc = lambda s: np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + 5
    d = fx.docs[0].tobytes()
    L, R = [enc(d[k:k + 2]) for k in range(0, 80, 2)], [enc(d[k + 3:k + 5]) for k in range(0, 80, 2)]
    ops, ds = np.arange(40) % 3, np.full(40, 12)
    ix = _open(fx.index)
    try:
        alone = ix.proximity(L, R, ops, ds, 1 << 20)
        assert len(alone[1])
        got, errors = [None] * 12, []
        gate = threading.Barrier(12)

        def work(t):
            try:
                gate.wait()
                for _ in range(4):
                    got[t] = ix.proximity(L, R, ops, ds, 1 << 20)
            except Exception as e:          # noqa: BLE001 (reported below)
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(12)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(60)
        assert not any(th.is_alive() for th in threads), "callers of femto_amd_proximity are stuck"
        assert not errors, errors
        for t in range(12):
            assert all(np.array_equal(g, w) for g, w in zip(got[t], alone)), t
    finally:
        ix.close()
