"""Every entry of the level table (ktab2) and every key of the context tables (ctx / ctxm / ctx2) against the reference.

The other GPU tests see these tables through the ~260 golden patterns of a fixture and through random sweeps.  Here one batch per
handle asks for EVERY entry: every string of 0 .. K table characters (expected (first, last) from table_util.level_answers, a
recurrence on the golden L that tests/test_table_util.py checks against the oracle on the CPU, and from the oracle itself),
the strings of K + 1 characters (the hand-over from the table to the stepping code), strings spoilt by a character outside the
table; and for the context tables every window of the prepared text of H - 1, H and H + 1 symbols, each followed by a copy
spoilt in one symbol.  count_device gives (first, last); the device chain with rows and row-free at max_occs = 3 gives the
offsets -- the row-free form is the one that trusts the SA[first] a one-row level-table entry or a ctx2 slot carries."""
import time

import numpy as np
import pytest

import femto_amd
from gpu_common import _open, device_chain
from oracle import pyoracle as po
from sa_util import suffix_array
from table_util import (CTX_BIG, PERIODIC_M, PERIODIC_NARROW_M, SEOF, Answers, compare_entries, level_answers, level_batch, level_offsets, oracle_answers,
                        periodic_batch, periodic_rows, periodic_sa, periodic_text, table_chars, text_windows)

pytestmark = pytest.mark.gpu

MAX_OCCS = 3
# fixture, K, rank mode (3: packed lines, 4: two-level lines), one-row entries at level K where the number is pinned
LEVELS = [("acgt48k", 8, 3, 23_104), ("runs3doc", 8, 3, None), ("b1000", 6, 3, None), ("chunks2doc", 5, 4, None), ("eng2doc", 2, 4, None)]
# variant -> (options, environment, K override)
LEVEL_VARIANTS = {"default": ({}, {}, None), "sa1_off": ({}, {"FEMTO_AMD_KTAB_SA1": "0"}, None),
                  "deep_big2": ({}, {"FEMTO_AMD_KTAB_DEEP_BIG": "2"}, None), "no_dense": ({"dense_arrays": 0}, {}, None),
                  "syms1": ({}, {}, 1), "syms2": ({}, {}, 2)}
MID = dict(two_level_lines=1, rank_mode=4, context_mid_table=1, context_syms=3, context2_syms=9)

_cache = {}


def _level_case(fixtures, name, K):
    """batch, expected values and level statistics of (fixture, K): computed once, shared by the handle variants, never changed"""
    key = ("level", name, K)
    if key not in _cache:
        fx = fixtures(name)
        chars = table_chars(fx.prepared_text())
        batch, entries = level_batch(chars, K, seed=1000 + K)
        first, last = level_answers(fx.gold["L"], chars, K)
        o = po.Oracle(fx.index)
        want = oracle_answers(o, batch, MAX_OCCS, threads=16)
        o.close()
        lo = level_offsets(len(chars), K)
        rows = last - first + 1
        assert (rows >= 0).all()
        _cache[key] = dict(batch=batch, entries=entries, want=want, level=Answers(first, last, None, None, None), t=len(chars),
                           rows_K=rows[lo[K]:], rows_parent=rows[lo[K - 1]:lo[K]])
    return _cache[key]


def _check_handle(ix, name, batch, want, what, level=None, entries=None):
    """count_device against the oracle (and the recurrence, for the table's own entries), then the chain with rows and row-free"""
    import torch
    dev = "cuda:0"
    n = len(batch.plen)
    d_plen, d_flat, d_starts = torch.from_numpy(batch.plen).to(dev), torch.from_numpy(batch.flat.view(np.int16)).to(dev), torch.from_numpy(batch.starts).to(dev)
    f, l = torch.full((n,), -7, dtype=torch.int64, device=dev), torch.full((n,), -7, dtype=torch.int64, device=dev)
    ix.count_device(n, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), f.data_ptr(), l.data_ptr())
    torch.cuda.synchronize()
    got = (f.cpu().numpy(), l.cpu().numpy())
    if level is not None:
        compare_entries(name, batch, level, count=got, upto=entries, what=("count_device vs recurrence",) + what)
    compare_entries(name, batch, want, count=got, what=("count_device vs oracle",) + what)
    cap = len(want.offs) + 16
    for row_free in (False, True):
        chain = device_chain(ix, batch.plen, batch.flat, batch.starts, MAX_OCCS, cap, row_free=row_free)
        compare_entries(name, batch, want, chain=chain, capacity=cap, what=("row-free" if row_free else "chain",) + what)


# (eng2doc's K is 2: its syms2 handle would be its default handle again)
@pytest.mark.parametrize("name,K,mode,one_row,variant", [lv + (v,) for lv in LEVELS for v in LEVEL_VARIANTS if (lv[0], v) != ("eng2doc", "syms2")])
def test_every_level_table_entry(fixtures, gpu_ok, monkeypatch, name, K, mode, one_row, variant):
    """Every entry of the level table, dead ones and one-row ones with their text position included, on the default handle, without
    the positions (FEMTO_AMD_KTAB_SA1=0, and dense_arrays=0: no suffix array to take them from), with every compact entry of
    two rows or more recomputed from its ancestors (FEMTO_AMD_KTAB_DEEP_BIG=2), and at the depths where "the last two levels are
    compact" has its edges (K = 1: one compact level, nothing above; K = 2: both levels below the root compact)."""
    t0 = time.time()
    opts, env, k_override = LEVEL_VARIANTS[variant]
    main = k_override is None
    K = K if main else k_override
    case = _level_case(fixtures, name, K)
    rows_K = case["rows_K"]
    live, one, dead = int((rows_K >= 2).sum()), int((rows_K == 1).sum()), int((rows_K == 0).sum())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ix = femto_amd.Index(fixtures(name).index, device=0, options=dict(opts, level_table_syms=K))
    pi = ix.pack_info()
    assert pi["ktab_syms"] == K and pi["level_table"] and ix.rank_mode == mode, (pi, ix.rank_mode)
    # what this run claims to exercise, from the reference's values
    if main:
        assert dead > 0, "no dead entry at the deepest level"
    else:      # the shallow tables: every level below the root is compact, and entries of two rows or more sit in it
        assert live > 0 and K <= 2 and len(rows_K) == case["t"] ** K
    if variant == "default":
        assert pi["sa_full"] and one > 0 and (one_row is None or one == one_row), (pi, one)      # one-row entries that carry SA[first]
    if variant == "no_dense":
        assert not pi["sa_full"], pi
    if variant == "deep_big2":      # a recomputation that climbs two levels: the entry and its parent both store "recompute"
        climbs = (rows_K.reshape(-1, case["t"]) >= 2) & (case["rows_parent"] >= 2)[:, None]
        assert K >= 2 and climbs.any()
    what = (variant, "K", K, "mode", mode)
    _check_handle(ix, name, case["batch"], case["want"], what, level=case["level"], entries=case["entries"])
    ix.close()
    print("\n[tables] level %s %s K=%d: %d entries (level K: %d of two rows or more, %d one-row, %d dead), %d patterns, %.2f s"
          % (name, variant, K, case["entries"], live, one, dead, len(case["batch"].plen), time.time() - t0))


# ---- context tables --------------------------------------------------------------------------------------------------------
def _context_case(fixtures, name, hs):
    """the window batch of (fixture, table lengths) and the oracle's answers, computed once"""
    lengths = tuple(sorted({h + d for h in hs if h for d in (-1, 0, 1)}))
    key = ("context", name, lengths)
    if key not in _cache:
        fx = fixtures(name)
        prepared = fx.prepared_text()
        batch, replaced = text_windows(prepared, lengths, seed=20241)
        o = po.Oracle(fx.index)
        want = oracle_answers(o, batch, MAX_OCCS, threads=16)
        o.close()
        rows = want.last - want.first + 1
        # The batch tests what it says: most spoilt windows miss, and every window of the text is found.  (A window with SEOF
        # INSIDE it runs over a document end; the reference orders the rows of the document ends by document, not by what
        # follows them, so whether it finds such a window is the index's luck -- chunks2doc's one such window per length is not
        # found, eng2doc's is.  Those windows stay in the batch and are compared like the others; SEOF as the first or the
        # last symbol is an ordinary occurrence and must be found.)
        assert (rows[replaced] <= 0).mean() > 0.5, (name, lengths, float((rows[replaced] <= 0).mean()))
        inside = np.zeros(len(batch.plen), dtype=bool)
        at = np.flatnonzero(batch.flat == SEOF)
        owner = np.searchsorted(batch.starts, at, side="right") - 1
        rel = at - batch.starts[owner]
        inside[owner[(rel > 0) & (rel < batch.plen[owner] - 1)]] = True
        # ... and how many are not found is pinned: none on eng2doc; on chunks2doc every window with its first document's end
        # inside, ln - 2 of every length ln (72 at the default lengths 11-13, 15-17; 36 at 2 .. 10)
        lost = ~replaced & (rows <= 0)
        assert not (lost & ~inside).any(), (name, lengths)
        assert int(lost.sum()) == (0 if name == "eng2doc" else sum(max(ln - 2, 0) for ln in lengths)), (name, lengths, int(lost.sum()))
        assert int((~replaced & inside).sum()) == (len(fx.docs) - 1) * sum(max(ln - 2, 0) for ln in lengths)
        assert (~replaced & ~inside & (batch.flat[np.minimum(batch.starts, len(batch.flat) - 1)] == SEOF)).any()      # SEOF first: part of the batch
        _cache[key] = dict(batch=batch, replaced=replaced, want=want, rows=rows, lengths=lengths)
    return _cache[key]


def _table_lengths(ix):
    pi = ix.pack_info()
    return pi, (pi["context_syms"], pi["context_mid_syms"], pi["context2_syms"])


def _report(kind, name, variant, hs, case, t0):
    rows, rep = case["rows"], case["replaced"]
    print("\n[tables] %s %s %s H=%s lengths=%s: %d windows (%d of two rows or more, %d one-row, %d not found) + %d spoilt (%d miss), %.2f s"
          % (kind, name, variant, hs, list(case["lengths"]), int((~rep).sum()), int((rows[~rep] >= 2).sum()), int((rows[~rep] == 1).sum()),
             int((rows[~rep] <= 0).sum()), int(rep.sum()), int((rows[rep] <= 0).sum()), time.time() - t0))


def _default_table_lengths(fixtures, name):
    """(H1, HM, H2) of the default handle of a fixture, read once"""
    key = ("default lengths", name)
    if key not in _cache:
        ix = _open(fixtures(name).index, 4)
        _cache[key] = _table_lengths(ix)[1]
        ix.close()
    return _cache[key]


@pytest.mark.parametrize("variant", ["default", "mid", "no_dense", "no_wide", "no_tables"])
@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc"])
def test_every_context_table_key(fixtures, gpu_ok, name, variant):
    """No H-gram of the text is lost in a hash table (probe wrap-around, a full bucket of four, the middle table's cut-down key), every
    ctx2 / ctxm slot's SA[first] is the position of its first row, and H-grams that do not occur miss: every window of the
    prepared text of H - 1, H, H + 1 symbols for every table length H the handle has.  no_wide (context2_table = 0) and
    no_tables (context_table = 0) send the default handle's whole batch down the paths a pattern takes when a table cannot
    answer -- the narrow table alone, and the level table with the stepping code -- and the answers must not change."""
    t0 = time.time()
    fx = fixtures(name)
    opts = {"mid": MID, "no_dense": dict(dense_arrays=0), "no_wide": dict(context2_table=0), "no_tables": dict(context_table=0)}.get(variant)
    ix = _open(fx.index, 4) if opts is None else femto_amd.Index(fx.index, device=0, options=opts)
    pi, hs = _table_lengths(ix)
    assert ix.rank_mode == 4
    if variant == "no_dense" and not pi["context_table"]:
        assert hs == (0, 0, 0) and not pi["sa_full"], pi      # the tables are built from the suffix array and the text: none without them
        ix.close()
        print("\n[tables] context %s no_dense: no context table, %.2f s" % (name, time.time() - t0))
        return
    if variant in ("no_wide", "no_tables"):
        dflt = _default_table_lengths(fixtures, name)
        assert pi["sa_full"] and pi["level_table"] and hs == ((dflt[0], 0, 0) if variant == "no_wide" else (0, 0, 0)), (pi, dflt)
        assert bool(pi["context_table"]) == (variant == "no_wide")
        case = _context_case(fixtures, name, dflt)
    else:
        assert pi["context_table"] and hs[0] > 0 and hs[2] > hs[0], pi
        if variant == "mid":
            assert hs[0] < hs[1] < hs[2], pi
        case = _context_case(fixtures, name, hs)
    _check_handle(ix, name, case["batch"], case["want"], (variant, "H", hs))
    ix.close()
    _report("context", name, variant, hs, case, t0)


# ---- the "too many rows" answer ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def periodic(tmp_path_factory):
    """Indexes that HAVE 2^24 - 1 rows and more under one H-gram: (ab)^M + a tail over nine other characters, 33.5 M rows, written
    on the host from the closed-form suffix array (tests/test_table_util.py checks both on the CPU).  M = 0xffffff + 7 puts the
    two alternating 16-grams at 0xffffff and 0xfffffe rows (the wide table's field at its two ends), M = 0xffffff + 5 the two
    12-grams (the narrow table's); shorter alternating strings have more rows.  get(M) -> dict(text, path, cases)."""
    made = {}

    def get(M):
        if M not in made:
            text = periodic_text(M, 3000, seed=1)
            path = str(tmp_path_factory.mktemp("periodic") / "index")
            femto_amd.build_index_from_sa(path, [text], periodic_sa(text, M, suffix_array), params=None, infos=["periodic"])
            made[M] = dict(text=text, path=path, cases={})
        return made[M]

    return get


# variant -> (M, options or None for the default handle, the table length whose two alternating keys sit at the field's ends)
TOO_MANY = {"wide_edge": (PERIODIC_M, None, 16), "all_three": (PERIODIC_M, MID, 0), "narrow_edge": (PERIODIC_NARROW_M, None, 12)}


@pytest.mark.parametrize("variant", list(TOO_MANY))
def test_context_value_of_too_many_rows_falls_through(periodic, gpu_ok, variant):
    """A context-table value is first row | rows in 24 bits; a range of 0xffffff rows or more is stored as 0xffffff, the look-up
    answers "too many" and the pattern takes the next table: ctx2 -> ctxm -> ctx -> the level table -> the steps.  No golden
    fixture has such a range; the periodic indexes have them.  wide_edge: the default handle (H = 12, 16) on the text whose two
    alternating 16-grams have 0xffffff (too many) and 0xfffffe rows (the largest range a table answers itself) -- the value
    pass 2 of ctx2_build_kernel stores at both ends of the field -- and whose 12-grams are all too many.  narrow_edge: the same
    for the 12-grams of the narrow table (ctx_ends_kernel), the wide table answering below the bound.  all_three: the handle
    with the middle table (H = 3, 6, 9), every alternating key of all three tables too many.  (The level table's own bound,
    2^23 rows with one-row positions, is passed by its entries of one and two symbols on the way.)"""
    t0 = time.time()
    M, opts, edge = TOO_MANY[variant]
    per = periodic(M)
    ix = _open(per["path"], 4) if opts is None else femto_amd.Index(per["path"], device=0, options=opts)
    pi, hs = _table_lengths(ix)
    assert ix.rank_mode == 4 and pi["context_table"] and pi["sa_full"] and pi["level_table"] and hs[0] > 0 and hs[2] > hs[0], pi
    if opts is None:
        assert (hs[0], hs[2]) == (12, 16), pi          # where the texts put the field's two ends
    else:
        assert 0 < hs[0] < hs[1] < hs[2], pi
    lengths = tuple(sorted({h + d for h in hs if h for d in (-1, 0, 1)}))
    if lengths not in per["cases"]:
        batch, rows, k = periodic_batch(per["text"], M, lengths, seed=9)
        o = po.Oracle(per["path"])
        want = oracle_answers(o, batch, MAX_OCCS, threads=16)
        o.close()
        got = want.last - want.first + 1
        assert np.array_equal(got[rows >= 0], rows[rows >= 0])                 # the oracle agrees with the closed form
        per["cases"][lengths] = (batch, want, got, k)
    batch, want, got, k = per["cases"][lengths]
    plen = batch.plen[:k]
    # What this run claims to exercise, from the closed form and the reference's values.  The keys of every table length that
    # are too many: all of them, except at the edge length (one) and in a wide table above the narrow edge (none) ...
    many = {h: sum(periodic_rows(M, h, ph) >= CTX_BIG for ph in (0, 1)) for h in hs if h}
    for h, n_many in many.items():
        assert ((plen == h) & (got[:k] >= CTX_BIG)).sum() == n_many == (1 if h == edge else 0 if edge == 12 and h > 12 else 2), (h, hs)
    # ... longer patterns whose look-up in table `at` ends in such a key, ordinary keys beside them (found once, not found) ...
    at = edge or hs[2]
    ends_in_b = batch.flat[batch.starts[:k] + plen - 1] == ord("b") + 5
    phase = np.where(ends_in_b, at & 1, 1 - (at & 1))                          # of the last `at` symbols of an alternating string
    tail_rows = np.array([periodic_rows(M, at, int(ph)) for ph in phase])
    unspoilt = (np.arange(k) & 1) == 0
    uses_at = (plen > at) & (plen < min([h for h in hs if h > at] or [1 << 30]))
    assert (unspoilt & uses_at & (tail_rows >= CTX_BIG)).any() and (got[k:] == 1).any() and (got[k:] == 0).any()
    # ... and at the edge length the field's last value that is NOT too many next to the first that is
    if edge:
        assert sorted(got[:k][(plen == edge) & unspoilt].tolist()) == [CTX_BIG - 1, CTX_BIG]
    _check_handle(ix, "periodic", batch, want, (variant, "H", hs))
    ix.close()
    print("\n[tables] too many rows %s M=0xffffff+%d H=%s: %d patterns, %d with >= 0xffffff rows, %.2f s (an index is written in its first case)"
          % (variant, M - CTX_BIG, hs, len(batch.plen), int((got >= CTX_BIG).sum()), time.time() - t0))
