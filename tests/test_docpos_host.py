"""The positional operators without a GPU: the reference's known answers through both restatements of tests/docpos_util.py, the
closed form against the loops on random lists, and the host forms' validation order on a parse-only handle."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
import docpos_util as dp

NEW_SYMBOLS = ["femto_amd_docpos_info", "femto_amd_docpos_chunks", "femto_amd_docpos_device", "femto_amd_docpos_documents_device", "femto_amd_docpos",
               "femto_amd_proximity"]
INT_MAX = 2 ** 31 - 1


def test_library_exports_the_docpos_symbols():
    lib = femto_amd.lib()
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    t = femto_amd.docpos_info()
    assert t >= 256 and t % 256 == 0
    assert femto_amd.docpos_chunks() >= 1024
    assert (femto_amd.DOCPOS_THEN, femto_amd.DOCPOS_WITHIN, femto_amd.DOCPOS_OR) == (dp.THEN, dp.WITHIN, dp.OR)


@pytest.mark.parametrize("f", [dp.loop, dp.closed])
def test_known_answers(f):
    """results_test.c:595-607 and :623-654"""
    for a, b, op, d, want in dp.KATS:
        assert f(a, b, op, d).tolist() == [list(p) for p in want], (f.__name__, op, d, a, b)


def test_duplicate_position_is_written_once():
    """(1, 5) stands in both lists and the next left element is within reach: withinResults would append (1, 5) twice"""
    a, b = [(1, 5), (1, 7)], [(1, 5)]
    for f in (dp.loop, dp.closed):
        assert f(a, b, dp.WITHIN, 3).tolist() == [[1, 5]]
        assert f(a, b, dp.WITHIN, 1).tolist() == [[1, 5]]
        assert f(a, b, dp.THEN, 3).tolist() == []                 # r == l yields nothing ...
        assert f(a, [(1, 5), (1, 6)], dp.THEN, 3).tolist() == []  # ... even when a later right element is in reach
        assert f(a, b, dp.THEN, -3).tolist() == [[1, 5]]
        assert f(a, b, dp.OR, 0).tolist() == [[1, 5], [1, 7]]


def random_cases(rng, n):
    """list pairs drawn so that ties, adjacent offsets, empty sides and a single document all occur"""
    ds = [0, 1, -1, 3, -3, INT_MAX, -INT_MAX]
    for k in range(n):
        ndocs = int(rng.choice([1, 1, 2, 4]))
        span = int(rng.choice([4, 8, 30]))
        na, nb = (int(rng.integers(0, 25)) for _ in range(2))
        if k % 17 == 0:
            na = 0
        if k % 19 == 0:
            nb = 0
        yield dp.random_list(rng, na, ndocs, span), dp.random_list(rng, nb, ndocs, span), int(rng.integers(0, 3)), ds[k % len(ds)]


def test_closed_form_equals_the_loop():
    rng = np.random.default_rng(20250117)
    shared = total = 0
    seen_d = set()
    for a, b, op, d in random_cases(rng, 2000):
        got, want = dp.closed(a, b, op, d), dp.loop(a, b, op, d)
        assert np.array_equal(got, want), (a.tolist(), b.tolist(), op, d)
        total += 1
        shared += bool(set(map(tuple, a.tolist())) & set(map(tuple, b.tolist())))
        seen_d.add(d)
    print("pairs with a position in both lists: %d of %d" % (shared, total))
    assert total == 2000 and shared >= 0.05 * total
    assert seen_d == {0, 1, -1, 3, -3, INT_MAX, -INT_MAX}


def _args(n, **over):
    """a well-formed argument list of femto_amd_docpos for n jobs of one pair each, with overrides"""
    z = np.zeros(max(n, 1), dtype=np.int64)
    one = np.ones(max(n, 1), dtype=np.int32)
    a = dict(a_doc=z, a_off=z, a_start=z.copy(), a_n=one.copy(), b_doc=z, b_off=z, b_start=z.copy(), b_n=one.copy(),
             op=np.zeros(max(n, 1), dtype=np.int32), distance=one.copy(), res_starts=np.zeros(n + 1, dtype=np.int64))
    a.update(over)
    return a


def _call_docpos(ix, n, a, null=()):
    pd, po, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    p = lambda k: None if k in null else C.c_void_p(a[k].ctypes.data)
    return femto_amd.lib().femto_amd_docpos(ix.handle, n, p("a_doc"), p("a_off"), p("a_start"), p("a_n"), p("b_doc"), p("b_off"), p("b_start"),
                                            p("b_n"), p("op"), p("distance"), p("res_starts"), None if "res_doc" in null else C.byref(pd),
                                            None if "res_off" in null else C.byref(po), None if "total" in null else C.byref(total))


def test_host_forms_validate_before_they_need_a_device(fixtures):
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)            # parse-only handle: validation comes first, then "no device"
    P, I = femto_amd.ERR_PARAM, femto_amd.ERR_INVALID
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.docpos([[(1, 2)]], [[(1, 3)]], [dp.THEN], [2])
        assert e.value.code == I                                          # well-formed: only the missing device stops it
        assert _call_docpos(ix, 2, _args(2)) == I
        bad = [(-1, _args(1), ()), (2, _args(2, a_n=np.array([1, -1], dtype=np.int32)), ()), (2, _args(2, b_n=np.array([-3, 1], dtype=np.int32)), ()),
               (2, _args(2, a_start=np.array([0, -1], dtype=np.int64)), ()), (2, _args(2, b_start=np.array([-1, 0], dtype=np.int64)), ()),
               (2, _args(2, op=np.array([0, 3], dtype=np.int32)), ()), (2, _args(2, op=np.array([-1, 0], dtype=np.int32)), ())]
        bad += [(1, _args(1), (k,)) for k in ("a_doc", "a_off", "a_start", "a_n", "b_doc", "b_off", "b_start", "b_n", "op", "distance", "res_starts",
                                              "res_doc", "res_off", "total")]
        for n, a, null in bad:
            assert _call_docpos(ix, n, a, null) == P, (n, null, {k: v.tolist() for k, v in a.items()})
        assert _call_docpos(ix, 0, _args(0), ("a_doc", "a_off", "a_start", "a_n", "b_doc", "b_off", "b_start", "b_n", "op", "distance")) == I

        pat = lambda s: np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + 5
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.proximity([pat(b"the")], [pat(b"of")], [dp.WITHIN], [10], 100)
        assert e.value.code == I
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.proximity([pat(b"the")], [pat(b"of")], [7], [10], 100)                       # unknown operator
        assert e.value.code == P
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.proximity([pat(b"the")], [np.array([40000], dtype=np.uint16)], [dp.OR], [0], 100)      # character code >= ALPHA_SIZE
        assert e.value.code == P
        lib = femto_amd.lib()
        plen, flat, starts = femto_amd.flatten([pat(b"the")])
        one = np.ones(1, dtype=np.int32)
        rs = np.zeros(2, dtype=np.int64)
        pd, po, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        vp = lambda x: C.c_void_p(x.ctypes.data)

        def prox(n=1, lp=plen, ls=starts, rp=plen, rstart=starts, res=rs, out=True):
            return lib.femto_amd_proximity(ix.handle, n, vp(lp), vp(flat), vp(ls), vp(rp), vp(flat), vp(rstart), vp(one), vp(one), 10,
                                           vp(res) if res is not None else None, C.byref(pd) if out else None, C.byref(po), C.byref(total))

        assert prox() == I
        assert prox(n=-1) == P
        assert prox(lp=-plen) == P and prox(rp=-plen) == P
        assert prox(ls=starts - 1) == P and prox(rstart=starts - 1) == P
        assert prox(res=None) == P and prox(out=False) == P
        assert lib.femto_amd_proximity(ix.handle, 1, None, vp(flat), vp(starts), vp(plen), vp(flat), vp(starts), vp(one), vp(one), 10, vp(rs),
                                       C.byref(pd), C.byref(po), C.byref(total)) == P
    finally:
        ix.close()
