"""The positional operators restated twice (include/femto_amd.h "positional operators"): the reference's two-pointer loops
(thenResults / withinResults, src/main/results.c:732 / 842, and the union of two document-offset lists) written out in plain
Python -- the specification, with the one departure that a position is written once -- and the closed form the kernels use, in
numpy.  A list is an (n, 2) int64 array of (document, offset) rows, strictly ascending."""
import numpy as np

THEN, WITHIN, OR = 0, 1, 2


def pairs(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def loop(a, b, op, d):
    """the loops of results.c, element by element"""
    a, b = [tuple(r) for r in pairs(a).tolist()], [tuple(r) for r in pairs(b).tolist()]
    out = []

    def append(p):
        if not out or out[-1] != p:          # (withinResults would append the position again and fail: here it is written once)
            assert not out or out[-1] < p
            out.append(p)

    i = j = 0
    if op == OR:
        while i < len(a) or j < len(b):
            if j >= len(b) or (i < len(a) and a[i] <= b[j]):
                append(a[i])
                i += 1
            else:
                append(b[j])
                j += 1
    elif op in (THEN, WITHIN):
        pos = abs(int(d))
        while i < len(a) and j < len(b):
            (ld, lo), (rd, ro) = a[i], b[j]
            if ld < rd:
                i += 1
            elif ld > rd:
                j += 1
            else:
                width = ro - lo
                if op == THEN:
                    if d < 0:
                        width = -width
                    emit = 0 < width <= pos
                else:
                    emit = abs(width) <= pos
                if emit:
                    append((ld, min(lo, ro)))
                if ro < lo:
                    j += 1
                else:
                    i += 1
    return pairs(out)


def _keys(a, b):
    m = int(max(a[:, 1].max(initial=0), b[:, 1].max(initial=0))) + 1
    top = int(max(a[:, 0].max(initial=0), b[:, 0].max(initial=0))) + 1
    assert top * m < 2 ** 62 and (len(a) == 0 or a.min() >= 0) and (len(b) == 0 or b.min() >= 0)
    return a[:, 0] * m + a[:, 1], b[:, 0] * m + b[:, 1], m


def closed(a, b, op, d):
    """every left element meets the first right element >= it, every right element the first left element > it"""
    a, b = pairs(a), pairs(b)
    ka, kb, m = _keys(a, b)
    assert (np.diff(ka) > 0).all() and (np.diff(kb) > 0).all()
    dist = abs(int(d))
    if op == OR:
        keys = np.union1d(ka, kb)
    elif op in (THEN, WITHIN):
        j = np.searchsorted(kb, ka, side="left")                  # l's partner: b[j]
        has_r = j < len(kb)
        jj = np.minimum(j, max(len(kb) - 1, 0))
        has_r &= (b[jj, 0] == a[:, 0]) if len(kb) else False
        wl = (b[jj, 1] - a[:, 1]) if len(kb) else np.zeros(len(ka), dtype=np.int64)
        i = np.searchsorted(ka, kb, side="right")                 # r's partner: a[i]
        has_l = i < len(ka)
        ii = np.minimum(i, max(len(ka) - 1, 0))
        has_l &= (a[ii, 0] == b[:, 0]) if len(ka) else False
        wr = (a[ii, 1] - b[:, 1]) if len(ka) else np.zeros(len(kb), dtype=np.int64)
        if op == THEN:
            left = has_r & (wl > 0) & (wl <= dist) & (d > 0)
            right = has_l & (wr > 0) & (wr <= dist) & (d < 0)
        else:
            left = has_r & (wl <= dist)
            right = has_l & (wr <= dist)
        keys = np.union1d(ka[left], kb[right])
    else:
        keys = np.zeros(0, dtype=np.int64)
    return np.stack([keys // m, keys % m], axis=1).astype(np.int64).reshape(-1, 2)


def batch(a_lists, b_lists, ops, ds, f=loop):
    """(res_starts, res_doc, res_off) of the packed results"""
    res = [f(a, b, int(op), int(d)) for a, b, op, d in zip(a_lists, b_lists, ops, ds)]
    starts = np.concatenate([[0], np.cumsum([len(r) for r in res], dtype=np.int64)]).astype(np.int64)
    allr = np.concatenate(res) if len(res) else np.zeros((0, 2), dtype=np.int64)
    return starts, np.ascontiguousarray(allr[:, 0]), np.ascontiguousarray(allr[:, 1])


def documents(lists):
    """(doc_starts, docs): the ascending distinct documents of every list"""
    res = [np.unique(pairs(x)[:, 0]) for x in lists]
    starts = np.concatenate([[0], np.cumsum([len(r) for r in res], dtype=np.int64)]).astype(np.int64)
    return starts, (np.concatenate(res) if len(res) else np.zeros(0, dtype=np.int64)).astype(np.int64)


def random_list(rng, n, ndocs, span):
    """n distinct (document, offset) pairs (fewer when the space is smaller) of ndocs documents and offsets below span, ascending"""
    n = min(n, ndocs * span)
    k = np.sort(rng.choice(ndocs * span, n, replace=False)).astype(np.int64)
    return np.stack([k // span, k % span], axis=1).reshape(-1, 2)


# ---- the known answers of src/main/results_test.c (:595-607 BOOL_OR_DOC, :623-654 THEN and WITHIN): (a, b, op, d, expected)
_E = []
_L1 = [(1, 5), (1, 12), (2, 4), (2, 14), (3, 1), (4, 4)]
_L2 = [(0, 0), (1, 2), (1, 6), (1, 10), (2, 1), (2, 6), (2, 10), (4, 5)]
_L3 = [(0, 0), (1, 2), (1, 6), (1, 10), (2, 1), (2, 3), (2, 10), (4, 5)]
_O1 = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8)]
_O2 = [(0, 0), (3, 1), (5, 1), (12, 1)]
KATS = [
    (_O1, _O2, OR, 0, [(0, 0), (1, 1), (2, 2), (3, 1), (3, 3), (4, 4), (5, 1), (5, 5), (6, 6), (7, 7), (8, 8), (12, 1)]),
    (_O1, _E, OR, 0, _O1),
    (_E, _O2, OR, 0, _O2),
    (_L1, _L2, THEN, 2, [(1, 5), (2, 4), (4, 4)]),
    (_L1, _L3, THEN, -2, [(1, 10), (2, 3)]),
    (_L1, _E, THEN, 2, _E),
    (_E, _L2, THEN, 2, _E),
    (_E, _E, THEN, 2, _E),
    (_L1, _L2, WITHIN, 3, [(1, 2), (1, 5), (1, 10), (2, 1), (2, 4), (4, 4)]),
    (_L1, _L2, WITHIN, -3, [(1, 2), (1, 5), (1, 10), (2, 1), (2, 4), (4, 4)]),
    (_L1, _E, WITHIN, 2, _E),
    (_E, _L2, WITHIN, 2, _E),
    (_E, _E, WITHIN, 2, _E),
]
