"""Document listing restated in numpy (include/femto_amd.h "document listing"): what femto_amd_doclist_device and
femto_amd_docset_device owe, from the definitions alone -- documents are contiguous in the prepared text, document d ends at
doc_ends[d] (exclusive), resolve_location (src/main/index.c:1587) counts the ends <= offset."""
from collections import namedtuple

import numpy as np

AND, OR, NOT = 0, 1, 2

# ndocs int32[npats]; docs int64 / hits int32 / live bool over the rows' ragged layout (live: the entries a list occupies --
# the others are unspecified); pair_doc / pair_off int64[rows]
Listing = namedtuple("Listing", "ndocs docs hits live pair_doc pair_off")


def doc_ends(docs):
    """exclusive end offset of every document in the prepared text: each length + 1 (its SEOF), cumulative"""
    return np.cumsum(np.array([len(d) + 1 for d in docs], dtype=np.int64))


def resolve(ends, offsets):
    """(document, offset in document) of text offsets"""
    offsets = np.asarray(offsets, dtype=np.int64)
    doc = np.searchsorted(ends, offsets, side="right").astype(np.int64)
    return doc, offsets - np.concatenate([[0], ends])[doc]


def listing(ends, offsets, out_starts):
    """per segment [out_starts[i], out_starts[i + 1]): sort, resolve, unique with counts"""
    offsets = np.asarray(offsets, dtype=np.int64)
    out_starts = np.asarray(out_starts, dtype=np.int64)
    rows = int(out_starts[-1])
    n = len(out_starts) - 1
    ndocs = np.zeros(n, dtype=np.int32)
    docs, hits = np.full(rows, -1, dtype=np.int64), np.full(rows, -1, dtype=np.int32)
    live = np.zeros(rows, dtype=bool)
    pair_doc, pair_off = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    for i in range(n):
        s, e = int(out_starts[i]), int(out_starts[i + 1])
        if e == s:
            continue
        off = np.sort(offsets[s:e])
        d, o = resolve(ends, off)
        u, c = np.unique(d, return_counts=True)
        ndocs[i] = len(u)
        docs[s:s + len(u)], hits[s:s + len(u)], live[s:s + len(u)] = u, c, True
        pair_doc[s:e], pair_off[s:e] = d, o
    return Listing(ndocs, docs, hits, live, pair_doc, pair_off)


def packed(want, out_starts):
    """the lists of a Listing one after another: (doc_starts, docs, hits)"""
    return np.concatenate([[0], np.cumsum(want.ndocs, dtype=np.int64)]), want.docs[want.live], want.hits[want.live]


def setop(a, b, op):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return {AND: np.intersect1d, OR: np.union1d, NOT: np.setdiff1d}[int(op)](a, b).astype(np.int64)


def setops(a_lists, b_lists, ops):
    """(res_starts, res_docs) of the packed results"""
    res = [setop(a, b, op) for a, b, op in zip(a_lists, b_lists, ops)]
    starts = np.concatenate([[0], np.cumsum([len(r) for r in res], dtype=np.int64)]).astype(np.int64)
    return starts, (np.concatenate(res) if len(res) else np.zeros(0, dtype=np.int64)).astype(np.int64)
