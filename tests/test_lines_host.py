"""No GPU: the two restatements of the line rule (tests/lines_util.py) agree on every anchor of every fixture; the counts that
keep tests/test_gpu_lines.py from being vacuous, re-derived from the restatement; the library exports the calls and a handle
without a device refuses them."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
import corpus_util as cu
from lines_util import FIXTURES, Lines, group_first, line_loops, lines_of_document

_lines = {}


def _L(fixtures, name):
    if name not in _lines:
        _lines[name] = Lines(fixtures(name))
    return _lines[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatements_agree(fixtures, name):
    for b in fixtures(name).docs:
        start, length, binary = lines_of_document(b, np.arange(len(b) + 1))
        raw = bytes(b)
        for o in range(len(b) + 1):
            assert line_loops(raw, o) == (start[o], length[o], binary[o]), (name, o)


def test_quirks():
    f = lambda s, o: line_loops(s, o)[:2]
    assert f(b"ab\ncd", 4) == (3, 1)            # runs into the end without a terminator: loses its last byte
    assert f(b"ab\ncd", 5) == (3, 2)            # o == L: [line_start, L)
    assert f(b"ab\ncd", 2) == (0, 2)            # on a terminator: the text before it
    assert f(b"ab\ncd\n", 4) == (3, 2)
    assert f(b"", 0) == (0, 0) and f(b"x", 0) == (0, 0) and f(b"x", 1) == (0, 1)
    assert line_loops(b"ab\0cd\n", 4) == (3, 2, True) and line_loops(b"ab\0cd\n", 1) == (0, 2, True)
    assert line_loops(b"a" * 3000 + b"\n", 1500) == (1500 - 1023, 2046, True)
    assert line_loops(b"a" * 1023 + b"\n", 1022) == (0, 1023, False) and line_loops(b"a" * 1024 + b"\n", 1023) == (0, 1024, True)
    assert line_loops(b"a" * 1024, 0) == (0, 1023, True) and line_loops(b"a" * 1023, 0) == (0, 1022, False)


# fixture: (anchors, binary anchors or None = all, distinct lines or None)
COUNTS = {"chunks2doc": (5502, 0, 465), "eng2doc": (40002, 289, 540), "bytes256": (12002, 6541, 152), "acgt48k": (49153, None, None),
          "runs3doc": (19005, 19003, None)}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_counts_keep_the_gpu_test_honest(fixtures, name):
    L = _L(fixtures, name)
    anchors, nbinary, distinct = COUNTS[name]
    assert L.N == anchors
    assert int(L.binary.sum()) == (anchors if nbinary is None else nbinary)
    if distinct is not None:
        starts, data = L.packed(L.pos, L.len)
        gf, ng = group_first(starts, data)
        assert ng == distinct and len(np.unique(gf)) == distinct
    if name in ("eng2doc", "chunks2doc"):
        assert L.binary.mean() <= 0.01
    if name == "bytes256":
        assert L.binary.any() and not L.binary.all()
        allb = np.concatenate(fixtures(name).docs)
        assert (allb == 13).any() and (allb == 0).any()
    if name == "eng2doc":       # a 1167-byte line and no \\0 byte: every binary anchor is a run-out, and both kinds occur
        docs = fixtures(name).docs
        assert max(len(l) for b in docs for l in bytes(b).split(b"\n")) == 1167 and not any((b == 0).any() for b in docs)
        anchor = np.arange(L.N)
        assert (L.binary & (anchor - L.pos == 1023)).any() and (L.binary & (L.pos + L.len - anchor == 1023)).any()
    if name == "runs3doc":
        assert 1 in [len(d) for d in fixtures(name).docs]


def test_library_exports_the_calls():
    for sym in ("femto_amd_lines_device", "femto_amd_line_bytes_device", "femto_amd_line_groups_device", "femto_amd_lines",
                "femto_amd_line_groups"):
        assert hasattr(femto_amd.lib(), sym), sym
    for m in ("lines", "line_groups", "lines_device", "line_bytes_device", "line_groups_device"):
        assert callable(getattr(femto_amd.Extractor, m))


def test_parse_only_handle_refuses(fixtures):
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)
    try:
        with pytest.raises(femto_amd.FemtoAmdError) as e:
            ix.extractor()
        assert e.value.code == 6 and "without a device" in str(e.value)
    finally:
        ix.close()
    # ... and the calls themselves answer an absent extractor with ERR_PARAM, not a crash
    lib = femto_amd.lib()
    one, tot, p = np.zeros(2, dtype=np.int64), C.c_int64(0), C.c_void_p()
    ptr = C.c_void_p(one.ctypes.data)
    assert lib.femto_amd_lines(None, 1, ptr, None, None, None, None, ptr, C.byref(p), C.byref(tot)) == 3
    assert lib.femto_amd_line_groups(None, 1, ptr, None, None, 0, ptr, C.byref(tot)) == 3
    assert lib.femto_amd_lines_device(None, 1, ptr, None, None, None, None, None, None) == 3
    assert lib.femto_amd_line_bytes_device(None, 1, None, ptr, ptr, ptr, None, 0, ptr, None) == 3
    assert lib.femto_amd_line_groups_device(None, 1, None, ptr, None, None, 0, ptr, ptr, None) == 3


# ---- the built corpus "edges" (tests/corpus_util.py): what tests/test_gpu_edges.py relies on, from the restatement alone ---------

@pytest.fixture(scope="module")
def edges():
    docs = cu.edges_docs()
    return docs, Lines(cu.Corpus(docs))


def _stop_at(L, q):
    """is text position q a terminator byte of a document (and not a document's SEOF slot, which Lines.text holds as 0)"""
    seof = np.zeros(L.N + 1, dtype=bool)
    seof[L.doc_ends - 1] = True
    q = np.asarray(q)
    ok = (q >= 0) & (q < L.N)
    c = L.text[np.where(ok, q, 0)]
    return ok & ~seof[np.where(ok, q, 0)] & ((c == 10) | (c == 13) | (c == 0))


def test_edges_corpus_is_what_the_issue_lists(edges):
    docs, L = edges
    lens = [len(d) for d in docs]
    assert len(docs) >= 700 and 60000 <= sum(lens) <= 80000 and L.N == sum(lens) + len(docs)
    assert lens[:cu.TINY] == [i % 18 for i in range(cu.TINY)] and lens.count(0) >= 16          # empty documents occur
    assert tuple(lens[cu.TINY:cu.TINY + len(cu.SINGLE_LINES)]) == cu.SINGLE_LINES
    allb = np.concatenate(docs)
    assert (allb == 13).any() and (allb == 0).any() and (allb == 10).any()
    long_line = docs[-cu.EDGE_RANDOM - 1]          # one \0 in the middle of 3000 bytes
    assert len(long_line) == 3000 and np.nonzero((long_line == 0) | (long_line == 10) | (long_line == 13))[0].tolist() == [1500]


def test_edges_reach_every_distance(edges):
    """a terminator exactly d behind the anchor for d = 255, 256, 257, 1022, 1023 (the last position of a round of 256, the first
    of the next, the last the scan sees) and exactly 1023 and 1024 ahead (seen; not seen: the scan runs out)"""
    docs, L = edges
    anchor = np.arange(L.N)
    back, ahead = anchor - L.pos, L.pos + L.len - anchor
    for d in (255, 256, 257, 1022, 1023):
        at = (back == d) & _stop_at(L, L.pos - 1) & (L.doc[np.maximum(L.pos - 1, 0)] == L.doc)
        assert at.any(), d
        for t in cu.TERMINATORS:
            assert (at & (L.text[np.maximum(L.pos - 1, 0)] == t)).any(), (d, t)
    # 1024 behind: out of sight, the scan runs out after 1023 bytes
    far = _stop_at(L, anchor - 1024) & (L.doc[np.maximum(anchor - 1024, 0)] == L.doc) & (back == 1023)
    assert far.any() and L.binary[far].all()
    seen = (ahead == 1023) & _stop_at(L, L.pos + L.len)
    assert seen.any() and (seen & ~L.binary).any()
    unseen = _stop_at(L, anchor + 1024) & (L.doc[np.minimum(anchor + 1024, L.N - 1)] == L.doc) & (ahead == 1023) & ~_stop_at(L, anchor + 1023)
    assert unseen.any() and L.binary[unseen].all()
    # both causes of `binary`: a \0 that ends the line on either side, and running out of room in a document without any \0
    nul_behind = _stop_at(L, L.pos - 1) & (L.text[np.maximum(L.pos - 1, 0)] == 0) & (L.pos > L.doc_starts[L.doc])
    nul_ahead = _stop_at(L, L.pos + L.len) & (L.text[np.minimum(L.pos + L.len, L.N - 1)] == 0)
    assert (L.binary & nul_behind).any() and (L.binary & nul_ahead).any()
    no_nul = np.array([not (d == 0).any() for d in docs])
    assert (L.binary & no_nul[L.doc]).any() and (~L.binary).any()


def test_edges_windows_hold_many_documents(edges):
    """at least one window of 2047 positions (1023 behind the anchor, 1024 from it on) holds 100 or more SEOFs; so does a round of
    256 positions hold dozens"""
    docs, L = edges
    seof = L.doc_ends - 1
    anchor = np.arange(L.N)
    in_window = np.searchsorted(seof, anchor + 1024, side="left") - np.searchsorted(seof, anchor - 1023, side="left")
    assert in_window.max() >= 100
    in_round = np.searchsorted(seof, anchor + 256, side="left") - np.searchsorted(seof, anchor, side="left")
    assert in_round.max() >= 24


def test_edges_restatements_agree(edges):
    docs, L = edges
    for d, b in enumerate(docs):
        start, length, binary = lines_of_document(b, np.arange(len(b) + 1))
        raw = bytes(b)
        for o in range(len(b) + 1):
            assert line_loops(raw, o) == (start[o], length[o], binary[o]), (d, o)
