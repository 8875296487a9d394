"""No GPU: the two restatements of the line rule (tests/lines_util.py) agree on every anchor of every fixture; the counts that
keep tests/test_gpu_lines.py from being vacuous, re-derived from the restatement; the library exports the calls and a handle
without a device refuses them."""
import ctypes as C

import numpy as np
import pytest

import femto_amd
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
