"""What femto_amd/common/host_common.hpp carries for document listing, the positional operators, boolean queries and
extraction alike, where the tests of those four do not pin it down: the refusal of a range-split part (code and message of each
family), the answer to a call with no jobs, a pattern batch that locates no row, and two symbol runs in one padded pattern
buffer (femto_amd_proximity).  All on the eng2doc fixture."""
import numpy as np
import pytest

import femto_amd
import doclist_util as du
import docpos_util as dp
from gpu_common import _open

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -77
INVALID = 6
# the messages of the four families, as their sources gave them before the check became one function
REFUSALS = {
    "doclist_device": "document listing is not available on a range-split part",
    "docpos_device": "positional operators are not available on a range-split part",
    "bquery_run_batch": "boolean queries are not available on a range-split part",
    "Extractor": "extraction is not available on a range-split part",
}


def _full(n, dtype=None):
    import torch
    return torch.full((n,), SENT, dtype=dtype or torch.int64, device=DEV)


def _enc(s):
    return np.frombuffer(s, dtype=np.uint8).astype(np.uint16) + 5


@pytest.fixture(scope="module")
def ix(fixtures, gpu_ok):
    h = _open(fixtures("eng2doc").index)
    yield h
    h.close()


@pytest.fixture(scope="module")
def split_part(fixtures, gpu_ok):
    """part 0 of a committed two-part range-split handle"""
    fx = fixtures("eng2doc")
    a = femto_amd.Index(fx.index, device=0, part=0, nparts=2)
    b = femto_amd.Index(fx.index, device=0, part=1, nparts=2)
    a.split_attach_local(b)
    b.split_attach_local(a)
    a.split_commit()
    b.split_commit()
    yield a
    a.close()
    b.close()


def _refused(call, family):
    with pytest.raises(femto_amd.FemtoAmdError) as e:
        call()
    assert e.value.code == INVALID, family
    assert str(e.value).endswith(": " + REFUSALS[family]), (family, str(e.value))


def test_range_split_part_refuses_every_family(split_part):
    import torch
    a = split_part
    z = torch.zeros(8, dtype=torch.int64, device=DEV)
    z32 = torch.zeros(8, dtype=torch.int32, device=DEV)
    outs = [_full(8) for _ in range(6)] + [_full(8, torch.int32) for _ in range(4)]
    o = [t.data_ptr() for t in outs]
    _refused(lambda: a.doclist_device(1, z.data_ptr(), z.data_ptr(), 8, z.data_ptr(), o[6], o[0], o[7], o[8], o[1], o[2], o[3], o[9]),
             "doclist_device")
    _refused(lambda: a.docpos_device(1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z32.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                     z32.data_ptr(), z32.data_ptr(), z32.data_ptr(), o[4], o[0], o[1], 8, o[5]), "docpos_device")
    q = femto_amd.BooleanQuery(b'"the" AND "of"')
    _refused(lambda: a.bquery_run_batch([q], 10), "bquery_run_batch")
    _refused(lambda: femto_amd.Extractor(a), "Extractor")
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs)


def test_device_forms_answer_an_empty_call(ix):
    import torch
    for name in ("docset_device", "docpos_device", "docpos_documents_device"):
        starts, total, res_a, res_b = _full(4), _full(4), _full(8), _full(8)
        if name == "docset_device":
            ix.docset_device(0, 0, 0, 0, 0, 0, 0, 0, starts.data_ptr(), res_a.data_ptr(), 8, total.data_ptr())
        elif name == "docpos_device":
            ix.docpos_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, starts.data_ptr(), res_a.data_ptr(), res_b.data_ptr(), 8, total.data_ptr())
        else:
            ix.docpos_documents_device(0, 0, 0, starts.data_ptr(), res_a.data_ptr(), 8, total.data_ptr())
        torch.cuda.synchronize()
        assert starts.cpu().tolist() == [0, SENT, SENT, SENT], name
        assert total.cpu().tolist() == [0, 0, SENT, SENT], name
        assert bool((res_a == SENT).all()) and bool((res_b == SENT).all()), name


def test_host_forms_answer_an_empty_call(ix):
    for name, got in (("documents", ix.documents([], 10)), ("docset", ix.docset([], [], [])), ("docpos", ix.docpos([], [], [], [])),
                      ("proximity", ix.proximity([], [], [], [], 10)), ("bquery_run_batch", ix.bquery_run_batch([], 10))):
        assert got[0].tolist() == [0], name
        assert all(len(a) == 0 for a in got[1:]), name


def test_patterns_that_locate_no_row(ix):
    """rows == 0: the walk is skipped, every buffer of `rows` elements is still allocated, the lists are empty"""
    absent = [np.array([6, 7, 8], dtype=np.uint16), np.array([7, 6], dtype=np.uint16)]     # bytes 1 2 3 / 2 1: not in English text
    first, last = ix.count(absent)
    assert (last < first).all()
    ds, docs, hits = ix.documents(absent, 100)
    assert ds.tolist() == [0, 0, 0] and len(docs) == 0 and len(hits) == 0
    rs, rd, ro = ix.proximity(absent, absent[::-1], [dp.WITHIN, dp.OR], [5, 0], 100)
    assert rs.tolist() == [0, 0, 0] and len(rd) == 0 and len(ro) == 0


def test_two_symbol_runs_in_one_pattern_buffer(ix, fixtures):
    """femto_amd_proximity uploads the left symbols and, behind them, the right symbols into one padded buffer: runs of 3 and 2
    symbols, an empty pattern on each side (it takes every row, up to the clamp)"""
    fx = fixtures("eng2doc")
    ends = du.doc_ends(fx.docs)
    left, right = [_enc(b"the"), _enc(b"")], [_enc(b""), _enc(b"an")]
    ops, ds, max_occs = [dp.WITHIN, dp.THEN], [2, 3], 1 << 20
    lists = []
    for batch in (left, right):
        noccs, offs = ix.locate_flat(*femto_amd.flatten(batch), max_occs)
        ost = np.concatenate([[0], np.cumsum(noccs)])
        assert all(noccs > 0)
        lists.append([np.stack(du.resolve(ends, np.sort(offs[ost[k]:ost[k + 1]])), axis=1) for k in range(2)])
    want = dp.batch(lists[0], lists[1], ops, ds)
    assert all(np.diff(want[0]) > 0)
    got = ix.proximity(left, right, ops, ds, max_occs)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
