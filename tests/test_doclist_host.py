"""Document listing without a GPU: the library exports the new entry points, a parse-only handle refuses them cleanly, and the
numpy restatement the GPU tests compare with resolves every golden located offset as the reference did."""
import os

import numpy as np
import pytest

import femto_amd
import doclist_util as du
from conftest import GOLDEN

NEW_SYMBOLS = ["femto_amd_doclist_info", "femto_amd_doclist_device", "femto_amd_docset_device", "femto_amd_doclist", "femto_amd_docset"]


def test_library_exports_the_doclist_symbols():
    lib = femto_amd.lib()
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    w, g = femto_amd.doclist_info()
    assert 1 <= w < g
    assert (femto_amd.DOCSET_AND, femto_amd.DOCSET_OR, femto_amd.DOCSET_NOT) == (du.AND, du.OR, du.NOT)


def test_parse_only_handle_refuses_documents(fixtures):
    ix = femto_amd.Index(fixtures("eng2doc").index, device=-1)
    pat = [np.frombuffer(b"the", dtype=np.uint8).astype(np.uint16) + 5]
    with pytest.raises(femto_amd.FemtoAmdError) as e:
        ix.documents(pat, 10)
    assert e.value.code == 6                        # FEMTO_AMD_ERR_INVALID
    with pytest.raises(femto_amd.FemtoAmdError) as e:
        ix.docset([[1, 2]], [[2]], [du.AND])
    assert e.value.code == 6
    ix.close()


@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc", "runs3doc"])
def test_restatement_resolves_like_the_reference(fixtures, name):
    """resolve_golden.npz holds the reference's (document, offset in document) of EVERY text offset of these fixtures"""
    G = np.load(os.path.join(GOLDEN, "resolve_golden.npz"))
    fx = fixtures(name)
    ends = du.doc_ends(fx.docs)
    assert np.array_equal(np.diff(np.concatenate([[0], ends])), G[name + "_len"])
    held = len(G[name + "_doc"])
    cases = list(fx.locate_cases())
    assert cases
    for mo, noccs, offs in cases:
        offs = offs.astype(np.int64)
        assert ((offs >= 0) & (offs < held)).all(), (name, mo)
        doc, off = du.resolve(ends, offs)
        assert np.array_equal(doc, G[name + "_doc"][offs]), (name, mo)
        assert np.array_equal(off, G[name + "_off"][offs]), (name, mo)
        # and the listing built on it: every pattern's documents ascend, their hits add up to its rows
        out_starts = np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)])
        want = du.listing(ends, offs, out_starts)
        ds, docs, hits = du.packed(want, out_starts)
        assert np.array_equal([hits[ds[i]:ds[i + 1]].sum() for i in range(len(noccs))], noccs)
        assert all((np.diff(docs[ds[i]:ds[i + 1]]) > 0).all() for i in range(len(noccs)))


def test_set_operations_restated():
    a, b = [1, 3, 5, 9], [3, 4, 9, 11]
    assert du.setop(a, b, du.AND).tolist() == [3, 9]
    assert du.setop(a, b, du.OR).tolist() == [1, 3, 4, 5, 9, 11]
    assert du.setop(a, b, du.NOT).tolist() == [1, 5]
    st, r = du.setops([a, [], a], [b, b, []], [du.NOT, du.OR, du.AND])
    assert st.tolist() == [0, 2, 6, 6] and r.tolist() == [1, 5, 3, 4, 9, 11]
