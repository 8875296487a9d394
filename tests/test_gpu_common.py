"""gpu_common.compare, the one check behind every GPU parity test: a fixture's goldens pass, and each single corruption fails."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_common import Chain, compare, want_from_golden


def test_compare_catches_every_single_corruption():
    want = want_from_golden(np.load(os.path.join(GOLDEN, "eng2doc.npz")))
    k = [mo for mo, _, _ in want.locate].index(7)
    _, noccs, offs = want.locate[k]
    cap = len(offs) + 16
    chain = Chain(want.first.copy(), want.last.copy(), noccs.copy(), np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)]),
                  offs.copy(), len(offs), 0)
    leaves = {key: v.copy() for key, v in want.leaves.items()}

    def bump(a, i=3):
        a = a.copy()
        a[i] += 1
        return a

    compare(want, ("unit",), k, count=(want.first, want.last), located=(noccs, offs), chain=chain, capacity=cap, leaves=leaves)
    compare(want, k=k, chain=chain._replace(offsets=offs[:5], overflow=1), capacity=5)        # a buffer that cuts the output short
    nz = int(np.flatnonzero(noccs)[0])
    for field, bad in (("first", bump(chain.first)), ("last", bump(chain.last)), ("noccs", bump(noccs, nz)), ("offsets", bump(offs, 0)),
                       ("offsets", offs[:-1]), ("out_starts", bump(chain.out_starts)), ("total", chain.total + 1), ("overflow", 1)):
        with pytest.raises(AssertionError):
            compare(want, k=k, chain=chain._replace(**{field: bad}), capacity=cap)
        if field in ("first", "last"):       # ... and through the host forms
            with pytest.raises(AssertionError):
                compare(want, count=(bad, want.last) if field == "first" else (want.first, bad))
        elif field in ("noccs", "offsets"):
            with pytest.raises(AssertionError):
                compare(want, k=k, located=(bad, offs) if field == "noccs" else (noccs, bad))
    for key in ("L", "occ", "off"):
        with pytest.raises(AssertionError):
            compare(want, leaves=dict(leaves, **{key: bump(leaves[key])}))
