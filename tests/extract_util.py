"""Test helper: two independent restatements of extraction (include/femto_amd.h "extraction").

(a) do_context_query (src/main/server.c:2567-2795) stepped over the reference's own per-row golden vectors: L[row] going back
    (LF is the inverse of fwd_row), fwd_ch / fwd_row going forward, each walk stopping after the first symbol <= SEOF;
(b) the prepared text T (every document's bytes + 5, then SEOF) and its suffix array (tests/sa_util.py)."""
import numpy as np

from sa_util import suffix_array

SEOF = 2
FIXTURES = ["acgt48k", "b1000", "bytes256", "chunks2doc", "counter400_default", "counter400_small", "eng2doc", "runs3doc",
            "construct_kat"]


class Restated:
    def __init__(self, fx):
        g = fx.gold
        self.L = g["L"].astype(np.int64)
        self.fwd_ch = g["fwd_ch"].astype(np.int64)
        self.fwd_row = g["fwd_row"].astype(np.int64)
        n = len(self.L)
        self.lf = np.full(n, -1, dtype=np.int64)
        ok = self.fwd_row >= 0
        self.lf[self.fwd_row[ok]] = np.nonzero(ok)[0]
        self.T = fx.prepared_text()
        self.N = len(self.T)
        self.sa = suffix_array(self.T)
        self.isa = np.empty(self.N, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.N, dtype=np.int64)
        self.doc_ends = np.cumsum([len(d) + 1 for d in fx.docs]).astype(np.int64)
        # the rows of the documents' SEOFs as construct.c:402-440 records them: rows 0 .. ndocs - 1 (EOF sorts first), each
        # filed under the document its marked offset lies in (golden `off`)
        self.eof_rows_gold = np.zeros(len(fx.docs), dtype=np.int64)
        for r in range(len(fx.docs)):
            o = int(g["off"][r])
            self.eof_rows_gold[int(np.searchsorted(self.doc_ends, o, side="right"))] = r

    # (a)
    def context_rows(self, row, before, after):
        out = np.zeros(before + after, dtype=np.uint16)
        r = row
        for j in range(before):
            c = self.L[r]
            out[before - 1 - j] = c
            if c <= SEOF:
                break
            r = self.lf[r]
        r = row
        for j in range(after):
            c = self.fwd_ch[r]
            out[before + j] = c
            if c <= SEOF:
                break
            r = self.fwd_row[r]
        return out

    # (b)
    def context_text(self, p, before, after):
        out = np.zeros(before + after, dtype=np.uint16)
        if p < 0 or p >= self.N:
            return out
        for j in range(before):
            c = self.T[(p - 1 - j) % self.N]
            out[before - 1 - j] = c
            if c <= SEOF:
                break
        for j in range(after):
            c = self.T[p + j]
            out[before + j] = c
            if c <= SEOF:
                break
        return out

    def context_window(self, p, before, after):
        """the stop rules as one window per anchor: [document start - 1, document end) (tests/test_extract_host.py pins it
        against the stepping restatements)"""
        p = np.asarray(p, dtype=np.int64)
        W = before + after
        out = np.zeros((len(p), W), dtype=np.uint16)
        ok = (p >= 0) & (p < self.N)
        d = np.searchsorted(self.doc_ends, np.where(ok, p, 0), side="right")
        ds = np.where(d > 0, self.doc_ends[np.maximum(d - 1, 0)], 0)
        q = p[:, None] - before + np.arange(W)[None, :]
        valid = ok[:, None] & (q >= (ds - 1)[:, None]) & (q < self.doc_ends[np.minimum(d, len(self.doc_ends) - 1)][:, None])
        out[valid] = self.T[q[valid] % self.N]
        return out

    def extract(self, pos, lens):
        out = []
        for p, n in zip(pos, lens):
            w = np.zeros(int(n), dtype=np.uint16)
            lo, hi = max(int(p), 0), min(int(p) + int(n), self.N)
            if hi > lo:
                w[lo - int(p):hi - int(p)] = self.T[lo:hi]
            out.append(w)
        return np.concatenate(out) if out else np.zeros(0, dtype=np.uint16)

    def document(self, d):
        s = int(self.doc_ends[d - 1]) if d else 0
        return self.T[s:int(self.doc_ends[d])].astype(np.uint16)


def random_requests(N, seed, n=400):
    """seeded (pos, len): empty requests, ranges across documents, the last position, the whole text, positions out of range"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, N, n).astype(np.int64)
    lens = rng.integers(0, min(N, 300) + 1, n).astype(np.int32)
    extra = [(0, 0), (N - 1, 1), (N - 1, 5), (0, N), (-3, 10), (-100, 5), (N, 4), (N + 1000, 3), (N - 2, 9),
             (-(1 << 62), 7), ((1 << 62), 7), (N // 2, 0)]
    pos = np.concatenate([pos, np.array([e[0] for e in extra], dtype=np.int64)])
    lens = np.concatenate([lens, np.array([e[1] for e in extra], dtype=np.int32)])
    return pos, lens
