"""Test helper: two independent restatements of extraction (include/femto_amd.h "extraction").

(a) do_context_query (src/main/server.c:2567-2795) stepped over the reference's own per-row golden vectors: L[row] going back
    (LF is the inverse of fwd_row), fwd_ch / fwd_row going forward, each walk stopping after the first symbol <= SEOF;
(b) the prepared text T (every document's bytes + 5, then SEOF) and its suffix array (tests/sa_util.py)."""
import numpy as np

from sa_util import suffix_array

SEOF = 2
FIXTURES = ["acgt48k", "b1000", "bytes256", "chunks2doc", "counter400_default", "counter400_small", "eng2doc", "runs3doc",
            "construct_kat"]


class TextRestated:
    """(b) alone, from the documents: what a corpus without golden vectors (tests/corpus_util.py) can be checked against"""

    def __init__(self, docs):
        docs = [np.frombuffer(bytes(d), dtype=np.uint8) for d in docs]          # (bytes or uint8 arrays)
        parts = []
        for d in docs:          # the prepared text: every document's bytes + 5, then SEOF
            parts += [d.astype(np.uint16) + 5, np.array([SEOF], dtype=np.uint16)]
        self._init_text(np.concatenate(parts), docs)

    def _init_text(self, T, docs):
        self.T = T
        self.N = len(self.T)
        self.sa = suffix_array(self.T)
        self.isa = np.empty(self.N, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.N, dtype=np.int64)
        self.doc_ends = np.cumsum([len(d) + 1 for d in docs]).astype(np.int64)
        self.eof_rows = self.isa[self.doc_ends - 1]          # the rows of the documents' SEOFs

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


class Restated(TextRestated):
    def __init__(self, fx):
        g = fx.gold
        self.L = g["L"].astype(np.int64)
        self.fwd_ch = g["fwd_ch"].astype(np.int64)
        self.fwd_row = g["fwd_row"].astype(np.int64)
        n = len(self.L)
        self.lf = np.full(n, -1, dtype=np.int64)
        ok = self.fwd_row >= 0
        self.lf[self.fwd_row[ok]] = np.nonzero(ok)[0]
        self._init_text(fx.prepared_text(), fx.docs)
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


def _extras(N):
    """the last position, the whole text, positions out of range on both sides and at +-2^62, empty requests"""
    return [(0, 0), (N - 1, 1), (N - 1, 5), (0, N), (-3, 10), (-100, 5), (N, 4), (N + 1000, 3), (N - 2, 9),
            (-(1 << 62), 7), ((1 << 62), 7), (N // 2, 0)]


def _requests(parts):
    pos = np.concatenate([np.asarray(p, dtype=np.int64) for p, _ in parts])
    lens = np.concatenate([np.asarray(n, dtype=np.int32) for _, n in parts])
    return pos, lens


def random_requests(N, seed, n=400):
    """seeded (pos, len): empty requests, ranges across documents, the last position, the whole text, positions out of range"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, N, n).astype(np.int64)
    lens = rng.integers(0, min(N, 300) + 1, n).astype(np.int32)
    extra = _extras(N)
    return _requests([(pos, lens), ([e[0] for e in extra], [e[1] for e in extra])])


ZERO_RUN = 300          # the least run of empty requests in crowded_requests


def crowded_requests(N, seed, n=12000):
    """n requests of 0, 0, 1 or 2 symbols -- thousands of them in one 2048-symbol tile of the packed output -- with runs of
    ZERO_RUN .. 2 * ZERO_RUN empty requests at the start, at the end and at seeded places between; the extras stand in front of
    the last run, so that the batch begins and ends inside a run"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(-2, N + 2, n).astype(np.int64)
    lens = np.array([0, 0, 1, 2], dtype=np.int32)[rng.integers(0, 4, n)]
    lens[:ZERO_RUN] = 0
    for at in rng.integers(ZERO_RUN, n - 3 * ZERO_RUN, 6):
        lens[at:at + int(rng.integers(ZERO_RUN, 2 * ZERO_RUN + 1))] = 0
    extra = _extras(N)
    tail = (rng.integers(0, N, ZERO_RUN), np.zeros(ZERO_RUN, dtype=np.int32))
    return _requests([(pos, lens), ([e[0] for e in extra], [e[1] for e in extra]), tail])


def all_empty_requests(N, seed, n=500):
    """n requests of length 0 and the extras' positions, out of range included, with length 0 too: a call whose total is 0"""
    rng = np.random.default_rng(seed)
    extra = _extras(N)
    return _requests([(rng.integers(0, N, n), np.zeros(n, dtype=np.int32)), ([e[0] for e in extra], np.zeros(len(extra), dtype=np.int32))])


def long_requests(N, seed, n=200):
    """the whole text, the whole text and more on both sides, 6000 symbols of which the last 3000 lie behind the text -- each
    dozens of 2048-symbol tiles of the packed output -- at seeded places among n requests of 0 .. 40 symbols"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, N, n).astype(np.int64)
    lens = rng.integers(0, 41, n).astype(np.int32)
    at = np.sort(rng.choice(np.arange(1, n - 1), 3, replace=False))
    for k, (p, m) in zip(at, [(0, N), (-5, N + 10), (N - 3000, 6000)]):
        pos[k], lens[k] = p, m
    extra = _extras(N)
    return _requests([(pos, lens), ([e[0] for e in extra], [e[1] for e in extra])])


def packed_starts(lens):
    """cum[r]: where request r begins in the packed output (n + 1 entries)"""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64).clip(0))])
