"""The rule of include/femto_amd.h "common sequences", restated in plain Python over the documents' bytes (what
Fixture.prepared_text() concatenates: a match never crosses a document's SEOF): matching statistics by the amortised rule, the
selection of maximal sequences, the distinct sequences keyed by THEIR BYTES (the library keys them by (len, first): that rule is
under test), and the scores from brute-force occurrence lists."""
import numpy as np

MIN_LEN, MAX_OCCS, MAX_PATTERN = 8, 100, 32768


def as_bytes(q):
    return bytes(np.ascontiguousarray(q, dtype=np.uint8)) if not isinstance(q, (bytes, bytearray)) else bytes(q)


class Text:
    """the documents of a fixture (or any list of byte strings)"""

    def __init__(self, docs):
        self.docs = [as_bytes(d) for d in docs]
        self.doc_starts = np.cumsum([0] + [len(d) + 1 for d in self.docs])[:-1]      # in the prepared text: one SEOF per document
        self.total_length = int(sum(len(d) + 1 for d in self.docs))

    def occurs(self, s):
        return any(s in d for d in self.docs)

    def occurrences(self, s):
        """[(document, offset in document)] of every occurrence, overlapping ones included"""
        out = []
        for k, d in enumerate(self.docs):
            at = d.find(s)
            while at >= 0:
                out.append((k, at))
                at = d.find(s, at + 1)
        return out

    def hits(self, s):
        """{document: occurrences}"""
        h = {}
        for k, _ in self.occurrences(s):
            h[k] = h.get(k, 0) + 1
        return h


def match_lengths(text, q, max_len=0):
    """len[j] = the largest l <= min(j + 1, max_len) with q[j - l + 1 .. j] in some document: try len[j - 1] + 1, shrink until found"""
    q = as_bytes(q)
    cap = MAX_PATTERN if max_len <= 0 else max_len
    out = np.zeros(len(q), dtype=np.int32)
    prev = 0
    for j in range(len(q)):
        cur = min(prev + 1, j + 1, cap)
        while cur > 0 and not text.occurs(q[j - cur + 1:j + 1]):
            cur -= 1
        out[j] = prev = cur
    return out


def select(lens, min_len=0):
    """the end positions whose match is not contained in the next one's"""
    m = MIN_LEN if min_len <= 0 else min_len
    n = len(lens)
    return [j for j in range(n) if lens[j] >= m and (j == n - 1 or lens[j + 1] <= lens[j])]


class Group:
    def __init__(self, s):
        self.bytes, self.len, self.starts = s, len(s), []

    @property
    def here(self):
        return len(self.starts)

    @property
    def min_start(self):
        return min(self.starts)

    @property
    def pattern(self):
        return np.frombuffer(self.bytes, dtype=np.uint8).astype(np.uint16) + 5


def groups_of(q, lens, min_len=0):
    """(sequences [(start, len)] in ascending end position, groups ordered by length descending then by their bytes -- the order of
    `first` among strings of one length --, group_of[k])"""
    q = as_bytes(q)
    seqs = [(j - int(lens[j]) + 1, int(lens[j])) for j in select(lens, min_len)]
    by = {}
    for s, l in seqs:
        by.setdefault(q[s:s + l], Group(q[s:s + l])).starts.append(s)
    groups = sorted(by.values(), key=lambda g: (-g.len, g.bytes))
    where = {g.bytes: i for i, g in enumerate(groups)}
    return seqs, groups, [where[q[s:s + l]] for s, l in seqs]


def index_numerator(text, groups, kept=None):
    return sum(g.len * min(g.here, len(text.occurrences(g.bytes))) for i, g in enumerate(groups) if kept is None or kept[i])


def document_scores(ndocs, groups, hits_of, kept=None):
    """(score numerator int64[ndocs], sequences int32[ndocs]) from hits_of(g) = {document: located occurrences}"""
    score, seqs = np.zeros(ndocs, dtype=np.int64), np.zeros(ndocs, dtype=np.int32)
    for i, g in enumerate(groups):
        if kept is not None and not kept[i]:
            continue
        for d, h in hits_of(g).items():
            score[d] += g.len * min(g.here, h)
            seqs[d] += 1
    return score, seqs


def ranked(text, n, score, seqs):
    """[(doc, numerator, sequences, numerator / min(n, document bytes))], best first, then by document"""
    rows = []
    for d in np.nonzero(score)[0]:
        dl = len(text.docs[d])
        rows.append((int(d), int(score[d]), int(seqs[d]), float(score[d]) / float(dl if 0 < dl < n else n)))
    return sorted(rows, key=lambda r: (-r[3], r[0]))
