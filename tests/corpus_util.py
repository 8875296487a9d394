"""Test helper: three corpora built from seeded numpy generators, for the tests that need more documents than a golden fixture
holds.  Nothing here touches the library: the documents are plain uint8 arrays, and the tests build their indexes from them in
module-scoped fixtures (femto_amd.build_index), as tests/test_gpu_doclist.py does.

  edges_docs()     "edges", for matching lines: hundreds of tiny and empty documents, single lines at the sizes where the scan of
                   lines.hip changes its round or runs out, terminators at exact distances, \\r, \\0.
  dna_docs()       "dna", for extraction on the packed 3-bit lines: hundreds of tiny and empty documents over ACGT and two long
                   ones; the first document is not empty and the last one is ("edges": the other way round).
  library_docs()   "library", for common sequences: hundreds of short documents over a 20-letter alphabet with planted passages
                   that occur in exactly 1, 2, 64, 65, 150 and 300 of them.
  library_query()  the query of the "library" tests."""
import numpy as np

# ---- "edges" --------------------------------------------------------------------------------------------------------------------

SINGLE_LINES = (15, 16, 17, 255, 256, 257, 1022, 1023, 1024, 1025, 2046, 2047, 2048)
TERMINATORS = (10, 13, 0)
DISTANCES = (255, 256, 257, 1022, 1023, 1024)
TINY, EDGE_RANDOM = 300, 480


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def edges_docs():
    """[uint8 array] in the order of the module's docstring: 300 tiny documents (lengths 0, 1, .., 17 in turn), the single lines,
    x*d + t + y*d for every terminator t and distance d, five special documents, random documents of 1..90 bytes"""
    rng = np.random.default_rng(20250711)
    abn = _u8(b"ab\n")
    letters = np.arange(ord("c"), ord("z") + 1, dtype=np.uint8)
    docs = [abn[rng.integers(0, 3, i % 18)] for i in range(TINY)]
    docs += [letters[rng.integers(0, len(letters), L)] for L in SINGLE_LINES]
    for t in TERMINATORS:
        for d in DISTANCES:
            docs.append(_u8(b"x" * d + bytes([t]) + b"y" * d))
    long_line = letters[rng.integers(0, len(letters), 3000)]
    long_line[1500] = 0
    docs += [_u8(b"\n"), _u8(b"\0"), _u8(b"\r\n\r\n"), _u8(b"\nstarts with a newline and ends with a return\r"), long_line]
    docs += [abn[rng.integers(0, 3, int(rng.integers(1, 91)))] for _ in range(EDGE_RANDOM)]
    return docs


# ---- "dna" ----------------------------------------------------------------------------------------------------------------------

DNA_TINY, DNA_RANDOM, DNA_LONG = 500, 300, (3000, 5000)


def dna_docs():
    """[uint8 array]: 250 tiny documents (lengths 1, 2, .., 17, 0 in turn), a document of 3000 bytes, 250 more tiny ones, random
    documents of 1..50 bytes with a document of 5000 bytes among them, one empty document"""
    rng = np.random.default_rng(20250714)
    acgt = _u8(b"ACGT")
    text = lambda n: acgt[rng.integers(0, 4, n)]
    tiny = [text((i + 1) % 18) for i in range(DNA_TINY)]
    rand = [text(int(rng.integers(1, 51))) for _ in range(DNA_RANDOM)]
    docs = tiny[:DNA_TINY // 2] + [text(DNA_LONG[0])] + tiny[DNA_TINY // 2:] + rand[:100] + [text(DNA_LONG[1])] + rand[100:]
    return docs + [text(0)]


class Corpus:
    """what tests/lines_util.Lines and the fixtures read of a committed fixture: the documents, and where its index stands"""

    def __init__(self, docs, index=None):
        self.docs = docs
        self.index = index


# ---- "library" ------------------------------------------------------------------------------------------------------------------

ALPHABET20 = np.frombuffer(b"abcdefghijklmnopqrst", dtype=np.uint8)
PASSAGE_LENS = (24, 31, 40, 47, 53, 60)
PASSAGE_DOCS = (1, 2, 64, 65, 150, 300)          # P1 .. P6 occur in exactly this many documents
PURE = (2, 2, 4, 4, 5)                           # the documents that ARE a passage and nothing else (indexes into the passages)
ORDINARY = 500
MAX_PLANTED = 185


class Library:
    """docs: [bytes]; passages: [bytes]; twice[k]: the documents that hold passage k twice; pure: the documents that are a
    passage and nothing else; twins: two byte-identical documents without a passage"""


def library_docs():
    rng = np.random.default_rng(20250712)
    noise = lambda n: bytes(ALPHABET20[rng.integers(0, 20, n)])
    lib = Library()
    lib.passages = [noise(n) for n in PASSAGE_LENS]
    items = [[] for _ in range(ORDINARY)]          # the passages every ordinary document holds
    planted = np.zeros(ORDINARY, dtype=np.int64)
    lib.twice = [[] for _ in PASSAGE_LENS]
    for k in reversed(range(len(PASSAGE_LENS))):          # the most frequent first: the rare ones go where there is room left
        n = PASSAGE_LENS[k]
        room = np.nonzero(planted + n <= MAX_PLANTED)[0]
        chosen = rng.choice(room, PASSAGE_DOCS[k] - PURE.count(k), replace=False)
        for d in chosen:
            items[d].append(k)
            planted[d] += n
        if PASSAGE_DOCS[k] >= 64:          # ... and a second time in up to five of them
            for d in chosen:
                if len(lib.twice[k]) < 5 and planted[d] + n <= MAX_PLANTED:
                    items[d].append(k)
                    planted[d] += n
                    lib.twice[k].append(int(d))
    docs = []
    for d in range(ORDINARY):
        order = [items[d][i] for i in rng.permutation(len(items[d]))]
        gaps = len(order) + 1          # noise in front, between and behind: at least one byte each
        total = max(int(rng.integers(12, 201)), int(planted[d]) + gaps)
        cut = np.sort(rng.integers(0, total - int(planted[d]) - gaps + 1, gaps - 1))
        sizes = np.diff(np.concatenate([[0], cut, [total - int(planted[d]) - gaps]])) + 1
        parts = [noise(int(sizes[0]))]
        for i, k in enumerate(order):
            parts += [lib.passages[k], noise(int(sizes[i + 1]))]
        docs.append(b"".join(parts))
        assert 12 <= len(docs[-1]) <= 200
    lib.pure = list(range(len(docs), len(docs) + len(PURE)))
    docs += [lib.passages[k] for k in PURE]
    twin = noise(90)
    lib.twins = [len(docs), len(docs) + 1]
    docs += [twin, twin]
    # the special documents move to seeded places among the others, so that a tie is not a tie of neighbours at the end
    perm = rng.permutation(len(docs))
    where = np.argsort(perm)
    lib.docs = [docs[i] for i in perm]
    lib.pure = sorted(int(where[i]) for i in lib.pure)
    lib.twins = sorted(int(where[i]) for i in lib.twins)
    lib.twice = [sorted(int(where[i]) for i in t) for t in lib.twice]
    return lib


def library_query(lib):
    """about 2.4 KB: slices of 40 documents (both twins among them), every passage -- P3 and P5 twice --, noise between them;
    pieces[38:] are the twins' slices and the passages"""
    rng = np.random.default_rng(20250713)
    noise = lambda n: bytes(ALPHABET20[rng.integers(0, 20, n)])
    long_enough = [d for d, b in enumerate(lib.docs) if len(b) >= 60 and d not in lib.twins]
    chosen = [int(d) for d in rng.choice(long_enough, 38, replace=False)] + lib.twins
    pieces = []
    for d in chosen:
        b = lib.docs[d]
        if d in lib.twins:
            pieces.append(b[20:70])          # the same slice of both: equal numerators over equal lengths
        else:
            n = int(rng.integers(30, 51))
            at = int(rng.integers(0, len(b) - n + 1))
            pieces.append(b[at:at + n])
    pieces += list(lib.passages) + [lib.passages[2], lib.passages[4]]
    parts = []
    for i in rng.permutation(len(pieces)):
        # a byte no document holds on either side of the twins' slices and the passages: no match grows out of them into the
        # noise, so every passage is a sequence itself and the two copies of P3, of P5 and of the twins' slice are the SAME one
        fence = b"." if i >= 38 else b""
        parts += [fence, pieces[i], fence, noise(int(rng.integers(5, 16)))]
    return b"".join(parts)
