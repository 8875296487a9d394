"""`-m gpu`: femto_amd_bquery_run_batch and `femto_amd_search --boolean` against tests/bquery_util.py -- the boolean layer in plain
Python over BRUTE-FORCE leaf lists: every occurrence of a leaf's strings in the fixtures' documents, found by searching the text.
Leaves are written as words of a small vocabulary: a plain word is a string; "~word" is `APPROX 1 word`; the words of REGEX are
regular expressions."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bquery_util as bu
import doclist_util as du
import docpos_util as dp
import femto_amd
from femto_amd import build as b
from gpu_common import _open

pytestmark = pytest.mark.gpu

BIG = 1 << 24
REGEX = {"%tha": (rb"th[ae]", "th[ae]"), "%alt": (rb"(ra|oi)[su]", "(ra|oi)[su]")}      # word: (Python's, femto's)


def _find(docs, pat):
    out = []
    for k, d in enumerate(docs):
        at = -1
        while True:
            at = d.find(pat, at + 1)
            if at < 0:
                break
            out.append((k, at))
    return out


def _within_one_edit(s, w):
    """one substitution, insertion or deletion -- but not the deletion of w's FIRST character: the search reads the text
    backwards and ends on a character it consumed, so `femto_search --matches "APPROX 1 teah"` lists "tea", "tah", "Teah" and
    no "eah" (do_regexp_query over compile_regexp.c's automaton; the GPU search is pinned to it by tests/test_regexp.py)"""
    if s == w[1:]:
        return False
    if s == w:
        return True
    if len(s) == len(w):
        return sum(x != y for x, y in zip(s, w)) == 1
    if abs(len(s) - len(w)) != 1:
        return False
    lo, sh = (s, w) if len(s) > len(w) else (w, s)
    return any(lo[:i] + lo[i + 1:] == sh for i in range(len(lo)))


def _matched_strings(docs, full):
    """the strings do_regexp_query reports: walking back from every end position, the first (shortest) string that matches in
    full -- a range with a final state alive is a result and is not extended (tests/test_gpu_cli.py _occurrences)"""
    out = set()
    for d in docs:
        for end in range(1, len(d) + 1):
            for st in range(end - 1, max(-1, end - 12), -1):
                if full(d, st, end):
                    out.add(d[st:end])
                    break
    return out


class Model:
    def __init__(self, fx):
        self.docs = [d.tobytes() for d in fx.docs]
        self.cache, self.raw = {}, {}

    def pairs_of(self, word):
        """the leaf's rows: every occurrence of every string it matches; self.raw[word] keeps them BEFORE the repeats are dropped"""
        if word not in self.cache:
            if word.startswith("~"):
                w = word[1:].encode()
                strings = _matched_strings(self.docs, lambda d, st, end: _within_one_edit(d[st:end], w))
            elif word in REGEX:
                rx = re.compile(REGEX[word][0], re.S)
                strings = _matched_strings(self.docs, lambda d, st, end: rx.fullmatch(d, st, end) is not None)
            else:
                strings = {word.encode()}
            raw = [h for s in sorted(strings) for h in _find(self.docs, s)]
            self.raw[word] = raw
            self.cache[word] = dp.pairs(sorted(set(raw)))
        return self.cache[word]

    @staticmethod
    def leaf_text(word):
        return "APPROX 1 " + word[1:] if word.startswith("~") else REGEX[word][1] if word in REGEX else word

    def want(self, trees):
        return bu.packed([bu.evaluate(t, self.pairs_of) for t in trees])


def _compile(trees, rng=None):
    return [femto_amd.BooleanQuery(bu.to_text(t, rng, Model.leaf_text).encode()) for t in trees]


def _check(got, want, what):
    for g, w, part in zip(got, want, ("res_starts", "res_type", "res_doc", "res_off")):
        assert np.array_equal(g, w), (what, part, g[:20], w[:20])


@pytest.fixture(scope="module")
def eng(fixtures, gpu_ok):
    fx = fixtures("eng2doc")
    ix = _open(fx.index)
    yield fx, ix, Model(fx)
    ix.close()


# ("ytoe" stands in the first document only, "hhsd" in the second only, "zzzzqq" in neither)
HAND = [
    # each of the five operators at the root
    "nhre AND teah", "nhre OR zzzzqq", "nhre NOT ytoe", "nhre THEN 10 teah", "nhre WITHIN 5 teah",
    # depth 3 with mixed types; a left-associative chain
    "(nhre THEN 50 teah) AND (ras OR oiu) NOT hhsd", "((nhre WITHIN 3 ras) OR (teah THEN 40 oiu)) NOT (ilsrte AND ytoe)",
    "nhre AND teah OR ras NOT oiu AND iecs OR hre", "nhre THEN 9 teah THEN 9 ras WITHIN 30 oiu",
    # a leaf with no occurrence on either side of each operator
    "zzzzqq AND nhre", "nhre AND zzzzqq", "zzzzqq OR nhre", "zzzzqq NOT nhre", "nhre NOT zzzzqq", "zzzzqq THEN 5 nhre", "nhre THEN 5 zzzzqq",
    "zzzzqq WITHIN 5 nhre", "nhre WITHIN 5 zzzzqq", "(zzzzqq THEN nhre) OR (nhre WITHIN 2 zzzzqq)",
    # THEN without a number; one leaf; the same leaf on both sides
    "nhre THEN teah", "nhre", "zzzzqq", "nhre WITHIN 4 nhre", "(nhre THEN 4 nhre) OR (nhre WITHIN 4 nhre)",
    # a regular expression, an alternation, APPROX 1 (ranges that overlap), beside strings and under every kind of parent
    "%tha AND nhre", "%tha THEN 20 %alt", "(%alt WITHIN 6 nhre) NOT %tha", "~teah THEN 12 nhre", "~teah OR %alt", "~teah",
    # more rows than one wavefront (64) and than one workgroup (4096) lists
    "e THEN 3 nhre", "(e WITHIN 3 nhre) AND (e OR zzzzqq)", "e WITHIN 2 e",
]


def test_leaf_size_classes_and_repeats(eng):
    fx, ix, m = eng
    wave, group = femto_amd.doclist_info()
    assert wave < len(m.pairs_of("nhre")) < group < len(m.pairs_of("e"))
    # the APPROX leaf reaches one position through two strings ("tea" and "tea?"): without the dedup its list would not be strictly ascending
    m.pairs_of("~teah")
    assert len(m.raw["~teah"]) > len(set(m.raw["~teah"])) == len(m.pairs_of("~teah")) > len(m.pairs_of("teah")) > 0
    assert len(m.pairs_of("zzzzqq")) == 0 and len(m.pairs_of("%tha")) and len(m.pairs_of("%alt"))


def test_hand_picked_queries(eng):
    fx, ix, m = eng
    trees = [bu.parse(t) for t in HAND]
    want = m.want(trees)
    roots = {t[0]: 0 for t in trees if t[0] != "leaf"}
    for k, t in enumerate(trees):
        if t[0] != "leaf" and want[0][k + 1] > want[0][k]:
            roots[t[0]] += 1
    assert all(roots[op] for op in (bu.AND, bu.OR, bu.NOT, bu.THEN, bu.WITHIN)), roots
    qs = _compile(trees)
    assert [q.result_type for q in qs] == want[1].tolist()
    _check(ix.bquery_run_batch(qs, BIG), want, "all at once")
    # batches of 1 and of 2
    for k in (0, 3, 5, 20, 21, 27, 29):
        _check(ix.bquery_run_batch(qs[k:k + 1], BIG), m.want(trees[k:k + 1]), HAND[k])
    _check(ix.bquery_run_batch(qs[5:7], BIG), m.want(trees[5:7]), "two")
    _check(ix.bquery_run_batch(qs[26:28], BIG), m.want(trees[26:28]), "two with automata")
    _check(ix.bquery_run_batch([], BIG), m.want([]), "none")


VOCAB = ["nhre", "teah", "ras", "oiu", "hnrino", "ygezcgmso", "ilsrte", "eoo", "iecs", "hre", "zzzzqq", "%tha", "%alt", "~teah"]


def _random_batch(n=300, seed=5):
    rng = np.random.default_rng(seed)
    return [bu.random_tree(rng, int(rng.integers(1, 8)), VOCAB) for _ in range(n)], rng


def test_random_batch_in_one_call(eng):
    fx, ix, m = eng
    trees, rng = _random_batch()
    want = m.want(trees)
    sizes = np.diff(want[0])
    # the model alone says the batch is worth running
    assert (sizes > 0).sum() * 4 >= len(trees)
    for op in (bu.AND, bu.OR, bu.NOT, bu.THEN, bu.WITHIN):
        assert any(t[0] == op and sizes[k] > 0 for k, t in enumerate(trees)), bu.NAMES[op]
    fams = {}
    for t in trees:
        for h, f in bu.levels(t).items():
            fams.setdefault(h, set()).update(f)
    assert any(f == {"docset", "docpos"} for f in fams.values()) and max(fams) >= 4
    assert {bu.DOCUMENTS, bu.PAIRS} == set(want[1].tolist())
    _check(ix.bquery_run_batch(_compile(trees, rng), BIG), want, "300 trees")


def _leaf_words(tree):
    return [tree[1]] if tree[0] == "leaf" else _leaf_words(tree[2]) + _leaf_words(tree[3])


def test_more_queries_than_workgroups(eng):
    """One batch in which the persistent grids of the boolean layer (at most eight workgroups per CU) go round more than once:
    more queries than bq_gather_kernel has workgroups, more than twice the located rows one pass of the segmented unique holds,
    and a level with more set-operation jobs than docset_kernel has workgroups.  Sized from the device's CU count."""
    import torch
    fx, ix, m = eng
    C = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(21)
    trees = [bu.random_tree(rng, int(rng.integers(1, 4)), VOCAB) for _ in range(8 * C + 200)]
    plain = [w for w in VOCAB if w[0] not in "%~"]
    trees += [bu.parse("e WITHIN 2 " + plain[k % len(plain)]) for k in range(40)]

    def jobs(ts):
        """{(height, family): jobs}: a tree of at most three leaves has at most one operator of a height"""
        n = {}
        for t in ts:
            for h, fams in bu.levels(t).items():
                for f in fams:
                    n[(h, f)] = n.get((h, f), 0) + 1
        return n

    def rows(ts):
        return sum(len(m.raw[w]) for t in ts for w in _leaf_words(t))

    for w in VOCAB + ["e"]:
        m.pairs_of(w)
    need_rows = 2 * 256 * 8 * C
    either = bu.parse("~teah OR e")
    assert bu.levels(either) == {1: {"docset"}} and rows([either]) > 0
    more = max(8 * C + 1 - jobs(trees).get((1, "docset"), 0), 50, -(-(need_rows + 1 - rows(trees)) // rows([either])))
    trees += [either] * more
    trees = [trees[k] for k in rng.permutation(len(trees))]
    assert all(len(_leaf_words(t)) <= 3 for t in trees) and len(trees) > 8 * C
    assert rows(trees) > need_rows
    assert sum(_leaf_words(t).count("~teah") for t in trees) >= 50
    per_level = jobs(trees)
    assert per_level[(1, "docset")] > 8 * C and per_level[(1, "docpos")] > 300, per_level
    want = m.want(trees)
    assert (np.diff(want[0]) > 0).sum() * 4 >= len(trees) and {bu.DOCUMENTS, bu.PAIRS} == set(want[1].tolist())
    _check(ix.bquery_run_batch(_compile(trees, rng), BIG), want, "%d trees" % len(trees))


@pytest.mark.parametrize("name,vocab", [("chunks2doc", ["ffc", "afb", "hbhg", "feed", "b", "e ", "zzq"]), ("runs3doc", ["aaaa", "ab", "ba", "bb", "c", "zzq"])])
def test_other_fixtures(fixtures, gpu_ok, name, vocab):
    fx = fixtures(name)
    m = Model(fx)
    rng = np.random.default_rng(11)
    trees = [bu.random_tree(rng, int(rng.integers(1, 6)), vocab) for _ in range(60)]
    want = m.want(trees)
    assert (np.diff(want[0]) > 0).sum() * 4 >= len(trees)
    quote = lambda w: "'" + w + "'"                       # (a blank inside a leaf has to be quoted)
    qs = [femto_amd.BooleanQuery(bu.to_text(t, rng, quote).encode()) for t in trees]
    ix = _open(fx.index)
    try:
        _check(ix.bquery_run_batch(qs, BIG), want, name)
    finally:
        ix.close()


def test_clamp(eng):
    """max_occs_each = 3: the operators applied to the rows that were located -- the rows femto_amd_locate_flat returns under the
    same clamp, whose documents are femto_amd_doclist's on the same handle"""
    fx, ix, m = eng
    words = ["nhre", "teah", "ras", "oiu", "hnrino", "ytoe", "zzzzqq"]
    enc = lambda s: np.frombuffer(s.encode(), dtype=np.uint8).astype(np.uint16) + 5
    plen, flat, starts = femto_amd.flatten([enc(w) for w in words])
    noccs, offs = ix.locate_flat(plen, flat, starts, 3)
    ost = np.concatenate([[0], np.cumsum(noccs)])
    ends = du.doc_ends(fx.docs)
    clamped = {}
    for k, w in enumerate(words):
        d, o = du.resolve(ends, np.sort(offs[ost[k]:ost[k + 1]]))
        clamped[w] = np.stack([d, o], axis=1)
    assert any(0 < len(clamped[w]) < len(m.pairs_of(w)) for w in words)
    doc_starts, docs, _ = ix.documents([enc(w) for w in words], 3)
    for k, w in enumerate(words):
        assert np.array_equal(docs[doc_starts[k]:doc_starts[k + 1]], np.unique(clamped[w][:, 0])), w
    rng = np.random.default_rng(3)
    trees = [bu.parse(t) for t in HAND[:5]] + [bu.random_tree(rng, int(rng.integers(1, 6)), words, distances=(40, 400, 4000, bu.INT_MAX)) for _ in range(40)]
    want = bu.packed([bu.evaluate(t, lambda w: clamped[w]) for t in trees])
    assert len(want[2])
    _check(ix.bquery_run_batch(_compile(trees), 3), want, "clamped")


def _cli(args):
    return subprocess.run([b.SEARCH] + list(args), capture_output=True, timeout=300)


def test_search_cli_boolean(fixtures, gpu_ok):
    b.build_tools()
    fx = fixtures("eng2doc")
    m = Model(fx)
    infos = [os.path.basename(p).encode() for p in fx.doc_paths]
    q = "the THEN 10 of"
    for text in (q, "nhre THEN 10 teah", "(nhre WITHIN 5 teah) OR (the THEN 200 of)"):
        t, res = bu.evaluate(bu.parse(text), m.pairs_of)
        assert t == bu.PAIRS and (text == q or len(res))
        by_doc = [(d, [int(o) for dd, o in res.tolist() if dd == d]) for d in sorted(set(res[:, 0].tolist()))]
        r = _cli(["--boolean", "--offsets", fx.index, text])
        assert r.returncode == 0 and r.stdout == b"".join(infos[d] + b"\n\t" + b"".join(b" %d" % o for o in offs) + b"\n" for d, offs in by_doc), (r.stdout[:300], r.stderr)
        assert _cli(["--boolean", fx.index, text]).stdout == b"".join(infos[d] + b"\n" for d, _ in by_doc)
        j = json.loads(_cli(["--boolean", "--offsets", "--json", fx.index, text]).stdout)
        assert j["results"] == [[[infos[d].decode()], offs] for d, offs in by_doc], text
        assert j["pattern"] == femto_amd.BooleanQuery(text.encode()).echo.decode() and (text != q or j["pattern"] == '"the" THEN 10 "of"')
    # a document-typed result prints without offsets even with --offsets
    t, res = bu.evaluate(bu.parse("the AND of"), m.pairs_of)
    assert t == bu.DOCUMENTS and len(res)
    assert _cli(["--boolean", "--offsets", fx.index, "the AND of"]).stdout == b"".join(infos[d] + b"\n" for d in res.tolist())
    # a pattern without an operator goes on as it always has
    assert _cli(["--boolean", "--count", fx.index, "the"]).stdout == _cli(["--count", fx.index, "the"]).stdout != b""
    for flag in ("--count", "--matches"):
        r = _cli(["--boolean", flag, fx.index, q])
        assert r.returncode != 0 and flag.encode() in r.stderr and b"boolean" in r.stderr, (flag, r.stderr)
    r = _cli(["--boolean", fx.index, "(the THEN of) OR x"])
    assert r.returncode != 0 and b"Could not parse pattern" in r.stderr and b"type error" in r.stderr
    r = _cli([fx.index, q])
    assert r.returncode != 0 and b"Could not parse pattern" in r.stderr + r.stdout
