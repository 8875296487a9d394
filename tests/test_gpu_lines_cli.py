"""`-m gpu`: femto_amd_search --lines / --multilines (the reference's --grep / --multigrep output, served from the index) in
text, --null and --json form, for a literal and a regular expression, against the output formatted in python from the
restatement of tests/lines_util.py; the reference's own options stay refused."""
import os
import re
import subprocess

import pytest

import testpl
from femto_amd import build as b
from lines_util import Lines, format_lines, format_multilines

pytestmark = pytest.mark.gpu

JSON_HEAD = b'",\n "results":[\n   '


@pytest.fixture(scope="module")
def gpu_ok():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    b.build_tools()
    return True


def _run(args):
    return subprocess.run([b.SEARCH] + list(args), capture_output=True, timeout=300)


def _hits(docs, regex):
    """(doc, offset) of every match start, as --offsets lists them: per end position the shortest string that matches in full"""
    out = set()
    for di, d in enumerate(docs):
        for end in range(1, len(d) + 1):
            for st in range(end - 1, max(-1, end - 8), -1):
                if regex.fullmatch(d, st, end):
                    out.add((di, st))
                    break
    return sorted(out)


@pytest.mark.parametrize("name", ["eng2doc", "chunks2doc"])
def test_lines_and_multilines(fixtures, gpu_ok, name):
    fx = fixtures(name)
    L = Lines(fx)
    docs = [d.tobytes() for d in fx.docs]
    infos = [os.path.basename(p).encode() for p in fx.doc_paths]
    doclens = [len(d) for d in docs]
    literal = docs[0][40:43]
    rx = {"eng2doc": b"t[aeiou]n", "chunks2doc": b"[ae]b[c-f]"}[name]
    for query, regex in ((testpl.x_escaped(literal), re.compile(re.escape(literal), re.S)), (rx, re.compile(rx, re.S))):
        hits = _hits(docs, regex)
        assert hits, query
        anchored = [(d, int(L.doc_starts[d]) + o) for d, o in hits]
        r = _run(["--offsets", fx.index, query])
        assert r.returncode == 0 and sum(len(l.split()) for l in r.stdout.split(b"\n") if l.startswith(b"\t")) == len(hits)
        for flag, fmt in (("--lines", format_lines), ("--multilines", format_multilines)):
            r = _run([flag, fx.index, query])
            assert r.returncode == 0 and r.stdout == fmt(anchored, infos, doclens, L), (flag, query, r.stdout[:300], r.stderr)
            r = _run([flag, "--null", fx.index, query])
            assert r.returncode == 0 and r.stdout == fmt(anchored, infos, doclens, L, sep=b"\0"), (flag, query, r.stderr)
            r = _run([flag, "--json", fx.index, query])
            want = fmt(anchored, infos, doclens, L, json=True)
            assert r.returncode == 0 and r.stdout.startswith(b'{\n "pattern":"') and JSON_HEAD in r.stdout
            assert r.stdout.split(JSON_HEAD, 1)[1] == want.split(JSON_HEAD, 1)[1], (flag, query, r.stdout[:300])
    # no hit: nothing but the wrapper
    r = _run(["--lines", fx.index, b"zzzzqqq"])
    assert r.returncode == 0 and r.stdout == b""


def test_reference_options_stay_refused(fixtures, gpu_ok):
    fx = fixtures("eng2doc")
    for opt in ("--grep", "--multigrep", "--grepdir", "--suggest"):
        r = _run([opt, fx.index, "the"])
        assert r.returncode == 255 and ("%s is not supported" % opt).encode() in r.stderr
    r = _run(["--boolean", "--lines", fx.index, "the AND of"])
    assert r.returncode == 255 and b"--lines is not supported with the boolean operators" in r.stderr
