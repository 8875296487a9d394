#!/usr/bin/env python3
"""Golden vectors of automaton search for LARGE automata from the GENUINE do_regexp_query (container only).

    python tests/golden/make_regexp_large_golden.py

tests/golden/<name>_regexp.npz (make_regexp_golden.py) holds automata of at most 16 nodes and 777 transitions; the library
accepts 2048 nodes and 2^22 transitions, and the kernel lays its LDS out by the largest automaton of a batch
(tests/regexp_util.lds_plan).  This writes <name>_regexp_large.npz in the same flat layout (plus `tag`, a name per automaton,
and a pattern field as wide as the longest pattern text) for acgt48k, eng2doc, bytes256 and runs3doc:
  * string drivers: strings cut from the fixture's own documents of 23, 250, 1000 and 2040 symbols (24 .. 2041 nodes), exact,
    APPROX 1 for the first three and APPROX 2:1:2:1 for the shortest,
  * class patterns: strings of 220 and 380 symbols with every fifth symbol a class and every seventh a `.`, exact and APPROX 1,
  * wide drivers: a few nodes and more than 2048 transitions -- a literal prefix, 9 and 12 `.`, and the symbols that follow in
    the text (the search reads a pattern from its END: with nothing after the dots it visits every string of that length in
    the text, 190 k pops and 85 s of the restatement on eng2doc; with the text's next symbols it stays in the hundreds),
  * eng2doc: alternations of words of the text at about 130 and 760 nodes, exact and APPROX 1,
  * hand-made acyclic automata (regexp_util.random_large_nfa, independent of our parser) of 17..64, 65..512 and 513..2048
    nodes -- the ends of every band among them --, a third with error costs.
ref_tool ends a whole call when one automaton fails (ERR_OVERWORKED), so after a failed call every automaton is run in a
call of its own and those that fail are dropped and printed: at most one in ten of the hand-made ones may go, none of the
named ones.  Only data is committed: automata and expected results.
"""
import os
import subprocess
import sys
import tarfile
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import femto_amd  # noqa: E402
import regexp_util as ru  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HAND_PER_BAND = [12, 10, 8]
MAX_BYTES = 350_000


def quoted(s):
    """a string of the text as one quoted pattern term, every symbol escaped"""
    return b'"' + b"".join(b"\\x%02x" % c for c in s) + b'"'


def atom(c):
    return b"\\x%02x" % c


def class_pattern(s, other):
    """s with every fifth symbol a two-character class and every seventh a `.`, the first and last twelve symbols literal (the
    search has narrowed to a few rows before the first open symbol)"""
    out = []
    for k, c in enumerate(s):
        if k < 12 or k >= len(s) - 12 or (k % 5 and k % 7):
            out.append(atom(c))
        elif k % 7 == 0:
            out.append(b".")
        else:
            out.append(b"[" + atom(c) + atom(other[k % len(other)]) + b"]")
    return b"".join(out)


def named(name, docs):
    """(tag, pattern text, APPROX) of the fixture's named drivers"""
    d = max(docs, key=len)
    chars = np.unique(np.concatenate(docs))
    at = 50
    out = []
    for n in (23, 250, 1000, 2040):
        s = d[at:at + n]
        out.append(("str%d" % (n + 1), quoted(s), (0, 1, 1, 1)))
        if n < 2040:
            out.append(("str%d~1" % (n + 1), quoted(s), (1, 1, 1, 1)))
        if n == 23:
            out.append(("str24~2:1:2:1", quoted(s), (2, 1, 2, 1)))
        at += n + 37
    # (cut where the text is least repetitive, its start: inside the 3015-symbol run of runs3doc the APPROX 1 form is 106 k pops)
    for n, cut in ((220, 60), (380, 300)):
        p = class_pattern(d[cut:cut + n], chars)
        out.append(("class%d" % n, p, (0, 1, 1, 1)))
        out.append(("class%d~1" % n, p, (1, 1, 1, 1)))
    for dots, tail in ((9, 3), (12, 4)):
        s = d[at:at + 3 + dots + tail]
        out.append(("wide%d" % dots, quoted(s[:3]) + b"." * dots + quoted(s[3 + dots:]), (0, 1, 1, 1)))
        at += len(s) + 37
    if name == "eng2doc":
        words, seen = [], set()
        for w in d.tobytes().split():
            w = bytes(c for c in w if chr(c).isalpha())
            if len(w) >= 4 and w not in seen:
                seen.add(w)
                words.append(w)
        for total in (130, 760):
            pick, size = [], 0
            for w in words:
                if size + len(w) > total - 2:
                    break
                pick.append(w)
                size += len(w)
            p = b"(" + b"|".join(pick) + b")"
            out.append(("words%d" % total, p, (0, 1, 1, 1)))
            out.append(("words%d~1" % total, p, (1, 1, 1, 1)))
            words = words[len(pick):]
    return out


def run_ref(index, nfas, td):
    """the reference's lists, or None where it failed: one call for all, and after a failure one call each"""
    try:
        return po.ref_regexp_nfa(index, nfas, td, timeout=900)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired):
        pass
    out = []
    for a in nfas:
        try:
            out.append(po.ref_regexp_nfa(index, [a], td, timeout=120)[0])
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired):
            out.append(None)
    return out


def main():
    for name in ru.LARGE_FIXTURES:
        with tempfile.TemporaryDirectory() as td:
            with tarfile.open(os.path.join(OUT, name + ".tar.gz")) as tf:
                tf.extractall(td)
            index = os.path.join(td, "index")
            docs = [np.fromfile(os.path.join(td, f), dtype=np.uint8) for f in sorted(os.listdir(td)) if f.startswith("doc")]
            drivers = named(name, docs)
            tags = [t for t, _, _ in drivers]
            nfas = [femto_amd.Nfa.from_regex(p, k) for _, p, k in drivers]
            regex = [p for _, p, _ in drivers]
            approx = [k for _, _, k in drivers]
            rng = np.random.Generator(np.random.PCG64(sum(name.encode()) + 2048))
            alpha = ru.large_alpha(docs)
            for band, count in enumerate(HAND_PER_BAND):
                for k in range(count):
                    a = ru.random_large_nfa(rng, alpha, ru.band_nodes(rng, band, k, count), approx=k % 3 == 2)
                    tags.append("hand%d.%d_%d%s" % (band, k, a.num_nodes, "~" if a.settings[0] > 1 else ""))
                    nfas.append(a)
            t0 = time.time()
            res = run_ref(index, nfas, td)
            t_ref = time.time() - t0
            dropped = [tags[i] for i, r in enumerate(res) if r is None]
            assert not any(i < len(drivers) for i, r in enumerate(res) if r is None), ("a named driver failed in the reference", dropped)
            assert len(dropped) * 10 <= len(nfas) - len(drivers), ("more than one in ten hand-made automata dropped", dropped)
            keep = [i for i, r in enumerate(res) if r is not None]
            # (the restatement is what the GPU tests compare fresh automata with: where it differs from the reference, say so)
            o = po.Oracle(index)
            t0 = time.time()
            differ = [tags[i] for i in keep if not ru._same(o.nfa_search(nfas[i]), res[i])]
            t_restated = time.time() - t0
            o.close()
            kept = [nfas[i] for i in keep]
            res = [res[i] for i in keep]
            nd = len(drivers)
            gold = dict(
                n=np.int64(len(kept)),
                tag=np.array([tags[i].encode() for i in keep]),
                num_nodes=np.array([a.num_nodes for a in kept], dtype=np.int32),
                settings=np.array([a.settings for a in kept], dtype=np.int32),
                trans_start=np.concatenate([a.trans_start for a in kept]),
                trans_char=np.concatenate([a.trans_char for a in kept]),
                trans_dest=np.concatenate([a.trans_dest for a in kept]),
                is_start=np.concatenate([a.is_start for a in kept]),
                is_final=np.concatenate([a.is_final for a in kept]),
                regex=np.array([regex[i] if i < nd else b"" for i in keep]),
                from_regex=np.array([1 if i < nd else 0 for i in keep], dtype=np.uint8),
                approx=np.array([approx[i] if i < nd else (0, 0, 0, 0) for i in keep], dtype=np.int32),
                err_code=np.array([r[0] for r in res], dtype=np.int32),
                res_count=np.array([len(r[1]) for r in res], dtype=np.int64),
                res_first=np.concatenate([r[1] for r in res]),
                res_last=np.concatenate([r[2] for r in res]),
                res_len=np.concatenate([r[3] for r in res]),
                res_cost=np.concatenate([r[4] for r in res]),
            )
            path = os.path.join(OUT, name + "_regexp_large.npz")
            np.savez_compressed(path, **gold)
            size = os.path.getsize(path)
            assert size <= MAX_BYTES, (path, size)
            print("%s: kept %d of %d automata (%d named, %d hand-made), dropped %s; nodes up to %d, transitions up to %d, %d results, %d errors; "
                  "reference %.1f s, restatement %.1f s, restatement differs on %s; %d bytes"
                  % (name, len(kept), len(nfas), nd, len(kept) - nd, dropped or "none", int(gold["num_nodes"].max()),
                     max(len(a.trans_char) for a in kept), int(gold["res_count"].sum()), int((gold["err_code"] != 0).sum()),
                     t_ref, t_restated, differ or "none", size))


if __name__ == "__main__":
    main()
