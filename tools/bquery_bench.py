#!/usr/bin/env python3
"""tools/bquery_bench.py [--text-log2 K] [--docs D] [--queries N] [--max-occs M] [--steps S] [--baseline-queries B]: boolean queries
(include/femto_amd.h "boolean queries").  Prints one JSON line per measurement.

  batch     N random trees of two to seven leaves (AND OR NOT THEN WITHIN drawn evenly, drawn again until the tree types; the
            leaves are substrings of 4..8 bytes sampled from the text, written as {x ..} hex strings) over an index of 2^K bytes
            of textgen.t_eng text in D documents, answered by ONE femto_amd_bquery_run_batch; host clock around the blocking
            call, best and median of S steps after a warm-up.  Compiling the trees is timed apart.
  baseline  the first B of the same queries done ONE NODE AT A TIME through the host calls that exist without the batch call:
            femto_amd_doclist for a document-typed leaf, femto_amd_locate_flat + femto_amd_resolve_batch for a pair-typed one,
            femto_amd_docset / femto_amd_docpos for every operator (the distinct documents of a pair list under AND / NOT are
            taken on the host).  The two must agree, element for element.

This is also the command rocprofv3 --kernel-trace --stats profiles for profiles/bquery_stats.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AND, OR, NOT, THEN, WITHIN = 1, 2, 3, 4, 5
NAMES = {AND: "AND", OR: "OR", NOT: "NOT", THEN: "THEN", WITHIN: "WITHIN"}
DOCS, PAIRS = 0, 1


def type_of(t, wanted=DOCS):
    if not isinstance(t, tuple):
        return wanted
    op, _, l, r = t
    ask = PAIRS if op in (THEN, WITHIN) else DOCS
    lt, rt = type_of(l, ask), type_of(r, ask)
    if lt is None or rt is None:
        return None
    if op in (AND, NOT):
        return DOCS
    if op == OR:
        return lt if lt == rt else None
    return PAIRS if lt == rt == PAIRS else None


def random_tree(rng, n, npat):
    """a leaf is a pattern number; an operator (op, distance, left, right)"""
    if n == 1:
        return int(rng.integers(0, npat))
    k = int(rng.integers(1, n))
    op = int(rng.integers(AND, WITHIN + 1))
    return (op, int(rng.choice([8, 64, 512])) if op in (THEN, WITHIN) else 0, random_tree(rng, k, npat), random_tree(rng, n - k, npat))


def text_of(t, pats):
    if not isinstance(t, tuple):
        return "{x " + pats[t].tobytes().hex() + "}"
    op, d, l, r = t
    rt = text_of(r, pats)
    return "%s %s%s %s" % (text_of(l, pats), NAMES[op], " %d" % d if op in (THEN, WITHIN) else "", "(" + rt + ")" if isinstance(r, tuple) else rt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=24)
    ap.add_argument("--docs", type=int, default=20_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--vocabulary", type=int, default=2_000)
    ap.add_argument("--max-occs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-queries", type=int, default=300)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--workdir", default=os.environ.get("FEMTO_AMD_BENCH_DIR", "/tmp/femto_amd_bench"))
    args = ap.parse_args()
    import torch
    import femto_amd
    from femto_amd import textgen as tg
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    n = 1 << args.text_log2
    text = tg.t_eng(n, args.seed)
    cuts = np.linspace(0, n, args.docs + 1).astype(np.int64)
    path = os.path.join(args.workdir, f"eng_2p{args.text_log2}_d{args.docs}_s{args.seed}")
    if not os.path.exists(os.path.join(path, "_femto_index")):
        os.makedirs(args.workdir, exist_ok=True)
        t0 = time.perf_counter()
        femto_amd.build_index(path, [text[cuts[i]:cuts[i + 1]] for i in range(args.docs)], params=None, infos=None, device=0)
        print(json.dumps(dict(what="build_index", s=round(time.perf_counter() - t0, 1))), flush=True)
    ix = femto_amd.Index(path, device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    rng = np.random.default_rng(args.seed + 2)
    pats = []
    for _ in range(args.vocabulary):
        ln = int(rng.integers(4, 9))
        at = int(rng.integers(0, n - ln))
        pats.append(np.asarray(text[at:at + ln], dtype=np.uint8))
    trees = []
    while len(trees) < args.queries:
        t = random_tree(rng, int(rng.integers(2, 8)), len(pats))
        if type_of(t) is not None:
            trees.append(t)
    t0 = time.perf_counter()
    qs = [femto_amd.BooleanQuery(text_of(t, pats).encode()) for t in trees]
    compile_ms = (time.perf_counter() - t0) * 1e3
    nodes = sum(len(q.nodes) for q in qs)

    times, got = [], None
    for s in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        got = ix.bquery_run_batch(qs, args.max_occs)
        if s >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="bquery_run_batch", ms_best=round(min(times), 3), ms_median=round(float(np.median(times)), 3), steps=args.steps,
                          queries=len(qs), nodes=nodes, leaves=sum(q.num_leaves for q in qs), max_height=max(_height(t) for t in trees),
                          max_occs=args.max_occs, text_bytes=n, documents=args.docs, result_entries=int(got[0][-1]),
                          nonempty=int((np.diff(got[0]) > 0).sum()), us_per_query=round(min(times) * 1e3 / len(qs), 3),
                          compile_ms=round(compile_ms, 1), note="host clock around the blocking call")), flush=True)

    # ---- the same queries, one node at a time through the host calls
    enc = [p.astype(np.uint16) + 5 for p in pats]

    def node(t, wanted):
        if not isinstance(t, tuple):
            if wanted == DOCS:
                _, docs, _ = ix.documents([enc[t]], args.max_occs)
                return DOCS, docs
            _, offs = ix.locate([enc[t]], args.max_occs)
            d, o = ix.resolve_batch(np.sort(np.asarray(offs, dtype=np.int64)))
            order = np.lexsort((o, d))
            return PAIRS, np.stack([d[order], o[order]], axis=1).astype(np.int64).reshape(-1, 2)
        op, dist, l, r = t
        ask = PAIRS if op in (THEN, WITHIN) else DOCS
        (lt, lv), (rt, rv) = node(l, ask), node(r, ask)
        if op in (AND, NOT) or (op == OR and lt == DOCS):
            a = lv if lt == DOCS else np.unique(lv[:, 0])
            b = rv if rt == DOCS else np.unique(rv[:, 0])
            return DOCS, ix.docset([a], [b], [{AND: femto_amd.DOCSET_AND, OR: femto_amd.DOCSET_OR, NOT: femto_amd.DOCSET_NOT}[op]])[1]
        _, rd, ro = ix.docpos([lv], [rv], [{THEN: femto_amd.DOCPOS_THEN, WITHIN: femto_amd.DOCPOS_WITHIN, OR: femto_amd.DOCPOS_OR}[op]], [dist])
        return PAIRS, np.stack([rd, ro], axis=1).reshape(-1, 2)

    nb = min(args.baseline_queries, len(trees))
    if nb:
        t0 = time.perf_counter()
        base = [node(t, DOCS) for t in trees[:nb]]
        base_ms = (time.perf_counter() - t0) * 1e3
        for k, (t, v) in enumerate(base):
            s, e = int(got[0][k]), int(got[0][k + 1])
            assert t == got[1][k], "result types differ"
            want_doc = v[:, 0] if t == PAIRS else v
            want_off = v[:, 1] if t == PAIRS else np.zeros(len(v), dtype=np.int64)
            assert np.array_equal(got[2][s:e], want_doc) and np.array_equal(got[3][s:e], want_off), ("query", k, "differs")
        print(json.dumps(dict(what="one_node_at_a_time", ms=round(base_ms, 1), queries=nb, us_per_query=round(base_ms * 1e3 / nb, 1),
                              ratio_per_query=round(base_ms / nb / (min(times) / len(qs)), 1),
                              note="host calls of the parent commit, one per leaf and per operator; one pass, host clock")), flush=True)
    ix.close()


def _height(t):
    return 0 if not isinstance(t, tuple) else 1 + max(_height(t[2]), _height(t[3]))


if __name__ == "__main__":
    main()
