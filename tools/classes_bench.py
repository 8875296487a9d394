#!/usr/bin/env python3
"""tools/classes_bench.py [--text-log2 K] [--patterns N] [--out FILE]: search with character classes (include/femto_amd.h "search
with character classes") on the two texts of tools/mismatch_bench.py -- 2^K bytes in 64 documents -- and N patterns each:

  dnaN1, dnaN2, dnaN4   uniform ACGT (femto_amd/textgen.py t_acgt); 20-mers, half of them sampled from the text, half uniform
                        random, with 1, 2 and 4 random positions turned into N (the class ACGT).
  icase                 English-like text (t_eng); patterns of 8..64 bytes sampled from the text, every letter the class of its two
                        cases (icase_ast).
  periods               1 000 patterns of four periods over the English-like text: every lane lists every distinct 4-gram, serially
                        (the known limit of one lane per pattern).

and up to three ways, in one process per case:

  classes     femto_amd_classes_device with the capacity a counting call reported.  HIP events around back-to-back calls after one
              warm-up call, repeated until the window is at least --min-s seconds; the mean per call.
  automaton   the same patterns as texts of the query language through femto_amd_nfa_search_batch, on the first
              --automaton-patterns patterns (50 000; 8 for `periods`, whose lists are long).  Wall clock (time.perf_counter)
              around the one blocking call, after batches of 64 and 256 (of 2 and 4 for `periods`), automata compiled and marshalled
              beforehand; reported per pattern.  Searches that end with a status are counted, not hidden.
  expanded    (dnaN1 only) the four strings of every pattern written out -- on the device, not timed -- and counted by
              femto_amd_count_device; HIP events as for classes.  The tool checks that the non-empty ranges are as many as the
              results of classes.

Every GPU step is a child process of its own under its own time limit, and the first failure ends the run; one JSON line per
measurement, all written to --out (default profiles/classes_stats.txt) under the commit they were taken at."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mismatch_bench import NDOCS, index_path, policy_of, step_build, text_of, timed  # noqa: E402

STEPS = [("build_dna", 600), ("build_eng", 600), ("dnaN1", 600), ("dnaN2", 600), ("dnaN4", 600), ("icase", 900), ("periods", 900)]
CLASS = 0x8000


def class_words(members):
    w = np.zeros(4, dtype=np.uint64)
    for b in members:
        w[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return w


def patterns_of(args, case):
    """(which text, plen int32[n], flat uint16[], classes uint64[c, 4], what the patterns are)"""
    from femto_amd import textgen as tg
    rng = np.random.Generator(np.random.PCG64(args.seed + 7))
    if case.startswith("dnaN"):
        text = text_of(args, "dna")
        n, k = args.patterns, int(case[4:])
        half = n // 2
        plen, flat = tg.p_hit(20, 20, half, args.seed + 2, text)
        rlen, rflat = tg.p_rand(20, n - half, args.seed + 4)
        flat = np.concatenate([flat, rflat]).reshape(n, 20)[rng.permutation(n)]
        at = np.argsort(rng.random((n, 20)), axis=1)[:, :k]          # k different positions per pattern
        flat[np.arange(n)[:, None], at] = CLASS
        return "dna", np.concatenate([plen, rlen]), np.ascontiguousarray(flat.reshape(-1)), class_words(b"ACGT")[None, :], \
            "20-mers, half sampled from the text, half uniform random, %d position(s) each turned into N" % k
    text = text_of(args, "eng")
    if case == "icase":
        plen, flat = tg.p_hit(8, 64, args.patterns, args.seed + 2, text)
        b = flat.astype(np.int32) - 5
        letter = ((b >= 65) & (b <= 90)) | ((b >= 97) & (b <= 122))
        flat = np.where(letter, CLASS | ((b | 32) - 97), flat).astype(np.uint16)
        table = np.stack([class_words([65 + i, 97 + i]) for i in range(26)])
        return "eng", plen, np.ascontiguousarray(flat), table, "lengths 8..64 sampled from the text, every letter the class of its two cases"
    n = min(args.patterns, 1000)
    return "eng", np.full(n, 4, dtype=np.int32), np.full(4 * n, CLASS, dtype=np.uint16), class_words(range(256))[None, :], "four periods"


def regex_of(p, table):
    out = b""
    for s in p:
        s = int(s)
        if s & CLASS:
            mem = [b for b in range(256) if (int(table[s & ~CLASS][b >> 6]) >> (b & 63)) & 1]
            out += b"." if len(mem) == 256 else b"[" + b"".join(b"\\x%02x" % b for b in mem) + b"]"
        else:
            out += b"\\x%02x" % (s - 5)
    return out


def step_query(args, report, case):
    import torch
    import femto_amd
    dev = "cuda:0"
    which, plen, flat, table, what = patterns_of(args, case)
    n, nsyms, ncls = len(plen), int(plen.sum()), len(table)
    starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)]).astype(np.int64)
    ix = femto_amd.Index(index_path(args, which), device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    kind = policy_of(ix)
    st = torch.cuda.current_stream().cuda_stream
    i64 = lambda c: torch.zeros(max(c, 1), dtype=torch.int64, device=dev)      # noqa: E731
    d_syms = torch.from_numpy(flat.view(np.int16)).to(dev)
    d_starts = torch.from_numpy(starts).to(dev)
    d_cls = torch.from_numpy(np.ascontiguousarray(table).view(np.int64)).to(dev)
    d_rs, d_tot = i64(n + 1), i64(2)
    ix.classes_device(n, nsyms, d_syms, d_starts, ncls, d_cls, 0, d_rs, None, None, d_tot, stream=st)
    torch.cuda.synchronize()
    total = int(d_tot.cpu()[0])
    d_first, d_last = i64(total), i64(total)
    call = lambda: ix.classes_device(n, nsyms, d_syms, d_starts, ncls, d_cls, total, d_rs, d_first, d_last, d_tot, stream=st)      # noqa: E731
    clock = "HIP events, mean of back-to-back calls after a warm-up call"
    ms, reps = timed(call, args.min_s)
    assert d_tot.cpu().tolist() == [total, 0]
    us_a = ms * 1e3 / n
    per = np.diff(d_rs.cpu().numpy())
    report(what="classes", case=case, text=which, ms=round(ms, 4), calls=reps, patterns=n, symbols=nsyms, class_positions=int(((flat & CLASS) != 0).sum()),
           classes=ncls, us_per_pattern=round(us_a, 5), mpatterns_per_s=round(n / ms / 1e3, 4), results=total, most_results_of_a_pattern=int(per.max()),
           patterns_with_a_result=int((per > 0).sum()), policy=kind, pattern_set=what, clock=clock)

    # ---- the automaton route on the first M patterns
    def automaton(m):
        batch = femto_amd.NfaBatch([femto_amd.Nfa.from_regex(regex_of(flat[starts[q]:starts[q + 1]], table)) for q in range(m)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ix.nfa_search_batch(batch, max_results=1 << 24)
        return time.perf_counter() - t0, out
    few = case == "periods"
    automaton(2 if few else 64)
    automaton(4 if few else 256)
    m = min(n, 8 if few else args.automaton_patterns)      # (eight lists of a million 4-grams: the call's result buffer is 2^24)
    s_m, out = automaton(m)
    status = out[5]
    found = int(out[0][-1])
    mine = int(d_rs.cpu().numpy()[m])
    us_b = s_m * 1e6 / m
    report(what="automaton", case=case, text=which, patterns=m, seconds=round(s_m, 3), us_per_pattern=round(us_b, 3), kpatterns_per_s=round(m / s_m / 1e3, 3),
           results=found, searches_with_a_status=int((status != 0).sum()), classes_results_same_patterns=mine, classes_speedup_per_pattern=round(us_b / us_a, 2),
           clock="time.perf_counter around one blocking femto_amd_nfa_search_batch, automata compiled beforehand; after two smaller batches")
    assert found <= mine or status.any(), "the automaton route found results the call does not list"

    # ---- dnaN1: the four strings of every pattern, counted
    if case == "dnaN1":
        base = d_syms.view(n, 20)
        at = (base < 0).to(torch.int32).argmax(dim=1)          # (CLASS | 0 is negative as int16)
        lut = torch.tensor([ord(c) + 5 for c in "ACGT"], dtype=torch.int16, device=dev)
        v = base.unsqueeze(1).repeat(1, 4, 1)
        v[torch.arange(n, device=dev).repeat_interleave(4), torch.arange(4, device=dev).repeat(n), at.repeat_interleave(4)] = lut.repeat(n)
        nv = n * 4
        buf = torch.zeros(nv * 20 + 16, dtype=torch.int16, device=dev)
        buf[8:8 + nv * 20] = v.reshape(-1)
        del v
        v_plen = torch.full((nv,), 20, dtype=torch.int32, device=dev)
        v_starts = torch.arange(nv, dtype=torch.int64, device=dev) * 20
        v_first, v_last = i64(nv), i64(nv)
        count = lambda: ix.count_device(nv, v_plen.data_ptr(), buf.data_ptr() + 16, v_starts.data_ptr(), v_first.data_ptr(), v_last.data_ptr(), stream=st)      # noqa: E731
        ms_c, reps_c = timed(count, args.min_s)
        hits = int((v_first <= v_last).sum().item())
        assert hits == total, ("expansion and the call disagree", hits, total)
        report(what="expanded", case=case, text=which, ms=round(ms_c, 4), calls=reps_c, patterns=n, strings=nv, us_per_pattern=round(ms_c * 1e3 / n, 5),
               non_empty=hits, level_table=bool(ix.pack_info()["level_table"]), level_table_syms=int(ix.pack_info()["ktab_syms"]),
               classes_over_expanded=round(ms / ms_c, 3), clock=clock + "; the expansion itself is not timed")
    ix.close()


def commit():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return (head or "unknown") + (" plus uncommitted changes" if dirty else "")
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--automaton-patterns", type=int, default=50000)
    ap.add_argument("--commit", default=None, help="the commit the figures are taken at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_stats.txt"))
    ap.add_argument("--workdir", default=os.environ.get("FEMTO_AMD_BENCH_DIR", "/tmp/femto_amd_bench"))
    ap.add_argument("--step", default=None, help="(internal) run one GPU step and append its JSON lines to --rows")
    ap.add_argument("--rows", default=None)
    args = ap.parse_args()
    if args.step:
        def report(**kw):
            line = json.dumps(kw)
            print(line, flush=True)
            with open(args.rows, "a") as f:
                f.write(line + "\n")
        if args.step.startswith("build_"):
            step_build(args, report, args.step[6:])
        else:
            step_query(args, report, args.step)
        return 0
    os.makedirs(args.workdir, exist_ok=True)
    rows_path = os.path.join(args.workdir, "classes_rows.jsonl")
    open(rows_path, "w").close()
    for step, limit in STEPS:      # a step that fails or runs out of time ends the run: nothing more is started on the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", rows_path, "--text-log2", str(args.text_log2),
               "--patterns", str(args.patterns), "--seed", str(args.seed), "--min-s", str(args.min_s), "--automaton-patterns", str(args.automaton_patterns),
               "--workdir", args.workdir]
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc:
            print(f"step {step}: exit status {rc}", file=sys.stderr)
            return rc
    with open(rows_path) as f:
        rows = f.read()
    with open(args.out, "w") as f:
        f.write("profiles/classes_stats.txt -- `python tools/classes_bench.py` on one MI355X, %s, at commit %s: search with a character class\n"
                "per position for %d patterns (1 000 for `periods`) against %d MiB texts in %d documents (every structure resident), the same\n"
                "question through the automaton search and, for DNA reads with one N, the four strings of every pattern counted one by one.\n"
                "tools/classes_bench.py says how each figure is timed; DESIGN.md \"Search with character classes\" has the kernels' registers.\n"
                "The same patterns are searched call after call: what they touch of the index stays in the caches, for all three ways.\n\n"
                % (time.strftime("%Y-%m-%d"), args.commit or commit(), args.patterns, (1 << args.text_log2) >> 20, NDOCS))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
