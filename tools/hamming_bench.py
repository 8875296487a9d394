#!/usr/bin/env python3
"""tools/hamming_bench.py [--text-log2 K] [--patterns N] [--out FILE]: occurrences within k substitutions by exact seeds
(include/femto_amd.h "occurrences within k substitutions, by exact seeds") on the two texts of tools/mismatch_bench.py -- 2^K bytes
in 64 documents, the indexes that tool builds are reused -- and N patterns per case:

  dna100  uniform ACGT; 100-mers cut from the text with 0..k substitutions planted; k = 1, 2, 4, 8.
  dna20   uniform ACGT; 20-mers cut from the text with 0..k substitutions planted; k = 1 and k = 2.  At k = 2 the pieces hold 6, 7
          and 7 symbols -- some 25 000 candidates per pattern on 64 MiB -- so that case runs --short-patterns patterns (20 000).
  eng     English-like text; patterns of 32..64 bytes cut from the text with 0..k substitutions planted; k = 1, 2, 4.

A case whose candidates reach 2^30 (8 GiB of located offsets) is halved until they do not; every line says how many patterns it
ran, and gives candidates and results per pattern.

  hamming     femto_amd_hamming_device with the capacities a counting call reported.  HIP events around back-to-back calls after
              one warm-up call, repeated until the window is at least --min-s seconds; the mean per call.
  enumerated  (k <= 2) the route the tree had: femto_amd_mismatch_device on the same patterns, the rows of its ranges laid out by a
              prefix sum and located by femto_amd_locate_walk_device.  Timed the same way, in the same process, in windows that
              ALTERNATE with those of the new call.  Before any time is reported the (pattern, offset) pairs of both routes are
              compared at the timed size.

Every GPU step is a child process of its own under its own time limit, and the first failure ends the run; one JSON line per
measurement, all written to --out (default profiles/hamming_stats.txt)."""
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

import mismatch_bench as mb      # noqa: E402  (the texts, the index paths, the clock)

CASES = [("dna100", 1), ("dna100", 2), ("dna100", 4), ("dna100", 8), ("dna20", 1), ("dna20", 2), ("eng", 1), ("eng", 2), ("eng", 4)]
STEPS = [("build_dna", 600), ("build_eng", 600)] + [("%s_%d" % c, 600) for c in CASES]
CAND_LIMIT = 1 << 30


def patterns_of(args, case, k, n):
    """(plen int32[n], flat uint16[], what the patterns are): cuts of the text, pattern i with i mod (k + 1) substitutions planted"""
    from femto_amd import textgen as tg
    which = "eng" if case == "eng" else "dna"
    text = mb.text_of(args, which)
    lo, hi = {"dna100": (100, 100), "dna20": (20, 20), "eng": (32, 64)}[case]
    plen, flat = tg.p_hit(lo, hi, n, args.seed + 7, text)
    starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)])
    rng = np.random.Generator(np.random.PCG64(args.seed + 8 + k))
    have = np.unique(text).astype(np.uint16) + 5
    nsub = np.arange(n) % (k + 1)
    for j in range(k):          # the j-th planted substitution of every pattern that has one: positions may repeat, so at most nsub differ
        who = np.nonzero(nsub > j)[0]
        at = starts[who] + rng.integers(0, plen[who])
        flat[at] = have[(np.searchsorted(have, flat[at]) + rng.integers(1, len(have), len(who))) % len(have)]
    return plen, flat, "%s cut from the text, pattern i with up to i mod (k + 1) substitutions planted" % ("%d-mers" % lo if lo == hi else "%d..%d bytes" % (lo, hi))


def step_query(args, report, case, k):
    import torch
    import femto_amd
    dev = "cuda:0"
    which = "eng" if case == "eng" else "dna"
    ix = femto_amd.Index(mb.index_path(args, which), device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    N = int(ix.info.total_length)
    st = torch.cuda.current_stream().cuda_stream
    i64 = lambda c: torch.zeros(max(c, 1), dtype=torch.int64, device=dev)      # noqa: E731
    i32 = lambda c: torch.zeros(max(c, 1), dtype=torch.int32, device=dev)      # noqa: E731
    i16 = lambda c: torch.zeros(max(c, 1), dtype=torch.int16, device=dev)      # noqa: E731
    n = args.short_patterns if (case, k) == ("dna20", 2) else args.patterns
    while True:
        plen, flat, what = patterns_of(args, case, k, n)
        nsyms = int(plen.sum())
        starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)]).astype(np.int64)
        buf = i16(nsyms + 16)          # (8 symbols of slack on either side)
        buf[8:8 + nsyms] = torch.from_numpy(flat.view(np.int16)).to(dev)
        d_syms = buf.data_ptr() + 16
        d_starts = torch.from_numpy(starts).to(dev)
        d_rs, d_tot = i64(n + 1), i64(4)
        ix.hamming_device(n, nsyms, d_syms, d_starts, k, 0, 0, d_rs, None, None, d_tot, stream=st)      # the candidates ...
        torch.cuda.synchronize()
        cands = int(d_tot.cpu()[2])
        if cands < CAND_LIMIT:
            break
        n //= 2
    ix.hamming_device(n, nsyms, d_syms, d_starts, k, cands, 0, d_rs, None, None, d_tot, stream=st)      # ... and the results
    torch.cuda.synchronize()
    assert d_tot.cpu().tolist()[1:] == [1, cands, 0] or d_tot.cpu().tolist() == [0, 0, cands, 0]
    total = int(d_tot.cpu()[0])
    d_off, d_cost = i64(total), i32(total)
    call = lambda: ix.hamming_device(n, nsyms, d_syms, d_starts, k, cands, total, d_rs, d_off, d_cost, d_tot, stream=st)      # noqa: E731
    call()
    torch.cuda.synchronize()
    assert d_tot.cpu().tolist() == [total, 0, cands, 0]
    rs = d_rs.clone()
    mine = torch.repeat_interleave(torch.arange(n, device=dev), rs[1:] - rs[:-1]) * N + d_off[:total]
    assert bool((mine[1:] > mine[:-1]).all()), "the results are not in (pattern, offset) order"
    cost = d_cost[:total].cpu().numpy()
    clock = "HIP events, mean of back-to-back calls after a warm-up call"

    other = None
    if k <= 2:      # the route the tree had: the variants' ranges, then their rows located
        m_rs, m_tot = i64(n + 1), i64(2)
        ix.mismatch_device(n, nsyms, d_syms, d_starts, k, 0, m_rs, None, None, None, None, None, m_tot, stream=st)
        torch.cuda.synchronize()
        nvar = int(m_tot.cpu()[0])
        m_first, m_last, m_cost, m_pos, m_sym = i64(nvar), i64(nvar), i32(nvar), i32(2 * nvar), i16(2 * nvar)
        m_os, m_offs = i64(nvar + 1), i64(total)

        def other():
            ix.mismatch_device(n, nsyms, d_syms, d_starts, k, nvar, m_rs, m_first, m_last, m_cost, m_pos, m_sym, m_tot, stream=st)
            torch.cumsum(m_last[:nvar] - m_first[:nvar] + 1, 0, out=m_os[1:nvar + 1])
            ix.locate_walk_device(nvar, m_first.data_ptr(), m_os.data_ptr(), total, m_offs.data_ptr(), stream=st)
        other()
        torch.cuda.synchronize()
        assert int(m_os[nvar].item()) == total, ("the routes disagree on the number of occurrences", int(m_os[nvar].item()), total)
        rows = m_last[:nvar] - m_first[:nvar] + 1
        pat_of_var = torch.repeat_interleave(torch.arange(n, device=dev), m_rs[1:] - m_rs[:-1])
        theirs = torch.repeat_interleave(pat_of_var, rows) * N + m_offs[:total]
        assert torch.equal(torch.sort(theirs).values, mine), "the routes disagree on the (pattern, offset) pairs"
        their_cost = torch.repeat_interleave(m_cost[:nvar], rows)[torch.argsort(theirs)]
        assert torch.equal(their_cost, d_cost[:total]), "the routes disagree on the costs"

    ms_a = ms_b = 0.0
    reps_a = reps_b = 0
    windows = 2 if other else 1
    for _ in range(windows):      # the two routes in alternating windows
        ms, reps = mb.timed(call, args.min_s / windows)
        ms_a, reps_a = ms_a + ms * reps, reps_a + reps
        if other:
            ms, reps = mb.timed(other, args.min_s / windows)
            ms_b, reps_b = ms_b + ms * reps, reps_b + reps
    ms_a /= reps_a
    row = dict(what="hamming", case=case, text=which, k=k, ms=round(ms_a, 4), calls=reps_a, patterns=n, symbols=nsyms, candidates=cands, results=total,
               candidates_per_pattern=round(cands / n, 2), results_per_pattern=round(total / n, 3), us_per_pattern=round(ms_a * 1e3 / n, 5),
               mpatterns_per_s=round(n / ms_a / 1e3, 3), results_by_cost=np.bincount(cost, minlength=k + 1).tolist(), policy=mb.policy_of(ix),
               pattern_set=what, clock=clock)
    if other:
        ms_b /= reps_b
        row.update(enumerated_ms=round(ms_b, 4), enumerated_calls=reps_b, enumerated_variants=nvar, enumerated_over_hamming=round(ms_b / ms_a, 3),
                   enumerated="femto_amd_mismatch_device + prefix sum + femto_amd_locate_walk_device, same patterns, alternating windows; pairs and costs compared first")
    report(**row)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--short-patterns", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--cases", default=None, help="comma-separated subset of the steps, e.g. dna100_1,eng_2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_stats.txt"))
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
            mb.step_build(args, report, args.step[6:])
        else:
            case, k = args.step.rsplit("_", 1)
            step_query(args, report, case, int(k))
        return 0
    os.makedirs(args.workdir, exist_ok=True)
    rows_path = os.path.join(args.workdir, "hamming_rows.jsonl")
    open(rows_path, "w").close()
    wanted = set(args.cases.split(",")) if args.cases else None
    for step, limit in STEPS:      # a step that fails or runs out of time ends the run: nothing more is started on the GPU
        if wanted and not step.startswith("build_") and step not in wanted:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", rows_path, "--text-log2", str(args.text_log2),
               "--patterns", str(args.patterns), "--short-patterns", str(args.short_patterns), "--seed", str(args.seed), "--min-s", str(args.min_s),
               "--workdir", args.workdir]
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc:
            print(f"step {step}: exit status {rc}", file=sys.stderr)
            return rc
    with open(rows_path) as f:
        rows = f.read()
    with open(args.out, "w") as f:
        f.write("profiles/hamming_stats.txt -- `python tools/hamming_bench.py` on one MI355X, %s: occurrences within k substitutions by exact\n"
                "seeds against %d MiB texts in %d documents (every structure resident), and for k <= 2 the route the tree had --\n"
                "femto_amd_mismatch_device, then the rows of its ranges located -- on the same patterns in alternating windows.\n"
                "tools/hamming_bench.py says how each figure is timed; DESIGN.md \"Occurrences within k substitutions\" has the kernels' registers.\n"
                "The same patterns are searched call after call: what they touch of the index stays in the caches, for both routes.\n\n"
                % (time.strftime("%Y-%m-%d"), (1 << args.text_log2) >> 20, mb.NDOCS))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
