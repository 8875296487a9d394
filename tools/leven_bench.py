#!/usr/bin/env python3
"""tools/leven_bench.py [--text-log2 K] [--patterns N] [--out FILE]: occurrences within k edits by exact seeds
(include/femto_amd.h "occurrences within k edits, by exact seeds") on the two texts of tools/mismatch_bench.py -- 2^K bytes in 64
documents, the indexes that tool builds are reused -- and N patterns per case, cut from the text with 0 .. k edits planted: pattern
i has i mod (k + 1) of them, the first an insertion or a deletion, the others substitutions.

  dna100  uniform ACGT; 100-mers; k = 1, 2, 4, 8.
  eng     English-like text; patterns of 32..64 bytes; k = 1, 2.
  dna20   uniform ACGT; 20-mers; k = 1 and k = 2: the case where the seeds explode; it runs --short-patterns patterns (20 000).

A case whose candidates reach 2^30 or whose raw records reach 2^29 is halved until they do not; every line says how many patterns
it ran, and gives candidates, raw records and results per pattern.

  leven      femto_amd_leven_device with the capacities a counting call reported.  HIP events around back-to-back calls after one
             warm-up call, repeated until the window is at least --min-s seconds; the mean per call.
  hamming    (a) femto_amd_hamming_device on the same patterns: the same seeds and a cheaper check, so it is the floor.  Before a
             time is reported every one of its (pattern, offset) results is looked up among the new call's.
  edit       (b) k <= 2: today's route to the same offsets -- femto_amd_edit_device, then the rows of its ranges located
             (prefix sum + femto_amd_locate_walk_device) -- on the first --edit-patterns patterns of the batch; every located
             (pattern, offset) is looked up among the new call's results.  Reported per pattern.
  automaton  (c) k <= 2, the ACGT cases: the automaton search with APPROX k:1:1:1 on --automaton-patterns patterns, wall clock.

The three run in the same process in windows that ALTERNATE.  Every GPU step is a child process of its own under its own time
limit, and the first failure ends the run; one JSON line per measurement, all written to --out (default profiles/leven_stats.txt)."""
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

CASES = [("dna100", 1), ("dna100", 2), ("dna100", 4), ("dna100", 8), ("eng", 1), ("eng", 2), ("dna20", 1), ("dna20", 2)]
STEPS = [("build_dna", 600), ("build_eng", 600)] + [("%s_%d" % c, 600) for c in CASES]
CAND_LIMIT, RAW_LIMIT = 1 << 30, 1 << 29


def patterns_of(args, case, k, n):
    """(plen int32[n], flat uint16[], what the patterns are)"""
    from femto_amd import textgen as tg
    which = "eng" if case == "eng" else "dna"
    text = mb.text_of(args, which)
    lo, hi = {"dna100": (100, 100), "dna20": (20, 20), "eng": (32, 64)}[case]
    plen, flat = tg.p_hit(lo, hi, n, args.seed + 7, text)
    starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)])
    rng = np.random.Generator(np.random.PCG64(args.seed + 8 + k))
    have = np.unique(text).astype(np.uint16) + 5
    nedits = np.arange(n) % (k + 1)
    other = lambda codes, count: have[(np.searchsorted(have, codes) + rng.integers(1, len(have), count)) % len(have)]      # noqa: E731
    for j in range(1, k):          # the substitutions behind the indel: positions may repeat, so at most nedits - 1 differ
        who = np.nonzero(nedits > j)[0]
        at = starts[who] + rng.integers(0, plen[who])
        flat[at] = other(flat[at], len(who))
    edited = np.nonzero(nedits > 0)[0]
    ins, dele = edited[::2], edited[1::2]
    ins_at = starts[ins] + rng.integers(0, plen[ins])
    del_at = starts[dele] + rng.integers(0, plen[dele])
    flat = np.insert(flat, ins_at, other(flat[ins_at], len(ins)))          # (another character than the one it stands in front of)
    del_at = del_at + np.searchsorted(np.sort(ins_at), del_at, side="right")
    flat = np.delete(flat, del_at)
    plen = plen.copy()
    plen[ins] += 1
    plen[dele] -= 1
    assert int(plen.sum()) == len(flat) and plen.min() > k
    return plen, np.ascontiguousarray(flat), ("%s cut from the text, pattern i with i mod (k + 1) edits planted: one insertion or deletion, the others substitutions"
                                              % ("%d-mers" % lo if lo == hi else "%d..%d bytes" % (lo, hi)))


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
    n = args.short_patterns if case == "dna20" else args.patterns
    while True:
        plen, flat, what = patterns_of(args, case, k, n)
        nsyms = int(plen.sum())
        starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)]).astype(np.int64)
        buf = i16(nsyms + 16)          # (8 symbols of slack on either side)
        buf[8:8 + nsyms] = torch.from_numpy(flat.view(np.int16)).to(dev)
        d_syms = buf.data_ptr() + 16
        d_starts = torch.from_numpy(starts).to(dev)
        d_rs, d_tot = i64(n + 1), i64(5)
        ix.leven_device(n, nsyms, d_syms, d_starts, k, 0, 0, d_rs, None, None, None, d_tot, stream=st)      # the candidates ...
        torch.cuda.synchronize()
        cands = int(d_tot.cpu()[3])
        raw = 0
        if cands < CAND_LIMIT:
            ix.leven_device(n, nsyms, d_syms, d_starts, k, cands, 0, d_rs, None, None, None, d_tot, stream=st)      # ... and the raw records
            torch.cuda.synchronize()
            assert d_tot.cpu().tolist()[3:] == [cands, 0]
            raw = int(d_tot.cpu()[2])
            if raw < RAW_LIMIT:
                break
        n //= 2
    d_off, d_cost, d_len = i64(raw), i32(raw), i32(raw)
    call = lambda: ix.leven_device(n, nsyms, d_syms, d_starts, k, cands, raw, d_rs, d_off, d_cost, d_len, d_tot, stream=st)      # noqa: E731
    call()
    torch.cuda.synchronize()
    total = int(d_tot.cpu()[0])
    assert d_tot.cpu().tolist() == [total, 0, raw, cands, 0]
    rs = d_rs.clone()
    mine = torch.repeat_interleave(torch.arange(n, device=dev), rs[1:] - rs[:-1]) * N + d_off[:total]
    assert bool((mine[1:] > mine[:-1]).all()), "the results are not in (pattern, offset) order, each offset once"
    my_cost = d_cost[:total]
    cost = my_cost.cpu().numpy()
    clock = "HIP events, mean of back-to-back calls after a warm-up call"

    def held(theirs, their_cost, who):
        """every (pattern * N + offset) of `theirs` is a result here, at no higher cost"""
        at = torch.searchsorted(mine, theirs).clamp(max=total - 1)
        assert bool((mine[at] == theirs).all()), who + ": an offset that the new call lacks"
        assert bool((my_cost[at] <= their_cost).all()), who + ": an offset that the new call has at a higher cost"

    # (a) the floor: the same seeds, a window compare
    h_rs, h_tot = i64(n + 1), i64(4)
    ix.hamming_device(n, nsyms, d_syms, d_starts, k, cands, 0, h_rs, None, None, h_tot, stream=st)
    torch.cuda.synchronize()
    assert h_tot.cpu().tolist()[2:] == [cands, 0], "hamming and leven disagree on the candidates"
    h_total = int(h_tot.cpu()[0])
    h_off, h_cost = i64(h_total), i32(h_total)
    floor = lambda: ix.hamming_device(n, nsyms, d_syms, d_starts, k, cands, h_total, h_rs, h_off, h_cost, h_tot, stream=st)      # noqa: E731
    floor()
    torch.cuda.synchronize()
    held(torch.repeat_interleave(torch.arange(n, device=dev), h_rs[1:] - h_rs[:-1]) * N + h_off[:h_total], h_cost[:h_total], "hamming")

    # (b) today's route for k <= 2, on the batch's first patterns
    other, ne = None, min(n, args.edit_patterns)
    if k <= 2:
        e_syms = int(starts[ne])
        e_rs, e_tot = i64(ne + 1), i64(3)
        ix.edit_device(ne, e_syms, d_syms, d_starts, k, 0, e_rs, None, None, None, None, e_tot, stream=st)
        torch.cuda.synchronize()
        e_raw = int(e_tot.cpu()[2])
        e_first, e_last, e_cost, e_len = i64(e_raw), i64(e_raw), i32(e_raw), i32(e_raw)
        ix.edit_device(ne, e_syms, d_syms, d_starts, k, e_raw, e_rs, e_first, e_last, e_cost, e_len, e_tot, stream=st)
        torch.cuda.synchronize()
        nstr = int(e_tot.cpu()[0])
        rows = int((e_last[:nstr] - e_first[:nstr] + 1).sum().item())
        e_os, e_offs = i64(nstr + 1), i64(rows)

        def other():
            ix.edit_device(ne, e_syms, d_syms, d_starts, k, e_raw, e_rs, e_first, e_last, e_cost, e_len, e_tot, stream=st)
            torch.cumsum(e_last[:nstr] - e_first[:nstr] + 1, 0, out=e_os[1:nstr + 1])
            ix.locate_walk_device(nstr, e_first.data_ptr(), e_os.data_ptr(), rows, e_offs.data_ptr(), stream=st)
        other()
        torch.cuda.synchronize()
        per = e_last[:nstr] - e_first[:nstr] + 1
        pat_of = torch.repeat_interleave(torch.arange(ne, device=dev), e_rs[1:] - e_rs[:-1])
        held(torch.repeat_interleave(pat_of, per) * N + e_offs[:rows], torch.repeat_interleave(e_cost[:nstr], per), "edit + locate")

    ms_a = ms_f = ms_b = 0.0
    reps_a = reps_f = reps_b = 0
    for _ in range(2):      # the routes in alternating windows
        ms, reps = mb.timed(call, args.min_s / 2)
        ms_a, reps_a = ms_a + ms * reps, reps_a + reps
        ms, reps = mb.timed(floor, args.min_s / 2)
        ms_f, reps_f = ms_f + ms * reps, reps_f + reps
        if other:
            ms, reps = mb.timed(other, args.min_s / 2)
            ms_b, reps_b = ms_b + ms * reps, reps_b + reps
    ms_a, ms_f = ms_a / reps_a, ms_f / reps_f
    row = dict(what="leven", case=case, text=which, k=k, ms=round(ms_a, 4), calls=reps_a, patterns=n, symbols=nsyms, candidates=cands, raw_records=raw,
               results=total, candidates_per_pattern=round(cands / n, 2), results_per_pattern=round(total / n, 3),
               raw_per_result=round(raw / max(total, 1), 3), us_per_pattern=round(ms_a * 1e3 / n, 5), mpatterns_per_s=round(n / ms_a / 1e3, 3),
               results_by_cost=np.bincount(cost, minlength=k + 1).tolist(), hamming_ms=round(ms_f, 4), hamming_calls=reps_f, hamming_results=h_total,
               leven_over_hamming=round(ms_a / ms_f, 3), policy=mb.policy_of(ix), pattern_set=what, clock=clock)
    if other:
        ms_b /= reps_b
        row.update(edit_locate_ms=round(ms_b, 4), edit_locate_calls=reps_b, edit_locate_patterns=ne, edit_strings=nstr, edit_rows=rows,
                   edit_locate_us_per_pattern=round(ms_b * 1e3 / ne, 5), edit_locate_over_leven_per_pattern=round((ms_b / ne) / (ms_a / n), 3),
                   edit_locate="femto_amd_edit_device + prefix sum + femto_amd_locate_walk_device on the batch's first patterns, alternating windows; its offsets looked up first")
    if k <= 2 and which == "dna" and args.automaton_patterns:      # (c) the automaton search, wall clock
        na = min(n, args.automaton_patterns)
        nfas = [femto_amd.Nfa.from_regex((flat[starts[i]:starts[i + 1]] - 5).astype(np.uint8).tobytes(), (k, 1, 1, 1)) for i in range(na)]
        ix.nfa_search_batch(nfas[:64])
        t0 = time.perf_counter()
        res = ix.nfa_search_batch(nfas)
        dt = time.perf_counter() - t0
        row.update(automaton_ms=round(dt * 1e3, 2), automaton_patterns=na, automaton_results=int(res[0][-1]), automaton_us_per_pattern=round(dt * 1e6 / na, 4),
                   automaton="APPROX k:1:1:1 through nfa_search_batch on the batch's first patterns, wall clock of one call after a 64-pattern warm-up")
    report(**row)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--short-patterns", type=int, default=20000)
    ap.add_argument("--edit-patterns", type=int, default=20000)
    ap.add_argument("--automaton-patterns", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--cases", default=None, help="comma-separated subset of the steps, e.g. dna100_1,eng_2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leven_stats.txt"))
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
    rows_path = os.path.join(args.workdir, "leven_rows.jsonl")
    open(rows_path, "w").close()
    wanted = set(args.cases.split(",")) if args.cases else None
    for step, limit in STEPS:      # a step that fails or runs out of time ends the run: nothing more is started on the GPU
        if wanted and not step.startswith("build_") and step not in wanted:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", rows_path, "--text-log2", str(args.text_log2),
               "--patterns", str(args.patterns), "--short-patterns", str(args.short_patterns), "--edit-patterns", str(args.edit_patterns),
               "--automaton-patterns", str(args.automaton_patterns), "--seed", str(args.seed), "--min-s", str(args.min_s), "--workdir", args.workdir]
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc:
            print(f"step {step}: exit status {rc}", file=sys.stderr)
            return rc
    with open(rows_path) as f:
        rows = f.read()
    with open(args.out, "w") as f:
        f.write("profiles/leven_stats.txt -- `python tools/leven_bench.py` on one MI355X, %s: occurrences within k edits by exact seeds against\n"
                "%d MiB texts in %d documents (every structure resident); beside it, on the same patterns in alternating windows,\n"
                "femto_amd_hamming_device (the same seeds, a cheaper check: the floor) and, for k <= 2, femto_amd_edit_device with the rows of its\n"
                "ranges located (today's route to the same offsets) and the automaton search with APPROX.  tools/leven_bench.py says how each\n"
                "figure is timed; DESIGN.md \"Occurrences within k edits\" has the kernel's registers.  The same patterns are searched call after\n"
                "call: what they touch of the index stays in the caches, for every route.\n\n"
                % (time.strftime("%Y-%m-%d"), (1 << args.text_log2) >> 20, mb.NDOCS))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
