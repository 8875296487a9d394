#!/usr/bin/env python3
"""tools/mismatch_bench.py [--text-log2 K] [--patterns N] [--out FILE]: search with substitutions (include/femto_amd.h "search with
substitutions") on two texts of 2^K bytes in 64 documents and N patterns each:

  dna   uniform ACGT (femto_amd/textgen.py t_acgt); 20-mers, half of them sampled from the text with one substitution planted, half
        uniform random; k = 1 and k = 2.
  eng   English-like text (t_eng); patterns of 8..64 bytes sampled from the text; k = 1.

and three ways, in one process per workload:

  mismatch    femto_amd_mismatch_device with the capacity a counting call reported.  HIP events around back-to-back calls after one
              warm-up call, repeated until the window is at least --min-s seconds; the mean per call.
  automaton   the only way to ask the question without the call: the same patterns as APPROX k:1:k+1:k+1 (substitutions only)
              through femto_amd_nfa_search_batch, on the first --automaton-patterns patterns (50 000: the automata are compiled
              one by one on the host, and the route's time per pattern no longer changes with the batch at that size).  Wall
              clock (time.perf_counter) around the one blocking call, after batches of 64 and 256, automata compiled and
              marshalled beforehand; reported per pattern.
  enumerated  (dna, k = 1 only) the 61 strings within one substitution of every pattern written out -- on the device, not timed --
              and counted by femto_amd_count_device; HIP events as for mismatch.  The tool checks that the non-empty ranges are
              as many as the results of mismatch.

Every GPU step is a child process of its own under its own time limit, and the first failure ends the run; one JSON line per
measurement, all written to --out (default profiles/mismatch_stats.txt)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("build_dna", 600), ("build_eng", 600), ("dna1", 600), ("dna2", 600), ("eng1", 900)]
NDOCS = 64


def timed(fn, min_s):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 1
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_s * 1e3:
            return ms / reps, reps
        reps = max(reps * 2, int(reps * min_s * 1e3 / max(ms, 1e-3) * 1.1))


def text_of(args, which):
    from femto_amd import textgen as tg
    return tg.t_acgt(1 << args.text_log2, args.seed) if which == "dna" else tg.t_eng(1 << args.text_log2, args.seed)


def index_path(args, which):
    return os.path.join(args.workdir, f"{which}_2p{args.text_log2}_s{args.seed}_d{NDOCS}")


def step_build(args, report, which):
    import femto_amd
    path = index_path(args, which)
    if not os.path.exists(os.path.join(path, "_femto_index")):
        os.makedirs(args.workdir, exist_ok=True)
        text = text_of(args, which)
        t0 = time.perf_counter()
        femto_amd.build_index(path, np.array_split(text, NDOCS), params=None, infos=["doc%d" % k for k in range(NDOCS)], device=0)
        report(what="build", text=which, text_bytes=len(text), documents=NDOCS, seconds=round(time.perf_counter() - t0, 1))


def patterns_of(args, which):
    """(plen int32[n], flat uint16[], characters of the text, what the patterns are)"""
    from femto_amd import textgen as tg
    text = text_of(args, which)
    n = args.patterns
    nchars = int(np.count_nonzero(np.bincount(text, minlength=256)))
    if which == "eng":
        plen, flat = tg.p_hit(8, 64, n, args.seed + 2, text)
        return plen, flat, nchars, "lengths 8..64 sampled from the text"
    half = n // 2
    plen, flat = tg.p_hit(20, 20, half, args.seed + 2, text)
    rng = np.random.Generator(np.random.PCG64(args.seed + 3))
    at = np.arange(half, dtype=np.int64) * 20 + rng.integers(0, 20, half)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8).astype(np.uint16) + 5
    flat[at] = lut[(np.searchsorted(lut, flat[at]) + rng.integers(1, 4, half)) % 4]
    rlen, rflat = tg.p_rand(20, n - half, args.seed + 4)
    flat = np.ascontiguousarray(np.concatenate([flat, rflat]).reshape(n, 20)[rng.permutation(n)].reshape(-1))      # the two kinds mixed
    return np.concatenate([plen, rlen]), flat, nchars, "20-mers: half sampled from the text with one substitution planted, half uniform random"


def policy_of(ix):
    pi = ix.pack_info()
    if ix.rank_mode == 3:
        return ("RumPolicy" if pi["rank_units_marked"] else "RuPolicy") if pi["rank_units"] else "PackPolicy"
    if ix.rank_mode == 4:
        return "IndPolicy" if pi["char_rank_lines"] else "Pack2Policy"
    return "LanePolicy"


def step_query(args, report, which, k):
    import torch
    import femto_amd
    dev = "cuda:0"
    plen, flat, nsub, what = patterns_of(args, which)
    n, nsyms = len(plen), int(plen.sum())
    starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)]).astype(np.int64)
    ix = femto_amd.Index(index_path(args, which), device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    kind = policy_of(ix)
    st = torch.cuda.current_stream().cuda_stream
    i64 = lambda c: torch.zeros(max(c, 1), dtype=torch.int64, device=dev)      # noqa: E731
    i32 = lambda c: torch.zeros(max(c, 1), dtype=torch.int32, device=dev)      # noqa: E731
    i16 = lambda c: torch.zeros(max(c, 1), dtype=torch.int16, device=dev)      # noqa: E731
    d_syms = torch.from_numpy(flat.view(np.int16)).to(dev)
    d_starts = torch.from_numpy(starts).to(dev)
    d_rs, d_tot = i64(n + 1), i64(2)
    ix.mismatch_device(n, nsyms, d_syms, d_starts, k, 0, d_rs, None, None, None, None, None, d_tot, stream=st)
    torch.cuda.synchronize()
    total = int(d_tot.cpu()[0])
    d_first, d_last, d_cost, d_pos, d_sym = i64(total), i64(total), i32(total), i32(2 * total), i16(2 * total)
    call = lambda: ix.mismatch_device(n, nsyms, d_syms, d_starts, k, total, d_rs, d_first, d_last, d_cost, d_pos, d_sym, d_tot, stream=st)      # noqa: E731
    clock = "HIP events, mean of back-to-back calls after a warm-up call"
    ms, reps = timed(call, args.min_s)
    assert d_tot.cpu().tolist() == [total, 0]
    cost = d_cost[:total].cpu().numpy()
    us_a = ms * 1e3 / n
    report(what="mismatch", text=which, k=k, ms=round(ms, 4), calls=reps, patterns=n, symbols=nsyms, substitutes=nsub, lanes=nsyms * nsub,
           us_per_pattern=round(us_a, 5), mpatterns_per_s=round(n / ms / 1e3, 3), results=total, results_by_cost=np.bincount(cost, minlength=3).tolist(),
           patterns_with_a_result=int((np.diff(d_rs.cpu().numpy()) > 0).sum()), policy=kind, pattern_set=what, clock=clock)

    # ---- the automaton route: APPROX k:1:k+1:k+1 on the first M patterns
    def regexes(m):
        return [b"".join(b"\\x%02x" % (int(c) - 5) for c in flat[starts[q]:starts[q + 1]]) for q in range(m)]

    def automaton(m):
        batch = femto_amd.NfaBatch([femto_amd.Nfa.from_regex(r, (k, 1, k + 1, k + 1)) for r in regexes(m)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ix.nfa_search_batch(batch, max_results=1 << 22)
        return time.perf_counter() - t0, out
    automaton(64)
    automaton(256)
    m = min(n, args.automaton_patterns)
    s_m, out = automaton(m)
    assert not out[5].any(), "an automaton search ended with a status"
    found = int(out[0][-1])
    mine = int(d_rs.cpu().numpy()[m])
    us_b = s_m * 1e6 / m
    report(what="automaton", text=which, k=k, approx="%d:1:%d:%d" % (k, k + 1, k + 1), patterns=m, seconds=round(s_m, 3), us_per_pattern=round(us_b, 3),
           kpatterns_per_s=round(m / s_m / 1e3, 3), results=found, mismatch_results_same_patterns=mine, mismatch_speedup_per_pattern=round(us_b / us_a, 1),
           clock="time.perf_counter around one blocking femto_amd_nfa_search_batch, automata compiled beforehand; after batches of 64 and 256")
    assert found <= mine, "the automaton route found results the call does not list"

    # ---- dna, k = 1: the 61 strings of every pattern, counted
    if which == "dna" and k == 1:
        base = d_syms.view(n, 20)
        lut = torch.tensor([ord(c) + 5 for c in "ACGT"], dtype=torch.int16, device=dev)
        idx = torch.bucketize(base.to(torch.int32), lut.to(torch.int32))
        pos = torch.arange(20, device=dev).repeat_interleave(3)
        j = torch.arange(3, device=dev).repeat(20)
        v = base.unsqueeze(1).repeat(1, 61, 1)
        v[:, 1 + torch.arange(60, device=dev), pos] = lut[(idx[:, pos] + 1 + j) % 4]
        nv = n * 61
        buf = i16(nv * 20 + 16)
        buf[8:8 + nv * 20] = v.reshape(-1)
        del v, idx
        v_plen = torch.full((nv,), 20, dtype=torch.int32, device=dev)
        v_starts = torch.arange(nv, dtype=torch.int64, device=dev) * 20
        v_first, v_last = i64(nv), i64(nv)
        count = lambda: ix.count_device(nv, v_plen.data_ptr(), buf.data_ptr() + 16, v_starts.data_ptr(), v_first.data_ptr(), v_last.data_ptr(), stream=st)      # noqa: E731
        ms_c, reps_c = timed(count, args.min_s)
        hits = int((v_first <= v_last).sum().item())
        assert hits == total, ("enumeration and the call disagree", hits, total)
        report(what="enumerated", text=which, k=k, ms=round(ms_c, 4), calls=reps_c, patterns=n, variants=nv, us_per_pattern=round(ms_c * 1e3 / n, 5),
               non_empty=hits, level_table=bool(ix.pack_info()["level_table"]), level_table_syms=int(ix.pack_info()["ktab_syms"]),
               mismatch_over_enumerated=round(ms / ms_c, 3), clock=clock + "; the enumeration itself is not timed")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--automaton-patterns", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch_stats.txt"))
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
            step_query(args, report, args.step[:3], int(args.step[3:]))
        return 0
    os.makedirs(args.workdir, exist_ok=True)
    rows_path = os.path.join(args.workdir, "mismatch_rows.jsonl")
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
        f.write("profiles/mismatch_stats.txt -- `python tools/mismatch_bench.py` on one MI355X, %s: search with up to k substitutions for %d patterns\n"
                "against %d MiB texts in %d documents (every structure resident), the same question through the automaton search\n"
                "(APPROX k:1:k+1:k+1) and, for DNA and k = 1, the 61 strings of every pattern counted one by one.\n"
                "tools/mismatch_bench.py says how each figure is timed; DESIGN.md \"Search with substitutions\" has the kernels' registers.\n"
                "The same patterns are searched call after call: what they touch of the index stays in the caches, for all three ways.\n\n"
                % (time.strftime("%Y-%m-%d"), args.patterns, (1 << args.text_log2) >> 20, NDOCS))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
