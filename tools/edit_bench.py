#!/usr/bin/env python3
"""tools/edit_bench.py [--text-log2 K] [--patterns N] [--out FILE]: search within edit distance (include/femto_amd.h "search within
edit distance") on the two texts of tools/mismatch_bench.py -- 2^K bytes in 64 documents -- and N patterns each:

  dna   uniform ACGT (femto_amd/textgen.py t_acgt); 20-mers, half of them sampled from the text with one random edit planted (a
        substitution, an insertion or a deletion, a third each), half uniform random; k = 1 and k = 2.
  eng   English-like text (t_eng); patterns of 8..64 bytes sampled from the text with one such edit planted; k = 1.

and three ways, in one process per workload:

  edit        femto_amd_edit_device with the capacity (raw records) a counting call reported.  HIP events around back-to-back calls
              after one warm-up call, repeated until the window is at least --min-s seconds; the mean per call.  Reported with the
              raw records, the distinct results and their ratio, which says what pruning duplicate scripts at the source could save.
  mismatch    femto_amd_mismatch_device on the same patterns and k, timed the same way.  It answers less (substitutions only), so
              it is a floor, not a target.
  automaton   the only way to ask the question without the call: the same patterns as APPROX k:1:1:1 through
              femto_amd_nfa_search_batch, on the first --automaton-patterns patterns.  Wall clock (time.perf_counter) around the
              one blocking call, after batches of 64 and 256, automata compiled and marshalled beforehand; reported per pattern.
              The tool checks, on these patterns, that every automaton result (first, last, length, cost) is in the call's list
              under (first, length) with the same last and a cost no higher.  An absent result is read through the extractor: a
              string that holds a code below 5 is what the definition excludes (at most 5 % may be such); any other must be more
              than k operations away from its pattern by a plain dynamic programme -- the automaton route reports a few strings
              one symbol longer than the match it paid for -- and both kinds are counted.

Every GPU step is a child process of its own under its own time limit, and the first failure ends the run; one JSON line per
measurement, all written to --out (default profiles/edit_stats.txt)."""
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

from mismatch_bench import NDOCS, index_path, policy_of, step_build, text_of, timed      # noqa: E402

STEPS = [("build_dna", 600), ("build_eng", 600), ("dna1", 600), ("dna2", 900), ("eng1", 900)]


def planted(plen, flat, alphabet, rng):
    """one edit per pattern at a random position: substitution by another character, insertion of a random one, deletion"""
    starts = np.concatenate([[0], np.cumsum(plen, dtype=np.int64)])
    kind = rng.integers(0, 3, len(plen))
    at = (rng.random(len(plen)) * plen).astype(np.int64)
    ch = alphabet[rng.integers(0, len(alphabet), len(plen))]
    out = []
    for q in range(len(plen)):
        p = flat[starts[q]:starts[q + 1]]
        i, c = int(at[q]), ch[q]
        if kind[q] == 0:
            p = p.copy()
            p[i] = c if c != p[i] else alphabet[(int(np.searchsorted(alphabet, c)) + 1) % len(alphabet)]
        elif kind[q] == 1:
            p = np.insert(p, i, c)
        else:
            p = np.delete(p, i)
        out.append(p)
    return np.array([len(p) for p in out], dtype=np.int32), np.ascontiguousarray(np.concatenate(out), dtype=np.uint16)


def distance(p, w):
    """the fewest substitutions, deletions and insertions that turn p into w (byte codes only)"""
    row = list(range(len(w) + 1))
    for i in range(1, len(p) + 1):
        new = [i] + [0] * len(w)
        for j in range(1, len(w) + 1):
            new[j] = min(row[j - 1] + (int(p[i - 1]) != int(w[j - 1])), row[j] + 1, new[j - 1] + 1)
        row = new
    return row[len(w)]


def patterns_of(args, which):
    """(plen int32[n], flat uint16[], byte characters of the text, what the patterns are)"""
    from femto_amd import textgen as tg
    text = text_of(args, which)
    n = args.patterns
    alphabet = np.flatnonzero(np.bincount(text, minlength=256)).astype(np.uint16) + 5
    rng = np.random.Generator(np.random.PCG64(args.seed + 3))
    if which == "eng":
        plen, flat = tg.p_hit(8, 64, n, args.seed + 2, text)
        plen, flat = planted(plen, flat, alphabet, rng)
        return plen, flat, len(alphabet), "lengths 8..64 sampled from the text, one edit planted (substitution, insertion or deletion, a third each)"
    half = n // 2
    plen, flat = tg.p_hit(20, 20, half, args.seed + 2, text)
    plen, flat = planted(plen, flat, alphabet, rng)
    rlen, rflat = tg.p_rand(20, n - half, args.seed + 4)
    pats = np.split(flat, np.cumsum(plen)[:-1]) + np.split(rflat, n - half)
    order = rng.permutation(n)      # the two kinds mixed
    pats = [pats[i] for i in order]
    return (np.array([len(p) for p in pats], dtype=np.int32), np.ascontiguousarray(np.concatenate(pats), dtype=np.uint16), len(alphabet),
            "20-mers: half sampled from the text with one edit planted (substitution, insertion or deletion, a third each), half uniform random")


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
    clock = "HIP events, mean of back-to-back calls after a warm-up call"

    # ---- the call
    d_rs, d_tot = i64(n + 1), i64(3)
    ix.edit_device(n, nsyms, d_syms, d_starts, k, 0, None, None, None, None, None, d_tot, stream=st)
    torch.cuda.synchronize()
    raw = int(d_tot.cpu()[2])
    d_first, d_last, d_cost, d_len = i64(raw), i64(raw), i32(raw), i32(raw)
    call = lambda: ix.edit_device(n, nsyms, d_syms, d_starts, k, raw, d_rs, d_first, d_last, d_cost, d_len, d_tot, stream=st)      # noqa: E731
    ms, reps = timed(call, args.min_s)
    total = int(d_tot.cpu()[0])
    assert d_tot.cpu().tolist() == [total, 0, raw]
    rs = d_rs.cpu().numpy()
    first, last = d_first[:total].cpu().numpy(), d_last[:total].cpu().numpy()
    cost, length = d_cost[:total].cpu().numpy(), d_len[:total].cpu().numpy()
    us_a = ms * 1e3 / n
    report(what="edit", text=which, k=k, ms=round(ms, 4), calls=reps, patterns=n, symbols=nsyms, byte_characters=nsub,
           lanes=(nsyms + n) * (2 * nsub + 1), us_per_pattern=round(us_a, 5), mpatterns_per_s=round(n / ms / 1e3, 3), raw_records=raw, results=total,
           raw_per_result=round(raw / max(total, 1), 3), results_by_cost=np.bincount(cost, minlength=3).tolist(),
           patterns_with_a_result=int((np.diff(rs) > 0).sum()), policy=kind, pattern_set=what, clock=clock)

    # ---- substitutions only, the same patterns: a floor
    m_rs, m_tot = i64(n + 1), i64(2)
    ix.mismatch_device(n, nsyms, d_syms, d_starts, k, 0, m_rs, None, None, None, None, None, m_tot, stream=st)
    torch.cuda.synchronize()
    mt = int(m_tot.cpu()[0])
    m_first, m_last, m_cost, m_pos, m_sym = i64(mt), i64(mt), i32(mt), i32(2 * mt), i16(2 * mt)
    ms_m, reps_m = timed(lambda: ix.mismatch_device(n, nsyms, d_syms, d_starts, k, mt, m_rs, m_first, m_last, m_cost, m_pos, m_sym, m_tot, stream=st), args.min_s)
    report(what="mismatch", text=which, k=k, ms=round(ms_m, 4), calls=reps_m, patterns=n, results=mt, us_per_pattern=round(ms_m * 1e3 / n, 5),
           edit_over_mismatch=round(ms / ms_m, 2), clock=clock)
    del m_first, m_last, m_cost, m_pos, m_sym

    # ---- the automaton route: APPROX k:1:1:1 on the first M patterns
    def automaton(m):
        regexes = [b"".join(b"\\x%02x" % (int(c) - 5) for c in flat[starts[q]:starts[q + 1]]) for q in range(m)]
        batch = femto_amd.NfaBatch([femto_amd.Nfa.from_regex(r, (k, 1, 1, 1)) for r in regexes])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ix.nfa_search_batch(batch, max_results=1 << 22)
        return time.perf_counter() - t0, out
    automaton(64)
    automaton(256)
    m = min(n, args.automaton_patterns)
    s_m, out = automaton(m)
    a_start, a_first, a_last, a_len, a_cost, a_status = out[:6]
    assert not a_status.any(), "an automaton search ended with a status"
    found = int(a_start[-1])
    # both routes agree: every automaton result is listed under (pattern, first, length), with its last row and a cost no higher
    key = lambda q, f, ln: (q.astype(np.int64) << 44) | (f.astype(np.int64) << 8) | ln.astype(np.int64)      # noqa: E731
    assert ix.info.total_length < (1 << 36) and m < (1 << 19) and int(plen.max()) + 2 < 256
    mine_q = np.repeat(np.arange(n), np.diff(rs))[:int(rs[m])]
    mine = key(mine_q, first[:int(rs[m])], length[:int(rs[m])])
    assert (np.diff(mine) > 0).all()          # the order the header states, and no string twice
    theirs = key(np.repeat(np.arange(m), np.diff(a_start)), a_first[:found], a_len[:found])
    at = np.searchsorted(mine, theirs).clip(0, max(len(mine) - 1, 0))
    hit = mine[at] == theirs if len(mine) else np.zeros(found, dtype=bool)
    absent = np.flatnonzero(~hit)
    below5, farther = 0, 0
    for i in absent:          # only strings the definition excludes: a code below 5 in them, or more than k operations away
        q = int(np.searchsorted(a_start, i, side="right")) - 1
        ctx, _ = ix.context(rows=[int(a_first[i])], before=0, after=int(a_len[i]))
        if (ctx[0] < 5).any():
            below5 += 1
            continue
        d = distance(flat[starts[q]:starts[q + 1]], ctx[0])
        assert d > k, ("an automaton result the call does not list", q, int(a_first[i]), int(a_last[i]), int(a_len[i]), int(a_cost[i]), d)
        farther += 1
    assert below5 * 20 <= max(found, 1)
    assert (last[at[hit]] == a_last[:found][hit]).all() and (cost[at[hit]] <= a_cost[:found][hit]).all(), "a listed string with another last row or a higher cost"
    us_b = s_m * 1e6 / m
    report(what="automaton", text=which, k=k, approx="%d:1:1:1" % k, patterns=m, seconds=round(s_m, 3), us_per_pattern=round(us_b, 3),
           kpatterns_per_s=round(m / s_m / 1e3, 3), results=found, edit_results_same_patterns=int(rs[m]), absent_for_a_code_below_5=below5, absent_and_more_than_k_operations_away=farther,
           cheaper_in_the_call=int((cost[at[hit]] < a_cost[:found][hit]).sum()), edit_speedup_per_pattern=round(us_b / us_a, 1),
           clock="time.perf_counter around one blocking femto_amd_nfa_search_batch, automata compiled beforehand; after batches of 64 and 256")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--automaton-patterns", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_stats.txt"))
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
    rows_path = os.path.join(args.workdir, "edit_rows.jsonl")
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
        f.write("profiles/edit_stats.txt -- `python tools/edit_bench.py` on one MI355X, %s: search within edit distance k for %d patterns\n"
                "against %d MiB texts in %d documents (every structure resident), femto_amd_mismatch_device on the same patterns (it answers\n"
                "less: a floor) and the same question through the automaton search (APPROX k:1:1:1), which the tool checks the call against.\n"
                "tools/edit_bench.py says how each figure is timed; DESIGN.md \"Search within edit distance\" has the kernels' registers.\n"
                "The same patterns are searched call after call: what they touch of the index stays in the caches, for all three ways.\n\n"
                % (time.strftime("%Y-%m-%d"), args.patterns, (1 << args.text_log2) >> 20, NDOCS))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
