#!/usr/bin/env python3
"""tools/similar_bench.py [--text-log2 K] [--query-log2 Q] [--out FILE]: the sequences a file shares with the index (include/femto_amd.h
"common sequences") on an English-like text (femto_amd/textgen.py t_eng) split into documents, for two queries:

  fresh   2^Q bytes of t_eng from ANOTHER seed (another vocabulary: short matches);
  cut     2^Q bytes cut from the indexed text with one substitution per 64 bytes (long matches), max_len 32768.

and three ways:

  match_stats   femto_amd_match_stats_device alone.  HIP events around back-to-back calls after one warm-up call, repeated until the
                window is at least --min-s seconds; the mean per call.  The step counts come from
                femto_amd_match_stats_steps_device (one call, not timed).
  chain         match_stats + common_sequences + common_groups + similar_documents back to back on one stream, timed the same way.
  rounds        the same len[] the only way it could be had without the kernel: rounds of femto_amd_count_device over the
                still-alive end positions, patterns one symbol longer each round (the shape of the reference's step()); the counts
                are copied back and the survivors compacted with numpy between rounds.  Wall clock (time.perf_counter) around the
                whole loop, device idle before and after, after a warm-up of three rounds; the loop runs once.

The tool checks that rounds and kernel agree on every len[j] before it reports.  Every GPU step is a child process of its own
under its own time limit; one JSON line per measurement, all written to --out (default profiles/similar_stats.txt)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# -Rpass-analysis=kernel-resource-usage of match_stats_kernel<P, false> (hipcc --offload-arch=gfx950 -O3): VGPRs, waves per SIMD
RESOURCES = {"RumPolicy": (34, 8), "RuPolicy": (38, 8), "PackPolicy": (60, 7), "IndPolicy": (45, 8), "Pack2Policy": (66, 7), "LanePolicy": (67, 7)}
STEPS = [("build", 900), ("fresh", 300), ("cut", 600)]
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


def index_text(args):
    from femto_amd import textgen as tg
    return tg.t_eng(1 << args.text_log2, args.seed)


def index_path(args):
    return os.path.join(args.workdir, f"eng_2p{args.text_log2}_s{args.seed}_d{NDOCS}")


def step_build(args, report):
    import femto_amd
    path = index_path(args)
    if not os.path.exists(os.path.join(path, "_femto_index")):
        os.makedirs(args.workdir, exist_ok=True)
        text = index_text(args)
        docs = np.array_split(text, NDOCS)
        t0 = time.perf_counter()
        femto_amd.build_index(path, docs, params=None, infos=["doc%d" % k for k in range(NDOCS)], device=0)
        report(what="build", text_bytes=len(text), documents=NDOCS, seconds=round(time.perf_counter() - t0, 1))


def step_query(args, report, which):
    import torch
    import femto_amd
    from femto_amd import textgen as tg
    n = 1 << args.query_log2
    if which == "fresh":
        q = tg.t_eng(n, args.seed + 1)
    else:
        text = index_text(args)
        at = (len(text) // NDOCS) * 10 + 12345
        q = text[at:at + n].copy()
        q[::64] ^= 0x20
        del text
    dev = "cuda:0"
    ix = femto_amd.Index(index_path(args), device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    kind = "IndPolicy" if ix.pack_info()["char_rank_lines"] else "Pack2Policy"
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    buf[8:8 + n] = torch.from_numpy(q).to(dev)
    d_q = buf.data_ptr() + 8
    i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device=dev)      # noqa: E731
    i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)      # noqa: E731
    d_len, d_first, d_last, d_steps = i32(n), i64(n), i64(n), i64(2)
    stats = lambda: ix.match_stats_device(n, d_q, d_len, d_first, d_last, stream=st)      # noqa: E731
    ix.match_stats_steps_device(n, d_q, d_steps, stream=st)
    torch.cuda.synchronize()
    steps, single = d_steps.cpu().tolist()
    vg, occ = RESOURCES[kind]
    clock = "HIP events, mean of back-to-back calls after a warm-up call"
    ms, reps = timed(stats, args.min_s)
    lens = d_len.cpu().numpy()
    report(what="match_stats", query=which, ms=round(ms, 4), calls=reps, query_bytes=n, ns_per_byte=round(ms * 1e6 / n, 3), search_steps=steps,
           gsteps_per_s=round(steps / ms / 1e6, 3), single_row_step_share=round(single / max(steps, 1), 4), mean_len=round(float(lens.mean()), 2),
           max_len_seen=int(lens.max()), policy=kind, vgprs=vg, waves_per_simd=occ, clock=clock)

    # ---- the whole chain
    cap = n
    s_start, s_len, s_first, s_last, s_tot = i64(cap), i32(cap), i64(cap), i64(cap), i64(2)
    g_of, g_len, g_first, g_last, g_here, g_ms, ng = i64(cap), i32(cap), i64(cap), i64(cap), i32(cap), i64(cap), i64(2)
    nd = ix.info.number_of_documents
    score, seqs, tot = i64(nd), i32(nd), i64(2)
    ocap = 1 << 22
    offs = i64(ocap)

    def chain():
        stats()
        ix.common_sequences_device(n, d_len, d_first, d_last, s_start, s_len, s_first, s_last, cap, s_tot, stream=st)
        ix.common_groups_device(cap, s_tot, s_start, s_len, s_first, s_last, g_of, g_len, g_first, g_last, g_here, g_ms, ng, stream=st)
        ix.similar_documents_device(cap, ng, g_len, g_first, g_last, g_here, offs, ocap, score, seqs, tot, stream=st)
    chain()
    torch.cuda.synchronize()
    if tot.cpu().tolist()[1]:       # the rows did not fit: size the buffer to them
        ocap = int(tot.cpu().tolist()[0])
        offs = i64(ocap)
    ms_c, reps_c = timed(chain, args.min_s)
    assert tot.cpu().tolist()[1] == 0
    report(what="chain", query=which, ms=round(ms_c, 4), calls=reps_c, query_bytes=n, ns_per_byte=round(ms_c * 1e6 / n, 3),
           gsteps_per_s=round(steps / ms_c / 1e6, 3), sequences=int(s_tot.cpu()[0]), groups=int(ng.cpu()[0]), located_rows=int(tot.cpu()[0]),
           offsets_capacity=ocap, documents_scored=int((score != 0).sum().item()), clock=clock)

    # ---- rounds of femto_amd_count_device: pattern j of length L is symbols [j - L + 1, j] of the query, so a round uploads only
    # (plen, starts) of the alive positions
    sym = torch.zeros(n + 16, dtype=torch.int16, device=dev)
    sym[8:8 + n] = torch.from_numpy((q.astype(np.uint16) + 5).view(np.int16)).to(dev)
    d_sym = sym.data_ptr() + 16
    d_cf, d_cl = i64(n), i64(n)

    def rounds(limit):
        out = np.zeros(n, dtype=np.int32)
        alive = np.arange(n, dtype=np.int64)
        L = 1
        while len(alive) and L <= min(limit, 32768):
            alive = alive[alive >= L - 1]
            k = len(alive)
            if not k:
                break
            d_plen = torch.full((k,), L, dtype=torch.int32, device=dev)
            d_st = torch.from_numpy(alive - (L - 1)).to(dev)
            ix.count_device(k, d_plen.data_ptr(), d_sym, d_st.data_ptr(), d_cf.data_ptr(), d_cl.data_ptr(), stream=st)
            ok = (d_cf[:k] <= d_cl[:k]).cpu().numpy()
            alive = alive[ok]
            out[alive] = L
            L += 1
        return out, L - 1
    torch.cuda.synchronize()
    rounds(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r_len, nrounds = rounds(1 << 30)
    torch.cuda.synchronize()
    ms_r = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(r_len, lens), "rounds and kernel disagree"
    report(what="rounds_of_count_device", query=which, ms=round(ms_r, 2), rounds=nrounds, query_bytes=n, ns_per_byte=round(ms_r * 1e6 / n, 3),
           match_stats_speedup=round(ms_r / ms, 2), clock="time.perf_counter around the whole loop (host compaction between rounds included), "
           "device synchronised before and after; the loop runs once after a warm-up of three rounds")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--query-log2", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_stats.txt"))
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
        if args.step == "build":
            step_build(args, report)
        else:
            step_query(args, report, args.step)
        return 0
    os.makedirs(args.workdir, exist_ok=True)
    rows_path = os.path.join(args.workdir, "similar_rows.jsonl")
    open(rows_path, "w").close()
    for step, limit in STEPS:      # a step that fails or runs out of time ends the run: nothing more is started on the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", rows_path, "--text-log2", str(args.text_log2),
               "--query-log2", str(args.query_log2), "--seed", str(args.seed), "--min-s", str(args.min_s), "--workdir", args.workdir]
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc:
            print(f"step {step}: exit status {rc}", file=sys.stderr)
            return rc
    with open(rows_path) as f:
        rows = f.read()
    with open(args.out, "w") as f:
        f.write("profiles/similar_stats.txt -- `python tools/similar_bench.py` on one MI355X: matching statistics and the common-sequence chain\n"
                "for a %d MiB query against a %d MiB English-like text in %d documents (every structure resident), and the same len[] by\n"
                "rounds of femto_amd_count_device.  tools/similar_bench.py says how each figure is timed.  match_stats_kernel, from\n"
                "-Rpass-analysis=kernel-resource-usage (VGPRs, waves per SIMD): %s.\n"
                "The same query is searched call after call: the rank lines it touches are a small part of the index and stay in the\n"
                "caches, for the kernel and for the rounds alike.\n\n"
                % ((1 << args.query_log2) >> 20, (1 << args.text_log2) >> 20, NDOCS, ", ".join("%s %d / %d" % (k, v[0], v[1]) for k, v in RESOURCES.items())))
        f.write(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
