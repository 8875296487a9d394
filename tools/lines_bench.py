#!/usr/bin/env python3
"""tools/lines_bench.py [--text-log2 K] [--hits N] [--out FILE]: the line around every hit (include/femto_amd.h "matching
lines") on an English-like text (femto_amd/textgen.py t_eng, lines of ~150 bytes), two ways:

  lines     femto_amd_lines_device + femto_amd_line_bytes_device + femto_amd_line_groups_device on the offsets
            femto_amd_locate_device left in HBM -- each call alone, and the three as one chain.  HIP events around back-to-back
            calls after one warm-up call, repeated until the window is at least --min-s seconds; the mean per call is reported.
  context   what a caller had before these calls: femto_amd_context_device(1023, 1024) in chunks of --chunk anchors, every
            chunk copied back (2047 uint16 per hit), the terminators found with numpy, equal lines grouped in a dict.  Wall
            clock (time.perf_counter) from the first launch to the last group, device idle before and after; one warm-up of
            one chunk, then --context-reps full repeats, each reported.

Both produce line_pos / line_len of every hit and the number of distinct lines; the tool checks that they agree before it
reports.  One JSON line per measurement, also appended to --out (default profiles/lines_stats.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--hits", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--context-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines_stats.txt"))
    ap.add_argument("--workdir", default=os.environ.get("FEMTO_AMD_BENCH_DIR", "/tmp/femto_amd_bench"))
    args = ap.parse_args()
    import torch
    import femto_amd
    from femto_amd import textgen as tg
    n = 1 << args.text_log2
    text = tg.t_eng(n, args.seed)
    path = os.path.join(args.workdir, f"eng_2p{args.text_log2}_s{args.seed}")
    if not os.path.exists(os.path.join(path, "_femto_index")):
        os.makedirs(args.workdir, exist_ok=True)
        femto_amd.build_index(path, [text], params=None, infos=["bench"], device=0)
    rows = []

    def report(**kw):
        rows.append(json.dumps(kw))
        print(rows[-1], flush=True)

    dev = "cuda:0"
    rng = np.random.default_rng(args.seed)
    ix = femto_amd.Index(path, device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
    ex = ix.extractor()
    # patterns: 4-grams of the text, at most 64 rows each, as many as give --hits rows
    npat = args.hits // 8
    at = rng.integers(0, n - 4, npat)
    flat = (text[at[:, None] + np.arange(4)[None, :]].astype(np.uint16) + 5).reshape(-1)
    plen, starts = np.full(npat, 4, dtype=np.int32), np.arange(0, npat * 4, 4, dtype=np.int64)
    noccs, _ = ix.locate_flat(plen, flat, starts, 64)
    npat = int(np.searchsorted(np.cumsum(noccs.astype(np.int64)), args.hits, side="right"))
    hits = int(noccs[:npat].sum())
    d_plen, d_flat, d_pst = (torch.from_numpy(plen[:npat]).to(dev), torch.from_numpy(flat[:npat * 4].view(np.int16)).to(dev),
                             torch.from_numpy(starts[:npat]).to(dev))
    cap = hits
    d_nocc, d_st = torch.zeros(npat, dtype=torch.int32, device=dev), torch.zeros(npat + 1, dtype=torch.int64, device=dev)
    d_off, d_tot = torch.empty(cap, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ix.locate_device(npat, d_plen.data_ptr(), d_flat.data_ptr(), d_pst.data_ptr(), 64, 0, 0, d_nocc.data_ptr(), d_st.data_ptr(), d_off.data_ptr(),
                     cap, d_tot.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert d_tot.cpu().tolist() == [hits, 0]
    report(what="setup", text_bytes=n, patterns=npat, hits=hits, extractor_path=ex.info()["path"], device=torch.cuda.get_device_name(0))

    # ---- lines: bounds, bytes, groups
    d_doc, d_pos = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    d_len, d_fl = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
    d_bst, d_bt = torch.empty(cap + 1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    d_gf, d_ng = torch.empty(cap, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    bounds = lambda: ex.lines_device(cap, d_off.data_ptr(), d_tot.data_ptr(), d_doc.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(),   # noqa: E731
                                     d_fl.data_ptr(), stream=st)
    bounds()
    torch.cuda.synchronize()
    bcap = int(d_len.sum().item())
    d_by = torch.empty(bcap + 64, dtype=torch.uint8, device=dev)
    pack = lambda: ex.line_bytes_device(cap, d_pos.data_ptr(), d_len.data_ptr(), d_bst.data_ptr(), d_by.data_ptr(), bcap, d_bt.data_ptr(),   # noqa: E731
                                        d_n=d_tot.data_ptr(), stream=st)
    groups = lambda: ex.line_groups_device(cap, d_bst.data_ptr(), d_by.data_ptr(), d_gf.data_ptr(), d_ng.data_ptr(), d_flags=d_fl.data_ptr(),   # noqa: E731
                                           d_n=d_tot.data_ptr(), stream=st)

    def chain():
        bounds()
        pack()
        groups()
    clock = "HIP events, mean of back-to-back calls after a warm-up call"
    for what, fn in (("lines_bounds", bounds), ("lines_bytes", pack), ("lines_groups", groups), ("lines_chain", chain)):
        ms, reps = timed(fn, args.min_s)
        report(what=what, ms=round(ms, 4), calls=reps, hits=hits, line_bytes=bcap, mhits_per_s=round(hits / ms / 1e3, 2), clock=clock)
    assert d_bt.cpu().tolist() == [bcap, 0]
    g_pos, g_len, g_distinct = d_pos.cpu().numpy(), d_len.cpu().numpy(), int(d_ng.item())

    # ---- context: the windows back on the host, numpy for the terminators, a dict for the groups
    W = 2047
    d_ctx = torch.empty(args.chunk * W, dtype=torch.int16, device=dev)
    offs = d_off.cpu().numpy()
    doc_len = n      # one document: the window of a context never leaves it

    def context_way(limit):
        pos, lens, seen = np.zeros(limit, dtype=np.int64), np.zeros(limit, dtype=np.int32), {}
        for c0 in range(0, limit, args.chunk):
            cn = min(args.chunk, limit - c0)
            ex.context_device(cn, d_offsets=d_off.data_ptr() + 8 * c0, before=1023, after=1024, d_ctx=d_ctx.data_ptr(), stream=st)
            ctx = d_ctx[:cn * W].cpu().numpy().view(np.uint16).reshape(cn, W)
            stop = (ctx == 15) | (ctx == 18) | (ctx == 5)
            o = offs[c0:c0 + cn]
            back = stop[:, 1022::-1]                       # nearest first
            fb = back.any(axis=1)
            kb = np.where(fb, back.argmax(axis=1), np.minimum(o, 1023))
            fwd = stop[:, 1023:]
            ff = fwd.any(axis=1)
            room = doc_len - o
            kf = np.where(ff, fwd.argmax(axis=1), np.where(room >= 1024, 1023, np.maximum(room - 1, 0)))
            pos[c0:c0 + cn] = o - kb
            lens[c0:c0 + cn] = kb + kf
            raw = (ctx - 5).astype(np.uint8)
            for i in range(cn):
                seen.setdefault(raw[i, 1023 - kb[i]:1023 + kf[i]].tobytes(), c0 + i)
        return pos, lens, len(seen)

    torch.cuda.synchronize()
    context_way(min(args.chunk, hits))
    for rep in range(args.context_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c_pos, c_len, c_distinct = context_way(hits)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(c_pos, g_pos) and np.array_equal(c_len, g_len) and c_distinct == g_distinct
        report(what="context_1023_1024_numpy", ms=round(ms, 1), repeat=rep, hits=hits, copied_back_bytes=hits * W * 2, distinct_lines=c_distinct,
               mhits_per_s=round(hits / ms / 1e3, 3), clock="time.perf_counter around the whole loop, device synchronised before and after")
    ix.close()
    with open(args.out, "w") as f:
        f.write("profiles/lines_stats.txt -- `python tools/lines_bench.py` on one MI355X: the line around every located hit of a %d MiB\n"
                "English-like text, by the matching-lines calls and by context(1023, 1024) + copy back + numpy.  tools/lines_bench.py\n"
                "says how each figure is timed.\n\n" % (n >> 20))
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
