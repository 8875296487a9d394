#!/usr/bin/env python3
"""tools/extract_bench.py [--text-log2 K] [--windows N] [--only text|samples|context]: extraction on a random-ACGT index
(include/femto_amd.h "extraction").  Prints one JSON line per measurement; every time comes from HIP events around
back-to-back calls after a warm-up, in a window of at least --min-s seconds.

  text      the all-HBM handle (hbm_budget_bytes = everything free; it holds the text): N windows of 64 symbols at random offsets
  samples   the handle of 4 x text bytes without the text (sample path): table build, table bytes, the same windows and one
            whole-document extract (2^K + 1 symbols)
  context   before = after = 32 around N random rows on the all-HBM handle, and through locate_device -> context_device

Byte model (reported against 8 TB/s): text path 3 B per symbol (1 read, 2 written) + 24 B per request (pos, len, start);
sample path 2 B written + 128 B per LF step, with 1 + 2^(s-1) / len steps per symbol on average.  This is also the command
rocprofv3 --kernel-trace --stats profiles for profiles/extract_*.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12


def timed(fn, min_s):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, ms = 1, 0.0
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_s * 1e3:
            return ms / reps
        reps = max(reps * 2, int(reps * min_s * 1e3 / max(ms, 1e-3) * 1.1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=30)
    ap.add_argument("--windows", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--only", default="", choices=["", "text", "samples", "context"])
    ap.add_argument("--workdir", default=os.environ.get("FEMTO_AMD_BENCH_DIR", "/tmp/femto_amd_bench"))
    args = ap.parse_args()
    import torch
    import femto_amd
    from femto_amd import textgen as tg
    n = 1 << args.text_log2
    path = os.path.join(args.workdir, f"acgt_2p{args.text_log2}_s{args.seed}")
    if not os.path.exists(os.path.join(path, "_femto_index")):
        os.makedirs(args.workdir, exist_ok=True)
        femto_amd.build_index(path, [tg.t_acgt(n, args.seed)], params=None, infos=["bench"], device=0)
    dev = "cuda:0"
    rng = np.random.default_rng(args.seed)
    W = 64
    m = args.windows
    d_pos = torch.from_numpy(rng.integers(0, n - W, m).astype(np.int64)).to(dev)
    d_len = torch.full((m,), W, dtype=torch.int32, device=dev)
    d_starts = torch.arange(0, m * W, W, dtype=torch.int64, device=dev)
    d_out = torch.empty(m * W + 8, dtype=torch.int16, device=dev)

    def windows(ex):
        return lambda: ex.extract_device(m, d_pos.data_ptr(), d_len.data_ptr(), d_starts.data_ptr(), d_out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)

    def report(what, ms, syms, bytes_model, **kw):
        print(json.dumps(dict(what=what, ms=round(ms, 4), symbols=syms, gsym_per_s=round(syms / ms / 1e6, 3),
                              model_bytes=int(bytes_model), tb_per_s=round(bytes_model / ms / 1e9, 3),
                              of_peak=round(bytes_model / ms / 1e9 / (PEAK / 1e12), 3), **kw)), flush=True)

    if args.only in ("", "text", "context"):
        ix = femto_amd.Index(path, device=0, options={"hbm_budget_bytes": femto_amd.BUDGET_ALL})
        ex = ix.extractor()
        assert ex.info()["path"] == ex.PATH_TEXT
        if args.only in ("", "text"):
            report("text_windows64", timed(windows(ex), args.min_s), m * W, m * W * 3 + m * 20)
        if args.only in ("", "context"):
            d_rows = torch.from_numpy(rng.integers(0, n + 1, m).astype(np.int64)).to(dev)
            d_ctx = torch.empty(m * 64 + 8, dtype=torch.int16, device=dev)
            d_p = torch.empty(m, dtype=torch.int64, device=dev)
            ctx = lambda: ex.context_device(m, d_rows=d_rows.data_ptr(), before=32, after=32, d_ctx=d_ctx.data_ptr(),   # noqa: E731
                                            d_pos_out=d_p.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            report("context32_rows", timed(ctx, args.min_s), m * 64, m * 64 * 3 + m * 24)
            # the chain: locate 20-mers sampled from the text, then a window around every hit
            text = tg.t_acgt(n, args.seed)
            npat = max(1, m // 4)
            at = rng.integers(0, n - 20, npat)
            pats = (text[at[:, None] + np.arange(20)[None, :]].astype(np.uint16) + 5).reshape(-1)
            d_plen = torch.full((npat,), 20, dtype=torch.int32, device=dev)
            d_flat = torch.from_numpy(pats.view(np.int16)).to(dev)
            d_pst = torch.arange(0, npat * 20, 20, dtype=torch.int64, device=dev)
            cap = npat * 8
            d_n, d_st = torch.zeros(npat, dtype=torch.int32, device=dev), torch.zeros(npat + 1, dtype=torch.int64, device=dev)
            d_off, d_tot = torch.empty(cap, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
            d_ctx2 = torch.empty(cap * 64 + 8, dtype=torch.int16, device=dev)

            def chain():
                st = torch.cuda.current_stream().cuda_stream
                ix.locate_device(npat, d_plen.data_ptr(), d_flat.data_ptr(), d_pst.data_ptr(), 7, 0, 0, d_n.data_ptr(), d_st.data_ptr(),
                                 d_off.data_ptr(), cap, d_tot.data_ptr(), stream=st)
                ex.context_device(cap, d_offsets=d_off.data_ptr(), d_n=d_tot.data_ptr(), before=32, after=32, d_ctx=d_ctx2.data_ptr(),
                                  stream=st)
            ms = timed(chain, args.min_s)
            hits = int(d_tot[0])
            report("locate20_context32_chain", ms, hits * 64, hits * 64 * 3, patterns=npat, hits=hits)
        ix.close()

    if args.only in ("", "samples"):
        ix = femto_amd.Index(path, device=0, options={"hbm_budget_bytes": 4 * n, "text": 0})
        t0 = time.perf_counter()
        ex = ix.extractor()
        wall = (time.perf_counter() - t0) * 1e3
        info = ex.info()
        assert info["path"] == ex.PATH_SAMPLES
        print(json.dumps(dict(what="sample_table", bytes=info["bytes"], sample_shift=info["sample_shift"], build_ms=round(info["build_ms"], 1),
                              open_wall_ms=round(wall, 1), hbm_allocated=ix.structures()["hbm_allocated"])), flush=True)
        s = info["sample_shift"]
        steps = 1 + (1 << (s - 1)) / W
        report("samples_windows64", timed(windows(ex), args.min_s), m * W, m * W * (2 + 128 * steps) + m * 20)
        d_doc = torch.empty(n + 16, dtype=torch.int16, device=dev)
        d_dp = torch.zeros(1, dtype=torch.int64, device=dev)
        d_dl = torch.full((1,), n + 1, dtype=torch.int32, device=dev)
        d_ds = torch.zeros(1, dtype=torch.int64, device=dev)
        doc = lambda: ex.extract_device(1, d_dp.data_ptr(), d_dl.data_ptr(), d_ds.data_ptr(), d_doc.data_ptr(),   # noqa: E731
                                        torch.cuda.current_stream().cuda_stream)
        report("samples_whole_document", timed(doc, args.min_s), n + 1, (n + 1) * (2 + 128))
        ix.close()


if __name__ == "__main__":
    main()
