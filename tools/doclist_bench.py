#!/usr/bin/env python3
"""tools/doclist_bench.py [--text-log2 K] [--docs D] [--patterns N] [--max-occs M] [--steps S]: document listing on a
many-document index (include/femto_amd.h "document listing").  Prints one JSON line per measurement.

  The index: 2^K bytes of textgen.t_eng text cut into D documents of equal length (default 64 MiB, 100 000 documents), built
  with femto_amd.build_index.  The batch: N substrings of 6..12 bytes sampled from the text (those that straddle a document
  boundary match nothing), located with the clamp M.

  device   locate_device -> doclist_device on one stream, enqueue-only; HIP events around S back-to-back steps after a warm-up,
           and the same for locate_device alone (the difference is what the listing adds)
  host     the same lists the way tools/femto_amd_search.cpp makes them today: the located offsets copied to the host,
           resolve_batch, sort, unique (one numpy sort of (pattern, document) keys for the whole batch); host clock, a few steps

The two must agree list for list; the tool checks that before it reports.  This is also the command
rocprofv3 --kernel-trace --stats profiles for profiles/doclist_stats.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--max-occs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
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
    dev = "cuda:0"
    m = args.patterns
    plen, flat = tg.p_hit(6, 12, m, args.seed + 1, text)
    d_plen, d_flat, d_pst = torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(tg.starts_of(plen)).to(dev)
    d_n, d_st = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m + 1, dtype=torch.int64, device=dev)
    d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def locate(d_off, cap):
        ix.locate_device(m, d_plen.data_ptr(), d_flat.data_ptr(), d_pst.data_ptr(), args.max_occs, 0, 0, d_n.data_ptr(), d_st.data_ptr(),
                         d_off.data_ptr(), cap, d_tot.data_ptr(), stream=st)

    tiny = torch.empty(16, dtype=torch.int64, device=dev)
    locate(tiny, 16)                    # sizing run: the row total
    torch.cuda.synchronize()
    rows = int(d_tot[0])
    cap = rows + 16
    d_off = torch.empty(cap, dtype=torch.int64, device=dev)
    d_nd = torch.zeros(m, dtype=torch.int32, device=dev)
    d_docs, d_hits = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    d_dt, d_status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def chain():
        locate(d_off, cap)
        ix.doclist_device(m, d_st.data_ptr(), d_off.data_ptr(), cap, d_tot.data_ptr(), d_ndocs=d_nd.data_ptr(), d_docs=d_docs.data_ptr(),
                          d_hits=d_hits.data_ptr(), d_doc_total=d_dt.data_ptr(), d_status=d_status.data_ptr(), stream=st)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    ms_locate = timed(lambda: locate(d_off, cap))
    ms_chain = timed(chain)
    assert int(d_status[0]) == 0 and int(d_tot[0]) == rows
    out_starts, ndocs = d_st.cpu().numpy(), d_nd.cpu().numpy()
    sizes = np.diff(out_starts)
    w, g = femto_amd.doclist_info()
    common = dict(text_bytes=n, documents=args.docs, patterns=m, max_occs=args.max_occs, rows=rows, lists_total=int(d_dt[0]),
                  segments_wave=int((sizes <= w).sum()), segments_workgroup=int(((sizes > w) & (sizes <= g)).sum()), segments_global=int((sizes > g).sum()))
    print(json.dumps(dict(what="locate_device", ms=round(ms_locate, 4), steps=args.steps, **common)), flush=True)
    print(json.dumps(dict(what="locate_then_doclist_device", ms=round(ms_chain, 4), doclist_ms=round(ms_chain - ms_locate, 4), steps=args.steps,
                          gpat_per_s=round(m / ms_chain / 1e6, 3), grows_per_s=round(rows / ms_chain / 1e6, 3))), flush=True)

    # the host's way, from the same located rows
    seg = np.repeat(np.arange(m, dtype=np.int64), sizes)
    best, parts = None, None
    for _ in range(args.host_steps):
        t0 = time.perf_counter()
        offs = d_off[:rows].cpu().numpy()
        t1 = time.perf_counter()
        doc, _ = ix.resolve_batch(offs)
        t2 = time.perf_counter()
        key = np.sort(seg * (args.docs + 1) + doc)
        u, c = np.unique(key, return_counts=True)
        t3 = time.perf_counter()
        if best is None or t3 - t0 < best:
            best, parts = t3 - t0, (t1 - t0, t2 - t1, t3 - t2)
    h_seg, h_doc = u // (args.docs + 1), u % (args.docs + 1)
    h_nd = np.bincount(h_seg, minlength=m)
    assert np.array_equal(h_nd, ndocs), "the device's list sizes differ from the host's"
    slot = out_starts[:-1][h_seg] + (np.arange(len(u)) - np.concatenate([[0], np.cumsum(h_nd)])[:-1][h_seg])
    assert np.array_equal(d_docs.cpu().numpy()[slot], h_doc) and np.array_equal(d_hits.cpu().numpy()[slot], c), "the device's lists differ from the host's"
    print(json.dumps(dict(what="host_listing", ms=round(best * 1e3, 2), copy_back_ms=round(parts[0] * 1e3, 2), resolve_batch_ms=round(parts[1] * 1e3, 2),
                          sort_unique_ms=round(parts[2] * 1e3, 2), steps=args.host_steps, note="best of steps; host clock")), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
