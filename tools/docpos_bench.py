#!/usr/bin/env python3
"""tools/docpos_bench.py [--text-log2 K] [--docs D] [--patterns N] [--max-occs M] [--steps S] [--balance-n N]: the positional
operators (include/femto_amd.h "positional operators").  Prints one JSON line per measurement.

  chain    the index and the batch of tools/doclist_bench.py (2^K bytes of textgen.t_eng text in D documents, N substrings of
           6..12 bytes located with the clamp M); pattern k is combined with pattern k + N/2 (THEN 64 / WITHIN 64 / OR in turn):
           locate_device -> doclist_device (pairs form) -> docpos_device on one stream, enqueue-only.  HIP events around S
           back-to-back steps after a warm-up, for locate alone, locate + list and the whole chain: the differences are the steps.
  host     the same answer from the pair lists copied back, by the closed form in numpy (one searchsorted per side over
           (job, document, offset) keys for the whole batch); host clock, best of a few steps.  The two must agree.
  balance  N + N strictly ascending pairs (default N = 10 M) combined with WITHIN 8 as ONE job and as N / 10 jobs of 10 + 10 (the
           same arrays, only the views differ), in merged elements per second.  b[i] = a[i] + 0 or 1 and a's steps are 2..9, so
           every job's two slices cover the same range and both shapes find partners everywhere; the short shape only loses the
           partners across its job boundaries.  The yardstick is femto_amd_docset_device OR on the same lists as single int64
           keys (document * 4096 + offset), at both shapes.

This is also the command rocprofv3 --kernel-trace --stats profiles for profiles/docpos_stats.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THEN, WITHIN, OR = 0, 1, 2


def host_closed(jobs, pd, po, a_start, a_n, b_start, b_n, ops, ds):
    """the closed form for a whole batch: every job's result, as sorted (job, document, offset) keys"""
    m = int(po.max(initial=0)) + 1
    top = int(pd.max(initial=0)) + 1

    def keys(start, n):
        job = np.repeat(np.arange(jobs, dtype=np.int64), n)
        idx = np.repeat(start - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()), dtype=np.int64)
        return job, (job * top + pd[idx]) * m + po[idx]

    ja, ka = keys(a_start, a_n.astype(np.int64))
    jb, kb = keys(b_start, b_n.astype(np.int64))
    assert jobs * top * m < 2 ** 62
    j = np.minimum(np.searchsorted(kb, ka, side="left"), len(kb) - 1)
    near_l = kb[j] // m == ka // m                           # the first r >= l, in l's job and document
    wl = kb[j] - ka
    i = np.minimum(np.searchsorted(ka, kb, side="right"), len(ka) - 1)
    near_r = ka[i] // m == kb // m                           # the first l > r
    wr = ka[i] - kb
    opa, da = ops[ja], ds[ja].astype(np.int64)
    opb, db = ops[jb], ds[jb].astype(np.int64)
    left = np.where(opa == THEN, near_l & (da > 0) & (wl > 0) & (wl <= da), np.where(opa == WITHIN, near_l & (wl >= 0) & (wl <= abs(da)), True))
    right = np.where(opb == THEN, near_r & (db < 0) & (wr > 0) & (wr <= -db), np.where(opb == WITHIN, near_r & (wr > 0) & (wr <= abs(db)), True))
    return np.union1d(ka[left], kb[right]), top, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=26)
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--max-occs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--balance-n", type=int, default=10_000_000)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--workdir", default=os.environ.get("FEMTO_AMD_BENCH_DIR", "/tmp/femto_amd_bench"))
    args = ap.parse_args()
    import torch
    import femto_amd
    from femto_amd import textgen as tg
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = "cuda:0"
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
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn, steps=args.steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    if not args.skip_chain:
        m = args.patterns
        jobs = m // 2
        plen, flat = tg.p_hit(6, 12, m, args.seed + 1, text)
        d_plen, d_flat, d_pst = torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(tg.starts_of(plen)).to(dev)
        d_n, d_st = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m + 1, dtype=torch.int64, device=dev)
        d_tot = torch.zeros(2, dtype=torch.int64, device=dev)

        def locate(d_off, cap):
            ix.locate_device(m, d_plen.data_ptr(), d_flat.data_ptr(), d_pst.data_ptr(), args.max_occs, 0, 0, d_n.data_ptr(), d_st.data_ptr(),
                             d_off.data_ptr(), cap, d_tot.data_ptr(), stream=st)

        tiny = torch.empty(16, dtype=torch.int64, device=dev)
        locate(tiny, 16)                    # sizing run: the row total
        torch.cuda.synchronize()
        rows = int(d_tot[0])
        cap = rows + 16
        d_off = torch.empty(cap, dtype=torch.int64, device=dev)
        d_pd, d_po = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
        ops = (np.arange(jobs) % 3).astype(np.int32)
        ds = np.full(jobs, 64, dtype=np.int32)
        d_op, d_di = torch.from_numpy(ops).to(dev), torch.from_numpy(ds).to(dev)
        d_rs, d_rt = torch.zeros(jobs + 1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        d_rd, d_ro = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)

        def listing():
            locate(d_off, cap)
            ix.doclist_device(m, d_st.data_ptr(), d_off.data_ptr(), cap, d_tot.data_ptr(), d_pair_doc=d_pd.data_ptr(), d_pair_off=d_po.data_ptr(),
                              d_status=d_status.data_ptr(), stream=st)

        def chain():
            listing()
            ix.docpos_device(jobs, d_pd.data_ptr(), d_po.data_ptr(), d_st.data_ptr(), d_n.data_ptr(), d_pd.data_ptr(), d_po.data_ptr(),
                             d_st.data_ptr() + 8 * jobs, d_n.data_ptr() + 4 * jobs, d_op.data_ptr(), d_di.data_ptr(), d_rs.data_ptr(),
                             d_rd.data_ptr(), d_ro.data_ptr(), cap, d_rt.data_ptr(), stream=st)

        ms_locate = timed(lambda: locate(d_off, cap))
        ms_list = timed(listing)
        ms_chain = timed(chain)
        assert int(d_status[0]) == 0 and int(d_tot[0]) == rows and int(d_rt[1]) == 0
        total = int(d_rt[0])
        print(json.dumps(dict(what="locate_list_combine_device", ms=round(ms_chain, 4), locate_ms=round(ms_locate, 4), list_ms=round(ms_list - ms_locate, 4),
                              combine_ms=round(ms_chain - ms_list, 4), steps=args.steps, text_bytes=n, documents=args.docs, patterns=m, jobs=jobs,
                              max_occs=args.max_occs, rows=rows, result_pairs=total, tile=femto_amd.docpos_info(),
                              gelem_per_s_combine=round(rows / (ms_chain - ms_list) / 1e6, 3))), flush=True)
        out_starts, noccs = d_st.cpu().numpy(), d_n.cpu().numpy()
        best, parts = None, None
        for _ in range(args.host_steps):
            t0 = time.perf_counter()
            pd, po = d_pd[:rows].cpu().numpy(), d_po[:rows].cpu().numpy()
            t1 = time.perf_counter()
            keys, top, mm = host_closed(jobs, pd, po, out_starts[:jobs], noccs[:jobs], out_starts[jobs:2 * jobs], noccs[jobs:2 * jobs], ops, ds)
            t2 = time.perf_counter()
            if best is None or t2 - t0 < best:
                best, parts = t2 - t0, (t1 - t0, t2 - t1)
        assert len(keys) == total, "the device's result size differs from the host's"
        rs = d_rs.cpu().numpy()
        assert np.array_equal(np.bincount(keys // (top * mm), minlength=jobs), np.diff(rs)), "the device's result starts differ from the host's"
        assert np.array_equal(d_rd[:total].cpu().numpy(), keys // mm % top) and np.array_equal(d_ro[:total].cpu().numpy(), keys % mm), \
            "the device's results differ from the host's"
        print(json.dumps(dict(what="host_combine", ms=round(best * 1e3, 2), copy_back_ms=round(parts[0] * 1e3, 2), closed_form_ms=round(parts[1] * 1e3, 2),
                              steps=args.host_steps, note="best of steps; host clock")), flush=True)
        del d_off, d_pd, d_po, d_rd, d_ro

    # ---- balance: the same N + N pairs as one job and as jobs of 10 + 10
    per_short = 10
    nb = args.balance_n // per_short * per_short
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    ka = torch.cumsum(torch.randint(2, 10, (nb,), generator=g, device=dev, dtype=torch.int64), 0)
    kb = ka + torch.randint(0, 2, (nb,), generator=g, device=dev, dtype=torch.int64)
    a_doc, a_off, b_doc, b_off = ka >> 12, ka & 4095, kb >> 12, kb & 4095
    cap = 2 * nb
    d_rd, d_ro = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    d_rt = torch.zeros(2, dtype=torch.int64, device=dev)
    spreads = {}
    for shape, per in (("one_job", nb), ("jobs_of_10_plus_10", per_short)):
        jobs = nb // per
        start = torch.arange(jobs, dtype=torch.int64, device=dev) * per
        cnt = torch.full((jobs,), per, dtype=torch.int32, device=dev)
        d_rs = torch.zeros(jobs + 1, dtype=torch.int64, device=dev)
        for name, fn in (("docpos_within_8", lambda: ix.docpos_device(jobs, a_doc.data_ptr(), a_off.data_ptr(), start.data_ptr(), cnt.data_ptr(), b_doc.data_ptr(),
                                                                       b_off.data_ptr(), start.data_ptr(), cnt.data_ptr(), op.data_ptr(), di.data_ptr(),
                                                                       d_rs.data_ptr(), d_rd.data_ptr(), d_ro.data_ptr(), cap, d_rt.data_ptr(), stream=st)),
                         ("docset_or_yardstick", lambda: ix.docset_device(jobs, ka.data_ptr(), start.data_ptr(), cnt.data_ptr(), kb.data_ptr(), start.data_ptr(),
                                                                           cnt.data_ptr(), op.data_ptr(), d_rs.data_ptr(), d_rd.data_ptr(), cap, d_rt.data_ptr(), stream=st))):
            op = torch.full((jobs,), WITHIN if name.startswith("docpos") else femto_amd.DOCSET_OR, dtype=torch.int32, device=dev)
            di = torch.full((jobs,), 8, dtype=torch.int32, device=dev)
            steps = max(3, args.steps // 5)
            runs = [timed(fn, steps) for _ in range(3)]                 # three timed runs: their spread is the run-to-run spread
            assert int(d_rt[1]) == 0
            spreads[(shape, name)] = runs
            print(json.dumps(dict(what="balance", kernel=name, shape=shape, jobs=jobs, merged_elements=2 * nb, result=int(d_rt[0]),
                                  ms=[round(r, 4) for r in runs], gelem_per_s=round(2 * nb / min(runs) / 1e6, 3), steps=steps,
                                  note="three runs of `steps` back-to-back calls; elements per second from the best")), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
