"""`-m gpu`: the traced twins of the direct pipeline (femto_amd_trace_lines / femto_amd_trace_reads, csrc/trace_kernels.hip), which
bench.py's roofline takes its compulsory lines from.

The twins are the production kernels' sources, launched by the production launch code (csrc/direct_launch.hpp).  Per handle
configuration -- every rank layout of the search, the hand-over text tail and the walking row plan (dense_arrays=0), a handle
without text -- and for both forms of the chain (option trace_row_free) a trace must
  * count the rows femto_amd_locate_plan_device counts for the same batch and clamp,
  * report, per traced array, no more distinct lines than line reads,
  * report nothing for the arrays the layout lacks,
  * touch the level table or the context table in the count phase,
  * return the same numbers when it is run again, and
  * leave the scratch (flags, block sums) fit for the next real launch: the device chain still answers the goldens.
The batch is the fixture's golden pattern list repeated to 257 patterns: two workgroups share the block sums.
Every dictionary is printed (pytest -s shows them): two builds of the library must print the same lines."""
import numpy as np
import pytest

import femto_amd
from gpu_common import assert_answers, want_from_golden
from regexp_util import KINDS

pytestmark = pytest.mark.gpu

NPATS = 257
CLAMPS = [1, 300]
MODE3_LACKS = ("level1_lines", "level2_lines", "char_rank_lines", "context_table")
MODE4_LACKS = ("pack_lines", "rank_units")
# name -> (fixture, the rank layout by regexp_util.KINDS, options on top of the kind's, regions the handle has no array for)
CONFIGS = {
    "ru": ("acgt48k", "ru", {}, MODE3_LACKS),
    "rum": ("acgt48k", "rum", {}, MODE3_LACKS + ("text", "isa")),
    "pack": ("acgt48k", "pack", {}, MODE3_LACKS + ("rank_units",)),
    "rum_sampled": ("acgt48k", "rum", dict(text=1), MODE3_LACKS),                     # hand-over tail and mark spotting together
    "ru_sampled": ("acgt48k", "ru", dict(rank_units=2, dense_arrays=0), MODE3_LACKS),      # (auto would take the marked units here)
    "ru_no_text": ("acgt48k", "ru", dict(rank_units=2, text=0), MODE3_LACKS + ("text", "isa")),
    "ind": ("eng2doc", "ind", {}, MODE4_LACKS),
    "pack2": ("eng2doc", "pack2", {}, MODE4_LACKS + ("char_rank_lines",)),
    "ind_sampled": ("eng2doc", "ind", dict(dense_arrays=0), MODE4_LACKS),
}


def _open_config(path, name):
    """the handle of one configuration on GPU 0; skips when the fixture does not produce the layout the name claims"""
    _, kind, extra, _ = CONFIGS[name]
    opts = dict(KINDS[kind].options or {}, **extra)
    ix = femto_amd.Index(path, device=0, options=opts or None)
    pi, st = ix.pack_info(), ix.structures()
    ok = KINDS[kind].proves(ix)
    if opts.get("text") == 0:                         # no text, no suffix array: the rows are walked to marks
        ok = ok and st["text_sa_isa"] == 0 and not pi["sa_full"]
    elif opts.get("dense_arrays") == 0:               # sampled arrays with the text: the tail is handed over to count_tail_kernel
        ok = ok and st["text_sa_isa"] > 0 and not pi["sa_full"]
    else:                                             # everything resident: the inline tail, offsets from the suffix array
        ok = ok and pi["sa_full"] and pi["isa_full"]
    if not ok:
        ix.close()
        pytest.skip(f"{name}: the fixture does not open as this configuration ({pi}, text_sa_isa {st['text_sa_isa']})")
    return ix


def _batch(fx):
    """the fixture's golden patterns repeated to NPATS, 8 zero symbols on either side of the symbol array"""
    plen, flat, starts = fx.patterns
    reps = -(-NPATS // len(plen))
    pl = np.tile(plen, reps)[:NPATS].astype(np.int32)
    st = np.tile(starts, reps)[:NPATS].astype(np.int64) + 8
    return pl, np.concatenate([np.zeros(8, np.uint16), flat, np.zeros(8, np.uint16)]), st


def _fmt(d):
    return " ".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trace_follows_the_chain(gpu_ok, fixtures, name):
    import torch
    fx = fixtures(CONFIGS[name][0])
    lacks = CONFIGS[name][3]
    ix = _open_config(fx.index, name)
    try:
        dev = "cuda:0"
        plen, flat, starts = _batch(fx)
        d_plen, d_flat, d_starts = torch.from_numpy(plen).to(dev), torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(starts).to(dev)
        first, last = torch.zeros(NPATS, dtype=torch.int64, device=dev), torch.zeros(NPATS, dtype=torch.int64, device=dev)
        noccs, ostarts = torch.zeros(NPATS, dtype=torch.int32, device=dev), torch.zeros(NPATS + 1, dtype=torch.int64, device=dev)
        for mo in CLAMPS:
            ix.locate_plan_device(NPATS, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), mo, first.data_ptr(), last.data_ptr(),
                                  noccs.data_ptr(), ostarts.data_ptr())
            torch.cuda.synchronize()
            want_rows = int(ostarts[NPATS].item())
            assert want_rows == int(noccs.sum().item()) and want_rows > 0, (name, mo, want_rows)
            for rf in (0, 1):
                ix.set_option("trace_row_free", rf)
                what = (name, "max_occs", mo, "row_free", rf)
                cl, ll, rows = ix.trace_lines(NPATS, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), mo)
                cr, lr = ix.trace_reads()
                for phase, lines, reads in (("count", cl, cr), ("locate", ll, lr)):
                    print(f"trace {name} max_occs={mo} row_free={rf} {phase} lines: {_fmt(lines)}")
                    print(f"trace {name} max_occs={mo} row_free={rf} {phase} reads: {_fmt(reads)}")
                print(f"trace {name} max_occs={mo} row_free={rf} rows={rows}")
                assert rows == want_rows, what + (rows, want_rows)
                for phase, lines, reads in (("count", cl, cr), ("locate", ll, lr)):
                    for region in femto_amd.Index.TRACE_REGIONS:
                        assert 0 <= lines[region] <= reads[region], what + (phase, region, lines[region], reads[region])
                    for region in lacks:
                        assert lines[region] == 0 and reads[region] == 0, what + (phase, "a region the layout lacks", region, lines[region], reads[region])
                assert cl["level_table"] + cl["context_table"] > 0, what + ("the count phase reads neither table", cl)
                again = ix.trace_lines(NPATS, d_plen.data_ptr(), d_flat.data_ptr(), d_starts.data_ptr(), mo)
                assert again == (cl, ll, rows) and ix.trace_reads() == (cr, lr), what + ("a second trace differs", again, ix.trace_reads())
            ix.set_option("trace_row_free", 0)
        # the scratch the traces used serves the next real launches: with rows and row-free
        assert_answers(ix, *fx.patterns, want_from_golden(fx.gold), host=False, chain=True, row_free=True, what=(name, "after the traces"))
    finally:
        ix.close()
