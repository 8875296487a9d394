"""Worker of test_striped_index_across_processes: one rank of a 2-process striped index on one GPU.
argv: out_dir then (index_dir golden.npz) pairs.  Rank 0 derives the striped index and serves its stripes as file
descriptors; rank 1 attaches (femto_amd_open_striped_client).  Writes out_dir/ok<rank> when every check passed."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import femto_amd  # noqa: E402
from femto_amd import parallel  # noqa: E402
from gpu_common import assert_answers, compare, device_chain, patterns_of, want_from_golden  # noqa: E402  (tests/ is sys.path[0])


def check(ix, g, want_mode):
    assert ix.rank_mode == want_mode, (ix.rank_mode, want_mode)
    plen, flat, starts = patterns_of(g)
    for mode in (want_mode, 1):                      # the fast path of this alphabet and the wavelet path
        ix.set_rank_mode(mode)
        assert_answers(ix, plen, flat, starts, want_from_golden(g), leaves=True, what=mode)
    ix.set_rank_mode(want_mode)
    # the enqueue-only chain on device-resident inputs (what bench.py times)
    want = want_from_golden(g, clamps=(7,))
    cap = len(want.locate[0][2]) + 8
    compare(want, ("chain",), 0, chain=device_chain(ix, plen, flat, starts, 7, cap, stream=torch.cuda.current_stream().cuda_stream), capacity=cap)


def main():
    import faulthandler
    faulthandler.enable()
    out_dir = sys.argv[1]
    pairs = list(zip(sys.argv[2::3], sys.argv[3::3], sys.argv[4::3]))
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    for k, (index, gold_path, mode) in enumerate(pairs):
        g = np.load(gold_path)
        sock = os.path.join(out_dir, f"stripes{k}.sock")
        ix, keep = parallel.open_striped_shared(index, 0, sock, devices=[0, 0])
        pi = ix.pack_info()
        assert pi["level_table"] and pi["sa_full"], pi
        check(ix, g, int(mode))
        dist.barrier()
        ix.close()
        if keep is not None:
            keep.close()
        dist.barrier()
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
