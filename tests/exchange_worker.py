"""Worker of test_walker_exchange_across_processes: one rank of a range-split index (one process per rank) that locates by
WALKER EXCHANGE -- femto_amd/parallel.py exchange_locate with this rank's femto_amd_lf_steps_device as its step, so every
LF step of every walk runs on the part that owns the row, and walkers change process when their next row does.
argv: fixture_dir (index/ and doc* as conftest.Fixture unpacks them) out_dir.  Writes out_dir/ok<rank> when every check passed."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from femto_amd import parallel  # noqa: E402
from sa_util import suffix_array  # noqa: E402  (tests/ is sys.path[0])


def main():
    fixture_dir, out_dir = sys.argv[1:3]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    # the reference: the suffix array of the prepared text (every document's bytes + 5, then SEOF = 2)
    docs = [np.fromfile(os.path.join(fixture_dir, f), dtype=np.uint8) for f in sorted(os.listdir(fixture_dir)) if f.startswith("doc")]
    sa = suffix_array(np.concatenate([np.append(d.astype(np.uint16) + 5, np.uint16(2)) for d in docs]))
    ix = parallel.open_range_split(os.path.join(fixture_dir, "index"), dev)
    info = ix.info
    n, bs, nb = int(info.total_length), int(info.block_size), int(info.number_of_blocks)
    assert n == len(sa) and ix.split_info()["nparts"] == world and ix.split_info()["part"] == rank
    bounds = parallel.split_bounds(nb, world)
    seen = {"rows": 0, "first": None}

    def lf_step(rows):
        blk = rows // bs
        assert bool(((blk >= bounds[rank]) & (blk < bounds[rank + 1])).all()), "stepped a row this rank does not own"
        d = rows.to(f"cuda:{dev}")
        a, b = torch.empty_like(d), torch.empty_like(d)
        ix.lf_steps_device(d.numel(), d.data_ptr(), a.data_ptr(), b.data_ptr())
        torch.cuda.synchronize()
        if seen["first"] is None:
            seen["first"] = rows.clone()
        seen["rows"] += rows.numel()
        return a.cpu(), b.cpu()

    # this rank asks for a strided share of ALL rows (most of them owned by other ranks)
    want = torch.arange(rank, n, world * 3, dtype=torch.int64)
    stats = {}
    got = parallel.exchange_locate(lf_step, want, bs, nb, stats=stats, total_length=n)
    assert np.array_equal(got.numpy(), sa[want.numpy()]), (rank, int((got.numpy() != sa[want.numpy()]).sum()))
    assert 1 <= stats["rounds"] <= info.mark_period + 3, stats
    # the first rows this rank stepped are the walkers that START on its rows, and row mod (world * 3) names the rank that
    # asked for each: some were asked for by another rank
    mine = torch.arange(bounds[rank] * bs, min(bounds[rank + 1] * bs, n), dtype=torch.int64)
    assert seen["rows"] > 0 and seen["first"] is not None, (rank, seen["rows"])
    first = torch.sort(seen["first"]).values
    assert torch.equal(first, mine[mine % (world * 3) < world]), (rank, first.numel())
    assert int((first % (world * 3) != rank).sum()) > 0 and seen["rows"] > first.numel(), (rank, seen["rows"], first.numel())
    dist.barrier()      # keep every owner's memory alive until all ranks are done reading it
    ix.close()
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
