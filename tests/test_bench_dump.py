"""bench.py --dump-outputs on the host: the files it writes for a batch of CPU tensors shaped like the timed step's results --
float64, the row total, the sampled arrays equal to the results at the sampled positions, the same files from the same
results, and below 64 MB in all at the headline's batch size."""
import os

import numpy as np
import torch

import bench


class _Results:
    """the fields of benchlib.batch.Batch that dump_outputs reads, as CPU tensors"""

    def __init__(self, n, rows, seed):
        rng = np.random.default_rng(seed)
        self.torch, self.dev, self.n = torch, "cpu", n
        first = rng.integers(-1, rows, n)
        last = np.where(rng.random(n) < 0.01, first + rng.integers(0, 3, n), first - 1)
        noccs = np.maximum(last - first + 1, 0).astype(np.int32)
        ostarts = np.concatenate([[0], np.cumsum(noccs, dtype=np.int64)])
        total = int(ostarts[-1])
        self.d_res = torch.from_numpy(np.stack([first, last]))
        self.d_noccs = torch.from_numpy(noccs)
        self.d_ostarts = torch.from_numpy(ostarts)
        self.offsets = torch.from_numpy(np.concatenate([rng.integers(0, rows, total), np.full(64, -1)]))
        self.d_total = torch.tensor([total, 0], dtype=torch.int64)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_batch_is_dumped_whole(tmp_path):
    b = _Results(5000, 1 << 20, 1)
    bench.dump_outputs(str(tmp_path), b, row_free=False)
    got = _load(str(tmp_path))
    assert sorted(got) == ["first", "last", "noccs", "offsets", "out_ends", "out_starts", "total"]
    assert all(a.dtype == np.float64 for a in got.values())
    total = int(b.d_total[0])
    assert got["total"].tolist() == [total]
    assert np.array_equal(got["first"], b.d_res[0].numpy()) and np.array_equal(got["last"], b.d_res[1].numpy())
    assert np.array_equal(got["noccs"], b.d_noccs.numpy())
    assert np.array_equal(got["out_starts"], b.d_ostarts.numpy()[:-1]) and np.array_equal(got["out_ends"], b.d_ostarts.numpy()[1:])
    assert np.array_equal(got["offsets"], b.offsets.numpy()[:total])


def test_row_free_dump_has_no_rows(tmp_path):
    bench.dump_outputs(str(tmp_path), _Results(3000, 1 << 16, 2), row_free=True)
    assert "first" not in _load(str(tmp_path)) and "last" not in _load(str(tmp_path))


def test_headline_size_is_sampled_the_same_way_every_time(tmp_path):
    n = 10_000_000
    b = _Results(n, 1 << 30, 3)
    bench.dump_outputs(str(tmp_path / "a"), b, row_free=False)
    bench.dump_outputs(str(tmp_path / "b"), b, row_free=False)
    a, c = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[k], c[k]) for k in a) and sorted(a) == sorted(c)
    size = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert size <= 64 * 1000 * 1000, size
    assert len(a["first"]) == bench.DUMP_PATTERNS
    # the sampled positions are the same for every per-pattern array: (first, last) and the row counts agree pattern by pattern
    assert np.array_equal(a["noccs"], np.maximum(a["last"] - a["first"] + 1, 0))
    assert np.array_equal(a["out_ends"] - a["out_starts"], a["noccs"])
