"""CPU suite: bench.dump_outputs, the writer behind `bench.py --dump-outputs DIR` (float32 files, the 64 MiB cap, the seeded sample)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _step_and_out():
    step = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Linear(128, 13))
    g = torch.Generator().manual_seed(3)
    out = dict(loss=torch.tensor(0.75, dtype=torch.float64), score=torch.rand(4000, generator=g, dtype=torch.float16), note=1)
    return step, out


def test_dump_writes_every_returned_array_and_the_parameters(tmp_path):
    bench = _bench()
    step, out = _step_and_out()
    assert bench.dump_outputs(str(tmp_path), out, step) == ["loss", "parameters", "score"]
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == () and float(got["loss"]) == 0.75
    assert np.array_equal(got["score"], out["score"].float().numpy())
    assert np.array_equal(got["parameters"], torch.cat([p.detach().reshape(-1) for p in step.parameters()]).numpy())


def test_dump_samples_what_exceeds_the_limit_the_same_way_every_time(tmp_path):
    bench = _bench()
    step, out = _step_and_out()
    n_par = sum(p.numel() for p in step.parameters())
    limit = 3 * 4096 + 4 * 10000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, step, limit=limit)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert a["loss"].shape == () and a["score"].size == 4000        # small arrays whole
    assert a["parameters"].size == 10000 - 1 - 4000 < n_par           # the largest one sampled into what is left
    assert np.isin(a["parameters"], torch.cat([p.detach().reshape(-1) for p in step.parameters()]).numpy()).all()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
