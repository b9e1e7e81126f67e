"""CPU suite: the deferred ``OpenSegEvaluator`` under two ranks over gloo -- the histogram is all-reduced, the batches' records are
exchanged as tensors (one all_gather of the (4,) record, no object pickling), and nothing is read before ``summary()``."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["mIoU", "mAcc", "allAcc", "aupr", "auroc", "loss"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch(b, rank):
    g = torch.Generator().manual_seed(100 * b + rank)
    logits, score, seg = torch.randn(500, 6, generator=g), torch.rand(500, generator=g), torch.randint(0, 6, (500,), generator=g)
    seg[torch.rand(500, generator=g) < 0.1] = -1
    if rank == 1 and b == 1:
        seg[seg == 4] = 0   # this rank's batch holds no unknown point: its record (n_pos == 0) is gathered and dropped at the flush
    return logits, score, seg, torch.rand((), generator=g)


def _deferred_eval_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from pointcloudpdf_amd import evaluator

    dist.init_process_group("gloo", rank=rank, world_size=world)

    def no_pickling(*a, **k):
        raise AssertionError("the deferred evaluator exchanges tensors, not pickled objects")

    dist.all_gather_object = no_pickling
    ev = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=True)
    for b in range(3):
        logits, score, seg, loss = _batch(b, rank)
        ev.update(logits, score, seg, loss=loss)
        assert ev._aupr == [] and len(ev._records) == b + 1 and ev._records[-1].shape == (world, 4)
    out = ev.summary()
    out["n_records"] = len(ev.aupr)
    torch.save(out, os.path.join(out_dir, f"eval_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_deferred_evaluator_equals_the_eager_one(tmp_path):
    """engines/hooks/evaluator.py:199-221: every rank ends up with EVERY rank's record of a batch, so the summaries agree across ranks and
    equal the non-deferred one-process evaluation of all batches (each rank's loss list holds its own batches only)."""
    from pointcloudpdf_amd import evaluator

    world = 2
    mp.spawn(_deferred_eval_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    s = [torch.load(tmp_path / f"eval_{r}.pt", weights_only=False) for r in range(world)]
    one = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=False)
    own = [evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=False) for _ in range(world)]
    for b in range(3):
        for rank in range(world):
            logits, score, seg, loss = _batch(b, rank)
            one.update(logits, score, seg)
            own[rank].update(logits, score, seg, loss=float(loss))
    ref = one.summary()
    assert len(one.aupr) == 5 and s[0]["n_records"] == s[1]["n_records"] == 5
    for key in KEYS[:-1]:
        assert s[0][key] == s[1][key], key
        assert abs(s[0][key] - ref[key]) <= 1e-12, (key, s[0][key], ref[key])
    for rank in range(world):
        assert abs(s[rank]["loss"] - own[rank].summary()["loss"]) <= 1e-7
