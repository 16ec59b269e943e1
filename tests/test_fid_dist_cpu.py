"""CPU, gloo, world_size 2: evaluate_sharded(fid_features=...) -- per-rank Frechet statistics, ONE all-gather of the states after the
loop in which every rank takes part, rank 0's "fid" against the world-1 value."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fid_ref as R  # noqa: E402

N_IMAGES, BS = 43, 4          # world 2: 44 sampler items (image 0 wrapped in), 5 steps of 4 per rank -> 40 rows per feature set


def _evaluate(rank, world, n, bs, n_codes):
    from pit_hip.eval_dist import evaluate_sharded

    ext = R.StubExtractor()
    out = evaluate_sharded(R.StubModel(), R.stub_images, n, bs, rank, world, torch.device("cpu"), 4, n_codes=n_codes, fid_features=ext)
    return out, ext


def _worker(rank, world, port, n, bs, n_codes, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "vq-vae-from-gaussian-vae_amd"))
    from pit_hip.eval_dist import init_from_env

    env = init_from_env("gloo")
    out, ext = _evaluate(env["rank"], env["world"], n, bs, n_codes)
    q.put((rank, None if out is None else {k: out[k] for k in ("fid", "fid_count")}, len(ext.blocks)))
    dist.barrier()
    dist.destroy_process_group()


def _run_world(world, n, bs, n_codes=None):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, bs, n_codes, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict((r, (out, blocks)) for r, out, blocks in (q.get(timeout=240) for _ in range(world)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0                      # every rank returned: the post-loop gather met no early return
    return got


def _world1_over(ids):
    """The world-1 value over exactly the dataset items the two ranks evaluate, in any order: the features are per image."""
    from pit_hip.evaluations.fid.fid_score import FrechetStats, calculate_frechet_distance

    ext, model = R.StubExtractor(), R.StubModel()
    x = R.stub_images(ids)
    fx, fy = ext(x), ext(model.decode(x))
    sx, sy = FrechetStats(fx.shape[1], "cpu").update(fx), FrechetStats(fx.shape[1], "cpu").update(fy)
    (n, mx, cx), (_, my, cy) = sx.moments(), sy.moments()
    return calculate_frechet_distance(my, cy, mx, cx), n, R.fid_scale(my.numpy(), cy.numpy(), mx.numpy(), cx.numpy())


def test_two_rank_fid_equals_the_world_one_value():
    from pit_hip.eval_dist import shard_batches

    got = _run_world(2, N_IMAGES, BS)
    ids = [i for r in range(2) for b in shard_batches(N_IMAGES, 2, r, BS) for i in b]
    assert len(ids) == 40 and ids.count(0) == 1 and 42 not in ids         # (43, 4): 5 full steps per rank, the ragged tail dropped
    want, n, scale = _world1_over(ids)
    out0, blocks0 = got[0]
    assert got[1][0] is None and blocks0 == got[1][1] == 10
    assert out0["fid_count"] == n == 40
    assert isinstance(out0["fid"], float) and want > 1e-4 and abs(out0["fid"] - want) <= R.FID_RTOL * scale


def test_wrapped_items_count_and_bit_packed_record_returns_on_every_rank():
    """(9, 1) at world 2: the sampler pads 9 -> 10 by wrapping image 0 in, and it is inside the kept batches, so it counts twice
    (eval.py:205).  With n_codes the ranks other than 0 go on past the first early return to the violations check: still no
    deadlock."""
    got = _run_world(2, 9, 1, n_codes=65536)
    want, n, scale = _world1_over([0, 2, 4, 6, 8, 1, 3, 5, 7, 0])
    assert got[1][0] is None and got[0][0]["fid_count"] == n == 10
    assert abs(got[0][0]["fid"] - want) <= R.FID_RTOL * scale
