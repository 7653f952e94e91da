"""N>1 path on CPU: two gloo ranks on 127.0.0.1.  The collectives / sharding logic of
rlvi_amd/dist.py is exercised with the CPU oracle standing in for the HIP kernels (tests may
use the oracle as the checker), and the contract is the one of SURVEY 8(e): N ranks produce what
one device produces on the concatenated batch -- bit-identical pi on every rank."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, mode, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import rlvi_oracle as O
        from rlvi_amd import dist as rdist
        from rlvi_amd import synth
        O.set_threads(1)
        Bg, C = 1024 + 6, 10             # ragged: shards of 515 / 515
        d = synth.mstep_inputs(Bg, C, N=Bg, seed=9)
        # ---- one device on the concatenated batch
        res1, w1 = np.zeros(Bg, np.float32), d["weights"].copy()
        ref = O.mstep(d["logits"], d["labels"], d["idx"], w1, res1)
        O.update_sample_weights(res1, w1)
        # ---- this rank's shard, global 1/B scaling
        lo, hi = rdist.shard_range(Bg, rank, world)
        res = torch.zeros(Bg)
        w = torch.from_numpy(d["weights"].copy())
        out = O.mstep(d["logits"][lo:hi], d["labels"][lo:hi], d["idx"][lo:hi], w.numpy(),
                      res.numpy(), scale_div=rdist.global_batch(hi - lo))
        if mode == "general":
            rdist.exchange_residuals(res, torch.from_numpy(d["idx"][lo:hi]))
        else:
            # owner-contiguous layout: rank r owns [r*n, (r+1)*n)
            n = Bg // world
            own = np.arange(rank * n, (rank + 1) * n)
            res = torch.zeros(n * world)
            res[own[0]:own[-1] + 1] = torch.from_numpy(res1[own])
            rdist.exchange_residuals_owned(res, int(own[0]), int(own[-1]) + 1)
            assert np.array_equal(res.numpy(), res1[:n * world])
            q.put((rank, "ok"))
            return
        assert np.array_equal(res.numpy(), res1), "replicas differ from the single-device vector"
        # host helpers of round 3: rank 0's value everywhere; on a box without a GPU no device to share, on a
        # box with one both ranks drive cuda:0 and count each other
        assert rdist.rank0_value(10.0 + rank) == 10.0
        sharers = world if torch.cuda.is_available() else 1
        assert rdist.declare_device_sharing() == sharers and rdist.declare_device_sharing() == sharers
        # the per-rank losses and logit gradients SUM to the single-device ones
        t = torch.tensor([float(out["loss"]), float(out["prec1"]) * (hi - lo) / 100.0], dtype=torch.float64)
        rdist.reduce_scalars(t)
        assert abs(t[0].item() - float(ref["loss"])) <= 1e-6 * abs(float(ref["loss"]))
        assert round(t[1].item()) == round(float(ref["prec1"]) * Bg / 100.0)
        assert np.abs(out["grad"] - ref["grad"][lo:hi]).max() <= 1e-9
        # replicated E-step: identical bits on every rank, equal to the single-device pi
        wr = w.numpy().copy()
        rr = res.numpy().copy()
        O.update_sample_weights(rr, wr)
        assert np.array_equal(wr, w1)
        gathered = [torch.zeros(Bg) for _ in range(world)]
        dist.all_gather(gathered, torch.from_numpy(wr))
        assert all(torch.equal(g, gathered[0]) for g in gathered)
        # measured alternative: sharded vectors + packed scalar all-reduces per iteration
        rs = torch.from_numpy(res1.copy()) * 0
        rs = torch.from_numpy(res.numpy()[lo:hi].copy())
        ws_ = torch.from_numpy(d["weights"][lo:hi].copy())
        it = rdist.estep_allreduce_scalars(rs, ws_, Bg)
        it_ref = O.update_sample_weights(res.numpy().copy(), d["weights"].copy())
        assert it == it_ref
        np.testing.assert_allclose(ws_.numpy(), w1[lo:hi], rtol=2e-5, atol=1e-9)
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL " + repr(e) + "\n" + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["general", "owned"])
@pytest.mark.timeout(180)
def test_two_rank_sharding_matches_one_device(mode, oracle):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=150) for _ in range(world)]
    for p in procs:
        p.join(30)
    assert all(r[1] == "ok" for r in results), results


def test_shard_range_covers_everything():
    from rlvi_amd.dist import shard_range
    for n in (0, 1, 7, 8, 65536, 65537):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
