"""CPU, world_size 2, gloo: the exchange's 2D block follows the rig (num_output x head.num_cams rows, as bench.py sizes it), and
ranks that serve different rigs are refused where the exchange is built -- not at the first all-gather, which would mix or hang."""
import os

import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dist_gloo import _free_port


def _worker(rank, world, port, q, cams):
    import torch
    from simpb_amd.dist import DetectionGather
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rows = 20 * cams[rank]
    try:
        gather = DetectionGather(2, 20, torch.device("cpu"), rows2d=rows, compact2d=True)
        q.put((rank, "built", tuple(gather.recv2d.shape)))
    except ValueError as e:
        q.put((rank, "refused", str(e)))
    dist.barrier()
    dist.destroy_process_group()


def _run(cams):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, cams)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=120) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def test_ranks_with_the_same_rig_build_an_exchange_of_its_rows():
    got = _run((8, 8))
    assert [g[1] for g in got] == ["built", "built"] and all(g[2] == (2, 2, 160, 8) for g in got), got


def test_ranks_with_different_rigs_are_refused_at_construction():
    got = _run((6, 8))
    assert [g[1] for g in got] == ["refused", "refused"], got
    assert all("rows2d" in g[2] and "120" in g[2] and "160" in g[2] for g in got), got
