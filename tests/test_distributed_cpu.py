"""Multi-process (gloo, world_size 2 and 3) test of the output-column sharding + all-gather.  No GPU here, so the
per-rank compute is the CPU oracle injected as `forward_impl` (test infrastructure standing in for the HIP kernel);
what is under test is the host logic: column ranges, slicing of packed zero words, the exchange and the re-assembly."""
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


def _cpu_barrier():
    """gloo's own barrier.  dist.barrier() first asks torch which accelerator the machine has, and on a GPU machine that question
    initialises the GPU runtime in every rank: eight CPU-only ranks would hold the GPU open for nothing."""
    dist.monitored_barrier()


def _oracle_impl(x2, qweight, scales, zeros, g_idx, w_bit, asym, group_size, bias):
    from oracle import oracle as orc
    dt = orc.dt_code(x2.dtype)
    W = orc.mpq_dequant(qweight.numpy(), orc.torch_to_np(scales), orc.torch_to_np(zeros) if not asym else zeros.numpy(),
                        None if g_idx is None else g_idx.numpy(), w_bit, group_size, int(asym), dt)
    y = orc.gemm(orc.torch_to_np(x2), W, dt, None if bias is None else orc.torch_to_np(bias))
    return orc.np_to_torch(y, x2.dtype)


def _make(asym, w_bit=4, K=256, N=768, gs=64):
    g = torch.Generator().manual_seed(7)
    qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, (K * w_bit // 32, N), generator=g, dtype=torch.int64).to(torch.int32)
    scales = (torch.rand((K // gs, N), generator=g) * 0.01 + 0.005).half()
    if asym:
        zeros = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // gs, N * w_bit // 32), generator=g, dtype=torch.int64).to(torch.int32)
    else:
        zeros = (scales.float() * torch.rand((K // gs, N), generator=g) * 15).half()
    bias = torch.randn(N, generator=g).half()
    x = torch.randn((2, 3, K), generator=g).half()
    g_idx = torch.arange(K, dtype=torch.int32) // gs
    return qweight, scales, zeros, g_idx, bias, x, w_bit, gs


def _worker(rank, world, port, asym, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bitorch_engine.distributed import ColumnShardedMPQLinear, column_range
    qweight, scales, zeros, g_idx, bias, x, w_bit, gs = _make(asym)
    layer = ColumnShardedMPQLinear(qweight, scales, zeros, g_idx, bias, w_bit, gs, asym, rank, world, forward_impl=_oracle_impl)
    lo, hi = column_range(qweight.shape[1], rank, world)
    assert layer.qweight.shape[1] == hi - lo
    y = layer(x)
    full = _oracle_impl(x.reshape(-1, x.shape[-1]), qweight, scales, zeros, g_idx, w_bit, asym, gs, bias).view(2, 3, -1)
    ok = torch.equal(y, full)
    # the M-tiled (compute / exchange overlapped) schedule: 7 rows in tiles of 3 -> tiles of 3, 3, 1 rows
    g = torch.Generator().manual_seed(11)
    x7 = torch.randn((7, x.shape[-1]), generator=g).half()
    full7 = _oracle_impl(x7, qweight, scales, zeros, g_idx, w_bit, asym, gs, bias)
    y7 = layer.forward_overlapped(x7, m_tile=3)
    ok_tiled = torch.equal(y7, full7)
    equal_shards = len({hi - lo for lo, hi in layer.ranges}) == 1
    ok_rm = True
    for mt in (3, 16):  # tiled schedule, and the single-tile fallback: interleave=False ALWAYS means rank-major [W, M, N/W]
        if equal_shards:
            rm = layer.forward_overlapped(x7, m_tile=mt, interleave=False)
            ok_rm = ok_rm and rm.dim() == 3 and rm.shape[0] == world
            for r in range(world):  # block r is the column block of rank r
                rlo, rhi = column_range(qweight.shape[1], r, world)
                ok_rm = ok_rm and torch.equal(rm[r], full7[:, rlo:rhi])
        else:  # unequal shard widths cannot be laid out rank-major: an error, not a silently different layout
            try:
                layer.forward_overlapped(x7, m_tile=mt, interleave=False)
                ok_rm = False
            except RuntimeError:
                pass
    # direct exchange (grouped send / recv into the final place): interleaved [M, N] for any shard widths, rank-major with zero copies
    ok_direct = True
    for mt in (3, 16):
        yd = layer.forward_direct(x7, m_tile=mt)
        ok_direct = ok_direct and torch.equal(yd, full7)
        if equal_shards:
            rm = layer.forward_direct(x7, m_tile=mt, interleave=False)
            ok_direct = ok_direct and rm.shape == (world, 7, (qweight.shape[1]) // world)
            for r in range(world):
                rlo, rhi = column_range(qweight.shape[1], r, world)
                ok_direct = ok_direct and torch.equal(rm[r], full7[:, rlo:rhi])
        else:
            try:
                layer.forward_direct(x7, m_tile=mt, interleave=False)
                ok_direct = False
            except RuntimeError:
                pass
    ok_direct = ok_direct and torch.equal(layer.forward_direct(x), full)  # leading dims, one tile
    torch.save({"ok": ok and ok_tiled and ok_rm and ok_direct, "shape": tuple(y.shape)}, os.path.join(out_dir, f"r{rank}.pt"))
    _cpu_barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,asym", [(2, False), (2, True), (3, False)])
def test_column_sharded_layer_gloo(tmp_path, world, asym):
    port = _free_port()
    mp.spawn(_worker, args=(world, port, asym, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = torch.load(os.path.join(tmp_path, f"r{r}.pt"))
        assert res["ok"], f"rank {r}: gathered output differs from the unsharded result"
        assert res["shape"] == (2, 3, 768)


def _worker_c5(rank, world, port, out_dir):
    """configs[4]'s exact partition: N = 28672 over 8 ranks = 8 x 3584 columns (28 blocks of 128 each), K cut down so that the CPU
    oracle finishes in seconds (the partition is along N; K only scales the per-rank compute), M = 37 rows in tiles of 16 (16, 16, 5)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bitorch_engine.distributed import ColumnShardedMPQLinear, column_range
    qweight, scales, zeros, g_idx, bias, _, w_bit, gs = _make(False, K=128, N=28672, gs=64)
    layer = ColumnShardedMPQLinear(qweight, scales, zeros, g_idx, bias, w_bit, gs, False, rank, world, forward_impl=_oracle_impl)
    ok = layer.ranges == [(r * 3584, (r + 1) * 3584) for r in range(8)] and tuple(layer.qweight.shape) == (16, 3584)
    g = torch.Generator().manual_seed(13)
    x = torch.randn((37, 128), generator=g).half()
    full = _oracle_impl(x, qweight, scales, zeros, g_idx, w_bit, False, gs, bias)
    res = {"partition": ok}
    res["allgather"] = torch.equal(layer(x), full)
    res["overlapped"] = torch.equal(layer.forward_overlapped(x, m_tile=16), full)
    res["direct"] = torch.equal(layer.forward_direct(x, m_tile=16), full)
    for name, fn in (("overlapped_rank_major", layer.forward_overlapped), ("direct_rank_major", layer.forward_direct)):
        rm = fn(x, m_tile=16, interleave=False)
        res[name] = tuple(rm.shape) == (8, 37, 3584) and all(torch.equal(rm[r], full[:, r * 3584:(r + 1) * 3584]) for r in range(8))
    # every rank took part in every collective: the gathered result holds all eight column blocks, and the world really is 8
    res["world"] = dist.get_world_size() == 8
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    _cpu_barrier()
    dist.destroy_process_group()


def test_c5_partition_world_size_8_all_three_schedules_gloo(tmp_path):
    """N = 28672 -> 8 x 3584 across EIGHT processes, the plain all-gather, the M-tiled overlapped schedule and the
    direct exchange, interleaved and rank-major, with a ragged last row tile -- every rank's assembled y equals the unsharded layer."""
    port = _free_port()
    mp.spawn(_worker_c5, args=(8, port, str(tmp_path)), nprocs=8, join=True)
    for r in range(8):
        res = torch.load(os.path.join(tmp_path, f"r{r}.pt"))
        assert all(res.values()), f"rank {r}: {res}"


def test_column_ranges_cover_and_align():
    sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
    from bitorch_engine.distributed import column_range
    for N, W in ((28672, 8), (11008, 8), (4096, 3), (768, 5)):
        prev = 0
        for r in range(W):
            lo, hi = column_range(N, r, W)
            assert lo == prev and lo % 128 == 0 and hi % 128 == 0 and hi >= lo
            prev = hi
        assert prev == N
    assert column_range(28672, 3, 8) == (3 * 3584, 4 * 3584)
    with pytest.raises(ValueError):
        column_range(1000, 0, 2)
