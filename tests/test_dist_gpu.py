"""Multi-rank runs of the row-sharded path with the HIP engine (gathered result == single-GPU result,
byte for byte; the reference has no collectives on this path, so that is the whole contract).

  * test_sharded_equals_single_gpu_rccl: one rank per visible GPU over RCCL (backend "nccl"); on a one-GPU box one rank (RCCL
    does not put two ranks on one device): the same worker, every collective of the path through RCCL on a group of one.
  * test_sharded_equals_single_gpu_ranks_on_one_device: the same worker with two / three ranks sharing cuda:0 and the `gloo`
    backend moving the (host-staged) bytes -- runs on a one-GPU box, so the real kernels see n_ranks > 1: the histogram
    all-gather with its per-rank copies, the tie base read off the gathered histograms, ragged and empty slabs.
"""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cfg(**kw):
    base = dict(mant_bits=3, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64,
                num_format='bfp', weight_mant_bits=15, in_sparsity=False, w_sparsity=True,
                grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp',
                first='s', sparsity_mode='structured')
    base.update(kw)
    return base


def _worker(rank, world, port, backend, one_device, tmpdir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0 if one_device else rank)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from quantization_sparsity_interplay_amd import dist as qd
        from quantization_sparsity_interplay_amd.bfp import bfp_ops
        g = torch.Generator().manual_seed(99)
        bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)      # noqa: E731
        # rows: even split, ragged split, fewer rows than ranks (empty slabs), the LLaMA-7B q_proj shape; bf16 takes one 15-bit
        # radix pass, fp32 three (11 + 11 + 9 bits), each with its own histogram all-gather and the prefix carried in the workspace
        # (OPT and ViT, BASELINE configs 1 and 5, are fp32 models)
        for dt, shapes in ((torch.bfloat16, ((64, 256), (37, 512), (1, 128), (4096, 4096))),
                           (torch.float32, ((64, 256), (37, 512), (1, 128), (1024, 3072)))):
            for rows, cols in shapes:
                for tag in ("real", "coarse"):
                    full_c = (torch.randn(rows, cols, generator=g) * (0.02 if tag == "real" else 1.0))
                    if tag == "coarse":
                        full_c = (full_c * 2).round() / 2                               # few magnitudes: huge tie classes, cut inside a rank
                    full_c = full_c.to(dt)
                    full = full_c.to(dev)
                    local = qd.shard_rows(full, world, rank)
                    # structured: no collective in the data path
                    c = _cfg()
                    single = bfp_ops.float_to_bfp_blocked(full, **c, identifier='w')
                    got = qd.float_to_bfp_blocked_sharded(local, rows, gather=True, identifier='w', **c)
                    assert torch.equal(bits(got), bits(single)), ("2:4", dt, rows, cols, tag)
                    # unstructured: one threshold for the whole tensor, ties lowest global flat index first
                    for first in ('s', 'q'):
                        for frac in (0.5, 0.13):
                            cu = _cfg(sparsity_mode='unstructured', sparsity_frac=frac, first=first)
                            single = bfp_ops.float_to_bfp_blocked(full, **cu, identifier='w')
                            got = qd.float_to_bfp_blocked_sharded(local, rows, gather=True, identifier='w', **cu)
                            assert torch.equal(bits(got), bits(single)), ("unstructured", dt, rows, cols, tag, first, frac)
                    pruned = qd.all_gather_rows(qd.unstructured_sparsity_sharded(local, 0.5, full.numel()), rows)
                    assert torch.equal(bits(pruned), bits(bfp_ops._unstructured_sparsity(full, 'cuda', 0.5))), ("prune only", dt, rows, cols, tag)
                    if rows % world == 0 and cols % 64 == 0 and dt == torch.bfloat16:   # packed wire format
                        codes, exps = qd.float_to_bfp_packed_sharded(local, rows, 3, 64, gather=True, N=2, M=4)
                        c1, e1 = bfp_ops.float_to_bfp_packed(full, 3, 64, N=2, M=4)
                        assert torch.equal(codes, c1) and torch.equal(exps, e1), ("packed", rows, cols)
        # BASELINE config 4 at its own shape: a LLaMA-13B q_proj [5120,5120] bf16, 50 % unstructured then HBFP4, row-sharded
        # (5120 rows: even over 2 ranks, ragged over 3), every rank generating the same tensor on the device
        gd = torch.Generator(device=dev).manual_seed(13)
        full = (torch.randn(5120, 5120, generator=gd, device=dev) * 0.02).to(torch.bfloat16)
        local = qd.shard_rows(full, world, rank)
        cu = _cfg(sparsity_mode='unstructured', sparsity_frac=0.5, first='s')
        single = bfp_ops.float_to_bfp_blocked(full, **cu, identifier='w')
        got = qd.float_to_bfp_blocked_sharded(local, 5120, gather=True, identifier='w', **cu)
        assert torch.equal(bits(got), bits(single)), "cfg4 [5120,5120] sharded"
        assert int((got == 0).sum()) >= full.numel() // 2
        # the list form (every weight of a model, each rank its slabs): tensors dealt to streams so that one tensor's histogram
        # exchange runs beside the others' kernels -- same bytes as the per-tensor calls, structured and unstructured, bf16 and fp32
        for dt in (torch.bfloat16, torch.float32):
            gl = torch.Generator(device=dev).manual_seed(21)
            fulls = [(torch.randn(r, k, generator=gl, device=dev) * 0.02).to(dt) for r, k in ((512, 1024), (37, 512), (1024, 2048), (3, 256), (768, 768))]
            slabs = [qd.shard_rows(f, world, rank) for f in fulls]
            rts = [f.shape[0] for f in fulls]
            for cl in (_cfg(sparsity_mode='unstructured', sparsity_frac=0.5, first='s'), _cfg(sparsity_mode='unstructured', sparsity_frac=0.3, first='q'), _cfg()):
                want = [bfp_ops.float_to_bfp_blocked(f, **cl, identifier='w') for f in fulls]
                got = qd.float_to_bfp_blocked_many_sharded(slabs, rts, gather=True, identifier='w', lanes=3, exchange='tensor', **cl)
                for i, (a, b) in enumerate(zip(got, want)):
                    assert torch.equal(bits(a), bits(b)), ("list form", dt, cl['sparsity_mode'], cl['first'], i)
                # ONE exchange per radix pass for a group of tensors (groups of 2: three groups, the last one short)
                got = qd.float_to_bfp_blocked_many_sharded(slabs, rts, gather=True, identifier='w', exchange='list', group_size=2, **cl)
                for i, (a, b) in enumerate(zip(got, want)):
                    assert torch.equal(bits(a), bits(b)), ("list form, one exchange per group", dt, cl['sparsity_mode'], cl['first'], i)
                parts = qd.float_to_bfp_blocked_many_sharded(slabs, rts, gather=False, identifier='w', lanes=2, **cl)
                for i, (a, b) in enumerate(zip(parts, want)):
                    assert torch.equal(bits(a), bits(qd.shard_rows(b, world, rank))), ("list form, slabs", dt, cl['sparsity_mode'], i)
        # the overlapped gather (persistent side stream, staging buffer + strided copy) == the plain gather
        if 5120 % world == 0:
            c = _cfg()
            ov = qd.gather_overlapped(local, 5120, lambda p: bfp_ops.float_to_bfp_blocked(p, **c, identifier='w'), chunks=4)
            assert torch.equal(bits(ov), bits(bfp_ops.float_to_bfp_blocked(full, **c, identifier='w'))), "gather_overlapped"
        torch.cuda.synchronize()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def _run(world, backend, one_device, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), backend, one_device, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / f"ok{r}") for r in range(world))


def test_sharded_equals_single_gpu_rccl(tmp_path):
    n = torch.cuda.device_count()
    _run(max(1, min(n, 8)), "nccl", False, tmp_path)            # (several ranks on one device: the gloo test below)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_single_gpu_ranks_on_one_device(world, tmp_path):
    _run(world, "gloo", True, tmp_path)
