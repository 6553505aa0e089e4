#!/usr/bin/env python3
"""bench_sp24.py -- the 2:4-compressed Linear (patch.Sparse24BFPLinear: bfpq_sp24.hip up to bfp_ops.SP24_DECODE_TOKENS tokens, a
transient expansion to the dense route's operand above) against the dense packed Linear of the same config (patch.PackedBFPLinear), in one
process, interleaved (each point times the two modules back to back), hipGraph of 20 calls, median of 5.  HBFP4 2:4 and HBFP8 2:4 on
LLaMA-7B q_proj / gate_proj / down_proj at 1, 16, 64, 512 and 2048 tokens, bf16 activations; every call quantizes its activation.
Usage: python tools_dev/bench_sp24.py [out.json]   (default profiles/r08_sp24.json)"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import quantization_sparsity_interplay_amd as pkg
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, Sparse24BFPLinear


def graph_of(fn, iters=20):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def time_pair(fa, fb, iters=20, rounds=5):
    """medians (us per call) of a and b, their replays alternating"""
    ga, gb = graph_of(fa, iters), graph_of(fb, iters)
    ta, tb = [], []
    for _ in range(rounds):
        for g, ts in ((ga, ta), (gb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    del ga, gb
    return statistics.median(ta), statistics.median(tb)


def main(out_path):
    dev = "cuda:0"
    native.SHARE_ACT_IMAGE = False
    rows = []
    for bits in (4, 8):
        a = pkg.BFPConfig.hbfp(bits, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
        a['rounding_mode'] = 'determ'
        for layer, N, K in (("q_proj", 4096, 4096), ("gate_proj", 11008, 4096), ("down_proj", 4096, 11008)):
            lin = torch.nn.Linear(K, N, bias=False).to(dev).to(torch.bfloat16)
            with torch.no_grad():
                lin.weight.normal_(0, 0.02)
                dense, sparse = PackedBFPLinear.from_linear(lin, a), Sparse24BFPLinear.from_linear(lin, a)
                for T in (1, 16, 64, 512, 2048):
                    x = torch.randn(T, K, device=dev).to(torch.bfloat16)
                    td, ts = time_pair(lambda: dense(x), lambda: sparse(x))
                    rows.append(dict(format=f"HBFP{bits} 2:4", layer=layer, weight=[N, K], tokens=T, dense_us=round(td, 2), sp24_us=round(ts, 2),
                                     ratio=round(ts / td, 3), dense_bytes=dense.packed.nbytes(), sp24_bytes=sparse.sparse.nbytes(),
                                     sp24_route='sp24' if T <= bfp_ops.SP24_DECODE_TOKENS else 'expand'))
                    print(json.dumps(rows[-1]), flush=True)
            del dense, sparse, lin
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), method="one process, interleaved, hipGraph of 20 calls, median of 5",
                       sp24_decode_tokens=bfp_ops.SP24_DECODE_TOKENS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_sp24.json"))
