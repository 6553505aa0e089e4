"""One BFPAdam step, fp32 parameters, HBFP16 snap (weight_mant_bits 15, block 32): the loop (fused=False) against the fused list
launch (fused=True), and -- for information only, its arithmetic differs -- torch.optim.Adam(fused=True) followed by the engine's
snap per tensor.  Device-event time of one step after warm-up, the variants alternating in one process; prints one JSON line per
case and writes them all to --out.

    python bench_optim.py [--steps 20] [--warmup 5] [--cases big_determ,opt125m,...] [--out profiles/r09_bfpadam_fused.json]
"""
import argparse
import json
import statistics
import sys

import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.bfp.bfp_optim_lstm import BFPAdam

HBM_BPS = 8e12


def cfg(mode):
    return dict(mant_bits=7, epsilon=1e-8, rounding_mode=mode, device='cpu', block_size=32, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp',
                first='s', sparsity_mode='structured')


def opt125m_shapes():
    h, f, v = 768, 3072, 50272
    s = [(v, h), (2050, h)]
    for _ in range(12):
        s += [(h, h), (h,)] * 4 + [(f, h), (f,), (h, f), (h,)] + [(h,)] * 4
    return s + [(h,), (h,)]


def resnet50_shapes():
    s = [(64, 3, 7, 7), (64,), (64,)]
    cin = 64
    for w, n in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(n):
            s += [(w, cin, 1, 1), (w,), (w,), (w, w, 3, 3), (w,), (w,), (4 * w, w, 1, 1), (4 * w,), (4 * w,)]
            if b == 0:
                s += [(4 * w, cin, 1, 1), (4 * w,), (4 * w,)]
            cin = 4 * w
    return s + [(1000, 2048), (1000,)]


def llama7b_layer_shapes():
    h, f = 4096, 11008
    return [(h, h)] * 4 + [(f, h), (f, h), (h, f), (h,), (h,)]


CASES = {
    "big_determ": ([(4096, 11008)], 'determ', False),
    "big_stoc": ([(4096, 11008)], 'stoc', False),
    "big_amsgrad": ([(4096, 11008)], 'determ', True),
    "opt125m": (opt125m_shapes(), 'determ', False),
    "resnet50": (resnet50_shapes(), 'determ', False),
    "llama7b_layer": (llama7b_layer_shapes(), 'determ', False),
}


class TorchFusedThenSnap:
    """torch.optim.Adam(fused=True), then the engine's snap per parameter (for information: torch's fused Adam rounds differently)"""

    def __init__(self, params, amsgrad, bfp_args):
        self.params = params
        self.opt = torch.optim.Adam(params, lr=1e-3, amsgrad=amsgrad, fused=True)
        self.known = bfp_ops.unpack_bfp_args(dict(bfp_args))

    @torch.no_grad()
    def step(self):
        self.opt.step()
        for p in self.params:
            p.copy_(bfp_ops.float_to_bfp_blocked(p, sgd_update=True, **self.known))


def run_case(name, steps, warmup):
    shapes, mode, amsgrad = CASES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    variants = {}
    for v in ("loop", "fused", "torch_fused_then_snap"):
        params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        if v == "torch_fused_then_snap":
            opt = TorchFusedThenSnap(params, amsgrad, cfg(mode))
        else:
            opt = BFPAdam(params, lr=1e-3, amsgrad=amsgrad, bfp_args=cfg(mode), fused=(v == "fused"))
        variants[v] = opt
    times = {v: [] for v in variants}
    for it in range(warmup + steps):
        for v, opt in variants.items():                       # alternate the variants
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[v].append(a.elapsed_time(b) * 1e3)
    numel = sum(torch.Size(s).numel() for s in shapes)
    res = {"case": name, "tensors": len(shapes), "numel": numel, "rounding": mode, "amsgrad": amsgrad, "steps": steps,
           "us_median": {v: round(statistics.median(t), 1) for v, t in times.items()},
           "us_min": {v: round(min(t), 1) for v, t in times.items()}}
    if variants["fused"].fused_tensors != len(shapes):
        res["fused_tensors"] = variants["fused"].fused_tensors
    res["speedup_fused_vs_loop"] = round(res["us_median"]["loop"] / res["us_median"]["fused"], 2)
    bpe = 36 if amsgrad else 28
    res["fused_hbm_fraction"] = round(numel * bpe / (res["us_median"]["fused"] * 1e-6) / HBM_BPS, 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = []
    for name in a.cases.split(","):
        r = run_case(name, a.steps, a.warmup)
        print(json.dumps(r), flush=True)
        out.append(r)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "results": out}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
