#!/usr/bin/env python3
"""bench_act_sparsity.py -- pruned activations (in_sparsity) on the packed / matrix-unit paths, one MI355X, bf16, HBFP4 (mant_bits 3),
block 64.  hipGraph of `iters` calls, median of 5 (as bench_prefill.py):
  * the activation image of [2048, 4096] and [2048, 11008]: dense (bfpq_quantize_mx8), N:M in one pass (bfpq_quantize_mx8_nm: 2:4 s / q,
    4:8 s), the two-step route it replaces (bfpq_quantize_nm int8 codes + bfpq_mx8_from_hbfp), 50 % unstructured prune-first (selection +
    bfpq_quantize_threshold_mx8);
  * PackedBFP.linear for gate_proj ([11008, 4096] weight) with 2048 and 128 tokens: dense / 2:4 activations with a 2:4 weight, 50 % unstructured activations and weight,
    next to the BFPLinear fake-quantize route (float_to_bfp_blocked on both operands + F.linear) of the same config;
  * --grid: the same N:M images with the workgroup cap (bfpq_tune(BFPQ_TUNE_MAX_GRID), the unit every cap is a multiple of) swept.
Prints one JSON object; --out PATH also writes it there."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

A = native.ActSparsity


def timeit(fn, iters=20, rounds=5):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(ts)


def cfg(**kw):
    base = dict(mant_bits=3, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=True, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def images(res, shapes):
    for T, K in shapes:
        x = (torch.randn(T, K, device="cuda") * 0.5).to(torch.bfloat16)
        key = f"{T}x{K}"
        r = res.setdefault("image_us", {}).setdefault(key, {})
        r["dense"] = timeit(lambda: native.quantize_mx8(x, 3))
        for name, act in (("2:4 s", A('structured', 2, 4, 0.0, 's')), ("2:4 q", A('structured', 2, 4, 0.0, 'q')),
                          ("4:8 s", A('structured', 4, 8, 0.0, 's'))):
            r[name + " one pass"] = timeit(lambda: native.quantize_mx8(x, 3, act=act))

            def two_step(act=act):
                _, c, e = native.quantize_nm(x, 64, 3, 1e-8, N=act.N, M=act.M, sparsify_first=act.first == 's', want_deq=False, code_bits=8, want_exp=True)
                native.mx8_from_hbfp(c, e, K, 3, 8)
            r[name + " codes + image"] = timeit(two_step)
        r["50% unstructured s"] = timeit(lambda: native.quantize_mx8(x, 3, act=A('unstructured', 0, 0, 0.5, 's')))


def grid_sweep(res, shapes):
    L = native.load_library()
    try:
        for T, K in shapes:
            x = (torch.randn(T, K, device="cuda") * 0.5).to(torch.bfloat16)
            for name, act in (("2:4 s", A('structured', 2, 4, 0.0, 's')), ("2:4 q", A('structured', 2, 4, 0.0, 'q')),
                              ("4:8 s", A('structured', 4, 8, 0.0, 's'))):
                row = {}
                for unit in (512, 768, 1024, 1280, 1536):      # caps: 43/16 x unit (N:2 / N:4), 2 x unit (N:8)
                    L.bfpq_tune(0, unit)
                    row[str(unit)] = timeit(lambda: native.quantize_mx8(x, 3, act=act))
                res.setdefault("grid_unit_sweep_us", {}).setdefault(f"{T}x{K}", {})[name] = row
    finally:
        L.bfpq_tune(0, 1024)


def linears(res):
    N, K = 11008, 4096
    w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
    pw = bfp_ops.PackedBFP.quantize(w, 3, 64, N=2, M=4)
    pwu = bfp_ops.PackedBFP.quantize_unstructured(w, 3, 64, 0.5)     # (the reference's config shares sparsity_mode: unstructured weights too)
    for T in (2048, 128):
        x = (torch.randn(T, K, device="cuda") * 0.5).to(torch.bfloat16)
        r = res.setdefault("gate_proj_us", {}).setdefault(str(T), {})
        # weights and activations of one row share the config: dense and 2:4 activations with 2:4 weights, 50 % unstructured for both
        for name, act, c, p in (("dense act, 2:4 w", None, cfg(), pw),
                                ("2:4 act, 2:4 w", A('structured', 2, 4, 0.0, 's'), cfg(in_sparsity=True), pw),
                                ("50% unstructured act and w", A('unstructured', 0, 0, 0.5, 's'), cfg(in_sparsity=True, sparsity_mode='unstructured'), pwu)):
            native.SHARE_ACT_IMAGE = False                     # every call quantizes its activation
            try:
                r[name + " packed"] = timeit(lambda: p.linear(x, x_mant_bits=3, x_sparsity=act))
            finally:
                native.SHARE_ACT_IMAGE = True

            def fake(c=c):
                xq = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in')
                wq = bfp_ops.float_to_bfp_blocked(w, **c, identifier='w')
                torch.nn.functional.linear(xq, wq)
            r[name + " BFPLinear fake-quantize"] = timeit(fake, iters=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "mant_bits": 3}
    shapes = ((2048, 4096), (2048, 11008))
    images(res, shapes)
    linears(res)
    if args.grid:
        grid_sweep(res, shapes)
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
