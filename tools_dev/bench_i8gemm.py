#!/usr/bin/env python3
"""bench_i8gemm.py -- HBFP5-HBFP8 Linear forward from the packed weight on the int8 matrix unit (PackedBFP.linear_i8, bfpq_i8gemm.hip)
next to the route it replaces (the weight decoded to bf16 + F.linear on the fake-quantised activation: what PackedBFP.linear does with
8-bit codes) and F.linear on bf16 operands, all in one process.  LLaMA-7B q_proj / gate_proj / down_proj at 1..2048 tokens, for
HBFP6 x HBFP6, HBFP8 x HBFP8 and HBFP4 weight x HBFP8 activation.  hipGraph of 20 calls, median of 5; every call quantizes its activation.
Usage: python tools_dev/bench_i8gemm.py [layer-substring] [out.json]
       python tools_dev/bench_i8gemm.py --block {16,32} [out.json]: HBFP8 x HBFP8 at that block on the OPT-125m and ViT-L weights
       ([N, K] = [768,768], [3072,768], [768,3072], [1024,1024], [4096,1024], [1024,4096]), fp32 and bf16 models, 1 / 16 / 197 / 8x197 / 2048
       tokens: the int8 route (PackedBFP.linear_i8) against the fake route (the activation fake-quantised at the block, the weight dequantised to
       the model dtype, F.linear) and against F.linear on the unquantised weight."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops


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


def main_blocks(block, out_path):
    dev = "cuda:0"
    native.SHARE_ACT_IMAGE = False
    shapes = (("opt125m", 768, 768), ("opt125m", 3072, 768), ("opt125m", 768, 3072),
              ("vit_l16", 1024, 1024), ("vit_l16", 4096, 1024), ("vit_l16", 1024, 4096))
    m = 7
    rows = []
    for model, N, K in shapes:
        w32 = torch.randn(N, K, device=dev) * 0.02
        for dt in (torch.float32, torch.bfloat16):
            w = w32.to(dt)
            with torch.no_grad():
                pw = bfp_ops.PackedBFP.quantize(w, m, block)
                wdq = pw.dequantize().to(dt)
                for tokens in (1, 16, 197, 8 * 197, 2048):
                    x = torch.randn(tokens, K, device=dev).to(dt)
                    new = timeit(lambda: pw.linear_i8(x, x_mant_bits=m))
                    fake = timeit(lambda: F.linear(bfp_ops._act_fake_quant(x, m, 1e-8, None, block), pw.dequantize().to(dt)))
                    plain = timeit(lambda: F.linear(x, w))
                    rows.append(dict(model=model, weight=[N, K], dtype=str(dt).replace("torch.", ""), block=block, format="HBFP8xHBFP8",
                                     tokens=tokens, i8_us=round(new, 2), fake_us=round(fake, 2), f_linear_us=round(plain, 2),
                                     i8_tops=round(2.0 * tokens * N * K / new / 1e6, 1)))
                    print(json.dumps(rows[-1]), flush=True)
                del wdq
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump(rows, open(out_path, "w"), indent=1)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--block":
        return main_blocks(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    dev = "cuda:0"
    native.SHARE_ACT_IMAGE = False
    only = sys.argv[1] if len(sys.argv) > 1 else None
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    layers = (("q_proj", 4096, 4096), ("gate_proj", 4096, 11008), ("down_proj", 11008, 4096))
    formats = (("HBFP6xHBFP6", 5, 5), ("HBFP8xHBFP8", 7, 7), ("HBFP4wxHBFP8a", 3, 7))
    rows = []
    for name, fin, fout in layers:
        if only and only not in name:
            continue
        w = (torch.randn(fout, fin, device=dev) * 0.02).to(torch.bfloat16)
        with torch.no_grad():
            for fmt, wm, xm in formats:
                pw = bfp_ops.PackedBFP.quantize(w, wm, 64)
                pw._i8_codes()                                               # (4-bit codes: the one-time expansion, outside the timing)
                for tokens in (1, 16, 64, 128, 512, 2048):
                    x = torch.randn(tokens, fin, device=dev).to(torch.bfloat16)
                    new = timeit(lambda: pw.linear_i8(x, x_mant_bits=xm))
                    fallback = timeit(lambda: F.linear(bfp_ops._quantize_nm_ref_dtype(x, 64, xm, 1e-8, bfp_ops.rounding_modes.DETERM),
                                                       pw.dequantize().to(torch.bfloat16)))
                    plain = timeit(lambda: F.linear(x, w))
                    rows.append(dict(layer=name, format=fmt, tokens=tokens, in_features=fin, out_features=fout, i8_us=round(new, 2),
                                     fallback_us=round(fallback, 2), f_linear_bf16_us=round(plain, 2),
                                     i8_tflops=round(2.0 * tokens * fin * fout / new / 1e6, 1)))
                    print(json.dumps(rows[-1]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump(rows, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
