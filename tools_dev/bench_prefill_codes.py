#!/usr/bin/env python3
"""A/B of the prefill forward of a packed HBFP4 (2:4, block 64) bf16 Linear with and without the weight's e4m3 image, by the method of
profiles/r02_prefill.md (hipGraph of `iters` forwards, median of 5 replays, un-profiled), interleaved in one process:
  a   PackedBFPLinear(hold_image=True), image already made (two independent graphs, a and a2: the spread of a against itself);
  b   PackedBFPLinear(hold_image=False): the codes are the weight operand (bfpq_hbfp_linear_mx4w);
  c   PackedBFP._run_linear('fake'): dequantize per call + the library GEMM, the other image-free route;
  gemm_a / gemm_b: the two GEMM launches alone, operands prepared.
Every forward quantizes its activation (native.SHARE_ACT_IMAGE off), as a first projection does.  Usage: bench_prefill_codes.py [out.json]
(default profiles/r10_prefill_codes.json)."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import quantization_sparsity_interplay_amd as bfpq
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear

dev = "cuda:0"
REPEATS = 5
LAYERS = (("gate_proj", 4096, 11008), ("down_proj", 11008, 4096), ("q_proj", 4096, 4096))
TOKENS = (128, 512, 2048, 8192)


def graph_of(fn, iters):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def main():
    native.SHARE_ACT_IMAGE = False
    L = native.load_library()
    cfg = bfpq.BFPConfig.hbfp(4, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
    cfg['rounding_mode'] = 'determ'
    rows = []
    for name, fin, fout in LAYERS:
        lin = torch.nn.Linear(fin, fout, bias=False, dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            lin.weight.mul_(0.02 * fin ** 0.5)
        held = PackedBFPLinear.from_linear(lin, cfg)
        lean = PackedBFPLinear.from_linear(lin, cfg, hold_image=False)
        del lin
        pw = held.packed
        for T in TOKENS:
            iters = 10 if T <= 2048 else 4
            x = torch.randn(T, fin, device=dev).to(torch.bfloat16)
            x8, xs = native.quantize_mx8(x, 3)
            out = torch.empty((T, fout), dtype=torch.bfloat16, device=dev)
            w8, wsc = pw._mx8_image()
            parts = L.bfpq_hbfp_linear_mx8_parts(T, fout, fin)
            slabs = torch.empty((parts, T, fout), dtype=torch.float32, device=dev) if parts > 1 else None

            def gemm_a():
                st = torch.cuda.current_stream().cuda_stream
                if parts > 1:
                    native.check(L.bfpq_hbfp_linear_mx8_splitk(x8.data_ptr(), xs.data_ptr(), w8.data_ptr(), wsc.data_ptr(), None, out.data_ptr(),
                                                              slabs.data_ptr(), parts, T, fout, fin, 2, st), "mx8 split-K")
                else:
                    native.check(L.bfpq_hbfp_linear_mx8(x8.data_ptr(), xs.data_ptr(), w8.data_ptr(), wsc.data_ptr(), None, out.data_ptr(),
                                                       T, fout, fin, 2, st), "mx8")

            def gemm_b():
                st = torch.cuda.current_stream().cuda_stream
                if parts > 1:
                    native.check(L.bfpq_hbfp_linear_mx4w_splitk(x8.data_ptr(), xs.data_ptr(), pw.codes.data_ptr(), pw.exps.data_ptr(), None,
                                                               out.data_ptr(), slabs.data_ptr(), parts, T, fout, fin, 2, 3, st), "mx4w split-K")
                else:
                    native.check(L.bfpq_hbfp_linear_mx4w(x8.data_ptr(), xs.data_ptr(), pw.codes.data_ptr(), pw.exps.data_ptr(), None, out.data_ptr(),
                                                        T, fout, fin, 2, 3, st), "mx4w")

            with torch.no_grad():
                same = torch.equal(held(x), lean(x))
                arms = {"a": lambda: held(x), "b": lambda: lean(x), "a2": lambda: held(x),
                        "c": lambda: pw._run_linear('fake', x, None, 3, 1e-8, None), "gemm_a": gemm_a, "gemm_b": gemm_b}
                graphs = {k: graph_of(f, iters) for k, f in arms.items()}
            ts = {k: [] for k in arms}
            for _ in range(REPEATS):
                for k, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3 / iters)
            med = {k: statistics.median(v) for k, v in ts.items()}
            both = ts["a"] + ts["a2"]
            spread = max(max(both) - min(both), abs(med["a"] - med["a2"]))
            rows.append(dict(layer=name, tokens=T, in_features=fin, out_features=fout, split_k_parts=parts, bit_identical=bool(same),
                             a_image_us=med["a"], b_codes_us=med["b"], c_fake_us=med["c"], d_spread_of_a_us=spread, a_repeat_us=med["a2"],
                             b_over_a=med["b"] / med["a"], b_over_c=med["b"] / med["c"], gemm_image_us=med["gemm_a"], gemm_codes_us=med["gemm_b"],
                             raw_us={k: [round(t, 2) for t in v] for k, v in ts.items()}))
            print({k: (round(v, 2) if isinstance(v, float) else v) for k, v in rows[-1].items() if k != "raw_us"}, flush=True)
            del graphs, slabs, out, x, x8, xs
            torch.cuda.empty_cache()
        del held, lean, pw
        torch.cuda.empty_cache()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_prefill_codes.json")
    json.dump(dict(method="hipGraph, median of 5 interleaved replays, un-profiled; bf16, HBFP4 2:4 weights x HBFP4 activations, block 64; "
                          "every forward quantizes its activation; d = the larger of the range of the ten timings of a and |median a - median a2|",
                   rows=rows), open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
