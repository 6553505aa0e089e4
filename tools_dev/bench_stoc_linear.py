#!/usr/bin/env python3
"""bench_stoc_linear.py -- 'stoc' BFPLinear inference forwards on the matrix units (enable_stochastic_matrix_unit) against today's fake
route (both operands stochastically rounded to fp32 tensors, F.linear on fp32), interleaved in one process.  The new route reads a flag
back per call (exponent-overflow check), so neither side is captured into a graph: 20 eager calls between two events, median of 5
rounds, the two routes alternating round by round.
Rows: LLaMA-7B q_proj / gate_proj / down_proj in bf16 at T = 1, 16, 128, 512, 2048 for HBFP4 b64 2:4 (block-scaled route), HBFP6 b64
and b32 with 50 % prune-first unstructured weights, HBFP8 b64 with quantize-first unstructured weights (int8 route); OPT-125m fc1 / fc2 in
fp32, HBFP8 b32 and b64.  Also the operand launch alone (native.stoc_codes) on [4096, 11008] bf16.
Usage: python tools_dev/bench_stoc_linear.py [out.json]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops


def _cfg(m, block, **sp):
    c = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='stoc', mant_bits=m, block_size=block, epsilon=1e-8)
    c.update(sp)
    return c


US = dict(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5)
CONFIGS = [('hbfp4_b64_24', _cfg(3, 64, w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s'), True),
           ('hbfp6_b64_us', _cfg(5, 64, first='s', **US), 'int8'),
           ('hbfp6_b32_us', _cfg(5, 32, first='s', **US), 'int8'),
           ('hbfp8_b64_uq', _cfg(7, 64, first='q', **US), 'int8')]
LLAMA = (('q_proj', 4096, 4096), ('gate_proj', 11008, 4096), ('down_proj', 4096, 11008))
OPT = (('fc1', 3072, 768), ('fc2', 768, 3072))


def interleaved(fns, iters=20, rounds=5):
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3 / iters)
    return [statistics.median(t) for t in ts]


def row(model, layer, N, K, T, dtype, name, cfg, mu):
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(N, K, generator=g) * 0.02).to(dtype).cuda()
    x = torch.randn(T, K, generator=g).to(dtype).cuda()
    new = bfp_ops.BFPLinear(K, N, bias=False, **dict(cfg)).cuda().eval()
    old = bfp_ops.BFPLinear(K, N, bias=False, **dict(cfg)).cuda().eval()
    with torch.no_grad():
        new.weight.data = w
        old.weight.data = w
    new.enable_stochastic_matrix_unit(mu)
    with torch.no_grad():
        t_new, t_old = interleaved([lambda: new(x), lambda: old(x)])
    st = new._stoc_matrix_unit
    route = 'mx8' if st.stoc_mx_calls else ('int8' if st.stoc_i8_calls else 'fake')
    r = dict(model=model, layer=layer, N=N, K=K, T=T, dtype=str(dtype).replace('torch.', ''), config=name, matrix_unit=mu, route=route,
             new_us=round(t_new, 2), fake_us=round(t_old, 2), speedup=round(t_old / t_new, 2))
    print(json.dumps(r), flush=True)
    return r


def operand_launch():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(4096, 11008, generator=g).to(torch.bfloat16).cuda()
    out = {}
    for m, block in ((3, 64), (7, 64), (7, 32)):
        t = interleaved([lambda: native.stoc_codes(w, block, m, 1e-8, 12345)])[0]
        n = w.numel()
        nbytes = n * 2 + n + n // block
        out[f"m{m}_b{block}"] = dict(us=round(t, 2), TBps=round(nbytes / t / 1e6, 3), of_8TBps=round(nbytes / t / 8e6, 3))
    print(json.dumps(dict(operand_launch_4096x11008_bf16=out)), flush=True)
    return out


def main(out_path):
    rows = []
    for name, cfg, mu in CONFIGS:
        for layer, N, K in LLAMA:
            for T in (1, 16, 128, 512, 2048):
                rows.append(row('llama7b', layer, N, K, T, torch.bfloat16, name, cfg, mu))
    for block in (32, 64):
        for layer, N, K in OPT:
            for T in (1, 16, 128, 512, 2048):
                rows.append(row('opt125m', layer, N, K, T, torch.float32, f'hbfp8_b{block}', _cfg(7, block), 'int8'))
    res = dict(rows=rows, operand_launch=operand_launch(), device=torch.cuda.get_device_name(0))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
