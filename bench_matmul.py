#!/usr/bin/env python3
"""bench_matmul.py -- both attention matmuls of a GPT-2 block patched the reference's way (F_matmul_bfp, modeling_gpt2.py:207, 243, 297) on
one MI355X: Q K^T and P V, on the fake route (MxM_pre_processing + torch.matmul) and on the batched int8 matrix-unit route
(matrix_unit='int8'), hipGraph replay as bench_linear.py, the two routes alternating round by round in one process.  On a tree without
the route (F_matmul_bfp ignores the switch there) the int8 columns are null and "int8_route" says "absent".

Without --case: a driver that runs every case as its own child process under `timeout`, chained with && (a case that faults, hangs or
fails ends the run), each appending its rows to the --out file (default bench_out/bmm.json)."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# name: (batch, heads, T, head_dim)
SHAPES = {"gpt2s_b1": (1, 12, 1024, 64), "gpt2s_b8": (8, 12, 1024, 64), "d128_t2048_h32": (1, 32, 2048, 128), "gpt2s_b8_t128": (8, 12, 128, 64)}
CONFIGS = {"hbfp8_b64": dict(mant_bits=7, block_size=64), "hbfp4_b64": dict(mant_bits=3, block_size=64),
           "hbfp8_b16_w1of4": dict(mant_bits=7, block_size=16, w_sparsity=True, sparsity_mode='structured', N=1, M=4)}
DTYPES = ("bf16", "fp32")
OUT = os.path.join(ROOT, "bench_out", "bmm.json")


def replay_times(fns, iters, rounds):
    """median microseconds per call of each fn: one captured graph of `iters` calls each, `rounds` replays, the graphs alternating"""
    import torch
    graphs = []
    for fn in fns:
        fn(); fn(); torch.cuda.synchronize()                    # warm-up: code objects, the library's algorithm choice, workspaces
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay(); torch.cuda.synchronize()
        graphs.append(g)
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3 / iters)
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def run_case(shape, iters, rounds, out):
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, T, D = SHAPES[shape]
    rows = []
    for dname in DTYPES:
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        g = torch.Generator().manual_seed(1)
        q, k, v = (torch.randn(batch, heads, T, D, generator=g).to(dt).to(dev) for _ in range(3))
        causal = torch.ones(T, T, dtype=torch.bool, device=dev).tril()
        p = torch.softmax((q.float() @ k.float().transpose(-1, -2) / D ** 0.5).masked_fill(~causal, float('-inf')), dim=-1).to(dt)
        kt = k.transpose(-1, -2)
        for cname, c in CONFIGS.items():
            kw = bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs()
            kw.update({key: val for key, val in c.items() if key not in ('mant_bits', 'block_size')})
            fake = bfp_ops.F_matmul_bfp(**dict(kw))
            i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
            stats = getattr(i8, 'matmul_stats', None)
            if stats is not None and hasattr(bfp_ops, 'MATMUL_I8_MIN'):
                bfp_ops.MATMUL_I8_MIN = {key: 1 for key in bfp_ops.MATMUL_I8_MIN}     # time the route itself: every default floor off
            for mname, x, w in (("qk", q, kt), ("pv", p, v)):
                with torch.no_grad():
                    fns = [lambda: fake(x, w)] + ([lambda: i8(x, w)] if stats is not None else [])
                    med, spread = replay_times(fns, iters, rounds)
                    ran_i8 = stats is not None and stats.i8_calls > 0 and stats.fake_calls == 0
                row = dict(shape=shape, batch=batch, heads=heads, T=T, head_dim=D, dtype=dname, config=cname, matmul=mname, iters=iters, rounds=rounds,
                           fake_us=med[0], fake_min_max_us=spread[0], int8_route="ran" if ran_i8 else ("absent" if stats is None else "refused"),
                           int8_us=med[1] if ran_i8 else None, int8_min_max_us=spread[1] if ran_i8 else None,
                           speedup=med[0] / med[1] if ran_i8 else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
                if stats is not None:
                    stats.i8_calls = stats.fake_calls = 0
    os.makedirs(os.path.dirname(out), exist_ok=True)
    old = json.load(open(out)) if os.path.exists(out) else []
    json.dump(old + rows, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(SHAPES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case (driver mode)")
    ap.add_argument("--out", default=OUT, help="JSON file the rows are appended to")
    a = ap.parse_args()
    out = os.path.abspath(a.out)
    if a.case:
        return run_case(a.case, a.iters, a.rounds, out)
    if os.path.exists(out):
        os.remove(out)
    steps = [f"timeout -k 10 {a.timeout} {sys.executable} {os.path.abspath(__file__)} --case {s} --iters {a.iters} --rounds {a.rounds} --out {out}"
             for s in SHAPES]
    sys.exit(subprocess.call(" && ".join(steps), shell=True))


if __name__ == "__main__":
    main()
