#!/usr/bin/env python3
"""bench_kvcache.py -- one autoregressive decode step of one attention layer (the new token's key / value joined to S - 1 past ones,
scores, softmax, context; modeling_gpt2.py:345-348 with :207, 243) on one MI355X, three ways:
  fake   F_matmul_bfp with torch.cat pasts: MxM_pre_processing + torch.matmul, all of K and V quantized again at every step;
  int8   F_matmul_bfp(matrix_unit='int8') with torch.cat pasts: codes of all of K and V made at every step, the batched int8 GEMM;
  cache  bfp_ops.HBFPKVCache: append of one token + scores + softmax + context from the held codes,
  device the same step on HBFPKVCache(device_lengths=True): the lengths live on the device, so every replay of the captured step really
         advances (from S - 1 tokens on; the capacity is S plus the iters x (rounds + 1) + 2 tokens the run appends, scores over the
         whole capacity), context split over workgroups (--chunks-per-split, 0 = the library's choice),
  attend the device leg's cache and replay with scores, scale, softmax and context as the one call cache.attend(q, scale),
  gqa    (--case gqa_*: grouped-query attention) the attend leg on HBFPKVCache(kv_heads=...) fed the kv_heads key / value
         heads, against twin: the attend leg on the cache without kv_heads fed repeat_kv of them (both legs block 64, alternating),
  prompt (--case prompt_*: prompt attention) one step = append(prompt) + attend(q, causal=True) of a whole prompt of T tokens
         on an empty HBFPKVCache(prompt_rows=P), against loop16: what the cache can do without prompt_rows on the same tokens, ceil(T / 16)
         non-causal 16-row attend calls (a cost yardstick only), and matmul: the prompt route without it, mm(q, k^T), torch's softmax
         with a causal mask and mm(p, v) on F_matmul_bfp(matrix_unit='int8'), plus the append the cache still needs (all block 64),
  window (--case window_*: a first visible key per row) the attend leg (decode) or the prompt leg (window_prompt_*) on
         HBFPKVCache(window=W), against full: the same cache and length without a window, i.e. the path before window existed, and
         masked: what a user did before, scores() + torch's mask and softmax + context() (the prompt case: the matmul leg with a windowed
         mask); --case starts_ragged8: the attend leg on the ragged batch with a quarter of each sequence as left padding
         (HBFPKVCache(starts=True)) against full (all block 64),
  paged  (--case paged_*: a paged cache) the attend leg (paged_gpt2s_b8_s1024, paged_ragged8) or the prompt leg
         (paged_prompt_*) on HBFPKVCache(page_tokens=P, pages=N) -- P from --page-tokens, N what the batch needs, the sequences' pages
         interleaved in the pool -- against full: the same step on the cache without pages; the rows also hold both caches' nbytes(),
  fork   (--case fork_*: pages shared between sequences; both legs eager, since reorder plans on the host; HIP-event and
         wall time) fork_beam8_gpt2s_s1024: one beam-search step of 8 beams, reorder(beam_idx, tokens) + reserve + append of one token +
         attend on the paged cache (fork_beam8_h32_d128_s4096: the same at 32 heads of 128 and 4096 tokens), against select: the same step on the contiguous device-length cache with the reference's own
         reorder, index_select(0, beam_idx) of its five buffers and the lengths, copied back; fork_prompt8_s1024: 8 sequences behind a
         1024-token prompt with 64 own tokens each, the prompt appended and attended once and forked (once) against appended and
         attended by all 8 (each), with the pages in use and shared,
  c4     (--case c4_*: 4-bit codes; HBFP4 at block 64) the attend leg (c4_gpt2s_b8_s1024, c4_gpt2s_b8_s4096) or the prompt leg
         (c4_prompt_*) on HBFPKVCache(code_bits=4), contiguous (c4) and paged (c4_paged), against int8 and int8_paged: the same steps
         on the int8 cache of the same tree, the four alternating in one process; the rows also hold the caches' nbytes().  On a tree
         without code_bits the two int8 legs run alone: that is the parent's step for --parent-json,
and, for the cache alone, the append of a prefill chunk of S tokens.  Method of bench_matmul.py: hipGraph replay, the median of the
replays, the legs alternating round by round in one process.  (A captured append writes at the captured position: every replay redoes the
same step, which is what is timed.)  On a tree without the cache the cache columns are null and "cache" says "absent".

--parent-json FILE: after the run (or alone, with --merge-only, on an existing --out file) every row gains parent_fake_us / parent_int8_us
and their min / max from the row of the same shape, dtype and config in FILE, the output of this script on the parent commit.

Without --case: a driver that runs every case as its own child process under `timeout`, chained with && (a case that faults, hangs or
fails ends the run), each appending its rows to the --out file (default bench_out/kvcache.json).  --case ragged8: the device leg alone
on batch 8 with lengths spread from 128 to 4096 (no other leg holds such a batch).  --kv-heads N: the kv heads of a gqa case (default:
the case's own)."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from bench_matmul import replay_times  # noqa: E402

# name: (batch, heads, S, head_dim)
SHAPES = {"gpt2s_b1_s128": (1, 12, 128, 64), "gpt2s_b1_s1024": (1, 12, 1024, 64), "gpt2s_b1_s4096": (1, 12, 4096, 64),
          "gpt2s_b8_s128": (8, 12, 128, 64), "gpt2s_b8_s1024": (8, 12, 1024, 64), "gpt2s_b8_s4096": (8, 12, 4096, 64),
          "d128_h32_s2048": (1, 32, 2048, 128)}
CONFIGS = {"hbfp8_b64": dict(mant_bits=7, block_size=64), "hbfp4_b64": dict(mant_bits=3, block_size=64), "hbfp8_b16": dict(mant_bits=7, block_size=16)}
DTYPES = ("bf16", "fp32")
OUT = os.path.join(ROOT, "bench_out", "kvcache.json")


RAGGED = {"ragged8": (8, 12, (128, 695, 1262, 1829, 2396, 2963, 3530, 4096), 64)}
# name: (batch, heads, kv_heads, S, head_dim): the attention of LLaMA-2-70B / LLaMA-3 (modeling_llama.py:385-409), g = 4
GQA = {"gqa_h32_kv8_b1_s2048": (1, 32, 8, 2048, 128), "gqa_h32_kv8_b8_s2048": (8, 32, 8, 2048, 128)}


def device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps, attend=False, hide=None, **mode):
    """(cache, step) of the device leg: sequence b prefilled to lens[b] - 1 tokens, room for every token the run appends.  attend: the
    same cache and step with cache.attend in place of scores, torch's scale and softmax, and context.  mode: kv_heads (k and v then hold
    that many heads), window, starts.  hide (the composition only): cache -> the bool mask [B, 1, 1, capacity] of the keys torch hides"""
    import torch
    room = iters * (rounds + 1) + 2                                      # replay_times: two warm-up calls, the capture, rounds + 1 replays
    cap = max(lens) + room
    if mode.get('page_tokens'):                                          # a pool of just the pages the run needs
        P = mode['page_tokens']
        cap, mode = -(-cap // P) * P, dict(mode, pages=sum(-(-(n + room) // P) for n in lens))
    cache = i8.kv_cache(batch, heads, D, cap, dtype=dt, device=dev, device_lengths=True, chunks_per_split=cps, max_query_rows=1, **mode)
    if mode.get('page_tokens'):
        reserve_interleaved(cache, [n + room for n in lens])
    t = max(lens) - 1
    cache.append(k[:, :, :t].contiguous(), v[:, :, :t].contiguous(), torch.tensor([n - 1 for n in lens], dtype=torch.int32, device=dev))
    k_new, v_new, scale = k[:, :, -1:].contiguous(), v[:, :, -1:].contiguous(), 1.0 / D ** 0.5

    def step():
        cache.append(k_new, v_new)
        s = cache.scores(q).float() * scale
        if hide is not None:
            s = s.masked_fill(hide(cache), float('-inf'))
        p = torch.softmax(s, dim=-1).to(dt)
        return cache.context(p)

    def attend_step():
        cache.append(k_new, v_new)
        return cache.attend(q, scale)

    if attend:
        cache.prepare_attend()
    return cache, (attend_step if attend else step)


def reserve_interleaved(cache, tokens):
    """pages for tokens[b] tokens of every sequence b, a page per sequence at a time: neighbours in a sequence are not neighbours in the pool"""
    P = cache.page_tokens
    for n in range(P, max(tokens) + P, P):
        cache.reserve([min(n, t) for t in tokens])


def has_attend(bfp_ops):
    return hasattr(bfp_ops.HBFPKVCache, 'attend')


def run_ragged(name, iters, rounds, out, cps):
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, lens, D = RAGGED[name]
    rows = []
    for dname in DTYPES:
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        g = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, heads, max(lens), D, generator=g).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, 1, D, generator=g).to(dt).to(dev)
        for cname, c in CONFIGS.items():
            i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
            with torch.no_grad():
                cache, step = device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps)
                fns, acache = [step], None
                if has_attend(bfp_ops):
                    acache, astep = device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps, attend=True)
                    fns.append(astep)
                med, spread = replay_times(fns, iters, rounds)
                last = cache.lengths.tolist()
            assert cache.overflow.item() == 0 and (acache is None or (acache.overflow.item() == 0 and acache.lengths.tolist() == last))
            row = dict(shape=name, batch=batch, heads=heads, lengths=list(lens), lengths_at_end=last, head_dim=D, dtype=dname, config=cname,
                       iters=iters, rounds=rounds, chunks_per_split=cps, device_us=med[0], device_min_max_us=spread[0],
                       attend_us=med[1] if acache is not None else None, attend_min_max_us=spread[1] if acache is not None else None)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    old = json.load(open(out)) if os.path.exists(out) else []
    json.dump(old + rows, open(out, "w"), indent=1)


def run_gqa(name, iters, rounds, out, cps, kv_heads=None, only=None):
    """the legs gqa and twin of a grouped-query case, bf16 and fp32 at block 64 (only: one leg alone, bf16: what a kernel trace is taken from)"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, kvh, S, D = GQA[name]
    kvh = kv_heads or kvh
    g = heads // kvh
    c = CONFIGS["hbfp8_b64"]
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, S, D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, 1, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        with torch.no_grad():
            legs = {}
            if only != "twin":
                legs["gqa"] = device_leg(i8, batch, heads, D, [S] * batch, k, v, q, dt, dev, iters, rounds, cps, attend=True, kv_heads=kvh)
            if only != "gqa":
                kr, vr = (x.repeat_interleave(g, dim=1) for x in (k, v))                # repeat_kv (modeling_llama.py:264-273)
                legs["twin"] = device_leg(i8, batch, heads, D, [S] * batch, kr, vr, q, dt, dev, iters, rounds, cps, attend=True)
            med, spread = replay_times([step for _, step in legs.values()], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, S=S, head_dim=D, dtype=dname, config="hbfp8_b64", iters=iters, rounds=rounds,
                   chunks_per_split=cps, kv_bytes_bf16=2 * batch * kvh * S * D * 2)
        for (leg, (cache, _)), m, sp in zip(legs.items(), med, spread):
            assert cache.overflow.item() == 0
            row.update({f"{leg}_us": m, f"{leg}_min_max_us": sp, f"{leg}_cache_bytes": cache.nbytes(), f"{leg}_lengths_at_end": cache.lengths.tolist()})
        if len(legs) == 2:
            assert row["gqa_lengths_at_end"] == row["twin_lengths_at_end"] and row["gqa_cache_bytes"] * g == row["twin_cache_bytes"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump((json.load(open(out)) if os.path.exists(out) else []) + rows, open(out, "w"), indent=1)


# name: (batch, heads, kv_heads, T, head_dim, prompt_rows)
PROMPT = {"prompt_gpt2s_b8_t1024": (8, 12, 12, 1024, 64, 256), "prompt_h32_d128_b1_t2048": (1, 32, 32, 2048, 128, 512),
          "prompt_h32_kv8_b1_t2048": (1, 32, 8, 2048, 128, 512)}


def run_prompt(name, iters, rounds, out, prompt_rows=None, only=None):
    """the legs prompt, loop16 and matmul of a prompt case, bf16 and fp32 at block 64 (only: one leg alone, bf16: what a kernel trace is
    taken from).  Every step starts from an empty cache: it zeroes the lengths, appends the T tokens and attends"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, kvh, T, D, P = PROMPT[name]
    P = prompt_rows or P
    g = heads // kvh
    c = CONFIGS["hbfp8_b64"]
    scale = 1.0 / D ** 0.5
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, T, D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, T, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        if hasattr(bfp_ops, 'MATMUL_I8_MIN'):
            bfp_ops.MATMUL_I8_MIN = {key: 1 for key in bfp_ops.MATMUL_I8_MIN}          # time the route itself: every default floor off
        mk = lambda **mode: i8.kv_cache(batch, heads, D, T, dtype=dt, device=dev, device_lengths=True, kv_heads=kvh, **mode)
        caches = dict(prompt=mk(prompt_rows=P), loop16=mk(), matmul=mk())
        mask = ~torch.ones(T, T, dtype=torch.bool, device=dev).tril()
        q16 = [q[:, :, i:i + 16].contiguous() for i in range(0, T, 16)]

        def fill(cache):
            cache.lengths.zero_()
            cache.append(k, v)

        def prompt_step():
            fill(caches['prompt'])
            return caches['prompt'].attend(q, scale, causal=True)

        def loop16_step():
            fill(caches['loop16'])
            return [caches['loop16'].attend(x, scale) for x in q16]

        def matmul_step():
            fill(caches['matmul'])
            kr, vr = (x.repeat_interleave(g, dim=1) for x in (k, v)) if g > 1 else (k, v)   # repeat_kv (modeling_llama.py:264-273)
            s = i8(q, kr.transpose(-1, -2)).float() * scale
            return i8(torch.softmax(s.masked_fill(mask, float('-inf')), dim=-1).to(dt), vr)

        steps = dict(prompt=prompt_step, loop16=loop16_step, matmul=matmul_step)
        legs = [leg for leg in steps if only in (None, leg)]
        with torch.no_grad():
            for leg in legs:
                if leg != 'matmul':
                    caches[leg].prepare_attend()
            calls = i8.matmul_stats.i8_calls, i8.matmul_stats.fake_calls
            med, spread = replay_times([steps[leg] for leg in legs], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, T=T, head_dim=D, dtype=dname, config="hbfp8_b64", iters=iters, rounds=rounds,
                   prompt_rows=P, panel_ws_bytes=caches['prompt']._rows_ws.numel() if caches['prompt']._rows_ws is not None else None)
        for leg, m, sp in zip(legs, med, spread):
            assert caches[leg].overflow.item() == 0 and caches[leg].lengths.tolist() == [T] * batch
            row.update({f"{leg}_us": m, f"{leg}_min_max_us": sp})
        if 'matmul' in legs:
            assert i8.matmul_stats.i8_calls > calls[0] and i8.matmul_stats.fake_calls == calls[1]    # both products on the int8 route
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump((json.load(open(out)) if os.path.exists(out) else []) + rows, open(out, "w"), indent=1)


# name: (batch, heads, kv_heads, S, head_dim, window): sliding-window decode (sliding_window of Mistral / Mixtral / Qwen2 / Starcoder2)
WINDOW = {"window_gpt2s_b1_s4096_w1024": (1, 12, 12, 4096, 64, 1024), "window_h32_kv8_b1_s4096_w1024": (1, 32, 8, 4096, 128, 1024)}
# name: (batch, heads, kv_heads, T, head_dim, prompt_rows, window)
WINDOW_PROMPT = {"window_prompt_h32_d128_b1_t2048_w512": (1, 32, 32, 2048, 128, 512, 512)}
STARTS = {"starts_ragged8": "ragged8"}                               # a quarter of each sequence of the ragged batch is left padding


def _append_rows(out, rows):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump((json.load(open(out)) if os.path.exists(out) else []) + rows, open(out, "w"), indent=1)


def run_window(name, iters, rounds, out, cps, only=None):
    """the legs window, full and masked of a sliding-window decode case, or starts and full of the left-padded ragged batch; bf16 and
    fp32 at block 64 (only: one leg alone, bf16: what a kernel trace is taken from)"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    if name in STARTS:
        batch, heads, lens, D = RAGGED[STARTS[name]]
        kvh, W, pads, new = heads, None, [n // 4 for n in lens], "starts"
    else:
        batch, heads, kvh, S, D, W = WINDOW[name]
        lens, pads, new = [S] * batch, None, "window"
    c = CONFIGS["hbfp8_b64"]
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, max(lens), D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, 1, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        mode = dict(kv_heads=kvh)
        leg = lambda **kw: device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps, **mode, **kw)

        def hide(cache):                                             # the keys below the window of the row that was just appended
            n = torch.arange(cache.capacity, device=dev).view(1, 1, 1, -1)
            return n < (cache.lengths - W).view(-1, 1, 1, 1)

        with torch.no_grad():
            legs = {}
            if only in (None, new):
                legs[new] = leg(attend=True, window=W) if pads is None else leg(attend=True, starts=True)
                if pads is not None:
                    legs[new][0].starts.copy_(torch.tensor(pads, dtype=torch.int32, device=dev))
            if only in (None, "full"):
                legs["full"] = leg(attend=True)
            if pads is None and only in (None, "masked"):
                legs["masked"] = leg(hide=hide)
            med, spread = replay_times([step for _, step in legs.values()], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, lengths=list(lens), head_dim=D, window=W, starts=pads, dtype=dname,
                   config="hbfp8_b64", iters=iters, rounds=rounds, chunks_per_split=cps)
        ends = set()
        for (lname, (cache, _)), m, sp in zip(legs.items(), med, spread):
            assert cache.overflow.item() == 0
            ends.add(tuple(cache.lengths.tolist()))
            row.update({f"{lname}_us": m, f"{lname}_min_max_us": sp})
        assert len(ends) == 1
        row["lengths_at_end"] = list(ends.pop())
        rows.append(row)
        print(json.dumps(row), flush=True)
    _append_rows(out, rows)


def run_window_prompt(name, iters, rounds, out, only=None):
    """the legs window, full and masked of a sliding-window prompt, bf16 and fp32 at block 64: one step = append(prompt) +
    attend(q, causal=True) on an empty cache, as run_prompt; masked is its matmul leg with the windowed causal mask"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, kvh, T, D, P, W = WINDOW_PROMPT[name]
    g = heads // kvh
    c = CONFIGS["hbfp8_b64"]
    scale = 1.0 / D ** 0.5
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, T, D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, T, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        bfp_ops.MATMUL_I8_MIN = {key: 1 for key in bfp_ops.MATMUL_I8_MIN}              # time the route itself: every default floor off
        mk = lambda **mode: i8.kv_cache(batch, heads, D, T, dtype=dt, device=dev, device_lengths=True, kv_heads=kvh, **mode)
        caches = dict(window=mk(prompt_rows=P, window=W), full=mk(prompt_rows=P), masked=mk())
        ones = torch.ones(T, T, dtype=torch.bool, device=dev)
        mask = ~(ones.tril() & ones.triu(1 - W))                     # row i sees the keys i - W + 1 .. i

        def attend_step(cache):
            cache.lengths.zero_()
            cache.append(k, v)
            return cache.attend(q, scale, causal=True)

        def masked_step():
            caches['masked'].lengths.zero_()
            caches['masked'].append(k, v)
            kr, vr = (x.repeat_interleave(g, dim=1) for x in (k, v)) if g > 1 else (k, v)
            s = i8(q, kr.transpose(-1, -2)).float() * scale
            return i8(torch.softmax(s.masked_fill(mask, float('-inf')), dim=-1).to(dt), vr)

        steps = dict(window=lambda: attend_step(caches['window']), full=lambda: attend_step(caches['full']), masked=masked_step)
        legs = [leg for leg in steps if only in (None, leg)]
        with torch.no_grad():
            for leg in legs:
                if leg != 'masked':
                    caches[leg].prepare_attend()
            med, spread = replay_times([steps[leg] for leg in legs], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, T=T, head_dim=D, window=W, dtype=dname, config="hbfp8_b64", iters=iters,
                   rounds=rounds, prompt_rows=P)
        for leg, m, sp in zip(legs, med, spread):
            assert caches[leg].overflow.item() == 0 and caches[leg].lengths.tolist() == [T] * batch
            row.update({f"{leg}_us": m, f"{leg}_min_max_us": sp})
        rows.append(row)
        print(json.dumps(row), flush=True)
    _append_rows(out, rows)


# name: the decode shape, the ragged batch or the prompt case it pages
PAGED = {"paged_gpt2s_b8_s1024": "gpt2s_b8_s1024", "paged_ragged8": "ragged8", "paged_prompt_h32_d128_b1_t2048": "prompt_h32_d128_b1_t2048"}


def run_paged(name, iters, rounds, out, cps, page_tokens, only=None):
    """the legs paged and full of a paged case, bf16 and fp32 at block 64 (only: one leg alone, bf16: what a kernel trace is taken from).
    A decode case: the attend leg of device_leg.  A prompt case: one step = append(prompt) + attend(q, causal=True) on a cache whose
    lengths the step zeroes first, as run_prompt; the pages stay reserved"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    base = PAGED[name]
    prompt = base in PROMPT
    if prompt:
        batch, heads, kvh, T, D, PR = PROMPT[base]
        lens, Tq = [T] * batch, T
    elif base in RAGGED:
        batch, heads, lens, D = RAGGED[base]
        kvh, Tq = heads, 1
    else:
        batch, heads, S, D = SHAPES[base]
        lens, kvh, Tq = [S] * batch, heads, 1
    c = CONFIGS["hbfp8_b64"]
    scale = 1.0 / D ** 0.5
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, max(lens), D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, Tq, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        modes = dict(paged=dict(page_tokens=page_tokens), full={})
        legs = {}
        with torch.no_grad():
            for leg, mode in modes.items():
                if only not in (None, leg):
                    continue
                if not prompt:
                    legs[leg] = device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps, attend=True, kv_heads=kvh, **mode)
                    continue
                if mode:
                    mode = dict(mode, pages=batch * (T // page_tokens))
                cache = i8.kv_cache(batch, heads, D, T, dtype=dt, device=dev, device_lengths=True, kv_heads=kvh, prompt_rows=PR, **mode)
                if mode:
                    reserve_interleaved(cache, lens)
                cache.prepare_attend()

                def step(cache=cache):
                    cache.lengths.zero_()
                    cache.append(k, v)
                    return cache.attend(q, scale, causal=True)

                legs[leg] = (cache, step)
            med, spread = replay_times([step for _, step in legs.values()], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, lengths=list(lens), head_dim=D, dtype=dname, config="hbfp8_b64", iters=iters,
                   rounds=rounds, chunks_per_split=cps, page_tokens=page_tokens)
        ends = set()
        for (leg, (cache, _)), m, sp in zip(legs.items(), med, spread):
            assert cache.overflow.item() == 0
            ends.add(tuple(cache.lengths.tolist()))
            row.update({f"{leg}_us": m, f"{leg}_min_max_us": sp, f"{leg}_cache_bytes": cache.nbytes()})
            if cache.pages is not None:
                row.update(pages=cache.page_count, capacity=cache.capacity)
        assert len(ends) == 1
        row["lengths_at_end"] = list(ends.pop())
        rows.append(row)
        print(json.dumps(row), flush=True)
    _append_rows(out, rows)


# name: the decode shape or the prompt case it runs with 4-bit codes
C4 = {"c4_gpt2s_b8_s1024": "gpt2s_b8_s1024", "c4_gpt2s_b8_s4096": "gpt2s_b8_s4096", "c4_prompt_h32_d128_b1_t2048": "prompt_h32_d128_b1_t2048"}
C4_LEGS = {"c4": dict(code_bits=4), "int8": {}, "c4_paged": dict(code_bits=4, paged=True), "int8_paged": dict(paged=True)}


def run_c4(name, iters, rounds, out, cps, page_tokens, only=None):
    """the legs c4, int8, c4_paged and int8_paged of a c4 case, bf16 and fp32, HBFP4 at block 64 (only: one leg alone, bf16: what a kernel
    trace is taken from).  The steps are run_paged's: the attend leg of device_leg, or append(prompt) + attend(q, causal=True)"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    base = C4[name]
    prompt = base in PROMPT
    if prompt:
        batch, heads, kvh, T, D, PR = PROMPT[base]
        lens, Tq = [T] * batch, T
    else:
        batch, heads, S, D = SHAPES[base]
        lens, kvh, Tq = [S] * batch, heads, 1
    c = CONFIGS["hbfp4_b64"]
    scale = 1.0 / D ** 0.5
    has_c4 = hasattr(bfp_ops.HBFPKVCache, 'code_bits')                  # (the parent of DESIGN 5s has the int8 legs only)
    rows = []
    for dname in DTYPES if only is None else ("bf16",):
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        gen = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, kvh, max(lens), D, generator=gen).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, Tq, D, generator=gen).to(dt).to(dev)
        i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
        legs = {}
        with torch.no_grad():
            for leg, spec in C4_LEGS.items():
                if only not in (None, leg) or ('code_bits' in spec and not has_c4):
                    continue
                mode = {key: val for key, val in spec.items() if key != 'paged'}
                if spec.get('paged'):
                    mode['page_tokens'] = page_tokens
                if not prompt:
                    legs[leg] = device_leg(i8, batch, heads, D, lens, k, v, q, dt, dev, iters, rounds, cps, attend=True, kv_heads=kvh, **mode)
                    continue
                if spec.get('paged'):
                    mode['pages'] = batch * (T // page_tokens)
                cache = i8.kv_cache(batch, heads, D, T, dtype=dt, device=dev, device_lengths=True, kv_heads=kvh, prompt_rows=PR, **mode)
                if spec.get('paged'):
                    reserve_interleaved(cache, lens)
                cache.prepare_attend()

                def step(cache=cache):
                    cache.lengths.zero_()
                    cache.append(k, v)
                    return cache.attend(q, scale, causal=True)

                legs[leg] = (cache, step)
            med, spread = replay_times([step for _, step in legs.values()], iters, rounds)
        row = dict(shape=name, batch=batch, heads=heads, kv_heads=kvh, lengths=list(lens), head_dim=D, dtype=dname, config="hbfp4_b64", iters=iters,
                   rounds=rounds, chunks_per_split=cps, page_tokens=page_tokens)
        ends = set()
        for (leg, (cache, _)), m, sp in zip(legs.items(), med, spread):
            assert cache.overflow.item() == 0
            ends.add(tuple(cache.lengths.tolist()))
            row.update({f"{leg}_us": m, f"{leg}_min_max_us": sp, f"{leg}_cache_bytes": cache.nbytes()})
        assert len(ends) == 1
        row["lengths_at_end"] = list(ends.pop())
        rows.append(row)
        print(json.dumps(row), flush=True)
    _append_rows(out, rows)


# name: (batch, heads, head_dim, S): a beam search's step; (batch, heads, head_dim, prompt tokens, own tokens, prompt_rows): a shared prompt
FORK = {"fork_beam8_gpt2s_s1024": (8, 12, 64, 1024), "fork_beam8_h32_d128_s4096": (8, 32, 128, 4096),
        "fork_prompt8_s1024": (8, 12, 64, 1024, 64, 256)}
BEAM_IDX = [0, 0, 1, 3, 3, 3, 6, 7]


def eager_times(fns, iters, rounds, before=None):
    """per call of each fn, eager: (median HIP-event us, its (min, max), median wall us, its (min, max)) over `rounds` runs of `iters`
    calls, the fns alternating round by round; before(): run ahead of every timed run, outside the timing"""
    import statistics, time, torch
    for fn in fns:
        if before:
            before()
        fn(); fn(); torch.cuda.synchronize()
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            wall[i].append((time.perf_counter() - t0) * 1e6 / iters)
            ev[i].append(e0.elapsed_time(e1) * 1e3 / iters)
    return [(statistics.median(e), (min(e), max(e)), statistics.median(w), (min(w), max(w))) for e, w in zip(ev, wall)]


def run_fork_beam(name, iters, rounds, out, only=None):
    """the legs paged and select of a beam-search step, bf16 at block 64, pages of 64 tokens (only: one leg alone: a kernel trace)"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev, dt, P = "cuda:0", torch.bfloat16, 64
    batch, heads, D, S = FORK[name]
    c = CONFIGS["hbfp8_b64"]
    scale = 1.0 / D ** 0.5
    steps = 2 + iters * rounds
    cap = -(-(S + steps) // P) * P
    gen = torch.Generator().manual_seed(1)
    k, v = (torch.randn(batch, heads, S, D, generator=gen).to(dt).to(dev) for _ in range(2))
    q = torch.randn(batch, heads, 1, D, generator=gen).to(dt).to(dev)
    k_new, v_new = k[:, :, -1:].contiguous(), v[:, :, -1:].contiguous()
    i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
    mk = lambda **mode: i8.kv_cache(batch, heads, D, cap, dtype=dt, device=dev, device_lengths=True, max_query_rows=1, **mode)
    idx = torch.tensor(BEAM_IDX, device=dev)
    legs, held = {}, {}
    with torch.no_grad():
        if only in (None, "paged"):
            cache = mk(page_tokens=P, pages=batch * (cap // P))
            reserve_interleaved(cache, [S - 1] * batch)
            held["paged"] = [S - 1]                                  # the beams' common length, kept on the host as a generate() loop has it

            def paged_step(cache=cache, n=held["paged"]):
                cache.reorder(BEAM_IDX, [n[0]] * batch)
                cache.reserve(n[0] + 1)
                cache.append(k_new, v_new)
                n[0] += 1
                return cache.attend(q, scale)

            legs["paged"] = (cache, paged_step)
        if only in (None, "select"):
            cache = mk()

            def select_step(cache=cache):                            # _reorder_cache: index_select(0, beam_idx) of everything the cache holds
                for t in list(cache.buffers.values()) + [cache.lengths]:
                    t.copy_(t.index_select(0, idx))
                cache.append(k_new, v_new)
                return cache.attend(q, scale)

            legs["select"] = (cache, select_step)
        for cache, _ in legs.values():
            cache.append(k[:, :, :S - 1].contiguous(), v[:, :, :S - 1].contiguous())
            cache.prepare_attend()
        times = eager_times([step for _, step in legs.values()], iters, rounds)
    row = dict(shape=name, batch=batch, heads=heads, S=S, head_dim=D, dtype="bf16", config="hbfp8_b64", iters=iters, rounds=rounds, page_tokens=P,
               beam_idx=BEAM_IDX, capacity=cap)
    for (leg, (cache, _)), (ev, ev_mm, wall, wall_mm) in zip(legs.items(), times):
        assert cache.overflow.item() == 0 and cache.lengths.tolist() == [S - 1 + steps] * batch, (leg, cache.lengths.tolist())
        row.update({f"{leg}_us": ev, f"{leg}_min_max_us": ev_mm, f"{leg}_wall_us": wall, f"{leg}_wall_min_max_us": wall_mm,
                    f"{leg}_cache_bytes": cache.nbytes()})
        if cache.pages is not None:
            row.update(pages=cache.page_count, pages_in_use=cache.page_count - cache.pages_free, pages_shared=cache.pages_shared)
    print(json.dumps(row), flush=True)
    _append_rows(out, [row])


def run_fork_prompt(name, iters, rounds, out, only=None):
    """the legs once and each of a shared prompt, bf16 at block 64, pages of 64 tokens: every step starts from reset()"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev, dt, P = "cuda:0", torch.bfloat16, 64
    batch, heads, D, T, own, PR = FORK[name]
    c = CONFIGS["hbfp8_b64"]
    scale = 1.0 / D ** 0.5
    gen = torch.Generator().manual_seed(1)
    k, v = (torch.randn(batch, heads, T + own, D, generator=gen).to(dt).to(dev) for _ in range(2))
    k[:, :, :T], v[:, :, :T] = k[:1, :, :T], v[:1, :, :T]             # one prompt, then every sequence's own tokens
    q = torch.randn(batch, heads, T + own, D, generator=gen).to(dt).to(dev)
    kp, vp, qp = (x[:, :, :T].contiguous() for x in (k, v, q))
    ko, vo, qo = (x[:, :, T:].contiguous() for x in (k, v, q))
    first = torch.tensor([T] + [0] * (batch - 1), dtype=torch.int32, device=dev)
    i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
    per = (T + own) // P
    mk = lambda: i8.kv_cache(batch, heads, D, T + own, dtype=dt, device=dev, device_lengths=True, prompt_rows=PR, page_tokens=P, pages=batch * per)

    def once_step(cache):
        cache.reset()
        cache.reserve([T] + [0] * (batch - 1))
        cache.append(kp, vp, first)                                   # the prompt on row 0 alone
        cache.attend(qp, scale, causal=True)
        cache.fork(0, range(1, batch), T)
        cache.reserve(T + own)
        cache.append(ko, vo)
        return cache.attend(qo, scale, causal=True)

    def each_step(cache):
        cache.reset()
        cache.reserve(T + own)
        cache.append(kp, vp)
        cache.attend(qp, scale, causal=True)
        cache.append(ko, vo)
        return cache.attend(qo, scale, causal=True)

    legs = {}
    with torch.no_grad():
        for leg, fn in (("once", once_step), ("each", each_step)):
            if only in (None, leg):
                cache = mk()
                cache.prepare_attend()
                legs[leg] = (cache, lambda cache=cache, fn=fn: fn(cache))
        times = eager_times([step for _, step in legs.values()], iters, rounds)
    row = dict(shape=name, batch=batch, heads=heads, prompt=T, own=own, head_dim=D, dtype="bf16", config="hbfp8_b64", iters=iters, rounds=rounds,
               page_tokens=P, prompt_rows=PR)
    for (leg, (cache, _)), (ev, ev_mm, wall, wall_mm) in zip(legs.items(), times):
        assert cache.overflow.item() == 0 and cache.lengths.tolist() == [T + own] * batch
        used, shared = cache.page_count - cache.pages_free, cache.pages_shared
        assert (used, shared) == ((T // P + batch * (own // P), T // P) if leg == "once" else (batch * per, 0)), (leg, used, shared)
        row.update({f"{leg}_us": ev, f"{leg}_min_max_us": ev_mm, f"{leg}_wall_us": wall, f"{leg}_wall_min_max_us": wall_mm,
                    f"{leg}_pages_in_use": used, f"{leg}_pages_shared": shared})
    print(json.dumps(row), flush=True)
    _append_rows(out, [row])


def run_attend_only(shape, iters, rounds, out, cps):
    """the attend leg alone, bf16 at block 64: what a kernel trace of one step is taken from (--attend-only)"""
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev, dt = "cuda:0", torch.bfloat16
    batch, heads, S, D = SHAPES[shape]
    g = torch.Generator().manual_seed(1)
    k, v = (torch.randn(batch, heads, S, D, generator=g).to(dt).to(dev) for _ in range(2))
    q = torch.randn(batch, heads, 1, D, generator=g).to(dt).to(dev)
    c = CONFIGS["hbfp8_b64"]
    i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs())
    with torch.no_grad():
        cache, step = device_leg(i8, batch, heads, D, [S] * batch, k, v, q, dt, dev, iters, rounds, cps, attend=True)
        med, spread = replay_times([step], iters, rounds)
    assert cache.overflow.item() == 0
    row = dict(shape=shape, batch=batch, heads=heads, S=S, head_dim=D, dtype="bf16", config="hbfp8_b64", iters=iters, rounds=rounds,
               chunks_per_split=cps, attend_us=med[0], attend_min_max_us=spread[0], lengths_at_end=cache.lengths.tolist())
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump((json.load(open(out)) if os.path.exists(out) else []) + [row], open(out, "w"), indent=1)


def run_case(shape, iters, rounds, out, prefill_too=True, cps=0):
    import torch
    import quantization_sparsity_interplay_amd as bfpq
    from quantization_sparsity_interplay_amd.bfp import bfp_ops
    dev = "cuda:0"
    batch, heads, S, D = SHAPES[shape]
    rows = []
    for dname in DTYPES:
        dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[dname]
        g = torch.Generator().manual_seed(1)
        k, v = (torch.randn(batch, heads, S, D, generator=g).to(dt).to(dev) for _ in range(2))
        q = torch.randn(batch, heads, 1, D, generator=g).to(dt).to(dev)
        past_k, past_v, k_new, v_new = k[:, :, :S - 1].contiguous(), v[:, :, :S - 1].contiguous(), k[:, :, S - 1:].contiguous(), v[:, :, S - 1:].contiguous()
        scale = 1.0 / D ** 0.5
        for cname, c in CONFIGS.items():
            kw = bfpq.BFPConfig.hbfp(c['mant_bits'] + 1, c['block_size']).to_kwargs()
            fake = bfp_ops.F_matmul_bfp(**dict(kw))
            i8 = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
            stats = getattr(i8, 'matmul_stats', None)
            if stats is not None and hasattr(bfp_ops, 'MATMUL_I8_MIN'):
                bfp_ops.MATMUL_I8_MIN = {key: 1 for key in bfp_ops.MATMUL_I8_MIN}     # time the route itself: every default floor off
            cache = i8.kv_cache(batch, heads, D, S, dtype=dt, device=dev) if hasattr(i8, 'kv_cache') else None

            def cat_step(mm):
                k_all, v_all = torch.cat([past_k, k_new], dim=2), torch.cat([past_v, v_new], dim=2)
                p = torch.softmax(mm(q, k_all.transpose(-1, -2)).float() * scale, dim=-1).to(dt)
                return mm(p, v_all)

            def cache_step():
                cache.length = S - 1
                cache.append(k_new, v_new)
                p = torch.softmax(cache.scores(q).float() * scale, dim=-1).to(dt)
                return cache.context(p)

            def prefill():
                cache.length = 0
                cache.append(k, v)

            with torch.no_grad():
                fns = [lambda: cat_step(fake)] + ([lambda: cat_step(i8)] if stats is not None else [])
                dcache = acache = None
                if cache is not None:
                    cache.append(past_k, past_v)
                    fns.append(cache_step)
                    if 'device_lengths' in (bfp_ops.HBFPKVCache.__init__.__code__.co_varnames):
                        dcache, dstep = device_leg(i8, batch, heads, D, [S] * batch, k, v, q, dt, dev, iters, rounds, cps)
                        fns.append(dstep)
                        if has_attend(bfp_ops):
                            acache, astep = device_leg(i8, batch, heads, D, [S] * batch, k, v, q, dt, dev, iters, rounds, cps, attend=True)
                            fns.append(astep)
                med, spread = replay_times(fns, iters, rounds)
                att_us = att_spread = None
                if acache is not None:
                    assert acache.overflow.item() == 0 and acache.lengths.tolist() == dcache.lengths.tolist()
                    att_us, att_spread = med.pop(), spread.pop()
                if dcache is not None:
                    assert dcache.overflow.item() == 0
                    dev_us, dev_spread, dev_end = med.pop(), spread.pop(), dcache.lengths.tolist()
                ran_i8 = stats is not None and stats.i8_calls > 0 and stats.fake_calls == 0
                pre = replay_times([prefill], max(1, iters // 4), rounds) if cache is not None and prefill_too else None
            row = dict(shape=shape, batch=batch, heads=heads, S=S, head_dim=D, dtype=dname, config=cname, iters=iters, rounds=rounds,
                       fake_us=med[0], fake_min_max_us=spread[0], int8_route="ran" if ran_i8 else ("absent" if stats is None else "refused"),
                       int8_us=med[1] if ran_i8 else None, int8_min_max_us=spread[1] if ran_i8 else None,
                       cache="ran" if cache is not None else "absent", cache_us=med[-1] if cache is not None else None,
                       cache_min_max_us=spread[-1] if cache is not None else None,
                       device="ran" if dcache is not None else "absent", device_us=dev_us if dcache is not None else None,
                       device_min_max_us=dev_spread if dcache is not None else None, device_lengths_at_end=dev_end if dcache is not None else None,
                       chunks_per_split=cps if dcache is not None else None, attend_us=att_us, attend_min_max_us=att_spread,
                       prefill_append_us=pre[0][0] if pre else None, cache_bytes=cache.nbytes() if cache is not None else None,
                       kv_bytes=2 * k.numel() * k.element_size())
            rows.append(row)
            print(json.dumps(row), flush=True)
            cache = None
    os.makedirs(os.path.dirname(out), exist_ok=True)
    old = json.load(open(out)) if os.path.exists(out) else []
    json.dump(old + rows, open(out, "w"), indent=1)


def merge_parent(out, parent_json):
    """add the parent commit's two legs (the rows of parent_json, this script's output there) to the rows of `out`"""
    parent = {(r['shape'], r['dtype'], r['config']): r for r in json.load(open(parent_json))}
    rows = json.load(open(out))
    for r in rows:
        p = parent.get((r['shape'], r['dtype'], r['config']))
        if p is None:                                                     # (a case the parent cannot hold: the ragged batch)
            continue
        if r['shape'] in C4:                                              # the parent's int8 steps, contiguous and paged
            for leg in ("int8", "int8_paged"):
                r.update({f"parent_{leg}_us": p[f"{leg}_us"], f"parent_{leg}_min_max_us": p[f"{leg}_min_max_us"]})
            continue
        r.update(parent_fake_us=p['fake_us'], parent_fake_min_max_us=p['fake_min_max_us'], parent_int8_us=p['int8_us'],
                 parent_int8_min_max_us=p['int8_min_max_us'])
    json.dump(rows, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(SHAPES) + sorted(RAGGED) + sorted(GQA) + sorted(PROMPT) + sorted(WINDOW) + sorted(WINDOW_PROMPT) + sorted(STARTS) + sorted(PAGED) + sorted(FORK) + sorted(C4))
    ap.add_argument("--fork-leg", choices=("paged", "select", "once", "each"), help="with a fork_* case: that leg alone (a kernel trace)")
    ap.add_argument("--page-tokens", type=int, default=64, help="with a paged_* case: tokens per page (a multiple of 64)")
    ap.add_argument("--paged-leg", choices=("paged", "full"), help="with a paged_* case: that leg alone, bf16 (a kernel trace)")
    ap.add_argument("--c4-leg", choices=tuple(C4_LEGS), help="with a c4_* case: that leg alone, bf16 (a kernel trace)")
    ap.add_argument("--window-leg", choices=("window", "starts", "full", "masked"), help="with a window_* / starts_* case: that leg alone, bf16 (a kernel trace)")
    ap.add_argument("--prompt-rows", type=int, help="with a prompt case: the panel size (default: the case's own)")
    ap.add_argument("--prompt-leg", choices=("prompt", "loop16", "matmul"), help="with a prompt case: that leg alone, bf16 (a kernel trace)")
    ap.add_argument("--kv-heads", type=int, help="with a gqa case: its kv heads (a divisor of the case's heads; default: the case's own)")
    ap.add_argument("--leg", choices=("gqa", "twin"), help="with a gqa case: that leg alone, bf16 (a kernel trace of its step)")
    ap.add_argument("--chunks-per-split", type=int, default=0, help="64-token chunks per slice of the device leg's context (0: the library's choice)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case (driver mode)")
    ap.add_argument("--out", default=OUT, help="JSON file the rows are appended to")
    ap.add_argument("--parent-json", help="this script's output on the parent commit: its two legs are added to every row of --out")
    ap.add_argument("--skip-prefill", action="store_true", help="with --case: do not time the prefill append (a kernel trace of the decode step alone)")
    ap.add_argument("--attend-only", action="store_true", help="with --case: the attend leg alone, bf16 at block 64 (a kernel trace of one attend step)")
    ap.add_argument("--merge-only", action="store_true", help="run nothing: add --parent-json to an existing --out file")
    a = ap.parse_args()
    if a.window_leg:
        legs = ("starts", "full") if a.case in STARTS else ("window", "full", "masked") if a.case in WINDOW or a.case in WINDOW_PROMPT else ()
        if a.window_leg not in legs:
            ap.error(f"--window-leg {a.window_leg} does not go with --case {a.case}: its legs are {', '.join(legs) or 'none'}")
    if (a.kv_heads is not None or a.leg) and a.case not in GQA:
        ap.error("--kv-heads and --leg go with a gqa case (--case gqa_*)")
    if a.kv_heads is not None and (a.kv_heads < 1 or GQA[a.case][1] % a.kv_heads):
        ap.error(f"--kv-heads must be a divisor of the {GQA[a.case][1]} heads of {a.case} (got {a.kv_heads})")
    out = os.path.abspath(a.out)
    if a.merge_only:
        return merge_parent(out, a.parent_json)
    if a.case in FORK and len(FORK[a.case]) == 4:
        return run_fork_beam(a.case, a.iters, a.rounds, out, a.fork_leg)
    if a.case in FORK:
        return run_fork_prompt(a.case, min(a.iters, 4), a.rounds, out, a.fork_leg)
    if a.case in C4:
        return run_c4(a.case, min(a.iters, 4) if C4[a.case] in PROMPT else a.iters, a.rounds, out, a.chunks_per_split, a.page_tokens, a.c4_leg)
    if a.case in PAGED:
        return run_paged(a.case, min(a.iters, 4) if PAGED[a.case] in PROMPT else a.iters, a.rounds, out, a.chunks_per_split, a.page_tokens, a.paged_leg)
    if a.case in WINDOW or a.case in STARTS:
        return run_window(a.case, a.iters, a.rounds, out, a.chunks_per_split, a.window_leg)
    if a.case in WINDOW_PROMPT:
        return run_window_prompt(a.case, min(a.iters, 4), a.rounds, out, a.window_leg)
    if a.case in PROMPT:
        return run_prompt(a.case, min(a.iters, 4), a.rounds, out, a.prompt_rows, a.prompt_leg)
    if a.case in GQA:
        return run_gqa(a.case, a.iters, a.rounds, out, a.chunks_per_split, a.kv_heads, a.leg)
    if a.case in RAGGED:
        return run_ragged(a.case, a.iters, a.rounds, out, a.chunks_per_split)
    if a.case and a.attend_only:
        return run_attend_only(a.case, a.iters, a.rounds, out, a.chunks_per_split)
    if a.case:
        return run_case(a.case, a.iters, a.rounds, out, not a.skip_prefill, a.chunks_per_split)
    if os.path.exists(out):
        os.remove(out)
    steps = [f"timeout -k 10 {a.timeout} {sys.executable} {os.path.abspath(__file__)} --case {s} --iters {a.iters} --rounds {a.rounds} --chunks-per-split {a.chunks_per_split} --out {out}"
             for s in list(SHAPES) + list(RAGGED) + list(GQA) + list(PROMPT) + list(WINDOW) + list(WINDOW_PROMPT) + list(STARTS) + list(PAGED) + list(FORK) + list(C4)]
    rc = subprocess.call(" && ".join(steps), shell=True)
    if rc == 0 and a.parent_json:
        merge_parent(out, a.parent_json)
    sys.exit(rc)


if __name__ == "__main__":
    main()
