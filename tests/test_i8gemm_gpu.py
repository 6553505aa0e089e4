"""HBFP5-HBFP8 on the int8 matrix unit (bfpq_i8gemm.hip), bit for bit on exact operands and within the fp32 summation bound on random
data (run with `-m gpu` on an MI355X).  The drivers here (certified, expected, run_c, every_plan, ...) take the block; the runs at blocks
16 and 32 are in tests/test_i8gemm_blocks_gpu.py.

Exact operands come from tests/gemm_cases.py: every case asserts the certificate first (every fp32 partial sum exact in any order), so
the fp64 product rounded once to the output dtype IS the expected output, whatever tile variant, K split or kernel the plan picks.
At 7-bit mantissas the certificate limits K and the exponent spread: each case takes the widest spread that still certifies.
"""
import copy
import ctypes

import pytest
import torch

import gemm_cases as G
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, pack_linear_layers, patch_linear_layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = (torch.float32, torch.bfloat16, torch.float16)
TUNE_I8_VARIANT, TUNE_I8_PARTS = 4, 5
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
WIDTHS = (1, 3, 4, 5, 7)
TOKENS = (1, 2, 15, 16, 17, 31, 33, 64, 65, 127, 257, 2048)


def L():
    return native.load_library()


def ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def certified(T, N, K, xm, wm, seed, nm=(0, 0), with_bias=False, block=64):
    """exact operands with the widest exponent spreads (3 down to 1) that keep the certificate; returns the codes / exponents and the bias"""
    for sx, sw in ((3, 3), (3, 2), (2, 2), (2, 1), (1, 1)):
        xc, xe = G.hbfp_operand(T, K, xm, -3, sx, seed, device=DEV, block=block)
        wc, we = G.hbfp_operand(N, K, wm, -2, sw, seed + 1, nm=nm, pattern=(5, 7, 2), device=DEV, block=block)
        bq = None
        if with_bias:
            g = torch.Generator(device=DEV).manual_seed(seed + 2)
            bq = torch.randint(-60, 61, (N,), generator=g, device=DEV).double() * 4
        q, worst = G.exact_certificate(xc, xe, xm, wc, we, wm, bq, block=block)
        if worst < 2.0 ** 24:
            bias = None if bq is None else bq * q
            return xc, xe, wc, we, bias
    raise AssertionError(f"no certified spread for T={T} N={N} K={K} xm={xm} wm={wm} block {block}")


def expected(xc, xe, xm, wc, we, wm, bias, dt, block=64):
    want = G.values(xc, xe, xm, block=block) @ G.values(wc, we, wm, block=block).t()
    if bias is not None:
        want = want + bias.view(1, -1)
    return want.to(dt)


def family(block):
    """the C entries of a block: (name suffix, block argument) -- block 64 '' and none, blocks 16 / 32 the `b` entries and the block"""
    return ('', ()) if block == 64 else ('b', (block,))


def run_c(route, xc8, xe8, wc8, we8, bias, T, N, K, dt, wm, xm, parts=1, block=64):
    """one C entry point of the block's family directly: 'decode8', 'tile' (bfpq_hbfp_linear_i8[b]) or 'split'
    (bfpq_hbfp_linear_i8[b]_splitk with `parts`)"""
    sfx, blk = family(block)
    ops, tail = (ptr(xc8), ptr(xe8), ptr(wc8), ptr(we8), ptr(bias)), (*blk, DT_CODE[dt], wm, xm, stream())
    out = torch.empty((T, N), dtype=dt, device=DEV)
    if route == 'decode8':
        slabs = torch.empty(int(getattr(L(), f"bfpq_hbfp_linear_decode8{sfx}_ws")(T, N, K, *blk)), dtype=torch.float32, device=DEV)
        rc = getattr(L(), f"bfpq_hbfp_linear_decode8{sfx}")(*ops, ptr(out), ptr(slabs), T, N, K, *tail)
    elif route == 'tile':
        rc = getattr(L(), f"bfpq_hbfp_linear_i8{sfx}")(*ops, ptr(out), T, N, K, *tail)
    else:
        slabs = torch.empty((parts, T, N), dtype=torch.float32, device=DEV)
        rc = getattr(L(), f"bfpq_hbfp_linear_i8{sfx}_splitk")(*ops, ptr(out), ptr(slabs), parts, T, N, K, *tail)
    assert rc == 0, (route, rc)
    return out


def assert_bits(got, want, what):
    g, w = got.cpu(), want.cpu()
    iv = torch.int16 if g.dtype != torch.float32 else torch.int32
    same = (g.view(iv) == w.view(iv)) | (torch.isnan(g) & torch.isnan(w))
    if not bool(same.all()):
        i = int((~same).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())}/{same.numel()} outputs differ; first at flat {i}: got {float(g.flatten()[i])!r} "
                             f"want {float(w.flatten()[i])!r}")


def i8(t):
    return t.to(torch.int8).contiguous()


def every_plan(xc, xe, xm, wc, we, wm, bias, T, N, K, dt, what, block=64, variants=range(3)):
    """the public wrapper, the decode kernel, and (K % 256 == 0) every tile variant unsplit and split in 2, 3 and the maximum parts"""
    want = expected(xc, xe, xm, wc, we, wm, bias, dt, block=block)
    b = None if bias is None else bias.to(dt)
    xq = (i8(xc), i8(xe))
    got = native.hbfp_linear_i8(torch.empty((T, K), dtype=dt, device=DEV), i8(wc), i8(we), wm, xm, bias=b, out_dtype=dt, xq=xq,
                                block_size=block)
    assert_bits(got, want, f"{what} default plan")
    assert_bits(run_c('decode8', *xq, i8(wc), i8(we), b, T, N, K, dt, wm, xm, block=block), want, f"{what} decode8")
    sfx, blk = family(block)
    if not getattr(L(), f"bfpq_hbfp_linear_i8{sfx}_ok")(T, N, K, *blk):
        return
    trips = K // 256
    try:
        for v in variants:
            assert L().bfpq_tune(TUNE_I8_VARIANT, v) == 0
            assert_bits(run_c('tile', *xq, i8(wc), i8(we), b, T, N, K, dt, wm, xm, block=block), want, f"{what} variant {v}")
            for p in sorted({2, 3, trips} - {1}):
                assert_bits(run_c('split', *xq, i8(wc), i8(we), b, T, N, K, dt, wm, xm, parts=p, block=block), want,
                            f"{what} variant {v} parts {p}")
    finally:
        L().bfpq_tune(TUNE_I8_VARIANT, -1)


@pytest.mark.parametrize("xm", WIDTHS)
@pytest.mark.parametrize("wm", WIDTHS)
def test_exact_every_width(xm, wm):
    for T in (1, 33, 257):
        N, K = 80, 512
        xc, xe, wc, we, bias = certified(T, N, K, xm, wm, seed=100 * xm + 10 * wm + T, with_bias=(T % 2 == 1))
        every_plan(xc, xe, xm, wc, we, wm, bias, T, N, K, torch.bfloat16, f"xm {xm} wm {wm} T {T}")


@pytest.mark.parametrize("dt", DTS)
def test_exact_every_token_count(dt):
    for T in TOKENS:
        for with_bias in (False, True):
            N, K = 144, 768
            xc, xe, wc, we, bias = certified(T, N, K, 5, 7, seed=T * 3 + int(with_bias), with_bias=with_bias)
            every_plan(xc, xe, 5, wc, we, 7, bias, T, N, K, dt, f"{dt} T {T} bias {with_bias}")


def test_exact_k_not_multiple_of_256_and_nm_weights():
    for (T, N, K, nm) in ((20, 48, 320, (0, 0)), (300, 32, 192, (0, 0)), (65, 128, 512, (2, 4)), (17, 64, 1024, (4, 8))):
        xc, xe, wc, we, bias = certified(T, N, K, 7, 6, seed=T + N, nm=nm, with_bias=True)
        every_plan(xc, xe, 7, wc, we, 6, bias, T, N, K, torch.float32, f"T {T} N {N} K {K} nm {nm}")


def test_parts_switch_and_plan_choice():
    T, N, K = 128, 64, 2048
    xc, xe, wc, we, bias = certified(T, N, K, 4, 4, seed=9)
    want = expected(xc, xe, 4, wc, we, 4, None, torch.bfloat16)
    x = torch.empty((T, K), dtype=torch.bfloat16, device=DEV)
    try:
        for p in (0, 1, 2, 5, 8, 64):
            assert L().bfpq_tune(TUNE_I8_PARTS, p) == 0
            got = native.hbfp_linear_i8(x, i8(wc), i8(we), 4, 4, xq=(i8(xc), i8(xe)))
            assert_bits(got, want, f"parts switch {p}")
    finally:
        L().bfpq_tune(TUNE_I8_PARTS, 0)


@pytest.mark.parametrize("T", (1, 16, 17, 64, 300))
def test_exact_4bit_weights_through_the_expansion(T):
    N, K = 96, 512
    for wm in (1, 3):
        xc, xe, wc, we, bias = certified(T, N, K, 7, wm, seed=T + wm, with_bias=True)
        c4 = G.pack4(wc)
        c8 = native.codes4_to_i8(c4, N * K).view(N, K)
        assert torch.equal(c8, i8(wc))
        pk = bfp_ops.PackedBFP(c4, i8(we), (N, K), torch.bfloat16, wm, 64, 4)
        assert torch.equal(pk._i8_codes(), i8(wc))
        assert pk._i8_codes() is pk._i8_codes()                               # expanded once
        want = expected(xc, xe, 7, wc, we, wm, bias, torch.float32)
        got = native.hbfp_linear_i8(torch.empty((T, K), dtype=torch.float32, device=DEV), pk._i8_codes(), pk.exps, wm, 7,
                                    bias=bias.float(), xq=(i8(xc), i8(xe)))
        assert_bits(got, want, f"4-bit weights wm {wm} T {T}")


def test_nan_blocks_every_route():
    N, K = 64, 512
    for T in (3, 40):
        xc, xe, wc, we, _ = certified(T, N, K, 7, 7, seed=77)
        xe, we = xe.clone(), we.clone()
        xe[1, 2] = -128                                                        # token 1: every output NaN
        we[5, 7] = -128                                                        # feature 5: every output NaN
        want = expected(xc, xe.clamp_min(-127), 7, wc, we.clamp_min(-127), 7, None, torch.float32)
        want[1, :] = float("nan")
        want[:, 5] = float("nan")
        xq = (i8(xc), i8(xe))
        assert_bits(run_c('decode8', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7), want, f"decode8 NaN T {T}")
        try:
            for v in range(3):
                L().bfpq_tune(TUNE_I8_VARIANT, v)
                assert_bits(run_c('tile', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7), want, f"tile {v} NaN T {T}")
                assert_bits(run_c('split', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7, parts=2), want, f"split {v} NaN T {T}")
        finally:
            L().bfpq_tune(TUNE_I8_VARIANT, -1)


@pytest.mark.parametrize("shape", ((4096, 4096), (11008, 4096), (4096, 11008)))
@pytest.mark.parametrize("m", (5, 7))
def test_random_llama_shapes(shape, m):
    N, K = shape
    g = torch.Generator(device=DEV).manual_seed(N + K + m)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    wc, we = bfp_ops.float_to_bfp_packed(w, m, 64, code_bits=8)
    wv = G.values(wc.view(N, K).int(), we.int(), m)
    for T in (1, 16, 64, 2048):
        x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
        xc, xe = native.act_codes(x, m, 1e-8, None)
        xv = G.values(xc.int(), xe.int(), m)
        cfg = bfp_ops.unpack_bfp_args(dict(mant_bits=m, block_size=64, num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ',
                                           device=DEV))
        assert torch.equal(xv.to(torch.bfloat16), bfp_ops.float_to_bfp_blocked(x, **cfg, identifier='in'))
        want = xv @ wv.t()
        absprod = xv.abs() @ wv.abs().t()
        got = native.hbfp_linear_i8(x, wc.view(N, K), we, m, m, out_dtype=torch.float32)
        G.elementwise_bound(got, want, absprod, K // 64 + 8, torch.float32)
        again = native.hbfp_linear_i8(x, wc.view(N, K), we, m, m, out_dtype=torch.float32)
        assert torch.equal(got, again)


BASE = dict(num_format='bfp', sparsity_num_format='bfp', block_size=64, rounding_mode='determ', epsilon=1e-8)
WEIGHT_FORMS = {
    'dense': dict(),
    '2:4': dict(w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s'),
    '4:8 q-first': dict(w_sparsity=True, sparsity_mode='structured', N=4, M=8, first='q'),
    'unstructured 50%': dict(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='s'),
}
ACT_FORMS = {
    'dense': dict(),
    '2:4': dict(in_sparsity=True, N=2, M=4),
    'unstructured 50%': dict(in_sparsity=True, sparsity_frac=0.5),
}


def _cfg(m, wform, aform):
    a = dict(BASE, mant_bits=m, **WEIGHT_FORMS[wform])
    act = ACT_FORMS[aform]
    if act:
        if 'N' in act and a.get('sparsity_mode') == 'unstructured':
            return None                                                      # one sparsity_mode per config
        if 'sparsity_frac' in act and a.get('sparsity_mode') == 'structured':
            return None
        a.update(act)
        a.setdefault('sparsity_mode', 'structured' if 'N' in act else 'unstructured')
        a.setdefault('first', 's')
    return a


def _reference(x, lin, a):
    """the fp64 product of the reference's fake-quantised operands (MxM_pre_processing), its |x||w| and the bias"""
    xq, wq = bfp_ops.MxM_pre_processing(x, lin.weight, False, **bfp_ops.unpack_bfp_args(dict(a, device=DEV)))
    xv, wv = xq.double().reshape(-1, x.shape[-1]), wq.double()
    return xv @ wv.t() + lin.bias.double(), xv.abs() @ wv.abs().t() + lin.bias.double().abs()


MODULE_CASES = [(m, wf, af, (256, 512)) for m in (5, 7) for wf in WEIGHT_FORMS for af in ACT_FORMS if _cfg(m, wf, af) is not None]
MODULE_CASES.append((7, 'dense', 'dense', (24, 512)))          # out_features % 16 != 0: a shape the int8 unit refuses


@pytest.mark.parametrize("m,wform,aform,shape", MODULE_CASES,
                         ids=[f"{m}-{wf}-{af}" + ("" if shape == (256, 512) else f"-{shape[0]}x{shape[1]}") for m, wf, af, shape in MODULE_CASES])
def test_packed_module_matches_fake_quantised_bfplinear(m, wform, aform, shape):
    a = _cfg(m, wform, aform)
    N, K = shape
    torch.manual_seed(m)
    lin = torch.nn.Linear(K, N).to(DEV).to(torch.bfloat16)
    if shape != (256, 512):
        with torch.no_grad():        # (the fallback route adds the bias to the GEMM's rounded output: a second rounding, not in the bound)
            lin.bias.zero_()
    mod = PackedBFPLinear.from_linear(lin, a)
    assert mod.packed.code_bits == 8 and mod.codes.dtype == torch.int8
    for T in (7, 200):
        x = torch.randn(T, K, device=DEV).to(torch.bfloat16)
        with torch.no_grad():
            got = mod(x)
        want, absprod = _reference(x, lin, a)
        G.elementwise_bound(got, want, absprod, K // 64 + 10, torch.bfloat16)


def test_packed_module_hbfp5_prefill_keeps_the_block_scaled_route_and_state_dict():
    a = dict(BASE, mant_bits=4)
    torch.manual_seed(3)
    lin = torch.nn.Linear(512, 256).to(DEV).to(torch.bfloat16)
    mod = PackedBFPLinear.from_linear(lin, a)
    for T in (5, 100):
        x = torch.randn(T, 512, device=DEV).to(torch.bfloat16)
        with torch.no_grad():
            got = mod(x)
        want, absprod = _reference(x, lin, a)
        G.elementwise_bound(got, want, absprod, 512 // 64 + 10, torch.bfloat16)
    # state_dict: a fresh HBFP8 module of another Linear loads it and computes what the original does
    other = PackedBFPLinear.from_linear(torch.nn.Linear(512, 256).to(DEV).to(torch.bfloat16), dict(BASE, mant_bits=7))
    other.load_state_dict(mod.state_dict())
    x = torch.randn(33, 512, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        assert torch.equal(other(x), mod(x))
    assert other.packed.mant_bits == 4 and other.x_mant_bits == 4


def test_packed_module_state_dict_round_trip_hbfp8():
    torch.manual_seed(4)
    lin = torch.nn.Linear(512, 256).to(DEV).to(torch.bfloat16)
    mod = PackedBFPLinear.from_linear(lin, dict(BASE, mant_bits=7, in_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s'))
    sd = mod.state_dict()
    assert sd['codes'].dtype == torch.int8 and sd['codes'].shape == (256, 512)
    clone = copy.deepcopy(mod)
    clone.codes.zero_()
    clone.load_state_dict(sd)
    x = torch.randn(9, 512, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        assert torch.equal(clone(x), mod(x))


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=1000, max_position_embeddings=64)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


@pytest.mark.parametrize("m", (5, 7))
def test_pack_linear_layers_tiny_llama(m):
    pytest.importorskip("transformers")
    args = dict(BASE, mant_bits=m, w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s')
    base = _tiny_llama()
    fake, packed = copy.deepcopy(base), copy.deepcopy(base)
    patch_linear_layers(fake, args)
    fake.to(DEV)
    packed.to(DEV)
    names, saved = pack_linear_layers(packed, args)
    assert len(names) == 2 * 7 and saved > 0                                  # down_proj (K = 704) included: 8-bit codes take K % 64
    assert packed.model.layers[1].mlp.down_proj.packed.code_bits == 8
    for shape in ((1, 12), (2, 48)):
        tokens = torch.randint(0, 1000, shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        with torch.no_grad():
            a, b = fake(tokens).logits, packed(tokens).logits
        err = float((a - b).abs().max() / a.abs().max())
        assert err < 2e-3, (shape, err)


def test_cached_bfplinear_int8_unit():
    torch.manual_seed(6)
    a = dict(BASE, mant_bits=7)
    lin = bfp_ops.BFPLinear(512, 256, **dict(a)).to(DEV).to(torch.bfloat16).eval()
    lin.enable_weight_cache(matrix_unit='int8')
    cache = lin._weight_cache
    x = torch.randn(40, 512, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        y1 = lin(x)
        y1b = lin(x[:3])
        assert cache.i8_calls == 2 and cache.mx_calls == 0
        want, absprod = _reference(x, lin, a)
        G.elementwise_bound(y1, want, absprod, 512 // 64 + 10, torch.bfloat16)
        lin.weight.mul_(-1.0)                                                  # in place: the cached codes must follow
        y2 = lin(x)
        assert cache.i8_calls == 3
        want2, absprod2 = _reference(x, lin, a)
        G.elementwise_bound(y2, want2, absprod2, 512 // 64 + 10, torch.bfloat16)
        assert not torch.equal(y1, y2)
    assert y1b.shape == (3, 256)
    # matrix_unit=True keeps its meaning: HBFP8 is not on the block-scaled instruction
    lin2 = bfp_ops.BFPLinear(512, 256, **dict(a)).to(DEV).to(torch.bfloat16).eval()
    lin2.enable_weight_cache(matrix_unit=True)
    with torch.no_grad():
        lin2(x)
    assert lin2._weight_cache.mx_calls == 0 and lin2._weight_cache.i8_calls == 0


def test_graph_capture_packed_prefill():
    torch.manual_seed(8)
    lin = torch.nn.Linear(512, 256).to(DEV).to(torch.bfloat16)
    mod = PackedBFPLinear.from_linear(lin, dict(BASE, mant_bits=7))
    x = torch.randn(128, 512, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        eager = mod(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = mod(x)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)
