"""The int8 matrix-unit GEMM at HBFP blocks 16 and 32 (bfpq_i8gemm.hip, k_i8_gemm<BLK> / k_i8_decode<BLK>): bit for bit on certified exact
operands, NaN blocks, random OPT-125m / ViT-L shapes within the fp32 summation bound, the packed and cached modules of BASELINE configs 1
and 5, a packed model and a captured prefill (run with `-m gpu` on an MI355X).  Exact operands and drivers: tests/gemm_cases.py and tests/test_i8gemm_gpu.py."""
import copy

import pytest
import torch

import gemm_cases as G
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, pack_linear_layers, patch_linear_layers
from test_i8gemm_gpu import DEV, DTS, TUNE_I8_VARIANT, WIDTHS, L, assert_bits, certified, every_plan, expected, i8, run_c

pytestmark = pytest.mark.gpu
TOKENS = tuple(range(1, 18)) + (64, 65, 128, 197, 512, 2048, 301)
BLOCKS = (16, 32)


@pytest.mark.parametrize("blk", BLOCKS)
@pytest.mark.parametrize("xm", WIDTHS)
@pytest.mark.parametrize("wm", WIDTHS)
def test_exact_every_width(blk, xm, wm):
    for T in (1, 33, 257):
        N, K = 80, 512
        xc, xe, wc, we, bias = certified(T, N, K, xm, wm, seed=100 * xm + 10 * wm + T + blk, with_bias=(T % 2 == 1), block=blk)
        every_plan(xc, xe, xm, wc, we, wm, bias, T, N, K, torch.bfloat16, f"b{blk} xm {xm} wm {wm} T {T}", block=blk)


@pytest.mark.parametrize("blk", BLOCKS)
@pytest.mark.parametrize("dt", DTS)
def test_exact_every_token_count(blk, dt):
    for T in TOKENS:
        for with_bias in (False, True):
            N, K = 144, 768
            xc, xe, wc, we, bias = certified(T, N, K, 5, 7, seed=T * 3 + int(with_bias) + blk, with_bias=with_bias, block=blk)
            every_plan(xc, xe, 5, wc, we, 7, bias, T, N, K, dt, f"b{blk} {dt} T {T} bias {with_bias}", block=blk,
                       variants=range(3) if T in (1, 17, 197, 2048) else (0,))


@pytest.mark.parametrize("blk", BLOCKS)
def test_exact_k_not_multiple_of_256_and_nm_weights(blk):
    for (T, N, K, nm) in ((20, 48, 320, (0, 0)), (300, 32, 192, (0, 0)), (65, 128, 512, (2, 4)), (197, 64, 1024, (1, 4)), (17, 64, 1024, (4, 8))):
        xc, xe, wc, we, bias = certified(T, N, K, 7, 6, seed=T + N + blk, nm=nm, with_bias=True, block=blk)
        every_plan(xc, xe, 7, wc, we, 6, bias, T, N, K, torch.float32, f"b{blk} T {T} N {N} K {K} nm {nm}", block=blk)


@pytest.mark.parametrize("blk", BLOCKS)
@pytest.mark.parametrize("T", (1, 16, 17, 64, 300))
def test_exact_4bit_weights_through_the_expansion(blk, T):
    N, K = 96, 512
    for wm in (1, 3):
        xc, xe, wc, we, bias = certified(T, N, K, 7, wm, seed=T + wm + blk, with_bias=True, block=blk)
        pk = bfp_ops.PackedBFP(G.pack4(wc), i8(we), (N, K), torch.float32, wm, blk, 4)
        assert torch.equal(pk._i8_codes(), i8(wc))
        want = expected(xc, xe, 7, wc, we, wm, bias, torch.float32, block=blk)
        got = native.hbfp_linear_i8(torch.empty((T, K), dtype=torch.float32, device=DEV), pk._i8_codes(), pk.exps, wm, 7,
                                    bias=bias.float(), xq=(i8(xc), i8(xe)), block_size=blk)
        assert_bits(got, want, f"b{blk} 4-bit weights wm {wm} T {T}")


@pytest.mark.parametrize("blk", BLOCKS)
def test_nan_blocks_every_route(blk):
    N, K = 64, 512
    for T in (3, 40):
        xc, xe, wc, we, _ = certified(T, N, K, 7, 7, seed=77 + blk, block=blk)
        xe, we = xe.clone(), we.clone()
        xe[1, 5] = -128
        we[5, 11] = -128
        want = expected(xc, xe.clamp_min(-127), 7, wc, we.clamp_min(-127), 7, None, torch.float32, block=blk)
        want[1, :] = float("nan")
        want[:, 5] = float("nan")
        xq = (i8(xc), i8(xe))
        assert_bits(run_c('decode8', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7, block=blk), want, f"b{blk} decode8 NaN T {T}")
        try:
            for v in range(3):
                L().bfpq_tune(TUNE_I8_VARIANT, v)
                assert_bits(run_c('tile', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7, block=blk), want, f"b{blk} tile {v} NaN T {T}")
                assert_bits(run_c('split', *xq, i8(wc), i8(we), None, T, N, K, torch.float32, 7, 7, parts=2, block=blk), want, f"b{blk} split {v} NaN")
        finally:
            L().bfpq_tune(TUNE_I8_VARIANT, -1)


@pytest.mark.parametrize("blk", BLOCKS)
@pytest.mark.parametrize("shape", ((768, 768), (3072, 768), (768, 3072), (1024, 1024), (4096, 1024), (1024, 4096)))
def test_random_opt_vit_shapes(blk, shape):
    N, K, m = shape[0], shape[1], 7
    g = torch.Generator(device=DEV).manual_seed(N + K + blk)
    w = torch.randn(N, K, generator=g, device=DEV) * 0.02
    wc, we = bfp_ops.float_to_bfp_packed(w, m, blk, code_bits=8)
    wv = G.values(wc.view(N, K).int(), we.int(), m, block=blk)
    cfg = bfp_ops.unpack_bfp_args(dict(mant_bits=m, block_size=blk, num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ', device=DEV))
    for T in (1, 16, 197, 2048):
        x = torch.randn(T, K, generator=g, device=DEV)
        xc, xe = native.act_codes(x, m, 1e-8, None, block_size=blk)
        xv = G.values(xc.int(), xe.int(), m, block=blk)
        assert torch.equal(xv.float(), bfp_ops.float_to_bfp_blocked(x, **cfg, identifier='in'))
        want, absprod = xv @ wv.t(), xv.abs() @ wv.abs().t()
        got = native.hbfp_linear_i8(x, wc.view(N, K), we, m, m, block_size=blk)
        G.elementwise_bound(got, want, absprod, K // blk + 8, torch.float32)
        assert torch.equal(got, native.hbfp_linear_i8(x, wc.view(N, K), we, m, m, block_size=blk))


def want_of(x, lin, a):
    return _reference(x, lin, a)[0]


def absprod_of(x, lin, a):
    return _reference(x, lin, a)[1]


def _reference(x, lin, a):
    xq, wq = bfp_ops.MxM_pre_processing(x, lin.weight, False, **bfp_ops.unpack_bfp_args(dict(a, device=DEV)))
    xv, wv = xq.double().reshape(-1, x.shape[-1]), wq.double()
    b = lin.bias.double()
    return xv @ wv.t() + b, xv.abs() @ wv.abs().t() + b.abs()


BASE = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ', epsilon=1e-8)
CFG5 = dict(BASE, mant_bits=7, block_size=16, w_sparsity=True, in_sparsity=True, sparsity_mode='structured', N=1, M=4, first='s')
CFG1 = dict(BASE, mant_bits=7, block_size=32)
CFG_U = {first: dict(BASE, mant_bits=7, block_size=blk, in_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first=first)
         for first, blk in (('s', 32), ('q', 16))}


@pytest.mark.parametrize("name,a,shape", [("config5", CFG5, (4096, 1024)), ("config5", CFG5, (1024, 4096)), ("config1", CFG1, (3072, 768)),
                                          ("config1", CFG1, (768, 3072)), ("unstructured s-first b32", CFG_U['s'], (768, 768)),
                                          ("unstructured q-first b16", CFG_U['q'], (1024, 1024))])
def test_packed_module_configs(name, a, shape):
    N, K = shape
    torch.manual_seed(N + K)
    lin = torch.nn.Linear(K, N).to(DEV)
    mod = PackedBFPLinear.from_linear(lin, a)
    ref = bfp_ops.BFPLinear(K, N, **dict(a)).to(DEV).eval()
    ref.load_state_dict(lin.state_dict())
    for T in (1, 17, 197, 2 * 197):
        x = torch.randn(T, K, device=DEV)
        with torch.no_grad():
            route = bfp_ops.linear_route(T, N, K, mod.packed.code_bits, 7, 7, i8_max_tokens=bfp_ops.I8_MAX_TOKENS, block_size=a['block_size'])
            route = bfp_ops.linear_route(T, N, K, mod.packed.code_bits, 7, 7, i8_max_tokens=bfp_ops.I8_MAX_TOKENS, block_size=a['block_size'],
                                         dtype=x.dtype)
            assert route == 'int8', (name, T, route)             # (fp32 activations: the int8 unit at every token count)
            G.elementwise_bound(mod.packed.linear_i8(x, lin.bias, 7, 1e-8, mod.x_sparsity), want_of(x, ref, a), absprod_of(x, ref, a),
                                K // a['block_size'] + 10, torch.float32)
            got = mod(x)
            want, absprod = _reference(x, ref, a)
            G.elementwise_bound(got, want, absprod, K // a['block_size'] + 10, torch.float32)
            G.elementwise_bound(ref(x), want, absprod, K // a['block_size'] + 10, torch.float32)
    sd = mod.state_dict()
    mod2 = PackedBFPLinear.from_linear(torch.nn.Linear(K, N).to(DEV), a)
    mod2.load_state_dict(sd)
    x = torch.randn(5, K, device=DEV)
    with torch.no_grad():
        assert torch.equal(mod2(x), mod(x))
        assert torch.equal(mod2.cpu().to(DEV)(x), mod(x))


class _TinyViT(torch.nn.Module):
    def __init__(self, d=256, h=1024, depth=2):
        super().__init__()
        self.blocks = torch.nn.ModuleList(torch.nn.ModuleDict(dict(qkv=torch.nn.Linear(d, 3 * d), proj=torch.nn.Linear(d, d),
                                                                 fc1=torch.nn.Linear(d, h), fc2=torch.nn.Linear(h, d))) for _ in range(depth))
        self.head = torch.nn.Linear(d, 10)

    def forward(self, x):
        for b in self.blocks:
            q, k, v = b['qkv'](x).chunk(3, dim=-1)
            att = torch.softmax(q @ k.transpose(-1, -2) / 16.0, dim=-1)
            x = x + b['proj'](att @ v)
            x = x + b['fc2'](torch.nn.functional.gelu(b['fc1'](x)))
        return self.head(x.mean(dim=1))


@pytest.mark.parametrize("a", [CFG5, dict(BASE, mant_bits=7, block_size=16)], ids=["1:4", "dense"])
def test_pack_linear_layers_tiny_vit_block16(a):
    for tokens, dt in ((197, torch.float32), (8, torch.bfloat16)):     # fp32: the int8 tile at 394 tokens; bf16: the few-token kernel
        torch.manual_seed(3)
        fake = _TinyViT().to(DEV).to(dt).eval()
        packed = copy.deepcopy(fake)
        patch_linear_layers(fake, a, skip=("head",))
        names, saved = pack_linear_layers(packed, a, skip=("head",))
        assert len(names) == 8 and saved > 0
        for n in names:
            mod = packed.get_submodule(n)
            assert bfp_ops.linear_route(2 * tokens, mod.out_features, mod.in_features, mod.packed.code_bits, 7, 7,
                                        i8_max_tokens=bfp_ops.I8_MAX_TOKENS, block_size=16, dtype=dt) == 'int8', n
        x = torch.randn(2, tokens, 256, device=DEV).to(dt)
        calls = []
        real = native.hbfp_linear_i8
        native.hbfp_linear_i8 = lambda *args, **kw: calls.append(kw.get('block_size')) or real(*args, **kw)
        try:
            with torch.no_grad():
                y, want = packed(x), fake(x)
        finally:
            native.hbfp_linear_i8 = real
        assert calls == [16] * 8, calls                                  # every packed layer on the int8 unit at block 16
        err = float((y.float() - want.float()).abs().max() / want.float().abs().max())
        assert torch.isfinite(y).all() and err < (1e-4 if dt == torch.float32 else 2e-2), (dt, err)


@pytest.mark.parametrize("blk", BLOCKS)
def test_cached_bfplinear_int8_unit(blk):
    torch.manual_seed(6)
    a = dict(BASE, mant_bits=7, block_size=blk)
    lin = bfp_ops.BFPLinear(512, 256, **dict(a)).to(DEV).eval()
    lin.enable_weight_cache(matrix_unit='int8')
    cache = lin._weight_cache
    x = torch.randn(12, 512, device=DEV)                 # (within I8_SMALL_BLOCK_MAX_TOKENS)
    with torch.no_grad():
        y = lin(x)
        lin(x[:3])
        assert cache.i8_calls == 2 and cache.mx_calls == 0
        want, absprod = _reference(x, lin, a)
        G.elementwise_bound(y, want, absprod, 512 // blk + 10, torch.float32)


def test_graph_capture_block16_prefill():
    torch.manual_seed(8)
    lin = torch.nn.Linear(1024, 512).to(DEV)
    mod = PackedBFPLinear.from_linear(lin, CFG5)
    x = torch.randn(197, 1024, device=DEV)
    pk = mod.packed
    with torch.no_grad():                                  # (the int8 prefill itself, whatever the route table picks for 197 tokens)
        eager = pk.linear_i8(x, mod.bias, 7, 1e-8, mod.x_sparsity)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = pk.linear_i8(x, mod.bias, 7, 1e-8, mod.x_sparsity)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)
