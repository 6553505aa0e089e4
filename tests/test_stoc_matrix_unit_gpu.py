"""BFPLinear.enable_stochastic_matrix_unit on the MI355X: 'stoc' inference forwards on the int8 / block-scaled matrix units.  With one
torch.manual_seed the new route's operands, decoded, are the fake route's operands bit for bit; the output is F.linear of those operands
up to the fp32 summation order; torch's generator ends where the fake route leaves it; a block whose exponent could overflow the dtype
redoes the call on the fake route with the same seeds."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import patch_linear_layers
from gemm_cases import elementwise_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _any_token_count(monkeypatch):
    """the route at every token count and dtype (bfp_ops.STOC_MIN_TOKENS, the measured limits, is the host tests' subject)"""
    monkeypatch.setattr(bfp_ops, 'STOC_MIN_TOKENS', {torch.bfloat16: 1, torch.float32: 1})


def _cfg(m, block, **sp):
    c = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='stoc', mant_bits=m, block_size=block, epsilon=1e-8)
    c.update(sp)
    return c


CONFIGS = {
    'hbfp4_b64_dense': _cfg(3, 64),
    'hbfp4_b64_24s': _cfg(3, 64, w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s'),
    'hbfp4_b64_24q': _cfg(3, 64, w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='q'),
    'hbfp6_b64_us': _cfg(5, 64, w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='s'),
    'hbfp6_b32_us': _cfg(5, 32, w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='s'),
    'hbfp8_b64_uq': _cfg(7, 64, w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='q'),
    'hbfp8_b32_uq': _cfg(7, 32, w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='q'),
    'hbfp8_b16_14': _cfg(7, 16, w_sparsity=True, sparsity_mode='structured', N=1, M=4, first='s'),
    'hbfp8_b64_in24': _cfg(7, 64, in_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s'),
}
# (T, N, K, aligned): small, LLaMA-7B q_proj, and operands 2 bytes off 16-byte alignment (the single-pass kernel refuses them)
SHAPES = {'small': (40, 256, 512, True), 'q_proj': (48, 4096, 4096, True), 'unaligned': (33, 128, 448, False)}


def _tensor(shape, dtype, aligned, gen, scale=1.0):
    n = shape[0] * shape[1]
    buf = (torch.randn(n + 1, generator=gen) * scale).to(dtype).to(DEV)
    return (buf[:n] if aligned else buf[1:]).view(shape)


def _linear(cfg, w, bias=None, stoc=True):
    lin = bfp_ops.BFPLinear(w.shape[1], w.shape[0], bias is not None, **dict(cfg)).to(DEV).eval()
    with torch.no_grad():
        lin.weight = torch.nn.Parameter(w, requires_grad=False)
        lin.bias = None if bias is None else torch.nn.Parameter(bias, requires_grad=False)
    if stoc:
        lin.enable_stochastic_matrix_unit(stoc)
    return lin


def _capture(monkeypatch):
    rec = []
    real = bfp_ops.float_to_bfp_blocked

    def spy(t, *a, identifier='', **kw):
        y = real(t, *a, identifier=identifier, **kw)
        rec.append((identifier, y.detach().clone()))
        return y
    monkeypatch.setattr(bfp_ops, "float_to_bfp_blocked", spy)
    return rec


def _decode(codes, exps, m, block):
    c = codes.float().view(codes.shape[0], -1, block)
    e = exps.float().view(codes.shape[0], -1, 1)
    v = c * torch.pow(2.0, e - m)
    return torch.where(e == -128, torch.full_like(v, float('nan')), v).view(codes.shape)


def _unsigned_zeros(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def _new_route_operands(monkeypatch, cfg, seed, x, lin):
    """the codes the opt-in forward hands the GEMM, decoded to fp32"""
    got = []
    real = native.stoc_codes

    def spy(t, block, m, eps, s, act=None):
        c, e = real(t, block, m, eps, s, act)
        got.append(_decode(c, e, m, block))
        return c, e
    monkeypatch.setattr(native, "stoc_codes", spy)
    torch.manual_seed(seed)
    with torch.no_grad():
        y = lin(x)
    monkeypatch.setattr(native, "stoc_codes", real)
    return y, got, torch.get_rng_state()


def _fake(monkeypatch, cfg, seed, x, w, bias=None):
    rec = _capture(monkeypatch)
    lin = _linear(cfg, w, bias, stoc=False)
    torch.manual_seed(seed)
    with torch.no_grad():
        y = lin(x)
    monkeypatch.undo()
    ops = {k: v for k, v in rec}
    return y, ops['in'], ops['w'], torch.get_rng_state()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("mu", [True, 'int8'], ids=['mu_true', 'mu_int8'])
def test_operands_output_rng(monkeypatch, name, dtype, shape, mu):
    cfg = CONFIGS[name]
    T, N, K, aligned = SHAPES[shape]
    g = torch.Generator().manual_seed(zlib.crc32(f'{name}/{shape}'.encode()))
    x = _tensor((T, K), dtype, aligned, g)
    w = _tensor((N, K), dtype, aligned, g, 0.02)
    bias = torch.randn(N, generator=g).to(DEV)
    lin = _linear(cfg, w, bias, stoc=mu)
    st = lin._stoc_matrix_unit
    y, got, rng_new = _new_route_operands(monkeypatch, cfg, 1234, x, lin)
    want = 'mx8' if (mu is True and cfg['mant_bits'] <= 4 and cfg['block_size'] == 64 and K % 256 == 0 and T >= 32) else 'int8'
    assert (st.stoc_mx_calls, st.stoc_i8_calls, st.fallbacks) == ((want == 'mx8') * 1, (want == 'int8') * 1, 0)
    yf, xq, wq, rng_fake = _fake(monkeypatch, cfg, 1234, x, w, bias)
    # 1. operands bit for bit, up to the sign of a zero (the fake route keeps the reference's -0.0 for small negatives; an integer code
    #    has no sign of zero, and the GEMM's sums do not see it)
    assert len(got) == 2
    for a, b in ((got[0], xq), (got[1], wq)):
        assert a.dtype == b.dtype == torch.float32
        a, b = _unsigned_zeros(a), _unsigned_zeros(b.view(a.shape))
        bad = a.view(torch.int32) != b.view(torch.int32)
        assert not bool(bad.any()), f"{int(bad.sum())} operand elements differ, e.g. {a[bad][:4].tolist()} vs {b[bad][:4].tolist()}"
    # 2. output within the fp32 summation bound of the exact product of the captured operands
    assert y.dtype == torch.float32 and y.shape == yf.shape
    exact = xq.double() @ wq.double().t() + bias.double()
    absprod = xq.double().abs() @ wq.double().abs().t() + bias.double().abs()
    assert torch.equal(torch.isnan(y), torch.isnan(exact))
    elementwise_bound(y, exact, absprod, K // cfg['block_size'] + 2, torch.float32)
    # 3. the generator ends where the fake route leaves it
    assert torch.equal(rng_new, rng_fake)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_other_forwards_keep_todays_path(monkeypatch, dtype):
    """grad-enabled, fp16, bf16-bias and 'determ' forwards do not take the route and give what a module without the opt-in gives"""
    g = torch.Generator().manual_seed(5)
    x = _tensor((40, 512), dtype, True, g)
    w = _tensor((256, 512), dtype, True, g, 0.02)
    cases = [(CONFIGS['hbfp8_b64_uq'], x, w, None, True),                       # grad enabled
             (CONFIGS['hbfp8_b64_uq'], x.half(), w.half(), None, False),       # fp16
             (CONFIGS['hbfp8_b64_uq'], x, w, torch.randn(256).to(DEV).bfloat16(), False),   # bf16 bias
             (dict(CONFIGS['hbfp8_b64_uq'], rounding_mode='determ'), x, w, None, False)]
    for cfg, xx, ww, bias, grad in cases:
        lin = _linear(cfg, ww, bias)
        ref = _linear(cfg, ww, bias, stoc=False)
        outs = []
        for m in (lin, ref):
            torch.manual_seed(9)
            try:
                with torch.set_grad_enabled(grad):
                    outs.append(m(xx).detach())
            except RuntimeError as e:                                    # (F.linear may refuse the mixed-dtype bias: then both refuse)
                outs.append(type(e))
        st = lin._stoc_matrix_unit
        assert st.stoc_mx_calls == st.stoc_i8_calls == 0
        if isinstance(outs[0], torch.Tensor):
            assert torch.equal(outs[0].view(-1).view(torch.uint8), outs[1].view(-1).view(torch.uint8))
        else:
            assert outs[0] == outs[1]


def test_no_shared_activation_draw():
    """two modules on the same input in one no_grad block draw their own activation noise (no activation memo)"""
    g = torch.Generator().manual_seed(6)
    x = _tensor((64, 512), torch.bfloat16, True, g)
    w = _tensor((256, 512), torch.bfloat16, True, g, 0.02)
    seen = []
    real = native.stoc_codes

    def spy(t, *a, **k):
        c, e = real(t, *a, **k)
        seen.append(c.clone())
        return c, e
    a = _linear(CONFIGS['hbfp4_b64_dense'], w)
    b = _linear(CONFIGS['hbfp4_b64_dense'], w)
    native.stoc_codes = spy
    try:
        with torch.no_grad():
            a(x)
            b(x)
    finally:
        native.stoc_codes = real
    assert a._stoc_matrix_unit.stoc_mx_calls == b._stoc_matrix_unit.stoc_mx_calls == 1
    assert not torch.equal(seen[0], seen[2]), "the two activation draws are the same"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_exponent_overflow_falls_back(monkeypatch, dtype):
    """a block whose 2^e overflows the dtype: the call is redone on the fake route with the same two seeds"""
    g = torch.Generator().manual_seed(7)
    x = _tensor((40, 512), dtype, True, g)
    x[3, 64:128] *= 2.0 ** 126                                         # block maximum above 2^127: 2^e overflows the dtype
    w = _tensor((256, 512), dtype, True, g, 0.02)
    cfg = CONFIGS['hbfp6_b64_us']
    lin = _linear(cfg, w)
    torch.manual_seed(11)
    with torch.no_grad():
        y = lin(x)
    rng = torch.get_rng_state()
    assert lin._stoc_matrix_unit.fallbacks == 1
    yf, _, _, rng_f = _fake(monkeypatch, cfg, 11, x, w)
    assert torch.equal(y.view(torch.int32), yf.view(torch.int32))
    assert torch.equal(rng, rng_f)


def _tiny_llama(dtype):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).to(dtype).eval()


@pytest.mark.parametrize("mu", [True, 'int8'], ids=['mu_true', 'mu_int8'])
def test_patched_llama(mu):
    pytest.importorskip("transformers")
    cfg = CONFIGS['hbfp4_b64_24s']
    ids = torch.randint(0, 512, (1, 48), generator=torch.Generator().manual_seed(3)).to(DEV)
    outs, mods = [], None
    for stoc, seed in ((mu, 21), (False, 21), (False, 22)):
        model = _tiny_llama(torch.float32).to(DEV)            # (fp32: the fp32 output of a 'stoc' Linear meets no bf16 layer)
        names = patch_linear_layers(model, cfg, stoc_matrix_unit=stoc)
        assert names
        torch.manual_seed(seed)
        with torch.no_grad():
            outs.append(model(ids).logits.float())
        if stoc:
            mods = [m for m in model.modules() if isinstance(m, bfp_ops.BFPLinear)]
    for m in mods:
        st = m._stoc_matrix_unit
        assert st.stoc_mx_calls + st.stoc_i8_calls == 1 and st.fallbacks == 0, m
    # same seeds, same operands: the logits differ only by the summation order inside each Linear, carried through two layers -- far
    # less than the fake route differs from itself under another seed
    assert torch.isfinite(outs[0]).all()
    same = (outs[0] - outs[1]).abs().max().item()
    other = (outs[2] - outs[1]).abs().max().item()
    assert same <= 0.1 * other, (same, other)
