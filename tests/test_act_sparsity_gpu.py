"""Pruned activations (the reference's in_sparsity, identifier 'in') on the packed and matrix-unit Linear paths: the one-pass N:M
image, the unstructured image after the selection, PackedBFP / PackedBFPLinear with x_sparsity, the cached BFPLinear on the matrix
unit, the activation-image memo, a whole model and a captured prefill."""
import copy

import numpy as np
import pytest
import torch

import quantization_sparsity_interplay_amd as pkg
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, pack_linear_layers, patch_linear_layers
from util import DT
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = native.ActSparsity


def cfg(**kw):
    base = dict(mant_bits=3, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64,
                num_format='bfp', weight_mant_bits=15, in_sparsity=True, w_sparsity=False,
                grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp',
                first='s', sparsity_mode='structured')
    base.update(kw)
    return base


def synth(rows, cols, dtype, scale=0.02, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(dtype)


_E4 = np.zeros(256, dtype=np.float64)
for _m, _b in enumerate([0, 0x38, 0x40, 0x44, 0x48, 0x4a, 0x4c, 0x4e] + [0x50 + i for i in range(8)]):
    _E4[_b] = _m
    _E4[_b | 0x80] = -_m


def decode_image(x8, xs):
    """e4m3 mantissas (integers <= 15) x E8M0 block scales, in fp64 on the host"""
    return torch.from_numpy(_E4[x8.cpu().numpy()]) * torch.exp2(xs.cpu().double() - 127).repeat_interleave(64, dim=1)


def assert_images_equal(a8, asc, b8, bsc):
    """byte equality with the conventions of the dense image test: mantissas of a NaN block are don't-care, and a
    two's-complement int8 code has no -0 (magnitudes equal, signs of the non-zero mantissas equal)"""
    assert torch.equal(asc, bsc)
    nanblk = (bsc == 255).repeat_interleave(64, dim=1)
    a, b = a8.clone(), b8.clone()
    a[nanblk] = 0
    b[nanblk] = 0
    assert torch.equal(a & 0x7f, b & 0x7f)
    nz = (b & 0x7f) != 0
    assert torch.equal(a[nz], b[nz])
    return nanblk


def edge_input(rows, dname, seed=21):
    x = synth(rows, 1024, DT[dname], 1.0, seed=seed)
    x[0, :64] = 0                                                       # zero block
    x[1, 64:128] *= 3e4 if dname == "f16" else 1e30                     # extreme scales (cold tier)
    x[2, :64] *= 1e-7 if dname == "f16" else 1e-35
    x[3, 5] = float("inf")                                              # an inf block
    x[4, 64:128] = 0.75                                                 # rounding ties of every element
    x[5, :256] = torch.tensor([0.5, -0.5, 0.25, 0.5, 0.125, -0.125, 0.125, 0.125] * 32)   # ties at the N:M cut
    x[6, 128:384] = -0.3                                                # a whole group row of equal magnitudes
    # already-quantized values: after Q most groups tie at the cut (the q-first order sees them)
    x[7:12] = bfp_ops.float_to_bfp_blocked(x[7:12].to(DEV), **cfg(in_sparsity=False, mant_bits=1), identifier='in').cpu()
    return x


# ---- 1. the one-pass N:M image ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("first", ["s", "q"])
@pytest.mark.parametrize("N,M", [(2, 4), (1, 4), (4, 8), (2, 2)])
def test_nm_image_equals_codes_then_image_and_the_oracle(N, M, first, dname):
    x = edge_input(96, dname).to(DEV)
    act = A('structured', N, M, 0.0, first)
    for xm in (1, 2, 3, 4):
        x8, xs = native.quantize_mx8(x, xm, act=None if N == M else act)
        _, xc, xe = native.quantize_nm(x, 64, xm, 1e-8, N=N, M=M, sparsify_first=(first == 's'), want_deq=False, code_bits=8, want_exp=True)
        w8, ws = native.mx8_from_hbfp(xc, xe, 1024, xm, 8)
        nanblk = assert_images_equal(x8, xs, w8, ws)
        if dname != "f32":
            assert bool(nanblk.any())
        # the decoded image is the reference's activation operand
        want = O.float_to_bfp_blocked(x.cpu(), **cfg(mant_bits=xm, N=N, M=M, first=first, device='cpu'), identifier='in').double()
        val = decode_image(x8, xs)
        ok = ~nanblk.cpu() & torch.isfinite(want) & (xs.cpu().repeat_interleave(64, dim=1) > 0)
        assert torch.equal(val[ok], want[ok]), (xm, int((val[ok] != want[ok]).sum()))
        if N < M:                                                       # the entry point itself (not a fallback) ran
            o8, osc = torch.empty_like(x8), torch.empty_like(xs)
            lut = native.nm4_lut_dev(N, x.device) if M == 4 else None
            rc = native.load_library().bfpq_quantize_mx8_nm(native._ptr(x), native._ptr(o8), native._ptr(osc), 96, 1024, native.DTYPE_CODE[x.dtype],
                                                            xm, 1e-8, N, M, 1 if first == 's' else 0, native._ptr(native.exp_window_dev(x.dtype, x.device)),
                                                            native._ptr(lut), native._stream(x))
            assert rc == 0
            assert torch.equal(o8, x8) and torch.equal(osc, xs)


def test_nm8_image_without_the_rank_table():
    """N:8 groups whose ties straddle the cut replay nth_element in the kernel when no table is given: same image"""
    x = edge_input(64, "bf16").to(DEV)
    for first in ("s", "q"):
        act = A('structured', 3, 8, 0.0, first)
        a8, asc = native.quantize_mx8(x, 3, act=act)
        try:
            native.USE_NM8_TABLE = False
            b8, bsc = native.quantize_mx8(x, 3, act=act)
        finally:
            native.USE_NM8_TABLE = True
        assert torch.equal(a8, b8) and torch.equal(asc, bsc)


def test_nm_image_of_an_unsupported_m_takes_the_codes_route():
    x = synth(64, 768, torch.bfloat16, 1.0).to(DEV)
    act = A('structured', 2, 6, 0.0, 's')
    x8, xs = native.quantize_mx8(x, 3, act=act)
    want = bfp_ops.float_to_bfp_blocked(x, **cfg(N=2, M=6), identifier='in').double().cpu()
    assert torch.equal(decode_image(x8, xs), want)


_E4_DEV = {}


def decode_image_dev(x8, xs):
    """decode_image on the device (tensors too large for a host copy in fp64)"""
    lut = _E4_DEV.get(x8.device)
    if lut is None:
        lut = _E4_DEV[x8.device] = torch.from_numpy(_E4).to(x8.device)
    return lut[x8.long()] * torch.exp2(xs.double() - 127).repeat_interleave(64, dim=1)


def assert_image_decodes_to(x8, xs, want):
    """the image's values are `want`; a block the reference turns into NaN (fp16: an all-zero block, whose epsilon underflows) is the
    image's NaN block (scale byte 0xff)"""
    nanblk = (xs == 255).repeat_interleave(64, dim=1)
    assert torch.equal(torch.isnan(want), nanblk)
    assert torch.equal(decode_image_dev(x8, xs)[~nanblk], want[~nanblk])


@pytest.mark.parametrize("N,M,first", [(2, 4, 's'), (2, 4, 'q'), (4, 8, 's'), (4, 8, 'q')])
def test_nm_image_of_a_prefill_sized_activation(N, M, first):
    """[2048, 11008] bf16 (a LLaMA-7B down_proj input): 2.8 M lane items, several full sweeps of the grid, so the unguarded main loop
    of the one-pass kernel writes most of the image (the smaller cases above run in its guarded tail)"""
    x = synth(2048, 11008, torch.bfloat16, 1.0, seed=31).to(DEV)
    x[100:300] = bfp_ops.float_to_bfp_blocked(x[100:300], **cfg(in_sparsity=False, mant_bits=1), identifier='in')     # ties at the cut
    act = A('structured', N, M, 0.0, first)
    x8, xs = native.quantize_mx8(x, 3, act=act)
    _, xc, xe = native.quantize_nm(x, 64, 3, 1e-8, N=N, M=M, sparsify_first=(first == 's'), want_deq=False, code_bits=8, want_exp=True)
    w8, ws = native.mx8_from_hbfp(xc, xe, 11008, 3, 8)
    assert_images_equal(x8, xs, w8, ws)
    want = bfp_ops.float_to_bfp_blocked(x, **cfg(N=N, M=M, first=first), identifier='in').double()
    assert_image_decodes_to(x8, xs, want)


def _cut_early(rows, cols, dtype, seed):
    """an activation whose unstructured threshold at 50 % is a magnitude v held (with both signs) by the first tenth of the rows only, the
    rest strictly below v / 2 or above 2 v (half each): the cut -- where the ties of the pruned half end -- lies at 1/20 of the tensor,
    i.e. inside the first sweep of the apply launch's ordinary workgroups"""
    g = torch.Generator().manual_seed(seed)
    v = 0.375
    u = torch.rand(rows, cols, generator=g)
    sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    low = torch.rand(rows, cols, generator=g) < 0.5
    mag = torch.where(low, v * 0.5 * u, 2 * v + 4 * u)
    mag[: rows // 10] = v
    return (sign * mag).to(dtype)


@pytest.mark.parametrize("dname", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["cut_early", "tied"])
def test_unstructured_image_of_a_prefill_sized_activation(dname, kind):
    """[2048, 11008] (2.8 M lane items): the threshold-mode image kernel runs full unguarded sweeps, and an ordinary workgroup's tiles of
    the cut segment go through the unguarded store (redirected to the dump, exponent store with no lane enabled) while the cut workgroups
    store them.  Checked byte for byte against the codes route (selection + int8 codes + mx8_from_hbfp), value for value against the
    drop-in op, and for determinism."""
    dt = DT[dname]
    if kind == "cut_early":
        x = _cut_early(2048, 11008, dt, 41).to(DEV)
    else:
        x = bfp_ops.float_to_bfp_blocked(synth(2048, 11008, dt, 1.0, seed=42).to(DEV), **cfg(in_sparsity=False), identifier='in')
    act = A('unstructured', 0, 0, 0.5, 's')
    x8, xs = native.quantize_mx8(x, 3, act=act)
    ws_ = bfp_ops._workspace(x.device)
    native.select_threshold(x, x.numel() // 2, ws_)
    st = ws_.read_state()
    assert st["done"] == 1 and 0 < st["need"] <= st["ties"]
    if kind == "cut_early":
        # every tie lies in the first 204 rows and only some of them go: the cut segment is in the first sweep (unguarded trips)
        assert st["ties"] == 204 * 11008 and st["need"] == x.numel() // 2 - int((x.abs() < 0.375).sum()) and st["need"] < st["ties"]
    _, xc, xe = native.quantize_threshold(x, ws_, 64, 3, 1e-8, want_deq=False, code_bits=8, want_exp=True)
    w8, wsc = native.mx8_from_hbfp(xc, xe, 11008, 3, 8)
    assert_images_equal(x8, xs, w8, wsc)
    want = bfp_ops.float_to_bfp_blocked(x, **cfg(sparsity_mode='unstructured', sparsity_frac=0.5, first='s'), identifier='in').double()
    assert_image_decodes_to(x8, xs, want)
    assert int(((want == 0) | torch.isnan(want)).sum()) >= x.numel() // 2
    for _ in range(3):                                                  # no race between ordinary and cut workgroups
        y8, ys = native.quantize_mx8(x, 3, act=act)
        assert torch.equal(y8, x8) and torch.equal(ys, xs)


# ---- 2. the unstructured image ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape,tied", [((96, 1024), False), ((2048, 4096), True), ((300, 512), True)])
def test_unstructured_image_equals_the_drop_in(dname, shape, tied):
    """prune first: selection + the threshold-mode image; the drop-in result is pinned to the oracle's tie-class contract elsewhere.
    Tie-heavy activations (already-HBFP4 values) put thousands of ties into the cut segment."""
    dt = DT[dname]
    x = synth(*shape, dt, 1.0, seed=5).to(DEV)
    if tied:
        x = bfp_ops.float_to_bfp_blocked(x, **cfg(in_sparsity=False), identifier='in')
    for frac in (0.5, 0.3):
        c = cfg(sparsity_mode='unstructured', sparsity_frac=frac, first='s')
        want = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
        x8, xs = native.quantize_mx8(x, 3, act=A('unstructured', 0, 0, frac, 's'))
        assert torch.equal(decode_image(x8, xs), want)
        assert int((want == 0).sum()) >= int(x.numel() * frac)


@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_unstructured_quantize_first_image(dname):
    """S(Q(x)) through the composed route: the decoded image equals the drop-in op, and (outside the tie class, where the reference's
    positions are not reproduced) the oracle"""
    dt = DT[dname]
    x = synth(256, 1024, dt, 1.0, seed=8).to(DEV)
    c = cfg(sparsity_mode='unstructured', sparsity_frac=0.5, first='q')
    x8, xs = native.quantize_mx8(x, 3, act=A('unstructured', 0, 0, 0.5, 'q'))
    got = decode_image(x8, xs)
    want = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
    assert torch.equal(got, want)
    q = O.float_to_bfp_blocked(x.cpu(), **cfg(in_sparsity=False, device='cpu'), identifier='in').double()
    ref = O.float_to_bfp_blocked(x.cpu(), **dict(c, device='cpu'), identifier='in').double()
    k = int(x.numel() * 0.5)
    tau = q.abs().flatten().kthvalue(k).values
    outside = q.abs() != tau
    assert torch.equal(got[outside], ref[outside])


# ---- 3. PackedBFPLinear with in_sparsity -------------------------------------------------------------------------
CONFIGS = [
    dict(sparsity_mode='structured', N=2, M=4, first='s', w_sparsity=True),
    dict(sparsity_mode='structured', N=2, M=4, first='q', w_sparsity=True),
    dict(sparsity_mode='structured', N=1, M=4, first='s', w_sparsity=True),
    dict(sparsity_mode='structured', N=4, M=8, first='s', w_sparsity=True),
    dict(sparsity_mode='unstructured', sparsity_frac=0.5, first='s', w_sparsity=True),
    dict(sparsity_mode='unstructured', sparsity_frac=0.5, first='q', w_sparsity=False),     # (q-first unstructured weights are not packed)
]
TOL = {"f32": 2e-6, "bf16": 6e-3, "f16": 8e-4}


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_packed_linear_with_pruned_activations(ci, dname):
    dt = DT[dname]
    c = cfg(**CONFIGS[ci])
    torch.manual_seed(3)
    lin = torch.nn.Linear(512, 256).to(DEV).to(dt)
    pl = PackedBFPLinear.from_linear(lin, c)
    assert pl.x_sparsity == A.from_bfp_args(bfp_ops.unpack_bfp_args(dict(c)))
    ref = bfp_ops.BFPLinear(512, 256, True, **dict(c)).to(DEV).to(dt).eval()
    with torch.no_grad():
        ref.weight.copy_(lin.weight)
        ref.bias.copy_(lin.bias)
    wq = pl.packed.dequantize().double().cpu()
    for T in (1, 12, 40, 64, 200, 2048):                             # <= 64: decode kernels (the threshold spans every chunk); more: matrix unit
        x = synth(T, 512, dt, 1.0, seed=T).to(DEV)
        with torch.no_grad():
            got = pl(x)
            base = ref(x)
        assert got.shape == (T, 256) and got.dtype == dt
        xq = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
        want = xq @ wq.t() + lin.bias.detach().double().cpu()
        scale = float(want.abs().max())
        err = float((got.double().cpu() - want).abs().max()) / scale
        assert err < TOL[dname], (T, err)
        err2 = float((got.double().cpu() - base.double().cpu()).abs().max()) / scale
        assert err2 < 2 * TOL[dname], (T, err2)


def test_packed_linear_with_an_m_the_kernels_do_not_take():
    """an activation M outside {2, 4, 8} uses the codes route on every path; it must not raise"""
    c = cfg(N=2, M=16, w_sparsity=False)
    lin = torch.nn.Linear(512, 256).to(DEV).to(torch.bfloat16)
    pl = PackedBFPLinear.from_linear(lin, c)
    wq = pl.packed.dequantize().double().cpu()
    for T in (5, 300):
        x = synth(T, 512, torch.bfloat16, 1.0, seed=T).to(DEV)
        with torch.no_grad():
            got = pl(x)
        xq = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
        want = xq @ wq.t() + lin.bias.detach().double().cpu()
        assert float((got.double().cpu() - want).abs().max() / want.abs().max()) < 6e-3


# ---- 4. the cached BFPLinear on the matrix unit ---------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 3, 4])
def test_cached_bfplinear_matrix_unit_with_pruned_activations(ci):
    c = cfg(**CONFIGS[ci])
    dt = torch.bfloat16
    lin = bfp_ops.BFPLinear(1024, 384, False, **dict(c)).to(DEV).to(dt).eval().enable_weight_cache(matrix_unit=True)
    cache = lin.linear_op.weight_cache
    x = synth(200, 1024, dt, 1.0, seed=9).to(DEV)
    with torch.no_grad():
        got = lin(x).double().cpu()
    assert cache.mx_calls == 1
    wq = bfp_ops.float_to_bfp_blocked(lin.weight.detach(), **c, identifier='w').double().cpu()
    xq = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
    want = xq @ wq.t()
    assert float((got - want).abs().max() / want.abs().max()) < 6e-3
    with torch.no_grad():
        lin(synth(8, 1024, dt, 1.0).to(DEV))                             # short input: the ordinary route
    assert cache.mx_calls == 1
    lin.train()
    with torch.no_grad():
        lin(x)                                                          # training mode: the ordinary route
    assert cache.mx_calls == 1


# ---- 5. the activation-image memo ---------------------------------------------------------------------------------
def test_memo_keeps_images_of_different_specs_apart(monkeypatch):
    dt = torch.bfloat16
    x = synth(256, 512, dt, 1.0, seed=4).to(DEV)
    lins = [torch.nn.Linear(512, 256, bias=False).to(DEV).to(dt) for _ in range(3)]
    dense = PackedBFPLinear.from_linear(lins[0], cfg(in_sparsity=False))
    s24 = PackedBFPLinear.from_linear(lins[0], cfg())
    native.forget_shared_images()
    with torch.no_grad():
        a, b = dense(x), s24(x)
    for mod, c in ((dense, cfg(in_sparsity=False)), (s24, cfg())):
        xq = bfp_ops.float_to_bfp_blocked(x, **c, identifier='in').double().cpu()
        want = xq @ mod.packed.dequantize().double().cpu().t()
        got = a if mod is dense else b
        assert float((got.double().cpu() - want).abs().max() / want.abs().max()) < 6e-3
    assert not torch.equal(a, b)
    # three projections of one input with the same spec: one image
    calls = []
    real = native.quantize_mx8
    monkeypatch.setattr(native, "quantize_mx8", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    mods = [PackedBFPLinear.from_linear(l, cfg()) for l in lins]
    native.forget_shared_images()
    with torch.no_grad():
        outs = [m(x) for m in mods]
    assert len(calls) == 1
    with torch.no_grad():
        s24(x)
    assert len(calls) == 1
    with torch.no_grad():
        dense(x)                                                        # another spec: another image
    assert len(calls) == 2
    assert all(o.shape == (256, 256) for o in outs)


# ---- 6. a whole model ---------------------------------------------------------------------------------------------
def test_packed_model_with_pruned_activations():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    lc = LlamaConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                     vocab_size=1000, max_position_embeddings=64)
    base = LlamaForCausalLM(lc).to(torch.float32).eval()
    args = pkg.BFPConfig.hbfp(4, 64, w_sparsity=True, in_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
    fake, packed = copy.deepcopy(base), copy.deepcopy(base)
    patch_linear_layers(fake, args)
    fake.to(DEV)
    packed.to(DEV)
    names, _ = pack_linear_layers(packed, args)
    assert len(names) == 14
    for shape in ((1, 12), (2, 48)):
        tokens = torch.randint(0, 1000, shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        with torch.no_grad():
            a, b = fake(tokens).logits, packed(tokens).logits
        err = float((a - b).abs().max() / a.abs().max())
        assert err < 2e-3, (shape, err)
    sd = packed.state_dict()
    clone = copy.deepcopy(base).to(DEV)
    pack_linear_layers(clone, pkg.BFPConfig.hbfp(4, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs())
    assert clone.model.layers[0].mlp.up_proj.x_sparsity is None
    clone.load_state_dict(sd)
    assert clone.model.layers[0].mlp.up_proj.x_sparsity == A('structured', 2, 4, 0.0, 's')
    tokens = torch.randint(0, 1000, (1, 12), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        assert torch.equal(clone(tokens).logits, packed(tokens).logits)


# ---- 7. hipGraph capture ------------------------------------------------------------------------------------------
def test_captured_prefill_with_unstructured_activations():
    dt = torch.bfloat16
    lin = torch.nn.Linear(1024, 512).to(DEV).to(dt)
    pl = PackedBFPLinear.from_linear(lin, cfg(sparsity_mode='unstructured', sparsity_frac=0.5, first='s', w_sparsity=True))
    x = synth(256, 1024, dt, 1.0, seed=12).to(DEV)
    with torch.no_grad():
        eager = pl(x)                                                    # warm-up outside the capture: workspaces, tables, weight image
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = pl(x)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
    with torch.no_grad():
        x.copy_(synth(256, 1024, dt, 1.0, seed=13))
        g.replay()
        torch.cuda.synchronize()
        native.forget_shared_images()
        assert torch.equal(out, pl(x))
