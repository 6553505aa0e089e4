"""The block-scaled prefill GEMM with the packed tensor itself as the weight operand (native.hbfp_linear_mx4w, hold_image=False): run
with `-m gpu` on an MI355X.

  * bit for bit against the image route: hbfp_linear_mx4w(codes, exps) == hbfp_linear_mx8(mx8_from_hbfp(codes, exps)) on the raw bits,
    on the exact operands of tests/gemm_cases.py that the prefill tests of tests/test_gemm_exact_gpu.py use.  Both kernels walk K in the
    same order with exact block sums, so equality is the requirement, not a tolerance;
  * against the fp64 product of the two fake-quantised operands (the check of test_gpu_parity.py::test_packed_consumer_prefill_mx8,
    its tolerance) at a LLaMA-7B shape, independently of the image route;
  * memory: what a hold_image=False module holds after prefill forwards, from the formats (0.5 + 1/64 B per weight);
  * a small LLaMA packed with hold_image=False against the same model packed with hold_image=True.
"""

import pytest
import torch

import gemm_cases as G
import test_gemm_exact_gpu as E
from quantization_sparsity_interplay_amd import native, BFPConfig
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, pack_linear_layers

pytestmark = pytest.mark.gpu
DEV = E.DEV
DTS = E.DTS
L, ptr, stream = E.L, E.ptr, E.stream


def mx4w_call(x8, xs, codes, exps, bias, out, T, N, K, wm):
    native.check(L().bfpq_hbfp_linear_mx4w(ptr(x8), ptr(xs), ptr(codes), ptr(exps), ptr(bias), ptr(out), T, N, K,
                                           native.DTYPE_CODE[out.dtype], wm, stream()), "bfpq_hbfp_linear_mx4w")


def mx4w_splitk_call(x8, xs, codes, exps, bias, out, slabs, parts, T, N, K, wm):
    native.check(L().bfpq_hbfp_linear_mx4w_splitk(ptr(x8), ptr(xs), ptr(codes), ptr(exps), ptr(bias), ptr(out), ptr(slabs), parts, T, N, K,
                                                  native.DTYPE_CODE[out.dtype], wm, stream()), "bfpq_hbfp_linear_mx4w_splitk")


def packed(wc, we):
    """the canonical packed tensor of exact codes: nibbles as bfpq_quantize_nm writes them, int8 exponents"""
    return G.pack4(wc).contiguous(), we.to(torch.int8).contiguous()


def same_bits(got, ref, what):
    """torch.equal on the raw bits of every output (so NaN sits where NaN sits)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    a, b = got.contiguous().view(it), ref.contiguous().view(it)
    if not torch.equal(a, b):
        bad = a != b
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs differ from the image route; first at {idx}: "
                             f"got {float(got[tuple(idx)])!r} image route {float(ref[tuple(idx)])!r}")
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what


def special_blocks(wc, we):
    """a zero block, a NaN block (exponent -128) and a block scaled by 4096 in the weight, where its shape has room for them"""
    N, K = wc.shape
    wc[0, :64] = 0
    we[N // 2, (K // 64) - 1] = -128
    we[N - 1, (K // 64) // 2] += 12
    return wc, we


def test_codes_route_every_variant_equals_image_route():
    """the shapes of test_prefill_every_variant_bit_exact x every tile variant, both epilogues, bias on / off, N:M weights, every output
    dtype, with a zero block, a NaN block and a block scaled by 4096 in every weight; also checked against the exact product where it
    is finite"""
    nms = [(0, 0), (2, 4), (1, 4), (4, 8)]
    try:
        for i, (T, N, K) in enumerate(E.SHAPES):
            dt = DTS[i % 3]
            xc, xe = E.operand(T, K, 3, 0, 3, seed=10 + i)
            wc, we = E.w_operand(N, K, 3, 3, seed=50 + i, nm=nms[i % 4])
            bias, bq = E.make_bias(N, xe, we, 3, 3, dt, seed=90 + i) if i % 2 else (None, None)
            want = E.exact_want(xc, xe, 3, wc, we, 3, bq, bias, what=f"shape {T, N, K}").float().to(dt)
            x8, xs = E.x_image(xc, xe, 3)
            codes, exps = packed(wc, we)
            wcs, wes = special_blocks(wc.clone(), we.clone())
            codes_s, exps_s = packed(wcs, wes)
            w8s, wss = native.mx8_from_hbfp(codes_s, exps_s, K, 3, 4)
            for v in range(7):
                assert L().bfpq_tune(E.TUNE_MX8_VARIANT, v) == 0
                out = torch.empty((T, N), dtype=dt, device=DEV)
                mx4w_call(x8, xs, codes, exps, bias, out, T, N, K, 3)
                E.assert_bits(out, want, f"variant {v} shape {T, N, K} {dt}")
                ref = torch.empty((T, N), dtype=dt, device=DEV)
                E.mx8_call(x8, xs, w8s, wss, bias, ref, T, N, K)
                out = torch.empty((T, N), dtype=dt, device=DEV)
                mx4w_call(x8, xs, codes_s, exps_s, bias, out, T, N, K, 3)
                same_bits(out, ref, f"variant {v} shape {T, N, K} {dt}, special blocks")
                assert bool(torch.isnan(out[:, N // 2]).all()), "the NaN block's column"
                buf = torch.full((T * N + 2,), 3.0, dtype=dt, device=DEV)         # out one element in: the lane-by-lane epilogue
                mx4w_call(x8, xs, codes_s, exps_s, bias, buf[1:1 + T * N], T, N, K, 3)
                same_bits(buf[1:1 + T * N].view(T, N), ref, f"variant {v} shape {T, N, K} {dt}, unaligned out")
                assert float(buf[0]) == 3.0 and float(buf[-1]) == 3.0, "write outside out"
    finally:
        L().bfpq_tune(E.TUNE_MX8_VARIANT, -1)


def test_codes_route_mixed_launch_ragged_seam():
    """variant 5 and the chosen plan at T = 4096, N = 4100, K = 256 (test_prefill_mixed_launch_ragged_seam)"""
    T, N, K = 4096, 4100, 256
    xc, xe = E.operand(T, K, 3, 0, 3, seed=3)
    wc, we = E.w_operand(N, K, 3, 3, seed=4, nm=(2, 4))
    bias, bq = E.make_bias(N, xe, we, 3, 3, torch.bfloat16, seed=5)
    want = E.exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="mixed").float().to(torch.bfloat16)
    x8, xs = E.x_image(xc, xe, 3)
    codes, exps = packed(wc, we)
    w8, ws = native.mx8_from_hbfp(codes, exps, K, 3, 4)
    try:
        for v in (5, -1):
            assert L().bfpq_tune(E.TUNE_MX8_VARIANT, v) == 0
            out = torch.empty((T, N), dtype=torch.bfloat16, device=DEV)
            mx4w_call(x8, xs, codes, exps, bias, out, T, N, K, 3)
            E.assert_bits(out, want, f"variant {v}")
            ref = torch.empty_like(out)
            E.mx8_call(x8, xs, w8, ws, bias, ref, T, N, K)
            same_bits(out, ref, f"variant {v}")
    finally:
        L().bfpq_tune(E.TUNE_MX8_VARIANT, -1)


@pytest.mark.parametrize("T,N,K", [(100, 256, 1280), (33, 136, 11008)])
def test_codes_route_split_k_equals_image_route(T, N, K):
    """bfpq_hbfp_linear_mx4w_splitk with parts 2, 3, 5, 8, 64, bias on and off, every output dtype (test_prefill_split_k_bit_exact), the
    weight with a zero block, a NaN block and a block scaled by 4096"""
    xc, xe = E.operand(T, K, 3, 0, 3, seed=21)
    wc, we = E.w_operand(N, K, 3, 3, seed=22, nm=(2, 4))
    x8, xs = E.x_image(xc, xe, 3)
    codes, exps = packed(wc, we)
    codes_s, exps_s = packed(*special_blocks(wc.clone(), we.clone()))
    w8s, wss = native.mx8_from_hbfp(codes_s, exps_s, K, 3, 4)
    slabs = torch.empty((64, T, N), dtype=torch.float32, device=DEV)
    for dt in DTS:
        for with_bias in (False, True):
            bias, bq = E.make_bias(N, xe, we, 3, 3, dt, seed=23) if with_bias else (None, None)
            want = E.exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="split-K").float().to(dt)
            for parts in (2, 3, 5, 8, 64):
                out = torch.empty((T, N), dtype=dt, device=DEV)
                mx4w_splitk_call(x8, xs, codes, exps, bias, out, slabs, parts, T, N, K, 3)
                E.assert_bits(out, want, f"parts {parts} {dt} bias {with_bias}")
                ref = torch.empty((T, N), dtype=dt, device=DEV)
                E.splitk_call(x8, xs, w8s, wss, bias, ref, slabs, parts, T, N, K)
                mx4w_splitk_call(x8, xs, codes_s, exps_s, bias, out, slabs, parts, T, N, K, 3)
                same_bits(out, ref, f"parts {parts} {dt} bias {with_bias}, special blocks")


def test_codes_route_split_k_switch():
    """hbfp_linear_mx4w from a tensor with native.SPLIT_K on and off (test_prefill_split_k_switch_is_bit_identical), against
    hbfp_linear_mx8 on the image under the same switch"""
    T, N, K = 100, 512, 4096
    assert L().bfpq_hbfp_linear_mx4w_parts(T, N, K) > 1
    xc, xe = E.operand(T, K, 3, 0, 3, seed=31)
    wc, we = E.w_operand(N, K, 3, 3, seed=32)
    x = G.values(xc, xe, 3).to(torch.bfloat16)
    bias, bq = E.make_bias(N, xe, we, 3, 3, torch.bfloat16, seed=33)
    want = E.exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="switch").float().to(torch.bfloat16)
    codes, exps = packed(wc, we)
    w8, ws = native.mx8_from_hbfp(codes, exps, K, 3, 4)
    native.forget_shared_images()
    for on in (True, False):
        try:
            native.SPLIT_K = on
            got = native.hbfp_linear_mx4w(x, codes, exps, 3, 3, bias=bias)
            ref = native.hbfp_linear_mx8(x, w8, ws, 3, bias=bias)
        finally:
            native.SPLIT_K = True
        E.assert_bits(got, want, f"split {on}")
        same_bits(got, ref, f"split {on}")


def test_codes_route_mantissa_widths():
    """weight mantissas 1..3 with activation mantissas 3 and 4 (and 1, 2), N:M weights, every output dtype
    (test_prefill_mantissa_widths_and_code_widths)"""
    T, N, K = 129, 264, 768
    nms = [(0, 0), (2, 4), (1, 4), (4, 8)]
    i = 0
    for wm in (1, 2, 3):
        for xm in (1, 2, 3, 4):
            i += 1
            xc, xe = E.operand(T, K, xm, 0, 3, seed=100 + i)
            wc, we = E.w_operand(N, K, wm, 3, seed=200 + i, nm=nms[i % 4])
            dt = DTS[i % 3]
            want = E.exact_want(xc, xe, xm, wc, we, wm, what=f"wm {wm} xm {xm}").float().to(dt)
            x8, xs = E.x_image(xc, xe, xm)
            codes, exps = packed(wc, we)
            out = torch.empty((T, N), dtype=dt, device=DEV)
            mx4w_call(x8, xs, codes, exps, None, out, T, N, K, wm)
            E.assert_bits(out, want, f"wm {wm} xm {xm}")
            codes_s, exps_s = packed(*special_blocks(wc.clone(), we.clone()))
            ref = torch.empty_like(out)
            E.mx8_call(x8, xs, *native.mx8_from_hbfp(codes_s, exps_s, K, wm, 4), None, ref, T, N, K)
            mx4w_call(x8, xs, codes_s, exps_s, None, out, T, N, K, wm)
            same_bits(out, ref, f"wm {wm} xm {xm}, special blocks")


def test_codes_route_every_nibble_and_fp16_overflow():
    """all 16 nibble values (the code -8, which the quantizer never writes, included) against the image route, and sums beyond
    65504 in fp16 (test_fp16_overflow_is_inf_as_torch_casts_it)"""
    T, N, K = 16, 256, 1280
    xc, xe = E.operand(T, K, 3, 6, 3, seed=41)
    wc, we = E.w_operand(N, K, 3, 3, seed=42, e0=4)
    want = E.exact_want(xc, xe, 3, wc, we, 3, what="overflow").float().to(torch.float16)
    x8, xs = E.x_image(xc, xe, 3)
    codes, exps = packed(wc, we)
    out = torch.empty((T, N), dtype=torch.float16, device=DEV)
    mx4w_call(x8, xs, codes, exps, None, out, T, N, K, 3)
    E.assert_bits(out, want, "overflow")
    slabs = torch.empty((8, T, N), dtype=torch.float32, device=DEV)
    mx4w_splitk_call(x8, xs, codes, exps, None, out, slabs, 3, T, N, K, 3)
    E.assert_bits(out, want, "overflow, split-K")
    g = torch.Generator(device=DEV).manual_seed(43)
    raw = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    assert sorted(set((raw & 15).flatten().tolist())) == list(range(16))
    ref = torch.empty((T, N), dtype=torch.float32, device=DEV)
    E.mx8_call(x8, xs, *native.mx8_from_hbfp(raw, exps, K, 3, 4), None, ref, T, N, K)
    out = torch.empty((T, N), dtype=torch.float32, device=DEV)
    mx4w_call(x8, xs, raw, exps, None, out, T, N, K, 3)
    same_bits(out, ref, "every nibble")


def _cfg(**kw):
    base = dict(mant_bits=3, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _synth(rows, cols, dt, scale=0.02, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(dt)


def test_codes_route_against_the_fake_quantised_product():
    """LLaMA-7B gate_proj, 2048 tokens: the fp64 product of the two fake-quantised operands, with the tolerances of
    test_gpu_parity.py::test_packed_consumer_prefill_mx8 (2e-6 of the largest output in fp32; per element the fp32 summation bound),
    HBFP4 and HBFP5 activations, a zero block and a block on a very different scale in x"""
    T, N, K, dt = 2048, 11008, 4096, torch.bfloat16
    w = _synth(N, K, dt).to(DEV)
    x = _synth(T, K, dt, 1.0, seed=9).to(DEV)
    x[0, :64] = 0
    x[T - 1, 64:128] *= 4096
    pw = bfp_ops.PackedBFP.quantize(w, 3, 64, N=2, M=4)
    wq = pw.dequantize().double()
    for xm in (3, 4):
        assert native.hbfp_linear_mx4w_ok(T, N, K, 3, xm)
        xq = bfp_ops.float_to_bfp_blocked(x, **_cfg(mant_bits=xm), identifier='in').double()
        want = xq @ wq.t()
        native.forget_shared_images()
        got32 = native.hbfp_linear_mx4w(x, pw.codes, pw.exps, 3, xm, out_dtype=torch.float32)
        assert got32.shape == (T, N)
        g = got32.double()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(g), nan) and not bool(nan.any())
        err32 = (g - want)[~nan].abs().max() / want[~nan].abs().max()
        print(f"x_mant_bits {xm}: max error / max output = {float(err32):.3g}")
        assert float(err32) < 2e-6, (xm, float(err32))
        G.elementwise_bound(g, want, xq.abs() @ wq.abs().t(), K // 64 + 8, torch.float32)
    assert getattr(pw, "_mx8", None) is None


def test_lean_module_holds_codes_and_exponents_only():
    """[11008, 4096] bf16, HBFP4 2:4: after a 2048-token and a 128-token (split-K) forward a hold_image=False module holds
    N K / 2 + N K / 64 bytes and the allocator is back where it was; the default module holds the image on top (N K + N K / 64);
    a 16-token forward adds the decode kernel's tiled copy (another N K / 2 + N K / 64) to both.  The numbers follow from the
    formats: 4-bit codes, one int8 exponent per 64, e4m3 bytes + one E8M0 byte per 64."""
    N, K, dt = 11008, 4096, torch.bfloat16
    cfg = BFPConfig.hbfp(4, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
    cfg['rounding_mode'] = 'determ'
    lin = torch.nn.Linear(K, N, bias=False, dtype=dt, device=DEV)
    lean = PackedBFPLinear.from_linear(lin, cfg, hold_image=False)
    held = PackedBFPLinear.from_linear(lin, cfg)
    del lin
    base = N * K // 2 + N * K // 64
    assert L().bfpq_hbfp_linear_mx4w_parts(128, N, K) > 1
    x_long, x_short, x_dec = (_synth(T, K, dt, 1.0, seed=T).to(DEV) for T in (2048, 128, 16))
    outs = {}
    for name, mod in (("lean", lean), ("held", held)):
        native.forget_shared_images()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            y_long, y_short = mod(x_long), mod(x_short)
        outs[name] = (y_long.clone(), y_short.clone())
        del y_long, y_short
        native.forget_shared_images()
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated() - 2 * (2048 + 128) * N        # (the two clones kept for the comparison below)
        p = mod.packed
        if name == "lean":
            assert getattr(p, "_mx8", None) is None and getattr(p, "_tiles", None) is None
            assert p.resident_bytes() == base
            assert after == before, (after, before)
        else:
            assert p.resident_bytes() == base + N * K + N * K // 64
    same_bits(outs["lean"][0], outs["held"][0], "2048 tokens")
    same_bits(outs["lean"][1], outs["held"][1], "128 tokens (split-K)")
    for mod, want in ((lean, 2 * base), (held, 2 * base + N * K + N * K // 64)):
        with torch.no_grad():
            mod(x_dec)
        assert mod.packed.resident_bytes() == want
    assert getattr(lean.packed, "_mx8", None) is None
    assert "hold_image=False" in repr(lean) and f"resident_bytes={2 * base}" in repr(lean)


def test_lean_packed_model_equals_packed_model():
    """the small LLaMA of test_model_integration.py::test_packed_inference_model_matches_fake_quantised_model packed with
    hold_image=False: logits equal, bit for bit, those of the same model packed with hold_image=True (decode-sized and prefill-sized
    inputs), no module makes an image, and state_dict() carries the switch"""
    import copy
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=1000, max_position_embeddings=64)
    base = LlamaForCausalLM(cfg).to(torch.float32).eval()
    bfp_args = BFPConfig.hbfp(4, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
    bfp_args['rounding_mode'] = 'determ'
    model, lean, again = copy.deepcopy(base).to(DEV), copy.deepcopy(base).to(DEV), copy.deepcopy(base).to(DEV)
    names, saved = pack_linear_layers(model, bfp_args)
    names_l, saved_l = pack_linear_layers(lean, bfp_args, hold_image=False)
    assert names_l == names and saved_l == saved and len(names) == 14
    ids = torch.randint(0, 1000, (2, 48), generator=torch.Generator().manual_seed(5)).to(DEV)
    for batch in (ids, ids[:1, :12]):                                      # 96 tokens (prefill kernel) and 12 tokens (decode kernel)
        native.forget_shared_images()
        with torch.no_grad():
            a = model(batch).logits
            native.forget_shared_images()
            b = lean(batch).logits
        same_bits(b, a, f"logits, {batch.numel()} tokens")
    mods = [m for m in lean.modules() if isinstance(m, PackedBFPLinear)]
    assert len(mods) == 14 and all(not m.hold_image and getattr(m.packed, "_mx8", None) is None for m in mods)
    assert any(getattr(m.packed, "_mx8", None) is not None for m in model.modules() if isinstance(m, PackedBFPLinear))
    pack_linear_layers(again, bfp_args)                                     # (hold_image=True modules: the state dict must flip them)
    again.load_state_dict(lean.state_dict())
    assert all(not m.hold_image for m in again.modules() if isinstance(m, PackedBFPLinear))
    native.forget_shared_images()
    with torch.no_grad():
        c = again(ids).logits
        native.forget_shared_images()
        b = lean(ids).logits
    same_bits(c, b, "after the state_dict round trip")
