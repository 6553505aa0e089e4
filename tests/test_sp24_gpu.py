"""The 2:4-compressed packed weight on an MI355X (run with `-m gpu`): the device pack against the torch restatement (tests/sp24_ref.py),
the sparse-instruction product bit for bit on certified exact operands (tests/gemm_cases.py, drivers of tests/test_i8gemm_gpu.py),
NaN blocks, the fp32 summation bound at LLaMA-7B shapes, and Sparse24BFPLinear against the dense PackedBFPLinear."""
import copy
import ctypes

import pytest
import torch

import gemm_cases as G
import sp24_ref as S
from test_i8gemm_gpu import certified, expected, assert_bits, i8, run_c
import quantization_sparsity_interplay_amd as pkg
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, Sparse24BFPLinear, pack_linear_layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def to_sp24(wc, N, K, code_bits):
    """int codes [N, K] -> device sp24 (vals, idx) by bfpq_sp24_pack"""
    return native.sp24_pack(S.dense_bytes(wc.cpu().long(), code_bits).to(DEV), N, K, code_bits)


def run_sp24(xc, xe, vals, idx, we, bias, T, N, K, code_bits, dt, wm, xm):
    L = native.load_library()
    out = torch.empty((T, N), dtype=dt, device=DEV)
    slabs = torch.empty(int(L.bfpq_hbfp_linear_sp24_ws(T, N, K)), dtype=torch.float32, device=DEV)
    xc8, xe8, we8 = i8(xc), i8(xe), i8(we)                              # (held until the call returns)
    rc = L.bfpq_hbfp_linear_sp24(ptr(xc8), ptr(xe8), ptr(vals), ptr(idx), ptr(we8), ptr(bias), ptr(out), ptr(slabs), T, N, K,
                                 code_bits, DT_CODE[dt], wm, xm, stream())
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("code_bits", (4, 8))
@pytest.mark.parametrize("n", (1, 2))
def test_device_pack_matches_restatement(code_bits, n):
    for N, K in ((16, 64), (48, 576), (144, 320), (64, 4096 + 64), (4096, 11008)):
        c = S.random_nm(N, K, n, code_bits, seed=N + K + n)
        vals, idx = native.sp24_pack(S.dense_bytes(c, code_bits).to(DEV), N, K, code_bits)
        hv, hi = S.pack(c, code_bits)
        assert torch.equal(vals.cpu(), hv) and torch.equal(idx.cpu(), hi), (N, K)
        back, back8 = native.sp24_unpack(vals, idx, N, K, code_bits, codes=True, codes8=True)
        assert torch.equal(back.cpu(), S.dense_bytes(c, code_bits)), (N, K)
        assert torch.equal(back8.cpu().long(), c), (N, K)


@pytest.mark.parametrize("code_bits", (4, 8))
def test_three_non_zeros_raise(code_bits):
    c = S.random_nm(32, 256, 2, code_bits, seed=3)
    c[5, 8:12] = torch.tensor([1, -1, 1, 0])
    with pytest.raises(ValueError):
        native.sp24_pack(S.dense_bytes(c, code_bits).to(DEV), 32, 256, code_bits)


def _exact_case(T, N, K, nm, cb, wm, xm, dts, seed, with_bias):
    xc, xe, wc, we, bias = certified(T, N, K, xm, wm, seed, nm=nm, with_bias=with_bias)
    vals, idx = to_sp24(wc, N, K, cb)
    for dt in dts:
        want = expected(xc, xe, xm, wc, we, wm, bias, dt)
        b = None if bias is None else bias.to(dt)
        what = f"T {T} N {N} K {K} nm {nm} cb {cb} wm {wm} xm {xm} {dt} bias {with_bias}"
        got = run_sp24(xc, xe, vals, idx, we, b, T, N, K, cb, dt, wm, xm)
        assert_bits(got, want, what)
        xq8 = (i8(xc), i8(xe), i8(wc), i8(we))
        assert_bits(got, run_c('decode8', *xq8, b, T, N, K, dt, wm, xm), what + " vs hbfp_linear_i8")
        got = native.hbfp_linear_sp24(torch.empty((T, K), dtype=dt, device=DEV), vals, idx, i8(we), N, cb, wm, xm, bias=b, out_dtype=dt,
                                      xq=(i8(xc), i8(xe)))
        assert_bits(got, want, what + " wrapper")


@pytest.mark.parametrize("nm", ((2, 4), (1, 4)))
@pytest.mark.parametrize("cb,wm", ((4, 1), (4, 3), (8, 4), (8, 5), (8, 7)))
def test_exact_widths(nm, cb, wm):
    for i, xm in enumerate((1, 3, 5, 7)):
        _exact_case(17, 144, 320, nm, cb, wm, xm, (torch.float32, torch.bfloat16, torch.float16), seed=11 * wm + xm, with_bias=i % 2 == 1)


@pytest.mark.parametrize("T", (1, 2, 15, 16, 17, 33, 63, 64))
def test_exact_tokens(T):
    for j, (N, K) in enumerate(((16, 256), (144, 320), (4096, 4096), (16, 11008))):
        cb, wm, xm = ((4, 3, 5), (8, 7, 7), (8, 5, 3), (4, 1, 7))[j]
        _exact_case(T, N, K, (2, 4) if j % 2 == 0 else (1, 4), cb, wm, xm, (torch.float32, torch.bfloat16), seed=T * 13 + j, with_bias=T % 2 == 0)


def test_nan_blocks():
    N, K = 64, 512
    for cb, wm in ((4, 3), (8, 7)):
        for T in (3, 40):
            xc, xe, wc, we, _ = certified(T, N, K, 7, wm, seed=77, nm=(2, 4))
            xe, we = xe.clone(), we.clone()
            xe[1, 2] = -128                                                    # token 1: every output NaN
            we[5, 7] = -128                                                    # feature 5: every output NaN
            want = expected(xc, xe.clamp_min(-127), 7, wc, we.clamp_min(-127), wm, None, torch.float32)
            want[1, :] = float("nan")
            want[:, 5] = float("nan")
            vals, idx = to_sp24(wc, N, K, cb)
            assert_bits(run_sp24(xc, xe, vals, idx, we, None, T, N, K, cb, torch.float32, wm, 7), want, f"NaN cb {cb} T {T}")


@pytest.mark.parametrize("shape", ((4096, 4096), (11008, 4096), (4096, 11008)))
@pytest.mark.parametrize("m", (3, 7))
def test_random_llama_shapes(shape, m):
    N, K = shape
    g = torch.Generator(device=DEV).manual_seed(N + K + m)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    cb = bfp_ops.code_bits_for(m)
    p = bfp_ops.PackedBFP.quantize(w, m, 64, N=2, M=4)
    sp = bfp_ops.SparseBFP24.from_packed(p)
    wv = G.values(native.sp24_unpack(sp.vals, sp.idx, N, K, cb, codes=False, codes8=True).int(), p.exps.int(), m)
    for T in (1, 16, 64):
        x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
        xc, xe = native.act_codes(x, 7, 1e-8, None)
        xv = G.values(xc.int(), xe.int(), 7)
        want = xv @ wv.t()
        got = native.hbfp_linear_sp24(x, sp.vals, sp.idx, sp.exps, N, cb, m, 7, out_dtype=torch.float32)
        G.elementwise_bound(got, want, xv.abs() @ wv.abs().t(), K // 64 + K // 512 + 2, torch.float32)


def _lin(N, K, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N).to(DEV).to(dtype)
    with torch.no_grad():
        lin.weight.mul_(4.0)
    return lin


def _cfg(bits, nm=(2, 4), first='s', **kw):
    a = pkg.BFPConfig.hbfp(bits, 64, w_sparsity=True, N=nm[0], M=nm[1], sparsity_mode='structured', first=first, **kw).to_kwargs()
    a['rounding_mode'] = 'determ'
    return a


@pytest.mark.parametrize("bits", (4, 8))
@pytest.mark.parametrize("nm", ((2, 4), (1, 4)))
def test_module_against_dense_packed(bits, nm):
    N, K = 512, 1024
    lin = _lin(N, K)
    a = _cfg(bits, nm)
    dense, sparse = PackedBFPLinear.from_linear(lin, a), Sparse24BFPLinear.from_linear(lin, a)
    assert torch.equal(sparse.sparse.to_packed().codes, dense.codes)
    assert sparse.sparse.nbytes() == S.nbytes(N, K, dense.packed.code_bits)
    g = torch.Generator(device=DEV).manual_seed(bits)
    with torch.no_grad():
        for T in (65, 200, 512, 2048):                                          # above SP24_DECODE_TOKENS: the same kernel, the same operand
            x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
            assert torch.equal(sparse(x), dense(x)), T
        for T in (1, 7, 16, 64):
            x = torch.randn(2, T, K, generator=g, device=DEV).to(torch.bfloat16)[0]
            got, want = sparse(x).float(), dense(x).float()
            err = float((got - want).abs().max() / want.abs().max())
            assert err < 1e-2, (T, err)                                         # bf16 outputs, fp32 summation order differs


@pytest.mark.parametrize("act", (dict(in_sparsity=True), dict(in_sparsity=True, first='q'),
                                 dict(in_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, in_only=True)))
def test_module_pruned_activations(act):
    act = dict(act)
    N, K = 256, 512
    lin = _lin(N, K, seed=3)
    if act.pop('in_only', False):
        # unstructured activation pruning with a 2:4 weight: the weight keys of one config cannot say both, so the module's activation
        # spec is set directly (as PackedBFPLinear's x_sparsity)
        a = _cfg(4)
        dense, sparse = PackedBFPLinear.from_linear(lin, a), Sparse24BFPLinear.from_linear(lin, a)
        for first in ('s', 'q'):
            spec = native.ActSparsity('unstructured', 0, 0, 0.5, first)
            dense.x_sparsity = sparse.x_sparsity = spec
            _compare(dense, sparse, K)
        return
    a = _cfg(4, first=act.pop('first', 's'), **act)
    dense, sparse = PackedBFPLinear.from_linear(lin, a), Sparse24BFPLinear.from_linear(lin, a)
    assert sparse.x_sparsity is not None and sparse.x_sparsity == dense.x_sparsity
    _compare(dense, sparse, K)


def _compare(dense, sparse, K):
    g = torch.Generator(device=DEV).manual_seed(9)
    with torch.no_grad():
        for T in (5, 64, 300):
            x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
            got, want = sparse(x).float(), dense(x).float()
            if T > bfp_ops.SP24_DECODE_TOKENS:
                assert torch.equal(got, want), T
            else:
                assert float((got - want).abs().max() / want.abs().max()) < 1e-2, T


def test_module_state_dict_to_and_files(tmp_path):
    N, K = 256, 512
    lin = _lin(N, K, seed=5)
    a = _cfg(4)
    m = Sparse24BFPLinear.from_linear(lin, a)
    x = torch.randn(9, K, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        ref = m(x)
        fresh = Sparse24BFPLinear.from_linear(_lin(N, K, seed=6), a)
        fresh.load_state_dict(m.state_dict())
        assert torch.equal(fresh(x), ref)
        moved = copy.deepcopy(m).to("cpu")
        assert moved.vals.device.type == "cpu" and moved.idx.device.type == "cpu"
        moved.to(DEV)
        assert torch.equal(moved(x), ref)
        sp = m.sparse
        sp.save(str(tmp_path / "w.safetensors"))
        back = bfp_ops.SparseBFP24.load(str(tmp_path / "w.safetensors"), DEV)
        assert torch.equal(back.vals, sp.vals) and torch.equal(back.idx, sp.idx) and torch.equal(back.exps, sp.exps)
        dense = PackedBFPLinear.from_linear(lin, a).packed
        dense.save(str(tmp_path / "c24.safetensors"), compact24=True)
        back = bfp_ops.SparseBFP24.load(str(tmp_path / "c24.safetensors"), DEV)
        assert torch.equal(back.vals, sp.vals) and torch.equal(back.idx, sp.idx) and torch.equal(back.exps, sp.exps)
        assert sorted(k for k, v in vars(back).items() if isinstance(v, torch.Tensor)) == ["exps", "idx", "vals"]
        assert torch.equal(back.linear(x, lin.bias, 3), ref)


def test_no_dense_operand_after_prefill():
    N, K = 512, 1024
    for bits in (4, 8):
        m = Sparse24BFPLinear.from_linear(_lin(N, K, seed=bits), _cfg(bits))
        with torch.no_grad():
            m(torch.randn(2048, K, device=DEV).to(torch.bfloat16))
        sp = m.sparse
        held = {k for k, v in vars(sp).items() if isinstance(v, (torch.Tensor, tuple))}
        assert held == {"vals", "idx", "exps", "shape"}, held
        assert {k for k, _ in m.named_buffers()} == {"vals", "idx", "exps"}


@pytest.mark.parametrize("bits", (4, 8))
def test_graph_capture(bits):
    N, K = 512, 1024
    m = Sparse24BFPLinear.from_linear(_lin(N, K, seed=7), _cfg(bits))
    for T in (1, 512):
        x = torch.randn(T, K, device=DEV).to(torch.bfloat16)
        with torch.no_grad():
            want = m(x)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                m(x)                                                           # warm-up on the side stream
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = m(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), T


def test_tiny_llama_sparse24():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=1000, max_position_embeddings=64)
    base = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    for bits in (4, 8):
        args = _cfg(bits)
        dense, sparse = copy.deepcopy(base).to(DEV), copy.deepcopy(base).to(DEV)
        pack_linear_layers(dense, args)
        names, saved = pack_linear_layers(sparse, args, sparse24=True)
        assert len(names) == 2 * 7 and type(sparse.lm_head) is torch.nn.Linear
        mods = [m for m in sparse.modules() if isinstance(m, Sparse24BFPLinear)]
        cb = bfp_ops.code_bits_for(bits - 1)
        want = sum(m.in_features * m.out_features * 2 - S.nbytes(m.out_features, m.in_features, cb) for m in mods)
        assert saved == want
        for shape in ((1, 12), (2, 48)):
            tokens = torch.randint(0, 1000, shape, generator=torch.Generator().manual_seed(5)).to(DEV)
            with torch.no_grad():
                a, b = dense(tokens).logits.float(), sparse(tokens).logits.float()
            err = float((a - b).abs().max() / a.abs().max())
            assert err < 2e-2, (bits, shape, err)
