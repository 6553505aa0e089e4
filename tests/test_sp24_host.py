"""The 2:4-compressed packed weight (format sp24, csrc/bfpq_sp24.hip) without a GPU: the layout restated in torch (tests/sp24_ref.py),
its byte counts, which configurations may take it, the token route of SparseBFP24.linear, and the C entries' argument checks."""
import ctypes

import pytest
import torch

import sp24_ref as S
import quantization_sparsity_interplay_amd as pkg
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import Sparse24BFPLinear, pack_linear_layers

SHAPES = ((16, 64), (32, 192), (48, 576), (16, 640), (64, 4096 + 64))


@pytest.mark.parametrize("code_bits", (4, 8))
@pytest.mark.parametrize("n", (1, 2))
def test_layout_round_trip(code_bits, n):
    for N, K in SHAPES:
        c = S.random_nm(N, K, n, code_bits, seed=N * 7 + K + n + code_bits)
        vals, idx = S.pack(c, code_bits)
        assert torch.equal(S.unpack(vals, idx, N, K, code_bits), c), (N, K)


def test_kept_positions_are_distinct_ascending():
    c = torch.tensor([[0, 0, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, 0, 2, 0, -1] * 4])
    v, p, cnt = S.keep2(c)
    assert p[0, :8].tolist() == [0, 1, 0, 2, 0, 1, 1, 3]
    assert v[0, :8].tolist() == [0, 0, 0, 5, 3, 0, 2, -1]
    assert bool((p[:, 0::2] < p[:, 1::2]).all())


@pytest.mark.parametrize("code_bits,per_weight", ((4, 0.25 + 0.125 + 1 / 64), (8, 0.5 + 0.125 + 1 / 64)))
def test_byte_counts(code_bits, per_weight):
    for N, K in SHAPES + ((4096, 4096), (11008, 4096), (4096, 11008)):
        nv, ni = native.sp24_nbytes(N, K, code_bits)
        vals, idx = S.pack(torch.zeros(N, K, dtype=torch.int64), code_bits) if N * K <= 1 << 18 else (None, None)
        if vals is not None:
            assert (vals.numel(), idx.numel()) == (nv, ni)
        assert nv + ni + N * K // 64 == S.nbytes(N, K, code_bits) == N * K * per_weight
    # LLaMA-7B's Linear weights (6.48 G): 2.53 GB (HBFP4) / 4.15 GB (HBFP8)
    n7b = 32 * (4 * 4096 * 4096 + 3 * 4096 * 11008)
    assert round(n7b * (0.25 + 0.125 + 1 / 64) / 1e9, 2) == 2.53 and round(n7b * (0.5 + 0.125 + 1 / 64) / 1e9, 2) == 4.15


def _args(**kw):
    base = dict(w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s')
    base.update(kw)
    bits = base.pop('bits', 4)
    block = base.pop('block', 64)
    a = pkg.BFPConfig.hbfp(bits, block, **base).to_kwargs()
    a['rounding_mode'] = base.get('rounding_mode', 'determ')
    return a


REFUSED = {
    "4:8": dict(N=4, M=8),
    "3:4": dict(N=3, M=4),
    "unstructured": dict(sparsity_mode='unstructured', sparsity_frac=0.5),
    "block 32": dict(block=32),
    "stoc": dict(rounding_mode='stoc'),
    "dense": dict(w_sparsity=False),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_configs_without_the_pattern_are_refused(name):
    a = bfp_ops.unpack_bfp_args(_args(**REFUSED[name]))
    with pytest.raises(ValueError):
        bfp_ops.SparseBFP24.from_bfp_args(torch.zeros(64, 256), a)
    model = torch.nn.Sequential(torch.nn.Linear(256, 64), torch.nn.Linear(64, 32))
    with pytest.raises(ValueError):
        pack_linear_layers(model, _args(**REFUSED[name]), sparse24=True)
    assert all(type(m) is torch.nn.Linear for m in model)                   # nothing was replaced


@pytest.mark.parametrize("first", ('s', 'q'))
@pytest.mark.parametrize("nm", ((2, 4), (1, 4)))
@pytest.mark.parametrize("bits", (4, 8))
def test_configs_with_the_pattern_are_taken(first, nm, bits):
    bfp_ops.sp24_config_check(bfp_ops.unpack_bfp_args(_args(N=nm[0], M=nm[1], first=first, bits=bits)))


class _Recorder:
    def __init__(self):
        self.calls = []


def _fake_sparse(code_bits=4, N=64, K=256):
    nv, ni = native.sp24_nbytes(N, K, code_bits)
    return bfp_ops.SparseBFP24(torch.zeros(nv, dtype=torch.uint8), torch.zeros(ni, dtype=torch.uint8), torch.zeros(N, K // 64, dtype=torch.int8),
                               (N, K), torch.bfloat16, 3 if code_bits == 4 else 5, code_bits)


@pytest.mark.parametrize("limit", (64, 16, 1))
def test_route_constant_is_honoured(monkeypatch, limit):
    rec = []
    monkeypatch.setattr(bfp_ops, "SP24_DECODE_TOKENS", limit)
    monkeypatch.setattr(native, "hbfp_linear_sp24_ok", lambda T, N, K, cb, wm, xm: 1 <= T <= 64)
    monkeypatch.setattr(native, "hbfp_linear_sp24", lambda x, *a, **k: rec.append(('sp24', x.shape[0])) or torch.zeros(x.shape[0], 64))
    monkeypatch.setattr(bfp_ops, "linear_route", lambda T, *a, **k: rec.append(('expand', T)) or 'empty')
    monkeypatch.setattr(bfp_ops.SparseBFP24, "to_packed", lambda self: bfp_ops.PackedBFP(None, None, self.shape, self.dtype, 3, 64, 4))
    sp = _fake_sparse()
    for T in (1, 2, 16, 17, 64, 65, 512):
        rec.clear()
        sp.linear(torch.zeros(T, 256, dtype=torch.bfloat16), x_mant_bits=3)
        assert rec[0] == (('sp24', T) if T <= limit else ('expand', T)), (T, rec)
    rec.clear()
    sp.linear(torch.zeros(8, 256, dtype=torch.bfloat16), x_mant_bits=3, decode_tokens=4)
    assert rec[0] == ('expand', 8)


def test_module_extra_state_round_trip_on_cpu_buffers():
    sp = _fake_sparse(8)
    m = Sparse24BFPLinear(sp, torch.zeros(64), x_mant_bits=5, x_sparsity=native.ActSparsity('structured', 2, 4, 0.0, 'q'))
    sd = m.state_dict()
    assert {"vals", "idx", "exps", "bias", "_extra_state"} <= set(sd)
    m2 = Sparse24BFPLinear(_fake_sparse(8), None)
    m2.bias = torch.nn.Parameter(torch.ones(64), requires_grad=False)
    m2.load_state_dict(sd)
    assert m2.x_mant_bits == 5 and tuple(m2.x_sparsity) == ('structured', 2, 4, 0.0, 'q')
    assert m2.sparse.code_bits == 8 and m2.sparse.mant_bits == 5 and m2.sparse.shape == (64, 256)


def test_argument_validation_without_gpu():
    L = pkg.load_library()
    n = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)               # a non-null, never dereferenced pointer: rejected before any launch
    odd = ctypes.c_void_p(17)
    BF16 = native.BF16
    # bfpq_hbfp_linear_sp24(xc, xe, vals, idx, we, bias, out, slabs, T, N, K, code_bits, dtype, wm, xm, stream)
    lin = L.bfpq_hbfp_linear_sp24
    assert lin(n, one, one, one, one, n, one, one, 4, 256, 1024, 4, BF16, 3, 7, n) == -1            # null activation codes
    assert lin(one, one, n, one, one, n, one, one, 4, 256, 1024, 4, BF16, 3, 7, n) == -1            # null values
    assert lin(one, one, one, n, one, n, one, one, 4, 256, 1024, 4, BF16, 3, 7, n) == -1            # null positions
    assert lin(one, one, one, one, one, n, one, n, 4, 256, 1024, 4, BF16, 3, 7, n) == -1            # null slabs
    assert lin(odd, one, one, one, one, n, one, one, 4, 256, 1024, 4, BF16, 3, 7, n) == -1          # codes not 16-byte aligned
    assert lin(one, one, odd, one, one, n, one, one, 4, 256, 1024, 4, BF16, 3, 7, n) == -1          # values not 16-byte aligned
    assert lin(one, one, one, one, one, n, one, one, 4, 100, 1024, 4, BF16, 3, 7, n) == -2          # N % 16 != 0
    assert lin(one, one, one, one, one, n, one, one, 4, 256, 1000, 4, BF16, 3, 7, n) == -2          # K % 64 != 0
    assert lin(one, one, one, one, one, n, one, one, 65, 256, 1024, 4, BF16, 3, 7, n) == -2         # more than 64 tokens
    assert lin(one, one, one, one, one, n, one, one, 4, 256, 1024, 6, BF16, 3, 7, n) == -1          # 6-bit codes
    assert lin(one, one, one, one, one, n, one, one, 4, 256, 1024, 4, BF16, 5, 7, n) == -1          # 5-bit mantissa in 4-bit codes
    for wm, xm in ((0, 7), (8, 7), (3, 0), (3, 8)):
        assert lin(one, one, one, one, one, n, one, one, 4, 256, 1024, 8, BF16, wm, xm, n) == -1    # mantissas outside 1..7
    assert lin(one, one, one, one, one, n, one, one, 4, 256, 1024, 4, 9, 3, 7, n) == -1            # bad dtype
    assert lin(one, one, one, one, one, n, one, one, 0, 256, 1024, 4, BF16, 3, 7, n) == -1         # no tokens
    assert L.bfpq_hbfp_linear_sp24_ws(1, 4096, 4096) > 0 and L.bfpq_hbfp_linear_sp24_ws(65, 4096, 4096) == -2
    assert L.bfpq_hbfp_linear_sp24_ws(1, 4096, 4000) == -2
    # bfpq_sp24_pack(codes, vals, idx, N, K, code_bits, status, stream) / bfpq_sp24_unpack(vals, idx, codes, codes8, N, K, code_bits, stream)
    assert L.bfpq_sp24_pack(one, one, one, 64, 256, 5, one, n) == -1                                 # 5-bit codes
    assert L.bfpq_sp24_pack(n, one, one, 64, 256, 4, one, n) == -1                                   # null codes
    assert L.bfpq_sp24_pack(one, one, one, 64, 256, 4, n, n) == -1                                   # null status
    assert L.bfpq_sp24_pack(one, odd, one, 64, 256, 4, one, n) == -1                                 # misaligned values
    assert L.bfpq_sp24_pack(one, one, one, 40, 256, 4, one, n) == -2                                 # N % 16 != 0
    assert L.bfpq_sp24_pack(one, one, one, 64, 200, 8, one, n) == -2                                 # K % 64 != 0
    assert L.bfpq_sp24_pack(one, one, one, 0, 256, 4, one, n) == 0                                   # empty: no launch
    assert L.bfpq_sp24_unpack(one, one, n, n, 64, 256, 4, n) == -1                                   # no output
    assert L.bfpq_sp24_unpack(one, one, odd, n, 64, 256, 4, n) == -1                                 # misaligned output
    assert L.bfpq_sp24_unpack(one, one, one, n, 64, 256, 3, n) == -1                                 # 3-bit codes
    assert L.bfpq_sp24_unpack(one, one, one, one, 64, 100, 8, n) == -2                               # K % 64 != 0
