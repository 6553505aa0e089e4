"""Host checks of the exact GEMM operands (tests/gemm_cases.py) that tests/test_gemm_exact_gpu.py compares bit for bit: they are
fixed points of the oracle quantizer, their block exponents really vary, and the exactness certificate holds for the cases used."""
import pytest
import torch

import gemm_cases as G
from oracle import oracle as O


def _cfg(m):
    return dict(mant_bits=m, epsilon=1e-8, rounding_mode='determ', device='cpu', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp',
                first='s', sparsity_mode='structured')


@pytest.mark.parametrize("dname", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("m,e0,spread,nm", [(2, -1, 3, (0, 0)), (3, -2, 3, (2, 4)), (3, 0, 2, (1, 4)), (4, 1, 3, (4, 8)),
                                            (5, 0, 3, (0, 0)), (7, 0, 2, (0, 0)), (7, 3, 3, (2, 4))])
def test_exact_operands_are_oracle_fixed_points(m, e0, spread, nm, dname):
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dname]
    c, e = G.hbfp_operand(45, 768, m, e0, spread, seed=11 + m, nm=nm)
    v = G.values(c, e, m)
    t = v.to(dt)
    assert torch.equal(t.double(), v), "values not representable in the dtype"
    q = O.float_to_bfp_blocked(t, **_cfg(m), identifier='w')
    assert torch.equal(q.double(), v), "not a fixed point of the oracle quantizer"
    _, oexp = O.no_sparsity_float_to_bfp(t, 64, m, 1e-8, return_exponents=True)
    assert torch.equal(oexp.to(torch.int32), e), "block exponents differ from the oracle's"
    if nm != (0, 0):                                              # N:M-pruning the operand changes nothing either
        qs = O.float_to_bfp_blocked(t, **dict(_cfg(m), w_sparsity=True, N=nm[0], M=nm[1]), identifier='w')
        assert torch.equal(qs.double(), v)
        assert int((c.view(45, -1, nm[1]) != 0).sum(-1).max()) <= nm[0]
    # every block holds a code of magnitude 2^m - 1, no code exceeds it
    assert int(c.abs().max()) == (1 << m) - 1
    assert bool((c.abs().view(45, 12, 64).amax(-1) == (1 << m) - 1).all())


def test_exponents_vary_over_rows_and_blocks():
    c, e = G.hbfp_operand(129, 4096, 3, -2, 3, seed=5)
    mode = int(e.flatten().mode().values)
    assert float((e != mode).float().mean()) > 0.3                # (randn data: ~90 % of blocks share one exponent)
    assert bool((e.max(1).values != e.min(1).values).all())       # every row has more than one exponent
    assert bool((e.max(0).values != e.min(0).values).all())       # every block column too
    # no period that lines up with a tile edge: shifting by 16, 32, 128 rows or 2, 4 blocks changes some exponents
    for s in (16, 32, 128):
        assert not torch.equal(e[s:], e[:-s])
    for s in (2, 4):
        assert not torch.equal(e[:, s:], e[:, :-s])


def test_pack4_is_the_packed_layout():
    c, e = G.hbfp_operand(16, 256, 3, 0, 3, seed=1)
    p = G.pack4(c)
    lo = (p & 0xF).to(torch.int32)
    hi = (p >> 4).to(torch.int32)
    assert torch.equal(torch.where(lo > 7, lo - 16, lo), c[:, 0::2])
    assert torch.equal(torch.where(hi > 7, hi - 16, hi), c[:, 1::2])


@pytest.mark.parametrize("T,N,K,xm,wm,xs,ws", [(16, 64, 11008, 7, 3, 2, 2), (16, 64, 11008, 5, 1, 2, 3), (64, 64, 11008, 3, 3, 3, 3),
                                                (64, 64, 4096, 4, 4, 3, 3), (33, 48, 1280, 7, 3, 3, 3)])
def test_certificate_holds_for_the_gpu_cases(T, N, K, xm, wm, xs, ws):
    """the widths / spreads the GPU tests use at their largest K stay in the exact regime, and a case that does not is refused"""
    xc, xe = G.hbfp_operand(T, K, xm, 0, xs, seed=1)
    wc, we = G.hbfp_operand(N, K, wm, -2, ws, seed=2, pattern=(5, 7, 2))
    q, worst = G.exact_certificate(xc, xe, xm, wc, we, wm)
    assert worst < 2 ** 24
    assert q == 2.0 ** (int(xe.min()) + int(we.min()) - xm - wm)
    # the certificate really bounds the sums: the exact product, divided by q, is integral and within it
    s = G.values(xc, xe, xm) @ G.values(wc, we, wm).t() / q
    assert torch.equal(s, s.round()) and float(s.abs().max()) <= worst
    # and the fp32 sum in block order is exact, as the kernels' is
    acc = torch.zeros(T, N, dtype=torch.float32)
    xv, wv = G.values(xc, xe, xm), G.values(wc, we, wm)
    for b in range(K // 64):
        acc += (xv[:, 64 * b:64 * b + 64] @ wv[:, 64 * b:64 * b + 64].t()).float()
    assert torch.equal(acc.double(), s * q)


def test_certificate_refuses_a_case_outside_the_exact_regime():
    xc, xe = G.hbfp_operand(4, 11008, 7, 0, 3, seed=1)
    wc, we = G.hbfp_operand(4, 11008, 3, 0, 3, seed=2)
    xc[:] = 127
    wc[:] = 7
    with pytest.raises(AssertionError, match="exact fp32 regime"):
        G.assert_exact_regime(xc, xe, 7, wc, we, 3)


def test_elementwise_bound():
    want = torch.tensor([1.0, 3.0, 1e-3, float("nan")], dtype=torch.float64)
    absprod = torch.tensor([1.0, 3.0, 1.0, 1.0], dtype=torch.float64)
    G.elementwise_bound(want.to(torch.bfloat16), want, absprod, 4, torch.bfloat16)
    with pytest.raises(AssertionError):
        G.elementwise_bound(torch.tensor([1.0, 3.0 + 2 ** -20, 1e-3, 0.0]), want, absprod, 4, torch.float32)
    assert float(G.ulp(torch.tensor([1.0]).double(), torch.float16)) == 2.0 ** -10
    assert float(G.ulp(torch.tensor([0.0]).double(), torch.float16)) == 2.0 ** -24
