"""Exact HBFP operands at any block size (16 and 32 for the small-block int8 GEMM), with the certificate of gemm_cases.py.

gemm_cases.py fixes its block at 64; these builders take the block as an argument and keep its construction: every block holds a code
of magnitude 2^m - 1, and the block exponents vary over rows and blocks with period 3 (gemm_cases.exp_pattern), so a scale taken from
the wrong 16- or 32-block changes some output by a factor of 2 or 4.
"""
import torch

from gemm_cases import exp_pattern


def hbfp_operand(rows, K, m, e0, spread, seed, block, nm=(0, 0), pattern=(7, 5, 1), device="cpu"):
    """codes [rows, K] (int32, |c| <= 2^m - 1, N:M-pruned codes zero), block exponents [rows, K/block] (int32); every block has a
    kept code of magnitude 2^m - 1"""
    assert K % block == 0 and 1 <= m <= 7
    g = torch.Generator(device=device).manual_seed(seed)
    cmax = (1 << m) - 1
    codes = torch.randint(-cmax, cmax + 1, (rows, K), generator=g, device=device, dtype=torch.int32)
    N, M = nm
    nb = K // block
    if N and M and N < M:
        keys = torch.rand((rows, K // M, M), generator=g, device=device)
        keep = keys.argsort(dim=-1).argsort(dim=-1) < N
        codes = codes * keep.view(rows, K).to(torch.int32)
        r = torch.rand((rows, nb, block), generator=g, device=device)
        pos = r.masked_fill(~keep.view(rows, nb, block), -1.0).argmax(-1)
    else:
        pos = torch.randint(0, block, (rows, nb), generator=g, device=device)
    sign = torch.randint(0, 2, (rows, nb), generator=g, device=device, dtype=torch.int32) * 2 - 1
    codes.view(rows, nb, block).scatter_(2, pos.unsqueeze(-1), (sign * cmax).unsqueeze(-1))
    exps = exp_pattern(rows, nb, e0, spread, *pattern, device=device).to(torch.int32)
    return codes, exps


def values(codes, exps, m, block, dtype=torch.float64):
    """c * 2^(e - m), per element"""
    return (codes.double() * torch.exp2((exps - m).double()).repeat_interleave(block, dim=1)).to(dtype)


def exact_certificate(xc, xe, xm, wc, we, wm, block, bias_over_q=None):
    """gemm_cases.exact_certificate at this block: (q, max over outputs of (sum_k |x_k w_k| + |b|) / q)"""
    exmin, ewmin = int(xe.min()), int(we.min())
    a = xc.abs().double() * torch.exp2((xe - exmin).double()).repeat_interleave(block, dim=1)
    b = wc.abs().double() * torch.exp2((we - ewmin).double()).repeat_interleave(block, dim=1)
    s = a @ b.t()
    if bias_over_q is not None:
        s = s + bias_over_q.abs().double().view(1, -1)
    return 2.0 ** (exmin + ewmin - xm - wm), float(s.max())
