"""Exact HBFP operands for the GEMM tests, and the certificate that makes a bit-for-bit comparison meaningful.

An operand [rows, K] is built as codes and block exponents: value = c * 2^(e_rb - m) with |c| <= 2^m - 1, block 64 unless `block`
says otherwise (16 and 32 for the small-block int8 GEMM).  Every block
holds at least one code of magnitude 2^m - 1 (for m >= 2 that makes the quantizer's block exponent exactly e_rb, so the values are
fixed points of the HBFP quantizer), and e_rb varies over rows AND blocks in a pattern of period 3 -- no period that lines up with a
tile edge -- so a block scale taken from the wrong row, block or trip changes some output by a factor of 2 or 4.

Certificate (exact_certificate): with q the smallest scale 2^(ex + ew - xm - wm) of the problem, every term x_k w_k and the bias are
integer multiples of q; when (sum_k |x_k w_k| + |b|) / q < 2^24 for every output, every fp32 partial sum is exact in ANY order (block
order, slices, split-K slabs), so the fp64 product is the kernel's fp32 sum before its one rounding to the output dtype.

elementwise_bound is the looser per-element statement for random data: an fp32 sum of n roundings is within n 2^-24 sum|x_k w_k| of
the exact sum, and the output rounding adds half an ulp of the output dtype.
"""
import torch

BLOCK = 64
# (significand bits, smallest normal exponent) of the output dtypes
_FMT = {torch.float32: (24, -126), torch.float16: (11, -14), torch.bfloat16: (8, -126)}


def exp_pattern(rows, nb, e0, spread, a=7, b=5, c=1, device="cpu"):
    """block exponents e0 + ((a r + b j + c r j + r^2 + j^2) mod 3) mod spread: period 3 over rows and blocks, and (the squares)
    no row or block column is constant when spread is 3"""
    r = torch.arange(rows, device=device).view(-1, 1)
    j = torch.arange(nb, device=device).view(1, -1)
    return e0 + ((a * r + b * j + c * r * j + r * r + j * j) % 3) % max(int(spread), 1)


def hbfp_operand(rows, K, m, e0, spread, seed, nm=(0, 0), pattern=(7, 5, 1), device="cpu", block=BLOCK):
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
        keep = keys.argsort(dim=-1).argsort(dim=-1) < N                   # N random positions of every group of M
        codes = codes * keep.view(rows, K).to(torch.int32)
        r = torch.rand((rows, nb, block), generator=g, device=device)
        pos = r.masked_fill(~keep.view(rows, nb, block), -1.0).argmax(-1)  # a kept position of every block
    else:
        pos = torch.randint(0, block, (rows, nb), generator=g, device=device)
    sign = torch.randint(0, 2, (rows, nb), generator=g, device=device, dtype=torch.int32) * 2 - 1
    cb = codes.view(rows, nb, block)
    cb.scatter_(2, pos.unsqueeze(-1), (sign * cmax).unsqueeze(-1))        # the forced block maximum
    exps = exp_pattern(rows, nb, e0, spread, *pattern, device=device).to(torch.int32)
    return codes, exps


def values(codes, exps, m, dtype=torch.float64, block=BLOCK):
    """c * 2^(e - m), per element (fp64 is exact; other dtypes are asserted exact by the caller's round trip)"""
    scale = torch.exp2((exps - m).double()).repeat_interleave(block, dim=1)
    return (codes.double() * scale).to(dtype)


def pack4(codes):
    """int codes [rows, K] (|c| <= 7) -> two's-complement nibbles, low nibble first (PackedBFP's 4-bit layout)"""
    u = (codes & 0xF).to(torch.uint8)
    return u[:, 0::2] | (u[:, 1::2] << 4)


def exact_certificate(xc, xe, xm, wc, we, wm, bias_over_q=None, block=BLOCK):
    """(q, worst) with q = 2^(min ex + min ew - xm - wm) and worst = max over outputs of (sum_k |x_k w_k| + |b|) / q.
    Computed as an fp64 product of integers scaled by powers of two: exact while it stays below 2^53."""
    exmin, ewmin = int(xe.min()), int(we.min())
    a = xc.abs().double() * torch.exp2((xe - exmin).double()).repeat_interleave(block, dim=1)
    b = wc.abs().double() * torch.exp2((we - ewmin).double()).repeat_interleave(block, dim=1)
    s = a @ b.t()
    if bias_over_q is not None:
        s = s + bias_over_q.abs().double().view(1, -1)
    q = 2.0 ** (exmin + ewmin - xm - wm)
    return q, float(s.max())


def assert_exact_regime(xc, xe, xm, wc, we, wm, bias_over_q=None, what=""):
    q, worst = exact_certificate(xc, xe, xm, wc, we, wm, bias_over_q)
    assert worst < 2.0 ** 24, f"{what}: operands leave the exact fp32 regime (sum |x w| / q = {worst:.4g} >= 2^24)"
    return q


def ulp(v, dtype):
    """ulp of the output dtype at |v| (fp64 tensor), subnormal range included"""
    p, emin = _FMT[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.exp2(e - (p - 1))


def elementwise_bound(got, want, absprod, n_adds, dtype):
    """per-element check: |got - want| <= n_adds 2^-24 sum|x_k w_k| + 1/2 ulp_out, where want is finite (NaN handled by the caller)"""
    g, w = got.double().to(want.device), want
    ok = torch.isfinite(w)
    err = (g - w).abs()
    lim = n_adds * 2.0 ** -24 * absprod + 0.5 * ulp(torch.maximum(g.abs().nan_to_num(0.0), w.abs()), dtype)
    bad = ok & ~(err <= lim)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} outputs outside the fp32 summation bound; first flat index {i}: got {float(g.flatten()[i])!r} "
                             f"want {float(w.flatten()[i])!r} bound {float(lim.flatten()[i]):.3g}")
