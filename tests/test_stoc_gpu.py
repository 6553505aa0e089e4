"""'stoc' rounding on every route against the reference's law (tests/stoc_law.py, pinned on the CPU by test_stoc_host.py).

Per route: every output bit pattern lies in the law's support; class frequencies (>= 2^22 samples for every class held by at
least 1/32 of the route's elements, the real count for smaller ones) match the law within 6 sigma + 1/n + 2^-16 (the hot loop's 16-bit dither resolution); rounding decisions on fraction-1/2 elements
agree at 1/2 across lags, lane items, blocks, rows, calls and tensors; the same torch.manual_seed reproduces the bits.
Then the Linear / matmul / conv wrappers under 'stoc', and the multi-rank rehearsal with every rank seeded alike."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import stoc_law as SL
from oracle import oracle as O
from quantization_sparsity_interplay_amd.bfp import bfp_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = SL.HOT_DITHER_RES


def cfg(**kw):
    c = dict(mant_bits=3, epsilon=1e-8, rounding_mode='stoc', device='cuda', block_size=64, num_format='bfp',
             weight_mant_bits=15, in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.0, N=0, M=0,
             sparsity_num_format='bfp', first='s', sparsity_mode='structured')
    c.update(kw)
    return c


def grid_tensor(shape, dtype, mant_bits=3, M=0, N=0, half=False, seed=0, block=64):
    """values (j + f) * 2^-m with a rounding-invariant prune mask: in every aligned group of M, N random positions
    (dense: a random half) are 'big' (|t| >= 2) and the others 'small' (|t| < 1, zeros among them); element 0 of
    every block has t = 2^m - 1/2, so the exponent is 0 and interval = 2^-m on every block.  half: every fraction 1/2
    (small: t = +-1/2, big: +-(j + 1/2)).  Returns (x on the CPU, mask of the small elements)."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    qmax = 2 ** mant_bits - 1
    pos = torch.arange(n) % shape[-1]
    first = (pos % block) == 0
    if M:                                        # N random positions of every group (a block's first element among them)
        r = torch.where(first, torch.full((n,), 2.0), torch.rand(n, generator=g, dtype=torch.float64))
        rank = r.view(-1, M).argsort(dim=1, descending=True).argsort(dim=1)
        big = (rank < N).reshape(-1)
    else:
        big = torch.rand(n, generator=g) < 0.5
    if half:
        frac = torch.full((n,), 0.5, dtype=torch.float64)
    else:
        frac = torch.randint(0, 8, (n,), generator=g).double() / 8
        frac = torch.where(torch.rand(n, generator=g) < 0.1, torch.full_like(frac, 0.5), frac)
    j = torch.randint(2, qmax, (n,), generator=g).double()
    t = torch.where(big, j + frac, frac)
    if not half:
        t = torch.where(~big & (torch.rand(n, generator=g) < 0.05), torch.zeros_like(t), t)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    t = t * sign
    t = torch.where(first, torch.full_like(t, qmax - 0.5), t)
    big = big | first
    x = (t * 2.0 ** -mant_bits).to(dtype).view(shape)
    small = (~big).view(shape)
    return x, small


class Route:
    def __init__(self, name, dtype, shape, c, M=0, N=0, first='s', direct=False, mant_bits=3, prob=True, cold=None,
                 noncontig=False, unstructured=False):
        self.name, self.dtype, self.shape, self.c = name, dtype, shape, c
        self.M, self.N, self.first, self.direct, self.mant_bits = M, N, first, direct, mant_bits
        self.prob, self.cold, self.noncontig, self.unstructured = prob, cold, noncontig, unstructured

    def inputs(self, half=False, seed=0):
        """(x, mask) -- x on the CPU in the route's logical layout"""
        if self.cold is not None:
            x = self.cold(self.dtype, self.shape, seed)
            if self.unstructured:                # distinct magnitudes: the oracle's mask is the kernel's (zeros do not matter s-first)
                kept = O.unstructured_sparsity(x, self.c['sparsity_frac'])
                return x, (kept == 0) & (x != 0)
            return x, None
        block = self.shape[-1] if self.direct else self.c['block_size']
        if self.unstructured:                    # half the elements small: exactly the ones a 50 % global prune takes
            x, small = grid_tensor(self.shape, self.dtype, self.mant_bits, 4, 2, half, seed, block)
        else:
            x, small = grid_tensor(self.shape, self.dtype, self.mant_bits, self.M, self.N, half, seed, block)
        pruned = small if (self.M or self.unstructured) else None
        return x, pruned

    def call(self, xd):
        if self.direct:
            return bfp_ops._convert_blocked_float_to_bfp(xd, self.mant_bits, 1e-8, 'stoc', 'cuda')
        if self.noncontig:
            xd = xd.t().contiguous().t()
        return bfp_ops.float_to_bfp_blocked(xd, **self.c, identifier='w')

    def law(self, x, mask):
        if self.direct:
            return SL.law(x, x.shape[-1], self.mant_bits)
        return SL.law(x, self.c['block_size'], self.c['mant_bits'], N=self.N, M=self.M, mask=mask, first=self.first)


def _cold_blocks(dtype, shape, seed, nonfinite=True):
    """ordinary blocks with cold ones among them: all zero, NaN, inf, subnormal scale, fp16 2^e overflow (rows of 64)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 0.5
    x2 = x.view(-1, 64)
    x2[3] = 0.0
    if nonfinite:
        x2[5, 7] = float('nan')
        x2[9, 2] = float('inf')
    sub = {torch.float32: 2.0 ** -140, torch.float16: 2.0 ** -20, torch.bfloat16: 2.0 ** -132}[dtype]
    x2[11] *= sub
    if dtype == torch.float16:                                   # |v| in [33000, 65000]: e = 16, 2^16 overflows in fp16
        x2[13] = torch.sign(x2[13]) * (33000 + (x2[13].abs() * 20000).clamp(max=32000))
        x2[13, 0] = 65504.0
    return x.to(dtype)


def _cold_finite(dtype, shape, seed):
    return _cold_blocks(dtype, shape, seed, nonfinite=False)


def _cold_distinct(dtype, shape, seed):
    """_cold_blocks without NaN / inf and with pairwise distinct non-zero magnitudes (fp16, <= 20480 elements): a global
    prune has no tie at its cut, so which elements it takes does not depend on a tie rule"""
    assert dtype == torch.float16
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    mags = torch.arange(0x1400, 0x6400, dtype=torch.int32).to(torch.int16).view(torch.float16).double()  # [2^-10, 2^10)
    x = mags[torch.randperm(mags.numel(), generator=g)[:n]] * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    x2 = x.view(-1, 64)
    x2[3] = 0.0
    x2[11] = (torch.randperm(1023, generator=g)[:64] + 1).double() * 2.0 ** -24          # distinct subnormals
    x2[13] = (33024 + 32 * torch.randperm(1000, generator=g)[:64]).double().clamp(max=65504)  # e = 16: 2^16 overflows
    return x.view(shape).to(dtype)


def _above_sig(dtype, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    return (x * torch.exp2(-torch.randint(0, 14, shape, generator=g).double())).to(dtype)


def _routes():
    R = []
    for dt in (torch.bfloat16, torch.float16):
        tag = str(dt).split('.')[-1]
        R.append(Route(f"{tag}-dense", dt, (256, 1024), cfg()))
        for N, M in ((1, 2), (2, 4), (4, 8)):
            for first in ('s', 'q'):
                R.append(Route(f"{tag}-{N}:{M}-{first}", dt, (256, 1024),
                               cfg(w_sparsity=True, N=N, M=M, first=first), M=M, N=N, first=first))
        R.append(Route(f"{tag}-cold-blocks", dt, (64, 1024), cfg(), prob=False, cold=_cold_blocks))
        R.append(Route(f"{tag}-mant15", dt, (64, 1024), cfg(mant_bits=15), mant_bits=15, prob=False, cold=_above_sig))
    R.append(Route("f32-dense", torch.float32, (256, 1024), cfg()))
    R.append(Route("f32-2:4-s", torch.float32, (256, 1024), cfg(w_sparsity=True, N=2, M=4), M=4, N=2))
    R.append(Route("f32-2:4-q", torch.float32, (256, 1024), cfg(w_sparsity=True, N=2, M=4, first='q'), M=4, N=2, first='q'))
    R.append(Route("f32-cold-blocks", torch.float32, (64, 1024), cfg(), prob=False, cold=_cold_blocks))
    R.append(Route("bf16-ragged-cols", torch.bfloat16, (256, 1000), cfg()))
    R.append(Route("f16-block48", torch.float16, (256, 960), cfg(block_size=48)))
    R.append(Route("bf16-3d", torch.bfloat16, (8, 32, 1024), cfg()))
    R.append(Route("f32-noncontig", torch.float32, (256, 1024), cfg(), noncontig=True))
    R.append(Route("f32-ragged-cols", torch.float32, (256, 1000), cfg()))
    for M, N in ((16, 8), (32, 8)):
        for first in ('s', 'q'):
            R.append(Route(f"bf16-{N}:{M}-{first}", torch.bfloat16, (256, 1024),
                           cfg(w_sparsity=True, N=N, M=M, first=first), M=M, N=N, first=first))
    for shape, tag in (((256, 1024), "fused"), ((256, 1000), "fallback")):
        R.append(Route(f"bf16-unstructured-s-{tag}", torch.bfloat16, shape,
                       cfg(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5), first='s', unstructured=True))
    R.append(Route("f32-unstructured-s-fused", torch.float32, (256, 1024),
                   cfg(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5), first='s', unstructured=True))
    R.append(Route("bf16-unstructured-q", torch.bfloat16, (256, 1024),
                   cfg(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='q'), first='q', unstructured=True))
    R.append(Route("bf16-convert-direct", torch.bfloat16, (4096, 64), None, direct=True))
    R.append(Route("f16-convert-direct", torch.float16, (4096, 64), None, direct=True))
    # the fp16 block whose 2^e overflows (the reference returns 65536, fp16 holds only +inf) on every kind of route
    R.append(Route("f16-cold-ragged-cols", torch.float16, (64, 1000), cfg(), prob=False, cold=_cold_blocks))
    R.append(Route("f16-cold-block48", torch.float16, (64, 960), cfg(block_size=48), prob=False, cold=_cold_blocks))
    R.append(Route("f16-cold-8:16-s", torch.float16, (16, 1024), cfg(w_sparsity=True, N=8, M=16), M=16, N=8, prob=False,
                   cold=_cold_distinct))
    R.append(Route("f16-cold-convert-direct", torch.float16, (1024, 64), None, direct=True, prob=False, cold=_cold_blocks))
    R.append(Route("f16-cold-convert-direct-b48", torch.float16, (1024, 48), None, direct=True, prob=False, cold=_cold_blocks))
    for shape, tag in (((16, 1024), "fused"), ((16, 1000), "fallback")):
        R.append(Route(f"f16-cold-unstructured-s-{tag}", torch.float16, shape,
                       cfg(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5), first='s', unstructured=True,
                       prob=False, cold=_cold_distinct))
    return R


ROUTES = _routes()
PROB_ROUTES = [r for r in ROUTES if r.prob]


def gbits(y):
    """canonical fp32 bit patterns of a device result, as int64 (NaN -> 0x7fc00000)"""
    f = y.float().reshape(-1)
    b = f.view(torch.int32).long() & 0xffffffff
    return torch.where(torch.isnan(f), torch.full_like(b, 0x7fc00000), b)


class DevLaw:
    def __init__(self, route, x, mask):
        bits, probs, ncls = route.law(x, mask)
        self.bits_np, self.probs, self.ncls_np = bits, probs, ncls
        self.bits = torch.from_numpy(bits.astype(np.int64)).to(DEV)
        self.ncls = torch.from_numpy(ncls).to(DEV)

    def index(self, y):
        b = gbits(y)
        idx = torch.full_like(b, -1)
        for c in range(3):
            hit = (self.bits[:, c] == b) & (c < self.ncls) & (idx < 0)
            idx = torch.where(hit, torch.full_like(idx, c), idx)
        return idx


def _assert_in_support(dl, y, x, what):
    idx = dl.index(y)
    bad = (idx < 0).nonzero()
    if bad.numel():
        i = int(bad[0])
        got = int(gbits(y)[i])
        raise AssertionError(f"{what}: {bad.numel()} outputs outside the law's support; first: flat element {i}, "
                             f"x = {x.reshape(-1)[i].item()!r}, got {got:#010x} ({np.uint32(got).view(np.float32)!r}), "
                             f"support {[hex(v) for v in dl.bits_np[i, :dl.ncls_np[i]]]}")
    return idx


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
def test_stoc_support_bitwise(route):
    x, mask = route.inputs(seed=1)
    dl = DevLaw(route, x, mask)
    xd = x.to(DEV)
    for s in range(8):
        torch.manual_seed(100 + s)
        y = route.call(xd)
        assert y.dtype == torch.float32, "'stoc' returns fp32 (the reference's dither promotes a half input)"
        assert tuple(y.shape) == tuple(x.shape)
        _assert_in_support(dl, y, x, f"{route.name}, call {s}")


SAMPLES = 1 << 22
MIN_SHARE = 32              # every class held by >= 1/MIN_SHARE of a route's elements gets >= SAMPLES samples


@pytest.mark.parametrize("route", PROB_ROUTES, ids=lambda r: r.name)
def test_stoc_class_probabilities(route):
    x, mask = route.inputs(seed=2)
    dl = DevLaw(route, x, mask)
    n = x.numel()
    kind = np.zeros(n, np.int64)
    flat = x.reshape(-1).float().numpy()
    kind[flat == 0] = 1                                          # zero inputs: P(-0) on its own
    if mask is not None and route.first == 's':
        kind[mask.reshape(-1).numpy()] = 2                       # s-first pruned: P(-0) on its own
    key = np.concatenate([np.round(dl.probs, 12), dl.ncls_np[:, None], kind[:, None]], 1)
    _, gid = np.unique(key, axis=0, return_inverse=True)
    gid = gid.reshape(-1)
    G = int(gid.max()) + 1
    gid_d = torch.from_numpy(gid).to(DEV)
    counts = torch.zeros(G * 3, dtype=torch.int64, device=DEV)
    xd = x.to(DEV)
    calls = max(16, -(-(SAMPLES * MIN_SHARE) // n))              # (smaller classes: checked with their own, smaller count)
    torch.manual_seed(7)
    for _ in range(calls):
        idx = _assert_in_support(dl, route.call(xd), x, route.name)
        counts += torch.bincount(gid_d * 3 + idx, minlength=G * 3)
    counts = counts.view(G, 3).cpu().numpy()
    for g in range(G):
        members = np.nonzero(gid == g)[0]
        p = dl.probs[members[0]]
        tot = counts[g].sum()
        for c in range(int(dl.ncls_np[members[0]])):
            f = counts[g, c] / tot
            tol = SL.binom_tol(p[c], tot, RES)
            assert abs(f - p[c]) <= tol, (f"{route.name}: class {c} of elements like x = {flat[members[0]]!r} "
                                          f"(kind {kind[members[0]]}, {len(members)} elements, {tot} samples): "
                                          f"frequency {f:.6f}, law {p[c]:.6f}, tolerance {tol:.6f}")


def _agree(a, b, va, vb, what):
    m = va & vb
    n = int(m.sum())
    assert n >= 1 << 16, f"{what}: only {n} pairs"
    rate = float((a[m] == b[m]).double().mean())
    tol = SL.binom_tol(0.5, n, RES)
    assert abs(rate - 0.5) <= tol, f"{what}: decisions agree at rate {rate:.5f} over {n} pairs (law 0.5, tolerance {tol:.5f})"


IND_ROUTES = [r for r in PROB_ROUTES if not r.direct]


@pytest.mark.parametrize("route", IND_ROUTES, ids=lambda r: r.name)
def test_stoc_independence(route):
    x, mask = route.inputs(half=True, seed=3)
    valid = torch.ones(x.numel(), dtype=torch.bool)
    if mask is not None:
        valid &= ~mask.reshape(-1)
    blk = x.shape[-1] if route.direct else route.c['block_size']
    valid &= (torch.arange(x.numel()) % x.shape[-1]) % blk != 0     # (the block maxima: fraction 1/2 too, but kept aside)
    valid = valid.to(DEV)
    xd = x.to(DEV)
    torch.manual_seed(11)
    ups = [(route.call(xd).float().reshape(-1) > xd.float().reshape(-1)) for _ in range(8)]
    cols = x.shape[-1]
    vec = 4 if x.dtype == torch.float32 else 8
    n = x.numel()
    for lag in sorted({1, 2, 3, 4, 7, vec, blk, cols}):
        a = torch.cat([u[:n - lag] for u in ups])
        b = torch.cat([u[lag:] for u in ups])
        va = valid[:n - lag].repeat(len(ups))
        vb = valid[lag:].repeat(len(ups))
        _agree(a, b, va, vb, f"{route.name}: lag {lag}")
    a = torch.cat(ups[:-1])
    b = torch.cat(ups[1:])
    vv = valid.repeat(len(ups) - 1)
    _agree(a, b, vv, vv, f"{route.name}: same element, consecutive calls")
    if not route.noncontig:
        c = dict(route.c)
        for s in range(4):
            torch.manual_seed(20 + s)
            y0, y1 = bfp_ops.float_to_bfp_blocked_many([xd, xd.clone()], identifier='w', **c)
            if s == 0:
                pa, pb = [], []
            pa.append(y0.float().reshape(-1) > xd.float().reshape(-1))
            pb.append(y1.float().reshape(-1) > xd.float().reshape(-1))
        vv = valid.repeat(4)
        _agree(torch.cat(pa), torch.cat(pb), vv, vv, f"{route.name}: same element of two equal tensors of one list call")


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
def test_stoc_reproducible_from_torch_seed(route):
    x, _ = route.inputs(seed=4)
    xd = x.to(DEV)
    torch.manual_seed(1234)
    a = gbits(route.call(xd))
    torch.manual_seed(1234)
    b = gbits(route.call(xd))
    torch.manual_seed(1235)
    c = gbits(route.call(xd))
    assert torch.equal(a, b), f"{route.name}: same torch.manual_seed, different bits"
    assert not torch.equal(a, c), f"{route.name}: different seeds, same bits"


# ---- wrappers: BFPLinear, F_linear_bfp, F_matmul_bfp, BFPConv2d under 'stoc' -------------------------------------------
def _capture(monkeypatch):
    rec = []
    real = bfp_ops.float_to_bfp_blocked

    def spy(t, *a, identifier='', **kw):
        y = real(t, *a, identifier=identifier, **kw)
        rec.append((identifier, t.detach().clone(), y.detach().clone(), kw.get('block_size'), kw.get('mant_bits')))
        return y
    monkeypatch.setattr(bfp_ops, "float_to_bfp_blocked", spy)

    def no_pair(*a, **k):
        raise AssertionError("the one-launch activation + weight path has no stochastic rounding")
    monkeypatch.setattr(bfp_ops.native.FastQuant, "many", no_pair)
    return rec


def _check_operand(ident, t, y, block, mant):
    assert y.dtype == torch.float32
    x = t.contiguous().cpu()
    bits, _, ncls = SL.law(x, block, mant)
    got = SL.canon_bits(y.contiguous().cpu()).reshape(-1)
    idx = SL.class_index(got, bits, ncls)
    assert (idx >= 0).all(), f"operand {ident}: {(idx < 0).sum()} values outside the law's support"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["BFPLinear", "F_linear_bfp", "F_matmul_bfp", "BFPConv2d"])
def test_stoc_wrappers_quantize_by_the_law(monkeypatch, dtype, kind):
    torch.manual_seed(3)
    c = cfg(mant_bits=4)
    del c['device']
    bias = dtype == torch.float32
    if kind == "BFPLinear":
        m = bfp_ops.BFPLinear(256, 128, bias=bias, **c, device='cuda').to(DEV, dtype)
        x = torch.randn(4, 16, 256, device=DEV, dtype=dtype, requires_grad=True)
        w, b = m.weight, m.bias
        fwd = lambda xx: m(xx)                                                    # noqa: E731
        ref = lambda xq, wq, bb: torch.nn.functional.linear(xq, wq, bb)          # noqa: E731
    elif kind == "F_linear_bfp":
        op = bfp_ops.F_linear_bfp(**c, device='cuda')
        w = torch.randn(128, 256, device=DEV, dtype=dtype, requires_grad=True)
        b = torch.randn(128, device=DEV, dtype=dtype, requires_grad=True) if bias else None
        x = torch.randn(64, 256, device=DEV, dtype=dtype, requires_grad=True)
        fwd = lambda xx: op(xx, w, b)                                             # noqa: E731
        ref = lambda xq, wq, bb: torch.nn.functional.linear(xq, wq, bb)          # noqa: E731
    elif kind == "F_matmul_bfp":
        op = bfp_ops.F_matmul_bfp(**c, device='cuda')
        w = torch.randn(256, 128, device=DEV, dtype=dtype, requires_grad=True)
        b = None
        x = torch.randn(2, 32, 256, device=DEV, dtype=dtype, requires_grad=True)
        fwd = lambda xx: op(xx, w)                                                # noqa: E731
        ref = lambda xq, wq, bb: torch.matmul(xq, wq)                             # noqa: E731
    else:
        m = bfp_ops.BFPConv2d(8, 16, 3, padding=1, bias=bias, **c, device='cuda').to(DEV, dtype)
        x = torch.randn(2, 8, 16, 64, device=DEV, dtype=dtype, requires_grad=True)
        w, b = m.weight, m.bias
        fwd = lambda xx: m(xx)                                                    # noqa: E731
        ref = lambda xq, wq, bb: torch.nn.functional.conv2d(xq, wq, bb, padding=1)  # noqa: E731
    rec = _capture(monkeypatch)
    y = fwd(x)
    assert y.dtype == torch.float32, "the quantized operands are fp32 under 'stoc', so the GEMM is"
    fw = {r[0]: r for r in rec}
    assert set(fw) == {'in', 'w'}, [r[0] for r in rec]
    for ident, t, q, blk, mb in rec:
        _check_operand(ident, t, q, blk, mb)
    xq, wq = fw['in'][2], fw['w'][2]
    if kind == "F_matmul_bfp":
        wq = wq.transpose(-1, -2)                      # (quantized along K, handed back in the original layout)
        assert torch.equal(fw['w'][1], w.detach().transpose(-1, -2))
    xr = xq.clone().requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    want = ref(xr, wr, b.detach() if b is not None else None)
    assert torch.equal(y.detach().view(torch.int32), want.detach().view(torch.int32)), "output != op on the captured operands"
    g = torch.randn_like(y)
    rec.clear()
    y.backward(g)
    assert [r[0] for r in rec] == ['grad']
    _check_operand('grad', *rec[0][1:])
    gq = rec[0][2]
    want.backward(gq)
    assert torch.equal(x.grad.float().view(torch.int32), xr.grad.to(x.dtype).float().view(torch.int32))
    assert torch.equal(w.grad.float().view(torch.int32), wr.grad.to(w.dtype).float().view(torch.int32))


def test_stoc_weight_cache_is_bypassed(monkeypatch):
    c = cfg(mant_bits=4)
    del c['device']
    m = bfp_ops.BFPLinear(256, 128, bias=False, **c, device='cuda').to(DEV)
    m.enable_weight_cache(True)
    m.eval()
    x = torch.randn(8, 256, device=DEV)
    rec = _capture(monkeypatch)
    with torch.no_grad():
        torch.manual_seed(1)
        a = m(x)
        torch.manual_seed(2)
        b = m(x)
    cache = m._weight_cache
    assert cache.hits == 0 and cache.misses == 0
    assert [r[0] for r in rec] == ['in', 'w', 'in', 'w']
    assert not torch.equal(rec[1][2], rec[3][2]), "the weight is re-rounded on every call"
    assert not torch.equal(a, b)


# ---- the multi-rank rehearsal on one device, every rank seeded alike -------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dist_worker(rank, world, port, tmpdir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantization_sparsity_interplay_amd import dist as qd
        outs = {}
        for name, c in (("dense", cfg()), ("2:4", cfg(w_sparsity=True, N=2, M=4)),
                        ("unstructured", cfg(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5))):
            full, _ = grid_tensor((world * 64, 1024), torch.bfloat16, half=True, seed=5,
                                  M=4 if name != "dense" else 0, N=2 if name != "dense" else 0)
            local = qd.shard_rows(full.to(DEV), world, rank)
            torch.manual_seed(77)                        # every rank alike
            y = qd.float_to_bfp_blocked_sharded(local, full.shape[0], gather=False, identifier='w', **c)
            torch.manual_seed(77)
            ym = qd.float_to_bfp_blocked_many_sharded([local, local], [full.shape[0]] * 2, gather=False, identifier='w', **c)
            outs[name] = (y.cpu(), ym[0].cpu(), local.cpu())
        torch.save(outs, os.path.join(tmpdir, f"r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_stoc_sharded_ranks_seeded_alike_round_independently(tmp_path):
    world = 2
    mp.spawn(_dist_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(tmp_path / f"r{r}.pt") for r in range(world)]
    for name in ("dense", "2:4", "unstructured"):
        ups, vals = [], []
        for r in range(world):
            y, ym, local = res[r][name]
            M = 4 if name != "dense" else 0
            _, small = grid_tensor((world * 64, 1024), torch.bfloat16, half=True, seed=5, M=M, N=2 if M else 0)
            mask = small[r * 64:(r + 1) * 64] if name != "dense" else None
            for yy in (y, ym):
                bits, _, ncls = SL.law(local, 64, 3, mask=mask, first='s')
                idx = SL.class_index(SL.canon_bits(yy).reshape(-1), bits, ncls)
                assert (idx >= 0).all(), f"{name}, rank {r}: outputs outside the law's support"
            ups.append((y.float() > local.float()).reshape(-1))
            v = ((torch.arange(local.numel()) % 1024) % 64 != 0)
            if mask is not None:
                v &= ~mask.reshape(-1)
            vals.append(v)
        # same torch seed on both ranks, same slab positions: the decisions must still agree only at 1/2
        m = vals[0] & vals[1]
        n = int(m.sum())
        rate = float((ups[0][m] == ups[1][m]).double().mean())
        tol = SL.binom_tol(0.5, n, RES)
        assert abs(rate - 0.5) <= tol, f"{name}: shards agree at rate {rate:.4f} over {n} positions (law 0.5, tolerance {tol:.4f})"
