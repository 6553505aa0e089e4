"""Pure-torch restatement of the sp24 layout (csrc/bfpq_sp24.hip): the two kept codes of every group of 4 along K and their 2-bit
positions, tiled for the decode kernel.  Used by tests/test_sp24_host.py (CPU) and tests/test_sp24_gpu.py (device pack byte for byte)."""
import torch

IDX_CH = 8


def keep2(codes):
    """int codes [N, K] -> (values [N, K/2], positions [N, K/2]) of every group of 4: the non-zero positions first, then the lowest free
    ones, ascending; counts of non-zeros per group [N, K/4]"""
    N, K = codes.shape
    g = codes.view(N, K // 4, 4)
    nz = g != 0
    pos = torch.arange(4).view(1, 1, 4).expand_as(g)
    key = torch.where(nz, pos, pos + 4)
    sel = key.argsort(dim=-1, stable=True)[..., :2].sort(dim=-1).values
    vals = torch.gather(g, 2, sel)
    return vals.reshape(N, K // 2), sel.reshape(N, K // 2), nz.sum(-1)


def _tiles(per_lane, N, K):
    """[N, K/16, U] (row, lane-block of 16 K, bytes) -> [N/16, nb, 64, U] (tile, block, lane = r + 16 q, bytes)"""
    U = per_lane.shape[-1]
    return per_lane.view(N // 16, 16, K // 64, 4, U).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 64, 64, U)


def _chunked(t, CH):
    """[R, nb, 64, U] -> flat bytes: per tile, chunks of CH blocks, lane-major inside a chunk"""
    R, nb, _, U = t.shape
    parts = [t[:, c0:c0 + CH].permute(0, 2, 1, 3).reshape(R, -1) for c0 in range(0, nb, CH)]
    return torch.cat(parts, dim=1).reshape(-1)


def _unchunked(flat, R, nb, U, CH):
    t = flat.view(R, -1)
    out, o = [], 0
    for c0 in range(0, nb, CH):
        nbc = min(CH, nb - c0)
        out.append(t[:, o:o + 64 * nbc * U].reshape(R, 64, nbc, U).permute(0, 2, 1, 3))
        o += 64 * nbc * U
    return torch.cat(out, dim=1)


def pack(codes, code_bits):
    """int codes [N, K] (at most 2 non-zeros per group of 4) -> (vals uint8, idx uint8), the bytes bfpq_sp24_pack writes"""
    N, K = codes.shape
    v, p, cnt = keep2(codes.to(torch.int64))
    assert int(cnt.max()) <= 2
    v = v.view(N, K // 16, 8)
    if code_bits == 4:
        u = (v & 15).to(torch.uint8)
        vb = u[..., 0::2] | (u[..., 1::2] << 4)                   # value j in nibble j, low first
    else:
        vb = (v & 255).to(torch.uint8)
    ix = (p.view(N, K // 16, 8) << (2 * torch.arange(8))).sum(-1)
    ib = torch.stack([ix & 255, ix >> 8], dim=-1).to(torch.uint8)
    return _chunked(_tiles(vb, N, K), 16 // vb.shape[-1]), _chunked(_tiles(ib, N, K), IDX_CH)


def unpack(vals, idx, N, K, code_bits):
    """the inverse: int64 codes [N, K]"""
    nb, U = K // 64, (4 if code_bits == 4 else 8)
    vb = _unchunked(vals, N // 16, nb, U, 16 // U).to(torch.int64)          # [R, nb, 64, U]
    ib = _unchunked(idx, N // 16, nb, 2, IDX_CH).to(torch.int64)
    if code_bits == 4:
        v = torch.stack([vb & 15, vb >> 4], dim=-1).reshape(*vb.shape[:3], 8)
        v = torch.where(v >= 8, v - 16, v)
    else:
        v = torch.where(vb >= 128, vb - 256, vb)
    ix = ib[..., 0] | (ib[..., 1] << 8)
    pos = (ix.unsqueeze(-1) >> (2 * torch.arange(8))) & 3                 # [R, nb, 64, 8]
    grp = torch.zeros(*v.shape[:3], 4, 4, dtype=torch.int64)
    grp.scatter_(4, pos.view(*v.shape[:3], 4, 2), v.view(*v.shape[:3], 4, 2))
    # [R, nb, q r, 16] -> rows
    return grp.view(N // 16, nb, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K)


def dense_bytes(codes, code_bits):
    """int codes [N, K] -> the dense packed codes (4-bit: uint8 [N, K/2] nibbles low first; 8-bit: int8 [N, K])"""
    if code_bits == 8:
        return codes.to(torch.int8)
    u = (codes & 15).to(torch.uint8)
    return u[:, 0::2] | (u[:, 1::2] << 4)


def random_nm(N, K, n, bits, seed):
    """random int codes [N, K] of `bits`-bit two's complement with at most n non-zeros in every group of 4"""
    g = torch.Generator().manual_seed(seed)
    cmax = (1 << (bits - 1)) - 1
    c = torch.randint(-cmax - 1, cmax + 1, (N, K), generator=g)
    keep = torch.rand(N, K // 4, 4, generator=g).argsort(-1).argsort(-1) < n
    return c * keep.view(N, K)


def nbytes(N, K, code_bits):
    """bytes of the sp24 form with the exponents: (0.25 or 0.5) + 0.125 + 1/64 per weight"""
    return N * K * code_bits // 16 + N * K // 8 + N * K // 64
