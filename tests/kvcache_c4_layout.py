"""The layout of a 4-bit HBFP KV cache's code buffers (HBFPKVCache(code_bits=4)), restated in torch for the tests: two codes to
a byte, element 2 k in the low nibble of byte k and element 2 k + 1 in its high nibble, two's complement.  Not a test module."""
import torch


def pack(codes):
    """int8 codes in -8..7 [..., n] (n even) -> int8 bytes [..., n / 2]"""
    assert codes.dtype == torch.int8 and codes.shape[-1] % 2 == 0
    c = codes.to(torch.int16)
    assert c.numel() == 0 or (int(c.min()) >= -8 and int(c.max()) <= 7)
    lo, hi = c[..., 0::2] & 15, c[..., 1::2] & 15
    return (lo | (hi << 4)).to(torch.uint8).view(torch.int8)


def unpack(packed):
    """int8 bytes [..., n] -> int8 codes [..., 2 n], sign-extended"""
    assert packed.dtype == torch.int8
    b = packed.view(torch.uint8).to(torch.int16)
    both = torch.stack((b & 15, b >> 4), dim=-1)
    both = torch.where(both >= 8, both - 16, both)
    return both.reshape(*packed.shape[:-1], 2 * packed.shape[-1]).to(torch.int8)
