"""The HBFP KV cache's kernels pinned to recorded bits (csrc/bfpq_kvcache.hip).  The other test_kvcache*_gpu.py tests
compare one route with another, so a change made to every route at once passes them; this one compares every output with SHA-256
digests recorded once, tests/golden/kv_pinned.json.

Per (dtype, block, D) in fp32/64/64, bf16/32/64, fp16/16/32 and kv_heads 2 and 1 (group 1 and 2) of 2 heads, batch 3, capacity 192:
  - a device-length cache, prompt_rows 48, filled to the lengths (0, 65, 130) -- an empty head, a ragged last block, more than one key
    tile -- by a chunk, one token and a chunk of 5 that closes one block and opens the next: the five buffers after every append;
  - scores(), context() and attend(return_probs=True) of 1 and 3 rows, causal on and off, chunks_per_split 1 and 0 (context() of
    3 rows over p [.., 100]: a head longer than p);
  - the prompt attend() of 70 rows (two panels, the first of group x 48 rows: it crosses the 64-row workgroup and the 16-row tile),
    causal -- where some waves stop before the last block -- and not;
  - a host-length cache filled the same way to 65 tokens: its buffers, scores() and context() of 3 rows.
Inputs are made on the CPU from fixed seeds as integers times powers of two (exact in fp32, so no math library has a say) and are
finite; fp16 runs with an epsilon fp16 can hold (tests/test_kvcache_prompt_gpu.py says why).  NaN routing stays with the other tests: a
NaN in an output is digested as one fixed pattern.

Run as a script with --record it writes the fixture.  --record may only be run on a commit whose kernels are known good -- it pins
whatever they compute -- and the digests hold for one compiler: a new compiler may contract or reorder the fp32 softmax differently,
and the fixture is then recorded again on the commit before the upgrade's first kernel change.  A mismatch names the step."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                           # (as a script: conftest.py has not set the path)
    sys.path.insert(0, ROOT)
from quantization_sparsity_interplay_amd.bfp import bfp_ops         # noqa: E402
from util import bits, is_nan_bits                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(ROOT, "tests", "golden", "kv_pinned.json")
DT = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)
B, H, CAP = 3, 2, 192
LENS = (0, 65, 130)
APPENDS = ((124, (0, 59, 124)), (1, (0, 1, 1)), (5, (0, 5, 5)))       # (rows of the chunk, what each sequence takes of it)
HOST_APPENDS = (59, 1, 5)
PROMPT_ROWS, PROMPT_TQ = 48, 70
CASES = (("fp32", 64, 64, 7), ("bf16", 32, 64, 3), ("fp16", 16, 32, 7))   # dtype, block, D, mant_bits
KVHS = (2, 1)
BUFFERS = ("k_codes", "k_exps", "v_codes", "v_exps", "v_tail")


def _cfg(dtype, block, mant):
    return dict(mant_bits=mant, epsilon=2.0 ** -14 if dtype == torch.float16 else 1e-8, rounding_mode='determ', device='cuda', block_size=block,
                num_format='bfp', weight_mant_bits=15, in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4,
                sparsity_num_format='bfp', first='s', sparsity_mode='structured')


def _ints(shape, dtype, seed, positive=False):
    """16-bit integers times 2^-16 times a binade per row in 2^-6 .. 2^3: exact in fp32, rounded once to the dtype"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0 if positive else -(1 << 15), 1 << 15, shape, generator=g).float()
    e = torch.randint(-6, 4, shape[:-1] + (1,), generator=g)
    scale = ((e - 16 + 127).to(torch.int32) << 23).view(torch.float32)   # 2^(e - 16), from its bits
    return (m * scale).to(dtype).to(DEV)


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous()
        if t.is_floating_point():
            a = bits(t)
            a[is_nan_bits(a, t.dtype)] = 0x7FC0 if a.dtype == np.uint16 else 0x7FC00000
        else:
            a = t.cpu().numpy()
        h.update(str((str(t.dtype), tuple(t.shape))).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def digests(dname, block, D, mant, kvh):
    """{step: digest} of one case, in the order the steps run"""
    dtype, out = DT[dname], {}
    kw, seed, scale = _cfg(dtype, block, mant), 1000 * block + 10 * kvh, D ** -0.5
    S = sum(t for t, _ in APPENDS)
    k, v = _ints((B, kvh, S, D), dtype, seed), _ints((B, kvh, S, D), dtype, seed + 1)
    with torch.no_grad():
        dev = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, device_lengths=True, kv_heads=kvh, prompt_rows=PROMPT_ROWS, **kw)
        s0 = 0
        for i, (t, counts) in enumerate(APPENDS):
            dev.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous(), _i32(*counts))
            out[f"dev/append{i}"] = _digest(*(getattr(dev, n) for n in BUFFERS), dev.lengths, dev.overflow)
            s0 += t
        assert dev.lengths.tolist() == list(LENS) and dev.overflow.item() == 0
        for Tq, L in ((1, CAP), (3, 100)):
            q, p = _ints((B, H, Tq, D), dtype, seed + 2 + Tq), _ints((B, H, Tq, L), dtype, seed + 6 + Tq, positive=True)
            out[f"dev/scores/tq{Tq}"] = _digest(dev.scores(q))
            for cps in (1, 0):
                dev.chunks_per_split = cps
                out[f"dev/context/tq{Tq}/cps{cps}"] = _digest(dev.context(p))
                for causal in (False, True):
                    out[f"dev/attend/tq{Tq}/causal{int(causal)}/cps{cps}"] = _digest(*dev.attend(q, scale, causal=causal, return_probs=True))
        q = _ints((B, H, PROMPT_TQ, D), dtype, seed + 12)
        for causal in (False, True):
            out[f"dev/prompt/causal{int(causal)}"] = _digest(*dev.attend(q, scale, causal=causal, return_probs=True))
        assert dev.lengths.tolist() == list(LENS) and dev.overflow.item() == 0

        host = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, kv_heads=kvh, **kw)
        s0 = 0
        for t in HOST_APPENDS:
            host.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous())
            s0 += t
        out["host/appends"] = _digest(*(getattr(host, n) for n in BUFFERS))
        out["host/scores/tq3"] = _digest(host.scores(_ints((B, H, 3, D), dtype, seed + 13)))
        out["host/context/tq3"] = _digest(host.context(_ints((B, H, 3, s0), dtype, seed + 14, positive=True)))
    return out


def _key(dname, block, D, mant, kvh):
    return f"{dname}-b{block}-d{D}-m{mant}-kv{kvh}"


@pytest.mark.parametrize("kvh", KVHS)
@pytest.mark.parametrize("dname,block,D,mant", CASES, ids=[f"{c[0]}-b{c[1]}-d{c[2]}" for c in CASES])
def test_every_output_has_its_recorded_bits(dname, block, D, mant, kvh):
    want = json.load(open(FIXTURE))[_key(dname, block, D, mant, kvh)]
    got = digests(dname, block, D, mant, kvh)
    assert list(got) == list(want), "the steps of the test and of the fixture differ: see --record in the module's docstring"
    bad = [step for step in got if got[step] != want[step]]
    assert not bad, f"{_key(dname, block, D, mant, kvh)}: {len(bad)} of {len(got)} outputs differ from the recorded bits: {bad}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_kvcache_pinned_gpu.py --record   (only on a commit whose kernels are known good)")
    rec = {_key(*c, kvh): digests(*c, kvh) for c in CASES for kvh in KVHS}
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"recorded {sum(len(r) for r in rec.values())} digests in {FIXTURE}")
