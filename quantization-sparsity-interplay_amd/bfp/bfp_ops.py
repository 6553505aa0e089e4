"""Drop-in operator surface of the reference's src/transformers/bfp/bfp_ops.py, backed by the
MI355X HIP engine (libbfpq.so).  Same names, argument order, aliasing and exceptions as the
reference (file:line cited per function); the tensor math itself is NOT here -- it is in
csrc/bfpq_kernels.hip, reached through ..native.  ROCm-device tensors only: a CPU tensor raises
NativeUnavailable (there is deliberately no CPU fallback).

Differences from the reference, all documented in DESIGN.md:
  * 'stoc' rounding draws its dither from a counter-based generator seeded from torch's CPU RNG
    (torch.manual_seed controls it); the reference's torch.rand stream is not reproduced.
  * _unstructured_sparsity: which of the elements EQUAL to the threshold are pruned is "lowest flat
    index first"; the reference's choice is an artefact of a sequential introselect.
"""
import array
import collections
import contextlib
import math
import numbers
import threading

import torch
import torch.nn.functional as F

from .. import native
from .. import ops as _ops          # registers torch.ops.bfpq.* (traceable entry points)

__all__ = ["rounding_modes", "round_tensor", "get_exponent", "float_to_bfp_blocked", "float_to_bfp_blocked_many", "PreparedMany", "float_to_bfp_packed",
           "sparsify", "unpack_bfp_args", "F_linear_bfp", "F_matmul_bfp", "BFPLinear", "BFPConv2d", "WeightCache", "PackedBFP"]


class rounding_modes:
    """reference: bfp_ops.py:16-18"""
    STOC, DETERM = 'stoc', 'determ'
    modes = [STOC, DETERM]


_seed_salt = threading.local()     # .value non-zero inside seed_salt(): mixed into every 'stoc' seed drawn on this thread


@contextlib.contextmanager
def seed_salt(salt):
    """'stoc' seeds drawn inside (on this thread) are mixed with `salt`; the torch generator advances as without it.  The
    sharded paths (dist.py) salt with the global rank: jobs seed every process alike, and the dither is keyed by the
    shard-local element index, so without it every shard would round with the same dither field."""
    prev = getattr(_seed_salt, 'value', 0)
    _seed_salt.value = int(salt)
    try:
        yield
    finally:
        _seed_salt.value = prev


def _mix_seed(seed, salt):
    """splitmix64 finalizer of seed ^ salt * golden ratio, cut to a non-zero 62-bit seed"""
    m = (1 << 64) - 1
    z = (seed ^ (salt * 0x9E3779B97F4A7C15)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z = (z ^ (z >> 31)) & ((1 << 62) - 1)
    return z or 1


@contextlib.contextmanager
def _replay_seeds(seeds):
    """'stoc' seeds drawn inside (on this thread) are taken from `seeds` in order, without touching torch's generator: a call that
    redoes itself on another route rounds with the seeds it already drew"""
    prev = getattr(_seed_salt, 'replay', None)
    _seed_salt.replay = list(seeds)
    try:
        yield
    finally:
        _seed_salt.replay = prev


def _seed_for(mode):
    """0 -> round-half-even; otherwise a non-zero 62-bit seed taken from torch's CPU generator (salted by seed_salt)"""
    if mode == rounding_modes.DETERM:
        return 0
    if mode == rounding_modes.STOC:
        replay = getattr(_seed_salt, 'replay', None)
        if replay:
            return replay.pop(0)
        seed = int(torch.randint(1, 2 ** 62, (1,)).item())
        salt = getattr(_seed_salt, 'value', 0)
        return _mix_seed(seed, salt) if salt else seed
    raise NotImplementedError("Rounding mode %s is not implemented", mode)


def _quantize_nm_ref_dtype(t, block_size, mant_bits, epsilon, rounding_mode, N=0, M=0, sparsify_first=True):
    """quantize_nm with the reference's output dtype: 'stoc' on a half tensor comes back as fp32.
    The single-pass kernel writes that fp32 image directly; other shapes convert afterwards."""
    seed = _seed_for(rounding_mode)
    if seed == 0:                                      # round-half-even
        if torch.compiler.is_compiling():              # under torch.compile / export: the registered (traceable) op
            return torch.ops.bfpq.fake_quantize(t, int(block_size), int(mant_bits), float(epsilon), int(N), int(M), bool(sparsify_first), 0)
        return _fast_quant(block_size, mant_bits, epsilon, N, M, sparsify_first)(t)
    src = t.contiguous()
    if seed and t.dtype != torch.float32 and t.numel() and block_size > 0 and native.is_fused(src, block_size, N, M):
        _, y, _ = native.quantize_nm(src, block_size, mant_bits, epsilon, N=N, M=M, sparsify_first=sparsify_first,
                                     want_deq=False, code_bits=32, stoch_seed=seed)
        return y.view(t.shape)
    y, _, _ = native.quantize_nm(src, block_size, mant_bits, epsilon, N=N, M=M, sparsify_first=sparsify_first, stoch_seed=seed)
    return _stoc_dtype(y.view(t.shape), rounding_mode)


_fast_quants = {}


def _fast_quant(block_size, mant_bits, epsilon, N, M, sparsify_first):
    """the bound form of the drop-in call for one configuration (native.FastQuant), made once"""
    key = (block_size, mant_bits, epsilon, N, M, sparsify_first)
    f = _fast_quants.get(key)
    if f is None:
        f = _fast_quants[key] = native.FastQuant(block_size, mant_bits, epsilon, N, M, sparsify_first)
    return f


def _stoc_dtype(t, mode):
    """reference quirk: 'stoc' adds fp32 noise, so a half input comes back as fp32.  t is the result written in
    the input's dtype; for fp16 its +-inf stands for the fp32 result +-65536 (native.stoc_widen_f16)."""
    if mode != rounding_modes.STOC or t.dtype == torch.float32:
        return t
    return native.stoc_widen_f16(t) if t.dtype == torch.float16 else t.float()


def round_tensor(t, mode, device):
    """reference: bfp_ops.py:20-27 (elementwise; kept for API completeness, not on the fused path)"""
    if mode == rounding_modes.STOC:
        sampled = torch.rand(t.shape, device=t.device) - 0.5
        return sampled.add_(t).round()
    elif mode == rounding_modes.DETERM:
        return t.round()
    raise NotImplementedError("Rounding mode %s is not implemented", mode)


def get_exponent(t, epsilon):
    """reference: bfp_ops.py:29-33 -- t is [nblk, block]; returns the shared exponent per row, [nblk, 1],
    in t.dtype.  (int8 transport: exponents outside [-127, 127] saturate; NaN blocks come back as NaN.)"""
    native.require_device_tensor(t)
    assert t.dim() == 2
    _, _, e = native.quantize_nm(t, t.shape[1], 0, epsilon, want_deq=False, want_exp=True)
    out = e.to(t.dtype).view(-1, 1)
    return torch.where(e.view(-1, 1) == -128, torch.full_like(out, float('nan')), out)


def _convert_blocked_float_to_bfp(t, mant_bits, epsilon, rounding_mode, device):
    """reference: bfp_ops.py:35-44 -- every row of the 2-D t is one block"""
    native.require_device_tensor(t)
    assert t.dim() == 2
    seed = _seed_for(rounding_mode)
    src = t.contiguous()
    if seed and t.dtype != torch.float32 and t.numel() and native.is_fused(src, t.shape[1]):
        _, y, _ = native.quantize_nm(src, t.shape[1], mant_bits, epsilon, want_deq=False, code_bits=32, stoch_seed=seed)
        return y                                       # the fp32 result, written by the kernel
    y, _, _ = native.quantize_nm(src, t.shape[1], mant_bits, epsilon, stoch_seed=seed)
    return _stoc_dtype(y, rounding_mode)


def _no_sparsity_float_to_bfp(t, block_size, mant_bits, epsilon, rounding_mode, device):
    """reference: bfp_ops.py:46-59 -- blocks of block_size along the last dim, zero-padded per row"""
    native.require_device_tensor(t)
    return _quantize_nm_ref_dtype(t, block_size, mant_bits, epsilon, rounding_mode)


_select_ws = collections.OrderedDict()
_spare_ws = {}                     # device index -> workspaces made (and really zeroed) outside any capture, for streams first met inside one
_SELECT_WS_MAX = 16                # workspaces kept (5 MB each): least recently used (device, stream) pairs beyond that are dropped
_SPARES = 2


def _workspace(device):
    """select workspace of the current stream of `device` (the launches of one call talk through it, so two streams
    must not share one).  Kept per (device, stream), least recently used first out -- except workspaces a captured graph
    refers to, which stay for good (the graph holds their address).
    A workspace cannot be BORN inside a hipGraph capture: its zero-fill would be recorded instead of run, and its memory would
    belong to the graph's pool.  torch.cuda.graph() captures on a stream of its own, so a stream first met inside a capture
    gets one of the spare workspaces that every eager call keeps in stock; only a capture with no eager unstructured call
    before it on this device (capture needs a warm-up anyway) finds none."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    capturing = torch.cuda.is_current_stream_capturing()
    ws = _select_ws.get(key)
    if ws is None:
        if capturing:
            spares = _spare_ws.get(idx)
            if not spares:
                raise RuntimeError("the unstructured path needs a workspace that exists before graph capture starts: "
                                   "run one unstructured call on this device outside torch.cuda.graph(...) first (outside the capture)")
            ws = spares.pop()
        else:
            ws = native.SelectWorkspace(torch.device("cuda", idx))
        _select_ws[key] = ws
        if len(_select_ws) > _SELECT_WS_MAX:
            for old in [k for k, w in _select_ws.items() if not w.pinned and k != key][:len(_select_ws) - _SELECT_WS_MAX]:
                del _select_ws[old]
    else:
        _select_ws.move_to_end(key)
    if capturing:
        ws.pinned = True
    else:
        spares = _spare_ws.setdefault(idx, [])
        while len(spares) < _SPARES:
            spares.append(native.SelectWorkspace(torch.device("cuda", idx)))
    return ws


def _unstructured_sparsity(t, device, sparsity_frac=0):
    """reference: bfp_ops.py:61-71 -- zero the int(numel*frac) smallest |v| of the whole tensor"""
    assert (sparsity_frac > 0)
    native.require_device_tensor(t)
    if t.numel() == 0:
        return t.clone()
    k = native.prune_count(t, sparsity_frac)
    ws = _workspace(t.device)
    native.select_threshold(t, k, ws)
    return native.threshold_apply(t, ws).view(t.shape)


def _structured_N_M_sparsity(t, device, N=0, M=0):
    """reference: bfp_ops.py:73-91 -- per group of M along the last dim keep the N largest |v|"""
    assert ((N > 0) and (M > 0) and (N <= M))
    native.require_device_tensor(t)
    if N == M:
        return t.contiguous().clone().view(t.shape)
    y, _, _ = native.quantize_nm(t, 0, 0, 0.0, N=N, M=M)
    return y.view(t.shape)


def _sparsify(t, sparsity, sparsity_mode, device, N, M, sparsity_frac):
    """reference: bfp_ops.py:93-102"""
    if sparsity == True:  # noqa: E712  (the reference compares with ==; 1 counts as True)
        if sparsity_mode == 'structured':
            return _structured_N_M_sparsity(t, device, N, M)
        elif sparsity_mode == 'unstructured':
            return _unstructured_sparsity(t, device, sparsity_frac)
        else:
            raise ValueError(f'Unknown sparsity mode: {sparsity_mode} given as argument')
    else:
        return t


def _quantize(t, num_format, block_size, mant_bits, weight_mant_bits, sgd_update, epsilon, rounding_mode, device, identifier):
    """reference: bfp_ops.py:104-122"""
    if num_format == 'fp32':
        return t
    elif num_format == 'bfp':
        if sgd_update:
            mant_bits = weight_mant_bits
        return _no_sparsity_float_to_bfp(t, block_size, mant_bits, epsilon, rounding_mode, device)
    elif num_format == 'int':
        # per-channel symmetric integer grid (int_ops.Quantizer with its defaults); fp32 result as in the reference
        if sgd_update:
            mant_bits = weight_mant_bits
        quant_t = native.int_quantize(t, mant_bits, identifier == 'w')
        assert (t.shape == quant_t.shape)
        return quant_t
    else:
        raise ValueError(f'Unknown quantization format: {num_format} given as argument')


def _select_sparsity(in_sparsity, w_sparsity, grad_sparsity, identifier):
    """reference: bfp_ops.py:132-139"""
    if in_sparsity == True and identifier == 'in':  # noqa: E712
        return True
    elif w_sparsity == True and identifier == 'w':  # noqa: E712
        return True
    elif grad_sparsity == True and identifier == 'grad':  # noqa: E712
        return True
    return False


def float_to_bfp_blocked(t, mant_bits, epsilon, rounding_mode, device, block_size,
                         num_format, weight_mant_bits, in_sparsity, w_sparsity, grad_sparsity,
                         sparsity_frac, N, M, sparsity_num_format, first, sparsity_mode, identifier='', sgd_update=False,
                         mx_w_elem_format='', mx_a_elem_format='', scale_bits=0, bfloat=0):
    """reference: bfp_ops.py:124-149.  Structured sparsity + 'bfp' (or 'fp32') runs as ONE fused
    kernel launch in either order; everything else composes the same steps the reference does."""
    assert (num_format == 'bfp')
    assert (((sparsity_num_format == 'bfp') and (block_size > 0)) or (sparsity_num_format == 'fp32') or (sparsity_num_format == 'int'))

    sparsity = _select_sparsity(in_sparsity, w_sparsity, grad_sparsity, identifier)

    if sparsity and sparsity_mode == 'structured' and sparsity_num_format == 'bfp':
        assert ((N > 0) and (M > 0) and (N <= M))
        native.require_device_tensor(t)
        mb = weight_mant_bits if sgd_update else mant_bits
        return _quantize_nm_ref_dtype(t, block_size, mb, epsilon, rounding_mode, N=N if N < M else 0, M=M if N < M else 0,
                                      sparsify_first=(first == 's'))

    if sparsity and sparsity_mode == 'unstructured' and sparsity_num_format == 'bfp' and first == 's':
        # global threshold (radix select), then prune + quantize in ONE pass over the tensor
        assert (sparsity_frac > 0)
        native.require_device_tensor(t)
        if t.numel() == 0:
            return t.clone()
        k = native.prune_count(t, sparsity_frac)
        mb = weight_mant_bits if sgd_update else mant_bits
        ws = _workspace(t.device)
        if rounding_mode == rounding_modes.DETERM:
            # one entry point: selection launch + fused prune + quantize launch
            return native.prune_quantize(t, k, ws, block_size, mb, epsilon).view(t.shape)
        native.select_threshold(t, k, ws)
        y, _, _ = native.quantize_threshold(t, ws, block_size, mb, epsilon, stoch_seed=_seed_for(rounding_mode))
        return _stoc_dtype(y.view(t.shape), rounding_mode)

    if first == 's':
        sparse_t = _sparsify(t, sparsity, sparsity_mode, device, N, M, sparsity_frac)
        return _quantize(sparse_t, sparsity_num_format, block_size, mant_bits, weight_mant_bits, sgd_update, epsilon, rounding_mode, device, identifier)
    else:
        quant_t = _quantize(t, sparsity_num_format, block_size, mant_bits, weight_mant_bits, sgd_update, epsilon, rounding_mode, device, identifier)
        return _sparsify(quant_t, sparsity, sparsity_mode, device, N, M, sparsity_frac)


# ---- additive public surface (no counterpart in the reference) -------------------------------
def _list_form(a, sparsity, sgd_update):
    """the list entry point of the library that computes configuration `a` (unpacked) for a list of tensors: 'prune' for
    s-first unstructured pruning then HBFP, round-half-even (native.PruneQuantizeList: prune int(numel * frac) elements);
    'fused' for HBFP with structured or no pruning, round-half-even (native.FastQuant's list call); None: the per-tensor call"""
    if (sgd_update or a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp' or a['rounding_mode'] != rounding_modes.DETERM
            or not a['block_size'] > 0):
        return None
    if not sparsity or (a['sparsity_mode'] == 'structured' and 0 < a['N'] <= a['M']):
        return 'fused'
    if a['sparsity_mode'] == 'unstructured' and a['first'] == 's' and a['sparsity_frac'] > 0:
        return 'prune'
    return None


def _by_device_dtype(tensors):
    """the indices of `tensors` per (device, dtype), groups in order of first appearance"""
    groups = {}
    for i, t in enumerate(tensors):
        native.require_device_tensor(t)
        groups.setdefault((t.device, t.dtype), []).append(i)
    return list(groups.values())


def _list_quant(a, sparsity):
    """the FastQuant plan of a 'fused' configuration"""
    nm = sparsity and a['N'] < a['M']
    return _fast_quant(a['block_size'], a['mant_bits'], a['epsilon'], a['N'] if nm else 0, a['M'] if nm else 0, a['first'] == 's')


def _prune_list(tensors, a):
    """the PruneQuantizeList of a 'prune' configuration for tensors of one device and dtype"""
    ks = [native.prune_count(t, a['sparsity_frac']) for t in tensors]
    return native.PruneQuantizeList(tensors, ks, a['block_size'], a['mant_bits'], a['epsilon'])


MANY_LANES = 3                       # streams a list of tensors without a list kernel is dealt to (the current one + side streams)
MANY_LANES_MIN_BYTES = 24 << 20      # ... when at least two of its tensors are this large (smaller ones: the host call costs more than it hides)


def _many_over_streams(tensors, fn):
    """[fn(t) for t in tensors] for configurations that have no list form in the library (several launches per tensor: quantize-first
    unstructured pruning, stochastic rounding, the 'int' format, N:8 on ragged rows ...).  The calls are independent, so large device
    tensors are dealt round-robin to MANY_LANES streams -- one tensor's launch boundaries, ramps and tails beside the other tensors'
    streaming, as the library's own list calls do it (native.PruneQuantizeList) -- with one fork and one join around the list."""
    big = [t for t in tensors if t.device.type == "cuda" and t.numel() * t.element_size() >= MANY_LANES_MIN_BYTES]
    if MANY_LANES < 2 or len(big) < 2 or len({t.device for t in big}) != 1 or any(t.device != big[0].device for t in tensors):
        return [fn(t) for t in tensors]
    return native._deal_over_streams(big[0].device, tensors, MANY_LANES, lambda _, t: fn(t))


def float_to_bfp_blocked_many(tensors, identifier='', **bfp_args):
    """float_to_bfp_blocked (bfp_ops.py:124-149) for a LIST of tensors with one configuration -- e.g. every Linear weight of
    a model -- in as few launches as possible: one per 64 tensors per dtype/device for the 'bfp' format with structured or no
    pruning and round-half-even (large tensors: a launch each, spread over two streams); for unstructured pruning before
    quantization, two launches per tensor over four independent lanes (native.PruneQuantizeList, issued eagerly); anything else
    is the per-tensor call, large tensors dealt to a few streams (_many_over_streams).  Returns the list of results in order."""
    a = unpack_bfp_args(dict(bfp_args))
    sgd_update = bool(bfp_args.get('sgd_update'))
    tensors = list(tensors)
    sparsity = _select_sparsity(a['in_sparsity'], a['w_sparsity'], a['grad_sparsity'], identifier)
    form = _list_form(a, sparsity, sgd_update)
    if form is None:
        return _many_over_streams(tensors, lambda t: float_to_bfp_blocked(t, **a, identifier=identifier, sgd_update=sgd_update))
    out = [None] * len(tensors)
    for idx in _by_device_dtype(tensors):
        ts = [tensors[i] for i in idx]
        ys = _prune_list([t.contiguous() for t in ts], a).run(graph=False) if form == 'prune' else _list_quant(a, sparsity).many(ts)
        for i, y in zip(idx, ys):
            out[i] = y.view(tensors[i].shape)
    return out


class PreparedMany:
    """float_to_bfp_blocked_many with the per-call host work done once: run() re-quantizes the bound tensors (whose storage
    must stay put, e.g. a model's weights) into the same output tensors -- one launch per 64 tensors (structured / dense), or
    the four-lane pipeline of the unstructured path (a hipGraph of it from PruneQuantizeList.GRAPH_FROM tensors on); one ctypes
    call per dtype/device group."""

    def __init__(self, tensors, identifier='', **bfp_args):
        a = unpack_bfp_args(dict(bfp_args))
        self.tensors = list(tensors)
        self._args, self._ident, self._sgd_update = a, identifier, bool(bfp_args.get('sgd_update'))
        sparsity = _select_sparsity(a['in_sparsity'], a['w_sparsity'], a['grad_sparsity'], identifier)
        form = _list_form(a, sparsity, self._sgd_update)
        self._groups = None
        if form is not None:
            self._groups = []
            for idx in _by_device_dtype(self.tensors):
                ts = [self.tensors[i] for i in idx]
                self._groups.append((idx, _prune_list(ts, a) if form == 'prune' else _list_quant(a, sparsity).prepare(ts)))

    def run(self):
        if self._groups is None:
            return [float_to_bfp_blocked(t, **self._args, identifier=self._ident, sgd_update=self._sgd_update) for t in self.tensors]
        out = [None] * len(self.tensors)
        for idx, prep in self._groups:
            for i, y in zip(idx, prep.run()):
                out[i] = y.view(self.tensors[i].shape)
        return out


def sparsify(t, sparsity_mode, N=0, M=0, sparsity_frac=0):
    """public alias of _sparsify with sparsity=True"""
    return _sparsify(t, True, sparsity_mode, str(t.device), N, M, sparsity_frac)


def code_bits_for(mant_bits):
    """the code width that holds a sign and `mant_bits` mantissa bits: 4, 8 or 16"""
    return 4 if mant_bits <= 3 else (8 if mant_bits <= 7 else 16)


def float_to_bfp_packed(t, mant_bits, block_size, epsilon=1e-8, N=0, M=0, first='s', code_bits=None, with_dequant=False):
    """Packed HBFP: integer mantissas (two's complement, 4/8/16 bits; 4-bit = two per byte, low nibble
    first) + one int8 shared exponent per block, value = code * 2**(exp - mant_bits).  N:M pruning is
    implied by zero codes.  Returns (codes, exps) or (codes, exps, dequantised)."""
    native.require_device_tensor(t)
    if code_bits is None:
        code_bits = code_bits_for(mant_bits)
    deq, codes, exps = native.quantize_nm(t, block_size, mant_bits, epsilon, N=N, M=M, sparsify_first=(first == 's'),
                                          want_deq=with_dequant, code_bits=code_bits, want_exp=True)
    return (codes, exps, deq.view(t.shape)) if with_dequant else (codes, exps)


DECODE_TOKENS = 64           # up to this many tokens: the decode kernel (4-bit codes), and the int8 unit ahead of the block-scaled one
I8_MAX_TOKENS = 512          # 8-bit-code PackedBFPLinear: the int8 unit up to here; above, the other routes measured faster
CACHED_MX8_MIN_TOKENS = 32   # the cached BFPLinear(matrix_unit=True) takes the block-scaled route from here on (a tile row)
# blocks 16 and 32, by (block, activation dtype): PackedBFP.linear and PackedBFPLinear take the int8 unit up to this many tokens (None: any
# number), measured against the fake route on the OPT-125m and ViT-L shapes (profiles/r06_i8gemm_b16.json / _b32.json): fp32 wins
# at every measured count, bf16 up to 16 (block 16) / 197 (block 32) tokens; fp16 takes the bf16 limits, as does a dtype not listed
I8_SMALL_BLOCK_MAX_TOKENS = {(16, torch.float32): None, (32, torch.float32): None,
                             (16, torch.bfloat16): 16, (32, torch.bfloat16): 197, (16, torch.float16): 16, (32, torch.float16): 197}


# hold_image=False: the codes-operand GEMM (native.hbfp_linear_mx4w) runs the 'mx8' route of a 4-bit weight, except where it did not beat the other
# image-free route (dequantize per call + library GEMM) by more than the run-to-run spread: from this many tokens on, for weights of up to
# this many elements (profiles/r10_prefill_codes.json: q_proj [4096, 4096] at 8192 tokens 190.2 against 192.2 us, spread 9.8; every other
# measured shape -- 128..2048 tokens, and gate_proj / down_proj at 8192 -- 7..66 % faster)
CODES_FAKE_MIN_TOKENS, CODES_FAKE_MAX_WEIGHT = 8192, 4096 * 4096
# time of a hold_image=False forward over the hold_image=True forward (image already made), bf16 HBFP4 x HBFP4, LLaMA-7B projections, at
# 128 / 512 / 2048 / 8192 tokens (same file; the spread of the image route against itself is 1-5 % there)
HOLD_IMAGE_TIME = {'gate_proj': (1.40, 1.73, 1.46, 1.19), 'down_proj': (1.13, 1.51, 1.65, 1.07), 'q_proj': (1.14, 1.35, 1.63, 1.27)}


def codes_route(T, N, K):
    """what the 'mx8' route of a 4-bit block-64 weight runs with hold_image=False: 'mx4w' (native.hbfp_linear_mx4w) or 'fake'"""
    return 'fake' if T >= CODES_FAKE_MIN_TOKENS and N * K <= CODES_FAKE_MAX_WEIGHT else 'mx4w'


def i8_small_block_max_tokens(block_size, dtype):
    """I8_SMALL_BLOCK_MAX_TOKENS of this block and activation dtype (dtype None or not listed: the bf16 entry)"""
    return I8_SMALL_BLOCK_MAX_TOKENS.get((block_size, dtype), I8_SMALL_BLOCK_MAX_TOKENS[(block_size, torch.bfloat16)])


def linear_route(T, N, K, code_bits, w_mant_bits, x_mant_bits, decode_tokens=DECODE_TOKENS, i8_max_tokens=0, mx8_min_tokens=1,
                 block_size=64, dtype=None):
    """Which kernel runs F.linear(Q_in(x), W) for T tokens, W [N, K] packed with `code_bits`-bit codes: 'empty' (nothing to launch),
    'decode4' (PackedBFP.linear_decode), 'int8' (native.hbfp_linear_i8), 'mx8' (native.hbfp_linear_mx8) or 'fake' (the fake-quantised
    activation times the dequantised weight).  The consumer's options: decode_tokens; i8_max_tokens, up to how many tokens 8-bit codes
    run on the int8 unit (0: never, None: no limit; past decode_tokens 'mx8' goes first); mx8_min_tokens (None: never 'mx8').
    Blocks 16 and 32 have one matrix-unit route, the int8 unit (4-bit codes through their int8 expansion): i8_max_tokens=None takes it at
    any token count (the cached forward, as at block 64), any other value up to i8_small_block_max_tokens(block_size, dtype), dtype being
    the activation's; decode_tokens and mx8_min_tokens apply to block 64 only."""
    if T == 0:
        return 'empty'
    if block_size in native.I8_BLOCKS:
        lim = None if i8_max_tokens is None else i8_small_block_max_tokens(block_size, dtype)
        if code_bits in (4, 8) and (lim is None or T <= lim) and native.hbfp_linear_i8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size):
            return 'int8'
        return 'fake'
    if code_bits == 4 and block_size == 64 and T <= decode_tokens and N % 16 == 0 and K % 256 == 0:
        return 'decode4'
    mx8_allowed = code_bits in (4, 8) and mx8_min_tokens is not None and T >= mx8_min_tokens
    int8 = code_bits == 8 and (i8_max_tokens is None or T <= i8_max_tokens)
    mx8 = None
    if int8 and T > decode_tokens:
        mx8 = mx8_allowed and native.hbfp_linear_mx8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size)
        int8 = not mx8
    if int8 and native.hbfp_linear_i8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size):
        return 'int8'
    if mx8 is None:
        mx8 = mx8_allowed and native.hbfp_linear_mx8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size)
    return 'mx8' if mx8 else 'fake'


PACKED_BLOCKS = (64, 32, 16)  # the blocks PackedBFP.from_bfp_args packs (16 and 32 run on the int8 unit only)


class PackedBFP:
    """A tensor in packed HBFP form: integer mantissas + one int8 exponent per block (+ what is needed to
    decode it).  N:M / unstructured pruning needs no extra field: pruned elements are zero codes."""

    def __init__(self, codes, exps, shape, dtype, mant_bits, block_size, code_bits):
        self.codes, self.exps = codes, exps
        self.shape, self.dtype = tuple(shape), dtype
        self.mant_bits, self.block_size, self.code_bits = int(mant_bits), int(block_size), int(code_bits)

    @classmethod
    def quantize(cls, t, mant_bits, block_size, epsilon=1e-8, N=0, M=0, first='s', code_bits=None):
        if code_bits is None:
            code_bits = code_bits_for(mant_bits)
        codes, exps = float_to_bfp_packed(t, mant_bits, block_size, epsilon, N, M, first, code_bits)
        return cls(codes, exps, t.shape, t.dtype, mant_bits, block_size, code_bits)

    @classmethod
    def quantize_unstructured(cls, t, mant_bits, block_size, sparsity_frac, epsilon=1e-8, code_bits=None):
        """packed Q(S_unstructured(t)) -- global magnitude pruning of int(numel * frac) elements, then HBFP (the reference's
        float_to_bfp_blocked with sparsity_mode 'unstructured', first 's': bfp_ops.py:61-71, 141-144) -- in the three launches of the
        unstructured path, the last one writing codes + exponents instead of the tensor"""
        native.require_device_tensor(t)
        if code_bits is None:
            code_bits = code_bits_for(mant_bits)
        assert sparsity_frac > 0
        k = native.prune_count(t, sparsity_frac)
        ws = _workspace(t.device)
        native.select_threshold(t, k, ws)
        _, codes, exps = native.quantize_threshold(t, ws, block_size, mant_bits, epsilon, want_deq=False, code_bits=code_bits, want_exp=True)
        return cls(codes, exps, t.shape, t.dtype, mant_bits, block_size, code_bits)

    @classmethod
    def from_bfp_args(cls, w, a, code_bits=None):
        """the weight operand Q_w(w) of configuration `a` (unpacked bfp_args), packed: format 'bfp', block 64, 32 or 16, mant_bits 1..7,
        round-half-even; N:M pruning from the w_sparsity keys (order from `first`), unstructured pruning for first='s' (prune, then
        quantize: one fused launch writes the codes).  Configurations that cannot be packed (unstructured pruning after quantization,
        stochastic rounding) are refused.  code_bits: the code width, code_bits_for(mant_bits) by default."""
        assert a['num_format'] == 'bfp' and a['sparsity_num_format'] == 'bfp' and a['block_size'] in PACKED_BLOCKS and 1 <= a['mant_bits'] <= 7, \
            "a packed weight holds 4- or 8-bit codes: an HBFP config with block_size 64, 32 or 16 and mant_bits <= 7 (HBFP2-HBFP8)"
        if a['w_sparsity'] and a['sparsity_mode'] == 'unstructured' and a['first'] != 's':
            raise ValueError("unstructured pruning AFTER quantization (first='q') is not packed")
        if a['w_sparsity'] and a['sparsity_mode'] not in ('structured', 'unstructured'):
            raise ValueError('Sparsity mode not implemented')
        if a['rounding_mode'] != 'determ':
            raise ValueError("a packed weight is quantized with round-half-even: rounding_mode must be 'determ'")
        if a['w_sparsity'] and a['sparsity_mode'] == 'unstructured':
            return cls.quantize_unstructured(w, a['mant_bits'], a['block_size'], a['sparsity_frac'], a['epsilon'], code_bits)
        N, M = (a['N'], a['M']) if a['w_sparsity'] else (0, 0)                  # (structured: the other modes returned or raised above)
        return cls.quantize(w, a['mant_bits'], a['block_size'], a['epsilon'], N, M, a['first'], code_bits)

    def dequantize(self, out=None):
        """== the reference's fake-quantised tensor (a -0.0 there is +0.0 here)"""
        cols = self.shape[-1] if len(self.shape) else 1
        return native.dequantize(self.codes, self.exps, cols, self.dtype, self.block_size, self.mant_bits, self.code_bits,
                                 out=None if out is None else out.view(-1, cols)).view(self.shape)

    def nbytes(self):
        return self.codes.numel() * self.codes.element_size() + self.exps.numel()

    def resident_bytes(self):
        """bytes this weight holds on its device right now: codes, exponents and every derived copy that is alive -- the MFMA-tiled copy
        of the decode kernel (`_tiles`, made by the first forward of <= 64 tokens), the int8 expansion of 4-bit codes (`_i8`) and the
        e4m3 / E8M0 image of the block-scaled GEMM (`_mx8`, made by the first prefill unless hold_image=False)"""
        n = self.nbytes()
        for name in ("_tiles", "_i8", "_mx8"):
            held = getattr(self, name, None)
            if held is not None:
                n += sum(t.numel() * t.element_size() for t in (held if isinstance(held, (tuple, list)) else (held,)))
        return n

    def linear_decode(self, x, x_mant_bits=7, epsilon=1e-8, x_sparsity=None, xq=None):
        """x @ W^T for <= 64 tokens straight from the packed weight (self is W [N, K], 4-bit codes, block 64, N % 16 == 0,
        K % 128 == 0, K >= 256), in one launch on an MFMA-tiled copy of the weight made once (native.hbfp_linear_decode_tiled):
        the activation is quantized to HBFP(x_mant_bits + 1) block 64 and every block's dot product is an exact
        integer sum on the int8 matrix cores.  x_sparsity (native.ActSparsity): the activation
        is pruned as well (unstructured: one threshold over all of x).  xq: its operand made beforehand (native.act_codes)."""
        assert self.code_bits == 4 and self.block_size == 64 and len(self.shape) == 2
        N, K = self.shape
        if not (N % 16 == 0 and K % 128 == 0 and K >= 256):
            raise ValueError(f"linear_decode needs N % 16 == 0, K % 128 == 0 and K >= 256 (got N={N}, K={K})")
        if xq is None and x_sparsity is not None:
            xq = native.act_codes(x.reshape(-1, K), x_mant_bits, epsilon, x_sparsity)
        if getattr(self, "_tiles", None) is None:
            self._tiles = native.mfma_tiles(self.codes, self.exps)
        return native.hbfp_linear_decode_tiled(x, self._tiles[0], self._tiles[1], N, self.mant_bits, x_mant_bits, epsilon, xq=xq)

    def linear(self, x, bias=None, x_mant_bits=7, epsilon=1e-8, decode_tokens=DECODE_TOKENS, x_sparsity=None, hold_image=True):
        """F.linear(Q_in(x), W_packed, bias) for any number of tokens, W = self [N, K] (the forward of a BFPLinear whose
        weight is held packed; activations HBFP(x_mant_bits + 1), block 64, round-half-even), on the kernel linear_route picks:
        4-bit codes up to `decode_tokens` tokens straight from the codes (linear_decode); else the block-scaled matrix instruction
        where both operands' mantissas fit 4 bits; else the weight decoded once per call and the library GEMM.
        x_sparsity (native.ActSparsity or None): the activation is pruned as the reference's in_sparsity does (N:M per row, or
        one unstructured threshold over ALL tokens of the call).
        hold_image=False: the 'mx8' route of 4-bit block-64 codes reads the codes themselves (native.hbfp_linear_mx4w) and the
        1.016 B per weight image is never made: same bits, 1.07-1.73 x the image route's
        time (bfp_ops.HOLD_IMAGE_TIME has the ratio per measured shape; codes_route: a small weight at >= 8192 tokens takes the
        dequantize + library GEMM route instead, which keeps no image either)."""
        K = self.shape[-1]
        T = x.numel() // K if K else 0
        route = linear_route(T, self.shape[0], K, self.code_bits, self.mant_bits, x_mant_bits, decode_tokens, block_size=self.block_size,
                             dtype=x.dtype)
        return self._run_linear(route, x, bias, x_mant_bits, epsilon, x_sparsity, hold_image)

    def _run_linear(self, route, x, bias, x_mant_bits, epsilon, x_sparsity, hold_image=True):
        """F.linear(Q_in(x), W_packed, bias) on `route` (a linear_route name); hold_image as in linear()"""
        if route == 'int8':
            return self.linear_i8(x, bias, x_mant_bits, epsilon, x_sparsity)
        N, K = self.shape[0], self.shape[-1]
        lead = x.shape[:-1]
        x2 = x.reshape(-1, K)
        if route == 'empty':
            return x.new_zeros(lead + (N,))
        if route == 'mx8' and not hold_image and self.code_bits == 4 and self.block_size == 64:
            route = codes_route(x2.shape[0], N, K)
        if route == 'mx4w':
            # the same GEMM with the codes and exponents themselves as the weight operand: nothing derived from the weight is kept
            return native.hbfp_linear_mx4w(x2, self.codes, self.exps, self.mant_bits, x_mant_bits, epsilon, bias=bias,
                                           act=x_sparsity).view(lead + (N,))
        if route == 'mx8':
            # both operands as e4m3 mantissas + E8M0 block scales on the block-scaled matrix instruction (exact block dot products,
            # fp32 across blocks, bias fused); the weight's image is made once per device
            return native.hbfp_linear_mx8(x2, *self._mx8_image(), x_mant_bits, epsilon, bias=bias, act=x_sparsity).view(lead + (N,))
        if route == 'decode4':
            xq = None if x_sparsity is None else native.act_codes(x2, x_mant_bits, epsilon, x_sparsity)   # (all tokens: one threshold)
            out = self.linear_decode(x2, x_mant_bits, epsilon, xq=xq)
        else:
            out = F.linear(_act_fake_quant(x2, x_mant_bits, epsilon, x_sparsity, self.block_size), self.dequantize().to(x.dtype))
        if bias is not None:
            out = out + bias
        return out.view(lead + (N,))

    def linear_i8(self, x, bias=None, x_mant_bits=7, epsilon=1e-8, x_sparsity=None):
        """F.linear(Q_in(x), W_packed, bias) for any number of tokens on the int8 matrix unit (native.hbfp_linear_i8): self is W [N, K]
        with 4- or 8-bit codes, block 64, 32 or 16, mant_bits 1..7; activations HBFP(x_mant_bits + 1), x_mant_bits 1..7, the weight's
        block, round-half-even, pruned by x_sparsity (native.ActSparsity or None) as in linear().  Every block product is an exact integer
        sum, fp32 across blocks.  4-bit codes are expanded to int8 codes once per device (kept with the weight)."""
        assert self.code_bits in (4, 8) and self.block_size in PACKED_BLOCKS and len(self.shape) == 2, \
            "linear_i8 takes a 2-D weight with 4- or 8-bit codes and block 64, 32 or 16"
        N, K = self.shape
        lead = x.shape[:-1]
        x2 = x.reshape(-1, K)
        if x2.shape[0] == 0:
            return x.new_zeros(lead + (N,))
        out = native.hbfp_linear_i8(x2, self._i8_codes(), self.exps, self.mant_bits, x_mant_bits, epsilon, bias=bias, act=x_sparsity,
                                    block_size=self.block_size)
        return out.view(lead + (N,))

    def _i8_codes(self):
        """the weight's codes as int8 [N, K]: the codes themselves (code_bits 8), or their one-time expansion (code_bits 4)"""
        if self.code_bits == 8:
            return self.codes
        if getattr(self, "_i8", None) is None or self._i8.device != self.codes.device:
            self._i8 = native.codes4_to_i8(self.codes, self.shape[0] * self.shape[1]).view(self.shape)
        return self._i8

    def _mx8_image(self):
        if getattr(self, "_mx8", None) is None or self._mx8[0].device != self.codes.device:
            self._mx8 = native.mx8_from_hbfp(self.codes, self.exps, self.shape[-1], self.mant_bits, self.code_bits)
        return self._mx8

    def save(self, path, compact24=False):
        """safetensors file: tensors `codes`, `exps`; the rest as string metadata.  compact24=True stores a 2:4-sparse
        4-bit tensor as 2 nibbles + 2 x 2-bit positions per group of 4 (`vals`, `idx`: 0.375 B/element instead of 0.5)."""
        from safetensors.torch import save_file
        meta = dict(format="hbfp-packed-v1", shape=",".join(str(d) for d in self.shape), dtype=str(self.dtype).replace("torch.", ""),
                    mant_bits=str(self.mant_bits), block_size=str(self.block_size), code_bits=str(self.code_bits))
        if compact24:
            assert self.code_bits == 4 and self.codes.numel() % 4 == 0
            vals, idx = native.compact24(self.codes)
            meta["layout"] = "compact24"
            meta["codes_shape"] = ",".join(str(d) for d in self.codes.shape)
            save_file({"vals": vals.cpu(), "idx": idx.cpu(), "exps": self.exps.cpu().contiguous()}, path, metadata=meta)
            return
        save_file({"codes": self.codes.cpu().contiguous(), "exps": self.exps.cpu().contiguous()}, path, metadata=meta)

    @classmethod
    def load(cls, path, device="cuda"):
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as f:
            meta = f.metadata()
            assert meta.get("format") == "hbfp-packed-v1", meta
            exps = f.get_tensor("exps")
            if meta.get("layout") == "compact24":
                cshape = tuple(int(d) for d in meta["codes_shape"].split(","))
                codes = native.expand24(f.get_tensor("vals").to(device), f.get_tensor("idx").to(device)).view(cshape)
            else:
                codes = f.get_tensor("codes")
        shape = tuple(int(d) for d in meta["shape"].split(",")) if meta["shape"] else ()
        return cls(codes.to(device), exps.to(device), shape, getattr(torch, meta["dtype"]), int(meta["mant_bits"]),
                   int(meta["block_size"]), int(meta["code_bits"]))


SP24_DECODE_TOKENS = 64      # SparseBFP24.linear: up to this many tokens the sp24 kernel, more a transient expansion


def sp24_config_check(a):
    """raise ValueError unless configuration `a` (unpacked bfp_args) guarantees what the sp24 form holds: HBFP block 64, mant_bits 1..7,
    round-half-even, weights pruned N:M with M == 4 and N <= 2 (either order: at most N non-zeros in every group of 4 along K)"""
    if a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp' or a['block_size'] != 64 or not 1 <= a['mant_bits'] <= 7:
        raise ValueError("sp24 holds HBFP block-64 weights with mant_bits 1..7 (got num_format=%r, block_size=%r, mant_bits=%r)"
                         % (a['num_format'], a['block_size'], a['mant_bits']))
    if a['rounding_mode'] != 'determ':
        raise ValueError("an sp24 weight is quantized with round-half-even: rounding_mode must be 'determ'")
    if not a['w_sparsity'] or a['sparsity_mode'] != 'structured' or int(a['M']) != 4 or not 0 < int(a['N']) <= 2:
        raise ValueError("sp24 needs structured weight pruning N:4 with N <= 2 (got w_sparsity=%r, sparsity_mode=%r, N:M=%r:%r)"
                         % (a['w_sparsity'], a['sparsity_mode'], a.get('N'), a.get('M')))


class SparseBFP24:
    """A 2:4 (or 1:4) pruned HBFP weight [N, K] held compressed: the two kept 4- or 8-bit codes of every group of 4 along K (`vals`),
    their 2-bit positions (`idx`) and the [N, K/64] int8 block exponents of the dense packed weight (`exps`): 0.391 B per weight for
    4-bit codes, 0.641 B for 8-bit codes (native.sp24_nbytes; layout in csrc/bfpq_sp24.hip).  linear() runs up to SP24_DECODE_TOKENS
    tokens on the sparse int8 matrix instruction straight from this form; more tokens expand the weight, for that call only, to the
    operand the dense PackedBFP route of the same token count reads, and run that route.  No dense copy is kept."""
    block_size = 64

    def __init__(self, vals, idx, exps, shape, dtype, mant_bits, code_bits):
        self.vals, self.idx, self.exps = vals, idx, exps
        self.shape, self.dtype = tuple(shape), dtype
        self.mant_bits, self.code_bits = int(mant_bits), int(code_bits)

    @classmethod
    def from_packed(cls, p):
        """the sp24 form of a 2-D PackedBFP (block 64, 4- or 8-bit codes); ValueError if some group of 4 holds more than 2 non-zeros"""
        if p.block_size != 64 or p.code_bits not in (4, 8) or len(p.shape) != 2:
            raise ValueError("sp24 holds 2-D block-64 weights of 4- or 8-bit codes")
        N, K = p.shape
        if not native.sp24_shape_ok(N, K):
            raise ValueError(f"sp24 needs N % 16 == 0 and K % 64 == 0 (got N={N}, K={K})")
        vals, idx = native.sp24_pack(p.codes, N, K, p.code_bits)
        return cls(vals, idx, p.exps.contiguous(), p.shape, p.dtype, p.mant_bits, p.code_bits)

    @classmethod
    def from_bfp_args(cls, w, a):
        """Q_w(w) of configuration `a` (unpacked bfp_args) in sp24 form.  Only configurations that guarantee the pattern are taken
        (sp24_config_check); anything else raises ValueError.  The dense packed weight is made, compressed and dropped."""
        sp24_config_check(a)
        N, K = w.shape
        if not native.sp24_shape_ok(N, K):
            raise ValueError(f"sp24 needs N % 16 == 0 and K % 64 == 0 (got N={N}, K={K})")
        return cls.from_packed(PackedBFP.from_bfp_args(w, a))

    def to_packed(self):
        """the dense PackedBFP (codes of the same width; a new tensor, not kept here)"""
        N, K = self.shape
        return PackedBFP(native.sp24_unpack(self.vals, self.idx, N, K, self.code_bits), self.exps, self.shape, self.dtype, self.mant_bits,
                         64, self.code_bits)

    def dequantize(self, out=None):
        return self.to_packed().dequantize(out)

    def nbytes(self):
        return self.vals.numel() + self.idx.numel() + self.exps.numel()

    def linear(self, x, bias=None, x_mant_bits=7, epsilon=1e-8, x_sparsity=None, decode_tokens=None):
        """F.linear(Q_in(x), W, bias), W = self, activations HBFP(x_mant_bits + 1) block 64 round-half-even, pruned by x_sparsity
        (native.ActSparsity or None) as PackedBFP.linear does.  Up to decode_tokens (default SP24_DECODE_TOKENS) tokens:
        native.hbfp_linear_sp24.  More: the route PackedBFPLinear.forward takes for the same call (linear_route), on a transient
        expansion of the weight -- int8 codes for 'int8', the dense codes (whose e4m3 image or dequantised weight that route makes)
        for the others -- freed when the call returns."""
        N, K = self.shape
        T = x.numel() // K if K else 0
        lead = x.shape[:-1]
        if T == 0:
            return x.new_zeros(lead + (N,))
        lim = SP24_DECODE_TOKENS if decode_tokens is None else decode_tokens
        if T <= lim and native.hbfp_linear_sp24_ok(T, N, K, self.code_bits, self.mant_bits, x_mant_bits):
            return native.hbfp_linear_sp24(x.reshape(T, K), self.vals, self.idx, self.exps, N, self.code_bits, self.mant_bits, x_mant_bits,
                                           epsilon, bias=bias, act=x_sparsity).view(lead + (N,))
        route = linear_route(T, N, K, self.code_bits, self.mant_bits, x_mant_bits, i8_max_tokens=I8_MAX_TOKENS, block_size=64, dtype=x.dtype)
        if route == 'int8':
            c8 = native.sp24_unpack(self.vals, self.idx, N, K, self.code_bits, codes=self.code_bits == 8, codes8=self.code_bits == 4)
            return native.hbfp_linear_i8(x.reshape(T, K), c8, self.exps, self.mant_bits, x_mant_bits, epsilon, bias=bias,
                                         act=x_sparsity).view(lead + (N,))
        return self.to_packed()._run_linear(route, x, bias, x_mant_bits, epsilon, x_sparsity)

    def save(self, path):
        """safetensors file: tensors `vals`, `idx`, `exps`; the rest as string metadata"""
        from safetensors.torch import save_file
        meta = dict(format="hbfp-sp24-v1", shape=",".join(str(d) for d in self.shape), dtype=str(self.dtype).replace("torch.", ""),
                    mant_bits=str(self.mant_bits), block_size="64", code_bits=str(self.code_bits))
        save_file({"vals": self.vals.cpu().contiguous(), "idx": self.idx.cpu().contiguous(), "exps": self.exps.cpu().contiguous()}, path,
                  metadata=meta)

    @classmethod
    def load(cls, path, device="cuda"):
        """a file of save(), or a PackedBFP.save file (compact24 or dense codes): its codes are expanded and compressed on the device,
        and only the sp24 form is kept"""
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as f:
            meta = f.metadata()
            if meta.get("format") == "hbfp-sp24-v1":
                shape = tuple(int(d) for d in meta["shape"].split(","))
                return cls(f.get_tensor("vals").to(device), f.get_tensor("idx").to(device), f.get_tensor("exps").to(device), shape,
                           getattr(torch, meta["dtype"]), int(meta["mant_bits"]), int(meta["code_bits"]))
        return cls.from_packed(PackedBFP.load(path, device))


def _act_fake_quant(x, mant_bits, epsilon, act=None, block_size=64):
    """the reference's activation operand: float_to_bfp_blocked(x, identifier='in') with HBFP(mant_bits + 1), blocks of block_size,
    round-half-even, pruned as the ActSparsity spec `act` says (None: dense)"""
    mode, N, M, frac, first = act if act is not None else ('structured', 0, 0, 0.0, 's')
    return float_to_bfp_blocked(x, mant_bits=mant_bits, epsilon=epsilon, rounding_mode=rounding_modes.DETERM, device=str(x.device), block_size=block_size,
                                num_format='bfp', weight_mant_bits=0, in_sparsity=act is not None, w_sparsity=False, grad_sparsity=False,
                                sparsity_frac=frac, N=N, M=M, sparsity_num_format='bfp', first=first, sparsity_mode=mode, identifier='in')


# ---- module / functional wrappers (reference: bfp_ops.py:151-287) -----------------------------
def MxM_pre_processing(x, w, transpose, **bfp_args):
    """reference: bfp_ops.py:151-155 -- quantize both GEMM operands; with transpose the second operand is
    quantized along its contraction dim (blocks must run along K) and handed back in its original layout"""
    xq = float_to_bfp_blocked(x, **bfp_args, identifier='in')
    if transpose == True:  # noqa: E712
        wq = float_to_bfp_blocked(w.transpose(-1, -2), **bfp_args, identifier='w').transpose(-1, -2)
    else:
        wq = float_to_bfp_blocked(w, **bfp_args, identifier='w')
    return xq, wq


def _get_op_name(name, epsilon, mant_bits, rounding_mode, **kwargs):
    """reference: bfp_ops.py:157-158"""
    return '%s_BFP_%s_%d' % (name, rounding_mode, mant_bits)


FUSE_OPERAND_PAIR = True           # BFPLinear / BFPConv2d forward: quantize activation and weight in one launch when possible


def matrix_unit_value(matrix_unit):
    """WeightCache's matrix_unit switch, checked: False, True or 'int8' (anything else raises ValueError)"""
    if (isinstance(matrix_unit, str) or matrix_unit not in (True, False)) and matrix_unit != 'int8':
        raise ValueError(f"matrix_unit must be False, True or 'int8' (got {matrix_unit!r})")
    return 'int8' if matrix_unit == 'int8' else bool(matrix_unit)


_CACHE_KEYS = ('mant_bits', 'epsilon', 'rounding_mode', 'block_size', 'num_format', 'weight_mant_bits', 'w_sparsity',
               'sparsity_frac', 'N', 'M', 'sparsity_num_format', 'first', 'sparsity_mode')


class WeightCache:
    """Opt-in, INFERENCE-ONLY cache of the quantized (and sparsified) weight operand.  The reference re-runs the whole
    path on the unchanged weight in every forward (bfp_ops.py:151-166, 7 Linear layers per LLaMA block); with the cache an
    inference loop quantizes each weight once.  Off by default (reference semantics).
    Valid while (storage pointer, in-place version counter, dtype, device, shape, the configuration values that shape
    the weight operand) are unchanged.  It is BYPASSED whenever a stale entry could go unnoticed: while gradients are being
    recorded for the weight, or the owning module is in training mode (optimizers and EMA code update `p.data` in place,
    which does not bump the version counter), and for stochastic rounding.  After such an update in eval mode call
    invalidate()."""

    def __init__(self, module=None, matrix_unit=False):
        import weakref
        self.key = None
        self.value = None
        self.hits = 0
        self.misses = 0
        self._module = weakref.ref(module) if module is not None else None
        # matrix_unit: F.linear on the two fake-quantised operands is replaced by the block-scaled matrix instruction on their e4m3 + E8M0
        # images where the configuration allows it (same products and block sums, fp32 across blocks; see PackedBFP.linear); the weight's
        # image is cached like the fake-quantised weight, under the same key
        # matrix_unit='int8': the same for HBFP up to 8 bits (mant_bits <= 7) on the int8 matrix instruction (native.hbfp_linear_i8); the
        # cached image is then the weight's int8 codes + exponents
        self.matrix_unit = matrix_unit_value(matrix_unit)
        self.image_key = None
        self.image = None
        self.mx_calls = 0
        self.i8_calls = 0

    @staticmethod
    def _key(w, bfp_args):
        return (w.data_ptr(), native.tensor_version(w), w.dtype, w.device, tuple(w.shape), tuple(bfp_args.get(k) for k in _CACHE_KEYS))

    def usable(self, w, bfp_args):
        if bfp_args.get('rounding_mode') != rounding_modes.DETERM:
            return False
        if w.is_inference() or native.tensor_version(w) is None:
            return False                                     # no version counter: an in-place update could not be seen
        if torch.is_grad_enabled() and w.requires_grad:
            return False
        m = self._module() if self._module is not None else None
        return not (m is not None and m.training)

    def lookup(self, w, bfp_args):
        if not self.usable(w, bfp_args):
            return None
        if self.key == self._key(w, bfp_args):
            self.hits += 1
            return self.value.view_as(self.value)            # a fresh alias: the stored tensor never enters an autograd graph
        return None

    def store(self, w, wq, bfp_args=None):
        bfp_args = bfp_args or {}
        if bfp_args and not self.usable(w, bfp_args):
            return
        self.key = self._key(w, bfp_args)
        self.value = wq.detach()
        self.misses += 1

    def invalidate(self):
        self.key = None
        self.value = None
        self.image_key = None
        self.image = None
        native.forget_shared_images()

    def weight_image(self, w, bfp_args):
        """e4m3 + E8M0 image of Q_w(w) for the matrix unit, made from the packed codes of the weight (not from the fake-quantised
        tensor: HBFP quantization is not idempotent on a block whose maximum rounded down to a power of two)"""
        key = self._key(w, bfp_args)
        if self.image_key != key:
            pk = PackedBFP.from_bfp_args(w.detach(), bfp_args)
            self.image = native.mx8_from_hbfp(pk.codes, pk.exps, w.shape[-1], pk.mant_bits, pk.code_bits)
            self.image_key = key
        return self.image

    def weight_codes_i8(self, w, bfp_args):
        """int8 codes [N, K] + int8 exponents [N, K/block] of Q_w(w) for the int8 matrix unit (matrix_unit='int8'), kept under the same key"""
        key = self._key(w, bfp_args)
        if self.image_key != key:
            pk = PackedBFP.from_bfp_args(w.detach(), bfp_args, code_bits=8)
            self.image = (pk.codes.view(w.shape), pk.exps)
            self.image_key = key
        return self.image


def _pair_in_one_launch(x, w, bfp_args):
    """activation + weight of one Linear through ONE launch (native.FastQuant.many) when both take the drop-in kernel with
    the same plan: 'bfp' format, round-half-even, dense or structured pruning per operand; else None"""
    a = bfp_args
    if (a['sparsity_num_format'] != 'bfp' or a['rounding_mode'] != rounding_modes.DETERM or a['num_format'] != 'bfp'
            or not a['block_size'] > 0                        # (the asserting path says what the reference says, bfp_ops.py:130)
            or x.dtype != w.dtype or x.device != w.device or x.device.type != 'cuda' or torch.compiler.is_compiling()):
        return None
    sp_in, sp_w = a['in_sparsity'] == True, a['w_sparsity'] == True  # noqa: E712
    if (sp_in or sp_w):
        if a['sparsity_mode'] != 'structured' or not (0 < a['N'] <= a['M']):
            return None
    nm = (sp_in or sp_w) and a['N'] < a['M']
    f = _fast_quant(a['block_size'], a['mant_bits'], a['epsilon'], a['N'] if nm else 0, a['M'] if nm else 0, a['first'] == 's')
    xq, wq = f.many([x, w], [sp_in, sp_w])
    return xq.view(x.shape), wq.view(w.shape)


def _quantize_operands(x, w, transpose, bfp_args, cache):
    """(Q_in(x), Q_w(w)) -- reference MxM_pre_processing (bfp_ops.py:151-155), with the optional weight cache"""
    if cache is None or not cache.usable(w, bfp_args):
        if transpose != True and FUSE_OPERAND_PAIR:  # noqa: E712
            pair = _pair_in_one_launch(x, w, bfp_args)
            if pair is not None:
                return pair
        return MxM_pre_processing(x, w, transpose, **bfp_args)
    xq = float_to_bfp_blocked(x, **bfp_args, identifier='in')
    wq = cache.lookup(w, bfp_args)
    if wq is None:
        wq = _quantize_weight_operand(w, transpose, bfp_args)
        cache.store(w, wq, bfp_args)
    return xq, wq


class _OperandQuantizer(torch.autograd.Function):
    """forward: (x, w) -> (Q_in(x), Q_w(w)); backward: straight-through (reference NewOpIn, bfp_ops.py:163-170)"""

    @staticmethod
    def forward(ctx, x, w, transpose, bfp_args, cache):
        return _quantize_operands(x, w, transpose, bfp_args, cache)

    @staticmethod
    def backward(ctx, grad_x, grad_w):
        return grad_x, grad_w, None, None, None


def _quantize_weight_operand(w, transpose, bfp_args):
    """the second operand of MxM_pre_processing alone"""
    if transpose == True:  # noqa: E712
        return float_to_bfp_blocked(w.transpose(-1, -2), **bfp_args, identifier='w').transpose(-1, -2)
    return float_to_bfp_blocked(w, **bfp_args, identifier='w')


class _GradQuantizer(torch.autograd.Function):
    """forward: identity; backward: Q_grad(dL/dout) (reference NewOpOut, bfp_ops.py:175-182)"""

    @staticmethod
    def forward(ctx, out, bfp_args):
        ctx.bfp_args = bfp_args
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad_out):
        return float_to_bfp_blocked(grad_out, **ctx.bfp_args, identifier='grad'), None


def _pruning_ok(a, w_quantize_first):
    """the operand pruning the matrix-unit routes take: in_sparsity structured with 0 < N <= M or unstructured with 0 < sparsity_frac <= 1;
    w_sparsity N:M with M in (2, 4, 8) or unstructured -- prune-first only, unless w_quantize_first (the routes that make the weight's
    codes per call; the cached route's fused prune + quantize launch cannot prune after quantizing)"""
    if a['in_sparsity'] == True:  # noqa: E712
        if a['sparsity_mode'] == 'structured':
            if not (0 < a['N'] <= a['M']):
                return False
        elif a['sparsity_mode'] != 'unstructured' or not (0 < a['sparsity_frac'] <= 1):
            return False
    if a['w_sparsity'] == True:  # noqa: E712
        if a['sparsity_mode'] == 'unstructured':
            if not (0 < a['sparsity_frac'] <= 1) or not (w_quantize_first or a['first'] == 's'):
                return False
        elif a['sparsity_mode'] != 'structured' or not (0 < a['N'] <= a['M']) or a['M'] not in (2, 4, 8):
            return False
    return True


def _cached_route(x, w, a, cache):
    """linear_route of the cached Linear forward; anything but 'int8' or 'mx8' means the fake-quantize path.  matrix_unit=True: the
    block-scaled matrix instruction on the weight's e4m3 + E8M0 image (<= 4 mantissa bits, exact in e4m3; K % 256 == 0; from
    CACHED_MX8_MIN_TOKENS tokens, a tile row).  matrix_unit='int8': the int8 matrix instruction on its int8 codes (1..7 mantissa bits, any
    number of tokens, N % 16 == 0, K % 64 == 0; blocks 64, 32 and 16 alike).  Both need HBFP block 64 (or, for 'int8', 32 or 16), round-half-even, dense or pruned activations (structured with
    0 < N <= M, or unstructured), dense, N:M or prune-first unstructured weights and a 2-D weight."""
    int8 = cache.matrix_unit == 'int8'
    block_ok = a['block_size'] == 64 or (int8 and a['block_size'] in native.I8_BLOCKS)
    if (a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp' or not block_ok or not (1 <= a['mant_bits'] <= (7 if int8 else 4))
            or a['rounding_mode'] != rounding_modes.DETERM or w.dim() != 2 or x.device.type != 'cuda'
            or torch.compiler.is_compiling() or not cache.usable(w, a)):
        return 'fake'
    if not _pruning_ok(a, w_quantize_first=False):
        return 'fake'
    if a['w_sparsity'] == True and a['sparsity_mode'] == 'unstructured' and w.shape[-1] % 64:  # noqa: E712  (the fused prune + quantize launch writes the codes)
        return 'fake'
    K, m = x.shape[-1], a['mant_bits']
    T = x.numel() // K if K else 0
    if int8:
        return linear_route(T, w.shape[0], K, 8, m, m, decode_tokens=0, i8_max_tokens=None, mx8_min_tokens=None, block_size=a['block_size'])
    return linear_route(T, w.shape[0], K, code_bits_for(m), m, m, decode_tokens=0, mx8_min_tokens=CACHED_MX8_MIN_TOKENS)


class StocMatrixUnit:
    """Opt-in switch of a BFPLinear: its stochastically rounded ('stoc') inference forwards run on a matrix unit instead of F.linear on two
    fp32 operands.  Both operands are rounded with the seeds the fake route draws, straight into codes (native.stoc_codes); nothing is
    cached -- the reference draws fresh noise for the weight in every forward.  matrix_unit: True (the block-scaled unit where _stoc_route
    allows, else the int8 unit) or 'int8'.  stoc_mx_calls / stoc_i8_calls count the forwards each unit ran, fallbacks the calls redone on
    the fake route because a block's exponent could overflow the dtype."""

    def __init__(self, matrix_unit=True):
        self.matrix_unit = matrix_unit_value(matrix_unit)
        self.stoc_mx_calls = 0
        self.stoc_i8_calls = 0
        self.fallbacks = 0


# the stochastic matrix-unit route from this many tokens on, by operand dtype (None: never).  Measured against the fake 'stoc' route, both
# eager (the route reads a flag back per call), profiles/r07_stoc_linear.json: bf16 LLaMA-7B rows win from 512 tokens on (1.11-5.96x) and
# lose at 1-16 tokens (0.61-0.99x); fp32 OPT-125m rows lose at every count up to 2048 (0.61-0.90x).  A dtype not listed: the bf16 entry.
STOC_MIN_TOKENS = {torch.bfloat16: 512, torch.float32: None}


def _stoc_route(T, N, K, a, matrix_unit, dtype=None):
    """the GEMM of a 'stoc' forward of T tokens on an [N, K] weight under BFPLinear.enable_stochastic_matrix_unit(matrix_unit), for a
    configuration _stoc_eligible accepts, operands of `dtype`: 'mx8', 'int8' or 'fake'"""
    m, block = a['mant_bits'], a['block_size']
    lim = STOC_MIN_TOKENS.get(dtype, STOC_MIN_TOKENS[torch.bfloat16])
    if not matrix_unit or T < 1 or lim is None or T < lim:
        return 'fake'
    if (matrix_unit is True and T >= CACHED_MX8_MIN_TOKENS and block == 64 and m <= 4
            and native.hbfp_linear_mx8_ok(T, N, K, m, m, block)):
        return 'mx8'
    if native.hbfp_linear_i8_ok(T, N, K, m, m, block):
        return 'int8'
    return 'fake'


def _stoc_eligible(x, w, bias, a):
    """the forwards the stochastic matrix-unit route takes (the caller checks no_grad and the op): 'stoc', 'bfp' in both formats,
    blocks 64 / 32 / 16, 1..7 mantissa bits, bf16 or fp32 operands of one dtype on one ROCm device, a 2-D weight, no bias or an fp32
    one, pruning as the cached route takes it plus quantize-first unstructured weights"""
    if (a['rounding_mode'] != rounding_modes.STOC or a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp'
            or a['block_size'] not in (64,) + native.I8_BLOCKS or not (1 <= a['mant_bits'] <= 7)
            or w.dim() != 2 or x.dtype != w.dtype or x.dtype not in (torch.bfloat16, torch.float32)
            or x.device.type != 'cuda' or x.device != w.device or torch.compiler.is_compiling()
            or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())   # (the exponent check reads a flag back)
            or (bias is not None and bias.dtype != torch.float32)):
        return False
    return _pruning_ok(a, w_quantize_first=True)


def _weight_sparsity(a):
    """the weight operand's pruning as an ActSparsity (None: dense), as float_to_bfp_blocked(identifier='w') applies it"""
    if a['w_sparsity'] != True:  # noqa: E712
        return None
    return native.ActSparsity.from_bfp_args(dict(a, in_sparsity=True))


def _stoc_linear(x, w, bias, a, stoc):
    """F.linear(Q_in(x), Q_w(w), bias) of a 'stoc' forward on a matrix unit, or None when _stoc_route says 'fake' (nothing drawn then).
    The two seeds are drawn as the fake route draws them (activation first), so the operands are the fake route's, bit for bit, and
    torch's generator ends where it would.  A block whose exponent could overflow the dtype redoes the call on the fake route with the
    same seeds (one flag read back per call)."""
    if not _stoc_eligible(x, w, bias, a):
        return None
    N, K = w.shape
    x2 = x.reshape(-1, K)
    T = x2.shape[0]
    route = _stoc_route(T, N, K, a, stoc.matrix_unit, x.dtype)
    if route == 'fake':
        return None
    m, eps, block = a['mant_bits'], a['epsilon'], a['block_size']
    sx = _seed_for(rounding_modes.STOC)
    sw = _seed_for(rounding_modes.STOC)
    xc, xe = native.stoc_codes(x2.contiguous(), block, m, eps, sx, native.ActSparsity.from_bfp_args(a))
    wc, we = native.stoc_codes(w.contiguous(), block, m, eps, sw, _weight_sparsity(a))
    flag = native.exp_top_flag(xe, we)
    if route == 'mx8':
        stoc.stoc_mx_calls += 1
        out = native.hbfp_linear_mx8(x2, *native.mx8_from_hbfp(wc, we, K, m, 8), m, eps, bias=bias, out_dtype=torch.float32,
                                     x_image=native.mx8_from_hbfp(xc, xe, K, m, 8))
    else:
        stoc.stoc_i8_calls += 1
        out = native.hbfp_linear_i8(x2, wc, we, m, m, eps, bias=bias, out_dtype=torch.float32, xq=(xc, xe), block_size=block)
    if int(flag.item()):
        stoc.fallbacks += 1
        with _replay_seeds((sx, sw)):
            xq, wq = MxM_pre_processing(x, w, False, **a)
        return F.linear(xq, wq, bias)
    return out.view(tuple(x.shape[:-1]) + (N,))


def _gen_bfp_op(op, name, bfp_args, transpose=False, cache=None, stoc=None):
    """reference: bfp_ops.py:160-192 -- wraps `op(x, w, ...)` so that both operands are BFP-quantized
    (and sparsified) on the way in and the output gradient on the way back.  cache: optional WeightCache; stoc: optional
    StocMatrixUnit."""
    def bfp_op(x, w, *args, **kwargs):
        if not torch.is_grad_enabled():                 # inference: same values, no autograd nodes to build
            if stoc is not None and stoc.matrix_unit and op is F.linear and transpose is False:
                out = _stoc_linear(x, w, args[0] if args else kwargs.get('bias'), bfp_args, stoc)
                if out is not None:
                    return out
            route = _cached_route(x, w, bfp_args, cache) if cache is not None and cache.matrix_unit and op is F.linear else 'fake'
            if route in ('int8', 'mx8'):
                bias = args[0] if args else kwargs.get('bias')
                m, eps, act = bfp_args['mant_bits'], bfp_args['epsilon'], native.ActSparsity.from_bfp_args(bfp_args)
                if route == 'int8':
                    cache.i8_calls += 1
                    return native.hbfp_linear_i8(x, *cache.weight_codes_i8(w, bfp_args), m, m, eps, bias=bias, act=act,
                                                 block_size=bfp_args['block_size'])
                cache.mx_calls += 1
                return native.hbfp_linear_mx8(x, *cache.weight_image(w, bfp_args), m, eps, bias=bias, act=act)
            xq, wq = _quantize_operands(x, w, transpose, bfp_args, cache)
            return op(xq, wq, *args, **kwargs)
        xq, wq = _OperandQuantizer.apply(x, w, transpose, bfp_args, cache)
        return _GradQuantizer.apply(op(xq, wq, *args, **kwargs), bfp_args)

    bfp_op.__name__ = _get_op_name(name, **bfp_args)
    bfp_op.weight_cache = cache
    bfp_op.stoc_matrix_unit = stoc
    return bfp_op


def _get_bfp_op(op, name, bfp_args, transpose=False, cache=None, stoc=None):
    """reference: bfp_ops.py:194-200 (its cache dict is a local, so there too every layer gets its own op)"""
    return _gen_bfp_op(op, name, bfp_args, transpose, cache, stoc)


_BFP_ARG_DEFAULTS = dict(num_format='fp32', sparsity_num_format='fp32', rounding_mode='stoc', epsilon=1e-8,
                         mant_bits=0, block_size=0, weight_mant_bits=0, in_sparsity=False, w_sparsity=False,
                         grad_sparsity=False, N=0, M=0, first='s', sparsity_mode='unstructured', sparsity_frac=0,
                         mx_w_elem_format='', mx_a_elem_format='', bfloat=16, scale_bits=8, device='cpu')


def unpack_bfp_args(kwargs):
    """reference: bfp_ops.py:202-231 -- moves the 20 known keys out of `kwargs` (which is mutated) into a
    new dict, filling defaults; unknown keys stay behind in `kwargs`."""
    return {key: kwargs.pop(key, default) for key, default in _BFP_ARG_DEFAULTS.items()}


def F_linear_bfp(**kwargs):
    """reference: bfp_ops.py:233-238"""
    bfp_args = unpack_bfp_args(kwargs)
    return _get_bfp_op(F.linear, 'linear', bfp_args) if bfp_args['num_format'] == 'bfp' else F.linear


class MatmulStats:
    """what an F_matmul_bfp(matrix_unit='int8') op ran: i8_calls on the int8 matrix unit, fake_calls as the plain composition,
    cache_calls the scores / context products of the KV caches made by its kv_cache()"""

    def __init__(self):
        self.i8_calls = 0
        self.fake_calls = 0
        self.cache_calls = 0


# The batched int8 route by default: from this many rows of the first operand (T = x.shape[-2]) on, None: never.  Keyed by (operand
# dtype, block 64 or not, family): 'qk' is a contraction no longer than the output is wide (K <= N: Q K^T, bound by the output write),
# 'pv' the other one (K > N: P V, bound by reading P).  Measured against the fake route timed on the parent commit, hipGraph replay,
# GPT-2 small at batch 1 and 8 (T 1024 and 128) and a 32-head D = 128, T = 2048 shape (profiles/r11_bmm.json): fp32 block 64 wins
# everywhere (1.32-2.01x); bf16 block 64 wins P V (1.17-1.34x) and loses Q K^T from T = 1024 on (0.53-0.91x; 0.96-1.03x at T = 128);
# block 16 with a 1:4-pruned second operand wins only fp32 Q K^T (1.09-1.45x), is even or slower on fp32 P V (0.78-1.01x) and slower on
# bf16 (0.31-0.83x).  Block 32 and dense block 16 were not measured and take the block-16 entries; fp16 takes the bf16 ones.
MATMUL_I8_MIN = {
    (torch.float32, True, 'qk'): 1, (torch.float32, True, 'pv'): 1, (torch.float32, False, 'qk'): 1, (torch.float32, False, 'pv'): None,
    (torch.bfloat16, True, 'qk'): None, (torch.bfloat16, True, 'pv'): 1, (torch.bfloat16, False, 'qk'): None, (torch.bfloat16, False, 'pv'): None,
}


def matmul_i8_min(dtype, block_size, N, K):
    """the MATMUL_I8_MIN entry of a problem (a dtype not listed: the bf16 entry)"""
    key = (block_size == 64, 'qk' if K <= N else 'pv')
    return MATMUL_I8_MIN.get((dtype,) + key, MATMUL_I8_MIN.get((torch.bfloat16,) + key))


def matmul_route(x, w, a, matrix_unit):
    """the contraction of F_matmul_bfp(matrix_unit=...)(x, w) under the bfp_args a: 'int8' (native.hbfp_bmm_i8 on codes of both operands)
    or 'fake' (MxM_pre_processing + torch.matmul).  'int8' needs all of: matrix_unit 'int8'; no gradient recording; 'bfp' in both formats,
    round-half-even, block 16, 32 or 64, 1..7 mantissa bits; both operands of one dtype (fp32, bf16, fp16) on one ROCm device; not
    compiling; equal leading batch dimensions (broadcasting: 'fake'); x contiguous along its last dimension; K % block == 0,
    N % 16 == 0 and the C predicate; pruning as _pruning_ok takes it with quantize-first weights; T >= the problem's MATMUL_I8_MIN entry (matmul_i8_min).  Host
    logic only."""
    if matrix_unit != 'int8' or torch.is_grad_enabled():
        return 'fake'
    if (a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp' or a['rounding_mode'] != rounding_modes.DETERM
            or a['block_size'] not in (64,) + native.I8_BLOCKS or not (1 <= a['mant_bits'] <= 7)):
        return 'fake'
    if (not isinstance(x, torch.Tensor) or not isinstance(w, torch.Tensor) or x.dim() < 2 or w.dim() < 2 or x.dtype != w.dtype
            or x.dtype not in native.DTYPE_CODE or x.device.type != 'cuda' or x.device != w.device or torch.compiler.is_compiling()):
        return 'fake'
    if tuple(x.shape[:-2]) != tuple(w.shape[:-2]) or x.shape[-1] != w.shape[-2] or x.stride(-1) != 1:
        return 'fake'
    T, K, N = x.shape[-2], x.shape[-1], w.shape[-1]
    B = x.numel() // (T * K) if T * K else 0
    if B < 1 or K % a['block_size'] or N % 16 or not _pruning_ok(a, w_quantize_first=True):
        return 'fake'
    lim = matmul_i8_min(x.dtype, a['block_size'], N, K)
    if lim is None or T < lim or not native.hbfp_bmm_i8_ok(B, T, N, K, a['mant_bits'], a['mant_bits'], a['block_size']):
        return 'fake'
    return 'int8'


def _matmul_i8(x, w, a):
    """torch.matmul(Q_in(x), Q_w(w^T)^T) on the int8 matrix unit for a call matmul_route sends there.  x's codes: act_codes on its
    [B T, K] rows.  w's codes, blocks along K = its second-to-last dimension: where w^T is contiguous (key.transpose(-1, -2)) act_codes on
    the [B N, K] rows of that view, no copy; a dense w goes through the transposed quantizer (native.codes_transposed), one read; a pruned
    w through the transposed copy and act_codes, where the N:M tie order and the whole-tensor threshold live."""
    m, eps, block = a['mant_bits'], a['epsilon'], a['block_size']
    T, K, N = x.shape[-2], x.shape[-1], w.shape[-1]
    B = x.numel() // (T * K)
    xq = native.act_codes(x.reshape(B * T, K), m, eps, native.ActSparsity.from_bfp_args(a), block_size=block)
    wt, w_act = w.transpose(-1, -2), _weight_sparsity(a)
    if wt.is_contiguous():
        wq = native.act_codes(wt.reshape(B * N, K), m, eps, w_act, block_size=block)
    elif w_act is None:
        wq = native.codes_transposed(w.reshape(B, K, N), block, m, eps)
    else:
        wq = native.act_codes(wt.contiguous().view(B * N, K), m, eps, w_act, block_size=block)
    out = native.hbfp_bmm_i8(xq, wq, B, T, N, K, m, m, block_size=block, out_dtype=x.dtype)
    return out.view(tuple(x.shape[:-1]) + (N,))


def _gen_matmul_i8_op(bfp_args, matrix_unit):
    """the F_matmul_bfp op with the matrix-unit switch on: per call matmul_route picks the batched int8 GEMM or the plain composition
    (every gradient-recording call, and whatever the route refuses).  The op's matmul_stats (MatmulStats) counts both."""
    fake = _get_bfp_op(torch.matmul, 'matmul', bfp_args, True)
    stats = MatmulStats()

    def bfp_op(x, w, *args, **kwargs):
        if not args and not kwargs and matmul_route(x, w, bfp_args, matrix_unit) == 'int8':
            stats.i8_calls += 1
            return _matmul_i8(x, w, bfp_args)
        stats.fake_calls += 1
        return fake(x, w, *args, **kwargs)

    def kv_cache(batch, heads, head_dim, capacity, dtype=torch.bfloat16, device='cuda', **mode):
        """an HBFPKVCache under this op's bfp_args; its products count in matmul_stats.cache_calls.  mode: device_lengths=True (and
        chunks_per_split), kv_heads, prompt_rows, window, starts, page_tokens, pages and code_bits as HBFPKVCache takes them"""
        return HBFPKVCache(batch, heads, head_dim, capacity, dtype=dtype, stats=stats, **mode, **dict(bfp_args, device=device))

    bfp_op.__name__ = fake.__name__
    bfp_op.matmul_stats = stats
    bfp_op.kv_cache = kv_cache
    return bfp_op


def kv_cache_config_check(a, head_dim):
    """raise ValueError unless HBFPKVCache holds keys and values of head_dim under the configuration `a` (unpacked bfp_args): 'bfp' in both
    formats, round-half-even, block 16, 32 or 64, mant_bits 1..7, head_dim a multiple of the block and of 16, K and V dense.  Pruned K / V
    (w_sparsity) is refused: N:M along the open token block and the whole-tensor threshold both change as tokens arrive.  in_sparsity (the
    pruning of q and p) is taken as the batched int8 route takes it.  Host logic only."""
    if a['num_format'] != 'bfp' or a['sparsity_num_format'] != 'bfp':
        raise ValueError("HBFPKVCache holds HBFP codes: num_format and sparsity_num_format must be 'bfp' (got %r, %r)"
                         % (a['num_format'], a['sparsity_num_format']))
    if a['rounding_mode'] != rounding_modes.DETERM:
        raise ValueError("HBFPKVCache: stochastic rounding is refused (appended codes must not depend on a draw): rounding_mode must be "
                         "'determ' (got %r)" % (a['rounding_mode'],))
    if a['block_size'] not in (64,) + native.I8_BLOCKS or isinstance(a['block_size'], bool):
        raise ValueError("HBFPKVCache: block_size must be 16, 32 or 64 (got %r)" % (a['block_size'],))
    if isinstance(a['mant_bits'], bool) or not 1 <= a['mant_bits'] <= 7:
        raise ValueError("HBFPKVCache: mant_bits must be 1..7, codes are int8 (got %r)" % (a['mant_bits'],))
    if head_dim < 16 or head_dim % a['block_size'] or head_dim % 16:
        raise ValueError("HBFPKVCache: head_dim must be a multiple of block_size and of 16 (got head_dim=%r, block_size=%r)"
                         % (head_dim, a['block_size']))
    if a['w_sparsity'] == True:  # noqa: E712
        raise ValueError("HBFPKVCache: pruned K / V (w_sparsity) is refused: pruning does not compose with appending tokens")
    if not _pruning_ok(a, w_quantize_first=True):
        raise ValueError("HBFPKVCache: in_sparsity configuration not taken (sparsity_mode=%r, N:M=%r:%r, sparsity_frac=%r)"
                         % (a['sparsity_mode'], a['N'], a['M'], a['sparsity_frac']))


class HBFPKVCache:
    """Attention keys and values of B x H heads held as HBFP codes across decode steps (csrc/bfpq_kvcache.hip): what the
    reference's GPT-2 keeps as layer_past (modeling_gpt2.py:345-348) and quantizes again in full at every step.

        cache.append(k_new, v_new)   # each [B, H, t, D], any t >= 1; returns the new length
        cache.scores(q)              # [B, H, Tq, S] == F_matmul_bfp(**bfp_args)(q, K_all.transpose(-1, -2))
        cache.context(p)             # [B, H, Tq, D] == F_matmul_bfp(**bfp_args)(p, V_all), p [B, H, Tq, S]

    with K_all / V_all everything appended so far and S = cache.length, on the int8 matrix unit (exact block sums, fp32 across blocks in
    block order: the arithmetic of F_matmul_bfp(matrix_unit='int8')).  At every length the codes stand for
    float_to_bfp_blocked(K_all, identifier='w') and float_to_bfp_blocked(V_all.transpose(-1, -2), identifier='w') bit for bit, up to the
    sign of zero: V's blocks run along the tokens, so its open block is quantized again from the original values (v_tail) at every
    append, never from codes.  Up to 16 dense rows of q / p are quantized inside the product kernel; more rows, or in_sparsity, go through
    native.act_codes and the batched GEMM (there p is zero-padded to whole blocks first; with unstructured in_sparsity that needs
    S % block_size == 0, the whole-tensor threshold would count the pad).

    Inference only: every call raises ValueError while gradients are recorded.  The length lives on the host (a Python int), so a decode
    step cannot be captured in a hipGraph: a replay would append at the captured position.  keys() / values() dequantize, for inspection
    and tests.

    device_lengths=True lifts that: the lengths live on the device, one per sequence, so the batch may be ragged and one
    decode step -- append, scores, the caller's scale and softmax, context -- captured with torch.cuda.graph on one stream advances
    correctly on every replay.  Then

        cache.lengths                       # int32 [B] on the device, the only record of the lengths (cache.length raises)
        cache.overflow                      # int32 [1]: set to 1, and left so until reset(), by an append that was refused
        cache.append(k_new, v_new, counts)  # sequence b takes its first counts[b] (int32 [B] on the device, 0..t; None: all t) rows
                                            # at lengths[b] ..; one that would pass `capacity`, or whose count is outside 0..t, is
                                            # left untouched and raises `overflow`.  Returns None
        cache.scores(q, max_len)            # [B, H, Tq, max_len], max_len a host int in 1..capacity (default: capacity): column
                                            # n < lengths[b] is the product, every other column -inf.  A sequence longer than max_len
                                            # is the caller's error: its columns past max_len are absent, nothing reports it
        cache.context(p)                    # p [B, H, Tq, L], any 1 <= L <= capacity: sequence b contracts over its first
                                            # min(lengths[b], L) tokens; p at or past lengths[b] counts as zero, NaN and Inf included

    None of the three reads anything back, synchronises or allocates by a length: context()'s workspace is made once at construction
    for max_query_rows rows of p (default 16: 4 B per row, cached token and column of V, i.e. a quarter of v_codes per row at block 64,
    a sixteenth with max_query_rows=1, which is all a decode step needs; more rows than that raise ValueError).  Up to 16 dense rows of q / p only; more rows raise
    ValueError, and so does in_sparsity at construction.  context() splits the tokens over workgroups (chunks_per_split 64-token chunks
    per slice, 0: the library's choice) and adds the blocks in block order in a second launch: the same bits as the host-length cache
    for any slice size.  keys(b) / values(b) read lengths[b] back, for inspection.

    The whole step after the append is one call there:

        ctx = cache.attend(q, scale, max_len=None, causal=False)                     # [B, H, Tq, D]
        ctx, p = cache.attend(q, scale, max_len=None, causal=False, return_probs=True)   # p [B, H, Tq, max_len]

    equal to context(p) of p = softmax(scores(q, max_len).float() * scale, -1).to(dtype), in three launches and with no [.., S] array of
    the dtype in between: the scores reach the softmax as scores() rounds them, times float(scale) in fp32; the softmax runs in fp32
    (maximum, expf, a sum whose order depends on the row alone, a division) and is rounded once; from p on the bits are context(p)'s for
    every chunks_per_split.  causal=True takes the Tq rows to be the last Tq tokens held: row t sees the keys n <= lengths[b] - Tq + t.
    Keys a row does not see are exactly +0 in p; an empty sequence gives a zero context row, and a row that sees no key of a sequence
    that holds some (causal with Tq > lengths[b]) what context() makes of a p of zeros.  The fp32 score rows [B H, max_query_rows, cap] are a workspace made by the first attend() or by prepare_attend() --
    call either before capturing a graph -- and never grown; caches that never attend never hold it.

    kv_heads (grouped-query attention; the reference's LLaMA, modeling_llama.py:385-409): an int in 1..heads that divides
    heads; None or heads is the cache above.  The buffers, append(), keys() and values() then hold kv_heads heads per sequence -- nbytes()
    is 1 / g of the above, g = heads // kv_heads -- while scores(), context() and attend() take and return [B, heads, Tq, .] as before:
    query head h reads kv head h // g, the reference's repeat_kv order (:264-273), and nothing is repeated.  Every result is bit for
    bit that of an HBFPKVCache(batch, heads, ...) fed k.repeat_interleave(g, 1), v.repeat_interleave(g, 1).  The row limits (16,
    max_query_rows) stay limits per query head, and the workspaces hold the same bytes.  The g Tq rows of a kv head go through the
    kernels in tiles of 16: the rows of a tile share every load of the codes, which are read again per tile; on the host-length cache
    more than 16 rows take the act_codes route.

    prompt_rows=P (prompt attention; needs device_lengths=True): attend() then takes any Tq >= 1, so the prompt -- in one
    piece or in chunks, append(chunk); attend(q_chunk, scale, causal=True) -- runs on the codes append() has just made, with no second
    quantization of K and V and no [B, H, Tq, S] array of the dtype.  Tq <= 16 goes exactly where it goes without P.  More rows are
    walked in panels of P query tokens per query head, two launches per panel (q k^T of the panel into fp32 score rows; softmax and
    p v with the accumulators in registers: no block sums, no combine pass), with no read-back and no allocation but the results;
    cache_calls counts 2 per call.  causal, max_len, return_probs and kv_heads mean what they mean above, row t of Tq seeing the keys
    n <= lengths[b] - Tq + t.  Nothing a row computes depends on Tq, on P or on the rows beside it: every row is, bit for bit, the
    row attend() gives for it among up to 16, and context(p[:, :, i:i + 16]) gives ctx[:, :, i:i + 16].  P is an int, a multiple of
    16 in 16 .. prompt_rows_max(batch, heads, capacity) -- the most for which the panel workspace, the fp32 score rows
    [B heads, P, cap] made by prepare_attend() or the first long attend(), stays below 2^31 bytes -- and head_dim is at most 256.
    Small panels bound the workspace, large ones fill the device: a panel launches B heads P / 64 workgroups.  0, the default, is the
    cache above in every respect: nothing more is allocated and no new kernel is launched.  scores() and context() keep their 16-row
    limit, and the host-length cache stays as it is: both are outside this route.

    window=W and starts=True (a first visible key per row; both need device_lengths=True): what a row of attend() sees is a
    range of keys, not a prefix.  With len = lengths[b], v(t) = len - Tq + t + 1 (causal) or len, and hi(t) = clamp(v(t), 0,
    min(len, max_len)) as above, row t sees the keys lo(t) <= n < hi(t),

        lo(t) = max(0, starts[b] if starts, v(t) - W if window)

    starts=True gives the cache `cache.starts`, int32 [B] on the device, zero at construction and after reset(): the number of pad
    tokens at the front of sequence b of a left-padded batch (the reference's batched generate(); modeling_gpt2.py:228-230 and
    modeling_llama.py:402-404 hide them with the additive attention_mask).  The caller appends the pad tokens like any others and writes
    their count, cache.starts.copy_(pad_counts); the kernels read it at launch and never on the host, so a captured step follows a
    change between replays.  A negative start counts as 0.  window=W, an int >= 1, is sliding-window attention (sliding_window in
    modeling_attn_mask_utils.py: Mistral, Mixtral, Qwen2, Starcoder2): causal row i sees the W keys i - W + 1 .. i; without causal
    every row sees the last W keys of its sequence.  Nothing is evicted: a windowed cache still holds `capacity` tokens.  Keys below
    lo are exactly +0 in p; a row with lo >= hi sees nothing and is the row above that sees no key (p all +0, the context what
    context() makes of a p of zeros).  Every row is, bit for bit, the row the cache without them computes from scores that are -inf
    below lo, so ctx == context(p) still holds and nothing depends on Tq, prompt_rows, chunks_per_split or the rows beside it; key
    tiles, slices and token blocks below every row's lo are skipped.  Both compose with kv_heads, prompt_rows, max_len, causal,
    return_probs, chunks_per_split and max_query_rows, on both routes of attend().  Only attend() honours them: scores() and
    context() are products, not attention, and stay exactly as they are.  With neither (None, False: the defaults) the cache is the
    one above in every respect: the same entries, kernels, workspaces and bytes.

    page_tokens=P, pages=N (a paged cache; needs device_lengths=True): the sequences draw pages of P tokens (a multiple of
    64) from one pool of N pages instead of reserving `capacity` tokens each.  `capacity` (a multiple of P) is then the most tokens one
    sequence may hold, and the buffers hold pages, a page being P tokens of all kv heads of one sequence: k_codes [N, kv_heads, P, ldd],
    k_exps [N, kv_heads, P, D / block], v_codes [N, kv_heads, D, P], v_exps [N, kv_heads, D, P / block]; v_tail, the one open token
    block per head, stays per sequence.

        cache.page_table        # int32 [B, capacity / P] on the device, -1: no page; the kernels read it at launch, so a captured step
                                # follows what is written between replays
        cache.reserve(tokens)   # an int or B ints: every sequence gets the pages for that many tokens (never fewer than it has).  Host
                                # lists only -- no read-back -- and one small copy of the changed table rows; RuntimeError, with nothing
                                # changed, where the pool has too few free pages
        cache.assign(b, pages)  # reserve() with the caller's choice: these free pages, in this order, become sequence b's next ones
        cache.release(b)        # sequence b's pages go back to the pool, its table row to -1 and its length to 0; reset() releases all
        cache.pages_free        # free pages; nbytes() counts the pool, v_tail, the table and the lengths

    append() never allocates: a sequence whose chunk would reach a token without a page is refused as one that would pass `capacity`
    is -- left untouched, `overflow` raised -- so a captured append stays a captured append.  append(), scores(), context(), attend()
    on both routes, keys() and values() keep their signatures, and every result is, bit for bit, that of the cache without pages given
    the same calls: paging changes where the bytes lie, not what they are.  Composes with kv_heads, prompt_rows, max_len, causal and
    return_probs; with starts or window the constructor raises NotImplementedError (paging under a first visible key is not built).

    Sequences of a paged cache may share pages (csrc/bfpq_kvpages.hip): a page below a sequence's last one holds finished
    key rows and closed token blocks only and is never written again, so any number of table rows may name it.  Every page has a
    reference count, and is free exactly when it is 0:

        cache.reorder(index, tokens=None)   # new sequence b becomes old sequence index[b]: the reference's _reorder_cache, a beam
                                            # search's index_select(0, beam_idx), as a table edit, a copy of at most one page (the
                                            # open one) per duplicate and a move of v_tail and the lengths; then reserve(), append()
        cache.fork(src, dst, tokens=None)   # dst (an int or ints) become copies of src: a prompt appended and attended once
        cache.pages_shared                  # pages that more than one sequence names
        cache.page_refs                     # the counts, a host list (a copy)

    release(b) and reset() return a shared page to the pool when its last owner lets go.  No kernel of the cache changes: they read
    the table at launch.  What is not protected is said at reorder().

    code_bits=4 (4-bit codes; needs mant_bits <= 3, device_lengths=True and block_size 64): a code of mant_bits <= 3 lies in
    -7..7, so the two code buffers hold two to a byte -- k_codes [.., cap, ldd / 2], two codes of a key row along D; v_codes
    [.., D, cap / 2], two codes of a column along the tokens; element 2 k in the low nibble of byte k, 2 k + 1 in the high one, two's
    complement: PackedBFP's layout, what native.dequantize(.., code_bits=4) reads -- and half the bytes, paged or not: per token and
    kv head at D 64, 32 + 1 + 32 + 1 = 66 bytes where the int8 cache takes 130 and bf16 K and V 256.  The exponent buffers, v_tail,
    lengths, overflow, starts, the page table and the workspaces are unchanged.  The codes are the same integers in a narrower store:
    the kernels load half the bytes and widen them to the same int8 matrix-unit operand in registers, and every result -- scores(),
    context(), attend() on both routes, keys(), values(), lengths, overflow -- is bit for bit that of the cache without it on the same
    calls.  Composes with kv_heads, prompt_rows, max_len, causal, return_probs, chunks_per_split, with starts / window (contiguous) and
    with page_tokens / pages, fork() and reorder() included.  cache.code_bits reports it.  None or 8 (the default) is the cache above in
    every respect: the same entries, kernels, buffers and bytes.  Blocks 32 and 16 (a lane's share of a block there is 8 or 4 codes,
    so 4- and 2-byte loads) and the host-length cache are not built: ValueError."""

    window = None                  # no window, and ...
    starts = None                  # ... no starts, unless the constructor is given them
    pages = None                   # no pages either: native.KVPages(page_table, P, N, capacity) of a paged cache
    code_bits = 8                  # int8 codes, unless the constructor is given code_bits=4

    @staticmethod
    def prompt_rows_max(batch, heads, capacity):
        """the largest prompt_rows: a multiple of 16 whose fp32 score rows [batch heads, P, cap] stay below 2^31 bytes (0: none does)"""
        return ((1 << 31) - 16) // (4 * batch * heads * native.code_pitch(capacity)) // 16 * 16

    def __init__(self, batch, heads, head_dim, capacity, dtype=torch.bfloat16, device='cuda', stats=None, device_lengths=False,
                 chunks_per_split=0, max_query_rows=native.KV_DEC_MAX_TOKENS, kv_heads=None, prompt_rows=0, window=None, starts=False,
                 page_tokens=None, pages=None, code_bits=None, **bfp_args):
        a = unpack_bfp_args(bfp_args)
        if bfp_args:
            raise TypeError(f"HBFPKVCache: unknown arguments {sorted(bfp_args)}")
        kv_cache_config_check(a, head_dim)
        if code_bits is not None and (isinstance(code_bits, bool) or not isinstance(code_bits, int)):
            raise TypeError(f"HBFPKVCache: code_bits must be None, 8 or 4 (got {code_bits!r})")
        if code_bits not in (None, 8, 4):
            raise ValueError(f"HBFPKVCache: code_bits must be None, 8 or 4 (got {code_bits})")
        if code_bits == 4:
            if a['mant_bits'] > native.KV_C4_MAX_MANT:
                raise ValueError(f"HBFPKVCache: code_bits=4 holds codes in -7..7: mant_bits must be <= {native.KV_C4_MAX_MANT} "
                                 f"(got {a['mant_bits']})")
            if a['block_size'] != 64:
                raise ValueError(f"HBFPKVCache: code_bits=4 with block_size {a['block_size']} is not built (blocks 32 and 16 need 4- and "
                                 "2-byte loads of a lane's share of a block: a later change); block_size must be 64")
            if not device_lengths:
                raise ValueError("HBFPKVCache: code_bits=4 needs device_lengths=True (the host-length cache stays as it is)")
            self.code_bits = 4
        if dtype not in native.DTYPE_CODE:
            raise TypeError(f"HBFPKVCache: unsupported dtype {dtype}")
        if batch < 1 or heads < 1 or capacity < 1:
            raise ValueError(f"HBFPKVCache: batch, heads and capacity must be >= 1 (got {batch}, {heads}, {capacity})")
        if kv_heads is None:
            kv_heads = heads
        if isinstance(kv_heads, bool) or not isinstance(kv_heads, int):
            raise TypeError(f"HBFPKVCache: kv_heads must be an int or None (got {kv_heads!r})")
        if not 1 <= kv_heads <= heads or heads % kv_heads:
            raise ValueError(f"HBFPKVCache: kv_heads must be in 1..heads and divide heads (got kv_heads={kv_heads}, heads={heads})")
        self.args, self.act = a, native.ActSparsity.from_bfp_args(a)
        self.device_lengths, self.chunks_per_split = bool(device_lengths), int(chunks_per_split)
        if self.device_lengths and self.act is not None:
            raise ValueError("HBFPKVCache(device_lengths=True): in_sparsity is not taken (q and p are quantized inside the product kernels)")
        if not 0 <= self.chunks_per_split <= 16:
            raise ValueError(f"HBFPKVCache: chunks_per_split must be 0..16 (got {chunks_per_split})")
        if isinstance(max_query_rows, bool) or not isinstance(max_query_rows, int) or not 1 <= max_query_rows <= native.KV_DEC_MAX_TOKENS:
            raise ValueError(f"HBFPKVCache: max_query_rows must be 1..{native.KV_DEC_MAX_TOKENS} (got {max_query_rows!r})")
        self.max_query_rows = max_query_rows
        if isinstance(prompt_rows, bool) or not isinstance(prompt_rows, int):
            raise TypeError(f"HBFPKVCache: prompt_rows must be an int (got {prompt_rows!r})")
        if prompt_rows:
            if prompt_rows < 16 or prompt_rows % 16:
                raise ValueError(f"HBFPKVCache: prompt_rows must be 0 or a multiple of 16, at least 16 (got {prompt_rows})")
            if not self.device_lengths:
                raise ValueError("HBFPKVCache: prompt_rows needs device_lengths=True")
            if head_dim > native.KV_ROWS_MAX_HEAD_DIM:
                raise ValueError(f"HBFPKVCache: prompt_rows takes head_dim up to {native.KV_ROWS_MAX_HEAD_DIM} (got {head_dim})")
            if batch >= 1 and heads >= 1 and capacity >= 1 and prompt_rows > self.prompt_rows_max(batch, heads, capacity):
                raise ValueError(f"HBFPKVCache: prompt_rows={prompt_rows} makes a panel workspace of 2^31 bytes or more; the most here is "
                                 f"{self.prompt_rows_max(batch, heads, capacity)}")
        self.prompt_rows = prompt_rows
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, int):
                raise TypeError(f"HBFPKVCache: window must be None or an int (got {window!r})")
            if window < 1:
                raise ValueError(f"HBFPKVCache: window must be >= 1 (got {window})")
            if not self.device_lengths:
                raise ValueError("HBFPKVCache: window needs device_lengths=True")
            self.window = window
        if not isinstance(starts, bool):
            raise TypeError(f"HBFPKVCache: starts must be False or True (got {starts!r}); the counts go into cache.starts")
        if starts and not self.device_lengths:
            raise ValueError("HBFPKVCache: starts needs device_lengths=True")
        if page_tokens is None and pages is not None:
            raise ValueError("HBFPKVCache: pages needs page_tokens")
        if page_tokens is not None:
            for name, v in (("page_tokens", page_tokens), ("pages", pages)):
                if isinstance(v, bool) or not isinstance(v, int):
                    raise TypeError(f"HBFPKVCache: {name} must be an int (got {v!r}); a paged cache takes page_tokens=P, pages=N")
            if page_tokens < 64 or page_tokens % 64:
                raise ValueError(f"HBFPKVCache: page_tokens must be a multiple of 64 (got {page_tokens})")
            if pages < 1:
                raise ValueError(f"HBFPKVCache: pages must be >= 1 (got {pages})")
            if not self.device_lengths:
                raise ValueError("HBFPKVCache: page_tokens needs device_lengths=True")
            if starts or window is not None:
                raise NotImplementedError("HBFPKVCache: page_tokens with starts=True or window=W is not built: paging under a first "
                                          "visible key is a later change")
            if capacity % page_tokens:
                raise ValueError(f"HBFPKVCache: capacity must be a multiple of page_tokens (got {capacity}, {page_tokens}): the page "
                                 "table is capacity / page_tokens entries wide")
        self.batch, self.heads, self.head_dim, self.capacity, self.dtype = batch, heads, head_dim, capacity, dtype
        self.kv_heads, self.group = kv_heads, heads // kv_heads  # query head h reads kv head h // group
        self.block, self.mant_bits, self.epsilon = a['block_size'], a['mant_bits'], a['epsilon']
        self.cap = native.code_pitch(capacity)                   # tokens the buffers hold: a multiple of 64 and of the block
        if not native.kv_ok(head_dim, self.cap, self.block) or (page_tokens and not native.kv_ok(head_dim, page_tokens, self.block)):
            raise ValueError(f"HBFPKVCache: head_dim {head_dim} x capacity {capacity} at block {self.block} is not taken")
        self.stats = stats if stats is not None else MatmulStats()
        self._length = 0
        B, H, D, cap, blk = batch, kv_heads, head_dim, self.cap, self.block
        z = lambda *shape, dt=torch.int8: torch.zeros(shape, dtype=dt, device=device)
        HB, hc = (pages, page_tokens) if page_tokens else (B, cap)   # the buffers' leading dimension: the pool's pages, or the sequences
        cpb = 8 // self.code_bits                                 # codes per byte of the two code buffers
        self.buffers = dict(k_codes=z(HB, H, hc, native.code_pitch(D) // cpb), k_exps=z(HB, H, hc, D // blk), v_codes=z(HB, H, D, hc // cpb),
                            v_exps=z(HB, H, D, hc // blk), v_tail=z(B, H, blk, D, dt=dtype))
        for name, t in self.buffers.items():
            setattr(self, name, t)
        if self.device_lengths:
            self.lengths, self.overflow = z(B, dt=torch.int32), z(1, dt=torch.int32)
            self._ws = self._workspace(max_query_rows)            # context()'s only workspace: made here, never grown
            self._att_ws = None                                   # attend()'s fp32 score rows: made by its first call
            self._rows_ws = None                                  # the panel's fp32 score rows (prompt_rows): likewise
            if starts:
                self.starts = z(B, dt=torch.int32)                # the first visible key of every sequence: written by the caller
            if page_tokens:
                self.page_tokens, self.page_count = page_tokens, pages
                width = capacity // page_tokens
                # the table and, behind it, the job list of a reorder(): one small copy brings both
                self._table_dev = torch.full((B * (width + native.KV_JOB_WORDS),), -1, dtype=torch.int32, device=device)
                self.page_table = self._table_dev[:B * width].view(B, width)
                self.pages = native.KVPages(self.page_table, page_tokens, pages, capacity)
                self._table_host = torch.full((B, capacity // page_tokens), -1, dtype=torch.int32)   # the table as reserve() last wrote it
                self._owned = [[] for _ in range(B)]              # every sequence's pages, in token order
                self._free = collections.deque(range(pages))      # taken from the left, returned to the right
                self._refs = [0] * pages                          # table rows that name each page: free exactly when 0
                self._move_ws = None                              # reorder()'s staging buffer: made by its first call, kept
                self._uploads, self._upload_at = None, 0          # reorder()'s pinned host buffers, used in turn, each with an event

    # ---- the pages of a paged cache: host lists, nothing read back ---------------------------------------------------------------
    def _paged(self, what):
        if self.pages is None:
            raise ValueError(f"HBFPKVCache.{what} needs a paged cache (page_tokens=P, pages=N)")

    def _seq(self, what, b):
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.batch:
            raise ValueError(f"HBFPKVCache.{what}: a sequence index in 0..{self.batch - 1} (got {b!r})")

    def _give(self, grants):
        """grants {b: pages}: they leave the free list and become the next pages of sequence b; the changed table rows go to the device in
        one copy.  The caller has checked that every page is free and every row has room"""
        grants = {b: list(pg) for b, pg in grants.items() if len(pg)}
        if not grants:
            return
        taken = {p for pg in grants.values() for p in pg}
        self._free = collections.deque(p for p in self._free if p not in taken)
        for b, pg in grants.items():
            n = len(self._owned[b])
            self._table_host[b, n:n + len(pg)] = torch.tensor(pg, dtype=torch.int32)
            self._owned[b].extend(pg)
            for p in pg:
                self._refs[p] = 1
        lo, hi = min(grants), max(grants) + 1
        self.page_table[lo:hi].copy_(self._table_host[lo:hi])

    @property
    def pages_free(self):
        self._paged('pages_free')
        return len(self._free)

    def reserve(self, tokens):
        """every sequence gets pages for `tokens` tokens (an int, or one int per sequence); one that has as many keeps what it has.
        RuntimeError, with the table and the free list as they were, where the pool has too few free pages"""
        self._paged('reserve')
        want = list(tokens) if isinstance(tokens, (list, tuple)) else [tokens] * self.batch
        if len(want) != self.batch or any(isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= self.capacity for n in want):
            raise ValueError(f"HBFPKVCache.reserve takes an int or {self.batch} ints in 0..{self.capacity} (got {tokens!r})")
        P = self.page_tokens
        more = [max(0, (n + P - 1) // P - len(self._owned[b])) for b, n in enumerate(want)]
        if sum(more) > len(self._free):
            raise RuntimeError(f"HBFPKVCache.reserve: the pool is exhausted: {sum(more)} pages wanted, {len(self._free)} of "
                               f"{self.page_count} free")
        free = list(self._free)
        grants, at = {}, 0
        for b, n in enumerate(more):
            grants[b], at = free[at:at + n], at + n
        self._give(grants)

    def assign(self, b, pages):
        """reserve() with the caller's choice of pages: `pages`, distinct free pages of the pool, become sequence b's next ones in this
        order.  ValueError, with nothing changed, for a page that is not free or a row that has no room"""
        self._paged('assign')
        self._seq('assign', b)
        pages = list(pages)
        free = set(self._free)
        if any(isinstance(p, bool) or not isinstance(p, int) for p in pages) or len(set(pages)) != len(pages) or not set(pages) <= free:
            raise ValueError(f"HBFPKVCache.assign takes distinct free pages of the pool (got {pages!r})")
        if len(self._owned[b]) + len(pages) > self._table_host.shape[1]:
            raise ValueError(f"HBFPKVCache.assign: sequence {b} holds {len(self._owned[b])} pages of at most {self._table_host.shape[1]}")
        self._give({b: pages})

    def _drop(self, pages):
        """one table row lets go of these pages: those no other row names go to the right of the free queue, in this order"""
        for p in pages:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                self._free.append(p)

    def release(self, b):
        """sequence b's pages go back to the pool -- those it shares with another sequence (fork, reorder) once the last of them lets
        go; its table row becomes -1 and its length 0"""
        self._paged('release')
        self._seq('release', b)
        self._drop(self._owned[b])
        self._owned[b] = []
        self._table_host[b] = -1
        self.page_table[b:b + 1].copy_(self._table_host[b:b + 1])
        self.lengths[b:b + 1].zero_()

    # ---- pages shared between sequences: a full page is immutable, so any number of table rows may name it ---------------
    @property
    def pages_shared(self):
        """pages that more than one sequence names"""
        self._paged('pages_shared')
        return sum(1 for n in self._refs if n > 1)

    @property
    def page_refs(self):
        """how many sequences name each page of the pool (a copy); a page is free exactly when its count is 0"""
        self._paged('page_refs')
        return list(self._refs)

    def _plan_reorder(self, index, tokens):
        """reorder() as a pure function of the host state: (the sequences' new page lists, the new counts, the new free queue, the
        jobs of native.kv_rows_move).  Raises with nothing changed; ValueError for bad arguments, RuntimeError where the pool has too
        few pages for the copies"""
        B, P = self.batch, self.page_tokens
        if len(index) != B or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < B for i in index):
            raise ValueError(f"HBFPKVCache.reorder takes {B} sequence indices in 0..{B - 1} (got {index!r})")
        if len(tokens) != B or any(isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= self.capacity for n in tokens):
            raise ValueError(f"HBFPKVCache.reorder: tokens must be {B} ints in 0..{self.capacity}, the sequences' lengths (got {tokens!r})")
        heirs = {}                                                # source -> the new rows it becomes, ascending
        for b, s in enumerate(index):
            heirs.setdefault(s, []).append(b)
        for s in heirs:
            if tokens[s] > len(self._owned[s]) * P:
                raise ValueError(f"HBFPKVCache.reorder: sequence {s} has pages for {len(self._owned[s]) * P} tokens, tokens says {tokens[s]}")
        owned, refs, copies = [None] * B, list(self._refs), {}    # copies: the rows that get a fresh page -> its slot
        for s, rows in heirs.items():
            own = self._owned[s]
            if len(rows) == 1:
                owned[rows[0]] = own                              # the only heir: the list moves with the table row
                continue
            full, open_page = tokens[s] // P, tokens[s] % P != 0
            heir = s if index[s] == s else rows[0]                # keeps s's open page and whatever s had reserved beyond it
            shared = own[:full]
            for p in shared:
                refs[p] += len(rows) - 1
            for b in rows:
                if b == heir:
                    owned[b] = own
                elif open_page:
                    owned[b], copies[b] = shared + [-1], full
                else:
                    owned[b] = list(shared)
        free = list(self._free)
        for s in range(B):                                        # what no new row names is released, in row order, and may serve below
            if s not in heirs:
                for p in self._owned[s]:
                    refs[p] -= 1
                    if refs[p] == 0:
                        free.append(p)
        if len(copies) > len(free):
            raise RuntimeError(f"HBFPKVCache.reorder: the pool is exhausted: {len(copies)} pages wanted for the open pages of duplicated "
                               f"sequences, {len(free)} of {self.page_count} free or released by this call")
        jobs, taken = [], 0
        for b, s in enumerate(index):
            if b == s:
                continue                                          # its own heir: nothing moves
            src_page = dst_page = -1
            if b in copies:
                at = copies[b]
                src_page, dst_page, taken = self._owned[s][at], free[taken], taken + 1
                owned[b][at], refs[dst_page] = dst_page, 1
            jobs.append((s, b, src_page, dst_page, tokens[s]))
        return owned, refs, collections.deque(free[taken:]), jobs

    def reorder(self, index, tokens=None):
        """new sequence b becomes old sequence index[b] (the reference's _reorder_cache, index_select(0, beam_idx)): B ints in
        0..B-1 as a list or an integer tensor -- a tensor is read back to the host, one synchronisation.  tokens: the B old lengths
        as host ints; None reads cache.lengths back in that same synchronisation.  Full pages are shared, not copied: with L =
        tokens[s] and old sequence s named by k new rows, the L // P full pages are named by all k; if L % P != 0 one heir -- row s
        itself if index[s] == s, else the lowest such row -- keeps s's open page and what s had reserved beyond it, and each of
        the other k - 1 rows gets a fresh page from the left of the free queue, into which the device copies the open page, and
        nothing beyond it: call reserve() afterwards, as before any append.  Old sequences nobody names are released, and their
        pages may serve as fresh ones in the same call.  RuntimeError, with nothing changed, where the pool is short of the
        sum over s of (k_s - 1) * (L_s % P != 0) pages.  On the device (native.kv_rows_move, two launches, one small copy of the job
        list): v_tail and the length of every row that is not its own heir follow; rows with index[b] == b cost nothing.  A
        length travels only if it equals tokens[s]: a wrong count leaves the new row empty and sets `overflow` -- release() such a
        row -- and never gives a row that attends over pages it was not given.  Plans on the host, so it is not for a captured
        graph; captured steps replayed afterwards follow the new table.

        Not protected: a caller who writes cache.lengths[b] downwards on a row that shares pages and then appends overwrites pages
        other sequences read; release(b) is the way to reuse a row.  Speculative rollback is not part of this."""
        self._paged('reorder')
        on_host = not isinstance(index, torch.Tensor)
        if not on_host and (index.dim() != 1 or index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool):
            raise ValueError(f"HBFPKVCache.reorder: index must be a list or an integer tensor [{self.batch}] (got {index.dtype}, "
                             f"{tuple(index.shape)})")
        if tokens is None:
            if not on_host and index.device == self.lengths.device and index.numel() == self.batch:
                both = torch.cat([index.to(torch.int64), self.lengths.to(torch.int64)]).tolist()      # the one synchronisation
                index, tokens = both[:self.batch], both[self.batch:]
            else:
                tokens = self.lengths.tolist()
        if isinstance(index, torch.Tensor):
            index = index.tolist()
        if not isinstance(index, (list, tuple, range)) or not isinstance(tokens, (list, tuple)):
            raise ValueError(f"HBFPKVCache.reorder takes {self.batch} indices (a list or an integer tensor) and tokens=None or "
                             f"{self.batch} ints (got {index!r}, {tokens!r})")
        index, tokens = list(index), list(tokens)
        self._commit_reorder(*self._plan_reorder(index, tokens))

    def _commit_reorder(self, owned, refs, free, jobs):
        """the plan becomes the state: the lists, the counts, the queue; the table and the jobs go to the device in one copy that does
        not wait for the stream (a pinned buffer, four used in turn, each reused only once its last copy has run), then two launches"""
        self._owned, self._refs, self._free = owned, refs, free
        B, width = self._table_host.shape
        flat = [p for own in owned for p in own + [-1] * (width - len(own))] + [w for job in jobs for w in job]
        host = torch.frombuffer(array.array('i', flat), dtype=torch.int32)
        self._table_host.copy_(host[:B * width].view(B, width))
        dev, n = self.k_codes.device, len(flat)
        if jobs and self._move_ws is None:                        # the staging buffer, kept: at most B jobs, one v_tail's worth and B ints
            ws = native.kv_rows_move_ws_bytes(B, self.kv_heads, self.head_dim, self.block, self.dtype)
            self._move_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        if dev.type != 'cuda':
            self._table_dev[:n].copy_(host)                       # (device='meta': no memory behind the buffers, the plan is all there is)
            return
        with torch.cuda.device(dev):
            if self._uploads is None:
                self._uploads = [(torch.empty(self._table_dev.numel(), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(4)]
            pinned, event = self._uploads[self._upload_at]
            self._upload_at = (self._upload_at + 1) % len(self._uploads)
            event.synchronize()
            pinned[:n].copy_(host)
            self._table_dev[:n].copy_(pinned[:n], non_blocking=True)
            event.record()
        if not jobs:
            return
        native.kv_rows_move(self.k_codes, self.k_exps, self.v_codes, self.v_exps, self.v_tail, self.lengths, self.overflow,
                            self._table_dev[B * width:n].view(len(jobs), native.KV_JOB_WORDS), self._move_ws, self.kv_heads, self.block,
                            self.pages, code_bits=self.code_bits)

    def fork(self, src, dst, tokens=None):
        """sequence(s) dst -- an int or distinct ints, none of them src -- become copies of sequence src that share its full pages
        (a prompt appended and attended once, then fork(0, range(1, B))): reorder() with the identity except index[d] = src.  tokens:
        src's length as a host int; None reads it back.  What the dst rows held is released"""
        self._paged('fork')
        self._seq('fork', src)
        if isinstance(dst, (bool, str)) or not isinstance(dst, (int, list, tuple, range)):
            raise ValueError(f"HBFPKVCache.fork: dst must be a sequence index or a list of them (got {dst!r})")
        dst = [dst] if isinstance(dst, int) else list(dst)
        for d in dst:
            self._seq('fork', d)
        if src in dst or len(set(dst)) != len(dst):
            raise ValueError(f"HBFPKVCache.fork takes distinct destinations, none the source {src} (got {dst!r})")
        if tokens is None:
            tokens = int(self.lengths[src].item())
        if isinstance(tokens, bool) or not isinstance(tokens, int) or not 0 <= tokens <= self.capacity:
            raise ValueError(f"HBFPKVCache.fork: tokens must be an int in 0..{self.capacity}, the length of sequence {src} (got {tokens!r})")
        index = [src if b in dst else b for b in range(self.batch)]
        self._commit_reorder(*self._plan_reorder(index, [tokens if b == src else 0 for b in range(self.batch)]))

    @property
    def head_cap(self):
        """tokens of a head of the code buffers: a page's, or all the buffers hold"""
        return self.cap if self.pages is None else self.page_tokens

    @property
    def length(self):
        if self.device_lengths:
            raise AttributeError("HBFPKVCache(device_lengths=True) keeps no host length: read cache.lengths (int32 [B] on the device)")
        return self._length

    @length.setter
    def length(self, value):
        if self.device_lengths:
            raise AttributeError("HBFPKVCache(device_lengths=True) keeps no host length: write cache.lengths (int32 [B] on the device)")
        self._length = value

    def _workspace(self, Tq):
        """context()'s block sums for Tq query rows (of every query head) at any length up to the capacity"""
        n = native.kv_dec_ws_bytes(self.batch * self.heads, Tq, self.head_dim, self.cap, self.block)
        return torch.empty(n, dtype=torch.uint8, device=self.k_codes.device)

    def nbytes(self):
        held = list(self.buffers.values()) + ([self.page_table, self.lengths] if self.pages is not None else [])
        return sum(t.numel() * t.element_size() for t in held)

    def reset(self):
        if self.pages is not None:
            for own in self._owned:
                self._drop(own)
            self._owned = [[] for _ in range(self.batch)]
            self._table_host.fill_(-1)
            self.page_table.fill_(-1)
        if self.device_lengths:
            self.lengths.zero_()
            self.overflow.zero_()
            if self.starts is not None:
                self.starts.zero_()
        else:
            self.length = 0
        self.v_codes.zero_()

    def _operand(self, x, what, last, heads=None):
        """x [B, heads, t, last] (heads: the query heads unless given) as the rows of the kv heads, [B kv_heads, heads // kv_heads * t, last]"""
        heads = self.heads if heads is None else heads
        if torch.is_grad_enabled():
            raise ValueError(f"HBFPKVCache.{what}: inference only, called while gradients are recorded (use torch.no_grad())")
        want = (self.batch, heads, last)
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or (x.shape[0], x.shape[1], x.shape[3]) != want or x.shape[2] < 1:
            raise ValueError(f"HBFPKVCache.{what} takes [{self.batch}, {heads}, t >= 1, {last}] (got {tuple(getattr(x, 'shape', ()))})")
        if x.dtype != self.dtype or x.device != self.k_codes.device:
            raise ValueError(f"HBFPKVCache.{what}: the cache holds {self.dtype} on {self.k_codes.device} (got {x.dtype} on {x.device})")
        return x.reshape(self.batch * self.kv_heads, heads // self.kv_heads * x.shape[2], last)

    def _result(self, out, Tq):
        """[B kv_heads, group Tq, n] as [B, heads, Tq, n] (a view)"""
        return out.unflatten(1, (self.group, Tq)).reshape(self.batch, self.heads, Tq, out.shape[-1])

    def _rows(self, what, Tq, tiles_on_grid=False):
        """tiles_on_grid: the launch carries a workgroup per (kv head, tile of 16 rows) on a grid dimension of 65535 (k_kv_pv_split:
        context and attend; the qk kernel strides over the pairs).  A cache without groups leaves that limit to the C entry, as before"""
        if Tq > native.KV_DEC_MAX_TOKENS:
            raise ValueError(f"HBFPKVCache.{what}: device_lengths=True takes up to {native.KV_DEC_MAX_TOKENS} query rows (got {Tq})")
        tiles = self.batch * self.kv_heads * ((self.group * Tq + 15) // 16)
        if tiles_on_grid and self.group > 1 and tiles > 65535:
            raise ValueError(f"HBFPKVCache.{what}: {self.batch} x {self.kv_heads} kv heads of {self.group} x {Tq} query rows are {tiles} "
                             "tiles of 16 rows, the grid takes 65535")

    def append(self, k_new, v_new, counts=None):
        """k_new, v_new [B, kv_heads, t, D] become tokens length .. length + t - 1 (one launch for a prefill chunk or one token).  With
        device_lengths: per sequence, at lengths[b], the first counts[b] rows (the class docstring); two launches, returns None"""
        k, v = (self._operand(x, 'append', self.head_dim, self.kv_heads) for x in (k_new, v_new))
        t = k.shape[1]
        if v.shape[1] != t:
            raise ValueError(f"HBFPKVCache.append: {t} keys and {v.shape[1]} values")
        if not self.device_lengths and counts is not None:
            raise ValueError("HBFPKVCache.append: counts needs device_lengths=True")
        if self.device_lengths:
            if t > self.cap:
                raise ValueError(f"HBFPKVCache.append: a chunk of {t} tokens exceeds the buffers' {self.cap}")
            if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != (self.batch,)
                                       or counts.device != self.k_codes.device or not counts.is_contiguous()):
                raise ValueError(f"HBFPKVCache.append: counts must be a contiguous int32 tensor [{self.batch}] on {self.k_codes.device}")
            native.kv_append_dev(k.contiguous(), v.contiguous(), self.k_codes, self.k_exps, self.v_codes, self.v_exps, self.v_tail, self.lengths,
                                 counts, self.overflow, self.kv_heads, self.capacity, self.block, self.mant_bits, self.epsilon, pages=self.pages,
                                 code_bits=self.code_bits)
            return None
        if self.length + t > self.capacity:
            raise ValueError(f"HBFPKVCache.append: {self.length} + {t} tokens exceed the capacity {self.capacity}")
        native.kv_append(k.contiguous(), v.contiguous(), self.k_codes, self.k_exps, self.v_codes, self.v_exps, self.v_tail, self.length,
                         self.block, self.mant_bits, self.epsilon)
        self.length += t
        return self.length

    def _in_kernel(self, rows):
        """the host-length cache quantizes up to 16 dense rows per (kv) head inside the product kernel"""
        return self.act is None and rows <= native.KV_DEC_MAX_TOKENS

    def scores(self, q, max_len=None):
        """q [B, H, Tq, D] -> [B, H, Tq, S]: Q_in(q) @ Q_w(K_all)^T.  With device_lengths: [B, H, Tq, max_len], -inf from lengths[b] on.
        A product, not attention: window and starts do not act here"""
        x = self._operand(q, 'scores', self.head_dim)
        Tq = q.shape[2]
        if not self.device_lengths and max_len is not None:
            raise ValueError("HBFPKVCache.scores: max_len needs device_lengths=True")
        if self.device_lengths:
            self._rows('scores', Tq)
            n = self.capacity if max_len is None else max_len
            if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= self.capacity:
                raise ValueError(f"HBFPKVCache.scores: max_len must be an int in 1..{self.capacity} (got {max_len!r})")
            out = native.kv_bmm_dec_dev(x, self.k_codes, self.k_exps, native.KV_QK, n, self.head_cap, self.lengths, self.kv_heads, self.block,
                                        self.mant_bits, self.epsilon, group=self.group, pages=self.pages, code_bits=self.code_bits)
            self.stats.cache_calls += 1
            return self._result(out, Tq)
        S, D, BH, R, m = self.length, self.head_dim, x.shape[0], x.shape[1], self.mant_bits   # R = group * Tq rows per kv head
        if S < 1:
            raise ValueError("HBFPKVCache.scores: the cache is empty")
        if self._in_kernel(R):
            out = native.kv_bmm_dec(x, self.k_codes, self.k_exps, native.KV_QK, S, self.cap, self.block, m, self.epsilon)
        else:
            xq = native.act_codes(x.reshape(BH * R, D), m, self.epsilon, self.act, block_size=self.block)
            N = (S + 15) // 16 * 16                               # rows S .. N - 1 repeat key S - 1 and are dropped
            out = native.hbfp_bmm_i8_strided(xq, self.k_codes, self.k_exps, BH, R, N, D, self.cap, S, m, m, block_size=self.block,
                                             out_dtype=self.dtype)[:, :, :S]
        self.stats.cache_calls += 1
        return self._result(out, Tq)

    def context(self, p):
        """p [B, H, Tq, S] -> [B, H, Tq, D]: Q_in(p) @ Q_w(V_all^T)^T, blocks along the S cached tokens (the last one zero-padded).  With
        device_lengths: p [B, H, Tq, L], 1 <= L <= capacity, sequence b over its first min(lengths[b], L) tokens.  A product, not
        attention: window and starts do not act here"""
        if self.device_lengths:
            if not isinstance(p, torch.Tensor) or p.dim() != 4 or not 1 <= p.shape[-1] <= self.capacity:
                raise ValueError(f"HBFPKVCache.context takes p [..., L], 1 <= L <= {self.capacity} (got {tuple(getattr(p, 'shape', ()))})")
            x = self._operand(p, 'context', p.shape[-1])
            Tq = p.shape[2]
            self._rows('context', Tq, tiles_on_grid=True)
            if Tq > self.max_query_rows:
                raise ValueError(f"HBFPKVCache.context: {Tq} query rows, the workspace was made for max_query_rows={self.max_query_rows}")
            out = native.kv_bmm_dec_dev(x, self.v_codes, self.v_exps, native.KV_PV, self.head_dim, self.head_dim, self.lengths, self.kv_heads,
                                        self.block, self.mant_bits, self.epsilon, ws=self._ws, chunks_per_split=self.chunks_per_split,
                                        group=self.group, pages=self.pages, code_bits=self.code_bits)
            self.stats.cache_calls += 1
            return self._result(out, Tq)
        if not isinstance(p, torch.Tensor) or p.dim() != 4 or p.shape[-1] != self.length or self.length < 1:
            raise ValueError(f"HBFPKVCache.context takes p [..., {self.length}], the cached length >= 1 (got {tuple(getattr(p, 'shape', ()))})")
        x = self._operand(p, 'context', self.length)
        S, D, BH, R, m, blk = self.length, self.head_dim, x.shape[0], x.shape[1], self.mant_bits, self.block
        if self._in_kernel(R):
            out = native.kv_bmm_dec(x, self.v_codes, self.v_exps, native.KV_PV, D, D, blk, m, self.epsilon)
        else:
            Sp = (S + blk - 1) // blk * blk
            if Sp != S:
                if self.act is not None and (self.act.mode != 'structured' or blk % self.act.M):
                    raise ValueError(f"HBFPKVCache.context: in_sparsity {self.act.mode} on p needs S % block_size == 0 "
                                     f"(or N:M with M dividing the block); S = {S}")
                # the reference's zero pad of the last block (bfp_ops.py:50-53; for N:M its pad to M, :79-82, and all-zero groups); p is small
                x = F.pad(x, (0, Sp - S))
            xq = native.act_codes(x.reshape(BH * R, Sp), m, self.epsilon, self.act, block_size=blk)
            out = native.hbfp_bmm_i8_strided(xq, self.v_codes, self.v_exps, BH, R, D, Sp, D, D, m, m, block_size=blk, out_dtype=self.dtype)
        self.stats.cache_calls += 1
        return self._result(out, p.shape[2])

    def prepare_attend(self):
        """make attend()'s workspaces now (the fp32 score rows of max_query_rows rows over the whole capacity and, with prompt_rows, of
        a panel); they are never grown"""
        if not self.device_lengths:
            raise ValueError("HBFPKVCache.attend needs device_lengths=True")
        if self._att_ws is None:
            n = native.kv_attend_ws_bytes(self.batch * self.heads, self.max_query_rows, self.cap)
            self._att_ws = torch.empty(n, dtype=torch.uint8, device=self.k_codes.device)
        if self.prompt_rows and self._rows_ws is None:
            n = native.kv_attend_rows_ws_bytes(self.batch * self.heads, self.prompt_rows, self.cap)
            self._rows_ws = torch.empty(n, dtype=torch.uint8, device=self.k_codes.device)

    def attend(self, q, scale, max_len=None, causal=False, return_probs=False):
        """q [B, H, Tq, D] -> the context [B, H, Tq, D] of softmax(scores(q, max_len) * scale) (the class docstring); with return_probs
        also p [B, H, Tq, max_len].  device_lengths only; two products, three launches.  More than 16 rows need prompt_rows (the
        class docstring): two launches per panel.  A cache with window / starts takes the rows' first keys from them"""
        if not self.device_lengths:
            raise ValueError("HBFPKVCache.attend needs device_lengths=True")
        x = self._operand(q, 'attend', self.head_dim)
        Tq = q.shape[2]
        panels = self.prompt_rows > 0 and Tq > native.KV_DEC_MAX_TOKENS
        if not panels:
            self._rows('attend', Tq, tiles_on_grid=True)
            if Tq > self.max_query_rows:
                raise ValueError(f"HBFPKVCache.attend: {Tq} query rows, the workspaces were made for max_query_rows={self.max_query_rows}")
        if isinstance(scale, bool) or not isinstance(scale, numbers.Real) or not math.isfinite(scale) or abs(scale) > torch.finfo(torch.float32).max:
            raise ValueError(f"HBFPKVCache.attend: scale must be a finite real number (in fp32; got {scale!r})")
        n = self.capacity if max_len is None else max_len
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= self.capacity:
            raise ValueError(f"HBFPKVCache.attend: max_len must be an int in 1..{self.capacity} (got {max_len!r})")
        self.prepare_attend()
        if panels:
            out, p = native.kv_attend_rows(x, self.k_codes, self.k_exps, self.v_codes, self.v_exps, self.lengths, self.kv_heads, n, float(scale),
                                           bool(causal), self.block, self.mant_bits, self.epsilon, self._rows_ws, self.prompt_rows,
                                           return_probs=bool(return_probs), group=self.group, starts=self.starts, window=self.window,
                                           pages=self.pages, code_bits=self.code_bits)
            self.stats.cache_calls += 2
            out = self._result(out, Tq)
            return (out, self._result(p, Tq)) if return_probs else out
        out, p = native.kv_attend(x, self.k_codes, self.k_exps, self.v_codes, self.v_exps, self.lengths, self.kv_heads, n, float(scale),
                                  bool(causal), self.block, self.mant_bits, self.epsilon, self._att_ws, self._ws,
                                  chunks_per_split=self.chunks_per_split, return_probs=bool(return_probs), group=self.group,
                                  starts=self.starts, window=self.window, pages=self.pages, code_bits=self.code_bits)
        self.stats.cache_calls += 2
        out = self._result(out, Tq)
        return (out, self._result(p, Tq)) if return_probs else out

    def _held(self, b):
        """(first sequence, sequences, S) of keys() / values(): everything at the host length, or sequence b at lengths[b] (read back)"""
        if not self.device_lengths:
            if b is not None:
                raise ValueError("HBFPKVCache.keys / values: a sequence index needs device_lengths=True")
            return 0, self.batch, self.length
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.batch:
            raise ValueError(f"HBFPKVCache.keys / values: device_lengths=True takes a sequence index in 0..{self.batch - 1} (got {b!r})")
        return b, 1, int(self.lengths[b].item())

    def _gathered(self, buf, b, S, axis):
        """a paged buffer [N, kv_heads, .., ..] as sequence b's contiguous heads [kv_heads, .., ..], the pages of its first S tokens
        (the table row read back, as lengths[b] was) side by side along `axis`, the one the tokens run along"""
        n = (S + self.page_tokens - 1) // self.page_tokens
        idx = self.page_table[b, :n].to(torch.int64).clamp_(0, self.page_count - 1)
        t = buf[idx]                                              # [n, kv_heads, a, b]
        if axis == 2:
            return t.permute(1, 0, 2, 3).reshape(self.kv_heads, n * t.shape[2], t.shape[3])
        return t.permute(1, 2, 0, 3).reshape(self.kv_heads, t.shape[2], n * t.shape[3])

    def keys(self, b=None):
        """the cached keys dequantized, [B, kv_heads, S, D]; with device_lengths those of sequence b, [1, kv_heads, lengths[b], D]"""
        b0, nb, S = self._held(b)
        BH, D, cb = nb * self.kv_heads, self.head_dim, self.code_bits
        Dc = D * cb // 8                                          # bytes of a row's D codes
        if self.pages is not None:
            kc, ke = (self._gathered(t, b, S, 2) for t in (self.k_codes, self.k_exps))   # [kv_heads, tokens, .]
            c, e = kc[:, :S, :Dc].reshape(BH * S, Dc), ke[:, :S].reshape(BH * S, D // self.block)
            return native.dequantize(c, e, D, self.dtype, self.block, self.mant_bits, cb).view(nb, self.kv_heads, S, D)
        c = self.k_codes[b0:b0 + nb].view(BH, self.cap, -1)[:, :S, :Dc].reshape(BH * S, Dc)
        e = self.k_exps[b0:b0 + nb].view(BH, self.cap, -1)[:, :S].reshape(BH * S, D // self.block)
        return native.dequantize(c, e, D, self.dtype, self.block, self.mant_bits, cb).view(nb, self.kv_heads, S, D)

    def values(self, b=None):
        """the cached values dequantized, [B, kv_heads, S, D]; with device_lengths those of sequence b, [1, kv_heads, lengths[b], D]"""
        b0, nb, S = self._held(b)
        BH, D, blk, cb = nb * self.kv_heads, self.head_dim, self.block, self.code_bits
        Sp = (S + blk - 1) // blk * blk
        Sc = Sp * cb // 8                                         # bytes of a column's Sp codes
        if self.pages is not None:
            c = self._gathered(self.v_codes, b, S, 3).reshape(BH * D, -1)[:, :Sc].contiguous()
            e = self._gathered(self.v_exps, b, S, 3).reshape(BH * D, -1)[:, :Sp // blk].contiguous()
        else:
            c = self.v_codes[b0:b0 + nb].view(BH * D, -1)[:, :Sc].contiguous()
            e = self.v_exps[b0:b0 + nb].view(BH * D, -1)[:, :Sp // blk].contiguous()
        v = native.dequantize(c, e, Sp, self.dtype, blk, self.mant_bits, cb)[:, :S]
        return v.reshape(nb, self.kv_heads, D, S).transpose(-1, -2)


def F_matmul_bfp(matrix_unit=False, **kwargs):
    """reference: bfp_ops.py:240-245.  matrix_unit='int8': inference calls that matmul_route accepts run as one batched GEMM on the int8
    matrix unit (exact block sums, fp32 across blocks; agrees with the plain composition up to that summation order), everything else as
    without it; the op then carries matmul_stats.  False (the default): the reference's composition.  Any other value raises ValueError --
    True included: there is no block-scaled batched route."""
    mu = matrix_unit_value(matrix_unit)
    if mu is True:
        raise ValueError("F_matmul_bfp: matrix_unit must be False or 'int8' (there is no block-scaled batched route)")
    bfp_args = unpack_bfp_args(kwargs)
    if bfp_args['num_format'] != 'bfp':
        return torch.matmul
    return _gen_matmul_i8_op(bfp_args, mu) if mu else _get_bfp_op(torch.matmul, 'matmul', bfp_args, True)


class _BFPModule:
    """shared by BFPLinear / BFPConv2d: config capture before nn.Module.__init__, format dispatch in forward"""

    def _bfp_setup(self, kwargs, functional, op_name):
        self.bfp_args = unpack_bfp_args(kwargs)
        self._functional = functional
        self._op_name = op_name

    def _bfp_finish(self):
        self.num_format = self.bfp_args['num_format']
        return _get_bfp_op(self._functional, self._op_name, self.bfp_args)

    def enable_weight_cache(self, enabled=True, matrix_unit=False):
        """opt in to (or out of) caching the quantized weight across forwards; see WeightCache.  matrix_unit=True additionally
        runs the Linear itself on the block-scaled matrix instruction where the configuration allows (HBFP4-class, block 64,
        >= 32 tokens): the same block products, summed exactly inside a block and in fp32 across blocks instead of by the bf16
        library GEMM -- results agree with F.linear on the fake-quantised operands up to that summation order.  matrix_unit='int8' runs it
        instead on the int8 matrix instruction for HBFP up to 8 bits (block 64, 32 or 16, mant_bits 1..7, any number of tokens,
        N % 16 == 0 and K % 64 == 0; WeightCache.i8_calls counts these calls).  Any other value raises ValueError."""
        cache = WeightCache(self, matrix_unit=matrix_unit) if enabled else None
        self._weight_cache = cache                               # (patch.prime_weight_caches fills it for a whole model in one list call)
        return self._bfp_rebuild_op()

    def _bfp_rebuild_op(self):
        op = _get_bfp_op(self._functional, self._op_name, self.bfp_args, cache=getattr(self, '_weight_cache', None),
                         stoc=getattr(self, '_stoc_matrix_unit', None))
        if hasattr(self, 'linear_op'):
            self.linear_op = op
        else:
            self.conv_op = op
        return self

    def _bfp_forward(self, bfp_op, *operands):
        if self.num_format == 'fp32':
            return self._functional(*operands)
        if self.num_format == 'bfp':
            return bfp_op(*operands)
        raise NotImplementedError('NumFormat not implemented')


class BFPConv2d(_BFPModule, torch.nn.Conv2d):
    """reference: bfp_ops.py:247-268 (no extra parameters or buffers: state_dict == nn.Conv2d's)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, bias=True, **kwargs):
        self._bfp_setup(kwargs, F.conv2d, 'Conv2d')
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)
        self.conv_op = self._bfp_finish()

    def forward(self, input):
        return self._bfp_forward(self.conv_op, input, self.weight, self.bias, self.stride, self.padding,
                                 self.dilation, self.groups)


class BFPLinear(_BFPModule, torch.nn.Linear):
    """reference: bfp_ops.py:270-287 (no extra parameters or buffers: state_dict == nn.Linear's)"""

    def __init__(self, in_features, out_features, bias=True, **kwargs):
        self._bfp_setup(kwargs, F.linear, 'linear')
        torch.nn.Linear.__init__(self, in_features, out_features, bias)
        self.linear_op = self._bfp_finish()

    def forward(self, input):
        return self._bfp_forward(self.linear_op, input, self.weight, self.bias)

    def enable_stochastic_matrix_unit(self, matrix_unit=True):
        """opt in to (or, with False, out of) running 'stoc' inference forwards on a matrix unit (StocMatrixUnit): True takes the
        block-scaled unit where _stoc_route allows and the int8 unit elsewhere, 'int8' the int8 unit only; any other value raises
        ValueError.  It applies under no_grad to 'bfp' configurations with bf16 or fp32 operands of one dtype, a 2-D weight and no
        bias or an fp32 one; every other forward runs as without it.  The operands are those of the fake route for the same seeds; the
        output is fp32, the block products summed exactly and in fp32 across blocks.  Independent of enable_weight_cache."""
        mu = matrix_unit_value(matrix_unit)
        self._stoc_matrix_unit = StocMatrixUnit(mu) if mu else None
        return self._bfp_rebuild_op()
