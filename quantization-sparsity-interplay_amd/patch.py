"""Patch an existing torch model in place: every nn.Linear (optionally nn.Conv2d) that the reference's patched
model files build as BFPLinear / BFPConv2d becomes one, sharing the original parameters.

The reference does this by editing modeling_*.py (e.g. llama/modeling_llama.py:225-237,305-319: q/k/v/o and
gate/up/down become BFPLinear, lm_head stays nn.Linear, llama/modeling_llama.py:1166); for an unmodified upstream
model the same result is obtained by swapping the modules after construction."""
import torch

from . import native
from .bfp import bfp_ops


def patch_linear_layers(model, bfp_args, skip=("lm_head", "classifier", "score"), convs=False, cache_weights=False, matrix_unit=False,
                        stoc_matrix_unit=False):
    """Replace nn.Linear children by bfp_ops.BFPLinear(**bfp_args) that reuse weight / bias.  Modules whose
    qualified name ends with an entry of `skip` stay as they are (the reference leaves the LM heads alone).
    matrix_unit (False, True or 'int8'): with cache_weights, the cached Linear forward's matrix-unit route (BFPLinear.enable_weight_cache).
    stoc_matrix_unit (False, True or 'int8'): the 'stoc' inference forwards' matrix-unit route (BFPLinear.enable_stochastic_matrix_unit).
    Returns the list of patched module names."""
    bfp_ops.matrix_unit_value(matrix_unit)                  # (a wrong value raises before any module is replaced)
    stoc_matrix_unit = bfp_ops.matrix_unit_value(stoc_matrix_unit)
    patched = []
    for parent_name, parent in list(model.named_modules()):
        for child_name, child in list(parent.named_children()):
            full = f"{parent_name}.{child_name}" if parent_name else child_name
            if any(full.endswith(s) for s in skip):
                continue
            new = None
            if type(child) is torch.nn.Linear:
                new = bfp_ops.BFPLinear(child.in_features, child.out_features, child.bias is not None, **dict(bfp_args))
            elif convs and type(child) is torch.nn.Conv2d:
                new = bfp_ops.BFPConv2d(child.in_channels, child.out_channels, child.kernel_size, child.stride, child.padding,
                                        child.dilation, child.groups, child.bias is not None, **dict(bfp_args))
            if new is None:
                continue
            new.weight = child.weight                       # share the parameters: state_dict keys are unchanged
            new.bias = child.bias
            new.train(child.training)
            if cache_weights:
                new.enable_weight_cache(matrix_unit=matrix_unit if isinstance(new, bfp_ops.BFPLinear) else False)
            if stoc_matrix_unit and isinstance(new, bfp_ops.BFPLinear):
                new.enable_stochastic_matrix_unit(stoc_matrix_unit)
            setattr(parent, child_name, new)
            patched.append(full)
    return patched


def prime_weight_caches(model):
    """Fill the (opt-in, inference-only) weight caches of every BFPLinear / BFPConv2d of `model` with ONE list call per configuration
    (bfp_ops.float_to_bfp_blocked_many: large weights in launches of their own over several streams, small ones up to 64 per launch --
    LLaMA-7B's 224 weights in 4.1 ms) instead of one call per module on its first forward.  Modules whose cache is off or not usable
    right now (training mode, gradients being recorded, stochastic rounding) are left alone.  Returns the number of weights stored."""
    groups = {}
    for m in model.modules():
        cache = getattr(m, '_weight_cache', None)
        if cache is None or getattr(m, 'num_format', None) != 'bfp' or not isinstance(m, (bfp_ops.BFPLinear, bfp_ops.BFPConv2d)):
            continue
        with torch.no_grad():
            if not cache.usable(m.weight, m.bfp_args) or m.weight.device.type != 'cuda':
                continue
        key = (m.weight.dtype, m.weight.device, tuple(sorted((k, repr(v)) for k, v in m.bfp_args.items())))
        groups.setdefault(key, []).append(m)
    n = 0
    for mods in groups.values():
        with torch.no_grad():
            outs = bfp_ops.float_to_bfp_blocked_many([m.weight.detach() for m in mods], identifier='w', **dict(mods[0].bfp_args))
            for m, o in zip(mods, outs):
                m._weight_cache.store(m.weight, o, m.bfp_args)
                n += 1
    return n


class PackedBFPLinear(torch.nn.Module):
    """Inference-only Linear whose weight lives in packed HBFP form -- what a BFPLinear with w_sparsity / HBFP computes in its forward,
    with the weight quantized ONCE.  HBFP4 (mant_bits <= 3): 4-bit codes + one int8 exponent per block of 64 (0.516 B per weight
    instead of 2), run by PackedBFP.linear (up to 64 tokens straight from the codes on the int8 matrix cores, more tokens on the
    block-scaled matrix instruction or the library GEMM).  HBFP5-HBFP8 (mant_bits 4..7): 8-bit codes (1.016 B per weight), run by
    PackedBFP.linear_i8 on the int8 matrix instruction up to bfp_ops.I8_MAX_TOKENS tokens; more than 64 tokens of HBFP5, more tokens
    and shapes the int8 unit does not take run PackedBFP.linear's routes (bfp_ops.linear_route picks the route of every forward).
    HBFP blocks of 32 or 16 (4- or 8-bit codes) run on the int8 matrix instruction up to bfp_ops.i8_small_block_max_tokens(block, x.dtype)
    tokens (any number for fp32 activations).
    The codes and exponents are registered buffers (`codes`, `exps`): they follow .to() / .cuda(), appear in state_dict()
    and load back with load_state_dict(); shape / dtype / mantissa width / activation pruning travel as extra state.
    x_sparsity (native.ActSparsity or None): the activations are pruned as the reference's in_sparsity does.
    hold_image (default True): prefill forwards of a 4-bit block-64 weight keep an e4m3 image of the weight (1.016 B per weight on top
    of the 0.516 of the codes) from the first one on.  False: they read the codes themselves (native.hbfp_linear_mx4w), the image is
    never made and the outputs are the same bit for bit, at 1.07-1.73 x the time of the default
    (measured per shape: bfp_ops.HOLD_IMAGE_TIME; from 8192 tokens on a weight of up to 4096 x 4096 runs the dequantize + library GEMM route
    instead, bfp_ops.codes_route, which keeps no image either but sums in another order).  Travels as extra state."""

    def __init__(self, packed, bias=None, x_mant_bits=7, epsilon=1e-8, x_sparsity=None, hold_image=True):
        super().__init__()
        self.out_features, self.in_features = packed.shape
        self.x_mant_bits, self.epsilon = int(x_mant_bits), float(epsilon)
        self.x_sparsity = x_sparsity
        self.hold_image = bool(hold_image)
        self.register_buffer("codes", packed.codes)
        self.register_buffer("exps", packed.exps)
        self._meta = dict(shape=list(packed.shape), dtype=str(packed.dtype).replace("torch.", ""), mant_bits=packed.mant_bits,
                          block_size=packed.block_size, code_bits=packed.code_bits)
        self._packed = packed
        self.bias = None if bias is None else torch.nn.Parameter(bias.detach(), requires_grad=False)

    @property
    def packed(self):
        """the PackedBFP view of the buffers (rebuilt when .to() / load_state_dict() replaced them; the MFMA-tiled copy of the
        decode kernel is then re-made lazily on the new device)"""
        p = self._packed
        if p is None or p.codes is not self.codes or p.exps is not self.exps:
            m = self._meta
            p = self._packed = bfp_ops.PackedBFP(self.codes, self.exps, tuple(m['shape']), getattr(torch, m['dtype']), m['mant_bits'],
                                                 m['block_size'], m['code_bits'])
        return p

    def get_extra_state(self):
        return dict(self._meta, x_mant_bits=self.x_mant_bits, epsilon=self.epsilon,
                    x_sparsity=None if self.x_sparsity is None else self.x_sparsity.as_dict(), hold_image=self.hold_image)

    def set_extra_state(self, state):
        self._meta = {k: state[k] for k in ('shape', 'dtype', 'mant_bits', 'block_size', 'code_bits')}
        self.x_mant_bits, self.epsilon = int(state['x_mant_bits']), float(state['epsilon'])
        self.x_sparsity = native.ActSparsity.from_dict(state.get('x_sparsity'))     # (a state saved before activation pruning: dense)
        self.hold_image = bool(state.get('hold_image', True))                       # (a state saved before the switch: the image is held)
        self._packed = None

    @classmethod
    def from_linear(cls, lin, bfp_args, hold_image=True):
        """weight -> PackedBFP.from_bfp_args with the module's config (format 'bfp', block 64, 32 or 16, mant_bits 1..7 -- 4-bit codes up to 3,
        8-bit codes from 4 --, round-half-even, N:M or prune-first unstructured weight pruning); activations use mant_bits of the same
        config.  Pruned activations (in_sparsity: N:M or unstructured, either order, the same keys) are pruned in every forward, as the
        reference does.  Configurations this module cannot reproduce (unstructured WEIGHT pruning after quantization, stochastic
        rounding) are refused.  hold_image: as the constructor's."""
        a = bfp_ops.unpack_bfp_args(dict(bfp_args))
        pw = bfp_ops.PackedBFP.from_bfp_args(lin.weight.detach(), a)
        return cls(pw, lin.bias, a['mant_bits'], a['epsilon'], native.ActSparsity.from_bfp_args(a), hold_image=hold_image)

    def forward(self, x):
        p = self.packed
        N, K = p.shape
        T = x.numel() // K if K else 0
        route = bfp_ops.linear_route(T, N, K, p.code_bits, p.mant_bits, self.x_mant_bits, i8_max_tokens=bfp_ops.I8_MAX_TOKENS,
                                     block_size=p.block_size, dtype=x.dtype)
        return p._run_linear(route, x, self.bias, self.x_mant_bits, self.epsilon, self.x_sparsity, self.hold_image)

    def extra_repr(self):
        act = "" if self.x_sparsity is None else f", x_sparsity={tuple(self.x_sparsity)}"
        lean = "" if self.hold_image else ", hold_image=False"
        return (f"in_features={self.in_features}, out_features={self.out_features}, packed_bytes={self.packed.nbytes()}, "
                f"resident_bytes={self.packed.resident_bytes()}{act}{lean}")


class Sparse24BFPLinear(torch.nn.Module):
    """Inference-only Linear whose N:4-pruned (N <= 2) HBFP block-64 weight lives in the 2:4-compressed form (bfp_ops.SparseBFP24): the two
    kept codes of every group of 4 + their positions + the block exponents, 0.391 B per weight for 4-bit codes (mant_bits <= 3), 0.641 B
    for 8-bit codes (4..7).  Up to bfp_ops.SP24_DECODE_TOKENS tokens the forward runs on the sparse int8 matrix instruction straight from
    that form; more tokens run the route PackedBFPLinear takes, on an expansion of the weight made for that call only.  A sibling of
    PackedBFPLinear with the same conventions: buffers `vals`, `idx`, `exps` follow .to() and round-trip through state_dict(); shape /
    dtype / mantissa width / activation pruning travel as extra state; x_sparsity prunes the activations as the reference's in_sparsity."""

    def __init__(self, sparse, bias=None, x_mant_bits=7, epsilon=1e-8, x_sparsity=None):
        super().__init__()
        self.out_features, self.in_features = sparse.shape
        self.x_mant_bits, self.epsilon = int(x_mant_bits), float(epsilon)
        self.x_sparsity = x_sparsity
        self.register_buffer("vals", sparse.vals)
        self.register_buffer("idx", sparse.idx)
        self.register_buffer("exps", sparse.exps)
        self._meta = dict(shape=list(sparse.shape), dtype=str(sparse.dtype).replace("torch.", ""), mant_bits=sparse.mant_bits,
                          code_bits=sparse.code_bits)
        self._sparse = sparse
        self.bias = None if bias is None else torch.nn.Parameter(bias.detach(), requires_grad=False)

    @property
    def sparse(self):
        """the SparseBFP24 view of the buffers (rebuilt when .to() / load_state_dict() replaced them)"""
        s = self._sparse
        if s is None or s.vals is not self.vals or s.idx is not self.idx or s.exps is not self.exps:
            m = self._meta
            s = self._sparse = bfp_ops.SparseBFP24(self.vals, self.idx, self.exps, tuple(m['shape']), getattr(torch, m['dtype']),
                                                   m['mant_bits'], m['code_bits'])
        return s

    def get_extra_state(self):
        return dict(self._meta, x_mant_bits=self.x_mant_bits, epsilon=self.epsilon,
                    x_sparsity=None if self.x_sparsity is None else self.x_sparsity.as_dict())

    def set_extra_state(self, state):
        self._meta = {k: state[k] for k in ('shape', 'dtype', 'mant_bits', 'code_bits')}
        self.x_mant_bits, self.epsilon = int(state['x_mant_bits']), float(state['epsilon'])
        self.x_sparsity = native.ActSparsity.from_dict(state.get('x_sparsity'))
        self._sparse = None

    @classmethod
    def from_linear(cls, lin, bfp_args):
        """weight -> SparseBFP24.from_bfp_args with the module's config (which must guarantee the 2:4 / 1:4 pattern: ValueError
        otherwise); activations use mant_bits of the same config and are pruned as its in_sparsity keys say"""
        a = bfp_ops.unpack_bfp_args(dict(bfp_args))
        sp = bfp_ops.SparseBFP24.from_bfp_args(lin.weight.detach(), a)
        return cls(sp, lin.bias, a['mant_bits'], a['epsilon'], native.ActSparsity.from_bfp_args(a))

    def forward(self, x):
        return self.sparse.linear(x, self.bias, self.x_mant_bits, self.epsilon, self.x_sparsity)

    def extra_repr(self):
        act = "" if self.x_sparsity is None else f", x_sparsity={tuple(self.x_sparsity)}"
        return f"in_features={self.in_features}, out_features={self.out_features}, sp24_bytes={self.sparse.nbytes()}{act}"


def pack_linear_layers(model, bfp_args, skip=("lm_head", "classifier", "score"), sparse24=False, hold_image=True):
    """Inference deployment: replace nn.Linear / BFPLinear children by PackedBFPLinear (weights quantized once and
    held as 4-bit codes for mant_bits <= 3, 8-bit codes for 4..7; the original bf16/fp16 weight is dropped).  Needs an HBFP config with
    block_size 64, 32 or 16 and mant_bits <= 7 (+ optional N:M or unstructured pruning).  Returns the patched names and the bytes saved.
    sparse24=True: Sparse24BFPLinear instead (the 2:4-compressed form); the config must guarantee the pattern -- block 64, N:4 weight
    pruning with N <= 2 (bfp_ops.sp24_config_check) -- or ValueError is raised before any module is replaced.
    hold_image=False: the PackedBFPLinear modules run their prefill forwards from the codes and never make the weight's e4m3 image
    (PackedBFPLinear; Sparse24BFPLinear holds no image and ignores it).  The bytes saved count codes and exponents either way."""
    patched, saved = [], 0
    a = bfp_ops.unpack_bfp_args(dict(bfp_args))
    if sparse24:
        bfp_ops.sp24_config_check(a)
    # 8-bit codes, and every code width at blocks 16 / 32, run at any K % 64 == 0 (PackedBFP.linear_i8); sp24 takes any K % 64 == 0
    k_mult = 256 if bfp_ops.code_bits_for(a['mant_bits']) == 4 and a['block_size'] == 64 and not sparse24 else 64
    for parent_name, parent in list(model.named_modules()):
        for child_name, child in list(parent.named_children()):
            full = f"{parent_name}.{child_name}" if parent_name else child_name
            if any(full.endswith(s) for s in skip) or not isinstance(child, torch.nn.Linear):
                continue
            if child.in_features % k_mult or child.out_features % 16:
                continue                                    # shapes the packed kernels do not take stay as they are
            new = Sparse24BFPLinear.from_linear(child, bfp_args) if sparse24 else PackedBFPLinear.from_linear(child, bfp_args, hold_image)
            saved += child.weight.numel() * child.weight.element_size() - (new.sparse if sparse24 else new.packed).nbytes()
            setattr(parent, child_name, new)
            patched.append(full)
    return patched, saved
