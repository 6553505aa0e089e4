"""ctypes binding of libbfpq.so (include/bfpq.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the HIP stream; every byte of arithmetic on the
hot path happens in the HIP kernels of csrc/bfpq_kernels.hip.  There is NO CPU fallback: if the
library is missing, or a tensor is not on a ROCm device, the calls raise.
"""
import collections
import ctypes
import math
import os
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libbfpq.so"
_lock = threading.Lock()
_lib = None

F32, F16, BF16 = 0, 1, 2
DTYPE_CODE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
BFPQ_E_UNSUPPORTED = -2

EXP_WIN_ENTRIES = 320
NM4_LUT_ENTRIES = 729
NM4_MASK_BYTES = 5888
NM8_LUT_ENTRIES = 1 << 24
USE_NM8_TABLE = True               # False: N:8 groups with straddling ties replay nth_element in the kernel (tests)
SELECT_STATE_BYTES = 80
SELECT_HIST_ENTRIES = 32768 + 256
SELECT_HIST_COPIES = 8


# include/bfpq.h, entry by entry: name -> (restype, argtypes)
_vp, _i64, _i32, _u64, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_double
PROTOTYPES = {
    "bfpq_version": (_i32, []),
    "bfpq_tune": (_i32, [_i32, _i32]),
    "bfpq_error_string": (ctypes.c_char_p, [_i32]),
    "bfpq_exp_window_host": (_i32, [_i32, _vp]),
    "bfpq_nm4_lut_host": (_i32, [_i32, _vp]),
    "bfpq_nm4_masks_host": (_i32, [_i32, _vp]),
    "bfpq_nm4_lut_bind": (_i32, [_vp, _vp]),
    "bfpq_nm8_lut_host": (_i32, [_i32, _vp]),
    "bfpq_compact24": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "bfpq_expand24": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "bfpq_nm_prune_mask_host": (_u64, [_vp, _i32, _i32]),
    "bfpq_quantize_nm": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32, _i32, _i32, _i32, _u64, _vp, _vp, _vp, _vp]),
    "bfpq_fake_quantize": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "bfpq_fake_quantize_batched": (_i32, [_vp, _vp, _i32, _vp]),
    "bfpq_fake_quantize_list": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32]),
    "bfpq_is_fused": (_i32, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "bfpq_nm_sparsify": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    "bfpq_select_passes": (_i32, [_i32]),
    "bfpq_select_ws_bytes": (_i64, []),
    "bfpq_select": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp]),
    "bfpq_prune_quantize": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i64, _vp, _vp, _vp]),
    "bfpq_prune_quantize_batched": (_i32, [_vp, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i32, _vp, _vp]),
    "bfpq_prune_quantize_list": (_i32, [_vp, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i32, _vp, _vp, _i32]),
    "bfpq_select_hist": (_i32, [_vp, _i64, _i32, _i32, _i64, _i64, _vp, _vp, _vp]),
    "bfpq_select_resolve": (_i32, [_vp, _i64, _i32, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp]),
    "bfpq_select_resolve_ex": (_i32, [_vp, _i64, _i32, _i32, _i64, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _vp]),
    "bfpq_threshold_apply": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "bfpq_select_reset": (_i32, [_vp, _vp]),
    "bfpq_quantize_threshold": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32, _u64, _vp, _vp, _vp, _vp]),
    "bfpq_int_workspace_elems": (_i64, [_i64]),
    "bfpq_int_quantize": (_i32, [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp]),
    "bfpq_dequantize": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_stoc_widen_f16": (_i32, [_vp, _vp, _i64, _vp]),
    "bfpq_hbfp_linear_slices": (_i32, [_i64, _i64]),
    "bfpq_hbfp_linear_decode": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_tiled_ok": (_i32, [_i64, _i64]),
    "bfpq_hbfp_linear_decode_tiled": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "bfpq_mx8_from_hbfp": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "bfpq_quantize_mx8": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _dbl, _vp, _vp]),
    "bfpq_quantize_mx8_nm": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _dbl, _i32, _i32, _i32, _vp, _vp, _vp]),
    "bfpq_quantize_threshold_mx8": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _dbl, _vp, _vp, _vp]),
    "bfpq_hbfp_linear_mx8_ok": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_mx8": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp]),
    "bfpq_hbfp_linear_mx8_parts": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_mx8_splitk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp]),
    "bfpq_hbfp_linear_mx4w_ok": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_mx4w": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_mx4w_parts": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_mx4w_splitk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp]),
    "bfpq_e4m3_of_code4_host": (_i32, [_vp]),
    "bfpq_hbfp_linear_i8_ok": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_i8_parts": (_i32, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_i8": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_i8_splitk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_decode8_ws": (_i64, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_decode8": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "bfpq_codes4_to_i8": (_i32, [_vp, _vp, _i64, _vp]),
    "bfpq_exp_top_flag": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "bfpq_hbfp_linear_i8b_ok": (_i32, [_i64, _i64, _i64, _i32]),
    "bfpq_hbfp_linear_i8b_parts": (_i32, [_i64, _i64, _i64, _i32]),
    "bfpq_hbfp_linear_i8b": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_i8b_splitk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_linear_decode8b_ws": (_i64, [_i64, _i64, _i64, _i32]),
    "bfpq_hbfp_linear_decode8b": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_sp24_pack": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    "bfpq_sp24_unpack": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "bfpq_hbfp_linear_sp24_ws": (_i64, [_i64, _i64, _i64]),
    "bfpq_hbfp_linear_sp24": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_adam_step_list": (_i32, [_vp, _vp, _i32, _vp]),
    "bfpq_adam_step_list_ok": (_i32, [_i32, _i32]),
    "bfpq_hbfp_bmm_i8_ok": (_i32, [_i64, _i64, _i64, _i64, _i64, _i32]),
    "bfpq_hbfp_bmm_i8": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "bfpq_hbfp_codes_t": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _dbl, _vp, _vp]),
    "bfpq_hbfp_bmm_i8_strided": (_i32, [_vp, _vp, _vp, _vp, _vp] + [_i64] * 9 + [_i32, _i32, _i32, _i32, _vp]),
    "bfpq_kv_ok": (_i32, [_i64, _i64, _i32]),
    "bfpq_kv_append": (_i32, [_vp] * 7 + [_i64] * 6 + [_i32, _i32, _i32, _dbl, _vp, _vp]),
    "bfpq_kv_bmm_dec": (_i32, [_vp, _vp, _vp, _vp] + [_i64] * 9 + [_i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp]),
    "bfpq_kv_append_dev": (_i32, [_vp] * 10 + [_i64] * 7 + [_i32, _i32, _i32, _dbl, _vp, _vp]),
    "bfpq_kv_lens_advance": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "bfpq_kv_dec_ws_bytes": (_i64, [_i64, _i64, _i64, _i64, _i32]),
    "bfpq_kv_bmm_dec_dev": (_i32, [_vp] * 5 + [_i64] * 10 + [_i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _vp]),
    "bfpq_kv_attend_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "bfpq_kv_attend": (_i32, [_vp] * 8 + [_i64] * 9 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _vp]),
    "bfpq_kv_bmm_dec_gqa": (_i32, [_vp] * 5 + [_i64] * 11 + [_i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _vp]),
    "bfpq_kv_attend_gqa": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _vp]),
    "bfpq_kv_attend_rows_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "bfpq_kv_attend_rows": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64,
                                   _vp]),
    "bfpq_kv_attend_gqa_win": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64,
                                      _vp]),
    "bfpq_kv_attend_rows_win": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64,
                                       _vp, _i64, _vp]),
    "bfpq_kv_append_paged": (_i32, [_vp] * 10 + [_i64] * 7 + [_i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _vp]),
    "bfpq_kv_lens_advance_paged": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp]),
    "bfpq_kv_bmm_dec_paged": (_i32, [_vp] * 5 + [_i64] * 11 + [_i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64,
                                     _vp]),
    "bfpq_kv_attend_paged": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64,
                                    _i64, _vp]),
    "bfpq_kv_attend_rows_paged": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _i64,
                                         _i64, _vp, _i64, _i64, _vp]),
    "bfpq_kv_rows_move_ws_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32]),
    "bfpq_kv_rows_move": (_i32, [_vp] * 8 + [_i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i64, _i64, _vp]),
    # the _cb entries (4-bit codes): the entry each extends + [starts, window] + [cap] + [page_table, page_tokens, pages] + code_bits
    "bfpq_kv_append_cb": (_i32, [_vp] * 10 + [_i64] * 7 + [_i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _i32, _vp]),
    "bfpq_kv_bmm_dec_cb": (_i32, [_vp] * 5 + [_i64] * 11 + [_i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32,
                                  _vp]),
    "bfpq_kv_attend_cb": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp,
                                 _i64, _i64, _i32, _vp]),
    "bfpq_kv_attend_rows_cb": (_i32, [_vp] * 8 + [_i64] * 10 + [_dbl, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64,
                                      _vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "bfpq_kv_rows_move_cb": (_i32, [_vp] * 8 + [_i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i64, _i64, _i32, _vp]),
}


class NativeUnavailable(RuntimeError):
    """libbfpq.so is not built / not loadable, or the tensor is not on a ROCm device."""


def lib_path():
    return os.environ.get("BFPQ_LIB") or os.path.join(_HERE, _LIB_NAME)     # (BFPQ_LIB: an instrumented build, tools_dev/)


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return lib_path()


def load_library():
    """dlopen libbfpq.so and declare the prototypes of include/bfpq.h.  Raises NativeUnavailable."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise NativeUnavailable(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                    f"or `make -C {os.path.join(_HERE, 'csrc')}`")
        try:
            L = ctypes.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise NativeUnavailable(f"cannot load {path}: {e}") from e
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
        return _lib


EXPORTED_SYMBOLS = tuple(PROTOTYPES)


def check(rc, what):
    if rc != 0:
        msg = load_library().bfpq_error_string(rc).decode()
        raise RuntimeError(f"{what}: {msg} (code {rc})")


# ---- host-side tables -----------------------------------------------------------------------
def exp_window_host(dtype):
    buf = (ctypes.c_uint8 * EXP_WIN_ENTRIES)()
    check(load_library().bfpq_exp_window_host(DTYPE_CODE[dtype], ctypes.addressof(buf)), "bfpq_exp_window_host")
    return bytes(buf)


def nm4_lut_host(N):
    buf = (ctypes.c_uint8 * NM4_LUT_ENTRIES)()
    check(load_library().bfpq_nm4_lut_host(int(N), ctypes.addressof(buf)), "bfpq_nm4_lut_host")
    return bytes(buf)


def nm_prune_mask_host(keys, N, M):
    arr = (ctypes.c_uint32 * M)(*[int(k) for k in keys])
    return int(load_library().bfpq_nm_prune_mask_host(ctypes.addressof(arr), int(N), int(M)))


_table_cache = {}


def _device_table(kind, key, device, maker):
    ck = (kind, key, device.index if device.index is not None else torch.cuda.current_device())
    t = _table_cache.get(ck)
    if t is None:
        t = torch.frombuffer(bytearray(maker()), dtype=torch.uint8).to(device)
        _table_cache[ck] = t
    return t


def exp_window_dev(dtype, device):
    return _device_table("win", dtype, device, lambda: exp_window_host(dtype))


def nm4_masks_host(N):
    buf = (ctypes.c_uint8 * NM4_MASK_BYTES)()
    check(load_library().bfpq_nm4_masks_host(int(N), ctypes.addressof(buf)), "bfpq_nm4_masks_host")
    return bytes(buf)


def nm4_lut_dev(N, device):
    """the 729-byte table, and behind it (from byte 736 on, 16-byte aligned) its expansion to AND masks, bound to it in the
    library: the packed-output kernels copy the masks instead of expanding the bytes in every workgroup"""
    pad = (-NM4_LUT_ENTRIES) % 16
    first = ("lut", int(N), device.index if device.index is not None else torch.cuda.current_device()) not in _table_cache
    t = _device_table("lut", int(N), device, lambda: nm4_lut_host(N) + bytes(pad) + nm4_masks_host(N))
    if first:
        check(load_library().bfpq_nm4_lut_bind(t.data_ptr(), t.data_ptr() + NM4_LUT_ENTRIES + pad), "bfpq_nm4_lut_bind")
    return t


def nm8_lut_host(N):
    buf = (ctypes.c_uint8 * NM8_LUT_ENTRIES)()
    check(load_library().bfpq_nm8_lut_host(int(N), ctypes.addressof(buf)), "bfpq_nm8_lut_host")
    return buf                                            # (buffer protocol: _device_table copies it once)


def nm8_lut_dev(N, device):
    """16 MiB rank table for N:8 (built on first use per (N, device), ~0.1 s)"""
    return _device_table("lut8", int(N), device, lambda: nm8_lut_host(N))


# ---- tensor plumbing ------------------------------------------------------------------------
def require_device_tensor(t, what="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise NativeUnavailable(f"{what} is on {t.device}; the BFP engine runs on a ROCm device only (no CPU fallback)")
    if t.dtype not in DTYPE_CODE:
        raise TypeError(f"{what} has dtype {t.dtype}; supported: float32, float16, bfloat16")


def rows_cols(t):
    cols = t.shape[-1] if t.dim() > 0 else 1
    rows = (t.numel() // cols) if cols else 0
    return rows, cols


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def quantize_nm(t, block_size, mant_bits, epsilon, N=0, M=0, sparsify_first=True, want_deq=True, code_bits=0,
                want_exp=False, stoch_seed=0, out=None, codes_out=None, exps_out=None):
    """Launch bfpq_quantize_nm on t's device/stream.  Returns (deq | None, codes | None, exps | None)."""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    rows, cols = rows_cols(src)
    dev = src.device
    if src.numel() == 0:                       # nothing to launch; shapes as below
        nb = (cols + block_size - 1) // block_size if block_size > 0 else 0
        return (torch.empty_like(src) if want_deq else None,
                torch.empty((rows, (cols + 1) // 2 if code_bits == 4 else cols), dtype=torch.uint8 if code_bits == 4 else
                            (torch.int8 if code_bits == 8 else torch.int16), device=dev) if code_bits else None,
                torch.empty((rows, nb), dtype=torch.int8, device=dev) if (want_exp and block_size > 0) else None)
    with torch.cuda.device(dev):
        deq = None
        if want_deq:
            deq = out if out is not None else torch.empty_like(src)
        codes = exps = None
        if code_bits and codes_out is not None:
            codes = codes_out                                  # caller-owned, contiguous, right shape
        elif code_bits:
            if code_bits == 4:
                codes = torch.empty((rows, (cols + 1) // 2), dtype=torch.uint8, device=dev)
            elif code_bits == 8:
                codes = torch.empty((rows, cols), dtype=torch.int8, device=dev)
            elif code_bits == 32:
                codes = torch.empty((rows, cols), dtype=torch.float32, device=dev)
            else:
                codes = torch.empty((rows, cols), dtype=torch.int16, device=dev)
        if want_exp and block_size > 0 and exps_out is not None:
            exps = exps_out
        elif want_exp and block_size > 0:
            exps = torch.empty((rows, (cols + block_size - 1) // block_size), dtype=torch.int8, device=dev)
        win = exp_window_dev(src.dtype, dev) if block_size > 0 else None
        lut = nm4_lut_dev(N, dev) if M == 4 else (nm8_lut_dev(N, dev) if (M == 8 and USE_NM8_TABLE) else None)
        fused = L.bfpq_is_fused(rows, cols, DTYPE_CODE[src.dtype], int(block_size), int(N), int(M))
        scratch = None
        if not fused and deq is None and M > 0 and block_size > 0:
            scratch = torch.empty_like(src)
        rc = L.bfpq_quantize_nm(_ptr(src), _ptr(deq), _ptr(codes), _ptr(exps), rows, cols, DTYPE_CODE[src.dtype],
                                int(block_size), int(mant_bits), float(epsilon), int(N), int(M),
                                1 if sparsify_first else 0, int(code_bits), int(stoch_seed),
                                _ptr(win), _ptr(lut), _ptr(scratch), _stream(src))
        check(rc, "bfpq_quantize_nm")
    return deq, codes, exps


class _Plan(ctypes.Structure):
    """include/bfpq.h: bfpq_plan"""
    _fields_ = [("dtype", ctypes.c_int), ("block_size", ctypes.c_int), ("mant_bits", ctypes.c_int), ("N", ctypes.c_int),
                ("M", ctypes.c_int), ("sparsify_first", ctypes.c_int), ("epsilon", ctypes.c_double),
                ("exp_win_dev", ctypes.c_void_p), ("nm_lut_dev", ctypes.c_void_p)]


class _TensorDesc(ctypes.Structure):
    """include/bfpq.h: bfpq_tensor_desc"""
    _fields_ = [("in_dev", ctypes.c_void_p), ("out_dev", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64),
                ("apply_nm", ctypes.c_int), ("reserved", ctypes.c_int)]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _bind(Desc, field, tensors, extras, outs, what, copy=False):
    """the descriptors (Desc) of a list of tensors of one device and dtype for a list entry point of the library: tensor i gets
    one with `field` set to extras[i], or is left as it is where extras[i] is None (its result is itself); outs[i], where given,
    is its output.  Inputs must be contiguous (their storage is bound), or with copy=True are replaced by contiguous copies.
    Returns (device, dtype, outputs, descs, keep): keep[j] is the tensor descriptor j reads (alive while its launches run)."""
    n = len(tensors)
    descs = (Desc * max(n, 1))()
    outputs = [None] * n
    keep = []
    dev = dt = None
    for i, t in enumerate(tensors):
        if dev is None:
            require_device_tensor(t)
            dev, dt = t.device, t.dtype
        elif t.device != dev or t.dtype != dt:
            raise ValueError(f"{what}: the tensors of one list share device and dtype")
        x = extras[i]
        if x is None:
            outputs[i] = t
            continue
        if not t.is_contiguous():
            if not copy:
                raise ValueError(f"{what} needs contiguous inputs (their storage is bound)")
            t = t.contiguous()
        dst = torch.empty_like(t) if outs is None or outs[i] is None else outs[i]
        outputs[i] = dst
        if t.numel() == 0:
            continue
        cols = t.shape[-1] if t.dim() else 1
        d = descs[len(keep)]
        d.in_dev, d.out_dev, d.rows, d.cols = t.data_ptr(), dst.data_ptr(), t.numel() // cols, cols
        setattr(d, field, x)
        keep.append(t)
    return dev, dt, outputs, descs, keep


class _BoundList:
    """A list of tensors of one dtype on one device bound to a list entry point of the library (a _Desc per tensor, its own
    field _FIELD filled from the subclass's per-tensor values): outputs and descriptors are set up once, run() re-issues the
    launches.  The inputs are expected to keep their storage between runs (a model's weights); run() checks every bound
    pointer against the tensor's current one and re-binds a tensor whose storage moved (`model.to(...)`, `p.data = ...`,
    `load_state_dict(assign=True)`) -- a changed dtype, device or element count raises instead of reading freed memory.
    Results are written in place into .outputs."""

    def __init__(self, tensors, extras, outs):
        self.device, self.dtype, self.outputs, self._descs, keep = _bind(self._Desc, self._FIELD, tensors, extras, outs, type(self).__name__)
        self._k = len(keep)
        self._bound = [(t, t.data_ptr(), t.numel()) for t in keep]
        self._addr = ctypes.addressof(self._descs)

    def _rebind(self):
        """descriptor j reads self._bound[j][0]: follow tensors whose storage moved since they were bound; True if one did"""
        moved = False
        for j, (t, ptr, n) in enumerate(self._bound):
            cur = t.data_ptr()
            if cur == ptr:
                continue
            if t.dtype != self.dtype or t.device != self.device or t.numel() != n or not t.is_contiguous():
                raise RuntimeError(f"{type(self).__name__}: a bound tensor changed dtype / device / size / layout since it was bound "
                                   f"(was {n} x {self.dtype} on {self.device}, is {t.numel()} x {t.dtype} on {t.device}); build a new list")
            self._descs[j].in_dev = cur
            self._bound[j] = (t, cur, n)
            moved = True
        return moved


class FastQuant:
    """The drop-in call (round-half-even, dequantised tensor out) with everything constant bound once: per call it costs
    one output allocation and one six-argument ctypes call (bfpq_fake_quantize).  This is what the module wrappers issue
    per tensor; native.quantize_nm stays the general entry point."""

    __slots__ = ("block_size", "mant_bits", "epsilon", "N", "M", "sparsify_first", "_plans", "_fn")

    def __init__(self, block_size, mant_bits, epsilon, N=0, M=0, sparsify_first=True):
        self.block_size, self.mant_bits, self.epsilon = int(block_size), int(mant_bits), float(epsilon)
        self.N, self.M = (int(N), int(M)) if 0 < N < M else (0, 0)
        self.sparsify_first = bool(sparsify_first)
        self._plans = {}
        self._fn = load_library().bfpq_fake_quantize

    def _plan(self, dtype, dev):
        key = (dtype, dev.index)
        p = self._plans.get(key)
        if p is None:
            win = exp_window_dev(dtype, dev) if self.block_size > 0 else None
            lut = nm4_lut_dev(self.N, dev) if self.M == 4 else (nm8_lut_dev(self.N, dev) if (self.M == 8 and USE_NM8_TABLE) else None)
            plan = _Plan(DTYPE_CODE[dtype], self.block_size, self.mant_bits, self.N, self.M, 1 if self.sparsify_first else 0,
                         self.epsilon, win.data_ptr() if win is not None else None, lut.data_ptr() if lut is not None else None)
            p = self._plans[key] = (plan, ctypes.addressof(plan), win, lut)        # (the tensors are kept alive with the plan)
        return p

    def __call__(self, t, out=None):
        if t.device.type != "cuda" or t.dtype not in DTYPE_CODE:
            require_device_tensor(t)
        if self.block_size == 0 and self.M == 0:
            return t
        src = t if t.is_contiguous() else t.contiguous()
        dst = torch.empty_like(src) if out is None else out
        n = src.numel()
        if n == 0:
            return dst
        dev = src.device
        cols = src.shape[-1] if src.dim() else 1
        plan = self._plan(src.dtype, dev)
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                rc = self._fn(plan[1], src.data_ptr(), dst.data_ptr(), n // cols, cols, torch.cuda.current_stream(dev).cuda_stream)
        else:
            stream = _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
            rc = self._fn(plan[1], src.data_ptr(), dst.data_ptr(), n // cols, cols, stream)
        if rc:
            check(rc, "bfpq_fake_quantize")
        return dst

    def prepare(self, tensors, apply_nm=None, outs=None):
        """PreparedList for these tensors: outputs allocated and descriptors built once, .run() re-issues the launches.
        For tensors whose storage stays put (the weights of a model quantized every forward)."""
        return PreparedList(self, tensors, apply_nm, outs)

    def _apply_nm(self, apply_nm, n):
        """the apply_nm field of n tensors' descriptors (default: N:M pruning applies to all), None for a tensor the plan leaves
        as it is (no quantization, and no N:M pruning for it)"""
        flags = [True] * n if apply_nm is None else [bool(f) for f in apply_nm]
        return flags if self.block_size else [f if f and self.M else None for f in flags]

    def many(self, tensors, apply_nm=None, outs=None):
        """the same for a LIST of tensors of one dtype on one device, in as few launches as possible
        (bfpq_fake_quantize_batched: up to 64 tensors per launch).  apply_nm: per tensor, whether this plan's N:M pruning
        applies to it (default: to all).  Returns the list of results (a tensor the plan leaves untouched comes back itself)."""
        if not tensors:
            return []
        # (keep: contiguous copies live until the call returns, stream-ordered after that)
        dev, dt, res, descs, keep = _bind(_TensorDesc, "apply_nm", tensors, self._apply_nm(apply_nm, len(tensors)), outs, "FastQuant.many", copy=True)
        k = len(keep)
        if k:
            plan = self._plan(dt, dev)
            with torch.cuda.device(dev):
                aux = aux_stream_array(dev, 1) if k > 1 else None
                rc = load_library().bfpq_fake_quantize_list(plan[1], ctypes.addressof(descs), k, torch.cuda.current_stream(dev).cuda_stream,
                                                            ctypes.addressof(aux) if aux is not None else None, 1 if aux is not None else 0)
            if rc:
                check(rc, "bfpq_fake_quantize_list")
        return res


class PreparedList(_BoundList):
    """A list of tensors bound to one FastQuant plan (see _BoundList): run() is ONE ctypes call (bfpq_fake_quantize_batched)
    whatever the number of tensors."""

    _Desc, _FIELD = _TensorDesc, "apply_nm"

    def __init__(self, fq, tensors, apply_nm=None, outs=None):
        tensors = list(tensors)
        self.fq = fq
        super().__init__(tensors, fq._apply_nm(apply_nm, len(tensors)), outs)
        self._plan = fq._plan(self.dtype, self.device) if self._k else None
        self._fn = load_library().bfpq_fake_quantize_list
        # (large tensors of the list get launches of their own, spread over the current stream and this one)
        self._aux = aux_stream_array(self.device, 1) if self._k > 1 else None

    def run(self):
        if self._k:
            self._rebind()
            dev = self.device
            aux, n_aux = (ctypes.addressof(self._aux), len(self._aux)) if self._aux is not None else (None, 0)
            if torch.cuda.current_device() != dev.index:
                with torch.cuda.device(dev):
                    rc = self._fn(self._plan[1], self._addr, self._k, torch.cuda.current_stream(dev).cuda_stream, aux, n_aux)
            else:
                rc = self._fn(self._plan[1], self._addr, self._k,
                              _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream, aux, n_aux)
            if rc:
                check(rc, "bfpq_fake_quantize_list")
        return self.outputs


class SelectWorkspace:
    """Device scratch of the unstructured path (include/bfpq.h: ws_dev): bfpq_select_state, the ticket and coarse histogram of
    the one-launch selection (16-bit dtypes; left zero by its last workgroup), the histogram buffers of the fp32 launch pairs
    (cleared by the apply launch of the same call), and the tie bookkeeping.  One per (device, stream): the launches of one
    call communicate through it."""

    def __init__(self, device):
        self.device = device
        nbytes = int(load_library().bfpq_select_ws_bytes())
        self.ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=device)
        self.dirty = False                                 # a select whose histograms no apply launch has cleared yet
        self.pinned = False                                # a captured graph refers to this workspace: never dropped
        self.hist_ext = None                               # multi-GPU: the local histogram that gets all-gathered

    def ext_hist(self):
        if self.hist_ext is None:
            self.hist_ext = torch.zeros(SELECT_HIST_COPIES * SELECT_HIST_ENTRIES, dtype=torch.int32, device=self.device)
        return self.hist_ext

    def read_state(self):
        """host copy of bfpq_select_state (synchronises; for tests / diagnostics only)"""
        import struct
        raw = self.ws[:SELECT_STATE_BYTES // 8].cpu().numpy().tobytes()
        prefix, mask, k_rem, tau, done, need, ties, k, tie_base, flags, cut_lo, cut_hi, cut_within, cut_total = struct.unpack_from("<IIqIIqqqqIIIII", raw, 0)
        return dict(prefix=prefix, prefix_mask=mask, k_rem=k_rem, tau=tau, done=done, need=need, ties=ties, k=k,
                    tie_base=tie_base, flags=flags, cut_lo=cut_lo, cut_hi=cut_hi, cut_within=cut_within, cut_total=cut_total)


def select_threshold(t, k, ws, numel_global=None, allgather=None):
    """radix-select the k-th smallest magnitude of t (device tensor) and leave threshold + tie bookkeeping in ws.
    Single device: bfpq_select -- ONE launch for a 16-bit dtype (the histogram launch's last workgroup resolves), two for
    fp32 (the high 15 bits of the key, then the low 16).
    Multi-GPU: t is this rank's slab, k / numel_global are global, and allgather(hist) -> (hist_all [R, entries], R, rank)
    gathers the per-rank histograms (the one exchange of the path; an empty slab still joins it)."""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    code = DTYPE_CODE[src.dtype]
    n = src.numel()
    ng = n if numel_global is None else int(numel_global)
    null = ctypes.c_void_p(0)
    with torch.cuda.device(src.device):
        st = _stream(src)
        if ws.dirty:                                       # the previous fp32 select was never applied (diagnostic use)
            check(L.bfpq_select_reset(_ptr(ws.ws), st), "bfpq_select_reset")
            ws.dirty = False
        if allgather is None:
            if ng != n:
                raise ValueError("select_threshold: numel_global without an allgather")
            check(L.bfpq_select(_ptr(src), n, code, int(k), _ptr(ws.ws), st), "bfpq_select")
            return                                         # (leaves the workspace ready for the next call by itself)
        for p in range(L.bfpq_select_passes(code)):
            hist = ws.ext_hist()                           # zero on entry: resolve clears it again after the gather
            check(L.bfpq_select_hist(_ptr(src) if n else null, n, code, p, int(k), ng, _ptr(ws.ws), _ptr(hist), st), "bfpq_select_hist")
            hist_all, R, rank = allgather(hist)
            check(L.bfpq_select_resolve(_ptr(src) if n else null, n, code, p, int(k), _ptr(hist_all), int(R), int(rank), _ptr(ws.ws),
                                        _ptr(hist), st), "bfpq_select_resolve")


def select_threshold_list(ts, ks, wss, numel_globals, allgather):
    """select_threshold for a LIST of row-sharded tensors of one dtype on one device with ONE exchange per radix pass for the whole
    list (instead of one per tensor): every tensor's local histogram is launched first (its own workspace wss[i]), the 8 copies of each
    are summed, allgather(block [n, ENTRIES]) -> (gathered [R, n, ENTRIES], R, rank) moves them all in one collective, and tensor i
    resolves from its column of the gathered block (bfpq_select_resolve_ex: copies = 1, rank stride = n * ENTRIES).  A tensor whose
    slab is empty keeps a zero row.  Same thresholds, tie bases and cuts as the per-tensor exchange (the sums are the same integers)."""
    n = len(ts)
    if n == 0:
        return
    L = load_library()
    srcs = [t.contiguous() for t in ts]
    for t in srcs:
        require_device_tensor(t)
        if t.dtype != srcs[0].dtype or t.device != srcs[0].device:
            raise ValueError("select_threshold_list: the tensors of one list share device and dtype")
    dev, code = srcs[0].device, DTYPE_CODE[srcs[0].dtype]
    null = ctypes.c_void_p(0)
    E = SELECT_HIST_ENTRIES
    with torch.cuda.device(dev):
        st = _stream(srcs[0])
        for ws in wss[:n]:
            if ws.dirty:
                check(L.bfpq_select_reset(_ptr(ws.ws), st), "bfpq_select_reset")
                ws.dirty = False
        for p in range(L.bfpq_select_passes(code)):
            hists = [ws.ext_hist() for ws in wss[:n]]          # zero on entry: the resolve launch clears them again
            for src, k, ng, ws, h in zip(srcs, ks, numel_globals, wss, hists):
                m = src.numel()
                check(L.bfpq_select_hist(_ptr(src) if m else null, m, code, p, int(k), int(ng), _ptr(ws.ws), _ptr(h), st), "bfpq_select_hist")
            block = torch.stack(hists).view(n, SELECT_HIST_COPIES, E).sum(dim=1, dtype=torch.int32)       # [n, E]: the copies folded
            gathered, R, rank = allgather(block)
            gathered = gathered.contiguous()
            base = gathered.data_ptr()
            for i, (src, k, ws, h) in enumerate(zip(srcs, ks, wss, hists)):
                m = src.numel()
                check(L.bfpq_select_resolve_ex(_ptr(src) if m else null, m, code, p, int(k), ctypes.c_void_p(base + 4 * i * E), int(R), int(rank),
                                               1, n * E, _ptr(ws.ws), _ptr(h), st), "bfpq_select_resolve_ex")
            del gathered


def quantize_threshold(t, ws, block_size, mant_bits, epsilon, want_deq=True, code_bits=0, want_exp=False,
                       stoch_seed=0, out=None):
    """S-first unstructured: prune with the threshold held in ws and HBFP-quantize, one pass
    (bfpq_quantize_threshold).  Returns (deq | None, codes | None, exps | None) like quantize_nm."""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    rows, cols = rows_cols(src)
    code = DTYPE_CODE[src.dtype]
    dev = src.device
    with torch.cuda.device(dev):
        st = _stream(src)
        fused = L.bfpq_is_fused(rows, cols, code, int(block_size), 0, 0)
        deq = (out if out is not None else torch.empty_like(src)) if want_deq else None
        codes = exps = None
        if code_bits:
            shape = (rows, (cols + 1) // 2) if code_bits == 4 else (rows, cols)
            codes = torch.empty(shape, dtype={4: torch.uint8, 8: torch.int8, 16: torch.int16}[code_bits], device=dev)
        if want_exp:
            exps = torch.empty((rows, (cols + block_size - 1) // block_size), dtype=torch.int8, device=dev)
        scratch = torch.empty_like(src) if (not fused and deq is None) else None
        check(L.bfpq_quantize_threshold(_ptr(src), _ptr(deq), _ptr(codes), _ptr(exps), rows, cols, code, int(block_size),
                                        int(mant_bits), float(epsilon), int(code_bits), int(stoch_seed),
                                        _ptr(exp_window_dev(src.dtype, dev)), _ptr(ws.ws), _ptr(scratch), st),
              "bfpq_quantize_threshold")
        ws.dirty = False
    return deq, codes, exps


def prune_quantize(t, k, ws, block_size, mant_bits, epsilon, out=None):
    """the whole s-first unstructured drop-in op on one device, out = Q(S_k(t)) (bfpq_prune_quantize): the selection launch +
    the fused prune + quantize launch behind one call.  Round-half-even."""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    rows, cols = rows_cols(src)
    dev = src.device
    with torch.cuda.device(dev):
        dst = out if out is not None else torch.empty_like(src)
        if ws.dirty:
            check(L.bfpq_select_reset(_ptr(ws.ws), _stream(src)), "bfpq_select_reset")
        check(L.bfpq_prune_quantize(_ptr(src), _ptr(dst), rows, cols, DTYPE_CODE[src.dtype], int(block_size), int(mant_bits), float(epsilon),
                                    int(k), _ptr(exp_window_dev(src.dtype, dev)), _ptr(ws.ws), _stream(src)), "bfpq_prune_quantize")
        ws.dirty = False
    return dst


class _PruneDesc(ctypes.Structure):
    """include/bfpq.h: bfpq_prune_desc"""
    _fields_ = [("in_dev", ctypes.c_void_p), ("out_dev", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("k", ctypes.c_int64)]


_aux_streams = {}


def aux_streams(device, n=1):
    """n persistent side streams of the device: the aux lanes of the list calls (bfpq_fake_quantize_list, bfpq_prune_quantize_list)"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    lst = _aux_streams.setdefault(idx, [])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(torch.device("cuda", idx)))
    return lst[:n]


def aux_stream(device):
    return aux_streams(device, 1)[0]


_aux_arrays = {}


def aux_stream_array(device, n):
    """the raw handles of aux_streams(device, n) as a C array of void*, made once (the streams live as long as the process)"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    arr = _aux_arrays.get(key)
    if arr is None:
        arr = _aux_arrays[key] = (ctypes.c_void_p * n)(*[s.cuda_stream for s in aux_streams(device, n)])
    return arr


def _deal_over_streams(device, items, lanes, fn):
    """[fn(i, item) for i, item in enumerate(items)] for calls that are independent of one another: item i is issued on stream
    i % S of the caller's stream + aux_streams(device, S - 1), S = min(lanes, len(items)).  The side streams fork from the
    caller's stream before the first item and are joined back after the last; a result allocated on a side stream (anything fn
    returns other than the item itself) is recorded as used by the caller's stream."""
    main = torch.cuda.current_stream(device)
    streams = [main] + aux_streams(device, min(lanes, len(items)) - 1)
    for s in streams[1:]:
        s.wait_stream(main)
    out = []
    for i, x in enumerate(items):
        s = streams[i % len(streams)]
        with torch.cuda.stream(s):
            y = fn(i, x)
        if s is not main and y is not x:
            y.record_stream(main)
        out.append(y)
    for s in streams[1:]:
        main.wait_stream(s)
    return out


class PruneQuantizeList(_BoundList):
    """A list of tensors of one dtype on one device bound to the s-first unstructured drop-in op (bfpq_prune_quantize_list; see
    _BoundList): the workspaces too are set up once; run() is ONE ctypes call that spreads the tensors over N_WS independent
    lanes (the current stream and side streams, a workspace each; a tensor's two launches stay on its lane), or replays a
    hipGraph of that call.  ks: elements to prune per tensor, int(numel * frac) as the reference computes it (bfp_ops.py:66)."""

    N_WS = 4                 # lanes: the current stream + 3 side streams, a workspace each (13B list: 1 lane 16.8 ms, 2: 14.2, 3: 12.7, 4: 12.5)
    GRAPH_FROM = 8           # lists of at least this many tensors replay a hipGraph of the pipeline (captured on the first run)
    CAPTURE_AUX = 1          # side streams when the list is captured into a hipGraph (its own or the caller's): two lanes, the shape the
                             # other list graphs have.  A four-lane graph replayed after a two-lane list graph segfaulted inside
                             # hipGraphLaunch (ROCm 7.2, which runs a graph's branches on a per-device set of streams); eager calls keep N_WS

    _Desc, _FIELD = _PruneDesc, "k"

    def __init__(self, tensors, ks, block_size, mant_bits, epsilon, outs=None):
        self.block_size, self.mant_bits, self.epsilon = int(block_size), int(mant_bits), float(epsilon)
        super().__init__(list(tensors), [int(k) for k in ks], outs)
        if self._k:
            with torch.cuda.device(self.device):
                self._ws = [SelectWorkspace(self.device) for _ in range(self.N_WS)]
                self._ws_ptrs = (ctypes.c_void_p * self.N_WS)(*[w.ws.data_ptr() for w in self._ws])
                self._win = exp_window_dev(self.dtype, self.device)
                self._aux = aux_stream_array(self.device, self.N_WS - 1)
        self._fn = load_library().bfpq_prune_quantize_list
        self._graph = None

    def _issue(self, pipelined):
        dev = self.device
        with torch.cuda.device(dev):
            n_aux = len(self._aux) if pipelined else 0
            if n_aux and torch.cuda.is_current_stream_capturing():
                n_aux = min(n_aux, self.CAPTURE_AUX)
            rc = self._fn(self._addr, self._k, DTYPE_CODE[self.dtype], self.block_size, self.mant_bits, self.epsilon,
                          self._win.data_ptr(), ctypes.addressof(self._ws_ptrs), self.N_WS, torch.cuda.current_stream(dev).cuda_stream,
                          ctypes.addressof(self._aux) if n_aux else None, n_aux)
        if rc:
            check(rc, "bfpq_prune_quantize_list")

    def run(self, pipelined=True, graph=None):
        """graph: replay a hipGraph of the whole pipeline (captured on the first such run; every pointer in it is bound --
        a tensor whose storage moved drops the graph).  Default: for lists of GRAPH_FROM tensors or more, outside any
        capture already in progress.  The ~6 host calls per tensor (2 launches, 4 event operations) otherwise cost more
        host time than a small tensor's launches take on the device.  The capture (a device synchronise, an eager warm-up run)
        pays only for a list that is kept and re-run: a list made for one call runs with graph=False."""
        if self._k:
            if self._rebind():
                self._graph = None
            if graph is None:
                graph = self._k >= self.GRAPH_FROM
            if graph and pipelined and not torch.cuda.is_current_stream_capturing():
                if self._graph is None:
                    self._issue(True)                                     # (warm-up outside the capture)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.device(self.device), torch.cuda.graph(g):
                        self._issue(True)
                    self._graph = g
                with torch.cuda.device(self.device):
                    self._graph.replay()
            else:
                self._issue(pipelined)
        return self.outputs


def threshold_apply(t, ws, out=None):
    """zero everything below the threshold in ws plus the first `need` ties (flat order, lower ranks first)"""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    code = DTYPE_CODE[src.dtype]
    with torch.cuda.device(src.device):
        dst = out if out is not None else torch.empty_like(src)
        check(L.bfpq_threshold_apply(_ptr(src), _ptr(dst), src.numel(), code, _ptr(ws.ws), _stream(src)), "bfpq_threshold_apply")
        ws.dirty = False
    return dst


def int_channel_view(shape, weight):
    """(outer, C, inner): the per-channel view int_ops.Quantizer.find_params takes (reference int_ops.py:38-50)"""
    shape = tuple(shape)
    n = 1
    for d in shape:
        n *= d
    if weight:
        if len(shape) < 1:
            raise ValueError("'int' format needs at least a 1-D weight")
        return 1, shape[0], n // max(shape[0], 1)
    if len(shape) == 4:
        return shape[0], shape[1], shape[2] * shape[3]
    if len(shape) in (2, 3):
        return n // max(shape[-1], 1), shape[-1], 1
    raise ValueError("'int' format handles 2-D, 3-D and 4-D activations (reference int_ops.py:43-50)")


def int_quantize(t, bits, weight):
    """per-channel symmetric integer fake-quantization (bfpq_int_quantize); fp32 result like the reference"""
    require_device_tensor(t)
    L = load_library()
    src = t.contiguous()
    outer, C, inner = int_channel_view(src.shape, weight)
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    if src.numel() == 0:
        return out
    with torch.cuda.device(src.device):
        ws = torch.empty(2 * C, dtype=torch.int32, device=src.device) if outer != 1 else None
        check(L.bfpq_int_quantize(_ptr(src), _ptr(out), outer, C, inner, DTYPE_CODE[src.dtype], int(bits), _ptr(ws), _stream(src)),
              "bfpq_int_quantize")
    return out


def dequantize(codes, exps, cols, dtype, block_size, mant_bits, code_bits, out=None):
    """packed codes + exponents -> [rows, cols] tensor of `dtype` (bfpq_dequantize)"""
    if exps.device.type != "cuda" or codes.device != exps.device:
        raise NativeUnavailable("packed codes / exponents must live on one ROCm device")
    if dtype not in DTYPE_CODE:
        raise TypeError(f"unsupported dtype {dtype}")
    L = load_library()
    rows = exps.shape[0]
    dst = out if out is not None else torch.empty((rows, cols), dtype=dtype, device=exps.device)
    if rows * cols == 0:
        return dst
    with torch.cuda.device(exps.device):
        c, e = codes.contiguous(), exps.contiguous()
        check(L.bfpq_dequantize(_ptr(c), _ptr(e), _ptr(dst), rows, int(cols), DTYPE_CODE[dtype], int(block_size), int(mant_bits),
                                int(code_bits), ctypes.c_void_p(torch.cuda.current_stream(exps.device).cuda_stream)), "bfpq_dequantize")
    return dst


def stoc_widen_f16(t):
    """fp32 image of an fp16 'stoc' result (bfpq_stoc_widen_f16): +-inf -> +-65536, the reference's value"""
    require_device_tensor(t)
    assert t.dtype == torch.float16
    src = t.contiguous()
    if src.data_ptr() % 8:
        src = src.clone()
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(load_library().bfpq_stoc_widen_f16(_ptr(src), _ptr(out), src.numel(), _stream(src)), "bfpq_stoc_widen_f16")
    return out


def is_fused(t, block_size, N=0, M=0):
    """would quantize_nm take the single-pass kernel for this (contiguous) tensor?"""
    rows, cols = rows_cols(t)
    return bool(load_library().bfpq_is_fused(rows, cols, DTYPE_CODE[t.dtype], int(block_size), int(N), int(M))) and t.data_ptr() % 16 == 0


def compact24(codes):
    """2:4 compaction of a 4-bit code tensor (uint8, numel % 4 == 0): (vals uint8 [numel/2], idx uint8 [numel/4]).
    Raises ValueError if some group of 4 codes has more than 2 non-zeros (synchronises to read the flag)."""
    require_device_tensor_any(codes)
    c = codes.contiguous().view(-1)
    n = c.numel()
    if n % 4:
        raise ValueError("compact24 needs a multiple of 8 elements (4 code bytes)")
    with torch.cuda.device(c.device):
        vals = torch.empty(n // 2, dtype=torch.uint8, device=c.device)
        idx = torch.empty(n // 4, dtype=torch.uint8, device=c.device)
        status = torch.zeros(1, dtype=torch.int32, device=c.device)
        check(load_library().bfpq_compact24(_ptr(c), _ptr(vals), _ptr(idx), n, _ptr(status), _stream(c)), "bfpq_compact24")
    if int(status.item()):
        raise ValueError("compact24: a group of 4 codes has more than 2 non-zeros (the tensor is not 2:4 sparse)")
    return vals, idx


def expand24(vals, idx):
    """inverse of compact24: the 4-bit code bytes (uint8 [4 * idx.numel()])"""
    require_device_tensor_any(vals)
    n = idx.numel() * 4
    with torch.cuda.device(vals.device):
        codes = torch.empty(n, dtype=torch.uint8, device=vals.device)
        check(load_library().bfpq_expand24(_ptr(vals.contiguous()), _ptr(idx.contiguous()), _ptr(codes), n, _stream(vals)), "bfpq_expand24")
    return codes


def require_device_tensor_any(t):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise NativeUnavailable("the BFP engine runs on a ROCm device only (no CPU fallback)")


def mfma_tiles(wcodes, wexps):
    """one-time repack of a packed HBFP4 weight (codes [N, K/2] uint8, exps [N, K/64] int8, block 64) into the layout
    bfpq_hbfp_linear_decode_tiled reads: a pure permutation, done with torch views"""
    N, K = wexps.shape[0], wexps.shape[1] * 64
    assert N % 16 == 0 and K % 128 == 0
    t = wcodes.view(N // 16, 16, K // 128, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous().view(N // 16, K // 128, 64, 16)
    e = wexps.view(N // 16, 16, K // 128, 2).permute(0, 2, 1, 3).contiguous()
    return t, e


def _linear_operands(x, T, N, K, x_mant_bits, epsilon, act, xq, bias, out_dtype, block_size=64):
    """what the linears on int8 activation codes share, on x's device: the activation operand (xq as given, else act_codes of x pruned by
    `act`), the [T, N] output and the bias in out_dtype (None stays None)"""
    if xq is not None:
        xc, xe = xq[0].contiguous(), xq[1].contiguous()
    else:
        xc, xe = act_codes(x.reshape(T, K), x_mant_bits, epsilon, act, block_size=block_size)
    out = torch.empty((T, N), dtype=out_dtype, device=x.device)
    if bias is not None:
        bias = bias.to(out_dtype).contiguous()
    return xc, xe, out, bias


def hbfp_linear_decode_tiled(x, wtiles, wexpt, N, w_mant_bits, x_mant_bits=7, epsilon=1e-8, out_dtype=None, xq=None):
    """hbfp_linear_decode on the MFMA-tiled weight (see mfma_tiles).  xq: the activation operand made beforehand (act_codes: int8
    codes [T, K], int8 exponents [T, K/64]), e.g. pruned over more tokens than this call takes; x then only gives shape and dtype."""
    require_device_tensor(x)
    L = load_library()
    K = x.shape[-1]
    T = x.numel() // K
    if T < 1 or T > 64 or not L.bfpq_hbfp_linear_tiled_ok(N, K):
        raise ValueError(f"hbfp_linear_decode_tiled needs 1..64 tokens, N % 16 == 0, K % 128 == 0 and K >= 256 (got T={T}, N={N}, K={K})")
    dev = x.device
    out_dtype = out_dtype or x.dtype
    with torch.cuda.device(dev):
        # (token columns past T re-read row T-1: no padding rows)
        xc16, xe16, out, _ = _linear_operands(x, T, N, K, x_mant_bits, epsilon, None, xq, None, out_dtype)
        check(L.bfpq_hbfp_linear_decode_tiled(_ptr(wtiles), _ptr(wexpt), _ptr(xc16), _ptr(xe16), _ptr(out), T, N, K,
                                              DTYPE_CODE[out_dtype], int(w_mant_bits), int(x_mant_bits), _stream(x)),
              "bfpq_hbfp_linear_decode_tiled")
    return out.view(tuple(x.shape[:-1]) + (N,))


def hbfp_linear_decode(x, wcodes, wexps, w_mant_bits, x_mant_bits=7, epsilon=1e-8, out_dtype=None, xq=None):
    """out = x @ W^T for <= 16 tokens, W given as packed HBFP (4-bit codes [N, K/2], int8 exponents [N, K/64], block 64),
    x quantized on the fly to HBFP(x_mant_bits + 1) block 64; integer block dot products on the int8 matrix cores.
    xq: the activation operand made beforehand, as in hbfp_linear_decode_tiled."""
    require_device_tensor(x)
    L = load_library()
    K = x.shape[-1]
    T = x.numel() // K
    N = wexps.shape[0]
    slices = L.bfpq_hbfp_linear_slices(N, K)
    if T < 1 or T > 16 or slices < 0:
        raise ValueError(f"hbfp_linear_decode needs 1..16 tokens, N % 16 == 0 and K % 256 == 0 (got T={T}, N={N}, K={K})")
    dev = x.device
    out_dtype = out_dtype or x.dtype
    with torch.cuda.device(dev):
        # the activation quantizer writes straight into the 16-row operand buffers (rows >= T stay uninitialised:
        # each token's results live in its own lanes and rows >= T are never read back)
        xc16 = torch.empty((16, K), dtype=torch.int8, device=dev)
        xe16 = torch.empty((16, K // 64), dtype=torch.int8, device=dev)
        if xq is not None:
            xc16[:T].copy_(xq[0])
            xe16[:T].copy_(xq[1])
        else:
            quantize_nm(x.reshape(T, K), 64, x_mant_bits, epsilon, want_deq=False, code_bits=8, want_exp=True,
                        codes_out=xc16[:T], exps_out=xe16[:T])
        slabs = torch.empty((slices, 16, N), dtype=torch.float32, device=dev)
        out = torch.empty((T, N), dtype=out_dtype, device=dev)
        check(L.bfpq_hbfp_linear_decode(_ptr(wcodes.contiguous()), _ptr(wexps.contiguous()), _ptr(xc16), _ptr(xe16), _ptr(out),
                                        _ptr(slabs), T, N, K, DTYPE_CODE[out_dtype], int(w_mant_bits), int(x_mant_bits), _stream(x)),
              "bfpq_hbfp_linear_decode")
    return out.view(tuple(x.shape[:-1]) + (N,))


def mx8_from_hbfp(codes, exps, cols, mant_bits, code_bits):
    """packed HBFP (codes + int8 exponents, block 64, mantissas <= 4 bits) -> the operand image of the block-scaled matrix
    instruction: e4m3 bytes [rows, cols] + E8M0 scale bytes [rows, cols/64] (bfpq_mx8_from_hbfp)"""
    require_device_tensor_any(codes)
    L = load_library()
    rows = exps.numel() // (cols // 64)
    dev = codes.device
    with torch.cuda.device(dev):
        o8 = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        osc = torch.empty((rows, cols // 64), dtype=torch.uint8, device=dev)
        check(L.bfpq_mx8_from_hbfp(_ptr(codes.contiguous()), _ptr(exps.contiguous()), _ptr(o8), _ptr(osc), rows, cols, int(code_bits), int(mant_bits),
                                   torch.cuda.current_stream(dev).cuda_stream), "bfpq_mx8_from_hbfp")
    return o8, osc


class ActSparsity(collections.namedtuple("ActSparsity", "mode N M frac first")):
    """How an activation operand is pruned before (first = 's') or after (first = 'q') its HBFP quantization (as in the reference, any
    `first` other than 's' quantizes first): the reference's
    in_sparsity with identifier 'in' (bfp_ops.py:129-149).  mode 'structured' (N of every M along the rows) or 'unstructured'
    (the int(numel * frac) smallest magnitudes of the whole tensor).  Hashable: part of the activation-image memo key.
    None stands for dense activations."""

    @classmethod
    def from_bfp_args(cls, a):
        """the spec of a bfp_args dict (bfp_ops.unpack_bfp_args), or None when its activations are dense"""
        if a.get('in_sparsity') != True:  # noqa: E712  (the reference compares with ==)
            return None
        mode = a.get('sparsity_mode')
        if mode == 'structured':
            N, M = int(a['N']), int(a['M'])
            if not 0 < N <= M:
                raise ValueError(f"in_sparsity with N:M = {N}:{M}")
            return None if N == M else cls('structured', N, M, 0.0, 's' if a.get('first') == 's' else 'q')
        if mode == 'unstructured':
            frac = float(a['sparsity_frac'])
            if not frac > 0:
                raise ValueError(f"in_sparsity with sparsity_frac = {frac}")
            return cls('unstructured', 0, 0, frac, 's' if a.get('first') == 's' else 'q')
        raise ValueError(f'Unknown sparsity mode: {mode} given as argument')

    def as_dict(self):
        return dict(mode=self.mode, N=int(self.N), M=int(self.M), frac=float(self.frac), first=self.first)

    @classmethod
    def from_dict(cls, d):
        return None if d is None else cls(d['mode'], int(d['N']), int(d['M']), float(d['frac']), d['first'])


def _act_workspace(device):
    from .bfp.bfp_ops import _workspace            # (the per-stream select workspaces, capture-safe; a late import: bfp_ops imports this module)
    return _workspace(device)


def prune_count(t, frac):
    """the number of elements unstructured pruning zeroes in t: int(numel * frac), as the reference computes it (bfp_ops.py:66)"""
    k = int(t.numel() * frac)
    if k > t.numel():
        raise RuntimeError("selected index k out of range")      # what torch.topk raises in the reference
    return k


def act_codes(x, mant_bits, epsilon, act, codes_out=None, exps_out=None, block_size=64):
    """int8 codes [T, K] + int8 exponents [T, K/block_size] of the activation x [T, K], HBFP(mant_bits + 1) with blocks of block_size
    (64 for the decode kernels; 16 or 32 for hbfp_linear_i8 at those blocks), pruned by `act` (ActSparsity or None).  Unstructured
    pruning picks ONE threshold over all of x."""
    T, K = x.shape
    dev = x.device
    if act is None or act.mode == 'structured':
        N, M = (act.N, act.M) if act is not None else (0, 0)
        _, c, e = quantize_nm(x, block_size, mant_bits, epsilon, N=N, M=M, sparsify_first=(act is None or act.first == 's'), want_deq=False,
                              code_bits=8, want_exp=True, codes_out=codes_out, exps_out=exps_out)
        return c, e
    k = prune_count(x, act.frac)
    ws = _act_workspace(dev)
    if act.first == 's':
        select_threshold(x, k, ws)
        _, c, e = quantize_threshold(x, ws, block_size, mant_bits, epsilon, want_deq=False, code_bits=8, want_exp=True)
    else:
        # S(Q(x)): quantize (the tensor and its codes at once), select over the quantized tensor, prune it; a pruned element's code is
        # zeroed -- the exponents stay those of Q(x), so nothing depends on re-quantizing the pruned tensor
        q, c, e = quantize_nm(x, block_size, mant_bits, epsilon, code_bits=8, want_exp=True)
        select_threshold(q, k, ws)
        sq = threshold_apply(q, ws).view(T, K)
        c = torch.where(sq == 0, torch.zeros((), dtype=c.dtype, device=dev), c)
    if codes_out is not None:
        codes_out.copy_(c)
        exps_out.copy_(e)
        return codes_out, exps_out
    return c, e


def stoc_codes(t, block_size, mant_bits, epsilon, seed, act=None):
    """int8 codes [rows, cols] + int8 exponents [rows, cols/block_size] of the 2-D tensor t, HBFP(mant_bits + 1) rounded
    stochastically with `seed`, pruned by `act` (ActSparsity or None) -- the operand that bfp_ops.float_to_bfp_blocked(t, ..., 'stoc')
    makes with that seed, as codes.  Each form is the launch that route makes, with codes + exponents as its outputs: the quantizer picks
    its arithmetic tier per wave and its dither per element from the seed and the element's index alone, never from what it writes, so
    code * 2^(exp - mant_bits) is that route's value bit for bit.  The one exception is a block whose 2^e overflows the dtype: there the
    reference's clamp bound is infinite and a value may be +-2^m codes; exp_top_flag finds such blocks.  Dense and N:M: one launch
    (bfpq_quantize_nm).  Unstructured, prune first: the selection launch + the threshold quantizer.  Quantize first: quantize once to
    the tensor and its codes with one dither, select over the quantized tensor, then zero the pruned codes (the exponents stay those of
    Q(t), as in act_codes)."""
    if act is None or act.mode == 'structured':
        N, M = (act.N, act.M) if act is not None else (0, 0)
        # (N:M off the single-pass kernel is a pruning launch + a quantize launch that meet in the dequantised tensor)
        _, c, e = quantize_nm(t, block_size, mant_bits, epsilon, N=N, M=M, sparsify_first=(act is None or act.first == 's'),
                              want_deq=M > 0 and not is_fused(t, block_size, N, M), code_bits=8, want_exp=True, stoch_seed=seed)
        return c, e
    k = prune_count(t, act.frac)
    ws = _act_workspace(t.device)
    if act.first == 's':
        select_threshold(t, k, ws)
        _, c, e = quantize_threshold(t, ws, block_size, mant_bits, epsilon, want_deq=not is_fused(t, block_size), code_bits=8, want_exp=True,
                                     stoch_seed=seed)
        return c, e
    q, c, e = quantize_nm(t, block_size, mant_bits, epsilon, code_bits=8, want_exp=True, stoch_seed=seed)
    select_threshold(q, k, ws)
    sq = threshold_apply(q, ws).view(c.shape)
    return torch.where(sq == 0, torch.zeros((), dtype=c.dtype, device=c.device), c), e


def exp_top_flag(exp_a, exp_b):
    """int32 device tensor [1]: 1 when an exponent byte of exp_a or exp_b is 127 (bfpq_exp_top_flag), else 0"""
    dev = exp_a.device
    with torch.cuda.device(dev):
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        a, b = exp_a.contiguous(), exp_b.contiguous()
        check(load_library().bfpq_exp_top_flag(_ptr(a), a.numel(), _ptr(b), b.numel(), _ptr(flag), _stream(a)), "bfpq_exp_top_flag")
    return flag


def quantize_mx8(x, mant_bits, epsilon=1e-8, act=None):
    """a 2-D tensor [T, K] -> its HBFP(mant_bits + 1) block-64 image for the block-scaled matrix unit: e4m3 bytes [T, K] + E8M0
    scales [T, K/64], in one pass (bfpq_quantize_mx8); the two-step route (int8 codes + mx8_from_hbfp) only for shapes it refuses.
    act (ActSparsity): the image of the pruned activation -- N:M in one pass (bfpq_quantize_mx8_nm), unstructured prune-first as
    selection + the threshold-mode image (bfpq_quantize_threshold_mx8); what those refuse (and quantize-first unstructured) goes
    through the codes (act_codes) + mx8_from_hbfp."""
    require_device_tensor(x)
    L = load_library()
    T, K = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        if K % 64 == 0 and (act is None or act.mode == 'structured' or act.first == 's'):
            x = x.contiguous()
            x8 = torch.empty((T, K), dtype=torch.uint8, device=dev)
            xs = torch.empty((T, K // 64), dtype=torch.uint8, device=dev)
            win = _ptr(exp_window_dev(x.dtype, dev))
            if act is None:
                rc = L.bfpq_quantize_mx8(_ptr(x), _ptr(x8), _ptr(xs), T, K, DTYPE_CODE[x.dtype], int(mant_bits), float(epsilon), win, _stream(x))
            elif act.mode == 'structured':
                lut = nm4_lut_dev(act.N, dev) if act.M == 4 else (nm8_lut_dev(act.N, dev) if (act.M == 8 and USE_NM8_TABLE) else None)
                rc = L.bfpq_quantize_mx8_nm(_ptr(x), _ptr(x8), _ptr(xs), T, K, DTYPE_CODE[x.dtype], int(mant_bits), float(epsilon),
                                            int(act.N), int(act.M), 1 if act.first == 's' else 0, win, _ptr(lut), _stream(x))
            else:
                k = prune_count(x, act.frac)
                ws = _act_workspace(dev)
                select_threshold(x, k, ws)
                rc = L.bfpq_quantize_threshold_mx8(_ptr(x), _ptr(x8), _ptr(xs), T, K, DTYPE_CODE[x.dtype], int(mant_bits), float(epsilon),
                                                   win, _ptr(ws.ws), _stream(x))
                if rc == BFPQ_E_UNSUPPORTED:               # (the selection stands: the codes route below applies the same threshold)
                    _, xc, xe = quantize_threshold(x, ws, 64, mant_bits, epsilon, want_deq=False, code_bits=8, want_exp=True)
                    return mx8_from_hbfp(xc, xe, K, mant_bits, 8)
            if rc == 0:
                return x8, xs
            if rc != BFPQ_E_UNSUPPORTED:
                check(rc, "bfpq_quantize_mx8")
        xc = torch.empty((T, K), dtype=torch.int8, device=dev)
        xe = torch.empty((T, K // 64), dtype=torch.int8, device=dev)
        act_codes(x, mant_bits, epsilon, act, codes_out=xc, exps_out=xe)
        return mx8_from_hbfp(xc, xe, K, mant_bits, 8)


_last_image = {}          # device -> (key, the tensor itself, image): q/k/v (and gate/up) of a block are called on the same tensor
SPLIT_K = True            # False: never split K (A/B measurements)
SHARE_ACT_IMAGE = True    # False: every call quantizes its activation (single-layer benchmarks that re-use one input tensor)


def tensor_version(t):
    """in-place version counter of a tensor, or None where it has none (tensors created under torch.inference_mode())"""
    try:
        return t._version
    except RuntimeError:
        return None


def _shared_image(x2, mant_bits, epsilon, act=None):
    """quantize_mx8 with a one-entry memo per device: the projections that share an input (q/k/v, gate/up) quantize it once.
    The entry holds the tensor it was made from, so that tensor's memory cannot be handed to another tensor while the entry
    lives; the key includes the in-place version counter.  The memo is bypassed -- the image is made afresh and nothing is
    stored -- whenever the key cannot vouch for the bytes: while a hipGraph is being captured (the launch is recorded, not
    run: an entry made then would hold an image that was never computed), for inference-mode tensors (no version counter),
    and with SHARE_ACT_IMAGE off.  Writes the version counter does not see (`.data` assignments, raw-pointer writes such as
    this library's own `out=` arguments) are outside what the key can detect: callers that mutate an activation that way
    between two projections must call forget_shared_images() (PackedBFP.linear and the cached BFPLinear never do)."""
    if not SHARE_ACT_IMAGE or torch.cuda.is_current_stream_capturing():
        return quantize_mx8(x2, mant_bits, epsilon, act)
    ver = None if x2.is_inference() else tensor_version(x2)
    if ver is None:
        return quantize_mx8(x2, mant_bits, epsilon, act)
    key = (x2.data_ptr(), ver, tuple(x2.shape), tuple(x2.stride()), x2.dtype, int(mant_bits), float(epsilon),
           torch.cuda.current_stream(x2.device).cuda_stream, act)          # (act: the activation's pruning is part of its image)
    hit = _last_image.get(x2.device)
    if hit is not None and hit[0] == key:
        return hit[2]
    img = quantize_mx8(x2, mant_bits, epsilon, act)
    _last_image[x2.device] = (key, x2, img)
    return img


def forget_shared_images():
    """drop the per-device activation-image memo (and the activation each entry keeps alive)"""
    _last_image.clear()


def hbfp_linear_mx8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size=64):
    return block_size == 64 and 1 <= w_mant_bits <= 4 and 1 <= x_mant_bits <= 4 and bool(load_library().bfpq_hbfp_linear_mx8_ok(T, N, K))


def _mx_linear(entry, x, w_ops, N, tail, x_mant_bits, epsilon, bias, out_dtype, act, x_image):
    """the launch both forms of the block-scaled prefill GEMM share: C entries `entry`, `entry`_parts and `entry`_splitk, the weight
    operand `w_ops` (two tensors: image + scales, or codes + exponents), `tail` = the entry's arguments between out_dtype and stream"""
    require_device_tensor(x)
    L = load_library()
    K = x.shape[-1]
    T = x.numel() // K
    if not hbfp_linear_mx8_ok(T, N, K, 1, x_mant_bits):
        raise ValueError(f"{entry[5:]} needs K % 256 == 0 and activation mantissas of <= 4 bits (got T={T}, N={N}, K={K}, x_mant_bits={x_mant_bits})")
    dev = x.device
    out_dtype = out_dtype or x.dtype
    with torch.cuda.device(dev):
        x8, xs = x_image if x_image is not None else _shared_image(x.reshape(T, K), x_mant_bits, epsilon, act)
        out = torch.empty((T, N), dtype=out_dtype, device=dev)
        if bias is not None:
            bias = bias.to(out_dtype).contiguous()
        ops = (_ptr(x8), _ptr(xs), _ptr(w_ops[0]), _ptr(w_ops[1]), _ptr(bias) if bias is not None else None, _ptr(out))
        tail = (DTYPE_CODE[out_dtype],) + tuple(tail) + (_stream(x),)
        parts = getattr(L, entry + "_parts")(T, N, K) if SPLIT_K else 1
        if parts > 1:                                                  # few tokens: K split over several workgroups per tile, fp32 slabs
            slabs = torch.empty((parts, T, N), dtype=torch.float32, device=dev)
            check(getattr(L, entry + "_splitk")(*ops, _ptr(slabs), parts, T, N, K, *tail), entry + "_splitk")
        else:
            check(getattr(L, entry)(*ops, T, N, K, *tail), entry)
    return out.view(tuple(x.shape[:-1]) + (N,))


def hbfp_linear_mx8(x, w8, wscale, x_mant_bits, epsilon=1e-8, bias=None, out_dtype=None, act=None, x_image=None):
    """out = Q(x) @ W^T (+ bias) for any number of tokens on the block-scaled matrix instruction: x is quantized to
    HBFP(x_mant_bits + 1) block 64 (int8 codes + exponents), turned into its e4m3 / E8M0 image and multiplied with the
    weight's image (mx8_from_hbfp of the packed weight, made once).  act (ActSparsity or None): the activation is pruned first
    (quantize_mx8).  x_image: the activation's image made beforehand (e4m3 [T, K], E8M0 [T, K/64]); x then only gives shape."""
    return _mx_linear("bfpq_hbfp_linear_mx8", x, (w8, wscale), w8.shape[0], (), x_mant_bits, epsilon, bias, out_dtype, act, x_image)


def hbfp_linear_mx4w_ok(T, N, K, w_mant_bits, x_mant_bits, block_size=64):
    return block_size == 64 and 1 <= w_mant_bits <= 3 and 1 <= x_mant_bits <= 4 and bool(load_library().bfpq_hbfp_linear_mx4w_ok(T, N, K))


def hbfp_linear_mx4w(x, codes4, exps, w_mant_bits, x_mant_bits, epsilon=1e-8, bias=None, out_dtype=None, act=None, x_image=None):
    """hbfp_linear_mx8 with the packed weight itself as the weight operand: codes4 [N, K/2] (two's-complement nibbles, low nibble
    first) and exps [N, K/64] (int8) as PackedBFP holds them, w_mant_bits 1..3.  The kernel makes e4m3 bytes and E8M0 scales of them
    on the way to the matrix instruction, so no weight image is made, cached or kept; the result has the bits of hbfp_linear_mx8 on
    mx8_from_hbfp(codes4, exps).  The activation operand (act, x_image, the shared-image memo) is handled as there."""
    require_device_tensor_any(codes4)
    K = x.shape[-1]
    N = exps.shape[0]
    if not 1 <= int(w_mant_bits) <= 3:
        raise ValueError(f"hbfp_linear_mx4w takes 4-bit codes: w_mant_bits 1..3 (got {w_mant_bits})")
    if codes4.dtype != torch.uint8 or codes4.numel() * 2 != N * K or exps.dtype != torch.int8 or exps.numel() * 64 != N * K:
        raise ValueError(f"hbfp_linear_mx4w takes uint8 codes [N, K/2] and int8 exponents [N, K/64] (got {tuple(codes4.shape)} {codes4.dtype}, "
                         f"{tuple(exps.shape)} {exps.dtype}, K={K})")
    return _mx_linear("bfpq_hbfp_linear_mx4w", x, (codes4.contiguous(), exps.contiguous()), N, (int(w_mant_bits),), x_mant_bits, epsilon, bias,
                      out_dtype, act, x_image)


# ---- HBFP5-HBFP8 on the int8 matrix unit (bfpq_i8gemm.hip) ---------------------------------------
DECODE8_TOKENS = 16       # up to this many tokens the decode-shaped kernel runs; more take the LDS-tiled kernel where K % 256 == 0


I8_BLOCKS = (16, 32)      # the blocks besides 64 that hbfp_linear_i8 runs (one v_mfma_i32_16x16x32_i8 per block)


def hbfp_linear_i8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size=64):
    """hbfp_linear_i8 takes this problem: block 64, 32 or 16, mantissas of 1..7 bits on both sides, N % 16 == 0, K % 64 == 0 (the tiled
    kernel needs K % 256 == 0; other K go to the decode-shaped kernel at any token count)"""
    return (block_size in (64,) + I8_BLOCKS and 1 <= w_mant_bits <= 7 and 1 <= x_mant_bits <= 7 and T >= 1 and N >= 16 and N % 16 == 0
            and K >= 64 and K % 64 == 0 and load_library().bfpq_hbfp_linear_decode8_ws(T, N, K) >= 0)


def codes4_to_i8(codes4, n_codes):
    """4-bit packed codes (two's-complement nibbles, low first) -> int8 codes [n_codes] (bfpq_codes4_to_i8)"""
    require_device_tensor_any(codes4)
    L = load_library()
    dev = codes4.device
    with torch.cuda.device(dev):
        out = torch.empty(n_codes, dtype=torch.int8, device=dev)
        check(L.bfpq_codes4_to_i8(_ptr(codes4.contiguous()), _ptr(out), int(n_codes), torch.cuda.current_stream(dev).cuda_stream), "bfpq_codes4_to_i8")
    return out


def hbfp_linear_i8(x, wcodes8, wexps, w_mant_bits, x_mant_bits, epsilon=1e-8, bias=None, out_dtype=None, act=None, xq=None, block_size=64):
    """out = Q(x) @ W^T (+ bias) for any number of tokens with W packed as int8 codes [N, K] + int8 exponents [N, K/block_size]
    (w_mant_bits 1..7) and x quantized to HBFP(x_mant_bits + 1) with the same blocks (x_mant_bits 1..7, round-half-even), pruned by
    `act` (ActSparsity or None; unstructured: one threshold over all tokens of the call).  block_size 64, 32 or 16.  Block dot products
    are exact integer sums on the int8 matrix unit, fp32 across blocks in block order.  xq: the activation operand made beforehand
    (act_codes with the same block_size); x then only gives shape and dtype."""
    require_device_tensor(x)
    L = load_library()
    K = x.shape[-1]
    T = x.numel() // K
    N = wexps.shape[0]
    if not hbfp_linear_i8_ok(T, N, K, w_mant_bits, x_mant_bits, block_size):
        raise ValueError(f"hbfp_linear_i8 needs block 16, 32 or 64, N % 16 == 0, K % 64 == 0 and mantissas of 1..7 bits "
                         f"(got T={T}, N={N}, K={K}, w_mant_bits={w_mant_bits}, x_mant_bits={x_mant_bits}, block_size={block_size})")
    if wcodes8.dtype != torch.int8 or wcodes8.numel() != N * K:
        raise ValueError("hbfp_linear_i8 takes int8 weight codes [N, K] (4-bit codes: codes4_to_i8 first)")
    nb = K // block_size
    if wexps.numel() != N * nb or (xq is not None and (xq[0].numel() != T * K or xq[1].numel() != T * nb)):
        raise ValueError(f"hbfp_linear_i8 at block {block_size} takes exponents [N, K/{block_size}] = [{N}, {nb}] and an activation operand "
                         f"[T, K] + [T, K/{block_size}] (got {tuple(wexps.shape)}"
                         + ("" if xq is None else f", {tuple(xq[0].shape)} + {tuple(xq[1].shape)}") + ")")
    dev = x.device
    out_dtype = out_dtype or x.dtype
    with torch.cuda.device(dev):
        xc, xe, out, bias = _linear_operands(x, T, N, K, x_mant_bits, epsilon, act, xq, bias, out_dtype, block_size)
        wc, we = wcodes8.contiguous(), wexps.contiguous()
        ops = (_ptr(xc), _ptr(xe), _ptr(wc), _ptr(we), _ptr(bias), _ptr(out))
        # the C entry family of the block: block 64's take no block argument, the `b` entries take 16 or 32
        blk, sfx = ((), '') if block_size == 64 else ((int(block_size),), 'b')
        tail = blk + (DTYPE_CODE[out_dtype], int(w_mant_bits), int(x_mant_bits), _stream(x))
        if T > DECODE8_TOKENS and L.bfpq_hbfp_linear_i8_ok(T, N, K):
            parts = getattr(L, f"bfpq_hbfp_linear_i8{sfx}_parts")(T, N, K, *blk) if SPLIT_K else 1
            if parts > 1:                                              # few output tiles: K split, fp32 slabs added in part order
                slabs = torch.empty((parts, T, N), dtype=torch.float32, device=dev)
                name = f"bfpq_hbfp_linear_i8{sfx}_splitk"
                check(getattr(L, name)(*ops, _ptr(slabs), parts, T, N, K, *tail), name)
            else:
                name = f"bfpq_hbfp_linear_i8{sfx}"
                check(getattr(L, name)(*ops, T, N, K, *tail), name)
        else:
            slabs = torch.empty(int(L.bfpq_hbfp_linear_decode8_ws(T, N, K)), dtype=torch.float32, device=dev)
            name = f"bfpq_hbfp_linear_decode8{sfx}"
            check(getattr(L, name)(*ops, _ptr(slabs), T, N, K, *tail), name)
    return out.view(tuple(x.shape[:-1]) + (N,))



# ---- two HBFP activations on the int8 matrix unit, batched (bfpq_bmm.hip) ---------------------------------
def code_pitch(K):
    """the pitch of a code row of hbfp_bmm_i8: K rounded up to 64-byte chunks"""
    return (int(K) + 63) // 64 * 64


def hbfp_bmm_i8_ok(B, T, N, K, w_mant_bits, x_mant_bits, block_size=64):
    """hbfp_bmm_i8 takes this problem: block 64, 32 or 16, mantissas of 1..7 bits on both sides, any T >= 1, N % 16 == 0,
    K % block_size == 0 (bfpq_hbfp_bmm_i8_ok at the pitch code_pitch(K))"""
    return bool(1 <= w_mant_bits <= 7 and 1 <= x_mant_bits <= 7 and block_size in (64,) + I8_BLOCKS
                and load_library().bfpq_hbfp_bmm_i8_ok(int(B), int(T), int(N), int(K), code_pitch(K), int(block_size)))


def _pitched_codes(codes, rows, K, what):
    """int8 codes [rows, K] (or already [rows, code_pitch(K)]) -> [rows, code_pitch(K)] with zeros in the pad"""
    ldk = code_pitch(K)
    if codes.dtype != torch.int8 or codes.numel() not in (rows * K, rows * ldk):
        raise ValueError(f"hbfp_bmm_i8 takes int8 {what} codes [{rows}, {K}] or [{rows}, {ldk}] (got {tuple(codes.shape)}, {codes.dtype})")
    if codes.numel() == rows * ldk:
        return codes.contiguous()
    return torch.nn.functional.pad(codes.reshape(rows, K), (0, ldk - K))


def hbfp_bmm_i8(xq, wq, B, T, N, K, w_mant_bits, x_mant_bits, block_size=64, out_dtype=torch.float32):
    """out[b] = X[b] @ W[b]^T for b < B, both operands ready-made HBFP codes: xq = (int8 codes [B*T, K], int8 exponents [B*T, K/block_size])
    as act_codes makes them, wq = (codes [B*N, K], exponents [B*N, K/block_size]) from act_codes or codes_transposed (codes may also come
    with the pitch code_pitch(K), zeros in the pad; K % 64 != 0 is padded here).  Block dot products are exact integer sums on the int8
    matrix unit, fp32 across blocks in block order, one rounding to out_dtype.  Returns [B, T, N]."""
    if not hbfp_bmm_i8_ok(B, T, N, K, w_mant_bits, x_mant_bits, block_size):
        raise ValueError(f"hbfp_bmm_i8 needs block 16, 32 or 64, N % 16 == 0, K % block_size == 0 and mantissas of 1..7 bits "
                         f"(got B={B}, T={T}, N={N}, K={K}, w_mant_bits={w_mant_bits}, x_mant_bits={x_mant_bits}, block_size={block_size})")
    if out_dtype not in DTYPE_CODE:
        raise TypeError(f"unsupported dtype {out_dtype}")
    (xc, xe), (wc, we) = xq, wq
    nb = K // block_size
    if xe.numel() != B * T * nb or we.numel() != B * N * nb or xe.dtype != torch.int8 or we.dtype != torch.int8:
        raise ValueError(f"hbfp_bmm_i8 at block {block_size} takes int8 exponents [{B * T}, {nb}] and [{B * N}, {nb}] "
                         f"(got {tuple(xe.shape)} and {tuple(we.shape)})")
    xc, wc = _pitched_codes(xc, B * T, K, "x"), _pitched_codes(wc, B * N, K, "w")
    require_device_tensor_any(xc)
    dev = xc.device
    with torch.cuda.device(dev):
        xe, we = xe.contiguous(), we.contiguous()
        out = torch.empty((B, T, N), dtype=out_dtype, device=dev)
        check(load_library().bfpq_hbfp_bmm_i8(_ptr(xc), _ptr(xe), _ptr(wc), _ptr(we), _ptr(out), B, T, N, K, code_pitch(K), int(block_size),
                                              DTYPE_CODE[out_dtype], int(w_mant_bits), int(x_mant_bits),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "bfpq_hbfp_bmm_i8")
    return out


def codes_transposed(v, block_size, mant_bits, epsilon):
    """v [B, S, D] -> int8 codes [B, D, code_pitch(S)] + int8 exponents [B, D, S/block_size] of float_to_bfp_blocked(v.transpose(-1, -2)),
    HBFP(mant_bits + 1) round-half-even with blocks of block_size along S, dense (bfpq_hbfp_codes_t: one read of v, no transposed copy)"""
    require_device_tensor(v)
    if v.dim() != 3:
        raise ValueError(f"codes_transposed takes a [B, S, D] tensor (got {tuple(v.shape)})")
    B, S, D = v.shape
    if block_size not in (64,) + I8_BLOCKS or not 1 <= mant_bits <= 7 or S % block_size or D % 16:
        raise ValueError(f"codes_transposed needs block 16, 32 or 64, mant_bits 1..7, S % block_size == 0 and D % 16 == 0 "
                         f"(got S={S}, D={D}, block_size={block_size}, mant_bits={mant_bits})")
    src = v.contiguous()
    dev, ldk = src.device, code_pitch(S)
    with torch.cuda.device(dev):
        codes = torch.empty((B, D, ldk), dtype=torch.int8, device=dev)
        exps = torch.empty((B, D, S // block_size), dtype=torch.int8, device=dev)
        check(load_library().bfpq_hbfp_codes_t(_ptr(src), _ptr(codes), _ptr(exps), B, S, D, ldk, DTYPE_CODE[src.dtype], int(block_size),
                                               int(mant_bits), float(epsilon), _ptr(exp_window_dev(src.dtype, dev)), _stream(src)),
              "bfpq_hbfp_codes_t")
    return codes, exps


def hbfp_bmm_i8_strided(xq, wc, we, B, T, N, K, w_bstride, w_rows, w_mant_bits, x_mant_bits, block_size=64, out_dtype=torch.float32):
    """hbfp_bmm_i8 with the second operand read in place from a larger array (a KV cache's codes): wc [..., w_ld] int8 codes and
    we [..., w_exp_ld] int8 exponents, both contiguous, batch b starting w_bstride rows after batch b - 1, the first w_rows <= N rows of a
    batch valid (rows w_rows .. N - 1 of the result repeat row w_rows - 1: the caller drops them).  xq as for hbfp_bmm_i8.  Returns
    [B, T, N] (bfpq_hbfp_bmm_i8_strided)."""
    if not hbfp_bmm_i8_ok(B, T, N, K, w_mant_bits, x_mant_bits, block_size):
        raise ValueError(f"hbfp_bmm_i8_strided needs block 16, 32 or 64, N % 16 == 0, K % block_size == 0 and mantissas of 1..7 bits "
                         f"(got B={B}, T={T}, N={N}, K={K}, w_mant_bits={w_mant_bits}, x_mant_bits={x_mant_bits}, block_size={block_size})")
    if out_dtype not in DTYPE_CODE:
        raise TypeError(f"unsupported dtype {out_dtype}")
    xc, xe = xq
    nb = K // block_size
    if xe.numel() != B * T * nb or xe.dtype != torch.int8 or we.dtype != torch.int8 or wc.dtype != torch.int8:
        raise ValueError(f"hbfp_bmm_i8_strided at block {block_size} takes int8 codes and int8 x exponents [{B * T}, {nb}] (got {tuple(xe.shape)})")
    if not wc.is_contiguous() or not we.is_contiguous():
        raise ValueError("hbfp_bmm_i8_strided takes contiguous w codes and exponents")
    w_ld, w_exp_ld = wc.shape[-1], we.shape[-1]
    if wc.numel() < B * w_bstride * w_ld or we.numel() < B * w_bstride * w_exp_ld:
        raise ValueError(f"hbfp_bmm_i8_strided: w holds fewer than {B} x {w_bstride} rows (codes {tuple(wc.shape)}, exponents {tuple(we.shape)})")
    xc = _pitched_codes(xc, B * T, K, "x")
    require_device_tensor_any(xc)
    dev = xc.device
    with torch.cuda.device(dev):
        xe = xe.contiguous()
        out = torch.empty((B, T, N), dtype=out_dtype, device=dev)
        check(load_library().bfpq_hbfp_bmm_i8_strided(_ptr(xc), _ptr(xe), _ptr(wc), _ptr(we), _ptr(out), B, T, N, K, code_pitch(K), int(w_ld),
                                                      int(w_exp_ld), int(w_bstride), int(w_rows), int(block_size), DTYPE_CODE[out_dtype],
                                                      int(w_mant_bits), int(x_mant_bits),
                                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "bfpq_hbfp_bmm_i8_strided")
    return out


# ---- attention keys and values held as HBFP codes (bfpq_kvcache.hip) -------------------------------------------
KV_QK, KV_PV = 0, 1            # BFPQ_KV_QK, BFPQ_KV_PV
KV_DEC_MAX_TOKENS = 16         # BFPQ_KV_DEC_MAX_TOKENS: kv_bmm_dec quantizes up to this many rows of x itself


def kv_ok(D, cap, block_size):
    """the KV cache takes this head size and capacity (bfpq_kv_ok)"""
    return bool(load_library().bfpq_kv_ok(int(D), int(cap), int(block_size)))


class KVPages(collections.namedtuple("KVPages", "table tokens count capacity")):
    """a paged cache as the _paged entries take it (include/bfpq.h): table int32 [sequences, capacity // tokens] on the device (-1: no
    page), `tokens` per page (a multiple of 64), `count` pages in the pool, `capacity` the most tokens of one sequence.  The code and
    exponent buffers then hold count x heads heads of `tokens` tokens"""
    __slots__ = ()

    def args(self):
        """(page_table, page_tokens, pages) as they stand in front of the stream"""
        return _ptr(self.table), int(self.tokens), int(self.count)


def _kv_page_args(pages):
    """(page_table, page_tokens, pages) of the _cb entries: a KVPages', or those of the contiguous cache"""
    return (None, 0, 0) if pages is None else pages.args()


KV_C4_MAX_MANT = 3             # 4-bit codes hold -7..7: mant_bits <= 3 (and block 64)


def _kv_code_bits(what, code_bits, block_size, mant_bits):
    """code_bits of a KV cache's code buffers: 8 (int8 codes) or 4 (two to a byte; block 64 and mant_bits <= 3).  Returns the codes per byte"""
    if isinstance(code_bits, bool) or not isinstance(code_bits, int):
        raise TypeError(f"{what}: code_bits must be 8 or 4 (got {code_bits!r})")
    if code_bits == 8:
        return 1
    if code_bits != 4:
        raise ValueError(f"{what}: code_bits must be 8 or 4 (got {code_bits})")
    if int(block_size) != 64 or (mant_bits is not None and int(mant_bits) > KV_C4_MAX_MANT):
        raise ValueError(f"{what}: code_bits=4 needs block_size 64 and mant_bits <= {KV_C4_MAX_MANT} (got {block_size}, {mant_bits})")
    return 2


def _kv_pages(what, pages, B, heads, dev):
    """the checks on a KVPages of B sequences; returns the heads the code buffers hold"""
    if not isinstance(pages, KVPages):
        raise ValueError(f"{what}: pages must be a native.KVPages (got {type(pages).__name__})")
    P, N, cap = int(pages.tokens), int(pages.count), int(pages.capacity)
    if P < 64 or P % 64 or N < 1 or cap < P or cap % P:
        raise ValueError(f"{what}: page_tokens must be a multiple of 64 that divides the capacity, pages >= 1 (got {P}, {cap}, {N})")
    _kv_int32(what, "page_table", pages.table, B * (cap // P), dev)
    return N * heads


def _kv_buffers(what, BH, D, block_size, k_codes, k_exps, v_codes, v_exps, v_tail, dev, held=None, per_byte=1):
    """the checks of kv_append on the five cache buffers (held: the heads the code and exponent buffers hold, where not BH: a paged
    cache; per_byte: codes per byte of the two code buffers, whose last dimension is then ldd / per_byte, cap / per_byte); returns
    (cap, ldd), counted in codes"""
    if block_size not in (64,) + I8_BLOCKS:
        raise ValueError(f"{what}: block_size must be 16, 32 or 64 (got {block_size})")
    if k_codes.dim() < 2 or v_codes.dim() < 2:
        raise ValueError(f"{what} takes k_codes [..., cap, ldd] and v_codes [..., D, cap]")
    cap, ldd = k_codes.shape[-2], k_codes.shape[-1] * per_byte
    nbd, nbc = D // block_size, cap // block_size
    HB = BH if held is None else held
    sizes = dict(k_codes=(k_codes, HB * cap * ldd // per_byte), k_exps=(k_exps, HB * cap * nbd), v_codes=(v_codes, HB * D * cap // per_byte),
                 v_exps=(v_exps, HB * D * nbc), v_tail=(v_tail, BH * block_size * D))
    for name, (buf, numel) in sizes.items():
        if buf.device != dev or not buf.is_contiguous() or buf.numel() != numel or (name != "v_tail" and buf.dtype != torch.int8):
            raise ValueError(f"{what}: {name} must be contiguous on {dev} with {numel} elements"
                             f"{'' if name == 'v_tail' else ' of int8'} (got {tuple(buf.shape)}, {buf.dtype}, {buf.device})")
    if v_codes.shape[-1] * per_byte != cap:
        raise ValueError(f"{what} takes v_codes [..., D, cap] with k_codes' capacity")
    return cap, ldd


def _kv_int32(what, name, t, numel, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what}: {name} must be a contiguous int32 tensor of {numel} elements on {dev} "
                         f"(got {tuple(getattr(t, 'shape', ()))}, {getattr(t, 'dtype', None)}, {getattr(t, 'device', None)})")


def _kv_new(what, k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, block_size, heads=None, pages=None, per_byte=1):
    """the checks kv_append and kv_append_dev share on the new rows and the cache buffers; returns (BH, t, D, cap, ldd)"""
    require_device_tensor(k_new, "k_new")
    require_device_tensor(v_new, "v_new")
    require_device_tensor(v_tail, "v_tail")
    if k_new.dim() != 3 or v_new.shape != k_new.shape or v_new.dtype != k_new.dtype or v_tail.dtype != k_new.dtype:
        raise ValueError(f"{what} takes k_new and v_new [BH, t, D] of one dtype, the cache's (got {tuple(k_new.shape)} {k_new.dtype}, "
                         f"{tuple(v_new.shape)} {v_new.dtype}, v_tail {v_tail.dtype})")
    BH, t, D = k_new.shape
    if heads is not None and (heads < 1 or BH % heads):
        raise ValueError(f"{what}: {BH} heads in all are no multiple of heads = {heads}")
    held = None if pages is None else _kv_pages(what, pages, BH // heads, heads, k_new.device)
    cap, ldd = _kv_buffers(what, BH, D, block_size, k_codes, k_exps, v_codes, v_exps, v_tail, k_new.device, held, per_byte)
    if not k_new.is_contiguous() or not v_new.is_contiguous():
        raise ValueError(f"{what} takes contiguous k_new / v_new")
    return BH, t, D, cap, ldd


def kv_append(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, pos, block_size, mant_bits, epsilon):
    """k_new, v_new [BH, t, D] become tokens pos .. pos + t - 1 of the cache buffers (bfpq_kv_append: the layout is in include/bfpq.h);
    one launch for any t >= 1"""
    BH, t, D, cap, ldd = _kv_new("kv_append", k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, block_size)
    dev = k_new.device
    with torch.cuda.device(dev):
        check(load_library().bfpq_kv_append(_ptr(k_new), _ptr(v_new), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail), BH, D,
                                            int(pos), t, cap, ldd, DTYPE_CODE[k_new.dtype], int(block_size), int(mant_bits), float(epsilon),
                                            _ptr(exp_window_dev(k_new.dtype, dev)), _stream(k_new)), "bfpq_kv_append")


def kv_append_dev(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, lengths, counts, overflow, heads, limit, block_size, mant_bits,
                  epsilon, pages=None, code_bits=8):
    """kv_append at the positions lengths [B] (int32, on the device) holds, sequence b = head // heads taking the first counts[b] of the t
    rows (counts None: all), then lengths advanced by a second launch (bfpq_kv_append_dev, bfpq_kv_lens_advance).  A sequence that would
    pass `limit` tokens is left untouched and overflow[0] set to 1.  Nothing is read back.  pages (a KVPages): the buffers are a pool of
    pages (bfpq_kv_append_paged, bfpq_kv_lens_advance_paged), and a sequence one of whose tokens has no page is refused likewise.
    code_bits=4 (block 64, mant_bits <= 3): k_codes [.., cap, ldd / 2] and v_codes [.., D, cap / 2] hold two codes to a byte
    (bfpq_kv_append_cb, paged or not); 8 is the call above in every respect."""
    heads = int(heads)
    per_byte = _kv_code_bits("kv_append_dev", code_bits, block_size, mant_bits)
    BH, t, D, cap, ldd = _kv_new("kv_append_dev", k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, block_size, heads, pages, per_byte)
    dev, B = k_new.device, BH // heads
    _kv_int32("kv_append_dev", "lengths", lengths, B, dev)
    _kv_int32("kv_append_dev", "overflow", overflow, 1, dev)
    if counts is not None:
        _kv_int32("kv_append_dev", "counts", counts, B, dev)
    with torch.cuda.device(dev):
        L, stream = load_library(), _stream(k_new)
        if code_bits == 4:
            check(L.bfpq_kv_append_cb(_ptr(k_new), _ptr(v_new), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail),
                                      _ptr(lengths), _ptr(counts), _ptr(overflow), BH, heads, D, t, cap if pages is None else int(pages.capacity),
                                      int(limit), ldd, DTYPE_CODE[k_new.dtype], int(block_size), int(mant_bits), float(epsilon),
                                      _ptr(exp_window_dev(k_new.dtype, dev)), *_kv_page_args(pages), 4, stream), "bfpq_kv_append_cb")
            if pages is None:
                check(L.bfpq_kv_lens_advance(_ptr(lengths), _ptr(counts), B, t, int(limit), stream), "bfpq_kv_lens_advance")
            else:
                check(L.bfpq_kv_lens_advance_paged(_ptr(lengths), _ptr(counts), B, t, int(limit), int(pages.capacity), *pages.args(), stream),
                      "bfpq_kv_lens_advance_paged")
            return
        if pages is not None:
            check(L.bfpq_kv_append_paged(_ptr(k_new), _ptr(v_new), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail),
                                         _ptr(lengths), _ptr(counts), _ptr(overflow), BH, heads, D, t, int(pages.capacity), int(limit), ldd,
                                         DTYPE_CODE[k_new.dtype], int(block_size), int(mant_bits), float(epsilon),
                                         _ptr(exp_window_dev(k_new.dtype, dev)), *pages.args(), stream), "bfpq_kv_append_paged")
            check(L.bfpq_kv_lens_advance_paged(_ptr(lengths), _ptr(counts), B, t, int(limit), int(pages.capacity), *pages.args(), stream),
                  "bfpq_kv_lens_advance_paged")
            return
        check(L.bfpq_kv_append_dev(_ptr(k_new), _ptr(v_new), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail), _ptr(lengths),
                                   _ptr(counts), _ptr(overflow), BH, heads, D, t, cap, int(limit), ldd, DTYPE_CODE[k_new.dtype], int(block_size),
                                   int(mant_bits), float(epsilon), _ptr(exp_window_dev(k_new.dtype, dev)), stream), "bfpq_kv_append_dev")
        check(L.bfpq_kv_lens_advance(_ptr(lengths), _ptr(counts), B, t, int(limit), stream), "bfpq_kv_lens_advance")


KV_JOB_WORDS = 5                     # a job of kv_rows_move: src_row, dst_row, src_page, dst_page, tokens


def kv_rows_move_ws_bytes(n_jobs, kv_heads, D, block_size, dtype):
    """bytes of the staging buffer kv_rows_move needs for n_jobs jobs (bfpq_kv_rows_move_ws_bytes; no device needed)"""
    n = int(load_library().bfpq_kv_rows_move_ws_bytes(int(n_jobs), int(kv_heads), int(D), int(block_size), DTYPE_CODE[dtype]))
    if n < 0:
        check(n, "bfpq_kv_rows_move_ws_bytes")
    return n


def kv_rows_move(k_codes, k_exps, v_codes, v_exps, v_tail, lengths, overflow, jobs, stage, kv_heads, block_size, pages, code_bits=8):
    """the device side of a reorder of a paged cache's sequences (bfpq_kv_rows_move, include/bfpq.h): jobs int32 [n, 5] on the device
    (src_row, dst_row, src_page, dst_page, tokens); per job the open page copied into a fresh one, and v_tail and the length of src_row
    moved to dst_row through `stage` (uint8, kv_rows_move_ws_bytes(n, ...)), the length only where it equals `tokens` (else 0, and
    overflow[0] set).  Two launches; nothing is read back.  pages: the cache's KVPages.  code_bits=4: the code buffers hold two codes
    to a byte and a page's copy is half the bytes (bfpq_kv_rows_move_cb)"""
    per_byte = _kv_code_bits("kv_rows_move", code_bits, block_size, None)
    require_device_tensor(v_tail, "v_tail")
    dev, B = v_tail.device, lengths.numel()
    D = v_tail.shape[-1]
    held = _kv_pages("kv_rows_move", pages, B, kv_heads, dev)
    _kv_buffers("kv_rows_move", B * kv_heads, D, block_size, k_codes, k_exps, v_codes, v_exps, v_tail, dev, held, per_byte)
    _kv_int32("kv_rows_move", "lengths", lengths, B, dev)
    _kv_int32("kv_rows_move", "overflow", overflow, 1, dev)
    if not isinstance(jobs, torch.Tensor) or jobs.dim() != 2 or jobs.shape[1] != KV_JOB_WORDS:
        raise ValueError(f"kv_rows_move: jobs must be int32 [n, {KV_JOB_WORDS}] (got {tuple(getattr(jobs, 'shape', ()))})")
    n = jobs.shape[0]
    _kv_int32("kv_rows_move", "jobs", jobs, n * KV_JOB_WORDS, dev)
    if not isinstance(stage, torch.Tensor) or stage.dtype != torch.uint8 or stage.device != dev or not stage.is_contiguous():
        raise ValueError(f"kv_rows_move: stage must be a contiguous uint8 tensor on {dev}")
    with torch.cuda.device(dev):
        if code_bits == 4:
            check(load_library().bfpq_kv_rows_move_cb(_ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail), _ptr(lengths),
                                                      _ptr(overflow), _ptr(jobs), n, _ptr(stage), stage.numel(), B, int(kv_heads), D,
                                                      int(block_size), DTYPE_CODE[v_tail.dtype], int(pages.tokens), int(pages.count), 4,
                                                      _stream(v_tail)), "bfpq_kv_rows_move_cb")
            return
        check(load_library().bfpq_kv_rows_move(_ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(v_tail), _ptr(lengths),
                                               _ptr(overflow), _ptr(jobs), n, _ptr(stage), stage.numel(), B, int(kv_heads), D, int(block_size),
                                               DTYPE_CODE[v_tail.dtype], int(pages.tokens), int(pages.count), _stream(v_tail)),
              "bfpq_kv_rows_move")


def kv_dec_ws_bytes(BH, Tq, D, L, block_size):
    """bytes of the workspace kv_bmm_dec_dev's KV_PV family needs (bfpq_kv_dec_ws_bytes; no device needed)"""
    n = int(load_library().bfpq_kv_dec_ws_bytes(int(BH), int(Tq), int(D), int(L), int(block_size)))
    if n < 0:
        check(n, "bfpq_kv_dec_ws_bytes")
    return n


def _kv_group(what, rows, group):
    """the query rows per head of `rows` = group * Tq rows of a kv head serving `group` query heads"""
    if isinstance(group, bool) or not isinstance(group, int) or group < 1:
        raise ValueError(f"{what}: group must be an int >= 1 (got {group!r})")
    if rows % group:
        raise ValueError(f"{what}: {rows} rows per kv head are no multiple of group = {group}")
    return rows // group


def _kv_rows(what, x, form, group=1, heads=1):
    """the query-side tensor x [BH, group * Tq, last] of an entry (`form`: how its message spells it); returns (x contiguous, BH, R, Tq,
    last, heads)"""
    require_device_tensor(x, form.split()[0])
    if x.dim() != 3:
        raise ValueError(f"{what} takes {form} (got {tuple(x.shape)})")
    BH, R, last = x.shape
    Tq = _kv_group(what, R, group)
    heads = int(heads)
    if heads < 1 or BH % heads:
        raise ValueError(f"{what}: {BH} heads in all are no multiple of heads = {heads}")
    return x.contiguous(), BH, R, Tq, last, heads


def _kv_operand(what, BH, w_bstride, wc, we, dev):   # (a paged cache: BH the heads the pool holds)
    """one cached operand of kv_bmm_dec / kv_bmm_dec_dev: contiguous codes and exponents of BH x w_bstride rows (4-bit codes: the rows
    are half as long, which is the last dimension that this reads)"""
    for name, buf in (("codes", wc), ("exponents", we)):
        if buf.device != dev or buf.dtype != torch.int8 or not buf.is_contiguous() or buf.numel() < BH * int(w_bstride) * buf.shape[-1]:
            raise ValueError(f"{what}: the cached {name} must be contiguous int8 on {dev} with {BH} x {w_bstride} rows "
                             f"(got {tuple(buf.shape)}, {buf.dtype}, {buf.device})")


def _kv_cached(what, BH, D, block_size, k_codes, k_exps, v_codes, v_exps, dev, per_byte=1):
    """the four code and exponent buffers of BH cached heads (a paged cache: the heads the pool holds, of a page's tokens each) as the
    attend entries take them (per_byte: as _kv_buffers); returns (cap, ldd), counted in codes"""
    if k_codes.dim() < 2 or v_codes.dim() < 2:
        raise ValueError(f"{what} takes k_codes [..., cap, ldd] and v_codes [..., D, cap]")
    cap, ldd = k_codes.shape[-2], k_codes.shape[-1] * per_byte
    nbd, nbc = D // int(block_size), cap // int(block_size)
    for name, buf, numel in (("k_codes", k_codes, BH * cap * ldd // per_byte), ("k_exps", k_exps, BH * cap * nbd),
                             ("v_codes", v_codes, BH * D * cap // per_byte), ("v_exps", v_exps, BH * D * nbc)):
        if buf.device != dev or buf.dtype != torch.int8 or not buf.is_contiguous() or buf.numel() != numel:
            raise ValueError(f"{what}: {name} must be contiguous int8 on {dev} with {numel} elements "
                             f"(got {tuple(buf.shape)}, {buf.dtype}, {buf.device})")
    return cap, ldd


def _kv_ws(what, name, ws, need, dev):
    """a workspace: a contiguous uint8 tensor of at least `need` bytes; returns its bytes"""
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"{what}: {name} must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return ws.numel()


def _kv_scale(what, scale):
    scale = float(scale)
    if not math.isfinite(scale) or abs(scale) > torch.finfo(torch.float32).max:
        raise ValueError(f"{what}: scale must be finite in fp32 (got {scale})")
    return scale


def kv_bmm_dec_dev(x, wc, we, family, bound, w_bstride, lengths, heads, block_size, mant_bits, epsilon, ws=None, chunks_per_split=0, group=1,
                   pages=None, code_bits=8):
    """kv_bmm_dec with head b's cached length read from lengths[b // heads] on the device (bfpq_kv_bmm_dec_gqa).  KV_QK: x [BH, Tq, D],
    bound = max_len; returns [BH, Tq, max_len], -inf from the length on.  KV_PV: x [BH, Tq, L], bound = D; returns [BH, Tq, D]; ws: a
    uint8 tensor of at least kv_dec_ws_bytes(BH, Tq, D, L, block_size) bytes; chunks_per_split: 64-token chunks per slice of the
    contraction, 0 = the library's choice (the result does not depend on it).  group > 1 (grouped-query attention): the BH cached heads
    serve `group` query heads each, x and the result hold group * Tq rows per cached head -- query head r // Tq of the group, token
    r % Tq -- and the workspace is that of BH * group heads.  pages (a KVPages): wc / we are a pool of pages (bfpq_kv_bmm_dec_paged),
    w_bstride for KV_QK a page's tokens.  code_bits=4 (block 64, mant_bits <= 3): wc holds two codes to a byte, its rows half as long
    (bfpq_kv_bmm_dec_cb, paged or not); the result is that of the int8 codes, bit for bit."""
    x, BH, R, Tq, Kx, heads = _kv_rows("kv_bmm_dec_dev", x, "x [BH, Tq, Kx]", group, heads)
    per_byte = _kv_code_bits("kv_bmm_dec_dev", code_bits, block_size, mant_bits)
    dev = x.device
    _kv_operand("kv_bmm_dec_dev", BH if pages is None else _kv_pages("kv_bmm_dec_dev", pages, BH // heads, heads, dev), w_bstride, wc, we, dev)
    _kv_int32("kv_bmm_dec_dev", "lengths", lengths, BH // heads, dev)
    Nout = int(bound)
    ws_bytes = 0
    if family == KV_PV:
        ws_bytes = _kv_ws("kv_bmm_dec_dev", "ws", ws, kv_dec_ws_bytes(BH * group, Tq, Nout, Kx, block_size), dev)
    ldo = (Nout + 3) // 4 * 4
    with torch.cuda.device(dev):
        out = torch.empty((BH, R, ldo), dtype=x.dtype, device=dev)
        args = (_ptr(x), _ptr(wc), _ptr(we), _ptr(out), _ptr(lengths), BH, heads, Tq, group, Kx, Nout, Kx, wc.shape[-1] * per_byte, we.shape[-1],
                int(w_bstride), ldo, int(family), DTYPE_CODE[x.dtype], int(block_size), int(mant_bits), int(mant_bits), float(epsilon),
                _ptr(exp_window_dev(x.dtype, dev)), _ptr(ws if family == KV_PV else None), ws_bytes, int(chunks_per_split))
        if code_bits == 4:
            check(load_library().bfpq_kv_bmm_dec_cb(*args, 0 if pages is None else int(pages.capacity), *_kv_page_args(pages), 4, _stream(x)),
                  "bfpq_kv_bmm_dec_cb")
        elif pages is None:
            check(load_library().bfpq_kv_bmm_dec_gqa(*args, _stream(x)), "bfpq_kv_bmm_dec_gqa")
        else:
            check(load_library().bfpq_kv_bmm_dec_paged(*args, int(pages.capacity), *pages.args(), _stream(x)), "bfpq_kv_bmm_dec_paged")
    return out[:, :, :Nout] if ldo != Nout else out


def kv_attend_ws_bytes(BH, Tq, max_len):
    """bytes of kv_attend's fp32 score rows (bfpq_kv_attend_ws_bytes; no device needed)"""
    n = int(load_library().bfpq_kv_attend_ws_bytes(int(BH), int(Tq), int(max_len)))
    if n < 0:
        check(n, "bfpq_kv_attend_ws_bytes")
    return n


def _kv_window(what, BH, heads, starts, window, dev):
    """the first-key arguments of the _win entries: (starts or None, window as an int, 0 for none); both absent means the plain entry"""
    if starts is not None:
        _kv_int32(what, "starts", starts, BH // heads, dev)
    if window is None:
        window = 0
    elif isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{what}: window must be None or an int >= 1 (got {window!r})")
    return starts, window


def _kv_paged_cached(what, pages, starts, window, BH, heads, D, block_size, k_codes, k_exps, v_codes, v_exps, dev, per_byte=1):
    """_kv_cached for the attend entries, on a pool of pages where `pages` is given; returns (the cap the entry takes, ldd)"""
    if pages is None:
        return _kv_cached(what, BH, D, block_size, k_codes, k_exps, v_codes, v_exps, dev, per_byte)
    if starts is not None or window:
        raise NotImplementedError(f"{what}: a paged cache takes no starts and no window")
    held = _kv_pages(what, pages, BH // heads, heads, dev)
    P, ldd = _kv_cached(what, held, D, block_size, k_codes, k_exps, v_codes, v_exps, dev, per_byte)
    if P != int(pages.tokens):
        raise ValueError(f"{what}: the buffers hold heads of {P} tokens, a page has {pages.tokens}")
    return int(pages.capacity), ldd


def kv_attend(q, k_codes, k_exps, v_codes, v_exps, lengths, heads, max_len, scale, causal, block_size, mant_bits, epsilon, score_ws, sum_ws,
              chunks_per_split=0, return_probs=False, group=1, starts=None, window=None, pages=None, code_bits=8):
    """scores, scale, softmax and context of q [BH, Tq, D] against a device-length cache in three launches (bfpq_kv_attend_gqa): returns
    (context [BH, Tq, D], p [BH, Tq, max_len] or None).  score_ws / sum_ws: contiguous uint8 tensors of at least
    kv_attend_ws_bytes(BH, Tq, max_len) / kv_dec_ws_bytes(BH, Tq, D, max_len, block_size) bytes.  Nothing is read back.  group > 1: rows
    and workspaces as kv_bmm_dec_dev takes them (q, the context and p hold group * Tq rows per cached head; causal goes by the token).
    starts (int32 [BH // heads] on the device) and / or window (an int >= 1): the rows see the keys from max(starts[b], what they see
    minus window) on (bfpq_kv_attend_gqa_win); with neither, the call and its kernels are the ones without.  pages (a KVPages; with neither
    starts nor window): the buffers are a pool of pages (bfpq_kv_attend_paged).  code_bits=4 (block 64, mant_bits <= 3): the code buffers
    hold two codes to a byte (bfpq_kv_attend_cb, with or without starts / window / pages); the bits are those of the int8 codes."""
    q, BH, R, Tq, D, heads = _kv_rows("kv_attend", q, "q [BH, Tq, D]", group, heads)
    per_byte = _kv_code_bits("kv_attend", code_bits, block_size, mant_bits)
    dev = q.device
    starts, window = _kv_window("kv_attend", BH, heads, starts, window, dev)
    cap, ldd = _kv_paged_cached("kv_attend", pages, starts, window, BH, heads, D, block_size, k_codes, k_exps, v_codes, v_exps, dev, per_byte)
    _kv_int32("kv_attend", "lengths", lengths, BH // heads, dev)
    max_len, scale = int(max_len), _kv_scale("kv_attend", scale)
    score_bytes = _kv_ws("kv_attend", "score_ws", score_ws, kv_attend_ws_bytes(BH * group, Tq, max_len), dev)
    sum_bytes = _kv_ws("kv_attend", "sum_ws", sum_ws, kv_dec_ws_bytes(BH * group, Tq, D, max_len, block_size), dev)
    with torch.cuda.device(dev):
        out = torch.empty((BH, R, D), dtype=q.dtype, device=dev)
        p = torch.empty((BH, R, max_len), dtype=q.dtype, device=dev) if return_probs else None
        args = (_ptr(q), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(out), _ptr(p), _ptr(lengths), BH, heads, Tq, group, D,
                max_len, cap, ldd, D, max_len, scale, int(bool(causal)), DTYPE_CODE[q.dtype], int(block_size), int(mant_bits), int(mant_bits),
                float(epsilon), _ptr(exp_window_dev(q.dtype, dev)), _ptr(score_ws), score_bytes, _ptr(sum_ws), sum_bytes, int(chunks_per_split))
        if code_bits == 4:
            check(load_library().bfpq_kv_attend_cb(*args, _ptr(starts), window, *_kv_page_args(pages), 4, _stream(q)), "bfpq_kv_attend_cb")
        elif pages is not None:
            check(load_library().bfpq_kv_attend_paged(*args, *pages.args(), _stream(q)), "bfpq_kv_attend_paged")
        elif starts is None and not window:
            check(load_library().bfpq_kv_attend_gqa(*args, _stream(q)), "bfpq_kv_attend_gqa")
        else:
            check(load_library().bfpq_kv_attend_gqa_win(*args, _ptr(starts), window, _stream(q)), "bfpq_kv_attend_gqa_win")
    return out, p


KV_ROWS_MAX_HEAD_DIM = 256     # bfpq_kv_attend_rows keeps a row's accumulators for all of D in registers


def kv_attend_rows_ws_bytes(BH, P, max_len):
    """bytes of kv_attend_rows' fp32 score rows for panels of P rows of BH query heads (bfpq_kv_attend_rows_ws_bytes; no device needed)"""
    n = int(load_library().bfpq_kv_attend_rows_ws_bytes(int(BH), int(P), int(max_len)))
    if n < 0:
        check(n, "bfpq_kv_attend_rows_ws_bytes")
    return n


def kv_attend_rows(q, k_codes, k_exps, v_codes, v_exps, lengths, heads, max_len, scale, causal, block_size, mant_bits, epsilon, score_ws,
                   panel_rows, return_probs=False, group=1, starts=None, window=None, pages=None, code_bits=8):
    """kv_attend for any number of query rows (bfpq_kv_attend_rows): q [BH, group * Tq, D] is walked in panels of panel_rows tokens per
    query head, two launches per panel, the panel's fp32 score rows in score_ws (a contiguous uint8 tensor of at least
    kv_attend_rows_ws_bytes(BH * group, min(panel_rows, Tq), max_len) bytes).  Returns (context [BH, group * Tq, D], p
    [BH, group * Tq, max_len] or None); row for row kv_attend's bits.  Nothing is read back.  starts, window: as kv_attend
    (bfpq_kv_attend_rows_win); pages: as kv_attend (bfpq_kv_attend_rows_paged); code_bits: as kv_attend (bfpq_kv_attend_rows_cb)."""
    q, BH, R, Tq, D, heads = _kv_rows("kv_attend_rows", q, "q [BH, Tq, D]", group, heads)
    per_byte = _kv_code_bits("kv_attend_rows", code_bits, block_size, mant_bits)
    panel_rows = int(panel_rows)
    if panel_rows < 1:
        raise ValueError(f"kv_attend_rows: panel_rows must be >= 1 (got {panel_rows})")
    dev = q.device
    starts, window = _kv_window("kv_attend_rows", BH, heads, starts, window, dev)
    cap, ldd = _kv_paged_cached("kv_attend_rows", pages, starts, window, BH, heads, D, block_size, k_codes, k_exps, v_codes, v_exps, dev,
                                per_byte)
    _kv_int32("kv_attend_rows", "lengths", lengths, BH // heads, dev)
    max_len, scale = int(max_len), _kv_scale("kv_attend_rows", scale)
    score_bytes = _kv_ws("kv_attend_rows", "score_ws", score_ws, kv_attend_rows_ws_bytes(BH * group, min(panel_rows, Tq), max_len), dev)
    with torch.cuda.device(dev):
        out = torch.empty((BH, R, D), dtype=q.dtype, device=dev)
        p = torch.empty((BH, R, max_len), dtype=q.dtype, device=dev) if return_probs else None
        L, win, stream = load_library(), _ptr(exp_window_dev(q.dtype, dev)), _stream(q)
        for row0 in range(0, Tq, panel_rows):
            args = (_ptr(q), _ptr(k_codes), _ptr(k_exps), _ptr(v_codes), _ptr(v_exps), _ptr(out), _ptr(p), _ptr(lengths), BH, heads, Tq, group, D,
                    max_len, cap, ldd, D, max_len, scale, int(bool(causal)), DTYPE_CODE[q.dtype], int(block_size), int(mant_bits), int(mant_bits),
                    float(epsilon), win, _ptr(score_ws), score_bytes, None, 0, 0, row0, min(panel_rows, Tq - row0))
            if code_bits == 4:
                check(L.bfpq_kv_attend_rows_cb(*args, _ptr(starts), window, *_kv_page_args(pages), 4, stream), "bfpq_kv_attend_rows_cb")
            elif pages is not None:
                check(L.bfpq_kv_attend_rows_paged(*args, *pages.args(), stream), "bfpq_kv_attend_rows_paged")
            elif starts is None and not window:
                check(L.bfpq_kv_attend_rows(*args, stream), "bfpq_kv_attend_rows")
            else:
                check(L.bfpq_kv_attend_rows_win(*args, _ptr(starts), window, stream), "bfpq_kv_attend_rows_win")
    return out, p


def kv_bmm_dec(x, wc, we, family, Nout, w_bstride, block_size, mant_bits, epsilon):
    """x [BH, Tq <= 16, Kx] (dense) against one cached operand, x quantized inside the kernel
    (bfpq_kv_bmm_dec).  wc [..., ldw] / we [..., ldwe]: contiguous codes / exponents, w_bstride rows per head.  Returns [BH, Tq, Nout]:
    a view of a buffer whose row pitch is Nout rounded up to 4."""
    x, BH, _, Tq, Kx, _ = _kv_rows("kv_bmm_dec", x, "x [BH, Tq, Kx]")
    dev = x.device
    _kv_operand("kv_bmm_dec", BH, w_bstride, wc, we, dev)
    ldo = (int(Nout) + 3) // 4 * 4
    with torch.cuda.device(dev):
        out = torch.empty((BH, Tq, ldo), dtype=x.dtype, device=dev)
        check(load_library().bfpq_kv_bmm_dec(_ptr(x), _ptr(wc), _ptr(we), _ptr(out), BH, Tq, Kx, int(Nout), Kx, wc.shape[-1], we.shape[-1],
                                             int(w_bstride), ldo, int(family), DTYPE_CODE[x.dtype], int(block_size), int(mant_bits),
                                             int(mant_bits), float(epsilon), _ptr(exp_window_dev(x.dtype, dev)), _stream(x)), "bfpq_kv_bmm_dec")
    return out[:, :, :Nout] if ldo != Nout else out


# ---- 2:4-compressed packed weights on the sparse int8 matrix unit (bfpq_sp24.hip) -----------------
SP24_MAX_TOKENS = 64      # BFPQ_SP24_MAX_TOKENS: hbfp_linear_sp24 takes 1..64 tokens


def sp24_nbytes(N, K, code_bits):
    """(value bytes, position bytes) of an [N, K] weight in sp24 form: 2 kept codes + 2 x 2-bit positions per group of 4"""
    return N * K * code_bits // 16, N * K // 8


def sp24_shape_ok(N, K):
    return N >= 16 and N % 16 == 0 and K >= 64 and K % 64 == 0 and N * K < (1 << 32)


def sp24_pack(codes, N, K, code_bits):
    """dense packed codes of an [N, K] weight (4-bit: uint8 [N, K/2]; 8-bit: int8 [N, K], as quantize_nm writes them) -> sp24
    (vals uint8, idx uint8; bfpq_sp24_pack).  Raises ValueError if some group of 4 codes has more than 2 non-zeros (synchronises to
    read the flag, as compact24 does)."""
    require_device_tensor_any(codes)
    if code_bits not in (4, 8) or not sp24_shape_ok(N, K):
        raise ValueError(f"sp24 needs 4- or 8-bit codes, N % 16 == 0 and K % 64 == 0 (got N={N}, K={K}, code_bits={code_bits})")
    c = codes.contiguous()
    nv, ni = sp24_nbytes(N, K, code_bits)
    if c.numel() * c.element_size() != N * K * code_bits // 8:
        raise ValueError(f"sp24_pack: {tuple(c.shape)} {c.dtype} codes are not an [{N}, {K}] weight of {code_bits}-bit codes")
    dev = c.device
    with torch.cuda.device(dev):
        vals = torch.empty(nv, dtype=torch.uint8, device=dev)
        idx = torch.empty(ni, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        check(load_library().bfpq_sp24_pack(_ptr(c), _ptr(vals), _ptr(idx), N, K, int(code_bits), _ptr(status), _stream(c)), "bfpq_sp24_pack")
    if int(status.item()):
        raise ValueError("sp24_pack: a group of 4 codes has more than 2 non-zeros (the weight is not 2:4 sparse)")
    return vals, idx


def sp24_unpack(vals, idx, N, K, code_bits, codes=True, codes8=False):
    """sp24 -> dense codes of the same width (4-bit: uint8 [N, K/2]; 8-bit: int8 [N, K]) and / or int8 codes [N, K]
    (bfpq_sp24_unpack, one launch).  Returns the codes, the int8 codes, or (codes, int8 codes) when both are asked for."""
    require_device_tensor_any(vals)
    if not (codes or codes8):
        raise ValueError("sp24_unpack: ask for codes, int8 codes or both")
    dev = vals.device
    with torch.cuda.device(dev):
        c = None
        if codes:
            c = torch.empty((N, K // 2), dtype=torch.uint8, device=dev) if code_bits == 4 else torch.empty((N, K), dtype=torch.int8, device=dev)
        c8 = torch.empty((N, K), dtype=torch.int8, device=dev) if codes8 else None
        check(load_library().bfpq_sp24_unpack(_ptr(vals.contiguous()), _ptr(idx.contiguous()), _ptr(c), _ptr(c8), N, K, int(code_bits),
                                              _stream(vals)), "bfpq_sp24_unpack")
    if codes and codes8:
        return c, c8
    return c if codes else c8


def hbfp_linear_sp24_ok(T, N, K, code_bits, w_mant_bits, x_mant_bits):
    """hbfp_linear_sp24 takes this problem: 1..SP24_MAX_TOKENS tokens, 4-bit codes with 1..3 mantissa bits or 8-bit codes with 1..7,
    activations of 1..7 mantissa bits, N % 16 == 0, K % 64 == 0"""
    return (code_bits in (4, 8) and 1 <= w_mant_bits <= (3 if code_bits == 4 else 7) and 1 <= x_mant_bits <= 7 and 1 <= T <= SP24_MAX_TOKENS
            and sp24_shape_ok(N, K) and load_library().bfpq_hbfp_linear_sp24_ws(T, N, K) >= 0)


def hbfp_linear_sp24(x, wvals, widx, wexps, N, code_bits, w_mant_bits, x_mant_bits, epsilon=1e-8, bias=None, out_dtype=None, act=None, xq=None):
    """out = Q(x) @ W^T (+ bias) for 1..SP24_MAX_TOKENS tokens with W [N, K] in sp24 form (vals / idx of sp24_pack + the dense packed
    weight's int8 exponents [N, K/64]), x quantized to HBFP(x_mant_bits + 1) block 64, round-half-even, pruned by `act` (ActSparsity or
    None).  One v_smfmac_i32_16x16x64_i8 per block: exact integer block sums, fp32 across blocks.  xq: the activation operand made
    beforehand (act_codes); x then only gives shape and dtype."""
    require_device_tensor(x)
    L = load_library()
    K = x.shape[-1]
    T = x.numel() // K
    if not hbfp_linear_sp24_ok(T, N, K, code_bits, w_mant_bits, x_mant_bits):
        raise ValueError(f"hbfp_linear_sp24 needs 1..{SP24_MAX_TOKENS} tokens, N % 16 == 0, K % 64 == 0 and mantissas that fit the codes "
                         f"(got T={T}, N={N}, K={K}, code_bits={code_bits}, w_mant_bits={w_mant_bits}, x_mant_bits={x_mant_bits})")
    nv, ni = sp24_nbytes(N, K, code_bits)
    if wvals.numel() != nv or widx.numel() != ni or wexps.numel() != N * (K // 64):
        raise ValueError(f"hbfp_linear_sp24: an [{N}, {K}] weight has {nv} value bytes, {ni} position bytes and {N * (K // 64)} exponents")
    dev = x.device
    out_dtype = out_dtype or x.dtype
    with torch.cuda.device(dev):
        xc, xe, out, bias = _linear_operands(x, T, N, K, x_mant_bits, epsilon, act, xq, bias, out_dtype)
        slabs = torch.empty(int(L.bfpq_hbfp_linear_sp24_ws(T, N, K)), dtype=torch.float32, device=dev)
        check(L.bfpq_hbfp_linear_sp24(_ptr(xc), _ptr(xe), _ptr(wvals.contiguous()), _ptr(widx.contiguous()), _ptr(wexps.contiguous()),
                                      _ptr(bias), _ptr(out), _ptr(slabs), T, N, K, int(code_bits),
                                      DTYPE_CODE[out_dtype], int(w_mant_bits), int(x_mant_bits), _stream(x)), "bfpq_hbfp_linear_sp24")
    return out.view(tuple(x.shape[:-1]) + (N,))


# ---- fused BFPAdam step (bfpq_adam_step_list) -------------------------------------------------------------------------------
ADAM_MAX_LIST = 64                 # tensors per launch of bfpq_adam_step_list
adam_launches = 0                  # launches issued by AdamStepList.run so far (tests count them)


class _AdamHparams(ctypes.Structure):
    """include/bfpq.h: bfpq_adam_hparams"""
    _fields_ = [("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("amsgrad", ctypes.c_int), ("block_size", ctypes.c_int), ("mant_bits", ctypes.c_int), ("stoch", ctypes.c_int),
                ("epsilon", ctypes.c_double), ("exp_win_dev", ctypes.c_void_p)]


class _AdamTensor(ctypes.Structure):
    """include/bfpq.h: bfpq_adam_tensor"""
    _fields_ = [("p_dev", ctypes.c_void_p), ("grad_dev", ctypes.c_void_p), ("exp_avg_dev", ctypes.c_void_p), ("exp_avg_sq_dev", ctypes.c_void_p),
                ("max_exp_avg_sq_dev", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("step_size", ctypes.c_double),
                ("seed", ctypes.c_uint64)]


def adam_snap_ok(block_size, mant_bits):
    """True if the fused step takes this snap (block_size 0: no snap)"""
    return bool(load_library().bfpq_adam_step_list_ok(int(block_size), int(mant_bits)))


_ADAM_FIELDS = ("p_dev", "grad_dev", "exp_avg_dev", "exp_avg_sq_dev", "max_exp_avg_sq_dev")


class AdamStepList:
    """A list of fp32 parameters with their grads and Adam states bound to bfpq_adam_step_list: the descriptors are built once;
    run() writes each tensor's step size and seed, re-points a descriptor whose tensors moved (a grad set to None and made again
    has new storage), and issues one launch per 64 tensors on the current stream of the list's device.
    slots: per tensor the tuple (p, grad, exp_avg, exp_avg_sq, max_exp_avg_sq or None), contiguous fp32 on one ROCm device."""

    def __init__(self, slots, betas, eps, weight_decay, amsgrad, block_size=0, mant_bits=0, stoch=False, epsilon=0.0):
        slots = [tuple(s) for s in slots]
        self.n = len(slots)
        self.device = slots[0][0].device if slots else None
        self._descs = (_AdamTensor * max(self.n, 1))()
        self._ptrs = [[0] * 5 for _ in range(self.n)]
        for i, s in enumerate(slots):
            p = s[0]
            cols = p.shape[-1] if p.dim() else 1
            d = self._descs[i]
            d.rows, d.cols = (p.numel() // cols if cols else 0), cols
        self.hp = _AdamHparams(float(betas[0]), float(betas[1]), float(eps), float(weight_decay), 1 if amsgrad else 0, int(block_size),
                               int(mant_bits), 1 if stoch else 0, float(epsilon), None)
        self._win = None
        if block_size and self.device is not None:
            self._win = exp_window_dev(torch.float32, self.device)
            self.hp.exp_win_dev = self._win.data_ptr()
        self._fn = load_library().bfpq_adam_step_list
        self.launches = -(-sum(1 for i in range(self.n) if self._descs[i].rows * self._descs[i].cols) // ADAM_MAX_LIST)

    def run(self, slots, step_sizes, seeds=None):
        """slots: the same tensors as bound (their storage may have moved); step_sizes: per tensor the double step size; seeds: per
        tensor the stochastic snap's seed (None: round-half-even)"""
        global adam_launches
        descs, ptrs = self._descs, self._ptrs
        for i, s in enumerate(slots):
            d, pp = descs[i], ptrs[i]
            for j in range(5):
                t = s[j]
                cur = t.data_ptr() if t is not None else 0
                if cur != pp[j]:
                    setattr(d, _ADAM_FIELDS[j], cur)
                    pp[j] = cur
            d.step_size = step_sizes[i]
            if seeds is not None:
                d.seed = seeds[i]
        if not self.n:
            return
        dev = self.device
        with torch.cuda.device(dev):
            rc = self._fn(ctypes.addressof(self.hp), ctypes.addressof(descs), self.n, torch.cuda.current_stream(dev).cuda_stream)
        check(rc, "bfpq_adam_step_list")
        adam_launches += self.launches


def adam_step_list(slots, step_sizes, betas, eps, weight_decay=0.0, amsgrad=False, block_size=0, mant_bits=0, seeds=None, epsilon=0.0):
    """one fused Adam step (+ HBFP snap when block_size > 0; stochastic when seeds are given) over `slots` (see AdamStepList), bound
    for this call only; BFPAdam(fused=True) keeps its AdamStepList from step to step instead"""
    bound = AdamStepList(slots, betas, eps, weight_decay, amsgrad, block_size, mant_bits, seeds is not None, epsilon)
    bound.run(slots, step_sizes, seeds)
