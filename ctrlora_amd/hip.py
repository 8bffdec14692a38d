"""ctypes binding of libctrlora_hip.so (include/ctrlora_hip.h) for torch tensors.

PyTorch is plumbing here: device memory, the current HIP stream, torch.distributed.
Every function enqueues hand-written gfx950 kernels on `torch.cuda.current_stream()`.
There is NO fallback: if the library is missing or a kernel rejects its arguments the
call raises -- a product path that silently ran ATen / CPU code would void every
parity claim.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTRLORA_LIB") or os.path.join(_HERE, "libctrlora_hip.so")   # (CTRLORA_LIB: A/B builds of the same ABI)

BF16, F32 = 0, 1
LINEAR, CONV_S1, CONV_S2, CONV_UP2, CONV_T2, CONV_S2A, CONV_UP2P, CONV_T2P, CONV_S2K4 = 0, 1, 2, 3, 4, 5, 6, 7, 8
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GEGLU_SPLIT, ACT_GELU = 0, 1, 2, 3, 4


class HipError(RuntimeError):
    pass


class WgradDesc(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("lddy", C.c_long), ("x", C.c_void_p), ("ldx", C.c_long),
                ("dW", C.c_void_p), ("lddw", C.c_long), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("scale", C.c_float), ("tap", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Hout", C.c_int),
                ("Wout", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("reserved", C.c_int)]


class GemmParams(C.Structure):
    _fields_ = [
        ("A1", C.c_void_p), ("lda1", C.c_long), ("K1", C.c_int),
        ("W1", C.c_void_p), ("ldw1", C.c_long),
        ("A2", C.c_void_p), ("lda2", C.c_long), ("K2", C.c_int),
        ("W2", C.c_void_p), ("ldw2", C.c_long),
        ("M", C.c_int), ("N", C.c_int), ("mode", C.c_int),
        ("B", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Hout", C.c_int), ("Wout", C.c_int),
        ("zero_page", C.c_void_p), ("bias", C.c_void_p),
        ("rowbias", C.c_void_p), ("ldrb", C.c_long), ("rows_per_batch", C.c_int),
        ("residual", C.c_void_p), ("ldr", C.c_long),
        ("alpha", C.c_float), ("beta", C.c_float), ("act", C.c_int),
        ("C", C.c_void_p), ("ldc", C.c_long),
        ("out_f32", C.c_int), ("atomic", C.c_int), ("splitk", C.c_int),
        ("a1_group_n", C.c_int), ("a2_group_n", C.c_int), ("alpha_n", C.c_int),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("ln_stats", C.c_void_p),
    ]


_lib = None

# name -> argtypes (restype is int except where noted); mirrors include/ctrlora_hip.h
_P, _L, _I, _F = C.c_void_p, C.c_long, C.c_int, C.c_float
_SIGS = {
    "cl_abi_version": [],
    "cl_last_hip_error": [],
    "cl_set_workspace": [_P, _L],
    "cl_set_stream_workspace": [_P, _P, _L],
    "cl_gemm_force_config": [_I],
    "cl_gemm_force_splitk": [_I],
    "cl_gemm_tune_set": [_I] * 9,
    "cl_gemm_tune_clear": [],
    "cl_gemm_tune_size": [],
    "cl_gemm": [C.POINTER(GemmParams), _I, _P],
    "cl_lora_down": [_I, _P, _L, _P, _I, _P, _L, _I, _I, _P],
    "cl_lora_linear_fwd": [_I, _P, _L, _P, _P, _P, _L, _P, _I, _P, _L, _I, _P, _L, _I, _I, _I, _P],
    "cl_lora_linear_bwd_data": [_I, _P, _L, _P, _P, _P, _I, _P, _L, _P, _L, _P, _L, _I, _I, _I, _P],
    "cl_weight_grad": [_I, _P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _P],
    "cl_weight_grad_tn_group": [_I, _I, _P, _P, _P],
    "cl_weight_grad_tn": [_I, _P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _P, _P],
    "cl_conv3x3_fwd": [_I, _I, _P, _L, _P, _P, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P, _P],
    "cl_conv3x3_bwd_data": [_I, _I, _P, _L, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P, _P],
    "cl_conv1x1_fwd": [_I, _P, _L, _P, _P, _F, _P, _L, _F, _P, _L, _I, _I, _I, _P],
    "cl_groupnorm_ws_floats": [_I, _I, _I],
    "cl_groupnorm_silu_fwd": [_I, _P, _L, _P, _L, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _P],
    "cl_groupnorm_silu_bwd": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "cl_layernorm_fwd": [_I, _P, _L, _P, _L, _P, _P, _I, _I, _F, _P, _P],
    "cl_layernorm_bwd": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _I, _I, _P, _P, _P],
    "cl_attention_fwd": [_I, _P, _L, _P, _L, _P, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "cl_attention_bwd": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _I, _P, _I, _P, _P, _I, _P, _L, _P, _L,
                         _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "cl_attention_fwd_v2": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P],
    "cl_attention_fwd_ip": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _F, _I, _P],
    "cl_attention_bwd_v2": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _I, _P, _L, _P, _L, _P, _L,
                            _I, _I, _I, _I, _I, _F, _I, _P, _P],
    "cl_attention_causal_fwd": [_I, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P],
    "cl_geglu_fwd": [_I, _P, _L, _P, _L, _L, _I, _P],
    "cl_geglu_bwd": [_I, _P, _L, _P, _L, _P, _L, _L, _I, _P],
    "cl_silu_fwd": [_I, _P, _P, _L, _P],
    "cl_silu_bwd": [_I, _P, _P, _P, _L, _P],
    "cl_axpby": [_I, _P, _L, _P, _L, _L, _I, _F, _F, _P],
    "cl_transpose": [_I, _I, _P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _P],
    "cl_nchw_to_tok": [_I, _P, _P, _L, _I, _I, _I, _I, _P],
    "cl_tok_to_nchw": [_I, _P, _L, _P, _I, _I, _I, _F, _F, _P],
    "cl_colsum": [_I, _P, _L, _P, _L, _I, _I, _I, _F, _P],
    "cl_pool2x2": [_I, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P],
    "cl_pack2d": [_I, _P, _L, _P, _L, _L, _I, _I, _P],
    "cl_vit_patch_rows": [_I, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "cl_vit_tokens": [_I, _P, _L, _P, _P, _P, _L, _I, _I, _I, _P],
    "cl_clip_text_embed": [_I, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "cl_gather_rows": [_I, _P, _L, _P, _P, _L, _I, _I, _I, _P],
    "cl_repack": [_I, _P, _P, _P, _I, _I, _P],
    "cl_timestep_embedding": [_I, _P, _P, _P, _L, _I, _I, _P],
    "cl_qsample": [_P, _P, _P, _P, _P, _P, _I, _L, _P],
    "cl_mse_loss": [_P, _P, _P, _P, _L, _F, _P],
    "cl_p_losses_mse": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _F, _F, _F, _P],
    "cl_p_losses_w": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _F, _F, _F, _P, _I, _F, _P],
    "cl_loss_bands": [_P, _P, _I, _I, _I, _P, _P, _P],
    "cl_zero": [_P, _L, _P],
    "cl_softmax_rows": [_I, _P, _L, _P, _L, _L, _I, _F, _P],
    "cl_conv_tap_gather": [_I, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "cl_ddim_step": [_P, _P, _P, _P, _P, _I, _F, _P, _P, _L, _P],
    "cl_tick": [_P, _P],
    "cl_adamw_dev": [_P, _P, _P, _P, _L, _P, _P, _P],
    "cl_ddim_set_t": [_P, _P, _I, _P, _I, _P],
    "cl_ddim_step_dev": [_P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _L, _P],
    "cl_adamw": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P],
    "cl_timestep_embedding_f": [_I, _P, _P, _P, _L, _I, _I, _P],
    "cl_dpmpp_step": [_P, _P, _P, _P, _I, _I, _F, _P, _P, _P, _L, _P],
    "cl_dpmpp_step_dev": [_P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _L, _P],
    "cl_dpm_set_t": [_P, _P, _I, _P, _I, _P],
    "cl_posterior_sample_pair": [_P, _P, _P, _P, _P, _P, _I, _L, _F, _P],
    "cl_plms_step": [_P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _L, _P],
    "cl_plms_step_dev": [_P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _L, _P],
    "cl_qsample_blend": [_P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _I, _I, _L, _P],
    "cl_grad_norm_scratch_floats": [_I],
    "cl_grad_norm": [_P, _P, _I, _P, _P, _P, _P, _P],
    "cl_adamw_dev_clip": [_P, _P, _P, _P, _L, _P, _P, _P, _P],
    "cl_ema_update": [_P, _P, _L, _P, _P, _P],
    "cl_swap": [_P, _P, _L, _P],
    "cl_adamw_dev_groups": [_P, _P, _P, _P, _L, _P, _I, _P, _P, _P, _P],
    "cl_lr_schedule": [_P, _I, _P, _I, _P, _P],
}
_LONG_RESULT = ("cl_groupnorm_ws_floats", "cl_grad_norm_scratch_floats")
EXPORTED = tuple(_SIGS.keys())
# probe hooks (ctrlora_amd/csrc/debug_hooks.h): exported by the library, not part of include/ctrlora_hip.h
_DEBUG_SIGS = {
    "cl_debug_attention_variant": [_I],
    "cl_debug_attention_fuse_delta": [_I],
    "cl_debug_attention_last_launch": [_P],
    "cl_debug_groupnorm_form": [_I, _I],
    "cl_debug_groupnorm_group": [_I],
    "cl_debug_norm_last_launch": [_P],
    "cl_debug_groupnorm_coop": [_I],
    "cl_debug_groupnorm_coop_timeouts": [],
    "cl_debug_gemm_tag": [_I],
    "cl_debug_gemm_xs_rules": [_I],
    "cl_debug_wgrad_ring": [_I],
    "cl_debug_wgrad_last_launch": [_P],
    "cl_debug_wgrad_last_problem": [_I, _P],
    "cl_debug_ew_last_launch": [_P],
    "cl_debug_gemm_tag_count": [],
    "cl_debug_gemm_tag_clear": [],
    "cl_debug_gemm_tag_get": [_I, _P],
    "cl_debug_gemm_config": [_I, _P],
}


def lib():
    """Load the shared library once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} not found -- run `python -m ctrlora_amd.build` "
                           "(the CtrLoRA engine has no non-HIP fallback)")
        L = C.CDLL(LIB_PATH)
        for name, args in {**_SIGS, **_DEBUG_SIGS}.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_long if name in _LONG_RESULT else C.c_int
        _lib = L
        if os.environ.get("CTRLORA_ATTN_FUSE_DELTA", "1") == "0":      # A/B switch: separate attn_delta launch
            L.cl_debug_attention_fuse_delta(0)
        gn3 = os.environ.get("CTRLORA_GN_THREE_PASS", "0") == "1"      # A/B switch: GroupNorm with the finalize launch
        gn1 = os.environ.get("CTRLORA_GN_ONE_PASS", "1") != "0"        # A/B switch: one-launch (register-resident) GroupNorm
        if gn3 or not gn1:
            L.cl_debug_groupnorm_form(int(gn3), int(gn1))
        if os.environ.get("CTRLORA_GN_GROUP", "1") == "0":             # A/B switch: one workgroup per (sample, group) GroupNorm (norm.hip gng_*)
            L.cl_debug_groupnorm_group(0)
        if os.environ.get("CTRLORA_GN_COOP", "0") == "1":              # A/B switch: cooperative one-pass GroupNorm (norm_coop.hip; off: no faster)
            L.cl_debug_groupnorm_coop(1)
        L.cl_debug_gemm_xs_rules(int(XS_ENABLED))
        if os.environ.get("CTRLORA_WGRAD_RING"):                     # A/B switch: 4 = the round-1..4 ring depth
            L.cl_debug_wgrad_ring(int(os.environ["CTRLORA_WGRAD_RING"]))
        if os.environ.get("CTRLORA_GEMM_TUNED", "1") != "0":
            load_gemm_table(os.environ.get("CTRLORA_GEMM_TABLE", GEMM_TABLE_PATH))
            # overlays of the built-in table only: a table the user names is taken as it is
            if "CTRLORA_GEMM_TABLE" not in os.environ:
                if XS_ENABLED:  # round 5: signatures the x-stationary kernel (csrc/gemm_xs.hip, configuration 34) won
                    load_gemm_table(GEMM_XS_TABLE_PATH, clear=False)
                if R06_ENABLED and os.path.exists(GEMM_R06_TABLE_PATH):   # round 6: the loader / consumer kernel (csrc/gemm_w4.hip,
                    load_gemm_table(GEMM_R06_TABLE_PATH, clear=False)     # 40 / 41) and the deep-ring small tiles (42 .. 46)
    return _lib


GEMM_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuned_gfx950.json")
GEMM_XS_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuned_gfx950_xs.json")
GEMM_R06_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuned_gfx950_r06.json")
# A/B switch: 0 = the round-6 overlay (configurations 40 .. 46) is not loaded
R06_ENABLED = os.environ.get("CTRLORA_GEMM_R06", "1") != "0"
# A/B switch: 0 = no product goes to the x-stationary streaming kernel (neither through the launch table nor as the fused
# GEGLU projection of the no-grad forwards)
XS_ENABLED = os.environ.get("CTRLORA_GEMM_XS", "1") != "0"


# A/B switch: 0 = every LayerNorm stays its own launch
LN_PROLOGUE = os.environ.get("CTRLORA_LN_PROLOGUE", "1") != "0"


def xs_ln_ok(M: int, N: int, K: int, act: int = 0) -> bool:
    """Can LayerNorm(x) . W^T run as ONE launch (LayerNorm as the x-stationary kernel's prologue, csrc/gemm_xs.hip)?  The
    kernel's own preconditions: bf16 (the caller checks the dtype), K in {320, 640} with no second K segment, whole 32-column
    output blocks, a GEGLU product only where xs_geglu_ok() sends it to this kernel anyway."""
    if not (XS_ENABLED and LN_PROLOGUE) or K not in (320, 640) or M < 128:
        return False
    if act == ACT_GEGLU_SPLIT:
        return N % 64 == 0 and xs_geglu_ok(M, K, 0)
    return act == ACT_NONE and N % 32 == 0


def gemm_tags():
    """Launch-tag table of the contraction kernels (csrc/debug_hooks.h: cl_debug_gemm_tag; tools/prof_shapes.py)."""
    L = lib()
    out = []
    buf = (C.c_long * 12)()
    for i in range(int(L.cl_debug_gemm_tag_count())):
        _chk(L.cl_debug_gemm_tag_get(i, C.cast(buf, C.c_void_p)), "cl_debug_gemm_tag_get")
        v = list(buf)
        out.append(dict(dtype=v[0], mode=v[1], M=v[2], N=v[3], K1=v[4], K2=v[5], act=v[6], residual=v[7], tag=v[8],
                        workgroups=v[9], wg_size=v[10], launches=v[11]))
    return out


def xs_geglu_ok(M: int, K: int, r: int) -> bool:
    """Does the fused GEGLU projection of a no-grad forward go to the x-stationary kernel (act = ACT_GEGLU_SPLIT, natural row
    order)?  Measured against the tile kernels' fused GEGLU (profiles/r05_gemm_xs/probe_xs_fast_gelu.log): K = 320 at every M
    (73 vs 102 us at 32768 rows, 280 vs 450 at 131072), K = 640 from 8192 rows (253 vs 324 us at 32768; 71 vs 78 at 8192)."""
    if not XS_ENABLED or r not in (0, 128):
        return False
    return (K == 320 and M >= 128) or (K == 640 and M >= 8192)


def load_gemm_table(path: str, clear: bool = True) -> int:
    """Register the measured launch table (tools/gemm_autotune.py) with the library: rows
    [dtype, mode, M, N, K1, K2, geglu, cfg, splitk].  A missing file leaves the built-in rules in charge
    (CTRLORA_GEMM_TUNED=0 does the same on purpose, for A/B runs).  Returns the number of entries."""
    import json
    L = lib()
    if clear:
        L.cl_gemm_tune_clear()
    if not path or not os.path.exists(path):
        return 0
    with open(path) as f:
        tab = json.load(f)
    for row in tab.get("entries", []):
        _chk(L.cl_gemm_tune_set(*[int(v) for v in row[:9]]), "cl_gemm_tune_set")
    return int(L.cl_gemm_tune_size())


def _chk(rc: int, what: str):
    if rc != 0:
        detail = "unsupported shape/alignment"
        if rc != 1:
            L = lib()
            L.cl_last_hip_error_string.restype = C.c_char_p
            detail = f"HIP launch error {L.cl_last_hip_error()}: {L.cl_last_hip_error_string().decode()}"
        raise HipError(f"{what} failed with code {rc} ({detail})")


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise HipError(f"unsupported dtype {t.dtype}")


def dt_of(dtype: torch.dtype) -> int:
    return BF16 if dtype == torch.bfloat16 else F32


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def ld(t: Optional[torch.Tensor]) -> int:
    """Row stride (elements) of a 2-D view whose last dim is contiguous."""
    if t is None:
        return 0
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.stride(0)


ZERO_PAGE_BYTES = 16384   # conv halo source: >= 4 * Cin bytes (include/ctrlora_hip.h), 16 KiB covers Cin <= 4096
_zero_pages = {}
_workspace = None
WORKSPACE_BYTES = 64 << 20


_stream_ws = {}


def bind_stream_workspace(stream: "torch.cuda.Stream", nbytes: int = 32 << 20) -> None:
    """Give `stream` its own split-K scratch (needed before running contractions on it concurrently with
    another stream)."""
    key = stream.cuda_stream
    if key not in _stream_ws:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=stream.device)
        _chk(lib().cl_set_stream_workspace(key, buf.data_ptr(), nbytes), "cl_set_stream_workspace")
        _stream_ws[key] = buf


_side_streams = {}


def side_stream(device) -> "torch.cuda.Stream":
    """The process-wide second compute stream of a device (with its own split-K scratch)."""
    key = str(device)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        bind_stream_workspace(st)
        _side_streams[key] = st
    return st


def ensure_workspace(device) -> None:
    """Register the split-K scratch (fp32 partial slabs) with the library once per process."""
    global _workspace
    if _workspace is None:
        _workspace = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        _chk(lib().cl_set_workspace(_workspace.data_ptr(), WORKSPACE_BYTES), "cl_set_workspace")


def zero_page(device) -> torch.Tensor:
    k = str(device)
    if k not in _zero_pages:
        _zero_pages[k] = torch.zeros(ZERO_PAGE_BYTES, dtype=torch.uint8, device=device)
    return _zero_pages[k]


# ------------------------------------------------------------------ dense contractions

def gemm(a1, w1, out, *, a2=None, w2=None, bias=None, rowbias=None, rows_per_batch=0, residual=None,
         alpha=1.0, beta=0.0, act=ACT_NONE, mode=LINEAR, conv=None, k1=None, out_f32=False, atomic=False,
         splitk=1, M=None, N=None, dtype=None, a1_group_n=0, a2_group_n=0, alpha_n=0, ln=None):
    """out[M,N] = act(a1.w1^T + a2.w2^T + bias + rowbias[m // rows_per_batch]) * alpha + beta * residual.

    a1: [M,K1] (LINEAR) or the NHWC activation [B*Hin*Win, C] (conv modes, conv=(B,Hin,Win,Hout,Wout)).
    ln = (gamma, beta, eps, stats or None): LayerNorm of a1's rows as a prologue of the product (xs_ln_ok() says when).
    """
    p = GemmParams()
    if _workspace is None:
        ensure_workspace(a1.device)
    dty = dt(a1) if dtype is None else dtype
    p.A1 = a1.data_ptr(); p.lda1 = ld(a1); p.K1 = a1.shape[1] if k1 is None else k1
    p.W1 = w1.data_ptr(); p.ldw1 = ld(w1)
    if a2 is not None:
        p.A2 = a2.data_ptr(); p.lda2 = ld(a2); p.W2 = w2.data_ptr(); p.ldw2 = ld(w2)
        p.K2 = w2.shape[1] if a2_group_n else a2.shape[1]        # grouped: a2 holds one K2-wide block per output group
    p.M = out.shape[0] if M is None else M
    p.N = out.shape[1] if N is None else N
    p.mode = mode
    if conv is not None:
        p.B, p.Hin, p.Win, p.Hout, p.Wout = conv
        p.zero_page = zero_page(a1.device).data_ptr()
    p.bias = ptr(bias)
    if rowbias is not None:
        p.rowbias = rowbias.data_ptr(); p.ldrb = ld(rowbias); p.rows_per_batch = rows_per_batch
    if residual is not None:
        p.residual = residual.data_ptr(); p.ldr = ld(residual)
    p.alpha = alpha; p.beta = beta; p.act = act
    p.C = out.data_ptr(); p.ldc = ld(out)
    p.out_f32 = int(out_f32); p.atomic = int(atomic); p.splitk = splitk
    p.a1_group_n = a1_group_n; p.a2_group_n = a2_group_n; p.alpha_n = alpha_n
    if ln is not None:
        p.ln_gamma = ln[0].data_ptr(); p.ln_beta = ln[1].data_ptr(); p.ln_eps = ln[2]; p.ln_stats = ptr(ln[3])
    _chk(lib().cl_gemm(C.byref(p), dty, stream()), "cl_gemm")
    return out


# Opt-in (CTRLORA_WGRAD_F32_DETERMINISTIC=1; off by default, and then nothing below changes): the weight gradients of the fp32
# parity mode as a pure function of their operands.  cl_weight_grad splits K and accumulates with fp32 atomics, so the last bits of
# an fp32 step's gradients depend on the order in which the workgroups arrive; with the switch on, the same product goes through
# cl_gemm with dW as its own residual (dW = scale * product + dW), where the launcher splits K through the workspace and sums the
# slabs in a fixed order.  Another launch form and another summation order than the default's: for comparisons that need bits.
WGRAD_F32_DETERMINISTIC = os.environ.get("CTRLORA_WGRAD_F32_DETERMINISTIC", "0") == "1"


def weight_grad(dyT, xT, dW, scale=1.0):
    """dW[N,K] (fp32) += scale * dyT[N,Mp] . xT[K,Mp]^T  (split-K, fp32 atomics)."""
    if WGRAD_F32_DETERMINISTIC and dyT.dtype == torch.float32:
        # the epilogue reads and writes dW eight columns (two 16-byte vectors) at a time
        if dW.data_ptr() % 16 or ld(dW) % 8 or dW.shape[1] % 8:
            raise HipError(f"deterministic fp32 weight gradient: dW must be 16-byte aligned with a row stride and a width that are "
                           f"multiples of 8 (got offset {dW.data_ptr() % 16}, ld {ld(dW)}, width {dW.shape[1]})")
        gemm(dyT, xT, dW, residual=dW, alpha=scale, beta=1.0, out_f32=True)
        return
    _chk(lib().cl_weight_grad(dt(dyT), dyT.data_ptr(), ld(dyT), xT.data_ptr(), ld(xT), dW.data_ptr(), ld(dW),
                              dyT.shape[0], xT.shape[0], dyT.shape[1], scale, stream()), "cl_weight_grad")


def weight_grad_tn_group(problems):
    """problems: list of (dy [M,N] bf16, x [M,K] bf16, dW [N,K] fp32, scale[, conv]): ONE launch for all of them.
    conv = (tap, Hin, Win, Hout, Wout, stride, pad): one tap of a 3x3 conv's weight gradient (x = NHWC input)."""
    n = len(problems)
    if n == 0:
        return
    if _workspace is None:
        ensure_workspace(problems[0][0].device)
    arr = (WgradDesc * n)()
    for d, prob in zip(arr, problems):
        dy, x, dW, scale = prob[:4]
        d.dy = dy.data_ptr(); d.lddy = ld(dy); d.x = x.data_ptr(); d.ldx = ld(x)
        d.dW = dW.data_ptr(); d.lddw = ld(dW); d.M = dy.shape[0]; d.N = dy.shape[1]; d.K = x.shape[1]
        d.scale = scale
        d.tap = -1
        if len(prob) > 4 and prob[4] is not None:
            d.tap, d.Hin, d.Win, d.Hout, d.Wout, d.stride, d.pad = prob[4]
    _chk(lib().cl_weight_grad_tn_group(BF16, n, C.cast(arr, C.c_void_p), zero_page(problems[0][0].device).data_ptr(),
                                       stream()), "cl_weight_grad_tn_group")


def repack(dtype, flat, desc, tile_prefix, ndesc, total_tiles):
    _chk(lib().cl_repack(dt_of(dtype), flat.data_ptr(), desc.data_ptr(), tile_prefix.data_ptr(), ndesc, total_tiles,
                         stream()), "cl_repack")


def weight_grad_tn(dy, x, dW, scale=1.0):
    """dW[N,K] (fp32) += scale * dy[M,N]^T . x[M,K], bf16 operands as they are (no transposes)."""
    if _workspace is None:
        ensure_workspace(dy.device)
    _chk(lib().cl_weight_grad_tn(dt(dy), dy.data_ptr(), ld(dy), x.data_ptr(), ld(x), dW.data_ptr(), ld(dW),
                                 dy.shape[0], dy.shape[1], x.shape[1], scale, zero_page(dy.device).data_ptr(),
                                 stream()), "cl_weight_grad_tn")


# ------------------------------------------------------------------ normalisation

def groupnorm_ws(B, HW, C_) -> int:
    return int(lib().cl_groupnorm_ws_floats(B, HW, C_))


def groupnorm_fwd(x, y, gamma, beta, B, HW, eps, silu, stats, ws, groups=32):
    _chk(lib().cl_groupnorm_silu_fwd(dt(x), x.data_ptr(), ld(x), y.data_ptr(), ld(y), gamma.data_ptr(),
                                     beta.data_ptr(), B, HW, x.shape[1], groups, eps, int(silu), stats.data_ptr(),
                                     ws.data_ptr(), stream()), "cl_groupnorm_silu_fwd")
    return y


def groupnorm_bwd(x, dy, dx, gamma, beta, stats, B, HW, silu, ws, accum=None, dgamma=None, dbeta=None, groups=32):
    _chk(lib().cl_groupnorm_silu_bwd(dt(x), x.data_ptr(), ld(x), dy.data_ptr(), ld(dy), ptr(accum), ld(accum),
                                     dx.data_ptr(), ld(dx), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(), B, HW,
                                     x.shape[1], groups, int(silu), ptr(dgamma), ptr(dbeta), ws.data_ptr(), stream()),
         "cl_groupnorm_silu_bwd")
    return dx


def layernorm_fwd(x, y, gamma, beta, eps=1e-5, stats=None):
    _chk(lib().cl_layernorm_fwd(dt(x), x.data_ptr(), ld(x), y.data_ptr(), ld(y), gamma.data_ptr(), beta.data_ptr(),
                                x.shape[0], x.shape[1], eps, ptr(stats), stream()), "cl_layernorm_fwd")
    return y


def layernorm_bwd(x, dy, dx, gamma, stats, accum=None, dgamma=None, dbeta=None):
    _chk(lib().cl_layernorm_bwd(dt(x), x.data_ptr(), ld(x), dy.data_ptr(), ld(dy), ptr(accum), ld(accum),
                                dx.data_ptr(), ld(dx), gamma.data_ptr(), stats.data_ptr(), x.shape[0], x.shape[1],
                                ptr(dgamma), ptr(dbeta), stream()), "cl_layernorm_bwd")
    return dx


# ------------------------------------------------------------------ attention

def attention_fwd(q, k, vt, o, lse, B, H, N, Nkv, dh, scale):
    """q [B*N, >=H*dh], k [B*Nkv, ..], vt [B, H*dh, nkv_pad], o [B*N, H*dh], lse [B,H,lse_stride] or None."""
    _chk(lib().cl_attention_fwd(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), vt.data_ptr(), vt.shape[-1],
                                o.data_ptr(), ld(o), ptr(lse), 0 if lse is None else lse.shape[-1], B, H, N, Nkv, dh,
                                scale, stream()), "cl_attention_fwd")
    return o


def attention_bwd(q, k, v, o, do, qt, dot, kt, lse, delta, dq, dk, dv, B, H, N, Nkv, dh, scale):
    _chk(lib().cl_attention_bwd(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), v.data_ptr(), ld(v), o.data_ptr(),
                                ld(o), do.data_ptr(), ld(do), qt.data_ptr(), dot.data_ptr(), qt.shape[-1],
                                kt.data_ptr(), kt.shape[-1], lse.data_ptr(), delta.data_ptr(), lse.shape[-1],
                                dq.data_ptr(), ld(dq), ptr(dk), ld(dk), ptr(dv), ld(dv), B, H, N, Nkv, dh, scale,
                                stream()), "cl_attention_bwd")


ATTN_Q_PRESCALED = 1


def attention_fwd_v2(q, k, v, o, lse, B, H, N, Nkv, dh, scale, q_prescaled=False):
    """bf16, transpose-free: v is [B*Nkv, >=H*dh] like k.  q_prescaled: q holds q * scale * log2(e)
    (CL_ATTN_Q_PRESCALED: the to_q projection applied the factor in its epilogue)."""
    _chk(lib().cl_attention_fwd_v2(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), v.data_ptr(), ld(v), o.data_ptr(),
                                   ld(o), ptr(lse), 0 if lse is None else lse.shape[-1], B, H, N, Nkv, dh, scale,
                                   ATTN_Q_PRESCALED if q_prescaled else 0, stream()), "cl_attention_fwd_v2")
    return o


def attention_fwd_ip(q, k, v, k_ip, v_ip, o, B, H, N, Nkv, Nip, dh, scale, ip_scale, q_prescaled=False):
    """o = softmax(scale q k^T) v + ip_scale * softmax(scale q k_ip^T) v_ip per head, one launch (cl_attention_fwd_ip).
    k_ip [B*Nip, >=H*dh] (one image prompt per sample, Nip <= 64).  bf16: v / v_ip row-major like k; fp32: v / v_ip
    transposed [B, H*dh, pad64] (as attention_fwd)."""
    if dt(q) == BF16:
        lv, lvi = ld(v), ld(v_ip)
    else:
        lv, lvi = v.shape[-1], v_ip.shape[-1]
    _chk(lib().cl_attention_fwd_ip(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), v.data_ptr(), lv, k_ip.data_ptr(),
                                   ld(k_ip), v_ip.data_ptr(), lvi, o.data_ptr(), ld(o), B, H, N, Nkv, Nip, dh, scale,
                                   ip_scale, ATTN_Q_PRESCALED if q_prescaled else 0, stream()), "cl_attention_fwd_ip")
    return o


def attention_bwd_v2(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, N, Nkv, dh, scale, q_prescaled=False, row_ws=None):
    """row_ws: optional uint8 / any tensor of >= B * H * lse.shape[-1] * 32 bytes (see cl_attention_bwd_v2)."""
    assert row_ws is None or row_ws.numel() * row_ws.element_size() >= B * H * lse.shape[-1] * 32
    _chk(lib().cl_attention_bwd_v2(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), v.data_ptr(), ld(v), o.data_ptr(),
                                   ld(o), do.data_ptr(), ld(do), lse.data_ptr(), delta.data_ptr(), lse.shape[-1],
                                   dq.data_ptr(), ld(dq), ptr(dk), ld(dk), ptr(dv), ld(dv), B, H, N, Nkv, dh, scale,
                                   ATTN_Q_PRESCALED if q_prescaled else 0, ptr(row_ws), stream()), "cl_attention_bwd_v2")


# The two kernel families behind one forward and one backward.  Which one runs is a function of the dtype alone: bf16 takes the
# transpose-free kernels (_v2, the bf16 _ip), fp32 -- the parity mode -- the kernels that read materialised transposes
# [B, H*dh, rows padded with zeros to whole 64-wide tiles].  The engine calls these two and never builds such a scratch itself.

def _transposed(x, B, rows, inner, pad, out=None):
    """x [B*rows, >=inner] row-major -> [B, inner, pad] zero padded (scratch of the call unless the caller passes `out`)."""
    if out is None:
        out = torch.empty((B, inner, pad), dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (B, inner, pad) and out.dtype == x.dtype
    return transpose(x, out, B, rows, inner, pad, ldi=x.stride(0))


def attention(q, k, v, o, lse, B, H, N, Nkv, dh, scale, *, q_prescaled=False, ip=None, vt=None):
    """o = softmax(scale q k^T) v per head; q [B*N, >=H*dh], k and v [B*Nkv, >=H*dh] row-major, lse [B, H, stride] or None.
    ip = (k_ip, v_ip, Nip, ip_scale), v_ip row-major like k_ip: + ip_scale * softmax(scale q k_ip^T) v_ip in the same launch
    (attention_fwd_ip; forward only).  vt: the fp32 family's V^T scratch [B, H*dh, rup(Nkv, 64)] for a caller that replays
    fixed addresses; allocated here, and released on return, otherwise."""
    assert ip is None or lse is None
    if dt(q) == BF16:
        if ip is None:
            return attention_fwd_v2(q, k, v, o, lse, B, H, N, Nkv, dh, scale, q_prescaled=q_prescaled)
        k_ip, v_ip, Nip, ip_scale = ip
        return attention_fwd_ip(q, k, v, k_ip, v_ip, o, B, H, N, Nkv, Nip, dh, scale, ip_scale, q_prescaled=q_prescaled)
    assert not q_prescaled, "the fp32 kernels scale the scores themselves"
    vt = _transposed(v, B, Nkv, H * dh, (Nkv + 63) // 64 * 64, vt)
    if ip is None:
        return attention_fwd(q, k, vt, o, lse, B, H, N, Nkv, dh, scale)
    k_ip, v_ip, Nip, ip_scale = ip
    vt_ip = _transposed(v_ip, B, Nip, H * dh, 64)          # Nip <= 64: one masked tile
    return attention_fwd_ip(q, k, vt, k_ip, vt_ip, o, B, H, N, Nkv, Nip, dh, scale, ip_scale)


def attention_causal(q, k, v, o, B, H, N, dh, scale):
    """o[b, i] = softmax_{j <= i}(scale q_i k_j) v_j per head: causal self-attention, q / k / v / o [B*N, >= H*dh] row-major, d_head 64,
    N <= 128, bf16 or fp32 (cl_attention_causal_fwd, csrc/attention_causal.hip)."""
    assert dt(q) == dt(k) == dt(v) == dt(o)
    _chk(lib().cl_attention_causal_fwd(dt(q), q.data_ptr(), ld(q), k.data_ptr(), ld(k), v.data_ptr(), ld(v), o.data_ptr(), ld(o),
                                       B, H, N, dh, float(scale), stream()), "cl_attention_causal_fwd")
    return o


def attention_backward(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, N, Nkv, dh, scale, *, q_prescaled=False):
    """dq, dk, dv (dk / dv may be None) of attention(); lse as the forward wrote it, delta a scratch of lse's shape."""
    if dt(q) == BF16:
        # (-lse, -delta) of every query row as bf16 triples: lets the d_head-40 kernels fold them into their products
        row_ws = torch.empty(lse.numel() * 8, dtype=torch.float32, device=q.device) if (q_prescaled and dh == 40) else None
        return attention_bwd_v2(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, N, Nkv, dh, scale, q_prescaled=q_prescaled,
                                row_ws=row_ws)
    assert not q_prescaled, "the fp32 kernels scale the scores themselves"
    inner, npad, kpad = H * dh, (N + 63) // 64 * 64, (Nkv + 63) // 64 * 64
    qt = _transposed(q, B, N, inner, npad)
    dot = _transposed(do, B, N, inner, npad)
    kt = _transposed(k, B, Nkv, inner, kpad)
    attention_bwd(q, k, v, o, do, qt, dot, kt, lse, delta, dq, dk, dv, B, H, N, Nkv, dh, scale)


# ------------------------------------------------------------------ elementwise / layout

def geglu_fwd(h, out):
    _chk(lib().cl_geglu_fwd(dt(h), h.data_ptr(), ld(h), out.data_ptr(), ld(out), h.shape[0], out.shape[1], stream()),
         "cl_geglu_fwd")
    return out


def geglu_bwd(h, dout, dh):
    _chk(lib().cl_geglu_bwd(dt(h), h.data_ptr(), ld(h), dout.data_ptr(), ld(dout), dh.data_ptr(), ld(dh), h.shape[0],
                            dout.shape[1], stream()), "cl_geglu_bwd")
    return dh


def silu_fwd(x, y):
    _chk(lib().cl_silu_fwd(dt(x), x.data_ptr(), y.data_ptr(), x.numel(), stream()), "cl_silu_fwd")
    return y


def silu_bwd(x, dy, dx):
    _chk(lib().cl_silu_bwd(dt(x), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), stream()), "cl_silu_bwd")
    return dx


def axpby(x, y, a=1.0, b=1.0):
    """y = a*x + b*y over 2-D strided views."""
    _chk(lib().cl_axpby(dt(x), x.data_ptr(), ld(x), y.data_ptr(), ld(y), x.shape[0], x.shape[1], a, b, stream()),
         "cl_axpby")
    return y


def transpose(src, dst, Bt, R, C_, Rpad, ldi=None, bsi=None):
    """src [Bt][R][C] (row stride ldi, batch stride bsi) -> dst [Bt][C][Rpad] (zero padded)."""
    ldi = src.stride(-2) if ldi is None else ldi
    bsi = R * ldi if bsi is None else bsi
    _chk(lib().cl_transpose(dt(src), dt(dst), src.data_ptr(), ldi, bsi, dst.data_ptr(), Rpad, C_ * Rpad, Bt, R, C_,
                            Rpad, stream()), "cl_transpose")
    return dst


def nchw_to_tok(x_nchw, out, Cpad=None):
    B, Cin, H, W = x_nchw.shape
    x_nchw = x_nchw.contiguous()
    _chk(lib().cl_nchw_to_tok(dt(out), x_nchw.data_ptr(), out.data_ptr(), ld(out), B, Cin,
                              out.shape[1] if Cpad is None else Cpad, H * W, stream()), "cl_nchw_to_tok")
    return out


def tok_to_nchw(tok, out_nchw, alpha=1.0, beta=0.0):
    B, C_, H, W = out_nchw.shape
    _chk(lib().cl_tok_to_nchw(dt(tok), tok.data_ptr(), ld(tok), out_nchw.data_ptr(), B, C_, H * W, alpha, beta,
                              stream()), "cl_tok_to_nchw")
    return out_nchw


def colsum(x, out_f32, B, HW, scale=1.0):
    _chk(lib().cl_colsum(dt(x), x.data_ptr(), ld(x), out_f32.data_ptr(), ld(out_f32), B, HW, x.shape[1], scale,
                         stream()), "cl_colsum")
    return out_f32


def pool2x2(src, dst, B, H, W, accumulate=False):
    _chk(lib().cl_pool2x2(dt(src), src.data_ptr(), ld(src), dst.data_ptr(), ld(dst), B, H, W, dst.shape[1],
                          int(accumulate), stream()), "cl_pool2x2")
    return dst


def pack2d(src_f32, dst, Cpad=None):
    """fp32 [R, C] (strided) -> dst dtype [R, Cpad] with zero-filled pad columns."""
    R, C_ = src_f32.shape
    _chk(lib().cl_pack2d(dt(dst), src_f32.data_ptr(), ld(src_f32), dst.data_ptr(), ld(dst), R, C_,
                         dst.shape[1] if Cpad is None else Cpad, stream()), "cl_pack2d")
    return dst


def vit_patch_rows(pixels, out, P):
    """NCHW fp32 pixels [B, C, S, S] -> patch rows out [B (S/P)^2, Kpad] (columns (c, py, px), zero pad): cl_vit_patch_rows."""
    B, C_, S, S2 = pixels.shape
    assert S == S2 and pixels.dtype == torch.float32 and pixels.is_contiguous() and out.shape[0] == B * (S // P) ** 2
    _chk(lib().cl_vit_patch_rows(dt(out), pixels.data_ptr(), out.data_ptr(), ld(out), B, C_, S, P, out.shape[1], stream()),
         "cl_vit_patch_rows")
    return out


def clip_text_embed(ids, tok, pos, out):
    """out[b T + t] = tok[ids[b, t]] + pos[t] (ids [B, T] int64, tok [vocab, D] / pos [>= T, D] fp32): cl_clip_text_embed.  The
    kernel clamps an id outside [0, vocab); ids that come from the host are checked here, where that costs no sync."""
    B, T = ids.shape
    vocab, D = tok.shape
    assert ids.dtype == torch.long and ids.is_contiguous() and tok.is_contiguous() and pos.is_contiguous()
    assert out.shape == (B * T, D) and pos.shape[0] >= T and pos.shape[1] == D and tok.dtype == pos.dtype == torch.float32
    if not ids.is_cuda:
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
            raise HipError(f"cl_clip_text_embed: token id outside [0, {vocab})")
        ids = ids.to(out.device)
    _chk(lib().cl_clip_text_embed(dt(out), ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), ld(out), B, T, D, vocab,
                                  stream()), "cl_clip_text_embed")
    return out


def gather_rows(src, rows, dst):
    """dst[r] = src[rows[r]] (rows int64 on the device, clamped to src's rows): cl_gather_rows."""
    R, D = dst.shape
    assert rows.dtype == torch.long and rows.is_cuda and rows.is_contiguous() and rows.numel() == R and src.shape[1] == D
    assert src.dtype == dst.dtype
    _chk(lib().cl_gather_rows(dt(dst), src.data_ptr(), ld(src), rows.data_ptr(), dst.data_ptr(), ld(dst), R, D, src.shape[0], stream()),
         "cl_gather_rows")
    return dst


def vit_tokens(patch, cls, pos, out, B):
    """out[b, 0] = cls + pos[0]; out[b, 1 + i] = patch[b (T - 1) + i] + pos[1 + i] (cls [D], pos [T, D] fp32): cl_vit_tokens."""
    T, D = pos.shape
    assert out.shape == (B * T, D) and patch.shape == (B * (T - 1), D) and cls.is_contiguous() and pos.is_contiguous()
    _chk(lib().cl_vit_tokens(dt(out), patch.data_ptr(), ld(patch), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), ld(out), B, T, D,
                             stream()), "cl_vit_tokens")
    return out


def timestep_embedding(t_long, freqs, out):
    _chk(lib().cl_timestep_embedding(dt(out), t_long.data_ptr(), freqs.data_ptr(), out.data_ptr(), ld(out),
                                     t_long.shape[0], freqs.shape[0], stream()), "cl_timestep_embedding")
    return out


def timestep_embedding_f(t_f32, freqs, out):
    """timestep_embedding at floating-point times (t fp32, contiguous): cl_timestep_embedding_f."""
    assert t_f32.dtype == torch.float32 and t_f32.is_contiguous()
    _chk(lib().cl_timestep_embedding_f(dt(out), t_f32.data_ptr(), freqs.data_ptr(), out.data_ptr(), ld(out),
                                       t_f32.shape[0], freqs.shape[0], stream()), "cl_timestep_embedding_f")
    return out


def qsample(z, noise, t, sqrt_ac, sqrt_1mac, out):
    B = z.shape[0]
    _chk(lib().cl_qsample(z.data_ptr(), noise.data_ptr(), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(),
                          out.data_ptr(), B, z.numel() // B, stream()), "cl_qsample")
    return out


def qsample_blend(x0, noise, t, sqrt_ac, sqrt_1mac, mask, x, out):
    """out = q_sample(x0, t) * mask + (1 - mask) * x in one launch (cl_qsample_blend): x0 / noise / x / out [B, C, H, W], mask
    [B | 1, C | 1, H, W], t [B] long, the tables [T]; fp32 except t, contiguous.  out may be x.  Bit-identical to qsample()
    followed by the three torch fp32 ops."""
    B, Cn = x0.shape[0], x0.shape[1]
    hw = tuple(x0.shape[2:])
    if mask.dim() != x0.dim() or tuple(mask.shape[2:]) != hw or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, Cn):
        raise ValueError(f"mask {tuple(mask.shape)} is none of the layouts (B | 1, C | 1, H, W) of a sample {tuple(x0.shape)}")
    for v in (x0, noise, sqrt_ac, sqrt_1mac, mask, x, out):
        assert v.dtype == torch.float32 and v.is_contiguous()
    assert t.dtype == torch.long and t.is_contiguous() and t.numel() == B
    assert noise.shape == x0.shape == x.shape == out.shape and sqrt_ac.numel() == sqrt_1mac.numel()
    HW = 1
    for d in hw:
        HW *= int(d)
    # a dimension of size 1 is broadcast (with B == 1 or C == 1 both readings address the same plane)
    _chk(lib().cl_qsample_blend(x0.data_ptr(), noise.data_ptr(), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(),
                                sqrt_ac.numel(), mask.data_ptr(), int(mask.shape[0] != 1), int(mask.shape[1] != 1),
                                x.data_ptr(), out.data_ptr(), B, Cn, HW, stream()), "cl_qsample_blend")
    return out


def posterior_sample_pair(mom_a, e_a, out_a, scale, mom_b=None, e_b=None, out_b=None):
    """out = scale * (mean + std * e) for one posterior, or two of the same shape, in one launch (fp32, contiguous):
    mom = [B, 2C, h, w] (mean | std), e / out = [B, C, h, w].  Bit-identical to the three torch fp32 ops."""
    ts = [t for t in (mom_a, e_a, out_a, mom_b, e_b, out_b) if t is not None]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in ts)
    B = e_a.shape[0]
    per = e_a.numel() // B if B else 0          # an empty batch is the kernel's refusal (B < 1), not a division here
    assert mom_a.numel() == 2 * e_a.numel() == 2 * out_a.numel()
    assert mom_b is None or (mom_b.numel() == mom_a.numel() and e_b.numel() == e_a.numel() and out_b.numel() == out_a.numel())
    _chk(lib().cl_posterior_sample_pair(mom_a.data_ptr(), e_a.data_ptr(), out_a.data_ptr(), ptr(mom_b), ptr(e_b), ptr(out_b),
                                        B, per, float(scale), stream()), "cl_posterior_sample_pair")
    return out_a, out_b


def mse_loss(eps, target, d_eps, loss, gscale=1.0):
    _chk(lib().cl_mse_loss(eps.data_ptr(), target.data_ptr(), ptr(d_eps), loss.data_ptr(), eps.numel(), gscale,
                           stream()), "cl_mse_loss")
    return loss


def p_losses_mse(eps, target, d_eps, t, lvlb, out3, scratch, gscale=1.0, w_simple=1.0, w_elbo=0.0, per_sample=None):
    """Deterministic p_losses reduction: out3 = {loss_simple, loss_vlb, loss}; d_eps = d(w_simple*loss_simple)/d eps."""
    B = eps.shape[0]
    assert scratch.numel() >= 16 * B and eps.is_contiguous() and target.is_contiguous()
    _chk(lib().cl_p_losses_mse(eps.data_ptr(), target.data_ptr(), ptr(d_eps), ptr(t), ptr(lvlb), out3.data_ptr(),
                               ptr(per_sample), scratch.data_ptr(), B, eps.numel() // B, gscale, w_simple, w_elbo,
                               stream()), "cl_p_losses_mse")
    return out3


LOSS_KINDS = {"l2": 0, "huber": 1}


def p_losses_w(eps, target, d_eps, t, lvlb, out3, scratch, gscale=1.0, w_simple=1.0, w_elbo=0.0, per_sample=None, wt=None,
               kind=0, delta=1.0):
    """p_losses_mse with a per-timestep weight table `wt` (fp32 [T], indexed by t; None = all ones) and kind 0 = l2 / 1 = Huber
    with `delta`: out3[0] and out3[1] stay unweighted, out3[2] and d_eps carry wt[t_b] (include/ctrlora_hip.h: cl_p_losses_w)."""
    B = eps.shape[0]
    assert scratch.numel() >= 16 * B and eps.is_contiguous() and target.is_contiguous()
    assert wt is None or (wt.dtype == torch.float32 and wt.is_contiguous() and wt.device == eps.device)
    _chk(lib().cl_p_losses_w(eps.data_ptr(), target.data_ptr(), ptr(d_eps), ptr(t), ptr(lvlb), out3.data_ptr(), ptr(per_sample),
                             scratch.data_ptr(), B, eps.numel() // B, gscale, w_simple, w_elbo, ptr(wt), int(kind), float(delta),
                             stream()), "cl_p_losses_w")
    return out3


def loss_bands(per_sample, t, T, nbands, acc, n_valid=None):
    """acc (fp64 [nbands + 1][3]: count, sum, sum of squares per timestep band, last row = all) += the fp32 per-sample losses at
    timesteps t (int64); n_valid: None or a device int32, the first clamp(n_valid, 0, B) samples count (cl_loss_bands)."""
    B = per_sample.numel()
    assert per_sample.dtype == torch.float32 and per_sample.is_contiguous() and t.dtype == torch.int64 and t.is_contiguous()
    assert t.numel() == B and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == 3 * (nbands + 1)
    assert n_valid is None or (n_valid.dtype == torch.int32 and n_valid.numel() == 1)
    _chk(lib().cl_loss_bands(per_sample.data_ptr(), t.data_ptr(), B, int(T), int(nbands), ptr(n_valid), acc.data_ptr(), stream()),
         "cl_loss_bands")
    return acc


def conv_tap_gather(x, out, B, Hin, Win, Hout, Wout, tap, stride, pad):
    _chk(lib().cl_conv_tap_gather(dt(x), x.data_ptr(), ld(x), out.data_ptr(), ld(out), B, Hin, Win, Hout, Wout, x.shape[1], tap,
                                  stride, pad, stream()), "cl_conv_tap_gather")
    return out


def softmax_rows(scores_f32, probs, scale=1.0):
    """probs[M,N] (engine dtype) = softmax(scores_f32[M,N] * scale) per row."""
    M, N = scores_f32.shape
    _chk(lib().cl_softmax_rows(dt(probs), scores_f32.data_ptr(), ld(scores_f32), probs.data_ptr(), ld(probs), M, N, scale,
                               stream()), "cl_softmax_rows")
    return probs


def zero_(t):
    """In-place clear of a contiguous tensor: a fill kernel on the current stream (no ATen launch, no memset node: DESIGN.md 5)."""
    assert t.is_contiguous()
    _chk(lib().cl_zero(t.data_ptr(), t.numel() * t.element_size(), stream()), "cl_zero")
    return t


def ddim_step(x, e_c, e_u, noise, coef, index, scale, x_prev, pred_x0=None):
    _chk(lib().cl_ddim_step(x.data_ptr(), e_c.data_ptr(), ptr(e_u), ptr(noise), coef.data_ptr(), index, scale,
                            x_prev.data_ptr(), ptr(pred_x0), x.numel(), stream()), "cl_ddim_step")
    return x_prev


def adamw(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    _chk(lib().cl_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                        weight_decay, step, grad_scale, stream()), "cl_adamw")


def tick(counter):
    _chk(lib().cl_tick(counter.data_ptr(), stream()), "cl_tick")


def adamw_dev(p, g, m, v, hyper, step):
    """AdamW with device-resident hyper-parameters {lr, b1, b2, eps, wd, grad_scale} and step counter
    (hipGraph-replayable: nothing step-dependent is a kernel argument).  The caller advances `step` with
    tick() ONCE per optimizer step, before the first bank."""
    _chk(lib().cl_adamw_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(),
                            step.data_ptr(), stream()), "cl_adamw_dev")


GRAD_NORM_MAX_BUFS = 16


def grad_norm_scratch_floats(nbuf=1):
    return int(lib().cl_grad_norm_scratch_floats(nbuf))


def grad_norm(bufs, hyper, max_norm, out, scratch):
    """out[0] = hyper[5] * ||concat(bufs)||_2, out[1] = torch's clip coefficient for the device threshold `max_norm` (None or
    <= 0: tracking only, coef = 1).  bufs: up to 16 flat fp32 tensors.  Two launches, no host sync: capturable."""
    n = len(bufs)
    for b in bufs:
        assert b.dtype == torch.float32 and b.is_contiguous(), (b.dtype, b.stride())
    ptrs = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in bufs])
    counts = (C.c_long * max(n, 1))(*[b.numel() for b in bufs])
    _chk(lib().cl_grad_norm(ptrs, counts, n, hyper.data_ptr(), ptr(max_norm), out.data_ptr(), scratch.data_ptr(), stream()),
         "cl_grad_norm")
    return out


def adamw_dev_clip(p, g, m, v, hyper, step, clip):
    """adamw_dev on g * (grad_scale * clip[1]); clip = grad_norm's out.  clip[1] == 1 gives adamw_dev's bits."""
    _chk(lib().cl_adamw_dev_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(),
                                 step.data_ptr(), clip.data_ptr(), stream()), "cl_adamw_dev_clip")


ADAMW_MAX_GROUPS = 8
ADAMW_CHUNK = 64       # floats per entry of a chunk_group map: the alignment of every tensor in a flat buffer


def adamw_dev_groups(p, g, m, v, hyper_table, chunk_group, step, clip=None):
    """adamw_dev (adamw_dev_clip with `clip` = grad_norm's out) over one flat buffer whose 64-float chunks belong to the
    parameter groups of `hyper_table` (fp32 [G, 6], G <= 8): `chunk_group` (uint8 [numel / 64]) names each chunk's group."""
    assert hyper_table.dtype == torch.float32 and hyper_table.is_contiguous() and hyper_table.dim() == 2 and \
        hyper_table.shape[1] == 6, (hyper_table.dtype, tuple(hyper_table.shape))
    assert chunk_group.dtype == torch.uint8 and chunk_group.is_contiguous() and chunk_group.numel() * ADAMW_CHUNK == p.numel(), \
        (chunk_group.dtype, chunk_group.numel(), p.numel())
    _chk(lib().cl_adamw_dev_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper_table.data_ptr(),
                                   hyper_table.shape[0], chunk_group.data_ptr(), step.data_ptr(), ptr(clip), stream()),
         "cl_adamw_dev_groups")


def lr_schedule(hyper_table, lr_table, step):
    """hyper_table[k, 0] = lr_table[min(step - 1, T - 1), k] on the device: `lr_table` fp32 [T, G], `step` the counter after
    tick().  One small launch, capturable: a replayed step follows the table."""
    assert hyper_table.dtype == lr_table.dtype == torch.float32 and step.dtype == torch.int32
    assert hyper_table.is_contiguous() and lr_table.is_contiguous() and lr_table.dim() == 2 and \
        lr_table.shape[1] == hyper_table.shape[0] and hyper_table.shape[1] == 6, (tuple(hyper_table.shape), tuple(lr_table.shape))
    _chk(lib().cl_lr_schedule(hyper_table.data_ptr(), hyper_table.shape[0], lr_table.data_ptr(), lr_table.shape[0],
                              step.data_ptr(), stream()), "cl_lr_schedule")


def ema_update(shadow, p, decay, num_updates):
    """LitEma.forward over one flat fp32 buffer: shadow -= (1 - d) * (shadow - p), d from the device scalars `decay` (fp32) and
    `num_updates` (int32, advanced with tick() ONCE per optimizer step, before the first bank; negative = no warm-up)."""
    assert shadow.dtype == p.dtype == decay.dtype == torch.float32 and num_updates.dtype == torch.int32
    assert shadow.is_contiguous() and p.is_contiguous() and shadow.numel() == p.numel(), (shadow.shape, p.shape)
    _chk(lib().cl_ema_update(shadow.data_ptr(), p.data_ptr(), p.numel(), decay.data_ptr(), num_updates.data_ptr(), stream()),
         "cl_ema_update")


def swap_(a, b):
    """Exchange the contents of two contiguous fp32 tensors in place (one launch, no third buffer)."""
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    _chk(lib().cl_swap(a.data_ptr(), b.data_ptr(), a.numel(), stream()), "cl_swap")


def ddim_set_t(table, cursor, S, ts):
    _chk(lib().cl_ddim_set_t(table.data_ptr(), cursor.data_ptr(), S, ts.data_ptr(), ts.numel(), stream()), "cl_ddim_set_t")
    return ts


def ddim_step_dev(x, e_c, e_u, noise, coef, cursor, S, scale, x_prev, pred_x0=None):
    _chk(lib().cl_ddim_step_dev(x.data_ptr(), e_c.data_ptr(), ptr(e_u), ptr(noise), coef.data_ptr(), cursor.data_ptr(),
                                S, scale, x_prev.data_ptr(), ptr(pred_x0), x.numel(), stream()), "cl_ddim_step_dev")
    return x_prev


def _dpm_args(x, e_c, e_u, coef, S, hist, x_next, pred_x0):
    n = x.numel()
    assert coef.dtype == torch.float32 and coef.is_contiguous() and tuple(coef.shape) == (S, 8), tuple(coef.shape)
    assert hist.dtype == torch.float32 and hist.is_contiguous() and hist.numel() == 3 * n
    for t in (x, e_c, e_u, x_next, pred_x0):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    return n


def dpmpp_step(x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0=None):
    """One DPM-Solver++ multistep update on row `index` of the [S][8] table (cl_dpmpp_step); x_next may be x."""
    S = coef.shape[0]
    n = _dpm_args(x, e_c, e_u, coef, S, hist, x_next, pred_x0)
    _chk(lib().cl_dpmpp_step(x.data_ptr(), e_c.data_ptr(), ptr(e_u), coef.data_ptr(), index, S, scale, hist.data_ptr(),
                             x_next.data_ptr(), ptr(pred_x0), n, stream()), "cl_dpmpp_step")
    return x_next


def dpmpp_step_dev(x, e_c, e_u, coef, cursor, S, scale, hist, x_next, pred_x0=None):
    """dpmpp_step with the row taken from a device cursor (hipGraph-replayable): cl_dpmpp_step_dev."""
    n = _dpm_args(x, e_c, e_u, coef, S, hist, x_next, pred_x0)
    _chk(lib().cl_dpmpp_step_dev(x.data_ptr(), e_c.data_ptr(), ptr(e_u), coef.data_ptr(), cursor.data_ptr(), S, scale,
                                 hist.data_ptr(), x_next.data_ptr(), ptr(pred_x0), n, stream()), "cl_dpmpp_step_dev")
    return x_next


def dpm_set_t(coef, cursor, S, ts):
    """ts[:] = the model input time (fp32) of row min(cursor, S - 1) of the DPM-Solver++ table: cl_dpm_set_t."""
    assert ts.dtype == torch.float32 and ts.is_contiguous() and tuple(coef.shape) == (S, 8)
    _chk(lib().cl_dpm_set_t(coef.data_ptr(), cursor.data_ptr(), S, ts.data_ptr(), ts.numel(), stream()), "cl_dpm_set_t")
    return ts


# phases of cl_plms_step: the multistep update of iterations >= 1; iteration 0's predictor; iteration 0's final update
PLMS_MULTISTEP, PLMS_START, PLMS_FINISH = 0, 1, 2


def _plms_args(x, e_c, e_u, coef, S, hist, x_out, pred_x0):
    n = x.numel()
    assert coef.dtype == torch.float32 and coef.is_contiguous() and tuple(coef.shape) == (S, 4), tuple(coef.shape)
    assert hist.dtype == torch.float32 and hist.is_contiguous() and hist.numel() == 4 * n
    for t in (x, e_c, e_u, x_out, pred_x0):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    return n


def plms_step(x, e_c, e_u, coef, iteration, phase, scale, hist, x_out, pred_x0=None):
    """One PLMS update of iteration `iteration` on DDIM's [S][4] table (row S - 1 - iteration) and the [4][n] eps ring
    (cl_plms_step).  phase: PLMS_MULTISTEP (iteration >= 1), PLMS_START / PLMS_FINISH (iteration 0: the predictor into an
    x_out that is not x, then the final update of the ORIGINAL x with the evaluation at the predictor)."""
    S = coef.shape[0]
    n = _plms_args(x, e_c, e_u, coef, S, hist, x_out, pred_x0)
    _chk(lib().cl_plms_step(x.data_ptr(), e_c.data_ptr(), ptr(e_u), coef.data_ptr(), iteration, S, phase, scale,
                            hist.data_ptr(), x_out.data_ptr(), ptr(pred_x0), n, stream()), "cl_plms_step")
    return x_out


def plms_step_dev(x, e_c, e_u, coef, cursor, S, scale, hist, x_out, pred_x0=None):
    """The multistep phase of plms_step with the iteration taken from a device cursor, clamped to [1, S - 1]
    (hipGraph-replayable): cl_plms_step_dev."""
    n = _plms_args(x, e_c, e_u, coef, S, hist, x_out, pred_x0)
    _chk(lib().cl_plms_step_dev(x.data_ptr(), e_c.data_ptr(), ptr(e_u), coef.data_ptr(), cursor.data_ptr(), S, scale,
                                hist.data_ptr(), x_out.data_ptr(), ptr(pred_x0), n, stream()), "cl_plms_step_dev")
    return x_out
