"""ctypes binding of libvvhip.so (include/vvhip.h).  PyTorch is used only for device memory and streams.

The C ABI is declared once, in SIGNATURES, and lib() applies it (Part below: the binder of this header, CORE, and of every feature header, the PART of
a *_hip module): the wrappers pass plain Python values (an int64_t or float parameter is converted by its declaration, a pointer is
an address (data_ptr(), _p(t)), a struct goes through C.byref) and a value of the wrong kind raises ctypes.ArgumentError.  tests/test_abi_cpu.py holds table and struct mirrors against the header.

There is NO fallback: if the shared library is missing or a launcher reports an error, a RuntimeError is raised
(the GUI turns exceptions into a dialog -- reference videovanish.py:121-128,1341-1343).
"""
import ctypes as C
import os

import torch

BF16, F16, F32, U8 = 0, 1, 2, 3
SPLIT3 = 16      # vv_groupnorm out_dtype: the K-concatenated split-precision operand (see split3)
EPI_NONE, EPI_GEGLU = 0, 1
ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_SIGMOID = 0, 1, 2, 3, 4, 5
ABI_VERSION = 10
_DT = {"bf16": BF16, "fp16": F16}
_TORCH_H16 = {BF16: torch.bfloat16, F16: torch.float16}

PROFILE_TAG = ""   # prefix added to profile keys (nn.MotionModule sets "motion:" so bench.py can price the temporal block)
PROFILE = None   # bench.py sets this to a list: every MFMA-kernel launch is then bracketed by HIP events on the launch stream


class _Prof:
    """Bracket one launch with events on torch's current stream (the stream the kernel is launched on)."""

    def __init__(self, key, flops, nbytes):
        self.rec = None
        if PROFILE is not None:
            self.rec = [PROFILE_TAG + key, flops, nbytes, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]

    def __enter__(self):
        if self.rec is not None:
            self.rec[3].record()
        return self

    def __exit__(self, *a):
        if self.rec is not None:
            self.rec[4].record()
            PROFILE.append(self.rec)
        return False


# the in-tree build; tools that A/B another build of the library set hip._LIB_PATH before the first launch (tools/bench_*.py).  No
# environment variable is read anywhere in this module: behaviour is selected by API only.
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libvvhip.so")
PROFILE_SHAPES = False   # bench.py --profile-shapes: profile keys of the GEMM / attention launches carry their M, N, K (tools/shape_table.py)


class ConvParams(C.Structure):
    _fields_ = [("in0", C.c_void_p), ("in1", C.c_void_p), ("in_dtype", C.c_int32), ("C0", C.c_int32), ("C1", C.c_int32),
                ("F", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Hv", C.c_int32), ("Wv", C.c_int32),
                ("Hout", C.c_int32), ("Wout", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32),
                ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("weight", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32),
                ("Kpad", C.c_int32), ("Npad", C.c_int32), ("bias", C.c_void_p), ("rowvec", C.c_void_p),
                ("res0", C.c_void_p), ("res1", C.c_void_p), ("res_dtype", C.c_int32), ("out", C.c_void_p),
                ("out_dtype", C.c_int32), ("ldo", C.c_int32), ("epilogue", C.c_int32), ("out_scale", C.c_float), ("ksize_w", C.c_int32),
                ("act", C.c_int32), ("split_heads", C.c_int32), ("split_dim", C.c_int32), ("split_tokens", C.c_int32),
                ("tile_hint", C.c_int32), ("act_slope", C.c_float),
                ("sc_oh", C.c_int32), ("sc_ow", C.c_int32), ("sc_sy", C.c_int32), ("sc_sx", C.c_int32), ("sc_oy", C.c_int32), ("sc_ox", C.c_int32),
                ("gn_partials", C.c_void_p)]


class DeformParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_dtype", C.c_int32), ("offset", C.c_void_p), ("mask", C.c_void_p), ("raw", C.c_void_p),
                ("flow", C.c_void_p), ("max_residue", C.c_float), ("col", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("C", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("dil", C.c_int32),
                ("deform_groups", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32)]


class GroupNormParams(C.Structure):
    _fields_ = [("in0", C.c_void_p), ("in1", C.c_void_p), ("in_dtype", C.c_int32), ("C0", C.c_int32), ("C1", C.c_int32),
                ("F", C.c_int32), ("HW", C.c_int32), ("groups", C.c_int32), ("pool_frames", C.c_int32), ("eps", C.c_float),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("silu", C.c_int32), ("stats_ws", C.c_void_p),
                ("out", C.c_void_p), ("out_dtype", C.c_int32)]


class MotionParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("res1", C.c_void_p), ("out", C.c_void_p), ("out_dtype", C.c_int32), ("stream", C.c_void_p),
                ("params", C.c_void_p), ("gn_affine", C.c_void_p), ("C", C.c_int32), ("F", C.c_int32), ("heads", C.c_int32), ("HW", C.c_int32),
                ("n_slabs", C.c_int32), ("n_params", C.c_int32)]


class ChainParams(C.Structure):
    _fields_ = [("o", C.c_void_p), ("t_in", C.c_void_p), ("x", C.c_void_p), ("res1", C.c_void_p), ("out", C.c_void_p), ("out_dtype", C.c_int32),
                ("stream", C.c_void_p), ("params", C.c_void_p), ("M", C.c_int64), ("C", C.c_int32), ("heads", C.c_int32), ("text_len", C.c_int32),
                ("n_slabs", C.c_int32), ("n_params", C.c_int32), ("layout", C.c_int32), ("o_hw", C.c_int32)]


CHAIN_LAYOUT_IDS = {"rowsplit": 1}      # VV_CHAIN_LAYOUT_ROWSPLIT (vvhip.h): the one stream order the library accepts (0 and 2 are retired orders it refuses)


class ChainFrontParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("gn_affine", C.c_void_p), ("t_out", C.c_void_p), ("qkv", C.c_void_p), ("stream", C.c_void_p), ("params", C.c_void_p),
                ("M", C.c_int64), ("HW", C.c_int32), ("C", C.c_int32), ("heads", C.c_int32), ("n_slabs", C.c_int32), ("n_params", C.c_int32)]


class AttnParams(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
                ("q_bs", C.c_int64), ("k_bs", C.c_int64), ("v_bs", C.c_int64), ("o_bs", C.c_int64),
                ("q_rs", C.c_int64), ("k_rs", C.c_int64), ("v_rs", C.c_int64), ("o_rs", C.c_int64),
                ("B", C.c_int32), ("heads", C.c_int32), ("Nq", C.c_int32), ("Nkv", C.c_int32), ("D", C.c_int32),
                ("scale", C.c_float), ("q_hs", C.c_int64), ("k_hs", C.c_int64), ("v_hs", C.c_int64), ("q_prescaled", C.c_int32), ("lse", C.c_void_p), ("o_hs", C.c_int64)]


# Every function of include/vvhip.h: name -> (restype, argtypes), in the header's order.  Every pointer is P whatever its pointee: device addresses are
# ints, the host arrays (vv_blur_compose host_taps21, vv_u8_normalize mean3 / istd3) are ctypes arrays, structs are passed with C.byref.
P, I, L, Fl = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "vv_abi_version": (I, ()),
    "vv_last_error": (C.c_char_p, ()),
    "vv_device_count": (I, ()),
    "vv_device_name": (I, (I, P, I)),
    "vv_conv_gemm": (I, (P, I, P)),
    "vv_conv_gemm_route": (I, (P, I)),
    "vv_conv_gn_partial_blocks": (I, (I, I)),
    "vv_gn_finalize_partials": (I, (P, I, I, I, I, I, Fl, I, P, P)),
    "vv_groupnorm_nsplit": (I, (I, I)),
    "vv_groupnorm_apply_fin": (I, (P, P, I, P)),
    "vv_groupnorm": (I, (P, I, P)),
    "vv_groupnorm_stats": (I, (P, I, P)),
    "vv_gn_affine": (I, (P, P, P, I, I, P, P)),
    "vv_motion_module_c320": (I, (P, I, P)),
    "vv_spatial_chain_c320": (I, (P, I, P)),
    "vv_spatial_chain_front_c320": (I, (P, I, P)),
    "vv_gn_affine_frames": (I, (P, P, P, I, I, I, P, P)),
    "vv_layernorm": (I, (P, I, I, P, P, P, I, P, I, P)),
    "vv_attention": (I, (P, I, P)),
    "vv_attention_route": (I, (P, I)),
    "vv_attention_merge": (I, (P, P, I, I, I, I, I, P, I, P)),
    "vv_axpby_f32": (I, (P, P, Fl, Fl, P, L, P)),
    "vv_sched_step": (I, (P, P, P, Fl, Fl, Fl, Fl, Fl, P, L, P)),
    "vv_silu_f32": (I, (P, P, L, P)),
    "vv_add_inplace": (I, (P, P, I, L, I, P)),
    "vv_mask_collapse_dilate": (I, (P, I, I, I, I, I, P, P, P, P)),
    "vv_resize_bilinear_u8": (I, (P, I, I, I, I, P, I, I, P)),
    "vv_resize_nearest_u8": (I, (P, I, I, I, I, P, I, I, P)),
    "vv_ycbcr_to_rgb": (I, (P, P, P, I, I, I, I, I, I, P, P)),
    "vv_feather_composite": (I, (P, P, P, I, I, I, Fl, P, P)),
    "vv_chamfer_dt": (I, (P, I, I, I, I, P, P)),
    "vv_mask_bbox": (I, (P, I, I, I, P, P)),
    "vv_roi_paste_composite": (I, (P, I, I, P, P, P, I, I, I, I, I, Fl, P, P)),
    "vv_mask_tile_union": (I, (P, I, I, I, I, P, P)),
    "vv_mask_bbox_tiles": (I, (P, I, I, I, I, P, I, I, P, P)),
    "vv_avgpool2_f32": (I, (P, L, I, I, P, P)),
    "vv_corr_lookup": (I, (P, P, P, P, I, I, P, L, I, P, I, P)),
    "vv_raft_ctx_split": (I, (P, L, P, P, P, I, P)),
    "vv_raft_flow_prep": (I, (P, L, I, I, P, P, I, P)),
    "vv_gru_rh": (I, (P, P, L, P, I, P)),
    "vv_gru_update": (I, (P, P, L, P, P, I, P)),
    "vv_add_flow": (I, (P, P, I, L, P)),
    "vv_add_relu_f32": (I, (P, P, P, L, P)),
    "vv_convex_upsample": (I, (P, P, I, I, I, P, P)),
    "vv_fb_valid": (I, (P, P, I, I, P, P)),
    "vv_deform_im2col": (I, (P, I, P)),
    "vv_fc_input": (I, (P, P, I, I, I, I, P, P)),
    "vv_upsample2x_bilinear": (I, (P, I, I, I, I, I, P, I, P)),
    "vv_flow_combine": (I, (P, I, P, P, L, P, P)),
    "vv_gather_rows": (I, (P, P, L, I, P, P)),
    "vv_fold_patches": (I, (P, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P)),
    "vv_flow_down4": (I, (P, I, I, I, P, P)),
    "vv_gen_input": (I, (P, P, P, L, P, P)),
    "vv_gen_compose": (I, (P, I, P, P, L, P, I, P)),
    "vv_prop_fill": (I, (P, P, P, P, P, P, I, I, P, P)),
    "vv_prop_combine": (I, (P, P, P, P, P, P, I, I, P, P, P, P)),
    "vv_masked_sum_u8": (I, (P, P, L, P, P)),
    "vv_u8_to_f32": (I, (P, P, L, P)),
    "vv_u8_is_zero": (I, (P, P, L, P)),
    "vv_raft_prep": (I, (P, L, P, I, P)),
    "vv_preprocess": (I, (P, P, I, I, I, P, P, I, P)),
    "vv_brushnet_input": (I, (P, P, P, I, I, I, I, I, P, I, P)),
    "vv_pad_channels": (I, (P, L, I, I, Fl, P, I, P)),
    "vv_window_average": (I, (P, P, I, L, P, P)),
    "vv_pad_channels_f32": (I, (P, L, I, I, Fl, P, P)),
    "vv_split_f32": (I, (P, L, Fl, P, P, I, P)),
    "vv_split3": (I, (P, I, L, I, P, I, P)),
    "vv_decode_blend": (I, (P, I, P, I, L, P, P)),
    "vv_blur_compose": (I, (P, P, P, I, I, I, P, P, P, P)),
    "vv_u8_normalize": (I, (P, I, I, P, P, P, I, I, I, P)),
    "vv_layernorm_ex": (I, (P, L, I, P, P, Fl, I, P, I, I, I, P)),
    "vv_maxpool2x2": (I, (P, I, I, I, I, I, L, P, P)),
    "vv_rope_apply": (I, (P, L, I, I, I, P, I, I, P)),
    "vv_dwconv": (I, (P, I, I, I, P, P, I, P, P)),
    "vv_pixel_shuffle2": (I, (P, P, P, I, I, I, I, P, I, I, P)),
    "vv_resize_bilinear_f32": (I, (P, I, I, I, P, I, I, P)),
    "vv_mask_mem_input": (I, (P, L, I, Fl, Fl, P, I, P)),
    "vv_act": (I, (P, I, L, I, P)),
    "vv_prompt_points": (I, (P, P, I, Fl, P, P, I, P, P)),
    "vv_sine_pe_1d": (I, (P, I, I, Fl, P, P)),
    "vv_sam_select": (I, (P, I, I, P, P, I, Fl, Fl, P, P)),
    "vv_sam_pick": (I, (P, I, P, Fl, P, P)),
    "vv_select_f32": (I, (P, P, P, L, P, P)),
    "vv_add_rowvec_unless": (I, (P, P, P, L, I, P)),
    "vv_clamp_f32": (I, (P, L, Fl, Fl, P, P)),
    "vv_sam2_maskdown": (I, (P, I, I, I, Fl, Fl, P, P, P, P, P, P, P, P, Fl, P, P, I, P)),
    "vv_hyper_masks": (I, (P, P, I, I, I, P, P)),
    "vv_fill_holes": (I, (P, I, I, I, P, P)),
}
EXPORTS = list(SIGNATURES)


class Part:
    """One header's part of libvvhip.so: the header's file name, the symbol prefix, the ABI version, the label of the part in error messages ("" for
    vvhip.h itself) and `signatures` (name -> (restype, argtypes), in the header's order).  Nothing is resolved before lib() is first called.
    Every *_hip module declares its header this way: PART = hip.Part(...); lib = PART.lib; _check = PART.check."""

    def __init__(self, header, prefix, version, label, signatures):
        self.header, self.prefix, self.version, self.label, self.signatures = header, prefix, version, label, signatures
        self.dll = None      # the library handle with `signatures` applied, once the part has been used (tests reset it)

    def lib(self):
        """The library with this part's signatures applied (once): the core part loads _LIB_PATH, every other part binds over hip.lib().
        RuntimeError when the library has not been built, an export is missing or <prefix>abi_version() is not `version` -- never falls back."""
        if self.dll is None:
            if self is CORE:
                if not os.path.isfile(_LIB_PATH):
                    raise RuntimeError(f"videovanish_amd: HIP extension missing ({_LIB_PATH}); run videovanish_amd/csrc/build.sh "
                                       "or __graft_entry__.build() -- there is no CPU fallback")
                dll = C.CDLL(_LIB_PATH)
            else:
                dll = CORE.lib()
            for name, (restype, argtypes) in self.signatures.items():
                if not hasattr(dll, name):
                    raise RuntimeError(f"libvvhip.so does not export {name}")
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = restype, argtypes
            v = getattr(dll, self.prefix + "abi_version")()
            if v != self.version:
                raise RuntimeError(f"libvvhip.so {self.label + ' ' if self.label else ''}ABI version {v} != {self.version}")
            self.dll = dll
        return self.dll

    def check(self, rc, what):
        """RuntimeError with the library's message (<prefix>last_error()) when a launcher returned rc != 0."""
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {getattr(self.lib(), self.prefix + 'last_error')().decode()}")


CORE = Part("vvhip.h", "vv_", ABI_VERSION, "", SIGNATURES)
lib = CORE.lib
_check = CORE.check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else 0


def dt_of(t):
    return {torch.bfloat16: BF16, torch.float16: F16, torch.float32: F32, torch.uint8: U8}[t.dtype]


def h16(dtype):
    return _TORCH_H16[dtype]


def dtype_id(name):
    return _DT[name]


def _need_cuda(*ts):
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("videovanish_amd.hip: tensors must live on the GPU (no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError("videovanish_amd.hip: tensors must be contiguous")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            # kernels are launched on the CURRENT device's stream: a tensor on another GPU would be a cross-device pointer
            raise RuntimeError(f"videovanish_amd.hip: tensor on {t.device} but the current device is cuda:{cur} "
                               "(one process per GPU: torch.cuda.set_device(LOCAL_RANK) before building the model)")


# ---- the tensor checks the byte-image wrappers share (hip.roi_paste_composite and the *_hip modules) ---------------------------------------------
def _out_like(what, out, src, name):
    """The caller's out= of a wrapper that must not write over its input `src` (called `name` in the message), or a fresh tensor."""
    if out is None:
        return torch.empty_like(src)
    if out.shape != src.shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.data_ptr() == src.data_ptr():
        raise RuntimeError(f"{what}: out must be a contiguous u8 buffer of {name}'s shape, not {name} itself")
    return out


def _need_clip(what, frames, *masks):
    """frames [T,H,W,3] u8 and masks [T,H,W] u8 on the device -> (T, H, W)."""
    _need_cuda(frames, *masks)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise RuntimeError(f"{what}: the frames must be a [T >= 1, H, W, 3] uint8 tensor")
    T, H, W, _ = frames.shape
    for m in masks:
        if m.dtype != torch.uint8 or tuple(m.shape) != (T, H, W):
            raise RuntimeError(f"{what}: every mask must be a [T, H, W] uint8 tensor of the frames' size")
    return T, H, W


def _need_table(what, name, tab, T):
    """tab: one 256-entry byte table per frame and channel (a LUT, grain amplitudes)."""
    if tab.dtype != torch.uint8 or tuple(tab.shape) != (T, 3, 256):
        raise RuntimeError(f"{what}: {name} must be a [T, 3, 256] uint8 tensor")


def _need_window(what, patch, orig, mask2d, offsets):
    """The shapes the window pastes share (roi_paste_composite's arguments); -> (T, Hm, Wm, H0, W0)."""
    _need_cuda(patch, orig, mask2d, offsets)
    u8 = torch.uint8
    if patch.dtype != u8 or orig.dtype != u8 or patch.dim() != 4 or orig.dim() != 4 or patch.shape[3] != 3 or orig.shape[3] != 3 or patch.shape[0] < 1:
        raise RuntimeError(f"{what}: patch and orig must be [T >= 1, H, W, 3] uint8 tensors")
    T, Hm, Wm, _ = patch.shape
    _, H0, W0, _ = orig.shape
    if orig.shape[0] != T or offsets.dtype != torch.int32 or tuple(offsets.shape) != (T, 2) or (
            mask2d is not None and (mask2d.dtype != u8 or tuple(mask2d.shape) != (T, H0, W0))):
        raise RuntimeError(f"{what}: shapes / dtypes do not match")
    return T, Hm, Wm, H0, W0


# vv_conv_gemm_route codes (vvhip.h VV_ROUTE_*): 128-row kernels = loader + tile
ROUTE_TILE_128x160, ROUTE_TILE_128x128, ROUTE_TILE_128x16 = 0, 1, 2
ROUTE_GENERIC, ROUTE_GENERIC_F32, ROUTE_FAST, ROUTE_FAST32, ROUTE_HALO, ROUTE_LIN, ROUTE_FAST9, ROUTE_HALO_GN = 0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 0x80
ROUTE_256x320_LIN, ROUTE_256x320_CONV, ROUTE_256x256_LIN, ROUTE_256x256_CONV = 0x100, 0x101, 0x102, 0x103
ROUTE_256P8_LIN, ROUTE_256P8_CONV, ROUTE_256P8A_LIN, ROUTE_256P8A_CONV = 0x104, 0x105, 0x106, 0x107
_ROUTE_LOADERS = {ROUTE_GENERIC: "generic", ROUTE_GENERIC_F32: "generic-f32", ROUTE_FAST: "fast", ROUTE_FAST32: "fast32", ROUTE_HALO: "halo",
                  ROUTE_LIN: "lin", ROUTE_FAST9: "fast9", ROUTE_HALO_GN: "halo+gn"}
_ROUTE_TILES = {ROUTE_TILE_128x160: "128x160", ROUTE_TILE_128x128: "128x128", ROUTE_TILE_128x16: "128x16"}
_ROUTE_256 = {ROUTE_256x320_LIN: ("256x320", "lin"), ROUTE_256x320_CONV: ("256x320", "conv"), ROUTE_256x256_LIN: ("256x256", "lin"),
              ROUTE_256x256_CONV: ("256x256", "conv"), ROUTE_256P8_LIN: ("256x256p8", "lin"), ROUTE_256P8_CONV: ("256x256p8", "conv"),
              ROUTE_256P8A_LIN: ("256x256p8", "lin"), ROUTE_256P8A_CONV: ("256x256p8", "conv")}


def route_tile(code):
    """Output tile of a route (the profile label): "128x160", "256x320", "256x256p8" (both 8-phase forms), ..."""
    if code in _ROUTE_256:
        return _ROUTE_256[code][0]
    if code >= 0x10 and (code & ~15) in _ROUTE_LOADERS and (code & 15) in _ROUTE_TILES:
        return _ROUTE_TILES[code & 15]
    raise ValueError(f"not a vv_conv_gemm route: {code}")


def route_name(code):
    """Readable name of a route: "fast9 128x160", "256x320 conv", "256x256p8a lin", ..."""
    if code in _ROUTE_256:
        t, m = _ROUTE_256[code]
        return f"{t}{'a' if code in (ROUTE_256P8A_LIN, ROUTE_256P8A_CONV) else ''} {m}"
    return f"{_ROUTE_LOADERS[code & ~15]} {route_tile(code)}"


def _meta(v, dt):
    """conv_gemm_route operand: a tensor (any device, `meta` included) or a shape, taken as a tensor of dtype dt"""
    if v is None or isinstance(v, torch.Tensor):
        return v
    return torch.empty(tuple(v), dtype=dt, device="meta")


# ----------------------------------------------------------------------------------------------------------------
def conv_gemm(dtype, x0, weight, N, K, *, x1=None, F=1, Hin=1, Win=1, Hv=None, Wv=None, Hout=None, Wout=None, ksize=1,
              stride=1, pad_t=0, pad_l=0, bias=None, rowvec=None, res0=None, res1=None, out=None, out_dtype=None,
              epilogue=EPI_NONE, out_scale=1.0, C0=None, C1=0, ksize_w=0, act=ACT_NONE, out_col=0, split_heads=0, split_dim=0, split_tokens=0, tile_hint=0,
              act_slope=0.0, scatter=None, gn_partials=None, _route=False):
    """Launch vv_conv_gemm.  gn_partials (a GNPartials the caller made for this layer's output): the layer also leaves per-channel (sum, sum of squares) partials of its output there
    for the GroupNorm that reads it next (vv_conv_params.gn_partials; only the 128 x 160 halo-tile 3x3 kernel can, any other launch is refused).  x0/x1: NHWC activations ([F,Hin,Win,C] or any shape with C last); weight: [Npad,Kpad] h16.
    scatter = (OH, OW, sy, sx, oy, ox): row (f, y, x) of this launch goes to row (f*OH + y*sy + oy)*OW + x*sx + ox of `out` (required; residuals
    are read at the same rows) -- the four parity launches of a convolution over a nearest-2x upsampled image (nn.UpConv2x)."""
    if _route:      # conv_gemm_route: nothing is launched, pointers are passed as null / non-null flags
        x0, x1, weight, res0, res1 = _meta(x0, h16(dtype)), _meta(x1, h16(dtype)), _meta(weight, h16(dtype)), _meta(res0, torch.float32), _meta(res1, torch.float32)
        bias, rowvec, out = _meta(bias, torch.float32), _meta(rowvec, torch.float32), _meta(out, h16(dtype) if out_dtype is None else out_dtype)

        def ptr(t, ofs=0):
            return 0 if t is None else 1
    else:
        _need_cuda(x0, x1, weight, bias, rowvec, res0, res1, out)      # out_col: write into columns [out_col, out_col+N) of `out`

        def ptr(t, ofs=0):
            return 0 if t is None else t.data_ptr() + ofs
    Hv = Hin if Hv is None else Hv
    Wv = Win if Wv is None else Wv
    Hout = Hv if Hout is None else Hout
    Wout = Wv if Wout is None else Wout
    C0 = x0.shape[-1] if C0 is None else C0
    if x1 is not None:
        C1 = x1.shape[-1]
    M = F * Hout * Wout
    nout = N // 2 if epilogue == EPI_GEGLU else N
    if res0 is not None and res1 is not None and res0.dtype != res1.dtype:
        raise RuntimeError(f"vv_conv_gemm: res0 ({res0.dtype}) and res1 ({res1.dtype}) must share one dtype (one res_dtype field covers both)")
    res_dt = dt_of(res0) if res0 is not None else (dt_of(res1) if res1 is not None else F32)
    sc = (0, 0, 0, 0, 0, 0) if scatter is None else tuple(int(v) for v in scatter)
    if scatter is not None and (out is None or out.numel() < F * sc[0] * sc[1] * nout):
        raise RuntimeError("vv_conv_gemm: a scattered store needs the caller's [F*OH*OW, N] output tensor")
    if out is None:
        od = h16(dtype) if out_dtype is None else out_dtype
        out = torch.empty((M, nout), dtype=od, device="meta" if _route else x0.device)
    p = ConvParams(in0=ptr(x0), in1=ptr(x1), in_dtype=dt_of(x0), C0=C0, C1=C1, F=F, Hin=Hin,
                   Win=Win, Hv=Hv, Wv=Wv, Hout=Hout, Wout=Wout, ksize=ksize, stride=stride, pad_t=pad_t, pad_l=pad_l,
                   weight=ptr(weight), N=N, K=K, Kpad=weight.shape[1], Npad=weight.shape[0],
                   bias=ptr(bias), rowvec=ptr(rowvec), res0=ptr(res0), res1=ptr(res1),
                   res_dtype=res_dt, out=ptr(out, out_col * out.element_size()), out_dtype=dt_of(out), ldo=out.shape[-1],
                   epilogue=epilogue, out_scale=out_scale, ksize_w=ksize_w, act=act, split_heads=split_heads, split_dim=split_dim,
                   split_tokens=split_tokens, tile_hint=tile_hint, act_slope=act_slope,
                   sc_oh=sc[0], sc_ow=sc[1], sc_sy=sc[2], sc_sx=sc[3], sc_oy=sc[4], sc_ox=sc[5])
    if _route:
        p.gn_partials = 1 if gn_partials else 0
        return lib().vv_conv_gemm_route(C.byref(p), dtype)
    if gn_partials is not None:
        assert (gn_partials.F, gn_partials.nblk, gn_partials.HW, gn_partials.C) == (F, lib().vv_conv_gn_partial_blocks(Hout, Wout), Hout * Wout, N), "GroupNorm partials of another shape"
        p.gn_partials = _p(gn_partials.part)
    key = None
    if PROFILE is not None:
        # the tile of the kernel that runs, from the dispatcher itself (vv_conv_gemm_route)
        route = lib().vv_conv_gemm_route(C.byref(p), dtype)
        tile = route_tile(route) if route > 0 else "refused"
        if PROFILE_SHAPES:
            tile = f"M{M},N{N},K{K}|" + tile
        key = f"conv_gemm[{tile},{'f32in' if x0.dtype == torch.float32 else 'h16in'},k{ksize}{'x%d' % ksize_w if ksize_w and ksize_w != ksize else ''}]"
    nbytes = F * Hin * Win * (C0 + C1) * x0.element_size() + N * K * 2 + M * nout * out.element_size() + sum(
        M * N * r.element_size() for r in (res0, res1) if r is not None)
    with _Prof(key, 2.0 * M * N * K, nbytes):
        _check(lib().vv_conv_gemm(C.byref(p), dtype, _stream()), "vv_conv_gemm")
    return out


def conv_gemm_route(dtype, x0, weight, N, K, **kw):
    """The kernel vv_conv_gemm would launch for conv_gemm(dtype, x0, weight, N, K, **kw) (same arguments), as a ROUTE_* code (route_name / route_tile),
    or the negative VV_E_* code the launch would be refused with (vv_last_error() holds the message).  Nothing is launched and no GPU is needed: tensors
    may live on any device (`meta` included), and any tensor argument may be given as its shape instead (activations and weight: h16 of `dtype`;
    bias, rowvec, residuals: fp32; out: out_dtype)."""
    return conv_gemm(dtype, x0, weight, N, K, _route=True, **kw)


class GNPartials:
    """per-channel (sum, sum of squares) partials [F, nblk, N, 2] of a layer's output [F * Hout * Wout, N]: the caller makes it, conv_gemm(gn_partials=) fills it, groupnorm(partials=) reads it"""

    def __init__(self, F, Hout, Wout, N, device):
        self.nblk, self.F, self.HW, self.C = lib().vv_conv_gn_partial_blocks(Hout, Wout), F, Hout * Wout, N
        self.part = torch.empty((F, self.nblk, N, 2), dtype=torch.float32, device=device)

    def finalize(self, groups, eps, pool_frames=False):
        """-> fin [F, groups, 2] (mean, rstd): vv_gn_finalize_partials (double accumulation, fixed order)"""
        fin = torch.empty((self.F, groups, 2), dtype=torch.float32, device=self.part.device)
        _check(lib().vv_gn_finalize_partials(_p(self.part), self.F, self.nblk, self.C, self.HW, groups, eps, int(bool(pool_frames)), _p(fin), _stream()),
               "vv_gn_finalize_partials")
        return fin


def _gn_workspace(F, HW, Ctot, groups, device):      # -> (stats_ws of a GroupNorm over [F * HW, Ctot], address of `fin` in it: (mean, rstd) [F, groups, 2] behind the F * nsplit partial records)
    nsplit = lib().vv_groupnorm_nsplit(HW, Ctot)
    ws = torch.empty(F * (nsplit + 1) * groups * 2, dtype=torch.float32, device=device)
    return ws, ws.data_ptr() + F * nsplit * groups * 2 * ws.element_size()


def _gn_stats(dtype, x, gamma, beta, groups, eps, F, HW, pool_frames):
    """the statistics pass of a GroupNorm over x [F * HW, C] alone (vv_groupnorm_stats) -> (address of fin [F, groups, 2], the tensor that keeps it alive)"""
    Cc = x.shape[-1]
    ws, fin = _gn_workspace(F, HW, Cc, groups, x.device)
    gp = GroupNormParams(in0=_p(x), in1=0, in_dtype=dt_of(x), C0=Cc, C1=0, F=F, HW=HW, groups=groups, pool_frames=pool_frames, eps=eps,
                         gamma=_p(gamma), beta=_p(beta), silu=0, stats_ws=_p(ws), out=0, out_dtype=F32)
    with _Prof("groupnorm", 0.0, F * HW * Cc * x.element_size()):
        _check(lib().vv_groupnorm_stats(C.byref(gp), dtype, _stream()), "vv_groupnorm_stats")
    return fin, ws


def groupnorm(dtype, x0, gamma, beta, groups, eps, *, x1=None, F, HW, silu=False, pool_frames=False, out_dtype=None, act=None, partials=None):
    """partials (GNPartials of x0, one source): the statistics pass over HBM is skipped -- (mean, rstd) come from the producer's partial sums."""
    _need_cuda(x0, x1, gamma, beta)
    C0 = x0.shape[-1]
    C1 = x1.shape[-1] if x1 is not None else 0
    Ctot = C0 + C1
    ws, _ = _gn_workspace(F, HW, Ctot, groups, x0.device)
    if out_dtype == "split3":          # [M, 3C] h16 = [hi | lo * 2^4 | hi * 2^-10]: feeds a split-precision GEMM directly (no fp32 round trip)
        out = torch.empty((F * HW, 3 * Ctot), dtype=h16(dtype), device=x0.device)
        odt = SPLIT3
    else:
        out = torch.empty((F * HW, Ctot), dtype=h16(dtype) if out_dtype is None else out_dtype, device=x0.device)
        odt = dt_of(out)
    p = GroupNormParams(in0=_p(x0), in1=_p(x1), in_dtype=dt_of(x0), C0=C0, C1=C1, F=F, HW=HW,
                        groups=groups, pool_frames=int(pool_frames), eps=eps, gamma=_p(gamma), beta=_p(beta),
                        silu=int(act) if act is not None else int(silu), stats_ws=_p(ws), out=_p(out), out_dtype=odt)
    if partials is not None:
        assert x1 is None and (partials.F, partials.HW, partials.C) == (F, HW, C0), "GroupNorm partials do not describe this tensor"
        fin = partials.finalize(groups, eps, pool_frames)
        with _Prof("groupnorm", 0.0, F * HW * Ctot * (x0.element_size() + (6 if odt == SPLIT3 else out.element_size()))):
            _check(lib().vv_groupnorm_apply_fin(C.byref(p), _p(fin), dtype, _stream()), "vv_groupnorm_apply_fin")
        return out
    with _Prof("groupnorm", 0.0, F * HW * Ctot * (2 * x0.element_size() + (6 if odt == SPLIT3 else out.element_size()))):
        _check(lib().vv_groupnorm(C.byref(p), dtype, _stream()), "vv_groupnorm")
    return out


def _own_out(out, shape, dtype, like, what):
    """the caller's output tensor (out= of the fused level-0 wrappers; tests pass views into sentinel-filled buffers), or a fresh one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != like.device or not out.is_contiguous():
        raise RuntimeError(f"{what}: the given output must be a contiguous {dtype} tensor of shape {tuple(shape)} on {like.device}")
    return out


def motion_module_c320(dtype, x, stream_w, params, gamma, beta, groups, eps, *, F, HW, res1=None, out_dtype=torch.float32, out=None):
    """The fused motion module (vv_motion.hip): clip-pooled GroupNorm statistics -> per-channel affine -> ONE kernel for the whole block.
    out: write into the caller's contiguous [F * HW, C] tensor (its dtype is the output type) instead of a fresh one."""
    _need_cuda(x, stream_w, params, gamma, beta, res1)
    Cc = x.shape[-1]
    fin, keep = _gn_stats(dtype, x, gamma, beta, groups, eps, F, HW, 1)      # keep: owns fin until the launches below are enqueued
    aff = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    _check(lib().vv_gn_affine(fin, _p(gamma), _p(beta), Cc, groups, _p(aff), _stream()), "vv_gn_affine")
    out = _own_out(out, (F * HW, Cc), out_dtype if out is None else out.dtype, x, "motion_module_c320")
    mp = MotionParams(x=_p(x), res1=_p(res1), out=_p(out), out_dtype=dt_of(out), stream=_p(stream_w), params=_p(params), gn_affine=_p(aff), C=Cc, F=F, heads=8, HW=HW,
                      n_slabs=stream_w.shape[0], n_params=params.numel())
    with _Prof("motion_module_fused[c320]", 2.0 * 22 * Cc * Cc * F * HW + 8.0 * F * Cc * F * HW, F * HW * Cc * (x.element_size() * 2 + out.element_size())):
        _check(lib().vv_motion_module_c320(C.byref(mp), dtype, _stream()), "vv_motion_module_c320")
    return out


def layernorm(dtype, x, gamma, beta, pe=None, rows_per_frame=1, out=None):
    _need_cuda(x, gamma, beta, pe)
    M, Cc = x.shape
    out = _own_out(out, (M, Cc), h16(dtype), x, "layernorm")
    with _Prof("layernorm", 0.0, M * Cc * 6):
        _check(lib().vv_layernorm(_p(x), M, Cc, _p(gamma), _p(beta), _p(pe), rows_per_frame, _p(out), dtype, _stream()), "vv_layernorm")
    return out


def attention_q_scale(D):
    """factor a caller folds into its query projection for vv_attention(q_prescaled=1): softmax scale * log2(e)."""
    return float(D) ** -0.5 * 1.4426950408889634


# vv_attention_route codes (vvhip.h VV_ATTN_ROUTE_*): route = form | flags
ATTN_ROUTE_CROSS, ATTN_ROUTE_RAGGED = 1, 2
ATTN_ROUTE_SHORT, ATTN_ROUTE_SHORT_2W, ATTN_ROUTE_DMA64, ATTN_ROUTE_REG80, ATTN_ROUTE_W4x32, ATTN_ROUTE_W8x16 = 0x10, 0x20, 0x30, 0x40, 0x50, 0x60
ATTN_ROUTE_D512_W4, ATTN_ROUTE_D512_W8, ATTN_ROUTE_MFMA32_D40, ATTN_ROUTE_MFMA32_D40_Q2, ATTN_ROUTE_MFMA32_D80 = 0x70, 0x80, 0x90, 0xa0, 0xb0
_ATTN_ROUTES = {ATTN_ROUTE_SHORT: "short", ATTN_ROUTE_SHORT_2W: "short-2w", ATTN_ROUTE_DMA64: "dma64", ATTN_ROUTE_REG80: "reg80", ATTN_ROUTE_W4x32: "w4x32",
                ATTN_ROUTE_W8x16: "w8x16", ATTN_ROUTE_D512_W4: "d512-w4", ATTN_ROUTE_D512_W8: "d512-w8", ATTN_ROUTE_MFMA32_D40: "mfma32-d40",
                ATTN_ROUTE_MFMA32_D40_Q2: "mfma32-d40-q2", ATTN_ROUTE_MFMA32_D80: "mfma32-d80"}
_ATTN_ROUTE_FLAGS = {ATTN_ROUTE_DMA64: {0: " self", ATTN_ROUTE_CROSS: " cross"}, ATTN_ROUTE_REG80: {0: " self", ATTN_ROUTE_CROSS: " cross"},
                     ATTN_ROUTE_MFMA32_D40: {0: " whole", ATTN_ROUTE_RAGGED: " ragged"}, ATTN_ROUTE_MFMA32_D40_Q2: {0: " whole", ATTN_ROUTE_RAGGED: " ragged"},
                     ATTN_ROUTE_MFMA32_D80: {0: " whole", ATTN_ROUTE_RAGGED: " ragged"}}


def attn_route_name(code):
    """Readable name of a vv_attention route: "short", "dma64 cross", "mfma32-d40 ragged", ..."""
    form, flags = code & ~15, code & 15
    if form not in _ATTN_ROUTES or flags not in _ATTN_ROUTE_FLAGS.get(form, {0: ""}):
        raise ValueError(f"not a vv_attention route: {code}")
    return _ATTN_ROUTES[form] + _ATTN_ROUTE_FLAGS.get(form, {0: ""})[flags]


def attention_label(Nq, Nkv):
    """The kind in the profile key attention[kind,dD] (bench.py's kernel_times_s reads these keys): temporal = the short shapes, cross = the 77 text tokens"""
    return "temporal" if (Nq <= 32 and Nkv <= 32) else ("cross" if Nkv < 128 and Nq != Nkv else "spatial")


def attention(dtype, q, k, v, out, *, B, heads, Nq, Nkv, D, q_bs, k_bs, v_bs, o_bs, q_rs, k_rs, v_rs, o_rs, q_off=0, k_off=0, v_off=0,
              q_hs=0, k_hs=0, v_hs=0, q_prescaled=False, scale=None, lse=None, o_hs=0, _route=False):
    """q/k/v/out: h16 tensors (any shape); element offsets *_off select a column block inside a fused QKV buffer.
    q_prescaled: q already carries D**-0.5 * log2(e) (attention_q_scale(D) folded into the query projection)."""
    if _route:      # attention_route: nothing is launched, pointers are passed as null / non-null flags
        flag = lambda t: 0 if t is None else 1
        p = AttnParams(q=flag(q), k=flag(k), v=flag(v), o=flag(out), lse=flag(lse))
    else:
        _need_cuda(q, k, v, out)
        es = 2
        p = AttnParams(q=q.data_ptr() + q_off * es, k=k.data_ptr() + k_off * es, v=v.data_ptr() + v_off * es, o=_p(out), lse=_p(lse))
    p.q_bs, p.k_bs, p.v_bs, p.o_bs, p.q_rs, p.k_rs, p.v_rs, p.o_rs = q_bs, k_bs, v_bs, o_bs, q_rs, k_rs, v_rs, o_rs
    p.B, p.heads, p.Nq, p.Nkv, p.D = B, heads, Nq, Nkv, D
    p.scale = float(D) ** -0.5 if scale is None else float(scale)
    p.q_hs, p.k_hs, p.v_hs, p.o_hs, p.q_prescaled = q_hs, k_hs, v_hs, o_hs, 1 if q_prescaled else 0
    if _route:
        return lib().vv_attention_route(C.byref(p), dtype)
    kind = attention_label(Nq, Nkv)
    if PROFILE_SHAPES:
        kind = f"B{B},N{Nq}|" + kind
    with _Prof(f"attention[{kind},d{D}]", 4.0 * B * heads * Nq * Nkv * D, 2 * B * heads * D * (2 * Nq + 2 * Nkv)):
        _check(lib().vv_attention(C.byref(p), dtype, _stream()), "vv_attention")
    return out


def attention_route(dtype, q, k, v, out, **kw):
    """The kernel vv_attention would launch for attention(dtype, q, k, v, out, **kw) (same keywords), as an ATTN_ROUTE_* code (attn_route_name), or the negative
    VV_E_* code the launch would be refused with.  Needs no GPU: q / k / v / out / lse may be tensors on any device or bare shapes (None = a null pointer);
    only the keywords decide."""
    return attention(dtype, q, k, v, out, _route=True, **kw)


def deform_im2col(dtype, x, *, B, H, W, kh=3, kw=3, stride=1, pad=1, dil=1, deform_groups=1, offset=None, mask=None, raw=None, flow=None,
                  max_residue=0.0, out=None):
    """Deformed, modulated im2col matrix [M, kh*kw*C] (h16) of an NHWC tensor x [B*H*W, C]: see vv_deform_im2col in include/vvhip.h.
    Either (offset [M, 2*dg*K], mask [M, dg*K] | None) or raw [M, 3*dg*K] (+ flow [M, 2]) -- the DeformableAlignment front end."""
    _need_cuda(x, offset, mask, raw, flow)
    Cc = x.shape[-1]
    Ho = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    col = _own_out(out, (B * Ho * Wo, kh * kw * Cc), h16(dtype), x, "deform_im2col")
    for t in (offset, mask, raw, flow):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("vv_deform_im2col: offset / mask / raw / flow must be fp32")
    p = DeformParams(x=_p(x), x_dtype=dt_of(x), offset=_p(offset), mask=_p(mask), raw=_p(raw), flow=_p(flow), max_residue=max_residue,
                     col=_p(col), B=B, H=H, W=W, C=Cc, kh=kh, kw=kw, stride=stride, pad=pad, dil=dil, deform_groups=deform_groups, Ho=Ho, Wo=Wo)
    with _Prof("deform_im2col", 0.0, col.numel() * 2 * 5):
        _check(lib().vv_deform_im2col(C.byref(p), dtype, _stream()), "vv_deform_im2col")
    return col, Ho, Wo


def fc_input(flow, mask_u8, pad, out=None):
    """flow fp32 [T,H,W,2] + mask u8 [T,H,W] -> fp32 [T, H+2pad, W+2pad, 8] = (flow*(1-m) | m | 0..) replicate-padded."""
    _need_cuda(flow, mask_u8)
    T, H, W, _ = flow.shape
    out = _own_out(out, (T, H + 2 * pad, W + 2 * pad, 8), torch.float32, flow, "fc_input")
    _check(lib().vv_fc_input(_p(flow), _p(mask_u8), T, H, W, pad, _p(out), _stream()), "vv_fc_input")
    return out


def upsample2x_bilinear(dtype, x, B, H, W, out=None):
    """NHWC rows [B*H*W, C] (h16 or fp32) -> [B*2H*2W, C], bilinear, align_corners=True."""
    _need_cuda(x)
    Cc = x.shape[-1]
    out = _own_out(out, (B * 4 * H * W, Cc), x.dtype, x, "upsample2x_bilinear")
    _check(lib().vv_upsample2x_bilinear(_p(x), dt_of(x), B, H, W, Cc, _p(out), dtype, _stream()), "vv_upsample2x_bilinear")
    return out


def flow_combine(pred, flow, mask_u8, out=None):
    """pred fp32 [N, ld>=2], flow fp32 [..., 2] with N pixels, mask u8 [N] -> fp32 like flow: pred in the hole, flow outside."""
    _need_cuda(pred, flow, mask_u8)
    out = _own_out(out, flow.shape, torch.float32, flow, "flow_combine")
    _check(lib().vv_flow_combine(_p(pred), pred.shape[-1], _p(flow), _p(mask_u8), mask_u8.numel(), _p(out), _stream()), "vv_flow_combine")
    return out


def gather_rows(src, idx, out=None):
    """out[i] = src[idx[i]] (idx int32 on the device, < 0 -> zero row); rows must be multiples of 16 bytes."""
    _need_cuda(src, idx)
    out = _own_out(out, (idx.numel(), src.shape[-1]), src.dtype, src, "gather_rows")
    _check(lib().vv_gather_rows(_p(src), _p(idx), idx.numel(), src.shape[-1] * src.element_size(), _p(out), _stream()), "vv_gather_rows")
    return out


def fold_patches(dtype, x, B, fh, fw, Cc, h, w, k=7, stride=3, pad=3, normalise=False, gelu=False, out_dtype=torch.float32, out=None):
    """tap-major patch rows [B*fh*fw, k*k*C] -> [B*h*w, C] (F.fold; optional overlap normalisation and GELU)."""
    _need_cuda(x)
    out = _own_out(out, (B * h * w, Cc), out_dtype, x, "fold_patches")
    _check(lib().vv_fold_patches(_p(x), dt_of(x), B, fh, fw, Cc, h, w, k, stride, pad, int(normalise), int(gelu), _p(out), dt_of(out), dtype, _stream()),
           "vv_fold_patches")
    return out


def flow_down4(flow, out=None):
    """fp32 [T,H,W,2] -> fp32 [T,H/4,W/4,2] (bilinear 1/4, align_corners=False, values / 4)."""
    _need_cuda(flow)
    T, H, W, _ = flow.shape
    out = _own_out(out, (T, H // 4, W // 4, 2), torch.float32, flow, "flow_down4")
    _check(lib().vv_flow_down4(_p(flow), T, H, W, _p(out), _stream()), "vv_flow_down4")
    return out


def gen_input(frames_u8, mask_in_u8, mask_up_u8, out=None):
    """u8 [T,H,W,3] + two u8 [T,H,W] masks -> fp32 [T*H*W, 8] encoder input rows."""
    _need_cuda(frames_u8, mask_in_u8, mask_up_u8)
    n = mask_in_u8.numel()
    out = _own_out(out, (n, 8), torch.float32, frames_u8, "gen_input")
    _check(lib().vv_gen_input(_p(frames_u8), _p(mask_in_u8), _p(mask_up_u8), n, _p(out), _stream()), "vv_gen_input")
    return out


def gen_compose(pred, ori_u8, mask_u8, acc, first):
    _need_cuda(pred, ori_u8, mask_u8, acc)
    _check(lib().vv_gen_compose(_p(pred), pred.shape[-1], _p(ori_u8), _p(mask_u8), mask_u8.numel(), _p(acc), int(first), _stream()), "vv_gen_compose")
    return acc


def axpby(x, y, ca, cb, out=None):
    _need_cuda(x, y, out)
    out = torch.empty_like(x) if out is None else out
    _check(lib().vv_axpby_f32(_p(x), _p(y), ca, cb, _p(out), x.numel(), _stream()), "vv_axpby_f32")
    return out


def sched_step(x, eps, z, sa_t, sb_t, c_x0, c_eps, c_z=0.0, out=None):
    _need_cuda(x, eps, z, out)
    out = torch.empty_like(x) if out is None else out
    _check(lib().vv_sched_step(_p(x), _p(eps), _p(z), sa_t, sb_t, c_x0, c_eps, c_z,
                               _p(out), x.numel(), _stream()), "vv_sched_step")
    return out


def silu(x, out=None):
    _need_cuda(x)
    out = _own_out(out, x.shape, x.dtype, x, "silu")
    _check(lib().vv_silu_f32(_p(x), _p(out), x.numel(), _stream()), "vv_silu_f32")
    return out


def add_inplace(dtype, x, y):
    _need_cuda(x, y)
    assert x.dtype == torch.float32 and x.numel() == y.numel()
    _check(lib().vv_add_inplace(_p(x), _p(y), dt_of(y), x.numel(), dtype, _stream()), "vv_add_inplace")
    return x


def mask_collapse_dilate(masks, iters, out=None):
    """masks [T,H,W,ch] u8 -> [T,H,W] u8 {0,255}  (reference diffuerase.py:27-31)."""
    _need_cuda(masks)
    if masks.dim() == 3:
        masks = masks[..., None].contiguous()
    T, H, W, ch = masks.shape
    out = _own_out(out, (T, H, W), torch.uint8, masks, "mask_collapse_dilate")
    tmp = torch.empty_like(out)
    flags = torch.empty(T, dtype=torch.int32, device=masks.device)
    with _Prof("mask_collapse_dilate", 0.0, T * H * W * (ch + 1)):
        _check(lib().vv_mask_collapse_dilate(_p(masks), T, H, W, ch, int(iters), _p(out), _p(tmp), _p(flags), _stream()), "vv_mask_collapse_dilate")
    return out


def resize_u8(src, Hd, Wd, mode="bilinear", out=None):
    _need_cuda(src)
    s4 = src if src.dim() == 4 else src[..., None]
    T, Hs, Ws, ch = s4.shape
    dst = _own_out(out, (T, Hd, Wd, ch), torch.uint8, src, "resize_u8")
    fn = lib().vv_resize_bilinear_u8 if mode == "bilinear" else lib().vv_resize_nearest_u8
    with _Prof("resize_u8", 0.0, src.numel() + dst.numel()):
        _check(fn(_p(src), T, Hs, Ws, ch, _p(dst), Hd, Wd, _stream()), "vv_resize_u8")
    return dst if src.dim() == 4 else dst[..., 0]


def feather_composite(inpainted, orig, mask2d, feather_px, out=None):
    _need_cuda(inpainted, orig, mask2d)
    T, H, W, _ = inpainted.shape
    out = _own_out(out, inpainted.shape, torch.uint8, inpainted, "feather_composite")
    with _Prof("feather_composite", 0.0, T * H * W * (3 + 3 + 1 + 3)):
        _check(lib().vv_feather_composite(_p(inpainted), _p(orig), _p(mask2d), T, H, W, feather_px, _p(out), _stream()), "vv_feather_composite")
    return out


def mask_bbox(mask2d):
    """mask2d [T,H,W] u8 -> [T,4] int32 on the device: half-open (y0, x0, y1, x1) of each frame's non-zero bytes, (0, 0, 0, 0) when there is none."""
    _need_cuda(mask2d)
    T, H, W = mask2d.shape
    bbox = torch.empty((T, 4), dtype=torch.int32, device=mask2d.device)
    with _Prof("mask_bbox", 0.0, T * H * W + T * 16):
        _check(lib().vv_mask_bbox(_p(mask2d), T, H, W, _p(bbox), _stream()), "vv_mask_bbox")
    return bbox


def mask_tile_union(mask2d, tile):
    """mask2d [T,H,W] u8 -> [ceil(H/tile), ceil(W/tile)] u8 on the device: 1 where any frame has a non-zero byte in that tile, else 0."""
    _need_cuda(mask2d)
    T, H, W = mask2d.shape
    occ = torch.empty(((H + tile - 1) // tile, (W + tile - 1) // tile), dtype=torch.uint8, device=mask2d.device)
    with _Prof("mask_tile_union", 0.0, T * H * W + occ.numel()):
        _check(lib().vv_mask_tile_union(_p(mask2d), T, H, W, int(tile), _p(occ), _stream()), "vv_mask_tile_union")
    return occ


def mask_bbox_tiles(mask2d, tile, tiles, K):
    """mask2d [T,H,W] u8, tiles [n,3] int32 (ty, tx, label) on the device -> [T,K,4] int32: half-open (y0, x0, y1, x1) of label k's non-zero bytes in
    frame t, (0, 0, 0, 0) when there is none.  Reads only the listed tiles; entries outside the grid or with a label outside [0, K) are ignored."""
    _need_cuda(mask2d, tiles)
    T, H, W = mask2d.shape
    if tiles.dtype != torch.int32 or tiles.dim() != 2 or tiles.shape[1] != 3 or not tiles.is_contiguous():
        raise RuntimeError("mask_bbox_tiles: tiles must be a contiguous [n,3] int32 tensor")
    n = tiles.shape[0]
    if n == 0:                                   # no tile to read (an empty tensor has no address to hand over)
        return torch.zeros((T, K, 4), dtype=torch.int32, device=mask2d.device)
    bbox = torch.empty((T, K, 4), dtype=torch.int32, device=mask2d.device)
    with _Prof("mask_bbox_tiles", 0.0, n * T * tile * tile + bbox.numel() * 4):
        _check(lib().vv_mask_bbox_tiles(_p(mask2d), T, H, W, int(tile), _p(tiles), n, int(K), _p(bbox), _stream()), "vv_mask_bbox_tiles")
    return bbox


def roi_paste_composite(patch, orig, mask2d, offsets, h, w, feather_px, out=None):
    """patch [T,Hm,Wm,3] u8 (model output of the window), orig [T,H0,W0,3] u8, mask2d [T,H0,W0] u8, offsets [T,2] int32 (oy, ox) -> [T,H0,W0,3]:
    resize_u8(patch -> h, w) pasted at each frame's offset into orig, then feather_composite(., orig, mask2d, feather_px) -- in one pass.
    feather_px < 0: plain paste (mask2d may be None).  out: an optional [T,H0,W0,3] u8 buffer to write (not orig)."""
    _need_cuda(patch, orig, mask2d, offsets, out)
    T, Hm, Wm, _ = patch.shape
    _, H0, W0, _ = orig.shape
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (T, 2) or orig.shape[0] != T or patch.shape[3] != 3 or orig.shape[3] != 3 or (mask2d is not None and tuple(mask2d.shape) != (T, H0, W0)):
        raise RuntimeError("roi_paste_composite: shapes / dtypes do not match")
    out = _out_like("roi_paste_composite", out, orig, "orig")
    with _Prof("roi_paste_composite", 0.0, T * H0 * W0 * (3 + 1 + 3) + patch.numel()):
        _check(lib().vv_roi_paste_composite(_p(patch), Hm, Wm, _p(orig), _p(mask2d), _p(offsets), T, H0, W0, int(h), int(w), feather_px, _p(out),
                                            _stream()), "vv_roi_paste_composite")
    return out


def chamfer_dt(bin_u8, R, out=None):
    _need_cuda(bin_u8)
    T, H, W = bin_u8.shape
    out = _own_out(out, (T, H, W), torch.float32, bin_u8, "chamfer_dt")
    _check(lib().vv_chamfer_dt(_p(bin_u8), T, H, W, R, _p(out), _stream()), "vv_chamfer_dt")
    return out


def preprocess(dtype, frames, mask2d, want_img=True, want_masked=True, img=None, masked=None):
    _need_cuda(frames, mask2d)
    T, H, W, _ = frames.shape
    img = _own_out(img, (T, H, W, 8), h16(dtype), frames, "preprocess (img)") if want_img else None
    msk = _own_out(masked, (T, H, W, 8), h16(dtype), frames, "preprocess (masked)") if want_masked else None
    _check(lib().vv_preprocess(_p(frames), _p(mask2d), T, H, W, _p(img), _p(msk), dtype, _stream()), "vv_preprocess")
    return img, msk


def brushnet_input(dtype, lat, cond, mask2d, H, W, out=None):
    _need_cuda(lat, cond, mask2d)
    F, h, w, _ = lat.shape
    out = _own_out(out, (F, h, w, 16), h16(dtype), lat, "brushnet_input")
    _check(lib().vv_brushnet_input(_p(lat), _p(cond), _p(mask2d), F, h, w, H, W, _p(out), dtype, _stream()), "vv_brushnet_input")
    return out


def pad_channels(dtype, x, cpad, scale=1.0, out=None):
    _need_cuda(x)
    cin = x.shape[-1]
    rows = x.numel() // cin
    out = _own_out(out, x.shape[:-1] + (cpad,), h16(dtype), x, "pad_channels")
    _check(lib().vv_pad_channels(_p(x), rows, cin, cpad, scale, _p(out), dtype, _stream()), "vv_pad_channels")
    return out


def window_average(value, count, out=None):
    """value fp32 [T, ...], count fp32 [T] -> value / count per frame."""
    _need_cuda(value, count)
    T = value.shape[0]
    out = _own_out(out, value.shape, value.dtype, value, "window_average")
    _check(lib().vv_window_average(_p(value), _p(count), T, value.numel() // T, _p(out), _stream()), "vv_window_average")
    return out


def pad_channels_f32(x, cpad, scale=1.0, out=None):
    _need_cuda(x)
    cin = x.shape[-1]
    rows = x.numel() // cin
    out = _own_out(out, x.shape[:-1] + (cpad,), torch.float32, x, "pad_channels_f32")
    _check(lib().vv_pad_channels_f32(_p(x), rows, cin, cpad, scale, _p(out), _stream()), "vv_pad_channels_f32")
    return out


def split_f32(dtype, x, lo_scale, hi=None, lo=None):
    """fp32 tensor -> (hi, lo) h16 tensors of the same shape: hi = h16(x), lo = h16((x - hi) * lo_scale)."""
    _need_cuda(x)
    assert x.dtype == torch.float32
    hi = _own_out(hi, x.shape, h16(dtype), x, "split_f32 (hi)")
    lo = _own_out(lo, x.shape, h16(dtype), x, "split_f32 (lo)")
    _check(lib().vv_split_f32(_p(x), x.numel(), lo_scale, _p(hi), _p(lo), dtype, _stream()), "vv_split_f32")
    return hi, lo


def _packing():
    from . import packing
    return packing


def spatial_chain_c320(dtype, o, t_in, x, stream_w, params, *, res1=None, out_dtype=torch.float32, o_hw=0, out=None):
    """The fused tail of a level-0 spatial transformer block (vv_chain.hip): attn1 out-proj + residual, cross-attention to the text tokens,
    GEGLU feed-forward, proj_out + block residual in ONE kernel.  o: h16 [M,320] (o_hw = 0), or head-major [M / o_hw, 8, o_hw, 40] as vv_attention writes it
    with o_hs = o_hw * 40; t_in, x (, res1): fp32 [M,320].  out: write into the caller's contiguous [M,320] tensor (its dtype is the output type)."""
    _need_cuda(o, t_in, x, stream_w, params, res1)
    M, Cc = t_in.shape
    assert o.numel() == M * Cc and x.shape == (M, Cc) and o.dtype == h16(dtype) and t_in.dtype == x.dtype == torch.float32
    assert (o.shape == (M, Cc)) if o_hw == 0 else (M % o_hw == 0 and o.is_contiguous())
    out = _own_out(out, (M, Cc), out_dtype if out is None else out.dtype, x, "spatial_chain_c320")
    cp = ChainParams(o=_p(o), t_in=_p(t_in), x=_p(x), res1=_p(res1), out=_p(out),
                     out_dtype=dt_of(out), stream=_p(stream_w), params=_p(params), M=M, C=Cc, heads=8, text_len=77,
                     n_slabs=stream_w.shape[0], n_params=params.numel(), layout=CHAIN_LAYOUT_IDS[_packing().CHAIN_LAYOUT], o_hw=int(o_hw))
    flops = 2.0 * M * Cc * Cc * (1 + 1 + 1 + 12 + 1) + 4.0 * M * 77 * Cc
    with _Prof("spatial_chain_fused[c320]", flops, M * Cc * (2 + 4 + 4 + out.element_size())):
        _check(lib().vv_spatial_chain_c320(C.byref(cp), dtype, _stream()), "vv_spatial_chain_c320")
    return out


CHAIN_FRONT_MIN_HW = 9      # vv_spatial_chain_front_c320 stages the GroupNorm affine rows of the <= 127 / HW + 2 frames a 128-token block touches: 16 fit


def spatial_chain_front_c320(dtype, x, gamma, beta, groups, eps, stream_w, params, *, F, HW, partials=None, t_out=None, qkv_out=None):
    """The fused front of a level-0 spatial transformer block (vv_chain.hip): per-frame GroupNorm statistics -> per-channel affine -> ONE kernel for
    GroupNorm apply + proj_in + LayerNorm + the fused q|k|v projection.  Returns (t fp32 [M,320] = the block's residual stream, qkv h16 head-major
    [F][3][8][HW][40]).  HW >= CHAIN_FRONT_MIN_HW tokens per frame: the library refuses smaller frames (nn.SpatialTransformer runs them layer by layer).
    t_out / qkv_out: write into the caller's contiguous tensors of those shapes instead of fresh ones."""
    _need_cuda(x, gamma, beta, stream_w, params)
    M, Cc = x.shape
    assert M == F * HW and x.dtype == torch.float32
    aff = torch.empty((F, 2, Cc), dtype=torch.float32, device=x.device)
    if partials is not None:      # the producing convolution left per-channel partial sums of x (conv_gemm(gn_partials=)): no statistics pass over HBM
        assert (partials.F, partials.HW, partials.C) == (F, HW, Cc), "GroupNorm partials do not describe this tensor"
        keep = partials.finalize(groups, eps)
        fin = _p(keep)
    else:
        fin, keep = _gn_stats(dtype, x, gamma, beta, groups, eps, F, HW, 0)
    _check(lib().vv_gn_affine_frames(fin, _p(gamma), _p(beta), Cc, groups, F, _p(aff), _stream()), "vv_gn_affine_frames")
    t = _own_out(t_out, (M, Cc), torch.float32, x, "spatial_chain_front_c320 (t_out)")
    qkv = _own_out(qkv_out, (F, 3, 8, HW, Cc // 8), h16(dtype), x, "spatial_chain_front_c320 (qkv_out)")
    fp = ChainFrontParams(x=_p(x), gn_affine=_p(aff), t_out=_p(t), qkv=_p(qkv), stream=_p(stream_w),
                          params=_p(params), M=M, HW=HW, C=Cc, heads=8, n_slabs=stream_w.shape[0], n_params=params.numel())
    with _Prof("spatial_chain_front_fused[c320]", 2.0 * M * Cc * Cc * 4, M * Cc * (4 + 4 + 6)):
        _check(lib().vv_spatial_chain_front_c320(C.byref(fp), dtype, _stream()), "vv_spatial_chain_front_c320")
    return t, qkv


def split3(dtype, x, out=None):
    """[M, C] fp32 (or h16) -> [M, 3C] h16 = [hi | (x - hi) * 2^4 | hi * 2^-10]: the A operand of a K-concatenated split-precision GEMM (vv_split3)."""
    _need_cuda(x)
    assert x.dim() == 2 and x.is_contiguous()
    M, Cc = x.shape
    out = _own_out(out, (M, 3 * Cc), h16(dtype), x, "split3")
    with _Prof("split3", 0.0, x.numel() * (x.element_size() + 6)):
        _check(lib().vv_split3(_p(x), dt_of(x), M, Cc, _p(out), dtype, _stream()), "vv_split3")
    return out


def decode_blend(dec, w, acc):
    """dec [T,H,W,ld] fp32 ; w [T] fp32 ; acc [T,H,W,3] fp32 updated in place."""
    _need_cuda(dec, w, acc)
    T, H, W, ld = dec.shape
    _check(lib().vv_decode_blend(_p(dec), ld, _p(w), T, H * W, _p(acc), _stream()), "vv_decode_blend")
    return acc


def blur_compose(pix01, orig, mask2d, taps21, out=None):
    _need_cuda(pix01, orig, mask2d)
    T, H, W, _ = pix01.shape
    tmp = torch.empty((T, H, W), dtype=torch.float32, device=pix01.device)
    out = _own_out(out, (T, H, W, 3), torch.uint8, pix01, "blur_compose")
    taps = (C.c_float * 21)(*[float(x) for x in taps21])
    _check(lib().vv_blur_compose(_p(pix01), _p(orig), _p(mask2d), T, H, W, taps, _p(tmp), _p(out), _stream()), "vv_blur_compose")
    return out


# ---- K9/K10: RAFT / flow-guided propagation kernels ----------------------------------------------------------------
def avgpool2(x, out=None):
    """[N,h,w] fp32 -> [N,h//2,w//2]."""
    _need_cuda(x)
    N, h, w = x.shape
    out = _own_out(out, (N, h // 2, w // 2), torch.float32, x, "avgpool2")
    with _Prof("avgpool2[corr pyramid]", 0.0, x.numel() * 5):
        _check(lib().vv_avgpool2_f32(_p(x), N, h, w, _p(out), _stream()), "vv_avgpool2_f32")
    return out


def corr_lookup(dtype, pyr, coords, cpad=384, out=None):
    """pyr: 4 fp32 tensors [N,h_l,w_l]; coords [N,2] fp32 (x,y) -> h16 [N,cpad] (324 real channels)."""
    _need_cuda(*pyr, coords)
    N, h, w = pyr[0].shape
    out = _own_out(out, (N, cpad), h16(dtype), coords, "corr_lookup")
    with _Prof("corr_lookup", 0.0, N * (4 * 100 * 4 + 324 * 2 + 8)):
        _check(lib().vv_corr_lookup(_p(pyr[0]), _p(pyr[1]), _p(pyr[2]), _p(pyr[3]), h, w, _p(coords), N, cpad, _p(out), dtype, _stream()),
               "vv_corr_lookup")
    return out


def raft_ctx_split(dtype, cn, net, net16, xbuf):
    _need_cuda(cn, net, net16, xbuf)
    with _Prof("raft_elementwise", 0.0, cn.numel() * 4 + net.numel() * 6 + xbuf.shape[0] * 256):
        _check(lib().vv_raft_ctx_split(_p(cn), cn.shape[0], _p(net), _p(net16), _p(xbuf), dtype, _stream()), "vv_raft_ctx_split")


def raft_flow_prep(dtype, coords1, w, h, flow8, xbuf):
    _need_cuda(coords1, flow8, xbuf)
    with _Prof("raft_elementwise", 0.0, coords1.numel() * 4 + flow8.numel() * 2 + coords1.shape[0] * 4):
        _check(lib().vv_raft_flow_prep(_p(coords1), coords1.shape[0], w, h, _p(flow8), _p(xbuf), dtype, _stream()), "vv_raft_flow_prep")


def gru_rh(dtype, zr, h, rh):
    _need_cuda(zr, h, rh)
    with _Prof("raft_elementwise", 0.0, h.numel() * (2 + 4 + 2)):
        _check(lib().vv_gru_rh(_p(zr), _p(h), h.shape[0], _p(rh), dtype, _stream()), "vv_gru_rh")


def gru_update(dtype, zr, q, h, h16_out):
    _need_cuda(zr, q, h, h16_out)
    with _Prof("raft_elementwise", 0.0, h.numel() * (4 + 2 + 4 + 4 + 2)):
        _check(lib().vv_gru_update(_p(zr), _p(q), h.shape[0], _p(h), _p(h16_out), dtype, _stream()), "vv_gru_update")


def add_flow(coords1, dflow):
    _need_cuda(coords1, dflow)
    with _Prof("raft_elementwise", 0.0, coords1.numel() * 12):
        _check(lib().vv_add_flow(_p(coords1), _p(dflow), dflow.shape[-1], coords1.shape[0], _stream()), "vv_add_flow")


def add_relu(a, b, out=None):
    _need_cuda(a, b)
    out = _own_out(out, a.shape, a.dtype, a, "add_relu")
    with _Prof("add_relu", 0.0, a.numel() * 12):
        _check(lib().vv_add_relu_f32(_p(a), _p(b), _p(out), a.numel(), _stream()), "vv_add_relu_f32")
    return out


def convex_upsample(coords1, mask, h, w, F=1, out=None):
    """coords1 [F*h*w, 2], mask [F*h*w, 576] -> flow [8h, 8w, 2] (F = 1) or [F, 8h, 8w, 2]."""
    _need_cuda(coords1, mask)
    out = _own_out(out, (F, 8 * h, 8 * w, 2), torch.float32, coords1, "convex_upsample")
    with _Prof("convex_upsample", 0.0, mask.numel() * mask.element_size() + coords1.numel() * 4 + out.numel() * 4):
        _check(lib().vv_convex_upsample(_p(coords1), _p(mask), F, h, w, _p(out), _stream()), "vv_convex_upsample")
    return out[0] if F == 1 else out


def fb_valid(f_ab, f_ba, out=None):
    _need_cuda(f_ab, f_ba)
    H, W, _ = f_ab.shape
    out = _own_out(out, (H, W), torch.uint8, f_ab, "fb_valid")
    with _Prof("fb_valid[bilinear warp of the backward flow]", 0.0, H * W * (8 + 8 + 1)):
        _check(lib().vv_fb_valid(_p(f_ab), _p(f_ba), H, W, _p(out), _stream()), "vv_fb_valid")
    return out


def prop_fill(cur_t, cur_nb, known_t, known_nb, valid, flow, filled_t):
    _need_cuda(cur_t, cur_nb, known_t, known_nb, valid, flow, filled_t)
    H, W, _ = cur_t.shape
    with _Prof("prop_fill[bilinear warp]", 0.0, H * W * (3 + 3 + 2 + 1 + 8 + 3)):
        _check(lib().vv_prop_fill(_p(cur_t), _p(cur_nb), _p(known_t), _p(known_nb), _p(valid), _p(flow), H, W, _p(filled_t), _stream()), "vv_prop_fill")


def prop_combine(orig, a, b, fa, fb, hole, mean3, out=None, filled=None, want_filled=True):
    """-> (out u8 [H,W,3], filled u8 [H,W]); want_filled=False: the library gets no `filled` map (None is returned in its place)"""
    _need_cuda(orig, a, b, fa, fb, hole, mean3)
    H, W, _ = orig.shape
    out = _own_out(out, (H, W, 3), torch.uint8, orig, "prop_combine (out)")
    filled = _own_out(filled, (H, W), torch.uint8, orig, "prop_combine (filled)") if want_filled else None
    with _Prof("prop_combine", 0.0, H * W * (3 * 3 + 3 + 3 + 1)):
        _check(lib().vv_prop_combine(_p(orig), _p(a), _p(b), _p(fa), _p(fb), _p(hole), H, W, _p(mean3), _p(out), _p(filled), _stream()), "vv_prop_combine")
    return out, filled


def masked_sum_u8(frame, hole, out=None):
    """-> int64 tensor [4] (sum r, g, b over non-hole pixels, count) on the device."""
    _need_cuda(frame, hole)
    sums = _own_out(out, (4,), torch.int64, frame, "masked_sum_u8")
    _check(lib().vv_masked_sum_u8(_p(frame), _p(hole), hole.numel(), _p(sums), _stream()), "vv_masked_sum_u8")
    return sums


def u8_to_f32(x, out=None):
    _need_cuda(x)
    out = _own_out(out, x.shape, torch.float32, x, "u8_to_f32")
    _check(lib().vv_u8_to_f32(_p(x), _p(out), x.numel(), _stream()), "vv_u8_to_f32")
    return out


def u8_is_zero(x, out=None):
    _need_cuda(x)
    out = _own_out(out, x.shape, x.dtype, x, "u8_is_zero")
    _check(lib().vv_u8_is_zero(_p(x), _p(out), x.numel(), _stream()), "vv_u8_is_zero")
    return out


def raft_prep(dtype, img, out=None):
    """u8 [..., 3] -> h16 [..., 8] scaled to [-1,1]."""
    _need_cuda(img)
    out = _own_out(out, img.shape[:-1] + (8,), h16(dtype), img, "raft_prep")
    with _Prof("raft_prep", 0.0, img.numel() + out.numel() * 2):
        _check(lib().vv_raft_prep(_p(img), img.numel() // 3, _p(out), dtype, _stream()), "vv_raft_prep")
    return out


# ---- SAM 2 (include/vvhip.h "SAM 2" section) ---------------------------------------------------------------------
def u8_normalize(dtype, img_u8, mean, std, cpad=8, s2d=1, out=None):
    """uint8 [H, W, 3] -> h16 [(H/s2d)*(W/s2d), cpad] = ((x / 255) - mean) / std; s2d > 1: space-to-depth blocks, channel (dy*s2d + dx)*3 + c."""
    _need_cuda(img_u8)
    H, W = img_u8.shape[:2]
    out = _own_out(out, ((H // s2d) * (W // s2d), cpad), h16(dtype), img_u8, "u8_normalize")
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[1.0 / float(v) for v in std])
    _check(lib().vv_u8_normalize(_p(img_u8), H, W, m, s, _p(out), cpad, s2d, dtype, _stream()), "vv_u8_normalize")
    return out


def layernorm_ex(dtype, x, gamma, beta, eps, act=ACT_NONE, out_dtype=None, cpad=None, out=None):
    """LayerNorm over the last dim of fp32 [M, C] (any C) + optional activation; out_dtype None = h16, torch.float32 = fp32;
    cpad: output row length (zero padded channels, for a following conv whose input channels are padded)."""
    _need_cuda(x, gamma, beta)
    M, Cc = x.shape
    cp = Cc if cpad is None else cpad
    out = _own_out(out, (M, cp), h16(dtype) if out_dtype is None else out_dtype, x, "layernorm_ex")
    _check(lib().vv_layernorm_ex(_p(x), M, Cc, _p(gamma), _p(beta), eps, act, _p(out), dt_of(out), cp, dtype, _stream()), "vv_layernorm_ex")
    return out


def maxpool2x2(x, B, H, W, Cc=None, in_bs=0, x_off=0, out=None):
    """B images [H, W, C] (fp32 or h16; image b starts x_off + b * in_bs elements into x, in_bs = 0: contiguous) -> [B*(H/2)*(W/2), C]."""
    _need_cuda(x)
    Cc = x.shape[-1] if Cc is None else Cc
    out = _own_out(out, (B * (H // 2) * (W // 2), Cc), x.dtype, x, "maxpool2x2")
    _check(lib().vv_maxpool2x2(x.data_ptr() + x_off * x.element_size(), dt_of(x), B, H, W, Cc, in_bs, _p(out), _stream()),
           "vv_maxpool2x2")
    return out


def rope_apply(dtype, x, rows_rope, cos_sin, D, col0=0, ld=None):
    """in place: rows < rows_rope of the h16 matrix x, columns col0 .. col0 + D, rotated pairwise by cos_sin [n, D/2, 2] (row r uses r % n)."""
    _need_cuda(x, cos_sin)
    _check(lib().vv_rope_apply(_p(x), rows_rope, x.shape[-1] if ld is None else ld, col0, D, _p(cos_sin), cos_sin.shape[0], dtype,
                               _stream()), "vv_rope_apply")
    return x


def dwconv(x, H, W, w, bias, out=None):
    _need_cuda(x, w, bias)
    out = _own_out(out, x.shape, torch.float32, x, "dwconv")
    _check(lib().vv_dwconv(_p(x), H, W, x.shape[-1], _p(w), _p(bias), w.shape[-1], _p(out), _stream()), "vv_dwconv")
    return out


def pixel_shuffle2(dtype, y, bias, h, w, add=None, act=ACT_NONE, out_dtype=torch.float32, out=None):
    _need_cuda(y, bias, add)
    Cc = y.shape[-1] // 4
    out = _own_out(out, (4 * h * w, Cc), out_dtype, y, "pixel_shuffle2")
    _check(lib().vv_pixel_shuffle2(_p(y), _p(bias), _p(add), h, w, Cc, act, _p(out), dt_of(out), dtype, _stream()), "vv_pixel_shuffle2")
    return out


def resize_bilinear_f32(src, Hs, Ws, Hd, Wd, out=None):
    """fp32 [Hs*Ws, C] -> [Hd*Wd, C], F.interpolate(mode="bilinear", align_corners=False)."""
    _need_cuda(src)
    Cc = src.shape[-1]
    out = _own_out(out, (Hd * Wd, Cc), torch.float32, src, "resize_bilinear_f32")
    _check(lib().vv_resize_bilinear_f32(_p(src), Hs, Ws, Cc, _p(out), Hd, Wd, _stream()), "vv_resize_bilinear_f32")
    return out


def mask_mem_input(dtype, logits, binarize, scale, bias, out=None):
    _need_cuda(logits)
    n = logits.numel()
    out = _own_out(out, (n, 8), h16(dtype), logits, "mask_mem_input")
    _check(lib().vv_mask_mem_input(_p(logits), n, int(bool(binarize)), scale, bias, _p(out), dtype, _stream()), "vv_mask_mem_input")
    return out


def act_inplace(x, act):
    _need_cuda(x)
    _check(lib().vv_act(_p(x), dt_of(x), x.numel(), act, _stream()), "vv_act")
    return x


def prompt_points(coords, labels, inv_size, gauss, table, out=None):
    _need_cuda(coords, labels, gauss, table)
    P, D = labels.numel(), table.shape[-1]
    out = _own_out(out, (P, D), torch.float32, coords, "prompt_points")
    _check(lib().vv_prompt_points(_p(coords), _p(labels), P, inv_size, _p(gauss), _p(table), D, _p(out), _stream()), "vv_prompt_points")
    return out


def sine_pe_1d(pos, dim, temperature=10000.0, out=None):
    _need_cuda(pos)
    out = _own_out(out, (pos.numel(), dim), torch.float32, pos, "sine_pe_1d")
    _check(lib().vv_sine_pe_1d(_p(pos), pos.numel(), dim, temperature, _p(out), _stream()), "vv_sine_pe_1d")
    return out


def sam_select(masks, iou, obj_logit, multimask, delta, thresh, out=None):
    _need_cuda(masks, iou, obj_logit)
    sel = _own_out(out, (4,), torch.int32, masks, "sam_select")
    _check(lib().vv_sam_select(_p(masks), masks.shape[-1], masks.shape[0], _p(iou), _p(obj_logit), int(bool(multimask)), delta, thresh, _p(sel),
                               _stream()), "vv_sam_select")
    return sel


def sam_pick(masks, sel, no_obj_score, out=None):
    _need_cuda(masks, sel)
    out = _own_out(out, (masks.shape[-1],), torch.float32, masks, "sam_pick")
    _check(lib().vv_sam_pick(_p(masks), masks.shape[-1], _p(sel), no_obj_score, _p(out), _stream()), "vv_sam_pick")
    return out


def select_f32(a, b, flag, out=None):
    _need_cuda(a, b, flag)
    out = _own_out(out, a.shape, a.dtype, a, "select_f32")
    _check(lib().vv_select_f32(_p(a), _p(b), _p(flag), a.numel(), _p(out), _stream()), "vv_select_f32")
    return out


def add_rowvec_unless(x, vec, score):
    """x[m] += vec unless score[0] > 0 (score: fp32 on the device)."""
    _need_cuda(x, vec, score)
    _check(lib().vv_add_rowvec_unless(_p(x), _p(vec), _p(score), x.shape[0], x.shape[1], _stream()), "vv_add_rowvec_unless")
    return x


def clamp_f32(x, lo, hi, out=None):
    _need_cuda(x)
    out = _own_out(out, x.shape, x.dtype, x, "clamp_f32")
    _check(lib().vv_clamp_f32(_p(x), x.numel(), lo, hi, _p(out), _stream()), "vv_clamp_f32")
    return out


def fill_holes(mask, H, W, max_area, ws=None):
    """in place on fp32 [H*W].  ws: the caller's int32 [3*H*W] workspace instead of a fresh one."""
    _need_cuda(mask)
    ws = _own_out(ws, (3 * H * W,), torch.int32, mask, "fill_holes (ws)")
    _check(lib().vv_fill_holes(_p(mask), H, W, max_area, _p(ws), _stream()), "vv_fill_holes")
    return mask


def hyper_masks(hyper, up, out=None):
    """masks [nm, HW] = hyper [nm, C] @ up [HW, C]^T, fp32."""
    _need_cuda(hyper, up)
    nm, Cc = hyper.shape
    out = _own_out(out, (nm, up.shape[0]), torch.float32, up, "hyper_masks")
    _check(lib().vv_hyper_masks(_p(hyper), _p(up), up.shape[0], Cc, nm, _p(out), _stream()), "vv_hyper_masks")
    return out


def attention_split_kv(dtype, q, k, v, out, *, heads, Nq, Nkv, D, S, q_rs, k_rs, v_rs, o_rs, q_hs=0, k_hs=0, v_hs=0, scale=None):
    """one batch of `heads` heads over a LONG key sequence, the keys split into S equal chunks that run as S batches of vv_attention (S x the blocks)
    and are merged through their log-sum-exps (vv_attention_merge).  Nkv % S == 0.  q / k / v / out: row-major [N, heads * D]-style matrices."""
    if Nkv % S:
        raise RuntimeError(f"attention_split_kv: Nkv={Nkv} is not a multiple of S={S}")
    chunk = Nkv // S
    parts = torch.empty((S, Nq, o_rs), dtype=h16(dtype), device=q.device)
    lse = torch.empty((S, heads, Nq), dtype=torch.float32, device=q.device)
    attention(dtype, q, k, v, parts, B=S, heads=heads, Nq=Nq, Nkv=chunk, D=D, q_bs=0, k_bs=chunk * k_rs, v_bs=chunk * v_rs, o_bs=Nq * o_rs,
              q_rs=q_rs, k_rs=k_rs, v_rs=v_rs, o_rs=o_rs, q_hs=q_hs, k_hs=k_hs, v_hs=v_hs, scale=scale, lse=lse)
    _check(lib().vv_attention_merge(_p(parts), _p(lse), S, heads, Nq, D, o_rs, _p(out), dtype, _stream()), "vv_attention_merge")
    return out


def ycbcr_to_rgb(y, cb, cr, hshift, vshift, full_range=False, out=None):
    """planar uint8 YCbCr on the device (y [T, H, W], cb / cr [T, ceil(H >> vshift), ceil(W >> hshift)]) -> RGB uint8 [T, H, W, 3] (row n3)."""
    _need_cuda(y, cb, cr)
    T, H, W = y.shape
    out = _own_out(out, (T, H, W, 3), torch.uint8, y, "ycbcr_to_rgb")
    _check(lib().vv_ycbcr_to_rgb(_p(y), _p(cb), _p(cr), T, H, W, int(hshift), int(vshift), int(bool(full_range)), _p(out), _stream()), "vv_ycbcr_to_rgb")
    return out


def sam2_maskdown(dtype, logits, lo, S, binarize, scale, bias, l1, l2, eps=1e-6, mid=None, out=None):
    """fused front of the SAM 2 memory encoder's mask path (vv_sam2_maskdown): logits fp32 [lo*lo] -> h16 [(S/4)^2, 16].  l1 / l2: (w, b, gamma, beta)."""
    _need_cuda(logits, *l1, *l2)
    mid = _own_out(mid, ((S // 2) ** 2, 8), h16(dtype), logits, "sam2_maskdown (mid)")      # the first stage's output, a workspace to the caller
    out = _own_out(out, ((S // 4) ** 2, 16), h16(dtype), logits, "sam2_maskdown (out)")
    _check(lib().vv_sam2_maskdown(_p(logits), lo, S, int(bool(binarize)), scale, bias, _p(l1[0]), _p(l1[1]), _p(l1[2]), _p(l1[3]), _p(l2[0]), _p(l2[1]),
                                  _p(l2[2]), _p(l2[3]), eps, _p(mid), _p(out), dtype, _stream()), "vv_sam2_maskdown")
    return out
