"""ctypes binding of libmtt_hip.so (include/mtt_hip.h).

`call(name, **fields)` fills the descriptor struct of entry point `mtt_<name>` from keyword
arguments — torch tensors (or views: only the base address is used) for pointer fields, ints /
floats for the rest — launches it on torch's current HIP stream and raises on a non-zero status.

Every export is declared once: the family tables (DESCS, POSITIONAL, DESC_EXTRA, POSTPROC, EVAL,
AUGMENT, CS3D, RENDER, WS_QUERIES) and HELPERS make up SIGNATURES, symbol -> (restype, argtypes,
descriptor struct), and `load()` sets every restype / argtypes from it in one loop, checks every
descriptor size of SIZE_QUERIES in another, and nothing assigns a signature afterwards.  One
function, `_fill`, turns keyword fields into a descriptor for every launcher and size query.

There is NO fallback: if the shared library is missing or a tensor is not on a HIP device the
call raises.  (tests/ may monkeypatch `call` with the CPU emulator in oracle/abi_emul.py to
exercise the host-side wiring without a GPU; the product never does.)
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmtt_hip.so")

ABI_VERSION = 17
F32, BF16, SPLIT = 0, 1, 2
PREC_BF16, PREC_X3 = 0, 1
OP_K, OP_R, OP_CONV_K, OP_CONV_R = 0, 1, 2, 3
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_DAUX, ACT_MUL_AUX = 0, 1, 2, 3, 4, 5, 6
STORE_ROWS, STORE_PIXSHUF2 = 0, 1
GEMM_AUTO, GEMM_GENERAL, GEMM_DMA256, GEMM_DMA128, GEMM_GENERAL_EPILOGUE = 0, 1, 3, 4, 11
ATTN_AUTO, ATTN_PLAIN = 0, 1

i32, i64, f32, ptr = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class ConvGeom(C.Structure):
    _fields_ = [("H", i32), ("W", i32), ("C", i32), ("Cp", i32), ("dil", i32), ("flip", i32)]


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", ptr), ("B", ptr), ("D", ptr),
        ("M", i32), ("N", i32), ("K", i32),
        ("a_op", i32), ("b_op", i32),
        ("a_dtype", i32), ("b_dtype", i32), ("d_dtype", i32),
        ("prec", i32),
        ("lda", i64), ("ldb", i64), ("ldd", i64),
        ("a_mb", i32), ("a_bs", i64),
        ("d_mb", i32), ("d_bs", i64),
        ("batch", i32), ("batch_inner", i32),
        ("a_zo", i64), ("a_zi", i64), ("b_zo", i64), ("b_zi", i64), ("d_zo", i64), ("d_zi", i64),
        ("conv", ConvGeom),
        ("alpha", f32),
        ("colscale", ptr), ("colshift", ptr), ("col_zo", i64), ("col_zi", i64),
        ("act", i32),
        ("aux_in", ptr), ("aux_out", ptr), ("aux_dtype", i32), ("ldaux", i64), ("aux_zo", i64), ("aux_zi", i64),
        ("rowscale", ptr), ("n_prompt", i32),
        ("resid", ptr), ("ldr", i64), ("r_mb", i32), ("r_bs", i64), ("r_zo", i64), ("r_zi", i64),
        ("n_store", i32), ("store_mode", i32),
        ("ps_H", i32), ("ps_W", i32), ("ps_Co", i32),
        ("variant", i32),
        ("A_lo", ptr), ("B_lo", ptr), ("D_lo", ptr),
        ("colsum_out", ptr), ("colsum_ws", ptr),
        ("a_scale", ptr), ("a_shift", ptr), ("a_act", i32), ("a_aux16", ptr), ("ld_a16", i64),
        ("skip_scale", ptr), ("skip_mb", i32), ("skip_prompt", i32), ("skip_row0", i64),
    ]


class AttnDesc(C.Structure):
    _fields_ = [("qkv", ptr), ("out", ptr), ("rawlog", ptr), ("lse", ptr),
                ("B", i32), ("N", i32), ("nH", i32), ("T", i32), ("dtype", i32), ("prec", i32), ("scale", f32),
                ("variant", i32), ("qkv_lo", ptr), ("out_lo", ptr), ("skip_scale", ptr)]


class SoftmaxDesc(C.Structure):
    _fields_ = [("S", ptr), ("P", ptr), ("dP", ptr), ("dS", ptr), ("extra", ptr),
                ("rows", i64), ("cols", i64), ("ld", i64), ("s_dtype", i32), ("p_dtype", i32), ("scale", f32),
                ("rows_per_mat", i64), ("extra_rows", i32), ("extra_ld", i64)]


class LnDesc(C.Structure):
    _fields_ = [("x", ptr), ("y", ptr), ("gamma", ptr), ("beta", ptr), ("mean", ptr), ("rstd", ptr),
                ("dy", ptr), ("dx", ptr), ("dgamma", ptr), ("dbeta", ptr),
                ("rows", i64), ("C", i32), ("ldx", i64), ("ldy", i64), ("y_dtype", i32), ("eps", f32), ("dx_in", ptr), ("ws", ptr),
                ("y_lo", ptr), ("y32", ptr), ("ldy32", i64)]


class ChanLogitDesc(C.Structure):
    _fields_ = [("q", ptr), ("xn", ptr), ("rawchan", ptr),
                ("B", i32), ("T", i32), ("N", i32), ("C", i32), ("h", i32), ("w", i32), ("nh", i32), ("nw", i32),
                ("dtype", i32), ("ldq", i64), ("ws", ptr), ("xn_lo", ptr)]


class ModulateDesc(C.Structure):
    _fields_ = [("x", ptr), ("x_ld", i64), ("x_bs", i64), ("rawlog", ptr), ("rawchan", ptr), ("out", ptr),
                ("B", i32), ("T", i32), ("N", i32), ("C", i32), ("h", i32), ("w", i32), ("nh", i32), ("nw", i32),
                ("out_dtype", i32), ("hg", i32), ("out_lo", ptr)]


class CtrDesc(C.Structure):
    _fields_ = [("fea", ptr), ("out", ptr), ("wmix", ptr), ("T", i32), ("B", i32), ("rows_per_b", i64), ("ld", i64),
                ("C", i32), ("fea_dtype", i32), ("accumulate", i32), ("out_dtype", i32)]


class ResizeDesc(C.Structure):
    _fields_ = [("in_", ptr), ("out", ptr), ("B", i32), ("C", i32), ("Hin", i32), ("Win", i32), ("Hout", i32), ("Wout", i32),
                ("ld_in", i64), ("ld_out", i64), ("in_dtype", i32), ("out_dtype", i32), ("out_nchw", i32), ("accumulate", i32)]


setattr(ResizeDesc, "in", ResizeDesc.in_)        # `in` is a keyword: callers pass **{"in": t}, and it names the same field


class BnDesc(C.Structure):
    _fields_ = [("x", ptr), ("y", ptr), ("dy", ptr), ("dx", ptr),
                ("mean_out", ptr), ("m2_out", ptr), ("mean", ptr), ("rstd", ptr), ("gamma", ptr), ("beta", ptr),
                ("dsum", ptr), ("dsumxh", ptr),
                ("rows", i64), ("C", i32), ("ld", i64), ("dtype", i32), ("act", i32),
                ("Z", i32), ("x_zs", i64), ("p_zs", i64), ("g_dtype", i32)]


class DwconvDesc(C.Structure):
    _fields_ = [("x", ptr), ("w", ptr), ("y", ptr), ("scale", ptr), ("shift", ptr),
                ("Z", i32), ("B", i32), ("H", i32), ("W", i32), ("ld", i64), ("dtype", i32)]


class PoolDesc(C.Structure):
    _fields_ = [("x", ptr), ("y", ptr), ("B", i32), ("H", i32), ("W", i32), ("k", i32), ("ld", i64), ("dtype", i32)]


class LnMtDesc(C.Structure):
    _fields_ = [("x", ptr), ("y", ptr), ("gamma", ptr), ("beta", ptr), ("rows", i64), ("T", i32), ("D", i32),
                ("ldx", i64), ("ldy", i64), ("y_dtype", i32), ("eps", f32)]


class AttnMsgDesc(C.Structure):
    _fields_ = [("cur", ptr), ("prev", ptr), ("out", ptr), ("w", ptr), ("bias", ptr),
                ("B", i32), ("heads", i32), ("T", i32), ("qh", i32), ("qw", i32), ("K", i32), ("ldk", i64), ("ldkp", i64)]


class ConvtDesc(C.Structure):
    _fields_ = [("yall", ptr), ("out", ptr), ("bias", ptr), ("B", i32), ("H", i32), ("W", i32), ("Cop", i32),
                ("dtype", i32), ("out_dtype", i32)]


class UpconvDesc(C.Structure):
    _fields_ = [("z", ptr), ("y", ptr), ("bias", ptr), ("colscale", ptr),
                ("Z", i32), ("B", i32), ("h", i32), ("w", i32), ("C", i32), ("Cp", i32),
                ("z_dtype", i32), ("y_dtype", i32), ("act", i32)]


class AdamDesc(C.Structure):
    _fields_ = [("grads", ptr), ("params", ptr), ("exp_avg", ptr), ("exp_avg_sq", ptr), ("numel", ptr),
                ("chunk_tensor", ptr), ("chunk_off", ptr), ("n_chunks", i32),
                ("max_norm", f32), ("step_size", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("weight_decay", f32),
                ("inv_sqrt_bc2", f32), ("hyper", ptr), ("ws", ptr)]


class LossDesc(C.Structure):
    _fields_ = [("pred", ptr), ("label", ptr), ("dpred", ptr), ("loss", ptr), ("stats", ptr), ("B", i64), ("HW", i64),
                ("C", i32), ("Cl", i32), ("kind", i32), ("ignore", f32), ("pos_weight", f32), ("ws", ptr)]


class CtrwDesc(C.Structure):
    _fields_ = [("rawlog", ptr), ("w0", ptr), ("b0", ptr), ("w2", ptr), ("b2", ptr), ("wmix", ptr), ("B", i32), ("T", i32), ("nH", i32), ("N", i64)]


class DetLossDesc(C.Structure):
    _fields_ = [("pred", ptr), ("target", ptr), ("weight", ptr), ("out", ptr), ("sum", ptr), ("ws", ptr), ("N", i64), ("C", i32), ("kind", i32),
                ("wmode", i32), ("gamma", f32), ("alpha", f32), ("beta", f32)]


class GatherDesc(C.Structure):
    _fields_ = [("src", ptr), ("dst", ptr), ("idx", ptr), ("rows", i64), ("C", i32), ("ld_src", i64), ("ld_dst", i64),
                ("src_dtype", i32), ("dst_dtype", i32), ("B", i32), ("src_bs", i64), ("dst_bs", i64), ("idx_bs", i64), ("skip_neg", i32)]


class WinAttnDesc(C.Structure):
    _fields_ = [("qkv", ptr), ("out", ptr), ("rawmap", ptr), ("bias", ptr), ("mask", ptr), ("pix", ptr),
                ("nwin", i32), ("nW", i32), ("nH", i32), ("T", i32), ("ws2", i32), ("dtype", i32), ("scale", f32),
                ("map_ld", i64), ("map_off", i64), ("mfma", i32), ("biasT", ptr)]


class ChanAttnDesc(C.Structure):
    _fields_ = [("q", ptr), ("kvT", ptr), ("rawchan", ptr), ("cx", ptr),
                ("B", i32), ("T", i32), ("C", i32), ("ce", i32), ("nh", i32), ("nw", i32), ("kv_dtype", i32), ("ldk", i64), ("scale", f32), ("kvbias", ptr)]


class Conv3s2Desc(C.Structure):
    _fields_ = [("x", ptr), ("w", ptr), ("bias", ptr), ("y", ptr),
                ("B", i32), ("Ci", i32), ("Co", i32), ("H", i32), ("W", i32),
                ("x_bs", i64), ("x_cs", i64), ("x_off", i64), ("y_bs", i64), ("y_cs", i64), ("y_off", i64)]


class SegcopyDesc(C.Structure):
    _fields_ = [("table", ptr), ("chunk_seg", ptr), ("chunk_off", ptr), ("n_chunks", i32), ("src_base", i64), ("dst_base", i64)]


class GnDesc(C.Structure):
    _fields_ = [("x", ptr), ("y", ptr), ("y_lo", ptr), ("gamma", ptr), ("beta", ptr), ("mean", ptr), ("rstd", ptr),
                ("dy", ptr), ("dx", ptr), ("dgamma", ptr), ("dbeta", ptr),
                ("Z", i32), ("B", i32), ("HW", i64), ("C", i32), ("G", i32), ("ld", i64),
                ("x_dtype", i32), ("y_dtype", i32), ("dy_dtype", i32), ("dx_dtype", i32), ("relu", i32), ("eps", f32), ("ws", ptr)]


class DcnDesc(C.Structure):
    _fields_ = [("x", ptr), ("x_dtype", i32), ("ldx", i64), ("offset", ptr), ("ld_off", i64), ("mask", ptr), ("ld_mask", i64), ("mask_sigmoid", i32), ("off_dtype", i32),
                ("col", ptr), ("col_lo", ptr), ("col_dtype", i32), ("ldc", i64),
                ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("Cp", i32), ("Ho", i32), ("Wo", i32), ("stride", i32), ("pad", i32), ("dil", i32),
                ("dcol", ptr), ("dcol_dtype", i32), ("dx", ptr), ("dx_dtype", i32), ("doffset", ptr), ("dmask", ptr), ("ws", ptr)]


class NearestDesc(C.Structure):
    _fields_ = [("a", ptr), ("src", ptr), ("out", ptr), ("B", i32), ("C", i32), ("Ho", i32), ("Wo", i32), ("Hi", i32), ("Wi", i32),
                ("ld_a", i64), ("ld_src", i64), ("ld_out", i64), ("dtype", i32)]


class BboxPostDesc(C.Structure):
    _fields_ = [("x", ptr * 8), ("ldx", i64 * 8), ("dims", i32 * 8), ("ngroups", i32),
                ("out", ptr), ("scales", ptr), ("bbox2d", i32), ("B", i32), ("H", i32), ("W", i32),
                ("dout", ptr), ("dx", ptr * 8), ("dscales", ptr), ("ws", ptr)]


class Fcos3dDesc(C.Structure):
    _fields_ = [("cls", ptr * 8), ("bbox", ptr * 8), ("dir", ptr * 8), ("ctr", ptr * 8),
                ("dcls", ptr * 8), ("dbbox", ptr * 8), ("ddir", ptr * 8), ("dctr", ptr * 8),
                ("H", i32 * 8), ("W", i32 * 8),
                ("stride", f32 * 8), ("half", f32 * 8), ("radius", f32 * 8), ("rr_lo", f32 * 8), ("rr_hi", f32 * 8),
                ("nlev", i32), ("B", i32), ("n_lab", i32), ("C", i32), ("P", i64),
                ("img", ptr), ("gts", ptr), ("label", ptr), ("target", ptr), ("centerness", ptr),
                ("ws", ptr), ("out", ptr), ("stats", ptr), ("gout", ptr),
                ("code_weight", f32 * 13), ("loss_weight", f32 * 5),
                ("gamma", f32), ("alpha", f32), ("beta", f32), ("beta2d", f32), ("ctr_alpha", f32), ("dir_offset", f32)]


class DetDecodeDesc(C.Structure):
    _fields_ = [("cls", ptr * 8), ("bbox", ptr * 8), ("dir", ptr * 8), ("ctr", ptr * 8),
                ("H", i32 * 8), ("W", i32 * 8),
                ("stride", f32 * 8), ("half", f32 * 8), ("denorm", f32 * 8),
                ("cand_off", i32 * 9), ("key_off", i32 * 9),
                ("nlev", i32), ("B", i32), ("C", i32), ("N", i32), ("nms_pre", i32), ("rotated", i32), ("max_per_img", i32),
                ("dir_offset", f32), ("score_thr", f32), ("nms_thr", f32),
                ("inv", ptr), ("img_size", ptr),
                ("keys", ptr), ("sel", ptr),
                ("box9", ptr), ("cen2d", ptr), ("box2d", ptr), ("nmsbox", ptr), ("dircls", ptr), ("scores", ptr),
                ("seg_n", ptr), ("seg_idx", ptr), ("kept_n", ptr), ("kept", ptr),
                ("ws", ptr),
                ("out", ptr), ("count", ptr)]


class EvalDesc(C.Structure):
    _fields_ = [("pred", ptr), ("label", ptr), ("out", ptr), ("acc", ptr), ("ws", ptr), ("thresholds", ptr), ("class_map", ptr),
                ("B", i64), ("HW", i64),
                ("C", i32), ("Cl", i32), ("kind", i32), ("source", i32), ("n_classes", i32), ("n_thresh", i32), ("n_map", i32), ("mask_mode", i32),
                ("ignore", f32), ("pos_weight", f32), ("min_depth", f32), ("max_depth", f32)]


class AugDesc(C.Structure):
    _host_ = ("table_host", "off_host")       # host copies the entry point validates: `_fill` takes CPU tensors for these fields
    _fields_ = [("src", ptr), ("off", ptr), ("off_host", ptr), ("table", ptr), ("table_host", ptr), ("out", ptr), ("flags", ptr),
                ("src_numel", i64), ("cat_max_ratio", C.c_double),
                ("B", i32), ("h", i32), ("w", i32), ("C", i32), ("src_u8", i32), ("kind", i32), ("photometric", i32), ("depth_ignore", i32),
                ("fill", f32), ("mean", f32 * 3), ("std", f32 * 3)]


class Cs3dDesc(C.Structure):
    _host_ = ("xtab_host", "ytab_host")
    _fields_ = [("src", ptr), ("disp", ptr), ("xtab", ptr), ("ytab", ptr), ("xtab_host", ptr), ("ytab_host", ptr), ("xcoeff", ptr), ("ycoeff", ptr),
                ("out", ptr), ("semseg", ptr), ("flags", ptr),
                ("B", i32), ("H", i32), ("W", i32), ("h", i32), ("w", i32), ("xn", i32), ("yn", i32), ("xk", i32), ("yk", i32), ("bgr", i32),
                ("mean", f32 * 3), ("std", f32 * 3)]


class RenderDesc(C.Structure):
    _host_ = ("win_host",)
    _fields_ = [("src", ptr), ("out", ptr), ("table", ptr), ("win", ptr), ("win_host", ptr), ("minmax", ptr), ("out_pixels", i64),
                ("B", i32), ("C", i32), ("h", i32), ("w", i32), ("H", i32), ("W", i32), ("mode", i32), ("out_kind", i32), ("swap_rb", i32)]


# descriptor entry points mtt_<name>(const desc*, stream): name -> descriptor struct
DESCS = {
    "loss_fwd": LossDesc,
    "gemm": GemmDesc, "attn_fwd": AttnDesc, "softmax_fwd": SoftmaxDesc, "softmax_bwd": SoftmaxDesc,
    "layernorm_fwd": LnDesc, "layernorm_bwd": LnDesc, "chan_logits": ChanLogitDesc, "modulate": ModulateDesc,
    "ctr_mix": CtrDesc, "bilinear_fwd": ResizeDesc, "bilinear_bwd": ResizeDesc,
    "bn_apply": BnDesc, "bn_bwd_apply": BnDesc,
    "dwconv3x3s2": DwconvDesc, "avgpool_ceil": PoolDesc, "layernorm_mt": LnMtDesc, "attn_msg": AttnMsgDesc,
    "convt3x3s2_gather": ConvtDesc,
    "upconv4_expand": UpconvDesc, "upconv4_gather": UpconvDesc,
    "gather_rows": GatherDesc, "winattn_fwd": WinAttnDesc, "chanattn_fwd": ChanAttnDesc, "conv3s2_nchw": Conv3s2Desc,
    "segcopy": SegcopyDesc,
    "ctr_weights": CtrwDesc, "detloss_fwd": DetLossDesc,
    "groupnorm_fwd": GnDesc, "groupnorm_bwd": GnDesc, "dcn_im2col": DcnDesc, "dcn_col2im_bwd": DcnDesc,
    "nearest_add": NearestDesc, "nearest_add_bwd": NearestDesc, "fcos_bbox_post": BboxPostDesc, "fcos_bbox_post_bwd": BboxPostDesc,
    "fcos3d_targets": Fcos3dDesc, "fcos3d_loss_fwd": Fcos3dDesc, "fcos3d_loss_bwd": Fcos3dDesc,
}
# every sizeof() the library reports, checked against the mirror by load(): (query symbol, index or None, struct)
SIZE_QUERIES = [("mtt_desc_size", i, st) for i, st in enumerate([
    GemmDesc, AttnDesc, SoftmaxDesc, LnDesc, ChanLogitDesc, ModulateDesc, CtrDesc, ResizeDesc, BnDesc, ConvGeom,
    DwconvDesc, PoolDesc, LnMtDesc, AttnMsgDesc, ConvtDesc, AdamDesc, LossDesc, UpconvDesc,
    GatherDesc, WinAttnDesc, ChanAttnDesc, Conv3s2Desc, SegcopyDesc, CtrwDesc, DetLossDesc])]
SIZE_QUERIES += [("mtt_det_desc_size", i, st) for i, st in enumerate([GnDesc, DcnDesc, NearestDesc, BboxPostDesc])]       # ABI 14
SIZE_QUERIES += [("mtt_fcos3d_desc_size", None, Fcos3dDesc), ("mtt_det_decode_desc_size", None, DetDecodeDesc),           # ABI 15, 16
                 ("mtt_eval_desc_size", None, EvalDesc), ("mtt_aug_desc_size", None, AugDesc),                           # ABI 17
                 ("mtt_cs3d_desc_size", None, Cs3dDesc), ("mtt_render_desc_size", None, RenderDesc)]

# positional entry points mtt_<name>(args..., stream): name -> argtypes, the stream included
POSITIONAL = {
    "patchify16": [ptr, ptr, C.c_int, C.c_int, C.c_int, C.c_int, ptr],
    "patchify": [ptr, ptr, C.c_int, C.c_int, C.c_int, C.c_int, i64, C.c_int, ptr],
    "resize_nchw": [ptr, ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ptr],
    "boxes_overlap_bev": [ptr, C.c_int, ptr, C.c_int, ptr, C.c_int, ptr],
    "nms_bev": [ptr, C.c_int, f32, C.c_int, ptr, ptr, ptr, ptr],
    "cast2d": [ptr, ptr, i64, i64, i64, i64, C.c_int, C.c_int, C.c_int, ptr],
    "split_cast": [ptr, ptr, ptr, i64, i64, i64, i64, ptr],
    "pixshuf2": [ptr, ptr, i32, i32, i32, i32, i64, i64, C.c_int, C.c_int, ptr],
    "colsum": [ptr, ptr, i64, i32, i64, C.c_int, ptr, ptr],
    "colsum_batched": [ptr, ptr, i64, i32, i64, C.c_int, i32, i64, i64, ptr, ptr],
    "add_rows": [ptr, ptr, i64, i32, i64, i64, C.c_int, f32, ptr],
    "rowscale_cast": [ptr, ptr, i64, i32, i64, i64, C.c_int, C.c_int, ptr, i32, i32, ptr],
    "rowscale_cast_colsum": [ptr, ptr, i64, i32, i64, i64, C.c_int, C.c_int, ptr, i32, i32, ptr, ptr, ptr],
}

# descriptor + extra positional arguments: mtt_<name>(const desc*, extras..., stream)
DESC_EXTRA = {
    "bn_stats": (BnDesc, [ptr]), "bn_bwd_reduce": (BnDesc, [ptr]),
    "attn_msg_bwd": (AttnMsgDesc, [ptr, ptr, ptr, ptr, ptr, ptr]),
    "modulate_bwd": (ModulateDesc, [ptr, ptr, ptr, ptr, ptr]),
    "chan_logits_bwd": (ChanLogitDesc, [ptr, ptr, C.c_int, ptr]),
    "ctr_dw": (CtrDesc, [ptr, ptr, ptr]),
    "ctr_weights_bwd": (CtrwDesc, [ptr, ptr, ptr, ptr, ptr, ptr]),
    "detloss_bwd": (DetLossDesc, [ptr, ptr, f32, ptr]),
    "attn_bwd": (AttnDesc, [ptr, ptr, ptr, ptr]),
    "winattn_bwd": (WinAttnDesc, [ptr, ptr, ptr, ptr]),
    "chanattn_bwd": (ChanAttnDesc, [ptr, ptr, ptr, ptr, i64, ptr]),
    "conv3s2_nchw_bwd": (Conv3s2Desc, [ptr, ptr, ptr, ptr]),
    "grad_sqnorm": (AdamDesc, [ptr]),
    "adam_step": (AdamDesc, [ptr]),
    "loss_label_stats": (LossDesc, [ptr]),
    "loss_bwd": (LossDesc, [ptr]),
    "dwconv3x3s2_bwd": (DwconvDesc, [ptr, ptr, ptr]),
    "avgpool_ceil_bwd": (PoolDesc, [ptr, ptr]),
    "convt3x3s2_gather_bwd": (ConvtDesc, [ptr, ptr]),
}

# ABI 16: the inference post-processing of the 3ddet task (csrc/det_decode.hip), descriptor entry points like DESCS.  A table of its own:
# the kernel parity suite enumerates DESCS | POSITIONAL | DESC_EXTRA, and these are covered by tests/test_gpu_det_decode.py instead.
POSTPROC = {"det_select": DetDecodeDesc, "det_decode": DetDecodeDesc, "det_nms_seg": DetDecodeDesc, "det_collect": DetDecodeDesc}
DET_MAX_CAND, DET_MAX_CLASSES, DET_OUT_COLS = 8192, 16, 18            # MTT_DET_* of include/mtt_hip.h

# ABI 17: evaluation of the dense tasks (csrc/eval_ops.hip), descriptor entry points like DESCS.  A table of its own as well: covered by
# tests/test_gpu_eval.py.
EVAL = {"eval_map": EvalDesc, "eval_accum": EvalDesc}
EVAL_CONFUSION, EVAL_SAL, EVAL_DEPTH, EVAL_NORMALS, EVAL_EDGE = 0, 1, 2, 3, 4     # MTT_EVAL_* of include/mtt_hip.h
EVAL_FROM_LOGITS, EVAL_FROM_MAP = 0, 1

# Batch augmentation (csrc/augment.hip): additive exports under ABI 17, descriptor entry points like DESCS.  A table of its own: covered by
# tests/test_gpu_augment.py.  The host copies of the table (AugDesc._host_) are CPU tensors.
AUGMENT = {"aug_select": AugDesc, "aug_image": AugDesc, "aug_labels": AugDesc}
AUG_CANDS, AUG_COLS = 11, 40                                                      # MTT_AUG_* of include/mtt_hip.h
(AUG_H, AUG_W, AUG_SH, AUG_SW, AUG_RESIZED, AUG_FLIP, AUG_NTEST, AUG_CHOSEN) = range(8)
AUG_CAND_Y, AUG_CAND_X = 8, 19
(AUG_BRIGHT, AUG_BETA, AUG_FMODE, AUG_CONTRAST, AUG_CALPHA, AUG_SAT, AUG_SALPHA, AUG_HUE, AUG_HDELTA, AUG_SCALE) = range(30, 40)
AUG_PLAIN, AUG_DEPTH, AUG_NORMALS, AUG_HUMAN_PARTS = 0, 1, 2, 3
E_BADARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3                                     # MTT_E_*

# Cityscapes-3D batch preparation (csrc/cs3d.hip): additive exports under ABI 17 as well, covered by tests/test_gpu_cs3d.py.  The host
# copies of the index tables (Cs3dDesc._host_) are CPU tensors.
CS3D = {"cs3d_image": Cs3dDesc, "cs3d_labels": Cs3dDesc}
CS3D_TILE_H, CS3D_TILE_W, CS3D_MAX_ROWS, CS3D_MAX_COLS = 16, 64, 208, 5440         # MTT_CS3D_* of include/mtt_hip.h

# Rendering predictions (csrc/render.hip): additive exports under ABI 17 as well, covered by tests/test_gpu_render.py.  win_host is the
# host copy of the window table, a CPU tensor.
RENDER = {"render_map": RenderDesc, "render_minmax": RenderDesc}
RENDER_CLASS, RENDER_SIGMOID255, RENDER_SOFTMAX1_255, RENDER_NORMALS, RENDER_DEPTH = range(5)       # MTT_RENDER_* of include/mtt_hip.h
RENDER_OUT_U8, RENDER_OUT_LUT1, RENDER_OUT_LUT3, RENDER_OUT_RGB3, RENDER_OUT_F32 = range(5)         # MTT_RENDER_OUT_*

# workspace-size queries mtt_<entry>_ws_floats(const desc*) of the entry points whose cross-workgroup reductions go through caller-owned partials
WS_QUERIES = {"gemm_colsum": GemmDesc, "chan_logits": ChanLogitDesc, "modulate_bwd": ModulateDesc, "ctr_dw": CtrDesc, "attn_msg_bwd": AttnMsgDesc, "loss": LossDesc,
              "chanattn_bwd": ChanAttnDesc, "detloss": DetLossDesc,
              "groupnorm": GnDesc, "dcn_col2im": DcnDesc, "fcos_bbox_post": BboxPostDesc, "fcos3d": Fcos3dDesc}

# the exports that belong to no family: symbol -> (restype, argtypes), the types as include/mtt_hip.h has them
HELPERS = {
    "mtt_abi_version": (C.c_int, []),
    "mtt_desc_size": (C.c_size_t, [C.c_int]), "mtt_det_desc_size": (C.c_size_t, [C.c_int]),
    **{sym: (C.c_size_t, []) for sym, idx, _ in SIZE_QUERIES if idx is None},
    "mtt_gemm_variant": (C.c_int, [C.POINTER(GemmDesc)]), "mtt_adam_chunk": (C.c_int, []), "mtt_segcopy_chunk": (C.c_int, []),
    "mtt_bn_reduce_ws_floats": (C.c_size_t, [i64, i32, i32]), "mtt_colsum_ws_floats": (C.c_size_t, [i64, i32]),
    "mtt_rowscale_cast_colsum_ws_floats": (C.c_size_t, [i64, i32]), "mtt_layernorm_bwd_ws_floats": (C.c_size_t, [i64, i32]),
    "mtt_nms_ws_bytes": (C.c_size_t, [C.c_int]), "mtt_det_nms_ws_bytes": (C.c_size_t, [C.POINTER(DetDecodeDesc)]),
    "mtt_eval_ws_floats": (C.c_size_t, [C.POINTER(EvalDesc)]),
}


def _signatures():
    """every export: symbol -> (restype, argtypes, descriptor struct the launchers fill or None)"""
    sig = {sym: (res, at, None) for sym, (res, at) in HELPERS.items()}
    for entry, st in WS_QUERIES.items():
        sig["mtt_%s_ws_floats" % entry] = (C.c_size_t, [C.POINTER(st)], None)
    for family in (DESCS, POSTPROC, EVAL, AUGMENT, CS3D, RENDER):
        for name, st in family.items():
            sig["mtt_" + name] = (C.c_int, [C.POINTER(st), ptr], st)
    for name, at in POSITIONAL.items():
        sig["mtt_" + name] = (C.c_int, at, None)
    for name, (st, extra) in DESC_EXTRA.items():
        sig["mtt_" + name] = (C.c_int, [C.POINTER(st)] + extra + [ptr], st)
    return sig


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

_lib = None
_entry = {}                               # entry point name (no "mtt_") -> (function, descriptor struct or None), resolved by load()


def load():
    """Load the shared library (once), declare every export's signature and verify ABI version + descriptor sizes.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU/eager fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
    lib = C.CDLL(LIB_PATH)
    entry = {}
    for sym, (restype, argtypes, st) in SIGNATURES.items():
        fn = getattr(lib, sym)
        fn.restype, fn.argtypes = restype, argtypes
        entry[sym[4:]] = (fn, st)
    if lib.mtt_abi_version() != ABI_VERSION:
        raise RuntimeError("libmtt_hip.so ABI version mismatch")
    for sym, idx, st in SIZE_QUERIES:
        size = getattr(lib, sym)() if idx is None else getattr(lib, sym)(idx)
        if size != C.sizeof(st):
            raise RuntimeError(f"descriptor layout mismatch for {st.__name__}: C {size} vs ctypes {C.sizeof(st)}")
    _entry.update(entry)
    _lib = lib
    return lib


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported tensor dtype {t.dtype}")


def _addr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libmtt_hip.so operates on HIP device memory only (tensor is on %s)" % t.device)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fill(desc, fields, cpu_ok=False):
    """Fill descriptor `desc` from keyword fields and return it.  A tensor becomes its device address (a CPU tensor raises, unless cpu_ok:
    the descriptor is only inspected); in a field the struct lists in `_host_` it is the host copy the entry point validates and must be
    a CPU tensor.  conv={...} fills the nested mtt_conv_geom, a list or tuple fills an array element by element, None leaves the field
    NULL, ints (addresses included) and floats are assigned as they are."""
    host = getattr(desc, "_host_", ())
    for k, v in fields.items():
        if type(v) is int or type(v) is float:             # most fields by far: ahead of the costlier isinstance tests
            setattr(desc, k, v)
        elif isinstance(v, torch.Tensor):
            if k in host:
                if v.is_cuda:
                    raise RuntimeError(f"{k} is the host copy of the table and must be a CPU tensor")
                setattr(desc, k, v.data_ptr())
            else:
                setattr(desc, k, v.data_ptr() if cpu_ok else _addr(v))
        elif v is None:
            continue
        elif k == "conv":
            for ck, cv in v.items():
                setattr(desc.conv, ck, int(cv))
        elif isinstance(v, (list, tuple)):
            arr = getattr(desc, k)
            for i, e in enumerate(v):
                arr[i] = _addr(e) if isinstance(e, torch.Tensor) else e
        else:
            setattr(desc, k, v)
    return desc


def _query(symbol, st, fields, cpu_ok=False):
    """what `symbol(const desc*)` answers for a descriptor `st` filled from `fields`"""
    return int(getattr(load(), symbol)(C.byref(_fill(st(), fields, cpu_ok))))


def ws_floats(entry, **fields):
    """mtt_<entry>_ws_floats(desc) for the geometry in `fields` (ints only; pointer fields stay NULL)."""
    return _query("mtt_%s_ws_floats" % entry, WS_QUERIES[entry], fields)


def det_nms_ws_bytes(batch, classes, cands):
    """mtt_det_nms_ws_bytes for `batch` images, `classes` classes and `cands` candidates per image"""
    return _query("mtt_det_nms_ws_bytes", DetDecodeDesc, dict(B=int(batch), C=int(classes), N=int(cands)))


def eval_ws_floats(kind, batch, pixels):
    """mtt_eval_ws_floats for meter kind `kind` on `batch` images of `pixels` pixels"""
    return _query("mtt_eval_ws_floats", EvalDesc, dict(kind=int(kind), B=int(batch), HW=int(pixels)))


def gemm_variant(**kw):
    """Kernel mtt_gemm would dispatch these descriptor fields to (0 general 128x128, 3 LDS-DMA 256x256, 6 token-major weight gradient,
    8 LDS-DMA 256x256 on split operands; < 0: no kernel takes them).  Only inspects the descriptor, so CPU tensors are accepted."""
    return _query("mtt_gemm_variant", GemmDesc, kw, cpu_ok=True)


def _launch(name, kw, stream=None):
    """the status of mtt_<name> for the fields, `args` or `xargs` in kw, on `stream` (torch's current one by default)"""
    load()
    fn, st = _entry[name]
    if st is None:
        return fn(*[(_addr(a) if isinstance(a, torch.Tensor) else a) for a in kw["args"]], _stream() if stream is None else stream)
    xargs = [(_addr(a) if isinstance(a, torch.Tensor) else a) for a in kw.pop("xargs", ())]
    desc = _fill(st(), kw)
    return fn(C.byref(desc), *xargs, _stream() if stream is None else stream)


def call(name, **kw):
    """Launch `mtt_<name>`; tensors in `kw` become device pointers.  For descriptor entry points
    nested dict `conv={...}` fills mtt_conv_geom.  Positional entry points take `args=[...]`, those of
    DESC_EXTRA their extra arguments in `xargs=[...]`.  Raises on any non-zero status."""
    rc = _launch(name, kw)
    if rc != 0:
        raise RuntimeError(f"mtt_{name} failed with status {rc}" + (" (argument error)" if rc < 0 else " (hipError_t)"))


def status_call(name, stream=None, **fields):
    """Launch `mtt_<name>` of AUGMENT, CS3D or RENDER, whose entry points validate their descriptor on the host.  Returns 0 or the negative
    MTT_E_* status (a refused descriptor, nothing launched), so that a caller can tell it from a failed launch; a hipError_t raises."""
    rc = _launch(name, fields, stream)
    if rc > 0:
        raise RuntimeError(f"mtt_{name} failed with status {rc} (hipError_t)")
    return rc


aug_call = cs3d_call = render_call = status_call
