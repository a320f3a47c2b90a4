"""ctypes binding of libp2p_hip.so (the C ABI declared in include/p2p_hip.h).

The product path has no CPU fallback: if the shared library is missing, importing this module
raises, and every wrapper raises RuntimeError carrying p2p_last_error() on a non-zero status.
"""
import ctypes
import os

import torch  # noqa: F401  (must be loaded first so libamdhip64.so.7 resolves to torch's copy)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libp2p_hip.so")
# Kernel experiments (tools/ab_variants.sh) load another build through P2P_LIB_PATH -- only together with
# P2P_ALLOW_EXPERIMENT=1, so that a stray variable in a user's environment can never swap the library.
_ALLOW_EXPERIMENT = os.environ.get("P2P_ALLOW_EXPERIMENT") == "1"
if os.environ.get("P2P_LIB_PATH"):
    if not _ALLOW_EXPERIMENT:
        raise ImportError("P2P_LIB_PATH is set but P2P_ALLOW_EXPERIMENT=1 is not: refusing to load a library other than "
                          f"{LIB_PATH}")
    LIB_PATH = os.environ["P2P_LIB_PATH"]

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP extension first (python -m patch2pix_amd.build, "
        "or __graft_entry__.build()). There is no CPU fallback for the matching path.")

lib = ctypes.CDLL(LIB_PATH)

c_float_p = ctypes.c_void_p   # raw addresses (torch .data_ptr()) are passed as void*
c_stream = ctypes.c_void_p


class BnParams(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p)]


class RegressorParams(ctypes.Structure):
    _fields_ = [("conv1_w", ctypes.c_void_p), ("bn1", BnParams),
                ("conv2_w", ctypes.c_void_p), ("bn2", BnParams),
                ("fc1_w", ctypes.c_void_p), ("fc1_b", ctypes.c_void_p), ("bnf1", BnParams),
                ("fc2_w", ctypes.c_void_p), ("fc2_b", ctypes.c_void_p), ("bnf2", BnParams),
                ("fc3_w", ctypes.c_void_p), ("fc3_b", ctypes.c_void_p)]


class RegressorConfig(ctypes.Structure):
    _fields_ = [("n_feat", ctypes.c_int), ("feat_idx", ctypes.c_int * 4), ("feat_comb", ctypes.c_int),
                ("n_conv", ctypes.c_int), ("conv_dim", ctypes.c_int * 4), ("conv_ker", ctypes.c_int * 4),
                ("conv_str", ctypes.c_int * 4), ("n_fc", ctypes.c_int), ("fc_dim", ctypes.c_int * 4), ("psize", ctypes.c_int)]


class RegressorTensors(ctypes.Structure):
    _fields_ = [("conv_w", ctypes.c_void_p * 4), ("conv_bn", BnParams * 4),
                ("fc_w", ctypes.c_void_p * 4), ("fc_b", ctypes.c_void_p * 4), ("fc_bn", BnParams * 4),
                ("out_w", ctypes.c_void_p), ("out_b", ctypes.c_void_p)]


class NcnConfig(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int), ("kernel_size", ctypes.c_int * 4), ("channels", ctypes.c_int * 4),
                ("symmetric", ctypes.c_int)]


class NcnTensors(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p * 4), ("b", ctypes.c_void_p * 4)]


class ResizeItem(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_void_p), ("in_h", ctypes.c_int), ("in_w", ctypes.c_int),
                ("table_x", ctypes.c_void_p), ("table_y", ctypes.c_void_p), ("ksize_x", ctypes.c_int), ("ksize_y", ctypes.c_int)]


class Pyramid(ctypes.Structure):
    _fields_ = [("level", ctypes.c_void_p * 4), ("height", ctypes.c_int), ("width", ctypes.c_int)]


def _sig(name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


p2p_version = _sig("p2p_version", ctypes.c_int, [])
VERSION_EXPERIMENT = 0x40000000     # csrc/p2p_common.h: a build with timing-experiment switches (wrong results by design)
if p2p_version() & VERSION_EXPERIMENT and not _ALLOW_EXPERIMENT:
    raise ImportError(f"{LIB_PATH} is an experiment build (-DP2P_EXPERIMENT); set P2P_ALLOW_EXPERIMENT=1 to load it")
p2p_last_error = _sig("p2p_last_error", ctypes.c_char_p, [])
p2p_ncn_create = _sig("p2p_ncn_create", ctypes.c_int,
                      [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_void_p)])
p2p_ncn_destroy = _sig("p2p_ncn_destroy", None, [ctypes.c_void_p])
p2p_ncn_set_tile = _sig("p2p_ncn_set_tile", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 3)
p2p_ncn_create_config = _sig("p2p_ncn_create_config", ctypes.c_int,
                             [ctypes.POINTER(NcnConfig), ctypes.POINTER(NcnTensors), ctypes.POINTER(ctypes.c_void_p)])
p2p_ncn_is_generic = _sig("p2p_ncn_is_generic", ctypes.c_int, [ctypes.c_void_p])
p2p_ncn_set_mode = _sig("p2p_ncn_set_mode", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
p2p_ncn_get_mode = _sig("p2p_ncn_get_mode", ctypes.c_int, [ctypes.c_void_p])
# P2P_COARSE_FP16X2 (default, fp32-equivalent) / P2P_COARSE_FP16 (opt-in, one fp16 plane per operand: NOT fp32-equivalent)
COARSE_MODES = {"fp16x2": 0, "fp16": 1}
# a generic handle's own modes: 0 (default, exact fp32 MFMA) / P2P_COARSE_GENERIC_FP16X2 (opt-in, fp32-equivalent: every layer
# behind the first on the fp16 matrix cores, two fp16 planes per operand)
COARSE_MODES_GENERIC = {"generic": 0, "generic_fp16x2": 17}
p2p_regressor_create = _sig("p2p_regressor_create", ctypes.c_int,
                            [ctypes.POINTER(RegressorParams), ctypes.POINTER(ctypes.c_void_p)])
p2p_regressor_create_config = _sig("p2p_regressor_create_config", ctypes.c_int,
                                   [ctypes.POINTER(RegressorConfig), ctypes.POINTER(RegressorTensors),
                                    ctypes.POINTER(ctypes.c_void_p)])
p2p_regressor_destroy = _sig("p2p_regressor_destroy", None, [ctypes.c_void_p])
p2p_coarse_workspace_bytes = _sig("p2p_coarse_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 6)
p2p_coarse_workspace_bytes_for = _sig("p2p_coarse_workspace_bytes_for", ctypes.c_size_t, [ctypes.c_void_p] + [ctypes.c_int] * 6)
p2p_neigh_consensus_workspace_bytes = _sig("p2p_neigh_consensus_workspace_bytes", ctypes.c_size_t,
                                           [ctypes.c_void_p] + [ctypes.c_int] * 4)
p2p_coarse_forward = _sig("p2p_coarse_forward", ctypes.c_int,
                          [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 +
                          [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, c_stream])
p2p_coarse_forward_batch = _sig("p2p_coarse_forward_batch", ctypes.c_int,
                                [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 7 +
                                [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, c_stream])
p2p_neigh_consensus_batch = _sig("p2p_neigh_consensus_batch", ctypes.c_int,
                                 [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                                           ctypes.c_size_t, c_stream])
p2p_delta_unpack = _sig("p2p_delta_unpack", ctypes.c_int,
                        [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, c_stream])
p2p_coarse_matches = _sig("p2p_coarse_matches", ctypes.c_int,
                          [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 7 +
                          [ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_coarse_matches_batch = _sig("p2p_coarse_matches_batch", ctypes.c_int,
                                [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 +
                                [ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_coarse_matches_topk_batch = _sig("p2p_coarse_matches_topk_batch", ctypes.c_int,
                                     [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 10 +
                                     [ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_coarse_score_workspace_bytes = _sig("p2p_coarse_score_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)
p2p_coarse_score_batch = _sig("p2p_coarse_score_batch", ctypes.c_int,
                              [ctypes.c_void_p] + [ctypes.c_int] * 6 +
                              [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, c_stream])
SCORE_NORMS = {None: 0, "softmax": 1, "l1": 2}          # P2P_SCORE_NONE / _SOFTMAX / _L1
p2p_filter_coarse_workspace_bytes = _sig("p2p_filter_coarse_workspace_bytes", ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
p2p_filter_coarse_batch = _sig("p2p_filter_coarse_batch", ctypes.c_int,
                               [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, c_stream])
p2p_match_tail_batch = _sig("p2p_match_tail_batch", ctypes.c_int,
                            [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 4 + [c_stream])
p2p_epipolar_batch = _sig("p2p_epipolar_batch", ctypes.c_int,
                          [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_stream])
DTYPES = {"float32": 0, "float64": 1, "int64": 2}                   # P2P_F32 / _F64 / _I64
EPI_KINDS = {"sampson": 0, "sym": 1, "sym_sqrt": 2, "value": 3}     # P2P_EPI_SAMPSON / _SYM / _SYM_SQRT / _VALUE
EPI_MAX_BINS = 16
p2p_regress = _sig("p2p_regress", ctypes.c_int,
                   [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Pyramid), ctypes.POINTER(Pyramid),
                    ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_void_p, ctypes.c_size_t, c_stream])
p2p_regress_workspace_bytes = _sig("p2p_regress_workspace_bytes", ctypes.c_size_t, [ctypes.c_int])
p2p_regress_workspace_bytes_mode = _sig("p2p_regress_workspace_bytes_mode", ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
p2p_regress_workspace_bytes_for = _sig("p2p_regress_workspace_bytes_for", ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int])

p2p_regress_batch = _sig("p2p_regress_batch", ctypes.c_int,
                         [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Pyramid), ctypes.POINTER(Pyramid),
                          ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 +
                         [ctypes.c_void_p, ctypes.c_size_t, c_stream])

p2p_regress_batch_dev = _sig("p2p_regress_batch_dev", ctypes.c_int,
                             [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Pyramid), ctypes.POINTER(Pyramid),
                              ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 +
                             [ctypes.c_void_p, ctypes.c_size_t, c_stream])

p2p_conv_create = _sig("p2p_conv_create", ctypes.c_int,
                       [ctypes.c_void_p, ctypes.POINTER(BnParams)] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_void_p)])
p2p_conv_destroy = _sig("p2p_conv_destroy", None, [ctypes.c_void_p])
p2p_conv_set_tile = _sig("p2p_conv_set_tile", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int])
p2p_conv_set_mode = _sig("p2p_conv_set_mode", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
p2p_conv_get_mode = _sig("p2p_conv_get_mode", ctypes.c_int, [ctypes.c_void_p])
# P2P_CONV_FP16X2 (default, fp32-equivalent) / P2P_CONV_FP16 (opt-in, one fp16 plane per operand: NOT fp32-equivalent)
BACKBONE_MODES = {"fp16x2": 0, "fp16": 1}
p2p_conv_forward = _sig("p2p_conv_forward", ctypes.c_int,
                        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 +
                        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_stem_create = _sig("p2p_stem_create", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BnParams), ctypes.POINTER(ctypes.c_void_p)])
p2p_stem_destroy = _sig("p2p_stem_destroy", None, [ctypes.c_void_p])
p2p_stem_set_mode = _sig("p2p_stem_set_mode", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
p2p_stem_get_mode = _sig("p2p_stem_get_mode", ctypes.c_int, [ctypes.c_void_p])
p2p_stem_forward = _sig("p2p_stem_forward", ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p, c_stream])
p2p_maxpool_nhwc = _sig("p2p_maxpool_nhwc", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_nhwc_to_nchw = _sig("p2p_nhwc_to_nchw", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, c_stream])
p2p_absmax_batch = _sig("p2p_absmax_batch", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, c_stream])

p2p_resize_workspace_bytes = _sig("p2p_resize_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)
p2p_resize_bicubic_batch = _sig("p2p_resize_bicubic_batch", ctypes.c_int,
                                [ctypes.POINTER(ResizeItem)] + [ctypes.c_int] * 3 +
                                [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                 c_stream])

# the matching operators on their own (version 110)
p2p_correlation_batch = _sig("p2p_correlation_batch", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, c_stream])
p2p_maxpool4d_batch = _sig("p2p_maxpool4d_batch", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p, c_stream])
p2p_mutual_matching_workspace_bytes = _sig("p2p_mutual_matching_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)
p2p_mutual_matching_batch = _sig("p2p_mutual_matching_batch", ctypes.c_int,
                                 [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, c_stream])
p2p_conv4d_create = _sig("p2p_conv4d_create", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_void_p)])
p2p_conv4d_destroy = _sig("p2p_conv4d_destroy", None, [ctypes.c_void_p])
p2p_conv4d_forward_batch = _sig("p2p_conv4d_forward_batch", ctypes.c_int,
                                [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, c_stream])
p2p_l2_normalize = _sig("p2p_l2_normalize", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, c_stream])

p2p_regressor_set_mode = _sig("p2p_regressor_set_mode", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
p2p_regressor_get_mode = _sig("p2p_regressor_get_mode", ctypes.c_int, [ctypes.c_void_p])
REGRESS_MODES = {"f32": 0, "fp16x2": 3, "fp16x2w": 4}      # the fp32-equivalent modes
REGRESS_MODES_LOSSY = {"fp16": 5}     # P2P_REGRESS_FP16: opt-in, one fp16 plane per operand (not fp32-equivalent; kept apart from
                                      # the dict above, whose modes share the accuracy bars and the two-plane buffer layouts)
REGRESS_GENERIC = 16          # P2P_REGRESS_GENERIC: the mode id a handle made by p2p_regressor_create_config starts in
# the modes of a generic handle, both fp32-equivalent: exact fp32 MFMA, and P2P_REGRESS_GENERIC_FP16X2 (the convolution stack
# on two fp16 planes per operand, three MFMA products per product)
REGRESS_MODES_GENERIC = {"generic": 16, "generic_fp16x2": 17}
FEAT_COMB = {"pre": 0, "post": 1}

EXPORTS = ["p2p_version", "p2p_last_error", "p2p_ncn_create", "p2p_ncn_destroy", "p2p_ncn_set_tile", "p2p_regressor_create",
           "p2p_regressor_destroy", "p2p_coarse_workspace_bytes", "p2p_coarse_forward", "p2p_coarse_forward_batch",
           "p2p_neigh_consensus_batch", "p2p_delta_unpack", "p2p_coarse_matches", "p2p_coarse_matches_batch", "p2p_filter_coarse_workspace_bytes", "p2p_filter_coarse_batch", "p2p_match_tail_batch", "p2p_regress", "p2p_regress_workspace_bytes", "p2p_regress_workspace_bytes_mode", "p2p_regress_batch", "p2p_regress_batch_dev", "p2p_regressor_set_mode",
           "p2p_regressor_get_mode", "p2p_conv_create", "p2p_conv_destroy", "p2p_conv_set_tile", "p2p_conv_forward", "p2p_absmax_batch", "p2p_stem_create", "p2p_stem_destroy", "p2p_stem_forward",
           "p2p_maxpool_nhwc", "p2p_nhwc_to_nchw", "p2p_regressor_create_config", "p2p_regress_workspace_bytes_for",
           "p2p_coarse_matches_topk_batch", "p2p_ncn_create_config", "p2p_ncn_is_generic", "p2p_coarse_workspace_bytes_for",
           "p2p_neigh_consensus_workspace_bytes", "p2p_resize_workspace_bytes", "p2p_resize_bicubic_batch",
           "p2p_coarse_score_workspace_bytes", "p2p_coarse_score_batch", "p2p_epipolar_batch",
           "p2p_correlation_batch", "p2p_maxpool4d_batch", "p2p_mutual_matching_workspace_bytes", "p2p_mutual_matching_batch",
           "p2p_conv4d_create", "p2p_conv4d_destroy", "p2p_conv4d_forward_batch", "p2p_l2_normalize",
           "p2p_conv_set_mode", "p2p_conv_get_mode", "p2p_stem_set_mode", "p2p_stem_get_mode", "p2p_ncn_set_mode", "p2p_ncn_get_mode"]


def check(status, what):
    if status != 0:
        msg = p2p_last_error().decode("utf-8", "replace")
        if status == -3:
            raise NotImplementedError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed with status {status}: {msg}")
