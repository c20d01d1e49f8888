"""ctypes binding of the C ABI in include/siggan.h and the siggan_*.h headers beside it: one table of signatures per header,
all of them in ``GROUPS`` or, for headers added after siggan_dtw.h, in ``EXTRA_GROUPS`` / ``ADDED_GROUPS``.

The shared library is built in-tree by ``__graft_entry__.build()`` / ``csrc/Makefile`` and must be
present: there is no CPU or PyTorch fallback for this path -- a missing or stale library raises.
torch is imported first so the library resolves HIP against the runtime torch already loaded
(one HIP runtime per process)."""
import ctypes as C
import os

import torch  # noqa: F401  (must be loaded before the library; see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SIGGAN_LIB_PATH: load another build of the same ABI (A/B measurements of kernel variants); it must exist -- a missing
# library raises either way, there is nothing to fall back to
LIB_PATH = os.environ.get("SIGGAN_LIB_PATH") or os.path.join(_HERE, "libsiggan_hip.so")
ABI_VERSION = 4
M_COUNT = 16
# the implicit-GEMM epilogues in gconv.h's enum Epilogue order (siggan_prof_launch reports them by number)
EPILOGUES = ("raw", "bias_lrelu_drop", "affine_relu", "lrelu_bwd", "bn_bwd_stats")
METRIC_INDEX = {"d_loss": 0, "d_loss_real": 1, "d_loss_fake": 2, "d_real_mean": 3, "d_fake_mean": 4,
                "d_real_acc": 5, "d_fake_acc": 6, "d_grad_norm": 7, "g_loss": 8, "g_fake_mean": 9,
                "g_grad_norm": 10, "d_skipped": 11, "g_skipped": 12}
# columns of the per-image stroke counters (SIGGAN_IS_*): #{t < 0}, #{(t + 1) / 2 < thr}, #{t < thr}
IS_NEG, IS_INK_SIGNED, IS_INK_UNIT, IS_COUNT = 0, 1, 2, 3


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("latent_dim", C.c_int32), ("image_size", C.c_int32),
                ("image_channels", C.c_int32), ("max_batch", C.c_int32), ("dropout", C.c_float),
                ("leaky_slope", C.c_float), ("seed", C.c_uint64), ("dtype", C.c_int32), ("f16_grad_scale", C.c_float),
                ("spectral_norm", C.c_int32), ("g_leaky_slope", C.c_float)]


DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "f16": 2, "fp16": 2, "float16": 2}


class Storage(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "g_params", "g_grads", "g_exp_avg", "g_exp_avg_sq", "g_adam_steps", "g_bn_running_mean",
        "g_bn_running_var", "g_bn_batches", "d_params", "d_grads", "d_exp_avg", "d_exp_avg_sq", "d_adam_steps",
        "d_sn_u", "d_sn_v")]


class Hyper(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("label_smoothing", C.c_float), ("clip_max_norm", C.c_float), ("grad_scale", C.c_float)]


class LatentObjective(C.Structure):       # siggan_latent_objective
    _fields_ = [("recon_weight", C.c_float), ("realism_weight", C.c_float), ("prior_weight", C.c_float)]


class MlpConfig(C.Structure):       # include/siggan_mlp.h
    _fields_ = [("device", C.c_int32), ("latent_dim", C.c_int32), ("image_size", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 4), ("max_batch", C.c_int32), ("leaky_slope", C.c_float), ("seed", C.c_uint64)]


class MlpStorage(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "g_params", "g_grads", "g_exp_avg", "g_exp_avg_sq", "g_adam_steps", "g_bn_running_mean",
        "g_bn_running_var", "g_bn_batches", "d_params", "d_grads", "d_exp_avg", "d_exp_avg_sq", "d_adam_steps")]


VERIFIER_WEIGHT_FIELDS = (                 # include/siggan_verifier.h, state_dict() order
    "conv1_weight", "conv1_bias", "bn1_weight", "bn1_bias", "bn1_running_mean", "bn1_running_var",
    "conv2_weight", "conv2_bias", "bn2_weight", "bn2_bias", "bn2_running_mean", "bn2_running_var",
    "conv3_weight", "conv3_bias", "bn3_weight", "bn3_bias", "bn3_running_mean", "bn3_running_var",
    "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias", "cls0_weight", "cls0_bias", "cls3_weight", "cls3_bias")
VFMT_F32, VFMT_U8 = 0, 1
E_ARG = -1                                 # SIGGAN_E_ARG (= SIGGAN_E_INVALID)


class VerifierWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VERIFIER_WEIGHT_FIELDS] + [("bn_eps", C.c_float)]


class VerifierIdentity(C.Structure):      # siggan_verifier_identity
    _fields_ = [("embed_weight", C.c_float), ("score_weight", C.c_float)]


_P, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
_SIGNATURES = {
    "siggan_abi_version": (C.c_int, []),
    "siggan_last_error": (C.c_char_p, []),
    "siggan_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "siggan_destroy": (C.c_int, [_P]),
    "siggan_param_count": (_I64, [_P, C.c_int]),
    "siggan_param_tensors": (_I32, [_P, C.c_int]),
    "siggan_param_span": (C.c_int, [_P, C.c_int, _I32, C.POINTER(_I64), C.POINTER(_I64)]),
    "siggan_bn_count": (_I64, [_P]),
    "siggan_bn_layers": (_I32, [_P]),
    "siggan_sn_count": (_I64, [_P, C.c_int]),
    "siggan_workspace_bytes": (_I64, [_P]),
    "siggan_bind": (C.c_int, [_P, C.POINTER(Storage)]),
    "siggan_params_changed": (C.c_int, [_P]),
    "siggan_seed": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "siggan_rng_state": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "siggan_set_mode": (C.c_int, [_P, _I32]),
    "siggan_set_step_variant": (C.c_int, [_P, _I32]),
    "siggan_g_forward": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "siggan_g_generate_u8": (C.c_int, [_P, _P, _I32, _P, _P, _P, C.c_float, _P]),
    "siggan_d_forward": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
    "siggan_d_score_u8": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _P]),
    "siggan_dequant_table": (C.c_int, [C.POINTER(C.c_float)]),
    "siggan_g_latent_grad": (C.c_int, [_P, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "siggan_g_latent_objective_grad": (C.c_int, [_P, _P, _I32, _P, _P, C.POINTER(LatentObjective), _P, _P, _P, _P, _P, _P]),
    "siggan_g_latent_objective_grad_seeded": (C.c_int, [_P, _P, _I32, _P, _P, C.POINTER(LatentObjective), _P, _P, _P, _P, _P, _P, _P]),
    "siggan_g_param_grad": (C.c_int, [_P, _P, _I32, _P, _P, C.POINTER(LatentObjective), _I32, _P, _P, _P, _P, _P, _P]),
    "siggan_op_anchor": (C.c_int, [_P, _P, _P, _P, _I64, C.c_float, _P]),
    "siggan_d_step": (C.c_int, [_P, _P, _I32, _P, _P, C.POINTER(Hyper), _P, _P, _P]),
    "siggan_g_step": (C.c_int, [_P, _I32, _P, C.POINTER(Hyper), _P, _P, _P]),
    "siggan_d_grads": (C.c_int, [_P, _P, _I32, _P, _P, C.POINTER(Hyper), _P, _P]),
    "siggan_step_begin": (C.c_int, [_P, _P, _I32, _P, _P, _P, C.POINTER(Hyper), _P, _P]),
    "siggan_stage_real": (C.c_int, [_P, _P, _I32, _P]),
    "siggan_d_apply": (C.c_int, [_P, C.POINTER(Hyper), _P, _P, _P]),
    "siggan_g_grads": (C.c_int, [_P, _I32, _P, C.POINTER(Hyper), _P, _P]),
    "siggan_g_apply": (C.c_int, [_P, C.POINTER(Hyper), _P, _P, _P]),
    "siggan_op_conv4x4s2": (C.c_int, [_P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "siggan_op_conv4x4s2_wgrad": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "siggan_op_adam": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, C.POINTER(Hyper), _P]),
    "siggan_op_randn": (C.c_int, [_P, _P, _I64, _P]),
    "siggan_augment_batch": (C.c_int, [_I32, _P, _I64, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "siggan_image_stats": (C.c_int, [_I32, _P, _I32, _I64, C.c_float, _P, _P]),
    "siggan_comm_unique_id": (C.c_int, [_P]),
    "siggan_comm_init": (C.c_int, [_P, _I32, _I32, _P]),
    "siggan_comm_destroy": (C.c_int, [_P]),
    "siggan_comm_world": (_I32, [_P]),
    "siggan_comm_broadcast": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "siggan_device_info": (C.c_int, [_I32, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I64)]),
    "siggan_prof_enable": (C.c_int, [_P, _I32]),
    "siggan_prof_slots": (_I32, []),
    "siggan_prof_launch": (C.c_int, [_P, _I64, C.POINTER(_I32), _I32, C.POINTER(_I64)]),
    "siggan_prof_read": (C.c_int, [_P, _I32, C.c_char_p, _I32, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "siggan_debug_tensor": (C.c_int, [_P, C.c_char_p, _I32, _P, _I64, _P]),
    # fully-connected extension (include/siggan_mlp.h; build-defined, parity unpinned)
    "mlpgan_create": (C.c_int, [C.POINTER(MlpConfig), C.POINTER(_P)]),
    "mlpgan_destroy": (C.c_int, [_P]),
    "mlpgan_param_count": (_I64, [_P, C.c_int]),
    "mlpgan_param_tensors": (_I32, [_P, C.c_int]),
    "mlpgan_bn_count": (_I64, [_P]),
    "mlpgan_bind": (C.c_int, [_P, C.POINTER(MlpStorage)]),
    "mlpgan_seed": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "mlpgan_g_forward": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "mlpgan_d_forward": (C.c_int, [_P, _P, _I32, _P, _P]),
    "mlpgan_d_step": (C.c_int, [_P, _P, _I32, _P, C.POINTER(Hyper), _P, _P]),
    "mlpgan_g_step": (C.c_int, [_P, _I32, _P, C.POINTER(Hyper), _P, _P]),
    "mlpgan_op_gemm": (C.c_int, [_I32, _I32, _P, _P, _P, _I32, _I32, _I32, _P]),
}
EXPORTS = tuple(_SIGNATURES)
# Siamese signature verifier, eval-mode forward (include/siggan_verifier.h): new symbols beside ABI 4, listed on their own
_VERIFIER_SIGNATURES = {
    "siggan_verifier_create": (C.c_int, [_I32, _I32, _I32, C.POINTER(_P)]),
    "siggan_verifier_destroy": (C.c_int, [_P]),
    "siggan_verifier_bind": (C.c_int, [_P, C.POINTER(VerifierWeights), _P]),
    "siggan_verifier_embed": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "siggan_verifier_compare": (C.c_int, [_P, _P, _P, _I32, _P, _P]),
    "siggan_verifier_score": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "siggan_verifier_debug_tensor": (C.c_int, [_P, C.c_char_p, _P, _I64, _P]),
}
VERIFIER_EXPORTS = tuple(_VERIFIER_SIGNATURES)
# the verifier's eval-mode input gradient (include/siggan_verifier_grad.h): again only new symbols, on the same context
_VERIFIER_GRAD_SIGNATURES = {
    "siggan_verifier_input_grad_enable": (C.c_int, [_P]),
    "siggan_verifier_input_grad": (C.c_int, [_P, _P, _P, _I32, C.POINTER(VerifierIdentity), _P, _P, _P, _P, _P, _P]),
    "siggan_verifier_input_grad_debug": (C.c_int, [_P, C.c_char_p, _P, _I64, _P]),
}
VERIFIER_GRAD_EXPORTS = tuple(_VERIFIER_GRAD_SIGNATURES)

# the verifier's pair head over every (query, reference) pair (include/siggan_verifier_pairs.h): new symbols, same context
PAIR_MAX_DIM, PAIR_MAX_THRESHOLDS = 1024, 4096


class PairOutputs(C.Structure):           # siggan_pair_outputs
    _fields_ = [("score_dev", C.c_void_p), ("threshold_dev", C.c_void_p), ("n_thresholds", C.c_int32),
                ("genuine_count_dev", C.c_void_p), ("impostor_count_dev", C.c_void_p),
                ("best_genuine_dev", C.c_void_p), ("best_genuine_index_dev", C.c_void_p),
                ("best_impostor_dev", C.c_void_p), ("best_impostor_index_dev", C.c_void_p)]


_VERIFIER_PAIRS_SIGNATURES = {
    "siggan_verifier_pairs_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "siggan_verifier_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.POINTER(PairOutputs), C.c_void_p]),
}
VERIFIER_PAIRS_EXPORTS = tuple(_VERIFIER_PAIRS_SIGNATURES)

# per-row top-k lists out of the same pass (include/siggan_verifier_topk.h): new symbols again, listed on their own
PAIR_TOPK_MAX = 16


class PairTopk(C.Structure):              # siggan_pair_topk
    _fields_ = [("impostor_score_dev", C.c_void_p), ("impostor_index_dev", C.c_void_p),
                ("genuine_score_dev", C.c_void_p), ("genuine_index_dev", C.c_void_p)]


_VERIFIER_TOPK_SIGNATURES = {
    "siggan_verifier_pairs_topk_enable": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "siggan_verifier_pairs_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.POINTER(PairTopk), C.c_void_p]),
}
VERIFIER_TOPK_EXPORTS = tuple(_VERIFIER_TOPK_SIGNATURES)

# the verifier's train step (include/siggan_verifier_train.h): again only new symbols
VT_PARAM_TENSORS, VT_METRICS = 20, 4
VT_RUNNING_FIELDS = ("bn1_running_mean", "bn1_running_var", "bn2_running_mean", "bn2_running_var", "bn3_running_mean",
                     "bn3_running_var")


class VerifierTrainStorage(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("params", "grads", "exp_avg", "exp_avg_sq") + VT_RUNNING_FIELDS] + [("bn_eps", C.c_float)]


_D = C.c_double
_VERIFIER_TRAIN_SIGNATURES = {
    "siggan_verifier_trainer_create": (C.c_int, [_I32, _I32, _I32, C.POINTER(_P)]),
    "siggan_verifier_trainer_destroy": (C.c_int, [_P]),
    "siggan_verifier_trainer_param_count": (_I64, [_P]),
    "siggan_verifier_trainer_param_span": (C.c_int, [_P, _I32, C.POINTER(_I64), C.POINTER(_I64)]),
    "siggan_verifier_trainer_bind": (C.c_int, [_P, C.POINTER(VerifierTrainStorage), _I64]),
    "siggan_verifier_trainer_seed": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "siggan_verifier_train_grads": (C.c_int, [_P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _P, _P]),
    "siggan_verifier_train_apply": (C.c_int, [_P, _D, _D, _D, _D, _P]),
    "siggan_verifier_train_step": (C.c_int, [_P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _D, _D, _D, _D, _P, _P]),
    "siggan_verifier_train_debug": (C.c_int, [_P, C.c_char_p, _P, _I64, _P]),
}
VERIFIER_TRAIN_EXPORTS = tuple(_VERIFIER_TRAIN_SIGNATURES)

# the verifier trainer's input pipeline (include/siggan_verifier_data.h): one more symbol, listed on its own
_VERIFIER_DATA_SIGNATURES = {
    "siggan_pairs_augment": (C.c_int, [_I32, _P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _P]),
}
VERIFIER_DATA_EXPORTS = tuple(_VERIFIER_DATA_SIGNATURES)

# streaming fp64 feature moments (include/siggan_moments.h): new symbols again, listed on their own
MOMENTS_MAX_DIM = 1024
_MOMENTS_SIGNATURES = {
    "siggan_moments_create": (C.c_int, [_I32, _I32, C.POINTER(_P)]),
    "siggan_moments_destroy": (C.c_int, [_P]),
    "siggan_moments_reset": (C.c_int, [_P, _P]),
    "siggan_moments_update": (C.c_int, [_P, _P, _I32, _P]),
    "siggan_moments_read": (C.c_int, [_P, _P, _P, C.POINTER(_I64), _P]),
}
MOMENTS_EXPORTS = tuple(_MOMENTS_SIGNATURES)

# ranking and gathering of realism-filtered generation (include/siggan_select.h): context-free, new symbols again
SELECT_MAX = 65536
_SELECT_SIGNATURES = {
    "siggan_select_topk": (C.c_int, [_I32, _P, _I32, _I32, _P, _P]),
    "siggan_gather_u8": (C.c_int, [_I32, _P, _I32, _I64, _P, _I32, _I32, _P, _P]),
}
SELECT_EXPORTS = tuple(_SELECT_SIGNATURES)

# exact fp64 k-nearest-neighbour lists and ball counts (include/siggan_neighbors.h): context-free, new symbols again
KNN_MAX_K, KNN_MAX_DIM = 16, 1024
_NEIGHBORS_SIGNATURES = {
    "siggan_knn": (C.c_int, [_I32, _P, _I32, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "siggan_ball_count": (C.c_int, [_I32, _P, _I32, _P, _I32, _I32, _P, _P, _P]),
}
NEIGHBORS_EXPORTS = tuple(_NEIGHBORS_SIGNATURES)

# greedy farthest-point selection among feature rows (include/siggan_diverse.h): context-free, new symbols again
DIVERSE_MAX_N, DIVERSE_MAX_DIM, DIVERSE_ROW_TILE = 65536, 1024, 32
_DIVERSE_SIGNATURES = {
    "siggan_select_diverse_workspace": (C.c_size_t, [_I32]),
    "siggan_select_diverse": (C.c_int, [_I32, _P, _I32, _I32, _P, _P, _I32, _I32, C.c_double, _P, _P, _P, _P, _P, C.c_size_t, _P]),
}
DIVERSE_EXPORTS = tuple(_DIVERSE_SIGNATURES)

# Pillow's antialiased bilinear resize, bytes and fp32 with its transpose (include/siggan_resize.h): new symbols again
RESIZE_MAX_IN, RESIZE_MAX_OUT = 1024, 128
_RESIZE_SIGNATURES = {
    "siggan_resize_create": (C.c_int, [_I32, C.POINTER(_P)]),
    "siggan_resize_destroy": (C.c_int, [_P]),
    "siggan_resize_ksize": (_I32, [_I32, _I32]),
    "siggan_resize_table": (C.c_int, [_I32, _I32, _P, _P, _P]),
    "siggan_resize_u8": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _I32, _I32, _P]),
    "siggan_resize_f32": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _I32, _I32, _P]),
    "siggan_resize_f32_adjoint": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _I32, _I32, _P]),
}
RESIZE_EXPORTS = tuple(_RESIZE_SIGNATURES)

# connected ink components of byte images (include/siggan_components.h): context-free, one more symbol
CC_MAX_SIZE, CC_COUNT = 128, 9
_COMPONENTS_SIGNATURES = {
    "siggan_components_u8": (C.c_int, [_I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
}
COMPONENTS_EXPORTS = tuple(_COMPONENTS_SIGNATURES)

# single-scale SSIM between byte images (include/siggan_ssim.h): context-free, new symbols again
SSIM_TAPS, SSIM_SIGMA, SSIM_MIN_HEIGHT, SSIM_MIN_WIDTH, SSIM_MAX_SIZE = 11, 1.5, 11, 12, 128
SSIM_ALL, SSIM_SAME_SET, SSIM_PAIRED = 0, 1, 2
_SSIM_SIGNATURES = {
    "siggan_ssim_window": (C.c_int, [C.POINTER(C.c_float)]),
    "siggan_ssim_maps_bytes": (_I64, [_I32, _I32, _I32]),
    "siggan_ssim_prepare_u8": (C.c_int, [_I32, _P, _I32, _I32, _I32, _P, _P]),
    "siggan_ssim_pairs": (C.c_int, [_I32, _P, _P, _I32, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
}
SSIM_EXPORTS = tuple(_SSIM_SIGNATURES)

# stroke geometry of byte images (include/siggan_strokes.h): context-free, one more symbol
SK_MAX_SIZE, SK_WIDTH_BINS, SK_MAX_RADIUS2, SK_COUNT = 128, 16, 36, 23
_STROKES_SIGNATURES = {
    "siggan_strokes_u8": (C.c_int, [_I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
}
STROKES_EXPORTS = tuple(_STROKES_SIGNATURES)

# ink moments of signature images and their pixel gradient (include/siggan_shape.h): context-free, new symbols again
SHAPE_FEATURES, SHAPE_SUMS, SHAPE_SYY_MIN = 8, 6, 1e-12
_SHAPE_SIGNATURES = {
    "siggan_shape_f32": (C.c_int, [_I32, _P, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "siggan_shape_u8": (C.c_int, [_I32, _P, _I32, _I32, _P, _P]),
}
SHAPE_EXPORTS = tuple(_SHAPE_SIGNATURES)

# quadratic forms of an implicit kernel matrix with 0/1 group indicators (include/siggan_twosample.h): context-free, new symbols again
KERNEL_POLY, KERNEL_RBF = 0, 1
TWOSAMPLE_MAX_N, TWOSAMPLE_MAX_COLS, TWOSAMPLE_MAX_DIM, TWOSAMPLE_ROW_BLOCK = 16384, 4096, 1024, 32


class KernelSpec(C.Structure):            # siggan_kernel_spec
    _fields_ = [("kind", C.c_int32), ("degree", C.c_int32), ("gamma", C.c_double), ("coef0", C.c_double)]


_TWOSAMPLE_SIGNATURES = {
    "siggan_kernel_forms_workspace": (C.c_size_t, [_I32, _I32]),
    "siggan_kernel_forms": (C.c_int, [_I32, _P, _I32, _I32, C.POINTER(KernelSpec), _P, _I32, _P, _P, _P, C.c_size_t, _P]),
}
TWOSAMPLE_EXPORTS = tuple(_TWOSAMPLE_SIGNATURES)

# banded dynamic time warping between column profiles of byte images (include/siggan_dtw.h): context-free, new symbols again
DTW_MAX_SIZE = 128
DTW_ALL, DTW_SAME_SET, DTW_PAIRED = 0, 1, 2
_DTW_SIGNATURES = {
    "siggan_dtw_profiles_u8": (C.c_int, [_I32, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "siggan_dtw_pairs": (C.c_int, [_I32, _P, _I32, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
}
DTW_EXPORTS = tuple(_DTW_SIGNATURES)

# scan preprocessing over a ragged batch (include/siggan_preprocess.h): context-free, new symbols again
PP_MIN_SIDE, PP_MAX_SIDE, PP_MAX_MARGIN, PP_MAX_BATCH, PP_COUNT = 16, 1024, 64, 65536, 13
PP_NO_BBOX, PP_DEGENERATE, PP_OVERFLOW = 1, 2, 4


class PreprocessOptions(C.Structure):     # siggan_preprocess_options
    _fields_ = [(n, C.c_int32) for n in ("target", "denoise", "crop", "center", "equalize", "margin")]


_PREPROCESS_SIGNATURES = {
    "siggan_preprocess_workspace": (C.c_size_t, [_I64, _I32]),
    "siggan_preprocess_u8": (C.c_int, [_I32, _P, _I64, _P, _P, _I32, C.POINTER(PreprocessOptions), _P, _P, _P, _P, _P, C.c_size_t, _P]),
}

# the signature duplicator: smooth random warps of byte images (include/siggan_warp.h): context-free, one more symbol
WARP_MAX_SIZE, WARP_PARAMS, WARP_MAX_N, WARP_CELLS, WARP_STREAM, WARP_MAX_CTRL = 128, 12, 1 << 20, (8, 16, 32), 0x57415250, 8192
_WARP_SIGNATURES = {
    "siggan_warp_u8": (C.c_int, [_I32, _P, _I64, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, C.c_uint64, _P]),
}

# k-means++ seeding and Lloyd passes on feature rows (include/siggan_kmeans.h): context-free, new symbols again.  The tuple
# of names is KMEANS_SYMBOLS, not ..._EXPORTS: tests/test_call_cpu.py counts every name ending in EXPORTS against GROUPS.
KMEANS_MAX_N, KMEANS_MAX_DIM, KMEANS_MAX_K, KMEANS_MAX_ITERATIONS, KMEANS_STREAM = 65536, 1024, 256, 1000, 0x4B4D5050
KMEANS_SUM_BLOCK, KMEANS_FEATURE_SLAB = 64, 256
_KMEANS_SIGNATURES = {
    "siggan_kmeans_workspace": (C.c_size_t, [_I32, _I32, _I32]),
    "siggan_kmeans_seed": (C.c_int, [_I32, _P, _I32, _I32, _I32, C.c_uint64, _P, _P, _P, C.c_size_t, _P]),
    "siggan_kmeans_lloyd": (C.c_int, [_I32, _P, _I32, _I32, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
}
KMEANS_SYMBOLS = tuple(_KMEANS_SIGNATURES)

# every table up to siggan_dtw.h, in the order the symbols joined the ABI: load() binds them, build() checks the library
# exports them.  GROUPS and ALL_EXPORTS stop there: tests/test_call_cpu.py pins both, their last symbol and every name
# ending in EXPORTS, and existing tests do not change.  A new header therefore adds its table to EXTRA_GROUPS below and
# nowhere else, under a name that does not end in EXPORTS.
GROUPS = (_SIGNATURES, _VERIFIER_SIGNATURES, _VERIFIER_GRAD_SIGNATURES, _VERIFIER_PAIRS_SIGNATURES, _VERIFIER_TOPK_SIGNATURES,
          _VERIFIER_TRAIN_SIGNATURES, _VERIFIER_DATA_SIGNATURES, _MOMENTS_SIGNATURES, _SELECT_SIGNATURES, _NEIGHBORS_SIGNATURES,
          _RESIZE_SIGNATURES, _COMPONENTS_SIGNATURES, _SSIM_SIGNATURES, _STROKES_SIGNATURES, _DIVERSE_SIGNATURES, _SHAPE_SIGNATURES,
          _TWOSAMPLE_SIGNATURES, _DTW_SIGNATURES)
ALL_EXPORTS = tuple(name for group in GROUPS for name in group)
# the tables of headers added since: load() binds them after GROUPS, build() checks the library exports them as well
EXTRA_GROUPS = (_PREPROCESS_SIGNATURES,)
EXTRA_SYMBOLS = tuple(name for group in EXTRA_GROUPS for name in group)
# tests/test_preprocess_cpu.py pins EXTRA_GROUPS and EXTRA_SYMBOLS whole as they stood with siggan_preprocess.h, so they stop
# there too.  Headers added after it list their tables here; load() and build() walk this tuple as they walk the two above.
# A test of a new header checks that its own table is IN this tuple, never the tuple's whole value, so it can keep growing.
ADDED_GROUPS = (_WARP_SIGNATURES, _KMEANS_SIGNATURES)
ADDED_SYMBOLS = tuple(name for group in ADDED_GROUPS for name in group)

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C signature-gan_amd/csrc`). This path has no CPU/PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for group in GROUPS + EXTRA_GROUPS + ADDED_GROUPS:
        for name, (res, args) in group.items():
            fn = getattr(lib, name)      # AttributeError if the library does not export the symbol
            fn.restype, fn.argtypes = res, args
    if lib.siggan_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libsiggan_hip.so ABI {lib.siggan_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


class SigganError(RuntimeError):
    pass


def dequant_table():
    """float32 (256,) numpy array: the value siggan_d_score_u8 gives each byte (siggan_dequant_table; needs no device)."""
    import numpy as np
    buf = (C.c_float * 256)()
    check(load().siggan_dequant_table(buf))
    return np.frombuffer(buf, dtype=np.float32).copy()


def check(rc):
    """Map a C return code to the exception the reference would raise for the same misuse."""
    if rc == 0:
        return
    msg = load().siggan_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)           # e.g. bad image size: generator_vanilla_gan.py:106-107
    raise SigganError(f"siggan error {rc}: {msg}")
