"""ctypes binding of libyacht_hip.so (include/yacht_hip.h).

The product path has no CPU fallback: if the HIP library is missing, or a call fails, an
exception is raised.  Device buffers are passed as raw pointers (torch tensors'
``data_ptr()``); streams as ``hipStream_t`` integers.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
# YK_LIB_PATH: diagnostic builds only (tools/diag_select.py); the product loads the in-tree library
LIB_PATH = os.environ.get("YK_LIB_PATH") or os.path.join(HERE, "libyacht_hip.so")

YK_OK, YK_ERR_ARG, YK_ERR_HIP, YK_ERR_NOMEM, YK_ERR_CAPACITY, YK_ERR_STATE = 0, -1, -2, -3, -4, -5
YK_ERR_RANGE = -6
_ERR_NAMES = {YK_ERR_ARG: "bad argument", YK_ERR_HIP: "HIP error", YK_ERR_NOMEM: "out of device memory",
              YK_ERR_CAPACITY: "engine capacity exceeded", YK_ERR_STATE: "engine state error",
              YK_ERR_RANGE: "a value outside the range the operation accepts (a net weight with |w| >= 65520, "
                            "the fp16 split's range; sampling weights negative, NaN or without a finite positive total; "
                            "splice rows not strictly ascending within the CSR; a take index outside the CSR; "
                            "row pointers that start below 0 or decrease)"}
YK_REC_FAST = 0x100  # info[..., 6] of a fast move of the playout cap: the step status | this bit
YK_NET_ERR_SYNC = 1  # yk_net_errors: a value-head wave timed out on the v_head.2 hand-off

# per-element yk_step status -> the reference's exception (YachtGame.py:268-269, 306-307, 372, 508)
ST_OK, ST_VALUE_BID, ST_VALUE_SCORE, ST_RUNTIME, ST_ASSERT, ST_CAPACITY = 0, 1, 2, 3, 4, 5


class YkError(RuntimeError):
    def __init__(self, fn, code):
        hip = _lib.yk_last_hip_error() if _lib is not None else 0
        super().__init__(f"{fn} failed: {_ERR_NAMES.get(code, code)} (code {code}, hip error {hip})")
        self.code = code


class YkEngineConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int), ("sims", C.c_int), ("cpuct", C.c_double), ("temp_threshold", C.c_int),
                ("max_moves", C.c_int), ("prior", C.c_int), ("record_predictions", C.c_int),
                ("max_expansions", C.c_int), ("arena_entries", C.c_int64), ("record_stride", C.c_int),
                ("groups", C.c_int), ("dual_trees", C.c_int), ("dirichlet_alpha", C.c_double),
                ("dirichlet_eps", C.c_double)]


class YkEngineConfigFull(YkEngineConfig):
    """yk_engine_config_t field for field: YkEngineConfig's 80 bytes (the struct up to the root noise, whose
    layout tests/test_root_noise_host.py pins) and, appended as in the header, the fields added since.
    This is what SelfPlayEngine passes to yk_engine_create; the bare YkEngineConfig is only good for calls
    the library rejects before it reads past those 80 bytes."""
    _fields_ = [("record_root_values", C.c_int)]


# name -> argtypes (restype int unless listed in _RESTYPE)
P = C.c_void_p
I = C.c_int
U64 = C.c_uint64
U32 = C.c_uint32
SIGNATURES = {
    "yk_version": [],
    "yk_last_hip_error": [],
    "yk_rng_draw64": [U64, U32, U64],
    "yk_init_board": [P, P, P, U64, I, P],
    "yk_step": [P, P, P, U64, P, P, P, P, P, I, P],
    "yk_valid_mask": [P, P, P, P, I, P],
    "yk_ended": [P, P, P, P, I, P],
    "yk_canonical": [P, P, P, I, P],
    "yk_score_table": [P, P, P, I, P],
    "yk_score_dice": [P, P, I, P],
    "yk_featurize": [P, P, I, P],
    "yk_key_hash": [P, P, I, P],
    "yk_hash_prior": [P, P, P, I, P],
    "yk_net_create": [C.POINTER(P), I, I, C.POINTER(P), I],
    "yk_net_predict": [P, P, P, P, I, P],
    "yk_net_predict_features": [P, P, P, P, I, P],
    "yk_net_leaf_prior": [P, P, P, P, I, P],
    "yk_net_policy_action": [P, P, P, P, I, P],
    "yk_net_destroy": [P],
    "yk_net_set_precision": [P, I],
    "yk_net_errors": [P, P],
    "yk_engine_create": [C.POINTER(P), C.POINTER(YkEngineConfig), P],
    "yk_engine_destroy": [P],
    "yk_selfplay": [P, U64, U32, P],
    "yk_arena": [P, U64, U32, P, I, I, P],
    "yk_greedy_action": [P, P, I, P],
    "yk_trainer_create": [P, I, I, P, I, P],
    "yk_trainer_destroy": [P],
    "yk_trainer_buffers": [P, P, P, P],
    "yk_trainer_backward": [P, P, P, P, P, I, P],
    "yk_trainer_apply": [P, P],
    "yk_trainer_step": [P, P, P, P, P, I, P],
    "yk_trainer_backward_soft": [P, P, P, P, P, P, P, I, P],
    "yk_trainer_step_soft": [P, P, P, P, P, P, P, I, P],
    "yk_trainer_losses": [P, P],
    "yk_trainer_epoch_loss_begin": [P, C.c_double],
    "yk_trainer_epoch_loss_end": [P, P],
    "yk_trainer_get": [P, I, P],
    "yk_trainer_set": [P, I, P, C.c_int64],
    "yk_trainer_step_count": [P],
    "yk_trainer_set_row_offset": [P, C.c_int64],
    "yk_trainer_amp_state": [P, P],
    "yk_arena_results": [P, P, P, P, P, P, P],
    "yk_engine_set_opponent_net": [P, P],
    "yk_engine_stats": [P, P],
    "yk_engine_counters": [P, P, I],
    "yk_engine_profile": [P, I],
    "yk_engine_kernel_times": [P, P, P],
    "yk_engine_records": [P, P, P, P, P, P, P, P, P, P],
    "yk_engine_predictions": [P, P, P, P, P],
    "yk_engine_root_priors": [P, P, P],
    "yk_engine_root_prior": [P, I, P],
    "yk_dirichlet_noise": [U64, P, P, P, C.c_double, P, I, P],
    "yk_engine_record_bytes": [P],
    "yk_engine_pack_records": [P, P, C.c_int64, P],
    "yk_mcts_search": [P, P, U64, P, P, I, P, P],
    "yk_mcts_reset": [P],
    "yk_examples_from_records": [P, I, I, I, I, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, P],
    "yk_examples_policies": [P, I, I, I, I, C.c_int64, C.c_int64, C.c_int64, P, P, P, C.c_int64, P, P, P],
    "yk_examples_augment": [P, P, P, P, P, C.c_int64, C.c_int64, U64, U32, I, P, P, P, P, P],
    "yk_examples_value_targets": [P, I, I, I, I, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, P, P, P, P],
    "yk_net_logits": [P, P, P, P, I, P],
    "yk_examples_metrics": [P, C.c_int64, P, P, P, P, P, P, P, P, C.c_int64, P, P, P],
    "yk_net_evaluate": [P, P, P, P, P, P, P, P, C.c_int64, I, P, P, P],
    "yk_sample_weights": [P, C.c_int64, P, P, I, C.c_double, C.c_int64, P, P, P],
    "yk_sample_cdf": [P, C.c_int64, P, P, P],
    "yk_sample_draw": [P, C.c_int64, U64, U32, U64, C.c_int64, P, P],
    "yk_reanalyse_select": [C.c_int64, U64, U64, U32, C.c_double, P, C.c_int64, P, P],
    "yk_policies_from_counts": [P, C.c_int64, P, P, P, C.c_int64, P, P, P, P],
    "yk_policies_splice": [P, P, P, C.c_int64, P, C.c_int64, P, P, P, P, P, P, C.c_int64, P, P],
    "yk_engine_set_playout_cap": [P, I, C.c_double],
    "yk_playout_schedule": [U64, U32, C.c_double, I, P],
    "yk_examples_full_rows": [P, I, I, I, I, C.c_int64, P, C.c_int64, P, P],
    "yk_policies_take": [P, P, P, C.c_int64, P, C.c_int64, P, P, P, C.c_int64, P, P],
    "yk_engine_set_forced_playouts": [P, C.c_double, I],
    "yk_policy_prune": [P, P, P, P, P, P, C.c_int64, C.c_double, C.c_double, P, P],
    "yk_engine_set_fpu": [P, I, C.c_double, C.c_double],
    "yk_fpu_pick": [P, P, P, P, P, C.c_int64, C.c_double, C.c_double, P, P, P],
    "yk_engine_set_temperatures": [P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double],
    "yk_engine_temperatures": [P, P, P],
    "yk_temperature_schedule": [C.c_double, C.c_double, C.c_double, I, P],
    "yk_temperature_pick": [P, P, P, P, C.c_int64, P, P, P],
    "yk_root_temper": [P, P, P, I, P, P],
    "yk_ema_weight": [C.c_double, C.c_int64, P],
    "yk_ema_update": [P, P, C.c_int64, C.c_float, P],
    "yk_trainer_set_ema": [P, C.c_double, I],
    "yk_trainer_ema_buffer": [P, P],
    "yk_trainer_ema_get": [P, P],
    "yk_trainer_ema_set": [P, P, C.c_int64],
    "yk_trainer_ema_state": [P, P],
    "yk_trainer_set_legal_mask": [P, I],
    "yk_examples_check_legal": [P, P, P, P, P, P, C.c_int64, P, P, P],
    "yk_examples_metrics_legal": [P, C.c_int64, P, P, P, P, P, P, P, P, C.c_int64, P, P, P],
    "yk_net_evaluate_legal": [P, P, P, P, P, P, P, P, C.c_int64, I, P, P, P],
    "yk_engine_set_score_utility": [P, I, C.c_double, C.c_double],
    "yk_score_utility": [P, P, I, C.c_double, C.c_double, P, P, P],
    "yk_examples_utility_targets": [P, I, I, I, I, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double,
                                    C.c_double, P, P, P, P],
}
_RESTYPE = {"yk_version": C.c_char_p, "yk_rng_draw64": C.c_uint64, "yk_engine_record_bytes": C.c_int64,
            "yk_trainer_step_count": C.c_int64}

# added in rounds 5-6, with the soft policy targets, the root noise, the symmetry augmentation, the
# search-value targets, the held-out evaluation, the weighted sampling, the reanalysis, the playout cap, the
# averaged weights, the forced playouts, the first-play urgency, the legal-move mask, the self-play
# temperatures and the score-margin utility (A/B baselines may predate them)
_NEWER = {"yk_engine_counters", "yk_net_errors", "yk_trainer_backward_soft", "yk_trainer_step_soft",
          "yk_engine_root_priors", "yk_dirichlet_noise", "yk_examples_augment", "yk_examples_value_targets",
          "yk_net_logits", "yk_examples_metrics", "yk_net_evaluate", "yk_sample_weights", "yk_sample_cdf",
          "yk_sample_draw", "yk_reanalyse_select", "yk_policies_from_counts", "yk_policies_splice",
          "yk_engine_root_prior", "yk_engine_set_playout_cap", "yk_playout_schedule", "yk_examples_full_rows",
          "yk_policies_take", "yk_ema_weight", "yk_ema_update", "yk_trainer_set_ema", "yk_trainer_ema_buffer",
          "yk_trainer_ema_get", "yk_trainer_ema_set", "yk_trainer_ema_state", "yk_engine_set_forced_playouts",
          "yk_policy_prune", "yk_engine_set_fpu", "yk_fpu_pick", "yk_trainer_set_legal_mask",
          "yk_examples_check_legal", "yk_examples_metrics_legal", "yk_net_evaluate_legal",
          "yk_engine_set_temperatures", "yk_engine_temperatures", "yk_temperature_schedule", "yk_temperature_pick",
          "yk_root_temper", "yk_engine_set_score_utility", "yk_score_utility", "yk_examples_utility_targets"}
_lib = None


def build() -> str:
    """Compile libyacht_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", PKG_ROOT, "-j4"], check=True)
    return LIB_PATH


def lib():
    """Load the HIP library.  Fails loudly: there is no CPU fallback for the product path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make -C {PKG_ROOT}` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        lib_ = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            if os.environ.get("YK_LIB_PATH") and name in _NEWER and not hasattr(lib_, name):
                continue  # an older diagnostic baseline (A/B): entry points added since are absent
            fn = getattr(lib_, name)
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, C.c_int)
        _lib = lib_
    return _lib


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != YK_OK:
        raise YkError(name, rc)
    return rc


def ptr(t) -> int:
    """device pointer of a torch tensor (must be on the GPU and contiguous)."""
    if not t.is_cuda:
        raise ValueError("yacht_amd kernels take device tensors")
    if not t.is_contiguous():
        raise ValueError("yacht_amd kernels take contiguous tensors")
    return t.data_ptr()


def stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream
