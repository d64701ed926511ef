"""ctypes binding of ``libmkb_hip.so`` (C ABI: ``include/mkb_hip.h``).

The library is the ONLY compute backend of ``mkb_amd``: if it cannot be loaded, or a tensor is not on a
ROCm device, the call raises -- there is no CPU fallback (the CPU restatement under ``oracle/`` is test
infrastructure and is never imported from here).
"""
import ctypes
import pathlib
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint16, c_uint32, c_void_p

import torch

import os

# MKB_HIP_LIB selects an experimental build of the same ABI (tools/kbench.py); default = the in-tree product library
_LIB_PATH = pathlib.Path(os.environ.get("MKB_HIP_LIB") or (pathlib.Path(__file__).resolve().parent / "libmkb_hip.so"))
ABI_VERSION = 9  # == MKB_ABI_VERSION of include/mkb_hip.h (bumped whenever a symbol or a signature changes)

MODEL_IDS = {"TransE": 0, "RotatE": 1, "ComplEx": 2, "DistMult": 3, "pRotatE": 4}
MODE_DEFAULT, MODE_HEAD, MODE_TAIL = 0, 1, 2
PART_HEAD, PART_RELATION, PART_TAIL = 0, 1, 2  # mkb_part_t
ERR_INVALID, ERR_KEY, ERR_EMPTY, ERR_UNSUPPORTED = -1, -3, -4, -5
TOPK_MAX_K, TOPK_KEEP_TARGET = 1024, 1  # MKB_TOPK_MAX_K, MKB_TOPK_KEEP_TARGET
THRESHOLD_SEARCH_MAX_N = 131072  # MKB_THRESHOLD_SEARCH_MAX_N
LOSS_MARGIN, LOSS_PAIR_LOGISTIC, LOSS_SOFTMAX = 0, 1, 2  # mkb_loss_t


def mode_id(mode):
    """models/base.py:153-164: only the two batch strings select a candidate side."""
    return MODE_HEAD if mode == "head-batch" else MODE_TAIL if mode == "tail-batch" else MODE_DEFAULT


def side_id(mode, what):
    """``mode_id`` where only the two batch strings are legal; ``what``: the caller's half of the message ("1vsAll scores")."""
    if mode_id(mode) == MODE_DEFAULT:
        raise ValueError(f"{what} one side of a triple: mode must be 'head-batch' or 'tail-batch', not {mode!r}")
    return mode_id(mode)


class Tables(Structure):
    _fields_ = [("model", c_int32), ("hidden_dim", c_int32), ("n_entity", c_int64), ("n_relation", c_int64),
                ("entity_dim", c_int64), ("relation_dim", c_int64), ("ent", c_void_p), ("rel", c_void_p),
                ("modulus", c_void_p), ("gamma", c_float), ("phase_div", c_float)]


class Grads(Structure):  # mkb_grads_t; rows_clear (default 0): see include/mkb_hip.h
    _fields_ = [("g_ent", c_void_p), ("g_rel", c_void_p), ("g_modulus", c_void_p), ("rows_clear", c_int32)]


class AdamDense(Structure):  # mkb_adam_dense_t: a small dense tensor stepped inside another launch
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("n", c_int64), ("step", c_int64)]


class AdagradDense(Structure):  # mkb_adagrad_dense_t: a small dense tensor stepped inside mkb_adagrad_step's launch
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("sum", c_void_p), ("n", c_int64)]


class RowSeg(Structure):  # mkb_row_seg_t: rows of a table shard listed by shard index (world == 0) or global entity id
    _fields_ = [("ids", c_void_p), ("n", c_int64), ("rows", c_void_p), ("world", c_int32), ("rank", c_int32),
                ("local_ids", c_void_p)]


class HipLibraryError(RuntimeError):
    pass


_lib = None

# The argument groups the row-lazy Adam calls (mkb_adam_rows_*) share, spelled once so that they cannot drift apart:
#   param, grad, exp_avg, exp_avg_sq, last, consts, n_rows, D
_ROWS_TABLE = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64]
#   step, lr, beta1, beta2, eps, rider
_ROWS_STEP = [c_int64, c_double, c_double, c_double, c_float, POINTER(AdamDense)]
#   sampler, sample, B, mode, neg, pool, pos, cnt, touched, stream (the arguments of mkb_sampler_generate)
_SAMPLER_TAIL = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]

_SIGNATURES = {
    "mkb_abi_version": (c_int, []),
    "mkb_last_error": (c_char_p, []),
    "mkb_score_fwd": (c_int, [POINTER(Tables), c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "mkb_score_bwd_workspace_bytes": (c_int64, [POINTER(Tables), c_int64, c_int64, c_int]),
    "mkb_score_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                              c_void_p, c_void_p]),
    "mkb_adversarial": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_ns_loss": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_sampler_create": (c_int, [POINTER(c_void_p), c_int64, c_int64, c_int64, c_uint32, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mkb_sampler_generate": (c_int, _SAMPLER_TAIL),
    "mkb_sampler_status": (c_int, [c_void_p, c_void_p]),
    "mkb_sampler_set_rng": (c_int, [c_void_p, c_int, ctypes.c_uint64, ctypes.c_uint64]),
    "mkb_sampler_get_rng": (c_int, [c_void_p, POINTER(c_int), POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64)]),
    "mkb_sampler_get_state": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_void_p]),
    "mkb_sampler_set_state": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "mkb_sampler_destroy": (None, [c_void_p]),
    "mkb_pool_filter": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_pool_draw_alias": (c_int, [c_void_p, c_void_p, c_int64, c_int64, ctypes.c_uint64, ctypes.c_uint64, c_void_p, c_void_p, c_void_p]),
    "mkb_pool_supported": (c_int, [POINTER(Tables), c_int64, c_int64]),
    "mkb_pool_step_workspace_bytes": (c_int64, [POINTER(Tables), c_int64, c_int64]),
    "mkb_pool_step": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                              c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_pool_step_fwd": (c_int, [POINTER(Tables), c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "mkb_pool_step_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                  c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_pool_score_fwd": (c_int, [POINTER(Tables), c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                   c_void_p, c_void_p]),
    "mkb_pool_score_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    "mkb_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_double, c_double, c_double,
                              c_float, c_int, c_void_p]),
    "mkb_adam_step_multi": (c_int, [c_void_p, c_int, c_double, c_double, c_double, c_float, c_int, c_void_p, c_void_p]),
    "mkb_profile_enable": (c_int, [c_int, c_int]),
    "mkb_profile_read": (c_int, [c_int, POINTER(c_int64), POINTER(ctypes.c_double)]),
    "mkb_adam_rows_step": (c_int, _ROWS_TABLE + [c_void_p, c_int64] + _ROWS_STEP + [c_void_p]),
    "mkb_adam_rows_advance": (c_int, _ROWS_TABLE + [c_void_p, c_int64, c_int, c_int, c_void_p, c_int64] + _ROWS_STEP
                              + [c_void_p, c_void_p]),
    "mkb_adam_rows_advance_generate": (c_int, _ROWS_TABLE + [c_int, c_int, c_void_p, c_int64] + _ROWS_STEP + _SAMPLER_TAIL),
    "mkb_adagrad_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_float,
                                 c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "mkb_rows_route": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "mkb_rows_gather": (c_int, [c_void_p, c_int64, c_int64, POINTER(RowSeg), c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                c_int64, c_void_p, c_void_p, c_void_p]),
    "mkb_rows_scatter_add": (c_int, [c_void_p, c_int64, c_int64, POINTER(RowSeg), c_int, c_void_p, c_void_p, c_int64,
                                     c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mkb_rows_blocks_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    "mkb_rows_blocks_unpack": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p]),
    "mkb_rows_comm_available": (c_int, []),
    "mkb_rows_comm_unique_id": (c_int, [c_void_p]),
    "mkb_rows_comm_create": (c_int, [c_void_p, c_int, c_int, c_int64, POINTER(c_void_p)]),
    "mkb_rows_comm_destroy": (None, [c_void_p]),
    "mkb_rows_loop_hub_create": (c_int, [c_int, POINTER(c_void_p)]),
    "mkb_rows_loop_hub_destroy": (None, [c_void_p]),
    "mkb_rows_comm_create_loopback": (c_int, [c_void_p, c_int, c_int64, POINTER(c_void_p)]),
    "mkb_rows_comm_plan": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_void_p, c_void_p, c_void_p]),
    "mkb_rows_comm_take": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mkb_rows_comm_exchange": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_rows_comm_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "mkb_check_ids": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "mkb_kl_divergence": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_debug_sclk_mhz": (c_int, [c_void_p, c_void_p]),
    "mkb_rank_workspace_bytes": (c_int64, [POINTER(Tables), c_int64]),
    "mkb_rank": (c_int, [POINTER(Tables), c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                         c_void_p]),
    "mkb_rank_scores": (c_int, [POINTER(Tables), c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                c_void_p]),
    "mkb_topk_workspace_bytes": (c_int64, [POINTER(Tables), c_int64, c_int]),
    "mkb_topk": (c_int, [POINTER(Tables), c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                         c_int64, c_void_p]),
    "mkb_topk_masked": (c_int, [POINTER(Tables), c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p,
                                c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_topk_block": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "mkb_topk_nearest_workspace_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "mkb_topk_nearest": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                 c_void_p, c_int64, c_void_p]),
    "mkb_topk_nearest_dists": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_relation_fanout": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "mkb_rank_metrics": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "mkb_threshold_search_workspace_bytes": (c_int64, [c_int64, c_int]),
    "mkb_threshold_search": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_threshold_accuracy": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "mkb_rel_scores": (c_int, [POINTER(Tables), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "mkb_rel_rank_workspace_bytes": (c_int64, [POINTER(Tables), c_int64]),
    "mkb_rel_rank": (c_int, [POINTER(Tables), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_rel_topk_workspace_bytes": (c_int64, [POINTER(Tables), c_int64, c_int]),
    "mkb_rel_topk": (c_int, [POINTER(Tables), c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                             c_void_p]),
    "mkb_cand_score_fwd": (c_int, [POINTER(Tables), c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "mkb_cand_score_bwd_workspace_bytes": (c_int64, [POINTER(Tables), c_int64, c_int64, c_int]),
    "mkb_cand_score_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                   c_int64, c_void_p]),
    "mkb_reg_rows_workspace_bytes": (c_int64, [POINTER(Tables), c_int64]),
    "mkb_reg_rows": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_all_step_workspace_bytes": (c_int64, [POINTER(Tables), c_int64]),
    "mkb_all_score_fwd": (c_int, [POINTER(Tables), c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_all_softmax": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "mkb_all_score_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                  c_void_p]),
    "mkb_all_step": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_int64, c_void_p]),
    "mkb_all_bce": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float,
                            c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_all_kvs_step": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_all_softmax_filtered": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p, c_int64,
                                         c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mkb_all_filtered_step": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float, c_float,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mkb_rel_step_workspace_bytes": (c_int64, [POINTER(Tables), c_int64]),
    "mkb_rel_score_bwd": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "mkb_rel_step": (c_int, [POINTER(Tables), POINTER(Grads), c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_int64, c_void_p]),
}
# the all-entity losses of the distance models: argument for argument the mkb_all_* call each one mirrors
_SIGNATURES.update({"mkb_dist_all_" + new: _SIGNATURES["mkb_all_" + old] for new, old in (
    ("workspace_bytes", "step_workspace_bytes"), ("score_fwd", "score_fwd"), ("score_bwd", "score_bwd"), ("step", "step"),
    ("filtered_step", "filtered_step"), ("kvs_step", "kvs_step"))})

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """Load (once) and return the ctypes handle; raises HipLibraryError if the .so is missing."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise HipLibraryError(
                f"{_LIB_PATH} not found: build it with `python -m mkb_amd.csrc.build` "
                "(mkb_amd has no CPU fallback; the HIP library is the only compute path)")
        handle = ctypes.CDLL(str(_LIB_PATH))
        handle.mkb_abi_version.restype = c_int
        if handle.mkb_abi_version() != ABI_VERSION:  # first: a stale build must say so, not fail on a missing symbol later
            raise HipLibraryError(f"ABI version mismatch: library {handle.mkb_abi_version()}, binding {ABI_VERSION} "
                                  "(rebuild with `python -m mkb_amd.csrc.build`)")
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:  # symbols are added without a version bump: a library built before this binding lacks them
                raise HipLibraryError(f"{_LIB_PATH} does not export {name}: it was built from older sources "
                                      "(rebuild with `python -m mkb_amd.csrc.build`)") from None
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


PROF_KINDS = {"pool_bwd_q": 0, "pool_fwd": 1, "adam": 2, "sampler": 3, "loss": 4, "general_fwd": 5, "general_bwd": 6,
              "pool_bwd_x": 7}


def profile_enable(kind, on=True):
    check(lib().mkb_profile_enable(PROF_KINDS[kind], int(on)), "mkb_profile_enable")


def profile_read(kind):
    """-> (launches, total_ms) of the bracketed launches since the last read (synchronises)."""
    n, ms = c_int64(), ctypes.c_double()
    check(lib().mkb_profile_read(PROF_KINDS[kind], ctypes.byref(n), ctypes.byref(ms)), "mkb_profile_read")
    return n.value, ms.value


def check(rc, what):
    if rc != 0:
        msg = lib().mkb_last_error().decode("utf-8", "replace")
        raise HipLibraryError(f"{what} failed (status {rc}): {msg}")


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mkb_amd computes on ROCm devices only (no CPU fallback): move the model and its inputs to 'cuda'. "
                f"Got a tensor on {t.device}.")


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def aligned_bytes(n, device):
    """A 256-byte aligned uint8 view of ``n`` bytes of fresh device memory (torch's caching allocator: stream-ordered)."""
    raw = torch.empty(n + 256, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 256
    return raw[off: off + n]


class Workspace:
    """The scratch of a call made in chunks: ``ptr(need)`` -> a 256-byte aligned pointer to at least ``need`` bytes of one device
    buffer (torch's caching allocator: stream-ordered), which is allocated anew only when a chunk needs more than it holds."""

    def __init__(self, device):
        self.device, self.raw = device, None

    def ptr(self, need):
        if self.raw is None or self.raw.numel() < need + 256:
            self.raw = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        return c_void_p(self.raw.data_ptr() + (-self.raw.data_ptr()) % 256)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_exchange = getattr(torch._C, "_cuda_exchangeDevice", None)


def stream_ptr(device=None):
    """torch's current stream on ``device`` (default: the current device) as the ``hipStream_t`` the C ABI takes.  Through
    torch's raw-stream query when it is there: ``torch.cuda.current_stream()`` builds a Stream object per call (~4 us -- a
    step makes four to six library calls, and small configurations are bound by exactly this host time)."""
    if _raw_stream is not None:
        idx = device.index if device is not None and getattr(device, "index", None) is not None else torch.cuda.current_device()
        return c_void_p(_raw_stream(idx))
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


class on_device:
    """``with on_device(tensor.device):`` -- ``torch.cuda.device`` without its per-call argument parsing (the library calls
    sit inside one each: launches go to the device of their operands)."""

    __slots__ = ("idx", "prev", "ctx")

    def __init__(self, device):
        self.idx = device.index if getattr(device, "index", None) is not None else torch.cuda.current_device()
        self.prev, self.ctx = -1, None

    def __enter__(self):
        if _exchange is not None:
            self.prev = _exchange(self.idx)
        else:
            self.ctx = torch.cuda.device(self.idx)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if _exchange is not None:
            if self.prev >= 0 and self.prev != self.idx:
                _exchange(self.prev)
        else:
            self.ctx.__exit__(*exc)
        return False


def contiguous(t, dtype):
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()
