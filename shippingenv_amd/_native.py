"""ctypes binding of libshipenv_hip.so (the C-ABI of include/shipenv.h).

There is no fallback: if the gfx950 library is missing or fails to load,
``lib()`` raises ``NativeLibraryError``. The library is built in-tree by
``__graft_entry__.build()`` (or ``python -m shippingenv_amd.build``).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SHIPENV_LIB names another build of the same library (an A/B variant under _lib/abl)
LIB_PATH = os.environ.get("SHIPENV_LIB") or os.path.join(HERE, "_lib", "libshipenv_hip.so")
ABI_VERSION = 2  # include/shipenv.h SHIPENV_ABI_VERSION

SE_FLAG_AUTO_RESET = 1
SE_NONE = 255
SE_MAX_CARGO = (2 ** 31 - 1) // 3  # include/shipenv.h: |cargo| and |cargo + amount| stay within it

# per-env error classes (include/shipenv.h SE_ERR_*)
ERR_OK, ERR_OOB, ERR_SAME_PORT, ERR_PORT_RANGE, ERR_NOT_AT_PORT = 0, 1, 2, 3, 4
ERR_AMOUNT, ERR_NO_DEST, ERR_BAD_CATEGORY, ERR_NO_PORTS, ERR_BAD_INDEX = 5, 6, 7, 8, 9
ERR_NEED_DRAW = 10

# se_tape.used bits
USED_FUEL_GATE, USED_LOSS_TYPE, USED_BETA, USED_ARRIVE, USED_MOVED = 1, 2, 4, 8, 16

# se_sample_actions special types, se_rollout statuses
SAMPLE_RAISES, SAMPLE_NO_OTHER_PORT = -1, -2
ROLL_DONE, ROLL_MAX_STEPS, ROLL_RAISED, ROLL_ATTEMPTS, ROLL_BAD_SRC = 0, 1, 2, 3, 4
# se_rollout_plan statuses
PLAN_DONE, PLAN_END, PLAN_BAD_SRC = 0, 1, 4
# the navigator: table sentinels, se_nav_actions statuses, se_rollout_nav's extra status
NAV_INF, NAV_NONE = 0xFFFF, 255
NAV_OK, NAV_NO_DEST, NAV_UNREACHABLE = 0, 1, 2
PLAN_STUCK = 5
# se_rollout_qnet's extra status, and the agent index its action rows pad with
PLAN_RAISED = 6
QROLL_PAD = -5
# se_mcts_choose statuses
MCTS_OK, MCTS_CUT, MCTS_RAISED, MCTS_NEVER_RETURNS = 0, 1, 2, 3
MCTS_STUCK = 4  # se_mcts_choose_nav alone
MCTS_MAX_SIMULATIONS = 256
# se_sarsa_step statuses
SARSA_OK, SARSA_CUT, SARSA_RAISED, SARSA_NEVER_RETURNS = 0, 1, 2, 3
SARSA_MAX_ATTEMPTS = 64

# se_server_call ops
SERVER_STEP, SERVER_RESET_TO = 1, 2


class NativeLibraryError(RuntimeError):
    pass


class ShipEnvError(RuntimeError):
    """A negative status from the C-ABI (API misuse or a HIP failure)."""


class SeState(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in (
        "x", "y", "fuel", "cargo", "origin", "dest", "reward", "done", "err", "ep_return",
        "ep_start", "done_recs", "done_count", "reward64")]


class SeSarsaState(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("type", "a", "b", "fresh", "ep_len", "ep_return")]


class SePlanOut(C.Structure):
    """se_plan_out: what se_rollout_plan writes beside ret, counted and status (NULL: not wanted)."""
    _fields_ = [(name, C.c_void_p) for name in (
        "raised", "first_err", "first_err_at", "x", "y", "fuel", "cargo", "origin", "dest")]


class SeNavOut(C.Structure):
    """se_nav_out: what se_rollout_nav writes beside ret, counted and status (NULL: not wanted)."""
    _fields_ = [(name, C.c_void_p) for name in ("arrivals", "nav_status", "stuck_at")] + [("end", SePlanOut)]


class SeTableOut(C.Structure):
    """se_table_out: what se_rollout_sarsa writes beside ret, counted and status (NULL: not wanted)."""
    _fields_ = ([(name, C.c_void_p) for name in ("stuck_at", "sample_type", "act_type", "act_a", "act_b")] +
                [("ld", C.c_int64), ("end", SePlanOut)])


class SeQnetOut(C.Structure):
    """se_qnet_out: what se_rollout_qnet writes beside ret, counted and status (NULL: not wanted)."""
    _fields_ = [("act", C.c_void_p), ("ld", C.c_int64), ("explored", C.c_void_p), ("end", SePlanOut)]


class SeDoneRec(C.Structure):
    _fields_ = [("env", C.c_int32), ("ep_return", C.c_float), ("ep_len", C.c_int32),
                ("step", C.c_int32)]


_LIB = None


# Every symbol include/shipenv.h declares, with its argument types. The result type is int (a
# status) but for those in _RESTYPES.
_P, _i32, _i64, _u32, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
SIGNATURES = {
    "se_create": [C.POINTER(_P), C.c_int, _i64, _i64, _i32, _i32, _P, _i32, _P, _P, _P, _P, _u64, _u32],
    "se_set_ports": [_P, _i32, _P, _P, _P, _P],
    "se_bind": [_P, C.POINTER(SeState)],
    "se_reset": [_P, _P, _P],
    "se_reset_to": [_P, _P, _P, _P, _P],
    "se_step": [_P, _P, _P],
    "se_step_seq": [_P, _P, _i64, _i32, _P],
    "se_step_seq_mark": [_P, _P, _i64, _i32, _P, _P, _i32],
    "se_step_typed": [_P, _P, _P, _P, _P],
    "se_step_replay": [_P, _P, _P, _P, _P, _P],
    "se_step_agent_replay": [_P, _P, _P, _P],
    "se_observe": [_P, _P, _i64, _P],
    "se_valid_mask": [_P, _P, _P],
    "se_gen_actions": [_P, _P, _u32, _P],
    "se_sample_actions": [_P, _P, _P, _P, _u32, _P],
    "se_rollout": [_P, _P, _i64, _i32, _i32, _i64, _P, _P, _P, _P],
    "se_rollout_plan": [_P, _P, _i64, _P, _P, _P, _i64, _i32, _P, _P, _i64, _P, _P, _P, C.POINTER(SePlanOut), _P],
    "se_nav_build_host": [_i32, _i32, _P, _i32, _P, _P, _P, _P],
    "se_nav_create": [C.POINTER(_P), _P],
    "se_nav_rebuild": [_P],
    "se_nav_tables": [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_i32)],
    "se_nav_destroy": [_P],
    "se_nav_actions": [_P, C.c_double, _i32, _P, _P, _P, _P, _P, _P, _P],
    "se_rollout_nav": [_P, _P, _i64, _i32, C.c_double, _i32, _P, _i64, _P, _P, _P, C.POINTER(SeNavOut), _P],
    "se_mcts_create": [C.POINTER(_P), _P, _i32],
    "se_mcts_choose": [_P, _i32, C.c_double, _i32, _i32, _i64, _P, _P, _P, _P, _P, _P, _P],
    "se_mcts_choose_nav": [_P, _P, C.c_double, _i32, _i32, C.c_double, _i32, _i64, _P, _P, _P, _P, _P, _P, _P],
    "se_mcts_destroy": [_P],
    "se_sarsa_create": [C.POINTER(_P), _P, _i64],
    "se_sarsa_layout": [_P, C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32)],
    "se_sarsa_bind": [_P, _P, C.POINTER(SeSarsaState)],
    "se_sarsa_step": [_P, C.c_double, C.c_double, C.c_double, _i32, _i32, _i32, _u32, _P, _P, _P, _P, _P, _P],
    "se_sarsa_choose": [_P, C.c_double, _u32, _P, _P, _P, _P],
    "se_sarsa_destroy": [_P],
    "se_sarsa_create_sparse": [C.POINTER(_P), _P, _i64],
    "se_sarsa_bind_sparse": [_P, _P, _P, C.POINTER(SeSarsaState)],
    "se_sarsa_sparse_stats": [_P, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _P],
    "se_sarsa_sparse_grow": [_P, _P, _P, _i64, _P],
    "se_sarsa_sparse_home": [_i64, _i64],
    "se_rollout_sarsa": [_P, C.c_double, _P, _i64, _P, _i64, _i32, _P, _P, _P, C.POINTER(SeTableOut), _P],
    "se_rollout_qnet": [_P, _i32, C.c_double, _P, _i64, _P, _i64, _i32, _P, _P, _P, C.POINTER(SeQnetOut), _P],
    "se_qnet_create": [C.POINTER(_P), _P],
    "se_qnet_set_weights": [_P, _P, _P, _P, _P, _P, _P, _P],
    "se_policy": [_P, _P, C.c_double, _u32, _P, _i64, _P],
    "se_policy_f32": [_P, _P, C.c_double, _u32, _P, _i64, _P],
    "se_qnet_repack": [_P, _P, _P],
    "se_policy_record": [_P, _P, _P, C.c_double, _u32, _P],
    "se_policy_record_f32": [_P, _P, _P, C.c_double, _u32, _P],
    "se_qnet_destroy": [_P],
    "se_replay_create": [_P, _P, _i64],
    "se_replay_begin": [_P, _P, _P],
    "se_replay_end": [_P, _P, C.c_int32, _P],
    "se_replay_end_reset": [_P, _P, C.c_int32, _P],
    "se_step_record": [_P, _P, _P, C.c_int32, _P],
    "se_replay_size": [_P, _P, _P],
    "se_replay_sample": [_P, _i64, _P, _u32, _P, _P, _P, _P, _P, _P, _P],
    "se_replay_destroy": [_P],
    "se_qtrain_create": [_P, _P, _i64],
    "se_qtrain_bind": [_P, _P, _P, _P, _P, _P],
    "se_qtrain_pack": [_P, C.c_int32, _P],
    "se_qtrain_step": [_P, _i64, _P, _P, _P, _P, _P, _P] + [C.c_float] * 5 + [_P, _P, _P],
    "se_qtrain_step_policy": [_P, _P, _i64, _P, _P, _P, _P, _P, _P] + [C.c_float] * 5 + [_P, _P, _P],
    "se_qtrain_step_replay": [_P, _P, _P, _i64] + [C.c_float] * 5 + [_P, _i64, _P, _P],
    "se_qtrain_grad_size": [_P],
    "se_qtrain_grad": [_P, _i64, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P],
    "se_qtrain_apply": [_P, _P, _P] + [C.c_float] * 4 + [_P, _P, _P],
    "se_qtrain_destroy": [_P],
    "se_episode_stats": [_P, _P, _P],
    "se_clear_stats": [_P, _P],
    "se_done_layout": [_P, C.POINTER(_i64), C.POINTER(_i32)],
    "se_done_list": [_P, C.POINTER(_i64), C.POINTER(_i64)],
    "se_done_compact": [_P, _P, _P, _P],
    "se_get_counters": [_P, C.POINTER(_u64), C.POINTER(_u64)],
    "se_set_counters": [_P, _u64, _u64],
    "se_map_decode_luma": [C.c_char_p, C.c_size_t, _P, C.c_size_t, C.POINTER(_i32), C.POINTER(_i32)],
    "se_map_area_threshold": [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_uint8, _P, _P],
    "se_map_from_jpeg": [C.c_char_p, C.c_size_t, _i32, _i32, _P],
    "se_host_create": [C.POINTER(_P), _i32, _i32, _P, _i32, _P, _P, _P, _P],
    "se_host_set_ports": [_P, _i32, _P, _P, _P, _P],
    "se_host_step_replay": [_P, _i64, _P, _P, _P, _P, _P],
    "se_host_reset_to": [_P, _i64, _P, _P, _P, _P],
    "se_host_destroy": [_P],
    "se_host_alloc": [C.c_size_t, C.POINTER(_P)],
    "se_host_free": [_P],
    "se_server_create": [C.POINTER(_P), _P, _P],
    "se_server_call": [_P, _i32],
    "se_server_launches": [_P, C.POINTER(C.c_uint64)],
    "se_server_destroy": [_P],
    "se_destroy": [_P],
    "se_last_error": [],
    "se_abi_version": [],
}
_RESTYPES = {"se_last_error": C.c_char_p, "se_qtrain_grad_size": _i64, "se_sarsa_sparse_home": _i64}
EXPORTS = tuple(SIGNATURES)


def _ptr(t):
    """A device tensor's address as a ctypes argument (None: a null pointer)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _declare(lib):
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, C.c_int)


def lib():
    """Load the gfx950 library (once). Raises NativeLibraryError if it is unusable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch's ROCm runtime loads first. It ships its own HIP and an HSA runtime with the
    # soname libhsa-runtime64.so.1, the same soname as /opt/rocm's, which this library
    # needs: whichever is loaded first serves both HIP runtimes in the process. Loaded
    # before torch (shipping.Environment(<jpeg>) decodes the map through this library
    # before anything touches the GPU, as the reference's MCTS agent does), the
    # library's HIP later found no device once torch's runtime had initialised
    # (tests/test_compat_gpu.py::test_library_loaded_before_torch).
    import torch  # noqa: F401
    if os.environ.get("SHIPENV_LIB"):  # an A/B variant replaces the product library: say so
        import sys
        print(f"shippingenv_amd: SHIPENV_LIB overrides the library: {LIB_PATH}", file=sys.stderr, flush=True)
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    missing = [s for s in EXPORTS if not hasattr(handle, s)]
    if missing:
        raise NativeLibraryError(f"{LIB_PATH} lacks symbols {missing}")
    _declare(handle)
    if handle.se_abi_version() != ABI_VERSION:
        raise NativeLibraryError("ABI version mismatch; rebuild the library")
    _LIB = handle
    return _LIB


def check(rc):
    if rc != 0:
        msg = lib().se_last_error().decode(errors="replace")
        raise ShipEnvError(f"shipenv status {rc}: {msg}")
    return rc
