"""ctypes binding of the C ABI in include/sfhe.h.

The product library is ``sorting-fhe_amd/build/libsfhe.so`` (HIP, gfx950).
``load("oracle")`` loads ``oracle/_build/libsfhe_oracle.so``, the CPU oracle
build -- test infrastructure only (tests/, __graft_entry__.smoke and the
bench's cpu_baseline leg); product code paths call ``load()`` and fail
loudly when the HIP library is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
PRODUCT_LIB = os.path.join(PKG_ROOT, "build", "libsfhe.so")
ORACLE_LIB = os.path.join(REPO_ROOT, "oracle", "_build", "libsfhe_oracle.so")

SFHE_OK = 0
HESTD_128_CLASSIC = 0
HESTD_NOTSET = 3

# every symbol include/sfhe.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "sfhe_abi_version", "sfhe_last_error", "sfhe_backend", "sfhe_params_default",
    "sfhe_context_create", "sfhe_context_destroy", "sfhe_keygen", "sfhe_rotate_keygen",
    "sfhe_context_info", "sfhe_context_primes", "sfhe_set_plaintext_cache", "sfhe_set_quiet",
    "sfhe_sync", "sfhe_op_stats", "sfhe_encrypt", "sfhe_decrypt", "sfhe_ct_free",
    "sfhe_ct_clone", "sfhe_ct_info", "sfhe_ct_set_slots", "sfhe_ct_download", "sfhe_eval_add",
    "sfhe_eval_sub", "sfhe_eval_add_const", "sfhe_eval_mult_const", "sfhe_eval_mult_plain",
    "sfhe_eval_mult", "sfhe_eval_rotate", "sfhe_eval_rotate_sum", "sfhe_eval_chebyshev", "sfhe_sign", "sfhe_compare",
    "sfhe_direct_sort_params", "sfhe_doubled_sinc_coeffs", "sfhe_sorter_create",
    "sfhe_sorter_destroy", "sfhe_sorter_sort", "sfhe_sorter_rank", "sfhe_sorter_place",
    "sfhe_decompose", "sfhe_kernel_timing", "sfhe_kernel_timing_read",
    "sfhe_comm_uid", "sfhe_shard_rccl", "sfhe_shard_host", "sfhe_pool_bytes", "sfhe_live_contexts",
    "sfhe_serialize_lanes", "sfhe_stack_stats", "sfhe_comm_stats_reset", "sfhe_comm_stats", "sfhe_sorter_graph_nodes", "sfhe_sorter_create_rot",
    "sfhe_sorter_sort_hybrid1", "sfhe_hybrid1_params", "sfhe_sorter_graph_ntt_time",
    "sfhe_sorter_graph_family_time",
    "sfhe_sorter_sort_hybrid", "sfhe_hybrid_params", "sfhe_sorter_place_2n",
    "sfhe_bootstrap_setup", "sfhe_bootstrap_depth", "sfhe_bootstrap",
    "sfhe_sorter_sort_bitonic", "sfhe_kway_sort", "sfhe_kway_params",
    "sfhe_save", "sfhe_load", "sfhe_ct_save", "sfhe_ct_load",
    "sfhe_kway_create", "sfhe_kway_run", "sfhe_kway_destroy", "sfhe_kway_graph_nodes", "sfhe_kway_graph_family_time", "sfhe_shard_tail",
    "sfhe_key_rows",
    "sfhe_groups_rccl", "sfhe_groups_host", "sfhe_groups",
    "sfhe_encode_counts", "sfhe_bootstrap_graphs",
    "sfhe_decrypt_batch", "sfhe_decode_counts",
    "sfhe_encrypt_batch", "sfhe_sample_counts",
    "sfhe_sorter_sort_stable", "sfhe_sorter_rank_stable", "sfhe_tie_counts",
    "sfhe_const_term_counts",
    "sfhe_sorter_place_many", "sfhe_sorter_sort_records", "sfhe_sorter_records_graph_nodes", "sfhe_place_counts",
    "sfhe_select_params", "sfhe_sorter_select_ranked", "sfhe_sorter_select", "sfhe_eval_rotate_fold",
    "sfhe_select_counts",
    "sfhe_sorter_select_many", "sfhe_sorter_select_records", "sfhe_eval_rotate_fold_many", "sfhe_select_cols_counts",
    "sfhe_lex_sort_depth", "sfhe_sorter_rank_lex", "sfhe_sorter_sort_records_lex", "sfhe_sorter_select_records_lex",
    "sfhe_eval_lex_step", "sfhe_lex_counts",
    "sfhe_eval_mult_sum2", "sfhe_dot_counts",
    "sfhe_eval_mult_sum", "sfhe_sumn_counts",
    "sfhe_eval_mult_sum_many", "sfhe_sumn_batch_counts", "sfhe_ct_relabel_scale",
    "sfhe_group_params", "sfhe_sorter_group", "sfhe_eval_gate_sum_many", "sfhe_group_counts",
    "sfhe_window_params", "sfhe_sorter_window", "sfhe_eval_weight_sum_many", "sfhe_window_counts",
    "sfhe_join_params", "sfhe_sorter_join", "sfhe_eval_gate_or", "sfhe_join_counts",
]

MAX_COLUMNS = 8  # SFHE_MAX_COLUMNS
LEX_KEYS = 4  # SFHE_LEX_KEYS
FRAMES = {"rows": 0, "range": 1, "below": 2}  # SFHE_FRAME_*


class SfheError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [
        ("mult_depth", C.c_uint32),
        ("scaling_mod_size", C.c_uint32),
        ("first_mod_size", C.c_uint32),
        ("batch_size", C.c_uint32),
        ("ring_dim", C.c_uint32),
        ("security_level", C.c_int32),
        ("num_large_digits", C.c_uint32),
        ("device", C.c_int32),
        ("seed", C.c_uint64),
        ("scaling_technique", C.c_int32),
    ]


_VP = C.c_void_p
_PVP = C.POINTER(C.c_void_p)
_U32 = C.c_uint32
_PU32 = C.POINTER(C.c_uint32)
_SZ = C.c_size_t
_PSZ = C.POINTER(C.c_size_t)
_PD = C.POINTER(C.c_double)
_PI32 = C.POINTER(C.c_int32)
_PU64 = C.POINTER(C.c_uint64)

# host collectives of sfhe_shard_host (sfhe_allgather_fn / sfhe_bcast_fn)
_AG = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_BC = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)

_SIGS = {
    "sfhe_abi_version": (C.c_int, []),
    "sfhe_last_error": (C.c_char_p, []),
    "sfhe_backend": (C.c_char_p, []),
    "sfhe_params_default": (None, [C.POINTER(Params)]),
    "sfhe_context_create": (C.c_int, [C.POINTER(Params), _PVP]),
    "sfhe_context_destroy": (None, [_VP]),
    "sfhe_keygen": (C.c_int, [_VP]),
    "sfhe_rotate_keygen": (C.c_int, [_VP, _PI32, _SZ]),
    "sfhe_context_info": (C.c_int, [_VP, _PU32, _PU32, _PU32, _PU32, _PU32]),
    "sfhe_context_primes": (C.c_int, [_VP, _PU64, _SZ, _PSZ]),
    "sfhe_set_plaintext_cache": (C.c_int, [_VP, C.c_int]),
    "sfhe_set_quiet": (C.c_int, [_VP, C.c_int]),
    "sfhe_sync": (C.c_int, [_VP]),
    "sfhe_op_stats": (C.c_int, [_VP, _PU64, _PD, C.c_int]),
    "sfhe_encrypt": (C.c_int, [_VP, _PD, _SZ, _U32, _U32, _PVP]),
    "sfhe_decrypt": (C.c_int, [_VP, _VP, _PD, _SZ, _PSZ]),
    "sfhe_ct_free": (None, [_VP]),
    "sfhe_ct_clone": (C.c_int, [_VP, _PVP]),
    "sfhe_ct_info": (C.c_int, [_VP, _PU32, _PU32, _PU32]),
    "sfhe_ct_set_slots": (C.c_int, [_VP, _U32]),
    "sfhe_ct_download": (C.c_int, [_VP, _VP, _PU64, _SZ]),
    "sfhe_eval_add": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_eval_sub": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_eval_add_const": (C.c_int, [_VP, _VP, C.c_double, _PVP]),
    "sfhe_eval_mult_const": (C.c_int, [_VP, _VP, C.c_double, _PVP]),
    "sfhe_eval_mult_plain": (C.c_int, [_VP, _VP, _PD, _SZ, _U32, _PVP]),
    "sfhe_eval_mult": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_eval_rotate": (C.c_int, [_VP, _VP, C.c_int32, _PVP]),
    "sfhe_eval_rotate_sum": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_int32), C.c_size_t, _PVP]),
    "sfhe_bootstrap_setup": (C.c_int, [_VP, _U32, _U32, _U32]),
    "sfhe_bootstrap_depth": (C.c_int, [_VP, _U32, _U32, _U32, _PU32]),
    "sfhe_bootstrap": (C.c_int, [_VP, _VP, _U32, _U32, _PVP]),
    "sfhe_eval_chebyshev": (C.c_int, [_VP, _VP, _PD, _SZ, C.c_double, C.c_double, _PVP]),
    "sfhe_sign": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_compare": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_direct_sort_params": (C.c_int, [_U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_doubled_sinc_coeffs": (C.c_int, [_U32, _PD, _SZ, _PSZ]),
    "sfhe_sorter_create": (C.c_int, [_VP, _U32, C.c_int, _PVP]),
    "sfhe_sorter_destroy": (None, [_VP]),
    "sfhe_sorter_sort": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_sorter_rank": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_sorter_place": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_sorter_graph_nodes": (C.c_int, [_VP, _PU64]),
    "sfhe_sorter_create_rot": (C.c_int, [_VP, _U32, C.c_int, _PI32, _SZ, _PVP]),
    "sfhe_sorter_sort_hybrid1": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_hybrid1_params": (C.c_int, [_U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_sort_hybrid": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_hybrid_params": (C.c_int, [_U32, C.c_int, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_place_2n": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_sorter_sort_bitonic": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_save": (C.c_int, [_VP, C.c_char_p]),
    "sfhe_kway_create": (C.c_int, [_VP, _U32, C.c_int, C.c_int, _PVP]),
    "sfhe_kway_run": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _U32, _PVP]),
    "sfhe_kway_destroy": (None, [_VP]),
    "sfhe_kway_graph_nodes": (C.c_int, [_VP, _PU64]),
    "sfhe_kway_graph_family_time": (C.c_int, [_VP, _U32, C.c_int, _PD, _PU64, _PD]),
    "sfhe_load": (C.c_int, [C.c_char_p, _PVP]),
    "sfhe_ct_save": (C.c_int, [_VP, _VP, C.c_char_p]),
    "sfhe_ct_load": (C.c_int, [_VP, C.c_char_p, _PVP]),
    "sfhe_kway_sort": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _U32, _PVP]),
    "sfhe_kway_params": (C.c_int, [_U32, _PU32, _PU32, _PU32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_graph_ntt_time": (C.c_int, [_VP, C.c_int, _PD, _PU64, _PD]),
    "sfhe_sorter_graph_family_time": (C.c_int, [_VP, C.c_uint32, C.c_int, _PD, _PU64, _PD]),
    "sfhe_kernel_timing": (C.c_int, [_VP, _U32, _U32]),
    "sfhe_serialize_lanes": (C.c_int, [_VP, C.c_int]),
    "sfhe_stack_stats": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_comm_stats_reset": (C.c_int, [_VP, C.c_int]),
    "sfhe_comm_stats": (C.c_int, [_VP, _PU64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sfhe_kernel_timing_read": (C.c_int, [_VP, _U32, _PU64, _PU64, _PD, _PD]),
    "sfhe_decompose": (C.c_int, [_U32, _PI32, _SZ, C.c_int32, C.c_int32, C.c_int, _PI32, _PI32, _SZ, _PSZ]),
    "sfhe_comm_uid": (C.c_int, [_VP]),
    "sfhe_pool_bytes": (C.c_int, [_VP, _PU64]),
    "sfhe_live_contexts": (C.c_int, []),
    "sfhe_shard_rccl": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "sfhe_shard_host": (C.c_int, [_VP, C.c_int, C.c_int, _AG, _BC, _VP]),
    "sfhe_shard_tail": (C.c_int, [_VP, _PU32]),
    "sfhe_key_rows": (C.c_int, [_VP, _PU32]),
    "sfhe_groups_rccl": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "sfhe_groups_host": (C.c_int, [_VP, C.c_int, C.c_int, _AG, _VP]),
    "sfhe_groups": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sfhe_encode_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_bootstrap_graphs": (C.c_int, [_VP, _PU64]),
    "sfhe_decrypt_batch": (C.c_int, [_VP, C.POINTER(_VP), _SZ, _PD, _SZ, _PSZ]),
    "sfhe_decode_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_encrypt_batch": (C.c_int, [_VP, _PD, _SZ, _PSZ, _SZ, _U32, _PU32, C.POINTER(_VP)]),
    "sfhe_sample_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_sorter_sort_stable": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_sorter_rank_stable": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_tie_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_sorter_place_many": (C.c_int, [_VP, _VP, _PVP, C.c_size_t, _PVP]),
    "sfhe_sorter_sort_records": (C.c_int, [_VP, _VP, _PVP, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _PVP,
                                           _PVP]),
    "sfhe_sorter_records_graph_nodes": (C.c_int, [_VP, _PU64]),
    "sfhe_place_counts": (C.c_int, [_VP, _PU64, _PU64, _PU64, _PU64]),
    "sfhe_const_term_counts": (C.c_int, [_VP, _PU64, _PU64, _PU64]),
    "sfhe_select_params": (C.c_int, [_U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_select_ranked": (C.c_int, [_VP, _VP, _VP, _PU32, _SZ, _PVP]),
    "sfhe_sorter_select": (C.c_int, [_VP, _VP, _PU32, _SZ, C.c_int, C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_eval_rotate_fold": (C.c_int, [_VP, _VP, C.c_int32, _U32, _PVP]),
    "sfhe_select_counts": (C.c_int, [_VP, _PU64, _PU64, _PU64]),
    "sfhe_sorter_select_many": (C.c_int, [_VP, _VP, _PVP, _SZ, _PU32, _SZ, _PVP]),
    "sfhe_sorter_select_records": (C.c_int, [_VP, _VP, _PVP, _SZ, _PU32, _SZ, C.c_int, C.c_int, C.c_int, C.c_int,
                                             _PVP, _PVP]),
    "sfhe_eval_rotate_fold_many": (C.c_int, [_VP, _PVP, _SZ, C.c_int32, _U32, _PVP]),
    "sfhe_select_cols_counts": (C.c_int, [_VP, _PU64, _PU64, _PU64]),
    "sfhe_lex_sort_depth": (C.c_int, [_U32, C.c_int, C.c_int, C.c_int, _U32, _PU32]),
    "sfhe_sorter_rank_lex": (C.c_int, [_VP, _PVP, _SZ, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, _PVP]),
    "sfhe_sorter_sort_records_lex": (C.c_int, [_VP, _PVP, _SZ, C.POINTER(C.c_int), _PVP, _SZ, C.c_int, C.c_int,
                                               C.c_int, _PVP, _PVP]),
    "sfhe_sorter_select_records_lex": (C.c_int, [_VP, _PVP, _SZ, C.POINTER(C.c_int), _PVP, _SZ, _PU32, _SZ, C.c_int,
                                                 C.c_int, C.c_int, _PVP, _PVP]),
    "sfhe_eval_lex_step": (C.c_int, [_VP, _VP, _VP, _VP, _PVP]),
    "sfhe_lex_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_eval_mult_sum2": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _PVP]),
    "sfhe_dot_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_eval_mult_sum": (C.c_int, [_VP, _PVP, _PVP, C.c_size_t, _VP, _PVP]),
    "sfhe_sumn_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_eval_mult_sum_many": (C.c_int, [_VP, _PVP, _PVP, C.POINTER(C.c_size_t), C.c_size_t, _PVP, _PVP]),
    "sfhe_sumn_batch_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_ct_relabel_scale": (C.c_int, [_VP, C.c_double, _PVP]),
    "sfhe_group_params": (C.c_int, [_U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_group": (C.c_int, [_VP, _VP, _PVP, _SZ, C.c_int, C.c_int, C.c_int, C.c_int, _PVP, _PVP, _PVP]),
    "sfhe_eval_gate_sum_many": (C.c_int, [_VP, _PVP, _SZ, _PVP, _SZ, _PVP]),
    "sfhe_group_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_window_params": (C.c_int, [_U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_window": (C.c_int, [_VP, _VP, _PVP, _SZ, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PVP, _PVP]),
    "sfhe_eval_weight_sum_many": (C.c_int, [_VP, _PVP, _SZ, C.POINTER(_PD), _SZ, _U32, _PVP, _SZ, _PVP]),
    "sfhe_window_counts": (C.c_int, [_VP, _PU64, _PU64]),
    "sfhe_join_params": (C.c_int, [_U32, _U32, _PU32, _PI32, _SZ, _PSZ]),
    "sfhe_sorter_join": (C.c_int, [_VP, _PVP, _PVP, _SZ, _PVP, _SZ, C.c_int, C.c_int, C.c_int, _PVP, _PVP]),
    "sfhe_eval_gate_or": (C.c_int, [_VP, _VP, _VP, _PVP]),
    "sfhe_join_counts": (C.c_int, [_VP, _PU64, _PU64]),
}

_libs: dict = {}


def lib_path(backend: str = "hip") -> str:
    # SFHE_PRODUCT_LIB: an alternative HIP build (tools: kernel-variant sweeps)
    return os.environ.get("SFHE_PRODUCT_LIB", PRODUCT_LIB) if backend == "hip" else ORACLE_LIB


ABI_VERSION = 3  # include/sfhe.h SFHE_ABI_VERSION


def load(backend: str = "hip"):
    """Load the engine library.  backend='hip' is the product (raises if the
    HIP build is absent); backend='oracle' is the CPU oracle (tests only)."""
    if backend in _libs:
        return _libs[backend]
    path = lib_path(backend)
    if not os.path.exists(path):
        raise SfheError(
            f"{backend} library not built: {path} is missing "
            f"(run `make -C sorting-fhe_amd` for the HIP product, `make -C oracle` for the oracle)")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    # the ctypes structures and signatures above are those of include/sfhe.h
    # at SFHE_ABI_VERSION: refuse a library built from another version
    if lib.sfhe_abi_version() != ABI_VERSION:
        raise SfheError(f"{path}: C ABI version {lib.sfhe_abi_version()}, this binding speaks {ABI_VERSION} "
                        "(rebuild the library or use the matching sfhe.py)")
    _libs[backend] = lib
    return lib


def _darr(v: Sequence[float]):
    a = (C.c_double * len(v))(*[float(x) for x in v])
    return a


class Engine:
    """Thin object wrapper; one CKKS context + key pair."""

    def __init__(self, backend: str = "hip", *, mult_depth: int, ring_dim: int = 0,
                 batch_size: int = 0, scaling_mod_size: int = 40, first_mod_size: int = 60,
                 secure: bool = False, num_large_digits: int = 0, seed: int = 0x5EED5EED2025,
                 device: int = 0, rotations: Sequence[int] = (), keygen: bool = True,
                 scaling: str = "FLEXIBLEAUTOEXT", shard=None, groups=None):
        """shard: None, ("rccl", rank, world, uid) or ("host", rank, world, comm)
        (limb sharding, include/sfhe.h; every rank passes the same params).
        groups: None, ("rccl", group, groups, uid) or ("host", group, groups,
        comm): the sort's batches split over batch groups (sfhe_groups_*)."""
        self.lib = load(backend)
        self.backend = backend
        p = Params()
        self.lib.sfhe_params_default(C.byref(p))
        p.mult_depth = mult_depth
        p.ring_dim = ring_dim
        p.batch_size = batch_size
        p.scaling_mod_size = scaling_mod_size
        p.first_mod_size = first_mod_size
        p.security_level = HESTD_128_CLASSIC if secure else HESTD_NOTSET
        p.num_large_digits = num_large_digits
        p.seed = seed
        p.device = device
        p.scaling_technique = {"FLEXIBLEAUTO": 2, "FLEXIBLEAUTOEXT": 3}[scaling]
        self.ctx = C.c_void_p()
        self._chk(self.lib.sfhe_context_create(C.byref(p), C.byref(self.ctx)))
        self._comm_refs = None
        if shard is not None:
            kind, rank, world, arg = shard
            if kind == "rccl":
                self.shard_rccl(rank, world, arg)
            elif kind == "host":
                self.shard_host(rank, world, arg)
            else:
                raise ValueError(f"unknown shard transport {kind!r}")
        if groups is not None:
            kind, g, G, arg = groups
            if kind == "rccl":
                self.groups_rccl(g, G, arg)
            elif kind == "host":
                self.groups_host(g, G, arg)
            else:
                raise ValueError(f"unknown group transport {kind!r}")
        if keygen:
            self._chk(self.lib.sfhe_keygen(self.ctx))
            if rotations:
                self.rotate_keygen(rotations)

    @classmethod
    def load(cls, directory: str, backend: str = "hip") -> "Engine":
        """A context and keys from sfhe_save's file set (src/sort.h:31-102)."""
        self = cls.__new__(cls)
        self.lib = load(backend)
        self.backend = backend
        self._comm_refs = None
        self.ctx = C.c_void_p()
        self._chk(self.lib.sfhe_load(directory.encode(), C.byref(self.ctx)))
        return self

    def save(self, directory: str):
        self._chk(self.lib.sfhe_save(self.ctx, directory.encode()))

    def save_ct(self, ct: "Ct", path: str):
        self._chk(self.lib.sfhe_ct_save(self.ctx, ct.h, path.encode()))

    def load_ct(self, path: str) -> "Ct":
        return self._new(self.lib.sfhe_ct_load, self.ctx, path.encode())

    # -- plumbing --
    def _chk(self, rc: int):
        if rc != SFHE_OK:
            raise SfheError(f"sfhe error {rc}: {self.lib.sfhe_last_error().decode()}")

    def close(self):
        if self.ctx:
            self.lib.sfhe_context_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _new(self, fn, *args) -> "Ct":
        out = C.c_void_p()
        self._chk(fn(*args, C.byref(out)))
        return Ct(self, out)

    # -- limb sharding --
    def shard_rccl(self, rank: int, world: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        self._chk(self.lib.sfhe_shard_rccl(self.ctx, rank, world, buf))

    def shard_host(self, rank: int, world: int, comm):
        """comm: object with allgather(rank, send, recv, nbytes) and
        bcast(rank, buf, nbytes, root) over raw addresses (ThreadComm, GlooComm)."""
        ag = _AG(lambda _u, send, recv, nb: comm.allgather(rank, send, recv, nb))
        bc = _BC(lambda _u, buf, nb, root: comm.bcast(rank, buf, nb, root))
        self._chk(self.lib.sfhe_shard_host(self.ctx, rank, world, ag, bc, None))
        self._comm_refs = (ag, bc, comm)  # the library keeps the raw pointers

    def groups_rccl(self, group: int, groups: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        self._chk(self.lib.sfhe_groups_rccl(self.ctx, group, groups, buf))

    def groups_host(self, group: int, groups: int, comm):
        """comm: as shard_host's (only its allgather is used)."""
        ag = _AG(lambda _u, send, recv, nb: comm.allgather(group, send, recv, nb))
        self._chk(self.lib.sfhe_groups_host(self.ctx, group, groups, ag, None))
        self._group_refs = (ag, comm)

    def groups(self):
        """(group, groups) of the batch split ((0, 1): unsplit)."""
        g, G = C.c_int(), C.c_int()
        self._chk(self.lib.sfhe_groups(self.ctx, C.byref(g), C.byref(G)))
        return g.value, G.value

    def shard_tail(self) -> int:
        """Replicated-tail limb count of a sharded context (0: unsharded)."""
        v = C.c_uint32()
        self._chk(self.lib.sfhe_shard_tail(self.ctx, C.byref(v)))
        return v.value

    def key_rows(self) -> int:
        """Rows per digit part of this rank's switching keys (a slice when sharded)."""
        v = C.c_uint32()
        self._chk(self.lib.sfhe_key_rows(self.ctx, C.byref(v)))
        return v.value

    # -- context --
    def rotate_keygen(self, idx: Sequence[int]):
        a = (C.c_int32 * len(idx))(*idx)
        self._chk(self.lib.sfhe_rotate_keygen(self.ctx, a, len(idx)))

    def info(self) -> dict:
        v = [C.c_uint32() for _ in range(5)]
        self._chk(self.lib.sfhe_context_info(self.ctx, *[C.byref(x) for x in v]))
        return dict(ring_dim=v[0].value, mult_depth=v[1].value, num_q=v[2].value,
                    num_p=v[3].value, dnum=v[4].value)

    def primes(self) -> list:
        cnt = C.c_size_t()
        self._chk(self.lib.sfhe_context_primes(self.ctx, None, 0, C.byref(cnt)))
        buf = (C.c_uint64 * cnt.value)()
        self._chk(self.lib.sfhe_context_primes(self.ctx, buf, cnt.value, None))
        return list(buf)

    def sync(self):
        self._chk(self.lib.sfhe_sync(self.ctx))

    def set_quiet(self, q: bool = True):
        self._chk(self.lib.sfhe_set_quiet(self.ctx, int(q)))

    def set_plaintext_cache(self, on: bool):
        self._chk(self.lib.sfhe_set_plaintext_cache(self.ctx, int(on)))

    def op_stats(self, reset: bool = False) -> dict:
        c = (C.c_uint64 * 9)()
        b = C.c_double()
        self._chk(self.lib.sfhe_op_stats(self.ctx, c, C.byref(b), int(reset)))
        keys = ["keyswitch", "rescale", "tensor", "ptmult", "constmult", "add", "automorph",
                "ntt_limbs", "wsum_terms"]
        d = dict(zip(keys, list(c)))
        d["algo_bytes"] = b.value
        return d

    def encode_counts(self):
        """(device, host) plaintext encodings since the last op_stats reset."""
        d, h = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_encode_counts(self.ctx, C.byref(d), C.byref(h)))
        return d.value, h.value

    def pool_bytes(self) -> int:
        v = C.c_uint64()
        self._chk(self.lib.sfhe_pool_bytes(self.ctx, C.byref(v)))
        return v.value

    KFAM = {"ntt": 0, "conv": 1, "ks_inner": 2, "ntt_ks": 3}

    def kernel_timing(self, family: str, period: int = 1):
        self._chk(self.lib.sfhe_kernel_timing(self.ctx, self.KFAM[family], period))

    def serialize_lanes(self, on: bool = True):
        self._chk(self.lib.sfhe_serialize_lanes(self.ctx, int(on)))

    def stack_stats(self):
        """(merged pairs, launches alone) issued by stacked regions so far."""
        m, s1 = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_stack_stats(self.ctx, C.byref(m), C.byref(s1)))
        return m.value, s1.value

    def comm_stats_reset(self, timed: bool = True):
        """Zero the collective counters (timed: also time each eager collective)."""
        self._chk(self.lib.sfhe_comm_stats_reset(self.ctx, 1 if timed else 0))

    def comm_stats(self) -> dict:
        """Collectives this rank issued since comm_stats_reset: calls, bytes received, ms."""
        n, by, ms = C.c_uint64(), C.c_double(), C.c_double()
        self._chk(self.lib.sfhe_comm_stats(self.ctx, C.byref(n), C.byref(by), C.byref(ms)))
        return {"calls": n.value, "bytes": by.value, "ms": ms.value}

    def kernel_timing_read(self, family: str) -> dict:
        la, ti = C.c_uint64(), C.c_uint64()
        ms, by = C.c_double(), C.c_double()
        self._chk(self.lib.sfhe_kernel_timing_read(self.ctx, self.KFAM[family], C.byref(la),
                                                   C.byref(ti), C.byref(ms), C.byref(by)))
        return {"launches": la.value, "timed": ti.value, "ms": ms.value, "bytes": by.value}

    # -- data --
    def encrypt(self, values: Sequence[float], slots: int = 0, level: int = 0) -> "Ct":
        a = _darr(values)
        return self._new(self.lib.sfhe_encrypt, self.ctx, a, len(values), slots, level)

    def encrypt_batch(self, value_lists: Sequence[Sequence[float]], slots: int = 0, levels=None) -> list:
        """[encrypt(v, slots, level) for v, level in zip(value_lists, levels)] in
        one call (levels None: level 0 throughout): the same ciphertexts, with
        the sampling, the NTTs and the sums of each level batched."""
        lists = [list(v) for v in value_lists]
        if not lists:
            return []
        if levels is not None and len(levels) != len(lists):
            raise ValueError("levels must have one entry per input")
        count, stride = len(lists), max(1, max(len(v) for v in lists))
        buf = (C.c_double * (stride * count))()
        for k, v in enumerate(lists):
            buf[k * stride:k * stride + len(v)] = v
        lens = (C.c_size_t * count)(*[len(v) for v in lists])
        lv = (C.c_uint32 * count)(*[int(x) for x in levels]) if levels is not None else None
        outs = (_VP * count)()
        self._chk(self.lib.sfhe_encrypt_batch(self.ctx, buf, stride, lens, count, slots, lv, outs))
        return [Ct(self, C.c_void_p(h)) for h in outs]

    def sample_counts(self):
        """(device, host) small polynomials sampled since the last op_stats reset."""
        d, h = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_sample_counts(self.ctx, C.byref(d), C.byref(h)))
        return d.value, h.value

    def decrypt(self, ct: "Ct") -> list:
        n = ct.slots  # (sfhe_decrypt writes min(cap, slots) values: decrypt once)
        buf = (C.c_double * n)()
        self._chk(self.lib.sfhe_decrypt(self.ctx, ct.h, buf, n, None))
        return list(buf)

    def decrypt_batch(self, cts: Sequence["Ct"]) -> list:
        """[decrypt(c) for c in cts] with one device synchronisation for the
        whole list (any mix of levels and slot counts)."""
        cts = list(cts)
        if not cts:
            return []
        stride = max(c.slots for c in cts)
        hs = (_VP * len(cts))(*[c.h for c in cts])
        buf = (C.c_double * (stride * len(cts)))()
        lens = (C.c_size_t * len(cts))()
        self._chk(self.lib.sfhe_decrypt_batch(self.ctx, hs, len(cts), buf, stride, lens))
        return [list(buf[k * stride:k * stride + lens[k]]) for k in range(len(cts))]

    def decode_counts(self):
        """(device, host) decodings of decrypted ciphertexts since the last op_stats reset."""
        d, h = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_decode_counts(self.ctx, C.byref(d), C.byref(h)))
        return d.value, h.value

    def tie_counts(self):
        """(fused, composed) tie-term tensors of the stable rank since the last op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_tie_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def lex_step(self, v, q, u):
        """v + (1 - q) * u, one level below u (one relinearisation, one rescale): the
        lexicographic rank's Horner step.  v and q may sit at a numerically lower level than u."""
        return self._new(self.lib.sfhe_eval_lex_step, self.ctx, v.h, q.h, u.h)

    def mult_sum2(self, a, b, a2, b2, r=None):
        """a*b + a2*b2 (+ r), one level below the operands, from ONE relinearisation and
        rescale (operands at one level; r, if given, at the result's level)."""
        return self._new(self.lib.sfhe_eval_mult_sum2, self.ctx, a.h, b.h, a2.h, b2.h, r.h if r is not None else None)

    def mult_sum(self, terms, r=None):
        """sum of a*b over the (a, b) pairs of terms (+ r), one level below the operands, from ONE
        relinearisation and rescale (all operands at one level; r, if given, at the result's level)."""
        n = len(terms)
        a = (C.c_void_p * n)(*[t[0].h for t in terms])
        b = (C.c_void_p * n)(*[t[1].h for t in terms])
        return self._new(self.lib.sfhe_eval_mult_sum, self.ctx, a, b, n, r.h if r is not None else None)

    def mult_sum_many(self, ops):
        """[mult_sum(terms, r) for terms, r in ops] in one call: consecutive ops of one level and one
        term count go out as one batch; each result equals the op issued alone."""
        flat = [t for terms, _ in ops for t in terms]
        n = len(flat)
        a = (C.c_void_p * n)(*[t[0].h for t in flat])
        b = (C.c_void_p * n)(*[t[1].h for t in flat])
        counts = (C.c_size_t * len(ops))(*[len(terms) for terms, _ in ops])
        r = (C.c_void_p * len(ops))(*[x.h if x is not None else None for _, x in ops])
        out = (C.c_void_p * len(ops))()
        self._chk(self.lib.sfhe_eval_mult_sum_many(self.ctx, a, b, counts, len(ops), r, out))
        return [Ct(self, C.c_void_p(h)) for h in out]

    def sumn_batch_counts(self):
        """(batches, fallbacks): runs of one level and term count that mult_sum / mult_sum_many (the
        Chebyshev evaluator's included) issued, and evaluator chains that ran as separate products."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_sumn_batch_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def relabel_scale(self, ct, factor):
        """A copy of ct with its scale label multiplied by factor (rows untouched; for tests)."""
        return self._new(self.lib.sfhe_ct_relabel_scale, ct.h, float(factor))

    def sumn_counts(self):
        """(fused, composed) mult_sum ops (the Chebyshev evaluator's included) since the last op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_sumn_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def dot_counts(self):
        """(fused, composed) mult_sum2 calls (the sign polynomials' included) since the last op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_dot_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def gate_sum_many(self, qs, us):
        """[sum_b (1 - qs[b]) * us[c][b] for each column c], one level below the gates (one
        relinearisation and one rescale per column): the grouping's gated column sums.  The
        gates share one level; operands may sit at a numerically lower level."""
        qs, us = list(qs), [list(col) for col in us]
        for col in us:
            if len(col) != len(qs):
                raise SfheError("sfhe error -1: every column needs one operand per gate")
        qh = (_VP * max(len(qs), 1))(*[q.h if q is not None else None for q in qs])
        flat = [x.h if x is not None else None for col in us for x in col]
        uh = (_VP * max(len(flat), 1))(*flat)
        outs = (_VP * max(len(us), 1))()
        self._chk(self.lib.sfhe_eval_gate_sum_many(self.ctx, qh, len(qs), uh, len(us), outs))
        return [Ct(self, C.c_void_p(outs[i])) for i in range(len(us))]

    def group_counts(self):
        """(fused, composed) gate_sum_many calls (Sorter.group's included) since the last
        op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_group_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def weight_sum_many(self, vs, weights, us, slots: int = 0):
        """[sum_b (weights[b] + vs[b]) * us[c][b] for each column c], one level below the gates
        (one relinearisation and one rescale per column): the window sums' weighted column sums.
        weights[b] is a vector of slot values, encoded at vs' scale; the gates share one level;
        operands may sit at a numerically lower level."""
        vs, us = list(vs), [list(col) for col in us]
        weights = [[float(x) for x in w] for w in weights]
        if len(weights) != len(vs):
            raise SfheError("sfhe error -1: one weight vector per gate is needed")
        if len({len(w) for w in weights}) > 1:
            raise SfheError("sfhe error -1: the weight vectors must have one length")
        for col in us:
            if len(col) != len(vs):
                raise SfheError("sfhe error -1: every column needs one operand per gate")
        vh = (_VP * max(len(vs), 1))(*[v.h if v is not None else None for v in vs])
        rows = [_darr(w) for w in weights]
        wh = (_PD * max(len(rows), 1))(*[C.cast(r, _PD) for r in rows])
        flat = [x.h if x is not None else None for col in us for x in col]
        uh = (_VP * max(len(flat), 1))(*flat)
        outs = (_VP * max(len(us), 1))()
        self._chk(self.lib.sfhe_eval_weight_sum_many(self.ctx, vh, len(vs), wh, len(weights[0]) if weights else 0,
                                                     slots, uh, len(us), outs))
        return [Ct(self, C.c_void_p(outs[i])) for i in range(len(us))]

    def window_counts(self):
        """(fused, composed) weight_sum_many calls (Sorter.window's included) since the last
        op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_window_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def gate_or(self, a, b):
        """a + b - a * b (the OR of two 0/1 gates), one level below the lower operand (one
        relinearisation and one rescale); the operands may sit at different levels."""
        return self._new(self.lib.sfhe_eval_gate_or, self.ctx, a.h, b.h)

    def join_counts(self):
        """(fused, composed) gate_or calls (Sorter.join's included) since the last op_stats
        reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_join_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def lex_counts(self):
        """(fused, composed) lex_step tensors (rank_lex's included) since the last op_stats reset."""
        f, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_lex_counts(self.ctx, C.byref(f), C.byref(c)))
        return f.value, c.value

    def place_counts(self):
        """(hits, columns, fused, composed) of multi-column placements since the last op_stats
        reset: indicators evaluated, columns they served, giant-step sums formed by
        sfp_mac_plain2_cols and by the per-column path."""
        v = [C.c_uint64() for _ in range(4)]
        self._chk(self.lib.sfhe_place_counts(self.ctx, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def const_term_counts(self):
        """(merged, single, composed) constant terms c*x since the last op_stats reset: inside a
        multi-term launch, as one fused constant rescale, as a weighted sum then a rescale."""
        m, s1, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.sfhe_const_term_counts(self.ctx, C.byref(m), C.byref(s1), C.byref(c)))
        return m.value, s1.value, c.value

    # -- eval --
    def add(self, a, b):
        return self._new(self.lib.sfhe_eval_add, self.ctx, a.h, b.h)

    def sub(self, a, b):
        return self._new(self.lib.sfhe_eval_sub, self.ctx, a.h, b.h)

    def add_const(self, a, k: float):
        return self._new(self.lib.sfhe_eval_add_const, self.ctx, a.h, float(k))

    def mult_const(self, a, k: float):
        return self._new(self.lib.sfhe_eval_mult_const, self.ctx, a.h, float(k))

    def mult_plain(self, a, values: Sequence[float], slots: int = 0):
        return self._new(self.lib.sfhe_eval_mult_plain, self.ctx, a.h, _darr(values), len(values), slots)

    def mult(self, a, b):
        return self._new(self.lib.sfhe_eval_mult, self.ctx, a.h, b.h)

    def rotate(self, a, r: int):
        return self._new(self.lib.sfhe_eval_rotate, self.ctx, a.h, int(r))

    def rotate_sum(self, cts, rots):
        """sum_k rotate(cts[k], rots[k]) with one shared ModDown (EvalRotateSum)."""
        hs = (_VP * len(cts))(*[c.h for c in cts])
        rs = (C.c_int32 * len(rots))(*[int(r) for r in rots])
        return self._new(self.lib.sfhe_eval_rotate_sum, self.ctx, hs, rs, len(cts))

    def rotate_fold(self, a, stride: int, count: int):
        """sum_{k < count} rotate(a, k * stride), 2 <= count <= 8, with one ModUp and one ModDown
        (EvalRotateFold); every amount that is no multiple of a's slot count needs its key."""
        return self._new(self.lib.sfhe_eval_rotate_fold, self.ctx, a.h, int(stride), int(count))

    def select_counts(self):
        """(batches, fold_fused, fold_composed) since the last op_stats reset: indicator batches
        the selections ran, rotate_fold calls (the selections' included) whose inner products
        were one launch / composed of the generic primitives."""
        v = [C.c_uint64() for _ in range(3)]
        self._chk(self.lib.sfhe_select_counts(self.ctx, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def rotate_fold_many(self, cts, stride: int, count: int) -> list:
        """[rotate_fold(ct, stride, count) for ct in cts], the same residues, for ciphertexts at
        one level and slot count: on the device the key inner products of all of them run as
        tiles of columns that read each rotation key once (EvalRotateFoldMany)."""
        cts = list(cts)
        hs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        outs = (_VP * max(len(cts), 1))()
        self._chk(self.lib.sfhe_eval_rotate_fold_many(self.ctx, hs, len(cts), int(stride), int(count), outs))
        return [Ct(self, C.c_void_p(outs[k])) for k in range(len(cts))]

    def select_cols_counts(self):
        """(columns, fused, composed) since the last op_stats reset: columns the multi-column
        selections served, rotate_fold_many's launches of the column-tiled kernel, columns it
        passed to rotate_fold's path."""
        v = [C.c_uint64() for _ in range(3)]
        self._chk(self.lib.sfhe_select_cols_counts(self.ctx, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def bootstrap_setup(self, level_budget=(5, 5), slots: int = 0):
        """EvalBootstrapSetup + EvalBootstrapKeyGen for `slots`-slot ciphertexts."""
        self._chk(self.lib.sfhe_bootstrap_setup(self.ctx, level_budget[0], level_budget[1], slots))

    def bootstrap_depth(self, level_budget=(5, 5), slots: int = 0) -> int:
        v = C.c_uint32()
        self._chk(self.lib.sfhe_bootstrap_depth(self.ctx, level_budget[0], level_budget[1], slots, C.byref(v)))
        return v.value

    def bootstrap_graphs(self) -> int:
        """Bootstrap shapes replayed from a captured hipGraph so far."""
        v = C.c_uint64()
        self._chk(self.lib.sfhe_bootstrap_graphs(self.ctx, C.byref(v)))
        return v.value

    def bootstrap(self, a, iterations: int = 1, precision: int = 0):
        return self._new(self.lib.sfhe_bootstrap, self.ctx, a.h, iterations, precision)

    def kway(self, k: int, M: int) -> "KWay":
        """A persistent KWayAdapter<k^M> (reuses its encoded masks across sorts)."""
        h = C.c_void_p()
        self._chk(self.lib.sfhe_kway_create(self.ctx, k ** M, k, M, C.byref(h)))
        return KWay(self, h)

    def kway_sort(self, a, k: int, M: int, n: int = 3, dg: int = 2, df: int = 2, mult_depth: int = 40):
        """KWayAdapter<k^M>::sort (reference kway_adapter.h:66-72): the k-way
        network with CompositeSign(n, dg, df) and lazy bootstrapping."""
        return self._new(self.lib.sfhe_kway_sort, self.ctx, a.h, k, M, n, dg, df, mult_depth)

    def chebyshev(self, x, coeffs: Sequence[float], a: float = -1.0, b: float = 1.0):
        return self._new(self.lib.sfhe_eval_chebyshev, self.ctx, x.h, _darr(coeffs), len(coeffs),
                         float(a), float(b))

    def sign(self, x, n: int, dg: int, df: int):
        return self._new(self.lib.sfhe_sign, self.ctx, x.h, n, dg, df)

    def compare(self, a, b, n: int, dg: int, df: int):
        return self._new(self.lib.sfhe_compare, self.ctx, a.h, b.h, n, dg, df)

    def sorter(self, N: int, debug: bool = False, rotations=None) -> "Sorter":
        """DirectSort<N>; rotations = the constructor's rotIndices (None: the
        getSizeParameters list)."""
        h = C.c_void_p()
        if rotations is None:
            self._chk(self.lib.sfhe_sorter_create(self.ctx, N, int(debug), C.byref(h)))
        else:
            buf = (C.c_int32 * len(rotations))(*rotations)
            self._chk(self.lib.sfhe_sorter_create_rot(self.ctx, N, int(debug), buf, len(rotations), C.byref(h)))
        return Sorter(self, h, N)


class Ct:
    def __init__(self, eng: Engine, h):
        self.eng = eng
        self.h = h

    def __del__(self):
        try:
            if self.h:
                self.eng.lib.sfhe_ct_free(self.h)
                self.h = None
        except Exception:
            pass

    def info(self) -> dict:
        v = [C.c_uint32() for _ in range(3)]
        self.eng._chk(self.eng.lib.sfhe_ct_info(self.h, *[C.byref(x) for x in v]))
        return dict(level=v[0].value, slots=v[1].value, limbs=v[2].value)

    @property
    def level(self) -> int:
        return self.info()["level"]

    @property
    def slots(self) -> int:
        return self.info()["slots"]

    def set_slots(self, s: int):
        self.eng._chk(self.eng.lib.sfhe_ct_set_slots(self.h, s))

    def clone(self) -> "Ct":
        return self.eng._new(self.eng.lib.sfhe_ct_clone, self.h)

    def download(self):
        import numpy as np
        n = self.eng.info()["ring_dim"]
        words = 2 * self.info()["limbs"] * n
        buf = np.empty(words, dtype=np.uint64)
        self.eng._chk(self.eng.lib.sfhe_ct_download(
            self.eng.ctx, self.h, buf.ctypes.data_as(_PU64), words))
        return buf


class Sorter:
    def __init__(self, eng: Engine, h, N: int):
        self.eng, self.h, self.N = eng, h, N

    def __del__(self):
        try:
            if self.h:
                self.eng.lib.sfhe_sorter_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def sort(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        return self.eng._new(self.eng.lib.sfhe_sorter_sort, self.h, ct.h, n, dg, df)

    def rank(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        return self.eng._new(self.eng.lib.sfhe_sorter_rank, self.h, ct.h, n, dg, df)

    def sort_stable(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        """Tie-aware sort: duplicate values sort, equal values in input order.
        Needs mult_depth = direct_sort_params' depth + 1 (SfheError otherwise)."""
        return self.eng._new(self.eng.lib.sfhe_sorter_sort_stable, self.h, ct.h, n, dg, df)

    def rank_stable(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        """#{j : x_j < x_r} + #{j < r : x_j = x_r}; one level below rank()'s."""
        return self.eng._new(self.eng.lib.sfhe_sorter_rank_stable, self.h, ct.h, n, dg, df)

    def place(self, rank: Ct, ct: Ct) -> Ct:
        return self.eng._new(self.eng.lib.sfhe_sorter_place, self.h, rank.h, ct.h)

    def place_many(self, rank: Ct, cts) -> list:
        """place(rank, ct) of every column with ONE indicator evaluation per batch: the same
        residues as the separate calls.  Payload values must lie in [-1, 1]."""
        cts = list(cts)
        hs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_place_many(self.h, rank.h, hs, len(cts), outs))
        return [Ct(self.eng, C.c_void_p(outs[k])) for k in range(len(cts))]

    def sort_records(self, keys: Ct, cts=(), stable: bool = True, n: int = 3, dg: int = 2, df: int = 2):
        """(sorted keys, [columns in the keys' order]); stable: equal keys keep their input
        order and the context needs direct_sort_params' depth + 1 (SfheError otherwise)."""
        cts = list(cts)
        hs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        outs = (_VP * max(len(cts), 1))()
        k = C.c_void_p()
        self.eng._chk(self.eng.lib.sfhe_sorter_sort_records(self.h, keys.h, hs, len(cts), int(bool(stable)), n, dg,
                                                            df, C.byref(k), outs))
        return Ct(self.eng, k), [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))]

    @staticmethod
    def _targets(targets):
        t = [int(x) for x in targets]
        if any(x < 0 for x in t):
            raise SfheError("sfhe error -1: target rank out of range (0 .. N - 1)")
        return (C.c_uint32 * max(len(t), 1))(*t), len(t)

    def select_ranked(self, rank: Ct, ct: Ct, targets) -> Ct:
        """Slot i < len(targets) of the N-slot result holds the element of `ct` whose rank (in
        `rank`: rank() / rank_stable() of ct or of a key column) is targets[i]; the other slots
        hold 0 up to noise.  Distinct ranks in [0, N).  Needs the rotations of select_params."""
        buf, k = self._targets(targets)
        return self.eng._new(self.eng.lib.sfhe_sorter_select_ranked, self.h, rank.h, ct.h, buf, k)

    def select(self, ct: Ct, targets, stable: bool = False, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        """rank (stable: rank_stable, one level more) of ct, then select_ranked; always eager."""
        buf, k = self._targets(targets)
        return self.eng._new(self.eng.lib.sfhe_sorter_select, self.h, ct.h, buf, k, int(bool(stable)), n, dg, df)

    def select_many(self, rank: Ct, cts, targets) -> list:
        """select_ranked(rank, ct, targets) of every column with ONE indicator evaluation per
        batch: the same residues as the separate calls.  Payload values must lie in [-1, 1]."""
        cts = list(cts)
        buf, k = self._targets(targets)
        hs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_select_many(self.h, rank.h, hs, len(cts), buf, k, outs))
        return [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))]

    def select_records(self, keys: Ct, cts=(), targets=(0,), stable: bool = True, n: int = 3, dg: int = 2,
                       df: int = 2):
        """ORDER BY key LIMIT k over rows: (select(keys, targets), [columns' rows in the same
        order]); stable: equal keys keep their input order (one level more, as select)."""
        cts = list(cts)
        buf, k = self._targets(targets)
        hs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        outs = (_VP * max(len(cts), 1))()
        ko = C.c_void_p()
        self.eng._chk(self.eng.lib.sfhe_sorter_select_records(self.h, keys.h, hs, len(cts), buf, k,
                                                              int(bool(stable)), n, dg, df, C.byref(ko), outs))
        return Ct(self.eng, ko), [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))]

    def top_k_records(self, keys: Ct, cts, k: int, largest: bool = False, **kw):
        """The rows of the k smallest keys in ascending key order (largest: the k largest, descending)."""
        return self.select_records(keys, cts, [self.N - 1 - i for i in range(k)] if largest else list(range(k)),
                                   **kw)

    # -- ORDER BY several keys --
    @staticmethod
    def _lex(keys, descending):
        keys = list(keys)
        desc = [False] * len(keys) if descending is None else [bool(d) for d in descending]
        if len(desc) != len(keys):
            raise SfheError("sfhe error -1: one descending flag per key is needed")
        hs = (_VP * max(len(keys), 1))(*[k.h if k is not None else None for k in keys])
        return keys, hs, (C.c_int * max(len(keys), 1))(*[int(d) for d in desc])

    def rank_lex(self, keys, descending=None, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        """The rank of every row in (keys[0], keys[1], ..., input index) order, key i descending
        where descending[i]; 1 .. LEX_KEYS keys at one level.  len(keys) - 1 levels below
        rank_stable; with one ascending key exactly its residues."""
        keys, hs, ds = self._lex(keys, descending)
        return self.eng._new(self.eng.lib.sfhe_sorter_rank_lex, self.h, hs, len(keys), ds, n, dg, df)

    def sort_records_lex(self, keys, cts=(), descending=None, n: int = 3, dg: int = 2, df: int = 2):
        """ORDER BY keys[0], keys[1], ... over rows: ([sorted key columns], [payload columns in
        that order]); rows equal on every key keep their input order.  The context needs
        lex_sort_depth(N, (n, dg, df), len(keys)) levels (SfheError otherwise)."""
        keys, hs, ds = self._lex(keys, descending)
        cts = list(cts)
        cs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        kouts = (_VP * max(len(keys), 1))()
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_sort_records_lex(self.h, hs, len(keys), ds, cs, len(cts), n, dg, df,
                                                                kouts, outs))
        return ([Ct(self.eng, C.c_void_p(kouts[i])) for i in range(len(keys))],
                [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))])

    def select_records_lex(self, keys, cts=(), targets=(0,), descending=None, n: int = 3, dg: int = 2, df: int = 2):
        """ORDER BY keys ... LIMIT: the rows whose lexicographic ranks are `targets`, as
        ([key columns' rows], [payload columns' rows]).  Needs the rotations of select_params."""
        keys, hs, ds = self._lex(keys, descending)
        cts = list(cts)
        buf, k = self._targets(targets)
        cs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        kouts = (_VP * max(len(keys), 1))()
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_select_records_lex(self.h, hs, len(keys), ds, cs, len(cts), buf, k,
                                                                  n, dg, df, kouts, outs))
        return ([Ct(self.eng, C.c_void_p(kouts[i])) for i in range(len(keys))],
                [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))])

    def top_k_records_lex(self, keys, cts, k: int, descending=None, **kw):
        """The first k rows in (keys, input index) order."""
        return self.select_records_lex(keys, cts, list(range(k)), descending, **kw)

    # -- GROUP BY key --
    def group(self, keys: Ct, cts=(), index: bool = False, n: int = 3, dg: int = 2, df: int = 2):
        """COUNT(*), SUM(col) and ROW_NUMBER() over the rows sharing a key, in input order:
        {"count": slot r = rows with row r's key, "index": slot r = rows before r with its key
        (None unless index=True), "sums": [slot r = column's sum over the rows with r's key]}.
        The context needs group_params' depth for the sign configuration (SfheError otherwise);
        no placement is evaluated."""
        cts = list(cts)
        cs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        cnt, idx = _VP(), _VP()
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_group(self.h, keys.h, cs, len(cts), int(bool(index)), n, dg, df,
                                                     C.byref(cnt), C.byref(idx), outs))
        return {"count": Ct(self.eng, cnt), "index": Ct(self.eng, idx) if index else None,
                "sums": [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))]}

    # -- aggregates OVER (ORDER BY key) --
    def window(self, keys: Ct, cts=(), frame: str = "rows", count: bool = False, n: int = 3, dg: int = 2,
               df: int = 2):
        """SUM(col) OVER (ORDER BY key) and the counts that go with it, in input order:
        {"count": slot r = rows in row r's frame (None unless count=True), "sums": [slot r =
        column's sum over row r's frame]}.  Row j is in row r's frame where (key_j, j) <=
        (key_r, r) ("rows": running totals in stable order; count = ROW_NUMBER()), key_j <= key_r
        ("range": SQL's default frame; count = N * CUME_DIST()) or key_j < key_r ("below"; count =
        RANK() - 1).  The context needs window_params' depth for the sign configuration
        (SfheError otherwise); no placement is evaluated.  Payload values lie in [-1, 1]."""
        if frame not in FRAMES:
            raise SfheError(f"sfhe error -1: unknown frame {frame!r} (one of {', '.join(FRAMES)})")
        cts = list(cts)
        cs = (_VP * max(len(cts), 1))(*[c.h if c is not None else None for c in cts])
        cnt = _VP()
        outs = (_VP * max(len(cts), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_window(self.h, keys.h, cs, len(cts), FRAMES[frame], int(bool(count)),
                                                      n, dg, df, C.byref(cnt), outs))
        return {"count": Ct(self.eng, cnt) if count else None,
                "sums": [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cts))]}

    # -- a LEFT JOIN b ON a.k1 = b.k1 [AND ...] --
    def join(self, keys_a, keys_b, cols_b=(), n: int = 3, dg: int = 2, df: int = 2):
        """COUNT(b.*) and SUM(b.col) of table A LEFT JOIN table B on 1 to 4 keys, in A's input
        order: {"count": slot r = rows of B agreeing with A's row r on every key, "sums": [slot r
        = the column of B summed over those rows]}.  With unique B keys the count is the 0/1
        semi-join flag (1 - count the anti-join flag) and a sum is the looked-up value; a table
        joined with itself is GROUP BY k1, ..., km.  Per key, an A value and a B value are equal
        or at least the sign's resolution apart; both tables occupy N rows.  The context needs
        join_params' depth for the sign configuration (SfheError otherwise); no placement is
        evaluated."""
        keys_a, keys_b, cols_b = list(keys_a), list(keys_b), list(cols_b)
        if len(keys_a) != len(keys_b):
            raise SfheError(f"sfhe error -1: {len(keys_a)} keys of table A against {len(keys_b)} of table B")
        ka = (_VP * max(len(keys_a), 1))(*[k.h if k is not None else None for k in keys_a])
        kb = (_VP * max(len(keys_b), 1))(*[k.h if k is not None else None for k in keys_b])
        cs = (_VP * max(len(cols_b), 1))(*[c.h if c is not None else None for c in cols_b])
        cnt = _VP()
        outs = (_VP * max(len(cols_b), 1))()
        self.eng._chk(self.eng.lib.sfhe_sorter_join(self.h, ka, kb, len(keys_a), cs, len(cols_b), n, dg, df,
                                                    C.byref(cnt), outs))
        return {"count": Ct(self.eng, cnt), "sums": [Ct(self.eng, C.c_void_p(outs[i])) for i in range(len(cols_b))]}

    def top_k(self, ct: Ct, k: int, largest: bool = False, **kw) -> Ct:
        """The k smallest values in ascending order (largest: the k largest, descending)."""
        return self.select(ct, [self.N - 1 - i for i in range(k)] if largest else list(range(k)), **kw)

    def kth(self, ct: Ct, t: int, **kw) -> Ct:
        """The element of rank t (0 = the minimum, N - 1 = the maximum, N // 2 = the upper median) in slot 0."""
        return self.select(ct, [t], **kw)

    def records_graph_nodes(self) -> int:
        v = C.c_uint64()
        self.eng._chk(self.eng.lib.sfhe_sorter_records_graph_nodes(self.h, C.byref(v)))
        return v.value

    def sort_hybrid1(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2) -> Ct:
        """DirectSort<N>::sort_hybrid1 (reference sort_algo.h:1213-1229)."""
        return self.eng._new(self.eng.lib.sfhe_sorter_sort_hybrid1, self.h, ct.h, n, dg, df)

    def sort_hybrid(self, ct: Ct, n: int = 3, dg: int = 2, df: int = 2, variant: int = 0) -> Ct:
        """DirectSort<N>::sort_hybrid (variant 0, reference sort_algo.h:1049-1062) or
        sort_hybrid2 (variant 2, :1376-1389)."""
        return self.eng._new(self.eng.lib.sfhe_sorter_sort_hybrid, self.h, ct.h, variant, n, dg, df)

    def place_2n(self, rank: Ct, ct: Ct) -> Ct:
        """DirectSort<N>::rotationIndexCheck2N (reference sort_algo.h:587-656)."""
        return self.eng._new(self.eng.lib.sfhe_sorter_place_2n, self.h, rank.h, ct.h)

    def sort_bitonic(self, ct: Ct, n: int = 4, dg: int = 3, df: int = 3) -> Ct:
        """BitonicSort<N>::sort (reference sort_algo.h:1421-1486); values in [0, 255]."""
        return self.eng._new(self.eng.lib.sfhe_sorter_sort_bitonic, self.h, ct.h, n, dg, df)

    def graph_ntt_time(self, reps: int = 5):
        """(ms per sort, launches, algorithmic bytes) of the captured sort's
        NTT kernels replayed alone (sfhe_sorter_graph_ntt_time)."""
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        self.eng._chk(self.eng.lib.sfhe_sorter_graph_ntt_time(self.h, reps, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def graph_family_time(self, family: str, reps: int = 3):
        """(ms per sort, launches, NTT algorithmic bytes) of the captured
        sort's kernels of one family (KFAM names, "other" or "all") replayed
        alone (sfhe_sorter_graph_family_time)."""
        f = {**self.eng.KFAM, "other": 4, "all": 5}[family]
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        self.eng._chk(self.eng.lib.sfhe_sorter_graph_family_time(self.h, f, reps, C.byref(ms), C.byref(n),
                                                                 C.byref(b)))
        return ms.value, n.value, b.value

    def graph_nodes(self) -> int:
        v = C.c_uint64()
        self.eng._chk(self.eng.lib.sfhe_sorter_graph_nodes(self.h, C.byref(v)))
        return v.value


def direct_sort_params(N: int, backend: str = "hip"):
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_direct_sort_params(N, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_direct_sort_params(N, None, buf, cnt.value, None)
    return depth.value, list(buf)


def select_params(N: int, backend: str = "hip"):
    """(depth, rotations) for Sorter.select: direct_sort_params united with the radix-4 fold
    amounts {s, 2s, 3s : s = 4^i < N}."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_select_params(N, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_select_params(N, None, buf, cnt.value, None)
    return depth.value, list(buf)


def group_params(N: int, backend: str = "hip"):
    """(depth, rotations) for Sorter.group with N's default sign configuration: the stable
    rank's depth (no placement) and the rank's rotation amounts."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_group_params(N, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_group_params(N, None, buf, cnt.value, None)
    return depth.value, list(buf)


def join_params(N: int, nkeys: int = 1, backend: str = "hip"):
    """(depth, rotations) for Sorter.join on nkeys keys with N's default sign configuration:
    group_params' depth plus ceil(log2 nkeys), and the rank's rotation amounts."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_join_params(N, nkeys, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_join_params(N, nkeys, None, buf, cnt.value, None)
    return depth.value, list(buf)


def window_params(N: int, backend: str = "hip"):
    """(depth, rotations) for Sorter.window with N's default sign configuration: the stable
    rank's depth plus one (no placement) and the rank's rotation amounts."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_window_params(N, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_window_params(N, None, buf, cnt.value, None)
    return depth.value, list(buf)


def lex_sort_depth(N: int, cfg=None, m: int = 2, backend: str = "hip") -> int:
    """mult_depth of Sorter.sort_records_lex by m keys with sign configuration cfg = (n, dg, df)
    (None: (3, 2, 2), the methods' default): the stable sort's depth + m - 1."""
    lib = load(backend)
    n, dg, df = (3, 2, 2) if cfg is None else cfg
    depth = C.c_uint32()
    if lib.sfhe_lex_sort_depth(N, int(n), int(dg), int(df), int(m), C.byref(depth)) != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    return depth.value


class KWay:
    def __init__(self, eng: "Engine", h):
        self.eng, self.h = eng, h

    def __del__(self):
        try:
            if self.h:
                self.eng.lib.sfhe_kway_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def sort(self, ct: "Ct", n: int = 3, dg: int = 2, df: int = 2, mult_depth: int = 40) -> "Ct":
        return self.eng._new(self.eng.lib.sfhe_kway_run, self.h, ct.h, n, dg, df, mult_depth)

    def graph_nodes(self) -> int:
        """Nodes of the captured sort graph (0: none yet / eager)."""
        v = C.c_uint64()
        self.eng._chk(self.eng.lib.sfhe_kway_graph_nodes(self.h, C.byref(v)))
        return v.value

    def graph_family_time(self, family: str, reps: int = 1):
        """(ms per sort, launches, algorithmic bytes) of the captured sort's
        kernels of one family replayed alone, over its chain of graphs."""
        f = {**self.eng.KFAM, "other": 4, "all": 5}[family]
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        self.eng._chk(self.eng.lib.sfhe_kway_graph_family_time(self.h, f, reps, C.byref(ms), C.byref(n),
                                                               C.byref(b)))
        return ms.value, n.value, b.value


def kway_params(N: int, backend: str = "hip"):
    """KWayAdapter<N>::getSizeParameters: (batch, depth, level budget, rotations)."""
    lib = load(backend)
    b, d, b0, b1, cnt = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    rc = lib.sfhe_kway_params(N, C.byref(b), C.byref(d), C.byref(b0), C.byref(b1), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(f"sfhe error {rc}: {lib.sfhe_last_error().decode()}")
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_kway_params(N, None, None, None, None, buf, cnt.value, None)
    return b.value, d.value, (b0.value, b1.value), list(buf)


def hybrid_params(N: int, variant: int = 0, backend: str = "hip"):
    """(depth, rotation keys) of tests/DirectSortHTest.cpp (variant 0) or
    tests/DirectSortH2Test.cpp (variant 2) for N."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_hybrid_params(N, variant, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(f"sfhe error {rc}: {lib.sfhe_last_error().decode()}")
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_hybrid_params(N, variant, None, buf, cnt.value, None)
    return depth.value, list(buf)


def hybrid1_params(N: int, backend: str = "hip"):
    """(depth, rotation keys) of tests/DirectSortH1Test.cpp:36-117 for N."""
    lib = load(backend)
    depth = C.c_uint32()
    cnt = C.c_size_t()
    rc = lib.sfhe_hybrid1_params(N, C.byref(depth), None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_int32 * cnt.value)()
    lib.sfhe_hybrid1_params(N, None, buf, cnt.value, None)
    return depth.value, list(buf)


def doubled_sinc_coeffs(N: int, backend: str = "hip"):
    lib = load(backend)
    cnt = C.c_size_t()
    rc = lib.sfhe_doubled_sinc_coeffs(N, None, 0, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    buf = (C.c_double * cnt.value)()
    lib.sfhe_doubled_sinc_coeffs(N, buf, cnt.value, None)
    return list(buf)


def decompose(N: int, keys: Sequence[int], rotation: int, wrapN: int, algo: int, backend: str = "hip"):
    lib = load(backend)
    k = (C.c_int32 * len(keys))(*keys)
    cap = 64
    v = (C.c_int32 * cap)()
    s = (C.c_int32 * cap)()
    cnt = C.c_size_t()
    rc = lib.sfhe_decompose(N, k, len(keys), rotation, wrapN, algo, v, s, cap, C.byref(cnt))
    if rc == SFHE_OK and cnt.value > cap:  # long chains: ask again with room for all of them
        cap = cnt.value
        v, s = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        rc = lib.sfhe_decompose(N, k, len(keys), rotation, wrapN, algo, v, s, cap, C.byref(cnt))
    if rc != SFHE_OK:
        raise SfheError(lib.sfhe_last_error().decode())
    return [(v[i], s[i]) for i in range(min(cnt.value, cap))]


# ---- limb-sharding transports ------------------------------------------------

def live_contexts(backend: str = "hip") -> int:
    """Engine contexts alive in this process (sfhe_live_contexts)."""
    return load(backend).sfhe_live_contexts()


def comm_uid(backend: str = "hip"):
    """128-byte RCCL unique id (bytes), or None where the backend has no RCCL."""
    lib = load(backend)
    buf = (C.c_uint8 * 128)()
    if lib.sfhe_comm_uid(buf) != SFHE_OK:
        return None
    return bytes(buf)


class ThreadComm:
    """Host collectives between `world` threads of one process (each thread
    one rank; tests).  Callbacks run with the GIL held; the library calls
    them with the GIL released, so the ranks' device work overlaps."""

    def __init__(self, world: int, timeout: float = 600.0):
        import threading
        self.world = world
        self.bar = threading.Barrier(world, timeout=timeout)
        self.slots = [b""] * world

    def allgather(self, rank, send, recv, nbytes):
        self.slots[rank] = C.string_at(send, nbytes) if nbytes else b""
        self.bar.wait()
        for r in range(self.world):
            if nbytes:
                C.memmove(recv + r * nbytes, self.slots[r], nbytes)
        self.bar.wait()

    def bcast(self, rank, buf, nbytes, root):
        if rank == root:
            self.slots[root] = C.string_at(buf, nbytes) if nbytes else b""
        self.bar.wait()
        if rank != root and nbytes:
            C.memmove(buf, self.slots[root], nbytes)
        self.bar.wait()


class GlooComm:
    """Host collectives over an initialised torch.distributed process group
    (gloo: CPU tensors; one process per rank)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)

    def allgather(self, rank, send, recv, nbytes):
        import torch
        t = torch.frombuffer(bytearray(C.string_at(send, nbytes)), dtype=torch.uint8)
        outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(self.world)]
        self.dist.all_gather(outs, t, group=self.group)
        for r, o in enumerate(outs):
            C.memmove(recv + r * nbytes, o.numpy().ctypes.data, nbytes)

    def bcast(self, rank, buf, nbytes, root):
        import torch
        t = torch.frombuffer(bytearray(C.string_at(buf, nbytes)), dtype=torch.uint8)
        # root is a rank of this communicator; torch wants the global rank
        src = root if self.group is None else self.dist.get_global_rank(self.group, root)
        self.dist.broadcast(t, src=src, group=self.group)
        if rank != root:
            C.memmove(buf, t.numpy().ctypes.data, nbytes)


def run_split_threads(backend: str, world: int, groups: int, fn, **engine_kw):
    """Run fn(engine) on `world` thread ranks split into `groups` batch groups
    of world // groups ranks (rank = group * (world // groups) + r); each
    group limb-sharded over its own ThreadComm when it has more than one
    rank.  Returns the per-rank results (rank order)."""
    import threading
    per = world // groups
    if per * groups != world:
        raise ValueError("world must be a multiple of groups")
    limb = [ThreadComm(per) for _ in range(groups)]
    grp = [ThreadComm(groups) for _ in range(per)]
    outs, errs = [None] * world, []

    def body(rank):
        g, r = divmod(rank, per)
        try:
            shard = ("host", r, per, limb[g]) if per > 1 else None
            e = Engine(backend, shard=shard, groups=("host", g, groups, grp[r]), **engine_kw)
            outs[rank] = fn(e)
        except BaseException as ex:  # unblock the other ranks
            errs.append(ex)
            for c in limb + grp:
                c.bar.abort()

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return outs


def run_sharded_threads(backend: str, world: int, fn, **engine_kw):
    """Run fn(engine) on `world` limb-sharded engines, one thread per rank,
    over ThreadComm; returns the per-rank results (rank order)."""
    import threading
    comm = ThreadComm(world)
    outs, errs = [None] * world, []

    def body(r):
        try:
            e = Engine(backend, shard=("host", r, world, comm), **engine_kw)
            outs[r] = fn(e)
        except BaseException as ex:  # unblock the other ranks
            errs.append(ex)
            comm.bar.abort()

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return outs
