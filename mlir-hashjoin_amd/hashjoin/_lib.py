"""ctypes binding of libhj.so (include/hj.h).

The HIP extension is the product: there is no CPU fallback.  If libhj.so is
missing this module raises at import time, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("HJ_LIB", os.path.join(PKG_ROOT, "lib", "libhj.so"))
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "hj.h")

HJ_OK = 0
HJ_ERR_ARG = -1
HJ_ERR_HIP = -2
HJ_ERR_NOMEM = -3
HJ_ERR_STATE = -4
HJ_ERR_CAPACITY = -5
HJ_ERR_RANGE = -6

HJ_STRATEGY_AUTO = 0
HJ_STRATEGY_GLOBAL = 1
HJ_STRATEGY_RADIX = 2

HJ_EXISTS_SEMI = 0
HJ_EXISTS_ANTI = 1
HJ_JOIN_KERNEL_EXISTS = 6
HJ_JOIN_KERNEL_LOOKUP = 7
HJ_JOIN_KERNEL_GROUP = 8
HJ_JOIN_KERNEL_AGGREGATE = 9
HJ_JOIN_KERNEL_EXPAND = 10
HJ_JOIN_KERNEL_ASOF = 11
HJ_EXPAND_INNER = 0
HJ_EXPAND_OUTER = 1
HJ_ASOF_BACKWARD = 0
HJ_ASOF_FORWARD = 1
HJ_ASOF_STRICT = 2
# the expand probe's scan (hj_kernels.hip: kExpandTile counts per tile, kExpandFan tile sums per step of
# the one workgroup that scans them) -- the sizes at which its paths change, for the tests
EXPAND_SCAN_TILE = 2048
EXPAND_SCAN_FAN = 1024
# composite keys (hj_keys.hip: kKeysBlock threads walk kKeysTile rows per loop step over a grid capped at
# kKeysGridPerCu workgroups per CU) -- the sizes at which the observe / pack / unpack loops wrap, for the tests
HJ_KEYS_MAX_COLS = 4
KEYS_BLOCK = 256
KEYS_TILE = 2048
KEYS_GRID_PER_CU = 8
# the key filter (hj_filter.hip: kFilterBlock threads walk kFilterTile rows per loop step over a grid capped at
# kFilterGridPerCu workgroups per CU) -- the sizes at which the insert / apply loops wrap, for the tests
HJ_FILTER_PASS = 0
HJ_FILTER_REJECT = 1
FILTER_BLOCK = 256
FILTER_TILE = 2048
FILTER_GRID_PER_CU = 8
# the star probe (hj_kernels.hip, k_star: 2048-row tiles; a table of <= STAR_LDS_TABLE_BYTES is probed from LDS while
# the LDS-resident tables together stay <= STAR_LDS_BUDGET_BYTES)
HJ_STAR_MAX_DIMS = 4
HJ_STAR_INNER = 0
HJ_STAR_LEFT = 1
HJ_STAR_ANTI = 2
STAR_TILE = 2048
STAR_LDS_TABLE_BYTES = 64 * 1024
STAR_LDS_BUDGET_BYTES = 128 * 1024
# the star aggregate (k_star_agg): the group table's smallest capacity (hj_star_reserve_groups)
STAR_GROUP_MIN_CAPACITY = 2048
HJ_GROUP_MATCHED = 0
HJ_GROUP_ALL = 1
HJ_OUTER_BUILD = 1
HJ_OUTER_FULL = 2

_vp = C.c_void_p
_i64 = C.c_int64
_u64 = C.c_uint64
_int = C.c_int

# the star query (hj.h "Star query"): the fact side of a call
HJ_STAR_MAX_PREDS = 4
HJ_STAR_MAX_FACT_GROUPS = 2
HJ_PRED_IN = 0
HJ_PRED_OUT = 1
HJ_VALUE_A = 0
HJ_VALUE_ADD = 1
HJ_VALUE_SUB = 2
HJ_VALUE_MUL = 3


class StarFact(C.Structure):
    """hj_star_fact: a host struct read at call time."""
    _fields_ = [("npreds", _int), ("pcol", _vp * HJ_STAR_MAX_PREDS), ("plo", _i64 * HJ_STAR_MAX_PREDS),
                ("phi", _i64 * HJ_STAR_MAX_PREDS), ("pkind", _int * HJ_STAR_MAX_PREDS), ("vop", _int), ("vb", _vp),
                ("nfact", _int), ("fcol", _vp * HJ_STAR_MAX_FACT_GROUPS), ("fshift", _int * HJ_STAR_MAX_FACT_GROUPS),
                ("fbase", _i64 * HJ_STAR_MAX_FACT_GROUPS)]


def _load():
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so
    # (SONAME libamdhip64.so.7) and loads it by path.  Importing torch first
    # makes libhj.so's NEEDED libamdhip64.so.7 bind to that same instance
    # (matched by SONAME); loading libhj.so first would map /opt/rocm's copy
    # too, and two HSA runtimes in one process cannot share the device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libhj.so not found at {LIB_PATH}: build it with `make -C mlir-hashjoin_amd` "
            "(or __graft_entry__.build()); the hash join has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    sig = {
        "hj_abi_version": (_int, []),
        "hj_last_error": (C.c_char_p, []),
        "hj_device_info": (_int, [_int, C.POINTER(_i64)]),
        "hj_host_memo_hits": (_i64, []),
        "hj_host_set_reuse": (_int, [_int]),
        "hj_ctx_create": (_vp, [_int]),
        "hj_ctx_destroy": (None, [_vp]),
        "hj_ctx_reserve": (_int, [_vp, _i64, _int]),
        "hj_ctx_table_capacity": (_i64, [_vp]),
        "hj_ctx_radix_plan": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "hj_ctx_build_has_duplicates": (_int, [_vp]),
        "hj_ctx_join_kernel": (_int, [_vp]),
        "hj_ctx_set_timing": (_int, [_vp, _int]),
        "hj_ctx_last_timing": (_int, [_vp, C.POINTER(C.c_float)]),
        "hj_ctx_last_timing_ex": (_int, [_vp, C.POINTER(C.c_float)]),
        "hj_ctx_timing_accumulate": (_int, [_vp, _int]),
        "hj_ctx_timing_totals": (_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
        "hj_ctx_reserve_probe": (_int, [_vp, _i64, _int]),
        "hj_ctx_probe_hint": (_int, [_vp, _i64]),
        "hj_ctx_set_strategy": (_int, [_vp, _int]),
        "hj_ctx_strategy_used": (_int, [_vp]),
        "hj_ctx_set_radix_bits": (_int, [_vp, _int]),
        "hj_dev_build_i64": (_int, [_vp, _vp, _vp, _i64, _vp]),
        "hj_dev_count_i64": (_int, [_vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_i64": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_build_tuples_i64": (_int, [_vp, _vp, _i64, _vp]),
        "hj_dev_probe_tuples_i64": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_build_i32": (_int, [_vp, _vp, _i64, _i64, _vp]),
        "hj_dev_count_i32": (_int, [_vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_i32": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_exists_i64": (_int, [_vp, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_exists_tuples_i64": (_int, [_vp, _int, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_exists_i32": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_lookup_i64": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
        "hj_dev_lookup_i32": (_int, [_vp, _vp, _i64, C.c_int32, _vp, _vp, _vp, _vp]),
        "hj_dev_asof_i64": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
        "hj_dev_asof_i32": (_int, [_vp, _int, _vp, _vp, _i64, C.c_int32, _vp, _vp, _vp]),
        "hj_dev_expand_i64": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_expand_i32": (_int, [_vp, _int, _vp, _i64, C.c_int32, _vp, _vp, _i64, _vp, _vp]),
        "hj_ctx_reserve_expand": (_int, [_vp, _i64, _int]),
        "hj_dev_group_i64": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_group_tuples_i64": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_group_i32": (_int, [_vp, _int, _vp, _i64, _i64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_ctx_reserve_group": (_int, [_vp, _i64, _int]),
        "hj_dev_aggregate_i64": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_aggregate_tuples_i64": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_aggregate_i32": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_ctx_reserve_aggregate": (_int, [_vp, _i64, _int]),
        "hj_dev_probe_outer_i64": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_outer_tuples_i64": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_outer_i32": (_int, [_vp, _vp, _i64, _i64, C.c_int32, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_full_i64": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_full_tuples_i64": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_probe_full_i32": (_int, [_vp, _int, _vp, _i64, _i64, C.c_int32, C.c_int32, _vp, _vp, _i64, _vp,
                                         _vp]),
        "hj_keycodec_create": (_vp, [_int, _int, C.POINTER(C.c_int)]),
        "hj_keycodec_destroy": (None, [_vp]),
        "hj_dev_keycodec_reset": (_int, [_vp, _vp]),
        "hj_dev_keycodec_observe": (_int, [_vp, C.POINTER(_vp), _i64, _vp]),
        "hj_dev_keycodec_seal": (_int, [_vp, _vp]),
        "hj_dev_keycodec_pack": (_int, [_vp, C.POINTER(_vp), _i64, _vp, _vp]),
        "hj_dev_keycodec_pack_tuples": (_int, [_vp, C.POINTER(_vp), _vp, _i64, _vp, _vp]),
        "hj_dev_keycodec_unpack": (_int, [_vp, _vp, _i64, C.POINTER(_vp), _vp]),
        "hj_keycodec_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_i64),
                                    C.POINTER(_u64), C.POINTER(_u64)]),
        "hj_filter_blocks_for": (_i64, [_i64, _int]),
        "hj_filter_place": (_int, [_i64, _i64, C.POINTER(_i64), C.POINTER(C.c_uint32)]),
        "hj_filter_create": (_vp, [_int, _i64, _vp]),
        "hj_filter_destroy": (None, [_vp]),
        "hj_filter_words": (_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
        "hj_filter_reserve": (_int, [_vp, _i64]),
        "hj_dev_filter_clear": (_int, [_vp, _vp]),
        "hj_dev_filter_insert_i64": (_int, [_vp, _vp, _i64, _vp]),
        "hj_dev_filter_insert_tuples_i64": (_int, [_vp, _vp, _i64, _vp]),
        "hj_dev_filter_insert_i32": (_int, [_vp, _vp, _i64, _vp]),
        "hj_dev_filter_merge": (_int, [_vp, _vp, _vp]),
        "hj_dev_filter_apply_i64": (_int, [_vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_filter_apply_tuples_i64": (_int, [_vp, _int, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_filter_apply_i32": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_star_create": (_vp, [_int]),
        "hj_star_destroy": (None, [_vp]),
        "hj_star_reserve": (_int, [_vp, _i64]),
        "hj_star_last_plan": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_int),
                                     C.POINTER(_i64)]),
        "hj_dev_star_i64": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp), C.POINTER(_i64), _i64,
                                   C.POINTER(_vp), _vp, _i64, _vp, _vp]),
        "hj_dev_star_i32": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp), C.POINTER(C.c_int32),
                                   _i64, _i64, C.POINTER(_vp), _vp, _i64, _vp, _vp]),
        "hj_star_reserve_groups": (_int, [_vp, _i64]),
        "hj_star_group_capacity": (_i64, [_vp]),
        "hj_dev_star_aggregate_i64": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp),
                                             C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(_i64), _vp, _i64, _vp, _vp,
                                             _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_star_aggregate_i32": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(_i64), _vp, _i64, _vp,
                                             _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_star_query_i64": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp),
                                         C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(StarFact), _vp,
                                         _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_star_query_i32": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_vp),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(StarFact),
                                         _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_partition_i64": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp, _vp]),
        "hj_dev_partition_tuples_i64": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
        "hj_partition_of": (_int, [_i64, _int]),
        "hj_route_plan": (_int, [_i64, _int, C.POINTER(C.c_int)]),
        "hj_dev_route_i64": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp]),
        "hj_dev_build_routed_i64": (_int, [_vp, _vp, _i64, _vp, _int, _int, _int, _vp]),
        "hj_dev_probe_routed_i64": (_int, [_vp, _vp, _i64, _vp, _int, _int, _int, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_gen_pkfk_i64": (_int, [_u64, _i64, _u64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
        "hj_zipf_params": (_int, [_i64, C.c_double, C.POINTER(C.c_double)]),
        "hj_dev_gen_zipf_i64": (_int, [_u64, _i64, C.c_double, _i64, _i64, _vp, _vp, _vp]),
        "hj_dev_gen_uniform_i64": (_int, [_u64, _u64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
        "hj_dev_gen_uniform_i32": (_int, [_u64, _u64, C.c_int32, C.c_int32, _i64, _i64, _vp, _vp]),
        "hj_count_i32": (_i64, [_vp, _vp, _i64, _i64, _i64] * 2),
        "hj_probe_i32": (C.c_int32, [_vp, _vp, _i64, _i64, _i64] * 4),
        "hj_count_i64": (_i64, [_vp, _vp, _i64, _i64, _i64] * 4),
        "hj_probe_i64": (C.c_int32, [_vp, _vp, _i64, _i64, _i64] * 6),
        "hj_dev_count_rows_i32": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp]),
        "hj_dev_join_rows_i32": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp,
                                        _vp]),
        "hj_count_rows_i32": (_i64, [_vp, _vp, _i64, _i64, _i64, _i64, _i64] * 2),
        "hj_join_rows_i32": (_i64, [_vp, _vp, _i64, _i64, _i64, _i64, _i64] * 3),
        "_mlir_ciface_hj_join_rows_i32": (None, [_vp, _vp, _vp]),
        "hj_host_join_ooc_i64": (_i64, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _u64]),
        "hj_dev_select_f32": (_int, [_vp, _vp, _i64, _int, C.c_float, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_select_i64": (_int, [_vp, _vp, _i64, _int, _i64, _vp, _vp, _i64, _vp, _vp]),
        "hj_dev_stream_copy": (_int, [_vp, _vp, _i64, _int, _vp]),
        "hj_placement_stats": (None, [_vp, _vp, _vp, _vp]),
        "hj_placement_stats_ex": (None, [_vp, _vp, _vp]),
        "hj_placement_set_good": (C.c_double, [C.c_double]),
        "hj_placement_check": (_int, [_vp, _i64, _vp]),
        "hj_select_f32": (_i64, [_vp, _vp, _i64, _i64, _i64, C.c_float, _vp, _vp, _i64, _i64, _i64]),
        "_mlir_ciface_hj_join_i32": (None, [_vp, _vp, _vp]),
        "_mlir_ciface_hj_join_i64": (None, [_vp, _vp, _vp]),
        "_mlir_ciface_hj_join_kp_i64": (None, [_vp, _vp, _vp, _vp, _vp]),
        "hj_free_result": (None, [_vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L


lib = _load()


class HJError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != HJ_OK:
        msg = lib.hj_last_error().decode(errors="replace")
        raise HJError(f"{what} failed with {rc}: {msg}")
    return rc


def declared_symbols():
    """Every function name include/hj.h declares (for the ABI export test)."""
    import re
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^[A-Za-z_][\w \*]*?\b(\w+)\s*\(", text, flags=re.M)
    return sorted({n for n in names if n.startswith(("hj_", "_mlir_ciface_hj_"))})


def memref_struct(ctype, rank):
    class _M(C.Structure):
        _fields_ = [("allocated", C.POINTER(ctype)), ("aligned", C.POINTER(ctype)), ("offset", _i64),
                    ("sizes", _i64 * rank), ("strides", _i64 * rank)]
    return _M


MemRef1I32 = memref_struct(C.c_int32, 1)
MemRef1I64 = memref_struct(C.c_int64, 1)
MemRef2I32 = memref_struct(C.c_int32, 2)
MemRef2I64 = memref_struct(C.c_int64, 2)
