"""ctypes binding of ``libqs_amd.so`` (C ABI: ``include/qs_amd.h``).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc,
``--offload-arch=gfx950``).  There is no fallback: if the shared object is
missing or does not export a symbol the header declares, importing the compute
layer raises -- the transforms never silently run anywhere else.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# QS_AMD_LIB: development hook -- another build of the SAME library (kernel A/B runs inside one gpurun call)
LIB_PATH = os.environ.get("QS_AMD_LIB") or os.path.join(_HERE, "libqs_amd.so")

QS_F64 = 0
QS_C128 = 1

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_ptr = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/qs_amd.h line by line
SIGNATURES = {
    "qs_abi_version": (c_int, []),
    "qs_error_string": (ctypes.c_char_p, [c_int]),
    "qs_last_hip_error": (ctypes.c_char_p, []),
    "qs_matmul": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 10 + [c_int, c_ptr]),
    "qs_matmul_pairs": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 10 + [c_int, c_ptr]),
    "qs_matmul_pairs_mirrored": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 10 + [c_int, c_ptr]),
    "qs_matmul_pairs_lower": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 10 + [c_int, c_ptr]),
    "qs_matmul_upper": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 11 + [c_int, c_ptr]),
    "qs_triangle_pair": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "qs_transform_two_body_workspace": (c_i64, [c_int, c_i64, c_i64]),
    "qs_transform_two_body": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_mixed": (
        c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_inplace_workspace": (c_i64, [c_int, c_i64, c_i64]),
    "qs_transform_two_body_inplace": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_two_body_exchange_symmetric": (c_int, [c_int, c_ptr, c_i64, c_ptr, c_ptr]),
    "qs_transform_two_body_exchange": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_inplace_exchange": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_exchange_wanted": (c_int, [c_int, c_i64, c_i64]),
    "qs_exchange_mirror": (c_int, [c_int, c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_exchange_leading_pairs": (c_int, [c_int, c_i64, c_i64]),
    "qs_transform_two_body_exchange_leading_upper": (c_int, [c_int, c_i64, c_i64]),
    "qs_transform_two_body_exchange_lower_d": (c_int, [c_int, c_i64, c_i64]),
    "qs_exchange_mirror_lower": (c_int, [c_int, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_exchange_pair_transpose": (c_int, [c_int, c_ptr, c_ptr, c_i64, c_ptr]),
    "qs_exchange_pair_transpose_back": (c_int, [c_int, c_ptr, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_transform_two_body_partial_workspace": (c_i64, [c_int, c_i64, c_i64, c_i64]),
    "qs_transform_two_body_partial": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr]),
    "qs_transform_one_body": (
        c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr]),
    "qs_antisymmetrize": (c_int, [c_int, c_ptr, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_spin_expand_two_body": (
        c_int, [c_int, c_int, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr]),
    "qs_spin_expand_two_body_block": (
        c_int, [c_int, c_int, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr]),
    "qs_add_spin_one_body": (c_int, [c_int, c_int, c_ptr, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_spin_squared_two_body": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr]),
    "qs_tdho_coulomb_elements": (c_int, [c_ptr, c_i64, c_i64, c_i64, c_ptr]),
    "qs_tdho_coulomb_elements_nm": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr]),
    "qs_comm_unique_id": (c_int, [c_ptr]),
    "qs_comm_init": (c_int, [ctypes.POINTER(c_ptr), c_int, c_int, c_ptr]),
    "qs_comm_destroy": (c_int, [c_ptr]),
    "qs_comm_abort": (c_int, [c_ptr]),
    "qs_comm_rank": (c_int, [c_ptr]),
    "qs_comm_world": (c_int, [c_ptr]),
    "qs_last_comm_error": (ctypes.c_char_p, []),
    "qs_comm_set_option": (c_int, [c_ptr, ctypes.c_char_p, c_i64]),
    "qs_transform_two_body_sharded_workspace": (c_i64, [c_int, c_i64, c_i64, c_int, c_int]),
    "qs_transform_two_body_sharded": (
        c_int, [c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr]),
    "qs_sharded_exchange_plan": (c_int, [c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64]),
    "qs_sharded_rows_default_chunk": (c_i64, [c_int, c_i64, c_i64, c_int, c_ptr]),
    "qs_transform_two_body_sharded_rows_out_bytes": (c_i64, [c_int, c_i64, c_i64, c_int, c_int]),
    "qs_transform_two_body_sharded_rows_workspace": (c_i64, [c_int, c_i64, c_i64, c_i64]),
    "qs_transform_two_body_sharded_rows": (
        c_int, [c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr]),
    "qs_comm_rows_workspace": (c_i64, [c_ptr, c_int, c_i64, c_i64, c_i64]),
    "qs_sharded_rows_exchange_plan": (c_int, [c_i64, c_i64, c_int, c_int, c_ptr, c_i64, c_ptr, c_ptr, c_i64]),
    "qs_sharded_rows_exchange_plan_coalesced": (c_int, [c_i64, c_i64, c_int, c_int, c_ptr, c_i64, c_ptr, c_ptr, c_i64]),
    "qs_last_dispatch": (ctypes.c_char_p, []),
    "qs_tuning_set": (c_int, [ctypes.c_char_p, c_i64]),
    "qs_tuning_reset": (c_int, []),
    "qs_probe_mfma_f64": (c_int, [c_ptr, c_i64, c_i64, c_ptr]),
    "qs_probe_stream_copy": (c_int, [c_ptr, c_ptr, c_i64, c_ptr]),
    "qs_mean_field_workspace": (c_i64, [c_int, c_int, c_i64, c_i64, c_i64]),
    "qs_mean_field": (
        c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, ctypes.c_double, ctypes.c_double,
                c_ptr, c_i64, c_ptr]),
    "qs_mean_field_plan": (c_int, [c_int, c_int, c_i64, c_i64, c_i64, c_ptr, c_int]),
    "qs_mean_field_batch_workspace": (c_i64, [c_int, c_int, c_i64, c_i64, c_i64, c_i64]),
    "qs_mean_field_batch": (
        c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_ptr]),
    "qs_mean_field_batch_plan": (c_int, [c_int, c_int, c_i64, c_i64, c_i64, c_i64, c_ptr, c_int]),
    "qs_lead_contract": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 6 + [c_ptr]),
    "qs_transform_two_body_blocks_workspace": (c_i64, [c_int, c_int] + [c_i64] * 5),
    "qs_transform_two_body_blocks": (
        c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr] + [c_i64] * 6 + [c_ptr]),
    "qs_pair_contract_workspace": (c_i64, [c_int, c_int, c_i64, c_i64, c_i64]),
    "qs_pair_contract": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 4 + [c_ptr, c_i64, c_ptr]),
    "qs_pair_contract_antisym_workspace": (c_i64, [c_int, c_int, c_i64, c_i64]),
    "qs_pair_contract_antisym": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr, c_i64, c_ptr]),
    "qs_pair_contract_exchange_workspace": (c_i64, [c_int, c_int, c_i64, c_i64]),
    "qs_pair_contract_exchange": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr, c_i64, c_ptr]),
    "qs_det_ci_workspace": (c_i64, [c_int, c_int] + [c_i64] * 4),
    "qs_det_ci_diagonal": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr]),
    "qs_det_ci_sigma": (c_int, [c_int, c_int] + [c_ptr] * 6 + [c_i64] * 5 + [c_ptr, c_i64, c_ptr]),
    "qs_det_ci_density1": (c_int, [c_int, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr]),
    "qs_det_ci_transition_density1": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr]),
    "qs_det_ci_density2": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr]),
    "qs_string_ci_table": (c_int, [c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr]),
    "qs_string_ci_diagonal": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr]),
    "qs_string_ci_workspace": (c_i64, [c_int, c_int] + [c_i64] * 4),
    "qs_string_ci_group": (c_i64, [c_int, c_int] + [c_i64] * 5),
    "qs_string_ci_sigma": (c_int, [c_int, c_int] + [c_ptr] * 4 + [c_i64] * 3 + [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr]),
    "qs_string_ci_sigma_plan": (c_int, [c_int, c_int] + [c_i64] * 5 + [c_ptr]),
    "qs_string_ci_sigma_rows": (c_int, [c_int, c_int] + [c_ptr] * 4 + [c_i64] * 3 + [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_string_ci_sigma_sym_plan": (c_int, [c_int, c_int] + [c_i64] * 4 + [c_ptr, c_ptr, c_i64]),
    "qs_string_ci_sigma_sym": (c_int, [c_int, c_int] + [c_ptr] * 3 + [c_i64] * 3 + [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_ptr]),
    "qs_string_ci_density1": (c_int, [c_int, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr] * 4 + [c_i64, c_ptr]),
    "qs_string_ci_density2_workspace": (c_i64, [c_int] + [c_i64] * 4),
    "qs_string_ci_density2_plan": (c_int, [c_int] + [c_i64] * 4 + [c_ptr]),
    "qs_string_ci_density2": (c_int, [c_int, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr] * 5 + [c_i64, c_i64, c_ptr]),
    "qs_string_ci_density2_spin_workspace": (c_i64, [c_int] + [c_i64] * 4),
    "qs_string_ci_density2_spin_plan": (c_int, [c_int] + [c_i64] * 4 + [c_ptr]),
    "qs_string_ci_density2_spin": (c_int, [c_int, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr] * 8 + [c_i64, c_i64, c_ptr]),
    "qs_string_ci_spin_squared": (c_int, [c_int, c_ptr, c_ptr] + [c_i64] * 5 + [c_ptr, c_i64, c_ptr, c_ptr]),
    "qs_string_ci_one_body": (c_int, [c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr] + [c_i64] * 3 + [c_ptr, c_i64, c_ptr, c_ptr]),
    "qs_string_ci_ladder_table": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "qs_string_ci_ladder": (c_int, [c_int, c_int, c_ptr, c_i64, c_i64, c_ptr] + [c_i64] * 5 + [c_ptr, c_i64, c_ptr, c_ptr]),
    "qs_cholesky_two_body_workspace": (c_i64, [c_int, c_i64, c_i64]),
    "qs_cholesky_two_body_block": (c_i64, []),
    "qs_cholesky_two_body": (
        c_int, [c_int, c_ptr, c_i64, ctypes.c_double, c_ptr, c_i64, ctypes.POINTER(c_i64), c_ptr, c_ptr,
                ctypes.POINTER(ctypes.c_double), c_ptr, c_i64, c_ptr]),
    "qs_triples_energy_tile": (c_i64, [c_int]),
    "qs_triples_energy_budget": (c_i64, [c_i64]),
    "qs_triples_energy_workspace": (c_i64, [c_int, c_i64, c_i64]),
    "qs_triples_energy": (c_int, [c_int, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_ptr]),
    "qs_triples_energy_singles_workspace": (c_i64, [c_int, c_i64, c_i64]),
    "qs_triples_energy_singles": (
        c_int, [c_int, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr,
                c_ptr, c_i64, c_ptr]),
    "qs_tdho_quadrature_nodes": (c_int, [c_i64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "qs_tdho_coulomb_quadrature_workspace": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "qs_tdho_coulomb_quadrature": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_i64, c_ptr]),
    "qs_tdho_coulomb_vectors_workspace": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "qs_tdho_coulomb_vectors_rank": (c_int, [c_ptr, c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "qs_tdho_coulomb_vectors": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_i64, c_ptr]),
}

ABI_VERSION = 4


class QsLibraryError(RuntimeError):
    """The HIP extension is missing, stale, or a call into it failed."""


_lib = None


def load():
    """Load (once) and return the ctypes handle with every prototype set."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QsLibraryError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the transform path."
        )
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:  # missing ROCm runtime, wrong arch, ...
        raise QsLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise QsLibraryError(f"{LIB_PATH} does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.qs_abi_version() != ABI_VERSION:
        raise QsLibraryError(
            f"ABI mismatch: library {lib.qs_abi_version()}, binding {ABI_VERSION}"
        )
    _lib = lib
    return lib


def check(code, what):
    """Raise on a negative status from the C ABI."""
    if code >= 0:
        return code
    lib = load()
    msg = lib.qs_error_string(int(code)).decode()
    if code == -5:
        msg += " (" + lib.qs_last_hip_error().decode() + ")"
    if code == -8:
        msg += " (" + lib.qs_last_comm_error().decode() + ")"
    if code in (-1, -3, -6, -7):
        # the same user mistakes raise AssertionError in the reference's
        # setters (basis_set.py:93,103,113); a wrong extent is a ValueError
        raise ValueError(f"{what}: {msg}")
    raise QsLibraryError(f"{what}: {msg}")
