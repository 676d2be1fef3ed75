"""ctypes binding of libromhc.so (include/romhc.h).  Thin: prototypes, error mapping, handles.

There is no CPU fallback: if the shared library is missing or no MI355X is visible the import of
the product modules fails loudly (RomLibraryError).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
from scipy.linalg import LinAlgError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libromhc.so")

ROM_OK, ROM_ERR_INVALID, ROM_ERR_HIP, ROM_ERR_NOT_SPD, ROM_ERR_COMM, ROM_ERR_NOMEM = range(6)


class RomLibraryError(RuntimeError):
    pass


_lib = None

_c_double_p = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/romhc.h declares
PROTOTYPES = {
    "rom_last_error": (C.c_char_p, []),
    "rom_version": (C.c_int, []),
    "rom_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rom_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "rom_shutdown": (C.c_int, [_vp]),
    "rom_synchronize": (C.c_int, [_vp]),
    "rom_set_workspace_limit": (C.c_int, [_vp, C.c_size_t]),
    "rom_device_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "rom_timer_start": (C.c_int, [_vp]),
    "rom_timer_stop": (C.c_int, [_vp, _c_double_p]),
    "rom_profile_enable": (C.c_int, [_vp, C.c_int]),
    "rom_profile_reset": (C.c_int, [_vp]),
    "rom_profile_count": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "rom_profile_query": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_size_t, _c_double_p, C.POINTER(C.c_long),
                                    _c_double_p, _c_double_p]),
    "rom_buf_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "rom_buf_free": (C.c_int, [_vp]),
    "rom_buf_size": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "rom_buf_upload": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t]),
    "rom_buf_download": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t]),
    "rom_buf_fill": (C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_double]),
    "rom_buf_copy": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t]),
    "rom_buf_equal": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]),
    "rom_buf_gather_rows": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_size_t]),
    "rom_fem_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "rom_fem_destroy": (C.c_int, [_vp]),
    "rom_fem_dims": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                               C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rom_fem_load_vector_host": (C.c_int, [_vp, _vp]),
    "rom_assemble_batch": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "rom_solve_batch": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64]),
    "rom_solve_batch_async": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64]),
    "rom_solve_status": (C.c_int, [_vp]),
    "rom_fem_reduced_stride": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "rom_fem_expansion_is_linear": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "rom_fem_reduced_layout": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rom_fem_compact_stride": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "rom_fem_pack_reduced_async": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, C.c_int64]),
    "rom_fem_unpack_reduced_async": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, C.c_int64]),
    "rom_comm_allgather_packed_async": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, C.c_size_t, C.c_int]),
    "rom_solve_reduced_async": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64]),
    "rom_expand_batch_async": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, _vp, C.c_int64]),
    "rom_solve_work": (C.c_int, [_vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "rom_stencil_apply": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, C.c_int, _vp, C.c_int64]),
    "rom_h10norm": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int, _vp]),
    "rom_l2norm": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp]),
    "rom_gemm_nt": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_double, _vp, C.c_size_t, C.c_int64,
                              _vp, C.c_size_t, C.c_int64, C.c_double, _vp, C.c_size_t, C.c_int64]),
    "rom_gram": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64]),
    "rom_gemm_nn": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_double, _vp, C.c_size_t, C.c_int64,
                              _vp, C.c_size_t, C.c_int64, C.c_double, _vp, C.c_size_t, C.c_int64]),
    "rom_reduced_solve_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp]),
    "rom_buf_scale": (C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_double]),
    "rom_host_alloc": (C.c_int, [C.c_size_t, C.c_int, C.POINTER(C.POINTER(C.c_double))]),
    "rom_host_free": (C.c_int, [C.POINTER(C.c_double)]),
    "rom_center_rows": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp]),
    "rom_rows_scale": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp]),
    "rom_rows_sign_flip": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64]),
    "rom_evaluate_points": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "rom_riesz_h10": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "rom_riesz_norms_h10": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "rom_sensor_greedy": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double,
                                    _vp, _vp, _vp, _vp, _vp]),
    "rom_project_h10": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, C.c_int64, C.c_int, _vp, C.c_int64]),
    "rom_galerkin_rom": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, C.c_int, _vp, C.c_int64]),
    "rom_orthonormalize_rows": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp, C.c_int64]),
    "rom_greedy": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rom_error_curves": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, C.c_int64, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "rom_pod": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp]),
    "rom_fem_energy_map": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rom_h10norm_factored": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp]),
    "rom_greedy_factored": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rom_pod_factored": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp]),
    "rom_pod_ex": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, _vp, C.c_int64, _vp, _vp]),
    "rom_pca_tall": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp]),
    "rom_sine_transform": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]),
    "rom_pod_h10": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int64, _vp, _vp]),
    "rom_pod_h10_factored": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp]),
    "rom_symmetric_orthonormalize": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int64]),
    "rom_complete_orthonormal": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64]),
    "rom_small_eig_host": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp, _vp]),
    "rom_resid_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "rom_resid_destroy": (C.c_int, [_vp]),
    "rom_resid_append": (C.c_int, [_vp, _vp, C.c_int64, C.c_int]),
    "rom_resid_query": (C.c_int, [_vp, _vp]),
    "rom_resid_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "rom_resid_basis": (C.c_int, [_vp, _vp, C.c_int64]),
    "rom_resid_eval": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64]),
    "rom_weak_greedy": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int, C.c_double, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "rom_poly_terms": (C.c_int, [C.c_int, C.c_int, _vp, _vp]),
    "rom_poly_fit": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int,
                               C.c_double, C.POINTER(_vp), _vp]),
    "rom_poly_predict": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64,
                                   _vp]),
    "rom_poly_query": (C.c_int, [_vp, _vp]),
    "rom_poly_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "rom_poly_destroy": (C.c_int, [_vp]),
    "rom_mlp_layout": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    "rom_mlp_fit": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int, _vp,
                              C.c_int, C.c_double, C.c_int, _vp, C.c_int, C.c_double, C.c_int, C.POINTER(_vp), _vp]),
    "rom_mlp_loss_grad": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64, C.c_int64, C.c_double, _vp, _vp]),
    "rom_mlp_predict": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64,
                                  _vp]),
    "rom_mlp_query": (C.c_int, [_vp, _vp]),
    "rom_mlp_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "rom_mlp_destroy": (C.c_int, [_vp]),
    "rom_nearest": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int, C.c_int,
                              C.c_int, _vp, _vp, _vp]),
    "rom_kmeans_layout": (C.c_int, [C.c_int, C.c_int, _vp]),
    "rom_kmeans_init_maximin": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int, _vp]),
    "rom_kmeans_fit": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp,
                                 _vp]),
    "rom_kmeans_assign": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int64, C.c_int, _vp, _vp, _vp]),
    "rom_kmeans_query": (C.c_int, [_vp, _vp]),
    "rom_kmeans_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "rom_kmeans_destroy": (C.c_int, [_vp]),
    "rom_lm_polish": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp,
                                _vp, C.c_int, C.c_double, _vp, C.c_size_t, C.c_int64, _vp]),
    "rom_mcmc_layout": (C.c_int, [C.c_int, C.c_int, _vp]),
    "rom_mcmc": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                           C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t,
                           C.c_int64, _vp]),
    "rom_sensor_dopt_layout": (C.c_int, [C.c_int, C.c_int, _vp]),
    "rom_sensor_dopt_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, C.c_double, _vp,
                                       C.c_size_t, _vp]),
    "rom_sensor_dopt_scores": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp,
                                         C.c_size_t]),
    "rom_sensor_dopt": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64, C.c_int64, C.c_int,
                                  C.c_double, _vp, C.c_int, _vp, _vp, _vp]),
    "rom_poly_sense": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                 C.c_int, C.c_double, _vp, C.c_size_t, C.c_int64, _vp]),
    "rom_mlp_sense": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int, _vp,
                                _vp, _vp, _vp, C.c_int, C.c_double, _vp, C.c_size_t, C.c_int64, _vp]),
    "rom_bvls": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_size_t,
                           C.c_int64, _vp, _vp]),
    "rom_local_select_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "rom_local_select": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int, _vp,
                                   _vp, _vp, _vp, C.c_int, _vp, C.c_size_t, C.c_int64, _vp, _vp]),
    "rom_tree_fit": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int, _vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int,
                               _vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), _vp]),
    "rom_tree_predict": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, C.c_size_t, C.c_int64, _vp, C.c_size_t, C.c_int64,
                                   _vp]),
    "rom_tree_query": (C.c_int, [_vp, _vp]),
    "rom_tree_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "rom_tree_destroy": (C.c_int, [_vp]),
    "rom_comm_unique_id": (C.c_int, [C.c_char_p, C.c_size_t]),
    "rom_comm_init": (C.c_int, [_vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int]),
    "rom_comm_destroy": (C.c_int, [_vp]),
    "rom_comm_allgather": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t]),
    "rom_comm_allgather_async": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_int]),
    "rom_comm_wait_slot": (C.c_int, [_vp, C.c_int]),
    "rom_comm_wait": (C.c_int, [_vp, C.c_int]),
    "rom_comm_allreduce_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
}


def load_library(path: str = LIB_PATH):
    """dlopen libromhc.so and attach prototypes.  No GPU is touched here."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RomLibraryError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C romhighcontrast_amd/csrc` (hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load_library().rom_last_error().decode("utf-8", "replace")


def check(status: int):
    """Map a C status to the exception types the reference raises."""
    if status == ROM_OK:
        return
    msg = last_error()
    if status == ROM_ERR_NOT_SPD:
        raise LinAlgError(msg)  # scipy.linalg.solve(assume_a='pos') raises this in the reference
    if status == ROM_ERR_NOMEM:
        raise MemoryError(msg)
    raise RomLibraryError(f"libromhc error {status}: {msg}")


# downloads of at least this many bytes land in page-locked host memory (0 disables: ROMHC_PINNED_DOWNLOAD_BYTES)
PINNED_DOWNLOAD_BYTES = int(os.environ.get("ROMHC_PINNED_DOWNLOAD_BYTES", str(8 << 20))) or (1 << 62)


_download_sizes: dict = {}  # size -> number of large downloads of that size so far


def _pinned_array(lib, n: int):
    """A writable float64 array of n entries in page-locked memory from libromhc's pool; the block returns to the pool
    when the array (and every view of it) is gone.  Pinning new memory costs ten copies' worth of time, so that only
    happens for a size that keeps coming back (third request on); before, a block is used if the pool has one.
    None: the caller falls back to np.empty."""
    seen = _download_sizes[n] = _download_sizes.get(n, 0) + 1
    p = C.POINTER(C.c_double)()
    if lib.rom_host_alloc(n, 0 if seen >= 3 else 1, C.byref(p)) != 0 or not p:
        return None
    addr = C.cast(p, C.c_void_p).value
    raw = (C.c_double * n).from_address(addr)
    weakref.finalize(raw, lib.rom_host_free, C.cast(addr, C.POINTER(C.c_double)))
    return np.frombuffer(raw, dtype=np.float64)


def _host(arr: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(arr, dtype=np.float64)


class Context:
    """One GPU + stream.  Process-wide singleton per device (``get_context``)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        n = C.c_int(0)
        try:
            check(self.lib.rom_device_count(C.byref(n)))
        except RomLibraryError as e:
            raise RomLibraryError(f"no usable HIP device: {e}. libromhc needs an MI355X (gfx950).") from None
        if n.value < 1:
            raise RomLibraryError("no HIP device visible; libromhc needs an MI355X (gfx950). No CPU fallback.")
        h = _vp()
        check(self.lib.rom_init(device, C.byref(h)))
        self.h = h
        self.has_comm = False
        self.device = device

    # -- buffers ---------------------------------------------------------------------------
    def alloc(self, n: int) -> "Buffer":
        return Buffer(self, int(n))

    def upload(self, arr) -> "Buffer":
        arr = _host(arr)
        b = Buffer(self, arr.size)
        b.upload(arr)
        return b

    def synchronize(self):
        check(self.lib.rom_synchronize(self.h))

    def solve_status(self):
        """Wait for the sweeps enqueued with wait=False; raises (scipy LinAlgError) if any pivot was not positive."""
        check(self.lib.rom_solve_status(self.h))

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        check(self.lib.rom_device_name(self.h, buf, 256))
        return buf.value.decode()

    def set_workspace_limit(self, nbytes: int):
        check(self.lib.rom_set_workspace_limit(self.h, int(nbytes)))

    # -- timing ----------------------------------------------------------------------------
    def timer_start(self):
        check(self.lib.rom_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_double(0)
        check(self.lib.rom_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile(self, on: bool):
        check(self.lib.rom_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.rom_profile_reset(self.h))

    def profile_report(self):
        n = C.c_int(0)
        check(self.lib.rom_profile_count(self.h, C.byref(n)))
        out = {}
        for i in range(n.value):
            name = C.create_string_buffer(128)
            ms, fl, by = C.c_double(0), C.c_double(0), C.c_double(0)
            cnt = C.c_long(0)
            check(self.lib.rom_profile_query(self.h, i, name, 128, C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by)))
            out[name.value.decode()] = dict(total_ms=ms.value, launches=cnt.value, flops=fl.value, bytes=by.value)
        return out

    # -- dense ops ---------------------------------------------------------------------------
    def gemm_nt(self, m, n, k, A, a_off, lda, B, b_off, ldb, Cb, c_off, ldc, alpha=1.0, beta=0.0):
        check(self.lib.rom_gemm_nt(self.h, m, n, k, alpha, A.h, a_off, lda, B.h, b_off, ldb, beta, Cb.h, c_off, ldc))

    def gram(self, m, k, A, a_off, lda, Cb, c_off, ldc):
        check(self.lib.rom_gram(self.h, m, k, A.h, a_off, lda, Cb.h, c_off, ldc))

    def gemm_nn(self, m, n, k, A, a_off, lda, B, b_off, ldb, Cb, c_off, ldc, alpha=1.0, beta=0.0):
        check(self.lib.rom_gemm_nn(self.h, m, n, k, alpha, A.h, a_off, lda, B.h, b_off, ldb, beta, Cb.h, c_off, ldc))

    def reduced_solve_batch(self, n, kb, M, Ahat, w, rhs, rhs_per_system, c_out):
        check(self.lib.rom_reduced_solve_batch(self.h, n, kb, M, Ahat.h, w.h, rhs.h, 1 if rhs_per_system else 0,
                                               c_out.h))

    def center_rows(self, X: "Buffer", M, dim, mean: "Buffer", row0=0):
        check(self.lib.rom_center_rows(self.h, X.h, row0, M, dim, mean.h))

    def rows_scale(self, X: "Buffer", rows, dim, factors, row0=0):
        f = _host(np.asarray(factors, dtype=np.float64))
        check(self.lib.rom_rows_scale(self.h, X.h, row0, rows, dim, f.ctypes.data))

    def rows_sign_flip(self, X: "Buffer", rows, dim, row0=0):
        check(self.lib.rom_rows_sign_flip(self.h, X.h, row0, rows, dim))

    def l2norm(self, U: "Buffer", row0, K, dim) -> np.ndarray:
        out = np.empty(K)
        check(self.lib.rom_l2norm(self.h, U.h, row0, K, dim, out.ctypes.data))
        return out

    # -- basis stage (single C calls) ------------------------------------------------------------
    def orthonormalize_rows(self, X: "Buffer", n, dim, Q: "Buffer", x_row0=0, q_row0=0):
        check(self.lib.rom_orthonormalize_rows(self.h, X.h, x_row0, n, dim, Q.h, q_row0))

    def pod(self, X: "Buffer", M, dim, n, V: "Buffer", center=True, x_row0=0, v_row0=0, rel_floor=0.0):
        """rom_pod / rom_pod_ex: X is overwritten.  Returns (sigma (n,), info dict)."""
        sigma, info = np.zeros(max(n, 1)), np.zeros(8)
        check(self.lib.rom_pod_ex(self.h, X.h, x_row0, M, dim, n, 1 if center else 0, float(rel_floor), V.h, v_row0,
                                  sigma.ctypes.data, info.ctypes.data))
        return sigma[:n], _pod_info(info)

    def pca_tall(self, X: "Buffer", M, dim, n, V: "Buffer", S: "Buffer | None" = None, mean: "Buffer | None" = None, center=True,
                 x_row0=0, v_row0=0, s_row0=0):
        """rom_pca_tall: X is overwritten when center.  Returns (sigma (n,), info dict)."""
        sigma, info = np.zeros(max(n, 1)), np.zeros(8)
        check(self.lib.rom_pca_tall(self.h, X.h, x_row0, M, dim, n, 1 if center else 0, V.h, v_row0, S.h if S is not None else None,
                                    s_row0, mean.h if mean is not None else None, sigma.ctypes.data, info.ctypes.data))
        d = dict(resolved_modes=int(info[0]), passes=int(info[1]), decompositions=int(info[2]), executed_flops=float(info[3]),
                 worst_ratio=float(info[4]), stop_reason=("converged", "budget")[int(info[5])], host_syncs=int(info[6]))
        return sigma[:n], d

    def poly_fit(self, X: "Buffer", x_off, ldx, m, Y: "Buffer", y_off, ldy, q, M, degree, rcond=0.0) -> "PolyMap":
        """rom_poly_fit: the least-squares polynomial map of total degree <= ``degree`` from the m columns of X (from element
        x_off, row stride ldx) to the q columns of Y over M rows.  Neither block is modified.  Returns the PolyMap."""
        return PolyMap(self, X, x_off, ldx, m, Y, y_off, ldy, q, M, degree, rcond)

    def mlp_fit(self, X: "Buffer", x_off, ldx, m, Y: "Buffer", y_off, ldy, q, M, hidden, w0, activation="tanh", alpha=1e-4,
                scale_targets=True, max_iter=200, tol=1e-6, memory=10) -> "MLPHandle":
        """rom_mlp_fit: the MLP map m -> ``hidden`` -> q from the columns of X to the columns of Y over M rows (addressed as in
        ``poly_fit``; neither block is modified), trained from the flat initial parameters ``w0`` (``mlp_layout``) by the
        device L-BFGS.  max_iter = 0: the handle holds w0 and the scalings.  Returns the MLPHandle."""
        return MLPHandle(self, X, x_off, ldx, m, Y, y_off, ldy, q, M, hidden, w0, activation, alpha, scale_targets, max_iter, tol, memory)

    def tree_fit(self, X: "Buffer", x_off, ldx, m, Y: "Buffer", y_off, ldy, q, M, T=1, counts=None, max_depth=None,
                 min_samples_split=2, min_samples_leaf=1) -> "TreeMapHandle":
        """rom_tree_fit: T regression trees (a bagged forest) from the m columns of X (from element x_off, row stride ldx) to the
        q columns of Y over M rows, built level by level on the device.  ``counts``: (T, M) integer multiplicities of the rows
        per tree (the bootstrap), None: every row once.  Neither block is modified.  Returns the TreeMapHandle."""
        return TreeMapHandle(self, X, x_off, ldx, m, Y, y_off, ldy, q, M, T, counts, max_depth, min_samples_split, min_samples_leaf)

    def nearest(self, Q: "Buffer", q_off, ldq, M, P: "Buffer", p_off, ldp, K, r, t=1, mode=0):
        """rom_nearest: for the K rows of P the t rows of the library Q (M rows; both r columns from an element offset with a
        row stride) at the smallest squared distance, sorted by (distance, row).  mode 1: the exhaustive kernel for every query.
        Returns (idx (K, t) int64, dist2 (K, t), info dict)."""
        idx, dist2, info = np.zeros((int(K), int(t)), dtype=np.int64), np.zeros((int(K), int(t))), np.zeros(8)
        check(self.lib.rom_nearest(self.h, Q.h if Q is not None else None, int(q_off), int(ldq), int(M), P.h if P is not None else None,
                                   int(p_off), int(ldp), int(K), int(r), int(t), int(mode), idx.ctypes.data, dist2.ctypes.data,
                                   info.ctypes.data))
        d = dict(group_size=int(info[0]), groups_rescored=int(info[1]), certified=int(info[2]), fallbacks=int(info[3]),
                 launches=int(info[4]), host_syncs=int(info[5]), workspace_bytes=int(info[6]), executed_flops=float(info[7]))
        return idx, dist2, d

    def kmeans_layout(self, r, kc) -> dict:
        """rom_kmeans_layout (host only): see the module function ``kmeans_layout``."""
        return kmeans_layout(r, kc)

    def kmeans_init_maximin(self, X: "Buffer", x_off, ldx, r, M, kc) -> np.ndarray:
        """rom_kmeans_init_maximin: the kc rows of the deterministic farthest-point start (the row nearest to the column means,
        then always the row farthest from the rows chosen so far; lowest index among equals), int64."""
        kmeans_layout(r, kc)
        rows = np.zeros(int(kc), dtype=np.int64)
        _check_kmeans(self.lib.rom_kmeans_init_maximin(self.h, X.h if X is not None else None, int(x_off), int(ldx), int(r), int(M), int(kc),
                                                       rows.ctypes.data))
        return rows

    def kmeans_fit(self, X: "Buffer", x_off, ldx, r, M, kc, init, max_iter=50, tol=0.0, mode=0) -> "KMeansHandle":
        """rom_kmeans_fit: Lloyd's algorithm on the M rows of X (r columns from element x_off, row stride ldx; not modified) from
        the (kc, r) initial centroids ``init``.  mode 1: the exhaustive scan instead of the fused screen (the same bits).
        max_iter = 0: the handle holds ``init`` and its assignment.  Returns the KMeansHandle."""
        return KMeansHandle(self, X, x_off, ldx, r, M, kc, init, max_iter, tol, mode)

    def kmeans_assign(self, handle: "KMeansHandle", X: "Buffer", x_off, ldx, M, mode=0, dist2=True):
        """rom_kmeans_assign: (labels (M,) int32, dist2 (M,) or None, inertia) of the M rows of X against the handle's centroids."""
        return handle.assign(X, x_off, ldx, M, mode=mode, dist2=dist2)

    def lm_polish(self, n, k, r, Ahat: "Buffer", bhat: "Buffer", Gr: "Buffer", P: "Buffer", p_off, ldp, K, t, THETA0: "Buffer", lo, hi,
                  AUX: "Buffer | None" = None, max_iter=30, misfit_tol=1e-3, OUT: "Buffer | None" = None, out_off=0, ldo=None):
        """rom_lm_polish: inverse.polish_parameters on the device in reduced sensor coordinates (P: K rows p = U^T (w y) of r
        columns, Gr (r, n) = S V^T, AUX (K, 2) = perp2, scale or None), from the t starts THETA0 (K, t, k) per query inside the
        box [lo, hi].  OUT (rows of ldo >= k + n + 5 from out_off) is allocated when None; the coefficients stay in it at column
        k.  Returns (PolishResult, info dict)."""
        from .inverse import PolishResult
        n, k, K = int(n), int(k), int(K)
        ldo = k + n + 5 if ldo is None else int(ldo)
        lo = _host(np.broadcast_to(np.asarray(lo, dtype=np.float64), (k,)))
        hi = _host(np.broadcast_to(np.asarray(hi, dtype=np.float64), (k,)))
        if OUT is None and K > 0:
            OUT = self.alloc(int(out_off) + K * ldo)
        info = np.zeros(8)
        check(self.lib.rom_lm_polish(self.h, n, k, int(r), Ahat.h, bhat.h, Gr.h, P.h if P is not None else None, int(p_off), int(ldp), K,
                                     int(t), THETA0.h if THETA0 is not None else None, lo.ctypes.data, hi.ctypes.data,
                                     AUX.h if AUX is not None else None, int(max_iter), float(misfit_tol),
                                     OUT.h if OUT is not None else None, int(out_off), ldo, info.ctypes.data))
        rows = np.zeros((K, ldo))
        if K:   # (the last row may end with the buffer, k + n + 5 doubles in)
            rows.reshape(-1)[:(K - 1) * ldo + k + n + 5] = OUT.download((K - 1) * ldo + k + n + 5, offset=int(out_off))
        res = PolishResult(rows[:, :k].copy(), rows[:, k + n].copy(), rows[:, k:k + n].copy(), rows[:, k + n + 2] != 0.0,
                           rows[:, k + n + 3].astype(np.int64), rows[:, k + n + 1].copy(), rows[:, k + n + 4].astype(np.int64))
        d = dict(launches=int(info[0]), host_syncs=int(info[1]), workspace_bytes=int(info[2]), systems=int(info[3]),
                 iterations=int(info[4]), factorisations=int(info[5]))
        return res, d

    def mcmc_layout(self, n, k) -> dict:
        """rom_mcmc_layout: the state row of a chain, offsets by name and ``row``, its length (inverse.mcmc_layout)."""
        v = np.zeros(8, dtype=np.int64)
        check(self.lib.rom_mcmc_layout(int(n), int(k), v.ctypes.data))
        row, phi, ls, mean, M2, mean_c, kept, phi_min = (int(x) for x in v)
        return dict(theta=0, phi=phi, ls=ls, mean=mean, M2=M2, mean_c=mean_c, kept=kept, accepted=kept + 1, outside=kept + 2,
                    not_spd=kept + 3, phi_min=phi_min, theta_min=phi_min + 1, row=row)

    def mcmc(self, n, k, r, Ahat: "Buffer", bhat: "Buffer", Gr: "Buffer", P: "Buffer", p_off, ldp, K, t, INVVAR: "Buffer",
             LPROP: "Buffer", lo, hi, seed, steps, burn, thin, STATE: "Buffer", s_off=0, lds=None, SAMPLES: "Buffer | None" = None,
             smp_off=0, slots=0, chain0=0, step0=0) -> dict:
        """rom_mcmc: inverse.mcmc_host on the device in reduced sensor coordinates (P: K rows of r columns, INVVAR (K,) = 1 /
        sigma^2, LPROP (K, k, k) the proposal factors), t chains per query with the ids chain0 + position, the steps step0 ..
        step0 + steps - 1.  STATE (rows of lds >= the row of ``mcmc_layout`` from s_off) holds the starts in its first k columns
        (step0 = 0) or the rows to resume from and receives the rows; SAMPLES ([chain][slot][k] from smp_off) or None.  Returns
        the info dict."""
        k = int(k)
        lds = self.mcmc_layout(n, k)["row"] if lds is None else int(lds)
        lo = _host(np.broadcast_to(np.asarray(lo, dtype=np.float64), (k,)))
        hi = _host(np.broadcast_to(np.asarray(hi, dtype=np.float64), (k,)))
        info = np.zeros(8)
        h = lambda b: b.h if b is not None else None  # noqa: E731
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        seed -= (seed >> 63) << 64   # (the same 64 bits as a signed number)
        check(self.lib.rom_mcmc(self.h, int(n), k, int(r), Ahat.h, bhat.h, Gr.h, h(P), int(p_off), int(ldp), int(K), int(t), h(INVVAR),
                                h(LPROP), lo.ctypes.data, hi.ctypes.data, seed, int(chain0), int(step0),
                                int(steps), int(burn), int(thin), h(STATE), int(s_off), lds, h(SAMPLES), int(smp_off), int(slots),
                                info.ctypes.data))
        return dict(launches=int(info[0]), host_syncs=int(info[1]), workspace_bytes=int(info[2]), chains=int(info[3]),
                    steps=int(info[4]), evaluations=int(info[5]))

    def sensor_dopt_layout(self, n, k) -> dict:
        """rom_sensor_dopt_layout (host only): see the module function ``sensor_dopt_layout``."""
        return sensor_dopt_layout(n, k)

    def sensor_dopt_init(self, n, k, Ahat: "Buffer", bhat: "Buffer", THETA: "Buffer", t_off, ldt, M, T0, sigma,
                         STATE: "Buffer | None" = None, s_off=0):
        """rom_sensor_dopt_init: the design state of the empty sensor set for the M rows theta_j of THETA (k columns from t_off,
        stride ldt): per entry Z_j = X_j T0 / sigma and T_j = T0 (T0 (k, k): a factor of the prior covariance).  STATE (M blocks
        of ``sensor_dopt_layout(n, k)["entry"]`` doubles from s_off) is allocated when None.  Returns (STATE, info dict)."""
        n, k, M = int(n), int(k), int(M)
        lay = sensor_dopt_layout(n, k)
        T0 = _host(np.asarray(T0, dtype=np.float64).reshape(k, k))
        if STATE is None:
            STATE = self.alloc(int(s_off) + max(M, 1) * lay["entry"])
        info = np.zeros(8)
        _check_kmeans(self.lib.rom_sensor_dopt_init(self.h, n, k, Ahat.h, bhat.h, THETA.h, int(t_off), int(ldt), M, T0.ctypes.data,
                                                    float(sigma), STATE.h, int(s_off), info.ctypes.data))
        return STATE, dict(skipped=int(info[0]), launches=int(info[1]), host_syncs=int(info[2]), workspace_bytes=int(info[3]))

    def sensor_dopt_scores(self, n, k, STATE: "Buffer", s_off, M, E: "Buffer", e_off, lde, ncand, SCORE: "Buffer | None" = None,
                           sc_off=0) -> "Buffer":
        """rom_sensor_dopt_scores: SCORE[sc_off + x] = sum_j log1p(|Z_j^T e_x|^2) for the ncand rows e_x of E (n columns from
        e_off, stride lde): one scoring pass, no update -- the information map.  SCORE is allocated when None.  Returns SCORE."""
        if SCORE is None:
            SCORE = self.alloc(int(sc_off) + max(int(ncand), 1))
        _check_kmeans(self.lib.rom_sensor_dopt_scores(self.h, int(n), int(k), STATE.h, int(s_off), int(M), E.h, int(e_off), int(lde),
                                                      int(ncand), SCORE.h, int(sc_off)))
        return SCORE

    def sensor_dopt(self, n, k, STATE: "Buffer", s_off, M, E: "Buffer", e_off, lde, ncand, m, rel_tol=0.0, taken=None):
        """rom_sensor_dopt: up to m greedy D-optimal picks among the ncand candidate rows of E; STATE is updated in place, so a
        second call continues the design -- ``taken``: the picks of the earlier calls, which are not picked again.  Returns
        (picks (made,) int64, gain (made,), info dict); ValueError, naming the limit, outside the limits."""
        m = int(m)
        picks, gain, info = np.full(max(m, 1), -1, dtype=np.int32), np.zeros(max(m, 1)), np.zeros(8)
        tk = np.ascontiguousarray(np.zeros(0) if taken is None else taken, dtype=np.int32).ravel()
        _check_kmeans(self.lib.rom_sensor_dopt(self.h, int(n), int(k), STATE.h, int(s_off), int(M), E.h, int(e_off), int(lde), int(ncand),
                                               m, float(rel_tol), tk.ctypes.data if tk.size else None, int(tk.size),
                                               picks.ctypes.data, gain.ctypes.data, info.ctypes.data))
        made = int(info[0])
        d = dict(picks=made, stop_reason=int(info[1]), skipped=int(info[2]), nan_candidates=int(info[3]), launches=int(info[4]),
                 host_syncs=int(info[5]), workspace_bytes=int(info[6]), flops=float(info[7]))
        return picks[:made].astype(np.int64), gain[:made].copy(), d

    def poly_sense(self, m, d, r, Gr: "Buffer", P: "Buffer", p_off, ldp, K, t, T0: "Buffer", lo, hi, AUX: "Buffer | None" = None,
                   max_iter=30, misfit_tol=1e-3, OUT: "Buffer | None" = None, out_off=0, ldo=None):
        """rom_poly_sense: nonlinear.sense_scores on the device (Gr (r, P) = Sigma V^T of the sensing matrix, the terms of
        ``poly_terms(m, d)``; P: K rows p = U^T (w y) of r columns; AUX (K, 2) = perp2, scale or None), from the t starts T0
        (K, t, m) per query inside the box [lo, hi]; lo_j == hi_j pins coordinate j.  OUT (rows of ldo >= m + 5 from out_off) is
        allocated when None.  Returns (SenseResult, info dict)."""
        from .nonlinear import SenseResult
        m, K = int(m), int(K)
        ldo = m + 5 if ldo is None else int(ldo)
        lo = _host(np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,)))
        hi = _host(np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,)))
        if OUT is None and K > 0:
            OUT = self.alloc(int(out_off) + K * ldo)
        info = np.zeros(8)
        check(self.lib.rom_poly_sense(self.h, m, int(d), int(r), Gr.h, P.h if P is not None else None, int(p_off), int(ldp), K, int(t),
                                      T0.h if T0 is not None else None, lo.ctypes.data, hi.ctypes.data,
                                      AUX.h if AUX is not None else None, int(max_iter), float(misfit_tol),
                                      OUT.h if OUT is not None else None, int(out_off), ldo, info.ctypes.data))
        rows = np.zeros((K, ldo))
        if K:   # (the last row may end with the buffer, m + 5 doubles in)
            rows.reshape(-1)[:(K - 1) * ldo + m + 5] = OUT.download((K - 1) * ldo + m + 5, offset=int(out_off))
        res = SenseResult(rows[:, :m].copy(), rows[:, m].copy(), rows[:, m + 2] != 0.0, rows[:, m + 3].astype(np.int64),
                          rows[:, m + 1].copy(), rows[:, m + 4].astype(np.int64))
        d8 = dict(launches=int(info[0]), host_syncs=int(info[1]), workspace_bytes=int(info[2]), systems=int(info[3]),
                  iterations=int(info[4]), evaluations=int(info[5]))
        return res, d8

    def mlp_sense(self, m, hidden, activation, WH: "Buffer", r, Gr: "Buffer", P: "Buffer", p_off, ldp, K, t, T0: "Buffer", lo, hi,
                  AUX: "Buffer | None" = None, max_iter=30, misfit_tol=1e-3, OUT: "Buffer | None" = None, out_off=0, ldo=None):
        """rom_mlp_sense: nonlinear.mlp_sense_scores on the device: ``poly_sense`` with the features [1; t; last hidden layer] of
        the network m -> ``hidden`` with ``activation`` ("tanh", "logistic" / "sigmoid", "relu"); WH: the hidden layers' flat
        parameters (all W_l, outputs x inputs row-major, then all b_l), Gr (r, 1 + m + hidden[-1]).  Everything else as in
        ``poly_sense``; ``evaluations`` counts forward passes.  Returns (SenseResult, info dict)."""
        from .nonlinear import SenseResult
        m, K = int(m), int(K)
        if activation not in MLP_ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(MLP_ACTIVATIONS)}")
        hid = np.ascontiguousarray([int(v) for v in hidden], dtype=np.int32)
        ldo = m + 5 if ldo is None else int(ldo)
        lo = _host(np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,)))
        hi = _host(np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,)))
        if OUT is None and K > 0:
            OUT = self.alloc(int(out_off) + K * ldo)
        info = np.zeros(8)
        check(self.lib.rom_mlp_sense(self.h, m, len(hid), hid.ctypes.data if len(hid) else None, MLP_ACTIVATIONS[activation], WH.h, int(r),
                                     Gr.h, P.h if P is not None else None, int(p_off), int(ldp), K, int(t),
                                     T0.h if T0 is not None else None, lo.ctypes.data, hi.ctypes.data,
                                     AUX.h if AUX is not None else None, int(max_iter), float(misfit_tol),
                                     OUT.h if OUT is not None else None, int(out_off), ldo, info.ctypes.data))
        rows = np.zeros((K, ldo))
        if K:   # (the last row may end with the buffer, m + 5 doubles in)
            rows.reshape(-1)[:(K - 1) * ldo + m + 5] = OUT.download((K - 1) * ldo + m + 5, offset=int(out_off))
        res = SenseResult(rows[:, :m].copy(), rows[:, m].copy(), rows[:, m + 2] != 0.0, rows[:, m + 3].astype(np.int64),
                          rows[:, m + 1].copy(), rows[:, m + 4].astype(np.int64))
        d8 = dict(launches=int(info[0]), host_syncs=int(info[1]), workspace_bytes=int(info[2]), systems=int(info[3]),
                  iterations=int(info[4]), evaluations=int(info[5]))
        return res, d8

    def bvls(self, n, r, Gr: "Buffer", P: "Buffer", p_off, ldp, K, lo, hi, AUX: "Buffer | None" = None, max_iter=None,
             OUT: "Buffer | None" = None, out_off=0, ldo=None, bound=True):
        """rom_bvls: inverse.bvls_host on the device -- for the K rows p of P (r columns from p_off with stride ldp)
        min over lo <= c <= hi of ||p - Gr c||^2 with Gr (r, n) shared; AUX (K, 2) = perp2, scale or None; max_iter None: 5 n + 10.
        lo_j == hi_j pins coordinate j, infinite bounds are allowed.  OUT (rows of ldo >= n + 4 from out_off: c | misfit | bound
        variables | converged | passes) is allocated when None; ``bound`` False leaves BOUND out (the result's bound is then
        None).  Returns (BvlsResult, info dict)."""
        from .inverse import BvlsResult
        n, K = int(n), int(K)
        ldo = n + 4 if ldo is None else int(ldo)
        max_iter = 5 * n + 10 if max_iter is None else int(max_iter)
        lo = _host(np.broadcast_to(np.asarray(lo, dtype=np.float64), (n,)))
        hi = _host(np.broadcast_to(np.asarray(hi, dtype=np.float64), (n,)))
        if OUT is None and K > 0:
            OUT = self.alloc(int(out_off) + K * ldo)
        BOUND = self.alloc(K * n) if bound and K > 0 else None
        info = np.zeros(8)
        check(self.lib.rom_bvls(self.h, n, int(r), Gr.h, P.h if P is not None else None, int(p_off), int(ldp), K, lo.ctypes.data,
                                hi.ctypes.data, AUX.h if AUX is not None else None, max_iter, OUT.h if OUT is not None else None,
                                int(out_off), ldo, BOUND.h if BOUND is not None else None, info.ctypes.data))
        rows = np.zeros((K, ldo))
        if K:   # (the last row may end with the buffer, n + 4 doubles in)
            rows.reshape(-1)[:(K - 1) * ldo + n + 4] = OUT.download((K - 1) * ldo + n + 4, offset=int(out_off))
        st = None
        if bound:
            st = (BOUND.download(K * n).reshape(K, n) if K else np.zeros((0, n))).astype(np.int64)
        res = BvlsResult(rows[:, :n].copy(), rows[:, n].copy(), st, rows[:, n + 2] != 0.0, rows[:, n + 3].astype(np.int64))
        d8 = dict(launches=int(info[0]), host_syncs=int(info[1]), workspace_bytes=int(info[2]), systems=int(info[3]),
                  passes=int(info[4]), factorisations=int(info[5]), bound_variables=rows[:, n + 1].astype(np.int64))
        return res, d8

    def local_select_layout(self, n, k, rank, r) -> dict:
        """rom_local_select_layout (host only): see the module function ``local_select_layout``."""
        return local_select_layout(n, k, rank, r)

    def local_select(self, kc, n, k, rank, r, RT: "Buffer", GR: "Buffer", P: "Buffer", p_off, ldp, K, c_lo, c_hi, a_lo, a_hi,
                     max_iter=None, OUT: "Buffer | None" = None, out_off=0, ldo=None):
        """rom_local_select: inverse.local_select_host on the device -- RT the kc residual tables (rank x (1 + k n) each), GR the
        kc reduced sensor matrices (r x n each), P K rows of kc r reduced measurements (from p_off with stride ldp); the boxes
        kc x n (c_lo, c_hi) and kc x k (a_lo, a_hi) host arrays; max_iter None: 5 n + 10 and 5 k + 10.  OUT (rows of
        ldo >= n + k + 5 from out_off, row i kc + j: c | a | S | misfit | passes, passes | status) is allocated when None.
        ValueError outside the limits of ``local_select_layout`` or for a bad box.  Returns (LocalSelectResult, info dict)."""
        from .inverse import _local_select_result
        kc, n, k, rank, r, K = int(kc), int(n), int(k), int(rank), int(r), int(K)
        local_select_layout(n, k, rank, r)
        w = n + k + 5
        ldo = w if ldo is None else int(ldo)
        box = [_host(np.broadcast_to(np.asarray(b, dtype=np.float64), (kc, d))) for b, d in ((c_lo, n), (c_hi, n), (a_lo, k), (a_hi, k))]
        if OUT is None and K > 0:
            OUT = self.alloc(int(out_off) + K * kc * ldo)
        labels, info = np.full(K, -1, dtype=np.int32), np.zeros(8)
        _check_kmeans(self.lib.rom_local_select(self.h, kc, n, k, rank, r, RT.h, GR.h, P.h if P is not None else None, int(p_off),
                                                int(ldp), K, box[0].ctypes.data, box[1].ctypes.data, box[2].ctypes.data,
                                                box[3].ctypes.data, -1 if max_iter is None else int(max_iter),
                                                OUT.h if OUT is not None else None, int(out_off), ldo, labels.ctypes.data,
                                                info.ctypes.data))
        rows = np.zeros((K * kc, ldo))
        if K:   # (the last row may end with the buffer, n + k + 5 doubles in)
            rows.reshape(-1)[:(K * kc - 1) * ldo + w] = OUT.download((K * kc - 1) * ldo + w, offset=int(out_off))
        res = _local_select_result(rows[:, :w].reshape(K, kc, w), labels, n, k)
        d8 = dict(systems=int(info[0]), launches=int(info[1]), host_syncs=int(info[2]), workspace_bytes=int(info[3]),
                  passes=int(info[4]), factorisations=int(info[5]), flops=float(info[6]), unconverged=int(info[7]))
        return res, d8

    def symmetric_orthonormalize(self, V: "Buffer", n, dim, v_row0=0):
        check(self.lib.rom_symmetric_orthonormalize(self.h, V.h, v_row0, n, dim))

    def complete_orthonormal(self, V: "Buffer", found, rest, dim, v_row0=0):
        check(self.lib.rom_complete_orthonormal(self.h, V.h, v_row0, found, rest, dim))

    def small_eig(self, A, mode=0, rel_tol=0.0, gram_like=True):
        A = _host(A)
        n = A.shape[0]
        lam, T = np.empty(n), np.empty((n, n))
        check(self.lib.rom_small_eig_host(self.h, n, A.ctypes.data, mode, rel_tol, int(gram_like), lam.ctypes.data,
                                          T.ctypes.data))
        return lam, T

    # -- RCCL ----------------------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        check(self.lib.rom_comm_unique_id(buf, 128))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, nranks: int):
        check(self.lib.rom_comm_init(self.h, uid, len(uid), rank, nranks))
        self.has_comm = True

    def comm_destroy(self):
        self.has_comm = False
        check(self.lib.rom_comm_destroy(self.h))

    def allgather(self, send: "Buffer", send_off, recv: "Buffer", recv_off, count):
        check(self.lib.rom_comm_allgather(self.h, send.h, send_off, recv.h, recv_off, count))

    def allgather_async(self, send: "Buffer", send_off, recv: "Buffer", recv_off, count, slot=0):
        check(self.lib.rom_comm_allgather_async(self.h, send.h, send_off, recv.h, recv_off, count, slot))

    def comm_wait_slot(self, slot):
        check(self.lib.rom_comm_wait_slot(self.h, slot))

    def comm_wait(self, host_sync=True):
        check(self.lib.rom_comm_wait(self.h, 1 if host_sync else 0))

    def allreduce_host(self, vals, op="sum") -> np.ndarray:
        v = _host(np.atleast_1d(vals)).copy()
        check(self.lib.rom_comm_allreduce_host(self.h, v.ctypes.data, v.size, 1 if op == "max" else 0))
        return v


def poly_terms(m: int, degree: int) -> np.ndarray:
    """rom_poly_terms: the (P, m) exponent rows of the feature space, PolynomialFeatures(degree).powers_ (host only)."""
    lib = load_library()
    P = C.c_int(0)
    check(lib.rom_poly_terms(int(m), int(degree), C.byref(P), None))
    powers = np.zeros((P.value, int(m)), dtype=np.int32)
    check(lib.rom_poly_terms(int(m), int(degree), C.byref(P), powers.ctypes.data))
    return powers


def _check_kmeans(status: int):
    """``check`` with the limits and NaN / Inf of rom_kmeans_* as ValueError (scikit-learn's estimators raise that)."""
    if status == ROM_ERR_INVALID:
        raise ValueError(last_error())
    check(status)


def kmeans_layout(r: int, kc: int) -> dict:
    """rom_kmeans_layout (host only; the single place of the limits and of the LDS carve-up of the fused kernel).  ValueError
    outside the limits."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    if lib.rom_kmeans_layout(int(r), int(kc), out.ctypes.data) != ROM_OK:
        raise ValueError(last_error())
    keys = ("r_padded", "kc_padded", "lds_bytes", "slab_rows", "r1_padded", "tile_stride", "partial_doubles", "tiles_per_wave")
    return {k: int(v) for k, v in zip(keys, out)}


def local_select_layout(n: int, k: int, rank: int, r: int) -> dict:
    """rom_local_select_layout (host only; the single place of the limits and of the LDS carve-up of the fit kernel).
    ValueError, naming the limit, outside them."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    if lib.rom_local_select_layout(int(n), int(k), int(rank), int(r), out.ctypes.data) != ROM_OK:
        raise ValueError(last_error())
    keys = ("lds_bytes", "row_doubles", "rank_max", "kc_max", "factor_offset", "b_offset", "gram_offset", "launches")
    return {k_: int(v) for k_, v in zip(keys, out)}


def sensor_dopt_layout(n: int, k: int) -> dict:
    """rom_sensor_dopt_layout (host only; the single place of the limits on n and k and of an entry's block in STATE):
    Z^T (kp rows of n_padded) | T (kp x kp) at ``t_offset`` | status at ``status_offset`` | s of the last update.  ``chunk``:
    entries of one chunk of the scoring pass.  ValueError, naming the limit, outside the limits."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    if lib.rom_sensor_dopt_layout(int(n), int(k), out.ctypes.data) != ROM_OK:
        raise ValueError(last_error())
    keys = ("kp", "n_padded", "entry", "chunk", "lds_bytes", "t_offset", "status_offset", "table")
    return {k_: int(v) for k_, v in zip(keys, out)}


MLP_ACTIVATIONS = {"tanh": 0, "logistic": 1, "sigmoid": 1, "relu": 2}


def mlp_layout(m: int, hidden, q: int) -> dict:
    """rom_mlp_layout (host only; the single place of the limits): P, the padded weight doubles, the LDS bytes of the two
    kernels and the offsets of every W_l (outputs x inputs, row-major) and b_l in the flat parameter vector -- all W in
    layer order, then all b.  ValueError outside the limits."""
    lib = load_library()
    hid = np.ascontiguousarray(list(hidden), dtype=np.int32)
    out, off = np.zeros(8, dtype=np.int64), np.zeros(2 * (len(hid) + 1), dtype=np.int64)
    if lib.rom_mlp_layout(int(m), int(len(hid)), hid.ctypes.data if len(hid) else None, int(q), out.ctypes.data, off.ctypes.data) != ROM_OK:
        raise ValueError(last_error())
    nl = len(hid) + 1
    return dict(P=int(out[0]), padded_weights=int(out[1]), lds_eval=int(out[2]), lds_predict=int(out[3]), layers=nl,
                partial=int(out[5]), n_weights=int(out[6]), w_offsets=[int(v) for v in off[:nl]],
                b_offsets=[int(v) for v in off[nl:]], sizes=[int(m)] + [int(v) for v in hid] + [int(q)])


def _pod_info(info) -> dict:
    """The info dict of the POD calls (rom_pod's eight doubles)."""
    keys = ("resolved_modes", "completed_modes", "gram_passes", "sketch_passes")
    d = {k: int(info[i]) for i, k in enumerate(keys)}
    d.update(executed_flops=float(info[4]), useful_flops=float(info[5]), subspace_iterations=int(info[6]),
             stop_reason=("filled", "floor", "budget")[int(info[7])])
    return d


D2H_BYTES = [0]  # bytes copied from device buffers to the host through Buffer.download (tests assert on it)


class Buffer:
    """fp64 device buffer owned by the library; freed on garbage collection."""

    def __init__(self, ctx: Context, n: int):
        self.ctx = ctx
        self.n = int(n)
        h = _vp()
        check(ctx.lib.rom_buf_alloc(ctx.h, self.n, C.byref(h)))
        self.h = h

    def upload(self, arr, offset=0):
        arr = _host(arr)
        check(self.ctx.lib.rom_buf_upload(self.h, offset, arr.ctypes.data, arr.size))
        return self

    def download(self, n=None, offset=0, shape=None) -> np.ndarray:
        n = self.n - offset if n is None else int(n)
        D2H_BYTES[0] += 8 * n
        out = _pinned_array(self.ctx.lib, n) if n * 8 >= PINNED_DOWNLOAD_BYTES else None
        if out is None:
            out = np.empty(n, dtype=np.float64)
        check(self.ctx.lib.rom_buf_download(self.h, offset, out.ctypes.data, n))
        return out.reshape(shape) if shape is not None else out

    def fill(self, value=0.0, offset=0, n=None):
        check(self.ctx.lib.rom_buf_fill(self.h, offset, self.n - offset if n is None else n, float(value)))
        return self

    def copy_from(self, src: "Buffer", n, dst_off=0, src_off=0):
        check(self.ctx.lib.rom_buf_copy(self.h, dst_off, src.h, src_off, n))
        return self

    def same_bits_as(self, other: "Buffer", n, off=0, other_off=0) -> bool:
        eq = C.c_int(0)
        check(self.ctx.lib.rom_buf_equal(self.h, off, other.h, other_off, n, C.byref(eq)))
        return bool(eq.value)

    def gather_rows_from(self, src: "Buffer", rows, dim):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        check(self.ctx.lib.rom_buf_gather_rows(self.h, src.h, rows.ctypes.data, rows.size, dim))
        return self

    def scale(self, alpha, offset=0, n=None):
        check(self.ctx.lib.rom_buf_scale(self.h, offset, self.n - offset if n is None else n, float(alpha)))
        return self

    def free(self):
        if getattr(self, "h", None) is not None and self.h:
            self.ctx.lib.rom_buf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _MapHandle:
    """What the handles of the fitted maps share.  A subclass names the prefix of its symbols (``<prefix>_predict``, ``_query``,
    ``_destroy``) and the keys of its eight query words; its constructor sets ``ctx``, ``h`` (None until the fit has returned)
    and ``q``."""

    _PREFIX = ""
    _QUERY_KEYS = ()
    h = None

    def _fn(self, name):
        return getattr(self.ctx.lib, f"{self._PREFIX}_{name}")

    def query(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        check(self._fn("query")(self.h, out.ctypes.data))
        return {k: int(v) for k, v in zip(self._QUERY_KEYS, out)}

    def predict(self, X: Buffer, x_off, ldx, M, OUT: "Buffer | None" = None, o_off=0, ldo=None, Yref: "Buffer | None" = None, r_off=0,
                ldr=None, sumsq=False):
        """rom_poly_predict / rom_mlp_predict / rom_tree_predict: OUT <- the prediction for the M rows of X, or Yref -
        prediction; with ``sumsq`` returns the q column sums of squares of that (OUT may then be None: nothing of size M x q is
        written)."""
        ss = np.zeros(self.q) if sumsq else None
        check(self._fn("predict")(self.h, X.h if X is not None else None, int(x_off), int(ldx), int(M),
                                  OUT.h if OUT is not None else None, int(o_off), int(self.q if ldo is None else ldo),
                                  Yref.h if Yref is not None else None, int(r_off), int(self.q if ldr is None else ldr),
                                  ss.ctypes.data if sumsq else None))
        return ss

    def free(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PolyMap(_MapHandle):
    """Handle of a fitted polynomial map (rom_poly_*): owns the device coefficients, destroyed on collection."""

    _PREFIX = "rom_poly"
    _QUERY_KEYS = ("m", "d", "P", "q", "rank", "M_train", "passes", "host_syncs")
    _PARTS = {"c": 0, "h": 1, "W": 2, "dropped": 3}

    def __init__(self, ctx: Context, X: Buffer, x_off, ldx, m, Y: Buffer, y_off, ldy, q, M, degree, rcond=0.0):
        self.ctx = ctx
        self.h = None
        h, info = _vp(), np.zeros(8)
        check(ctx.lib.rom_poly_fit(ctx.h, X.h if X is not None else None, int(x_off), int(ldx), int(m),
                                   Y.h if Y is not None else None, int(y_off), int(ldy), int(q), int(M), int(degree), float(rcond),
                                   C.byref(h), info.ctypes.data))
        self.h = h
        self.m, self.q, self.degree = int(m), int(q), int(degree)
        self.info = dict(P=int(info[0]), rank=int(info[1]), passes=int(info[2]), delta_max=float(info[3]),
                         pivot_ratio=float(info[4]), executed_flops=float(info[5]), host_syncs=int(info[6]),
                         stop_reason=("full_rank", "terms_dropped", "budget")[int(info[7])])

    def download(self, part: str) -> np.ndarray:
        """Host copy of "c" (m,), "h" (m,), "W" (q, P) or the "dropped" flags (P,)."""
        P = self.info["P"]
        out = np.zeros({"c": (self.m,), "h": (self.m,), "W": (self.q, P), "dropped": (P,)}[part])
        check(self.ctx.lib.rom_poly_download(self.h, self._PARTS[part], out.ctypes.data, out.size))
        return out


class MLPHandle(_MapHandle):
    """Handle of a fitted MLP map (rom_mlp_*): owns the device weights and scalings, destroyed on collection."""

    _PREFIX = "rom_mlp"
    _QUERY_KEYS = ("m", "q", "hidden_layers", "P", "M_train", "iterations", "launches", "host_syncs")
    _PARTS = {"w": 0, "c": 1, "h": 2, "y_mean": 3, "y_scale": 4, "loss_curve": 5}
    _STOPS = ("gradient", "stagnation", "budget", "line_search")

    def __init__(self, ctx: Context, X: Buffer, x_off, ldx, m, Y: Buffer, y_off, ldy, q, M, hidden, w0, activation="tanh", alpha=1e-4,
                 scale_targets=True, max_iter=200, tol=1e-6, memory=10):
        self.ctx = ctx
        self.h = None
        self.layout = mlp_layout(m, hidden, q)          # (ValueError outside the limits, before any device call)
        if activation not in MLP_ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(MLP_ACTIVATIONS)}")
        w0 = _host(np.asarray(w0, dtype=np.float64).ravel())
        if w0.size != self.layout["P"]:
            raise ValueError(f"w0 holds {w0.size} parameters, the layout {self.layout['P']}")
        hid = np.ascontiguousarray(list(hidden), dtype=np.int32)
        h, info = _vp(), np.zeros(8)
        try:
            check(ctx.lib.rom_mlp_fit(ctx.h, X.h if X is not None else None, int(x_off), int(ldx), int(m),
                                      Y.h if Y is not None else None, int(y_off), int(ldy), int(q), int(M), len(hid), hid.ctypes.data,
                                      MLP_ACTIVATIONS[activation], float(alpha), 1 if scale_targets else 0, w0.ctypes.data,
                                      int(max_iter), float(tol), int(memory), C.byref(h), info.ctypes.data))
        except RomLibraryError as e:
            if "NaN / Inf" in str(e):   # (scikit-learn's estimators raise ValueError on such input)
                raise ValueError(str(e)) from None
            raise
        self.h = h
        self.m, self.q, self.P = int(m), int(q), self.layout["P"]
        self.activation, self.alpha = ("logistic" if activation == "sigmoid" else activation), float(alpha)
        self.info = dict(iterations=int(info[0]), evaluations=int(info[1]), loss=float(info[2]), grad_inf=float(info[3]),
                         stop_reason=self._STOPS[int(info[4])], launches=int(info[5]), host_syncs=int(info[6]),
                         executed_flops=float(info[7]))

    def download(self, part: str) -> np.ndarray:
        """Host copy of "w" (P,), "c", "h" (m,), "y_mean", "y_scale" (q,) or the "loss_curve" (iterations + 1,)."""
        n = {"w": self.P, "c": self.m, "h": self.m, "y_mean": self.q, "y_scale": self.q, "loss_curve": self.info["iterations"] + 1}[part]
        out = np.zeros(n)
        check(self.ctx.lib.rom_mlp_download(self.h, self._PARTS[part], out.ctypes.data, out.size))
        return out

    def weights(self):
        """(coefs, intercepts) in scikit-learn's shapes, (fan_in, fan_out) and (fan_out,), in scaled coordinates."""
        w, sz, lay = self.download("w"), self.layout["sizes"], self.layout
        coefs = [w[o:o + sz[l + 1] * sz[l]].reshape(sz[l + 1], sz[l]).T.copy() for l, o in enumerate(lay["w_offsets"])]
        return coefs, [w[o:o + sz[l + 1]].copy() for l, o in enumerate(lay["b_offsets"])]

    def loss_grad(self, X: Buffer, x_off, ldx, Y: Buffer, y_off, ldy, M, alpha=None):
        """rom_mlp_loss_grad: (L, its gradient (P,)) at the handle's weights on M rows of X and Y, the handle's scalings."""
        loss, grad = np.zeros(1), np.zeros(self.P)
        check(self.ctx.lib.rom_mlp_loss_grad(self.h, X.h if X is not None else None, int(x_off), int(ldx),
                                             Y.h if Y is not None else None, int(y_off), int(ldy), int(M),
                                             float(self.alpha if alpha is None else alpha), loss.ctypes.data, grad.ctypes.data))
        return float(loss[0]), grad


class TreeMapHandle(_MapHandle):
    """Handle of a fitted tree / forest (rom_tree_*): owns the device node arrays, destroyed on collection."""

    _PREFIX = "rom_tree"
    _QUERY_KEYS = ("m", "q", "T", "M_train", "nodes", "deepest_level", "launches", "host_syncs")
    _PARTS = ("first", "feature", "threshold", "left", "count", "value")

    def __init__(self, ctx: Context, X: Buffer, x_off, ldx, m, Y: Buffer, y_off, ldy, q, M, T=1, counts=None, max_depth=None,
                 min_samples_split=2, min_samples_leaf=1):
        self.ctx = ctx
        self.h = None
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(counts, dtype=np.int32)
            assert cnt.shape == (int(T), int(M)), f"tree_fit: counts of shape {cnt.shape}, expected ({T}, {M})"
        h, info = _vp(), np.zeros(8)
        check(ctx.lib.rom_tree_fit(ctx.h, X.h if X is not None else None, int(x_off), int(ldx), int(m),
                                   Y.h if Y is not None else None, int(y_off), int(ldy), int(q), int(M), int(T),
                                   cnt.ctypes.data if cnt is not None else None, int(max_depth or 0), int(min_samples_split),
                                   int(min_samples_leaf), C.byref(h), info.ctypes.data))
        self.h = h
        self.m, self.q, self.T = int(m), int(q), int(T)
        self.info = dict(nodes=int(info[0]), leaves=int(info[1]), deepest_level=int(info[2]), levels=int(info[3]),
                         launches=int(info[4]), host_syncs=int(info[5]), workspace_bytes=int(info[6]))

    def nodes(self) -> dict:
        """Host copies of the node arrays, the trees one after the other (tree t: nodes first[t] .. first[t + 1] - 1, breadth
        first): "first" (T + 1,), "feature" (-1 at a leaf), "threshold", "left" (the right child is left + 1; -1 at a leaf),
        "count" (weighted), "value" (nodes, q)."""
        n = self.info["nodes"]
        out = {}
        for what, part in enumerate(self._PARTS):
            a = np.zeros(self.T + 1 if what == 0 else n * self.q if what == 5 else n)
            check(self.ctx.lib.rom_tree_download(self.h, what, a.ctypes.data, a.size))
            out[part] = a.reshape(n, self.q) if what == 5 else a if what in (2, 4) else a.astype(np.int64)
        return out


class KMeansHandle:
    """Handle of a fitted k-means (rom_kmeans_*): owns the device centroids, shift and training labels, destroyed on
    collection."""

    _QUERY_KEYS = ("r", "kc", "M_train", "iterations", "converged", "stop_reason", "launches", "host_syncs")
    _PARTS = {"centroids": 0, "counts": 1, "inertia": 2, "shift": 3, "labels": 4}
    h = None

    def __init__(self, ctx: Context, X: Buffer, x_off, ldx, r, M, kc, init, max_iter=50, tol=0.0, mode=0):
        self.ctx = ctx
        self.h = None
        self.layout = kmeans_layout(r, kc)              # (ValueError outside the limits, before any device call)
        init = _host(np.asarray(init, dtype=np.float64))
        if init.shape != (int(kc), int(r)):
            raise ValueError(f"kmeans_fit: initial centroids of shape {init.shape}, expected ({kc}, {r})")
        h, info = _vp(), np.zeros(8)
        _check_kmeans(ctx.lib.rom_kmeans_fit(ctx.h, X.h if X is not None else None, int(x_off), int(ldx), int(r), int(M), int(kc),
                                             init.ctypes.data, int(max_iter), float(tol), int(mode), C.byref(h), info.ctypes.data))
        self.h = h
        self.r, self.kc, self.M = int(r), int(kc), int(M)
        self.info = dict(iterations=int(info[0]), converged=bool(info[1]), launches=int(info[2]), host_syncs=int(info[3]),
                         workspace_bytes=int(info[4]), chunks=int(info[5]), rows_rescored_more=int(info[6]),
                         executed_flops=float(info[7]))

    def query(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        check(self.ctx.lib.rom_kmeans_query(self.h, out.ctypes.data))
        return {k: int(v) for k, v in zip(self._QUERY_KEYS, out)}

    def download(self, part: str) -> np.ndarray:
        """Host copy of "centroids" (kc, r), "counts" (kc,) int64, "inertia" (iterations + 1,: of the assignment of every
        iteration, then of the final one), "shift" (r,) or the "labels" of the training rows (M,) int32."""
        it = self.info["iterations"]
        shape = {"centroids": (self.kc, self.r), "counts": (self.kc,), "inertia": (it + 1,), "shift": (self.r,), "labels": (self.M,)}[part]
        out = np.zeros(shape)
        check(self.ctx.lib.rom_kmeans_download(self.h, self._PARTS[part], out.ctypes.data, out.size))
        return out.astype(np.int64) if part == "counts" else out.astype(np.int32) if part == "labels" else out

    def assign(self, X: Buffer, x_off, ldx, M, mode=0, dist2=True):
        labels = np.zeros(int(M), dtype=np.int32)
        d2 = np.zeros(int(M)) if dist2 else None
        inertia = np.zeros(1)
        _check_kmeans(self.ctx.lib.rom_kmeans_assign(self.h, X.h if X is not None else None, int(x_off), int(ldx), int(M), int(mode),
                                                     labels.ctypes.data, d2.ctypes.data if dist2 else None, inertia.ctypes.data))
        return labels, d2, float(inertia[0])

    def free(self):
        if self.h:
            self.ctx.lib.rom_kmeans_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_contexts = {}


def get_context(device: int | None = None) -> Context:
    if device is None:
        device = int(os.environ.get("ROMHC_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


class Fem:
    """Handle of one FE space (blocks_geometry, N) on the device."""

    def __init__(self, ctx: Context, nrb: int, ncb: int, N: int):
        self.ctx = ctx
        h = _vp()
        check(ctx.lib.rom_fem_create(ctx.h, nrb, ncb, N, C.byref(h)))
        self.h = h
        nr, nc, ng, nt = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        dim = C.c_int64(0)
        check(ctx.lib.rom_fem_dims(h, C.byref(nr), C.byref(nc), C.byref(dim), C.byref(ng), C.byref(nt)))
        self.nr, self.nc, self.dim, self.n_interface, self.n_tiles = nr.value, nc.value, dim.value, ng.value, nt.value
        self.nrb, self.ncb, self.N, self.kblk = nrb, ncb, N, nrb * ncb

    def load_vector(self) -> np.ndarray:
        B = np.empty(self.dim)
        check(self.ctx.lib.rom_fem_load_vector_host(self.h, B.ctypes.data))
        return B

    def solve_batch(self, a: Buffer, M: int, U: Buffer, row0: int = 0, wait: bool = True):
        """wait=False only enqueues the sweep; call Context.solve_status() before trusting the rows."""
        fn = self.ctx.lib.rom_solve_batch if wait else self.ctx.lib.rom_solve_batch_async
        check(fn(self.h, a.h, M, U.h, row0))

    @property
    def reduced_stride(self) -> int:
        """doubles per system of the interface vector (what solve_reduced writes and expand reads)"""
        v = C.c_int64(0)
        check(self.ctx.lib.rom_fem_reduced_stride(self.h, C.byref(v)))
        return v.value

    @property
    def expansion_is_linear(self) -> bool:
        """True if expand() is a linear map of the interface vectors (U = Y B^T, `a` ignored)."""
        v = C.c_int(0)
        check(self.ctx.lib.rom_fem_expansion_is_linear(self.h, C.byref(v)))
        return bool(v.value)

    @property
    def reduced_inputs(self) -> np.ndarray:
        """positions of an interface vector that the expansion reads (the nodal edge blocks are its outputs)"""
        b, e = C.c_int64(0), C.c_int64(0)
        check(self.ctx.lib.rom_fem_reduced_layout(self.h, C.byref(b), C.byref(e)))
        return np.concatenate((np.arange(0, b.value), np.arange(e.value, self.reduced_stride)))

    @property
    def compact_stride(self) -> int:
        """doubles per system of the COMPACT interface vector (the entries the expansion reads: what travels between ranks)"""
        v = C.c_int64(0)
        check(self.ctx.lib.rom_fem_compact_stride(self.h, C.byref(v)))
        return v.value

    def pack_reduced(self, Y: Buffer, M: int, Yc: Buffer, y_row0: int = 0, c_row0: int = 0):
        """Yc[c_row0:c_row0+M] = the compact form of the interface vectors Y[y_row0:y_row0+M] (enqueued only)."""
        check(self.ctx.lib.rom_fem_pack_reduced_async(self.h, Y.h, y_row0, M, Yc.h, c_row0))

    def unpack_reduced(self, Yc: Buffer, M: int, Y: Buffer, c_row0: int = 0, y_row0: int = 0):
        """The inverse of pack_reduced: full-stride vectors with a zero nodal part (expand() fills it) (enqueued only)."""
        check(self.ctx.lib.rom_fem_unpack_reduced_async(self.h, Yc.h, c_row0, M, Y.h, y_row0))

    def allgather_packed_async(self, Y: Buffer, M: int, send: Buffer, recv: Buffer, recv_off: int = 0, slot: int = 0,
                               y_row0: int = 0):
        """Pack the M interface vectors Y[y_row0:] into `send` and all-gather them into `recv`, both on the
        communication stream (the compute stream is not blocked); slots as Context.allgather_async."""
        check(self.ctx.lib.rom_comm_allgather_packed_async(self.h, Y.h, y_row0, M, send.h, recv.h, recv_off, slot))

    def solve_reduced(self, a: Buffer, M: int, Y: Buffer, y_row0: int = 0):
        """Stage 1 of the sweep (enqueued only): interface vectors of the M systems into Y[y_row0:y_row0+M]."""
        check(self.ctx.lib.rom_solve_reduced_async(self.h, a.h, M, Y.h, y_row0))

    def expand(self, a: Buffer, M: int, Y: Buffer, U: Buffer, y_row0: int = 0, row0: int = 0):
        """Stage 2 (enqueued only): snapshot rows U[row0:row0+M] from the interface vectors Y[y_row0:y_row0+M]."""
        check(self.ctx.lib.rom_expand_batch_async(self.h, a.h, M, Y.h, y_row0, U.h, row0))

    def solve_work(self):
        v = [C.c_double(0) for _ in range(4)]
        check(self.ctx.lib.rom_solve_work(self.h, *[C.byref(x) for x in v]))
        return dict(flops_own=v[0].value, bytes_own=v[1].value, flops_banded=v[2].value, bytes_banded=v[3].value)

    def assemble_batch(self, a: Buffer, M: int, diag: Buffer, east: Buffer, north: Buffer):
        check(self.ctx.lib.rom_assemble_batch(self.h, a.h, M, diag.h, east.h, north.h))

    def stencil_apply(self, X: Buffer, K: int, Y: Buffer, a_one=None, x_row0=0, y_row0=0):
        if a_one is None:
            check(self.ctx.lib.rom_stencil_apply(self.h, None, 1, X.h, x_row0, K, Y.h, y_row0))
        else:
            a_one = _host(a_one)
            assert a_one.size == self.kblk
            check(self.ctx.lib.rom_stencil_apply(self.h, a_one.ctypes.data, 0, X.h, x_row0, K, Y.h, y_row0))

    def h10norm(self, U: Buffer, K: int, u_row0=0, V: Buffer | None = None, v_row0=0) -> np.ndarray:
        out = np.empty(K)
        check(self.ctx.lib.rom_h10norm(self.h, U.h, u_row0, V.h if V is not None else None, v_row0, K,
                                       out.ctypes.data))
        return out

    def project_h10(self, U: Buffer, M: int, Cb: Buffer | None, n: int, OUT: Buffer, u_row0=0, c_row0=0, out_row0=0):
        check(self.ctx.lib.rom_project_h10(self.h, U.h, u_row0, M, Cb.h if Cb is not None else None, c_row0, n, OUT.h,
                                           out_row0))

    def galerkin_rom(self, a: Buffer, M: int, Cb: Buffer | None, n: int, OUT: Buffer, c_row0=0, out_row0=0):
        check(self.ctx.lib.rom_galerkin_rom(self.h, a.h, M, Cb.h if Cb is not None else None, c_row0, n, OUT.h, out_row0))

    def greedy(self, U: Buffer, M: int, a: Buffer | None, h1norm, galerkin: bool, n: int, u_row0=0):
        """rom_greedy: (picks list, max relative errors list)."""
        h1 = _host(np.broadcast_to(np.asarray(h1norm, dtype=np.float64), (M,)))
        picks, errs = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1))
        check(self.ctx.lib.rom_greedy(self.h, U.h, u_row0, M, a.h if a is not None else None, h1.ctypes.data,
                                      1 if galerkin else 0, n, picks.ctypes.data, errs.ctypes.data))
        return [int(p) for p in picks[:n]], [float(e) for e in errs[:n]]

    def error_curves(self, U: Buffer, M: int, C: Buffer | None, N: int, a: Buffer | None = None, u_row0=0, c_row0=0):
        """rom_error_curves: H^1_0 errors of the projection (and, with parameters ``a``, of the Galerkin ROM) onto the
        nested spans of C[c_row0 .. +N) for every n = 0 .. N, over the snapshots U[u_row0 .. +M).  Returns NumPy arrays
        (proj (N+1, M), galerkin (N+1, M) or None, P (M, N), T (N, N), info dict)."""
        curves = 2 if a is not None else 1
        ERR = self.ctx.alloc(max(curves * (N + 1) * M, 1))
        Pb = self.ctx.alloc(max(M * N, 1))
        Tb = self.ctx.alloc(max(N * N, 1))
        info = np.zeros(4)
        check(self.ctx.lib.rom_error_curves(self.h, U.h, u_row0, M, C.h if C is not None else None, c_row0, N,
                                            a.h if a is not None else None, ERR.h, Pb.h, Tb.h, info.ctypes.data))
        err = ERR.download(curves * (N + 1) * M, shape=(curves, N + 1, M)) if M else np.zeros((curves, N + 1, 0))
        P = Pb.download(M * N, shape=(M, N)) if M * N else np.zeros((M, N))
        T = Tb.download(N * N, shape=(N, N)) if N else np.zeros((0, 0))
        routes = {-1: None, 0: "lds", 1: "global"}
        inf = {"dependent_rows": int(info[0]), "galerkin_route": routes[int(info[1])], "passes": int(info[2]),
               "edge_tiles": int(info[3])}
        return err[0], (err[1] if a is not None else None), P, T, inf

    # -- basis stage on compact interface vectors (factored snapshot blocks: rom_factored.hip) --------------
    def energy_map(self, parts=7):
        """rom_fem_energy_map: build / cache the geometry of the snapshots in interface-vector coordinates (1: H^1_0,
        2: Galerkin forms, 4: Euclidean; 1 keeps the way back from its coordinates).  Returns the ranks (k_h10, k_l2)."""
        k1, k2 = C.c_int(0), C.c_int(0)
        check(self.ctx.lib.rom_fem_energy_map(self.h, int(parts), C.byref(k1), C.byref(k2)))
        return k1.value, k2.value

    def h10norm_factored(self, Yc: Buffer, M: int, c_row0=0) -> np.ndarray:
        out = np.empty(max(M, 1))
        check(self.ctx.lib.rom_h10norm_factored(self.h, Yc.h, c_row0, M, out.ctypes.data))
        return out[:M]

    def greedy_factored(self, Yc: Buffer, M: int, a: Buffer | None, h1norm, galerkin: bool, n: int, c_row0=0):
        """rom_greedy_factored: (picks list, max relative errors list)."""
        h1 = _host(np.broadcast_to(np.asarray(h1norm, dtype=np.float64), (M,)))
        picks, errs = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1))
        check(self.ctx.lib.rom_greedy_factored(self.h, Yc.h, c_row0, M, a.h if a is not None else None, h1.ctypes.data,
                                               1 if galerkin else 0, n, picks.ctypes.data, errs.ctypes.data))
        return [int(p) for p in picks[:n]], [float(e) for e in errs[:n]]

    def pod_factored(self, Yc: Buffer, M: int, n: int, V: Buffer, center=True, c_row0=0, v_row0=0):
        """rom_pod_factored: modes as rows into V.  Returns (sigma (n,), info dict)."""
        sigma, info = np.zeros(max(n, 1)), np.zeros(8)
        check(self.ctx.lib.rom_pod_factored(self.h, Yc.h, c_row0, M, n, 1 if center else 0, V.h, v_row0, sigma.ctypes.data,
                                            info.ctypes.data))
        keys = ("resolved_modes", "completed_modes", "gram_passes", "sketch_passes")
        d = {k: int(info[i]) for i, k in enumerate(keys)}
        d.update(executed_flops=float(info[4]), subspace_iterations=int(info[6]), stop_reason=("filled", "floor", "budget")[int(info[7])])
        return sigma[:n], d

    # -- the H^1_0 inner product in spectral form (rom_spectral.hip) ------------------------------------------
    def sine_transform(self, X: Buffer, K: int, OUT: Buffer, pre=0, post=0, x_row0=0, out_row0=0):
        """rom_sine_transform: OUT[k] = Lambda^(post/2) o (S_r (Lambda^(pre/2) o X[k]) S_c) for K rows; X is not modified.
        (pre, post) = (0, 1): H^1_0 -> Euclidean coordinates, (-1, 0): the way back."""
        check(self.ctx.lib.rom_sine_transform(self.h, X.h, x_row0, K, int(pre), int(post), OUT.h, out_row0))

    def pod_h10(self, X: Buffer, M: int, n: int, V: Buffer, center=True, x_row0=0, v_row0=0, rel_floor=0.0):
        """rom_pod_h10: POD in the H^1_0 inner product; X is NOT modified.  Returns (sigma (n,), info dict as Context.pod)."""
        sigma, info = np.zeros(max(n, 1)), np.zeros(8)
        check(self.ctx.lib.rom_pod_h10(self.h, X.h, x_row0, M, n, 1 if center else 0, float(rel_floor), V.h, v_row0,
                                       sigma.ctypes.data, info.ctypes.data))
        return sigma[:n], _pod_info(info)

    def pod_h10_factored(self, Yc: Buffer, M: int, n: int, V: Buffer, center=True, c_row0=0, v_row0=0):
        """rom_pod_h10_factored: the same from compact interface vectors, modes as rows into V.  Returns (sigma (n,), info
        dict as Context.pod)."""
        sigma, info = np.zeros(max(n, 1)), np.zeros(8)
        check(self.ctx.lib.rom_pod_h10_factored(self.h, Yc.h, c_row0, M, n, 1 if center else 0, V.h, v_row0,
                                                sigma.ctypes.data, info.ctypes.data))
        return sigma[:n], _pod_info(info)

    def evaluate_points(self, U: Buffer, K: int, ix, iy, tx, ty, row0=0) -> np.ndarray:
        ix = np.ascontiguousarray(ix, dtype=np.int32)
        iy = np.ascontiguousarray(iy, dtype=np.int32)
        tx, ty = _host(tx), _host(ty)
        out = np.empty((K, ix.size))
        check(self.ctx.lib.rom_evaluate_points(self.h, U.h, row0, K, ix.size, ix.ctypes.data, iy.ctypes.data,
                                               tx.ctypes.data, ty.ctypes.data, out.ctypes.data))
        return out

    def riesz_h10(self, ix, iy, tx, ty, OMEGA: Buffer | None = None, row0=0, gram=True):
        """rom_riesz_h10: H^1_0 Riesz representers of the point evaluations (ix, iy, tx, ty as for evaluate_points) into
        the rows OMEGA[row0 ...] when OMEGA is given; returns their Gram matrix G (npts, npts) if ``gram``, else None."""
        ix = np.ascontiguousarray(ix, dtype=np.int32)
        iy = np.ascontiguousarray(iy, dtype=np.int32)
        tx, ty = _host(tx), _host(ty)
        m = ix.size
        G = np.empty((m, m)) if gram else None
        check(self.ctx.lib.rom_riesz_h10(self.h, m, ix.ctypes.data, iy.ctypes.data, tx.ctypes.data, ty.ctypes.data,
                                         OMEGA.h if OMEGA is not None else None, row0,
                                         G.ctypes.data if gram and m else None))
        return G

    def riesz_norms_h10(self, ix, iy, tx, ty) -> np.ndarray:
        """rom_riesz_norms_h10: ||omega_i||^2_{H^1_0} = r_i^T A_1^-1 r_i of the point evaluations (as for evaluate_points)."""
        ix = np.ascontiguousarray(ix, dtype=np.int32)
        iy = np.ascontiguousarray(iy, dtype=np.int32)
        tx, ty = _host(tx), _host(ty)
        out = np.empty(ix.size)
        check(self.ctx.lib.rom_riesz_norms_h10(self.h, ix.size, ix.ctypes.data, iy.ctypes.data, tx.ctypes.data,
                                               ty.ctypes.data, out.ctypes.data if ix.size else None))
        return out

    def sensor_greedy(self, Cb: Buffer, n: int, ix, iy, tx, ty, m: int, mode: int, rel_tol: float, c_row0=0):
        """rom_sensor_greedy: greedy selection of up to m of the candidate points for PBDW on span C[c_row0 .. +n).
        Returns (picks (m,) int64, -1 past a stop; crit (m,); A (m, n); alpha (m, n) in mode 1 else None; info dict)."""
        ix = np.ascontiguousarray(ix, dtype=np.int32)
        iy = np.ascontiguousarray(iy, dtype=np.int32)
        tx, ty = _host(tx), _host(ty)
        picks, crit = np.zeros(max(m, 1), dtype=np.int64), np.zeros(max(m, 1))
        A = np.zeros((max(m, 1), max(n, 1)))
        alpha = np.zeros((max(m, 1), max(n, 1))) if mode == 1 else None
        info = np.zeros(4)
        check(self.ctx.lib.rom_sensor_greedy(self.h, Cb.h if Cb is not None else None, c_row0, n, ix.size, ix.ctypes.data,
                                             iy.ctypes.data, tx.ctypes.data, ty.ctypes.data, m, mode, float(rel_tol),
                                             picks.ctypes.data, crit.ctypes.data, A.ctypes.data,
                                             alpha.ctypes.data if alpha is not None else None, info.ctypes.data))
        inf = {"dead_rows": int(info[0]), "picks": int(info[1]), "stop_reason": int(info[2]), "host_syncs": int(info[3])}
        return picks[:m], crit[:m], A[:m, :n], (alpha[:m, :n] if alpha is not None else None), inf

    # -- residual error bounds and the weak greedy (rom_resid.hip) ---------------------------------------------
    def resid(self, n_cap: int) -> "Resid":
        """rom_resid_create: an empty residual estimator for at most n_cap basis rows."""
        return Resid(self, n_cap)

    def weak_greedy(self, a: Buffer, M: int, n_max: int, resid: "Resid", BASIS: Buffer, weights: Buffer | None = None,
                    rel_tol=0.0, basis_row0=0):
        """rom_weak_greedy on a fresh estimator: (picks list, criteria list, info dict); the snapshots of the picks are
        the rows BASIS[basis_row0 ...] and ``resid`` holds the estimator of the basis built."""
        picks, crit = np.zeros(max(n_max, 1), dtype=np.int64), np.zeros(max(n_max, 1))
        info = np.zeros(6)
        check(self.ctx.lib.rom_weak_greedy(self.h, a.h, M, weights.h if weights is not None else None, n_max, float(rel_tol),
                                           resid.h, BASIS.h, basis_row0, picks.ctypes.data, crit.ctypes.data,
                                           info.ctypes.data))
        made = int(info[0])
        inf = {"picks": made, "dead_rows": int(info[1]), "stop_reason": ("n_max", "rel_tol", "exhausted")[int(info[2])],
               "rank": int(info[3]), "host_syncs": int(info[4]), "last_criterion": float(info[5])}
        return [int(p) for p in picks[:made]], [float(c) for c in crit[:made]], inf

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.ctx.lib.rom_fem_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Resid:
    """Handle of a residual estimator (rom_resid_*): the offline state of the bound ||r(a)||_{H^-1} of a Galerkin ROM."""

    _PARTS = {"R": 0, "Q": 1, "Ahat": 2, "bhat": 3, "W": 4, "ranks": 5, "dead": 6}

    def __init__(self, fem: Fem, n_cap: int):
        self.fem, self.ctx = fem, fem.ctx
        h = _vp()
        check(self.ctx.lib.rom_resid_create(fem.h, int(n_cap), C.byref(h)))
        self.h = h

    def append(self, Cb: Buffer, rows: int, c_row0=0):
        check(self.ctx.lib.rom_resid_append(self.h, Cb.h, c_row0, rows))
        return self

    def query(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        check(self.ctx.lib.rom_resid_query(self.h, out.ctypes.data))
        keys = ("n", "n_live", "P", "rank", "n_cap", "k", "dim", "host_syncs")
        return {k: int(v) for k, v in zip(keys, out)}

    def download(self, part: str) -> np.ndarray:
        """Host copy of "R" (rank, P), "Q" (rank, dim), "Ahat" (k, n, n), "bhat" (n,), "W" (n, dim), "ranks" (n + 1,)
        or "dead" (n,)."""
        q = self.query()
        n, k, dim, rank, P = q["n"], q["k"], q["dim"], q["rank"], q["P"]
        shape = {"R": (rank, P), "Q": (rank, dim), "Ahat": (k, n, n), "bhat": (n,), "W": (n, dim), "ranks": (n + 1,),
                 "dead": (n,)}[part]
        out = np.zeros(shape)
        check(self.ctx.lib.rom_resid_download(self.h, self._PARTS[part], out.ctypes.data if out.size else None, out.size))
        return out

    def basis(self, OUT: Buffer, out_row0=0):
        """OUT[out_row0 ...] = W (n rows): u_n = c W with the coefficients of ``eval``."""
        check(self.ctx.lib.rom_resid_basis(self.h, OUT.h, out_row0))

    def eval(self, a: Buffer, M: int, n: int, DELTA: Buffer, weights: Buffer | None = None, COEF: Buffer | None = None,
             a_row0=0, d_off=0, coef_row0=0):
        """rom_resid_eval: DELTA[d_off + m] = weights[m] ||r(a_m)||_{H^-1} on the nested basis of the first n rows."""
        check(self.ctx.lib.rom_resid_eval(self.h, a.h, a_row0, M, n, weights.h if weights is not None else None, DELTA.h,
                                          d_off, COEF.h if COEF is not None else None, coef_row0))

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.rom_resid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
