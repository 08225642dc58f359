"""ts-pws_amd -- MI355X-native time-scale phase-weighted stack (ts-PWS).

The product is the C-ABI shared library ``lib/libtspws_hip.so`` (hand-written
gfx950 HIP kernels + the C host entry point ``tspws_main``; headers in
``include/``).  This module is only the Python-side binding used by the tests
and ``bench.py``: ctypes signatures, a ``Plan`` wrapper, and helpers that run
the device-resident path on torch-allocated HBM buffers (torch provides device
memory, streams and torch.distributed -- plumbing, not compute).

There is no CPU fallback anywhere: if the library is missing or no HIP device
is present the calls raise.

Import with ``importlib.import_module("ts-pws_amd")`` (the directory name is
not a Python identifier).

Every argument check exists once; a new batched call takes them from here
rather than from a sibling method.  Module level: ``_offsets`` (``first`` ->
uint64 offsets, B, T), ``_host_array`` (numpy array of dtype and shape:
``mtr_out``, ``mtr``), ``_score_plane`` (``score`` -> float64 [T]).  On
``Plan``: ``_traces`` (the trace rows), ``_need`` (contiguous tensor of a dtype
on the plan's device, of a shape or of at least so many elements; ``_out`` and
``_refs`` are its pointer-returning forms), ``_rows_out`` (``ls_out`` /
``ts_out`` / ``mtr_out``, given or new), ``_sel`` (selections and masks),
``_coef_sets`` (``Y``), ``_strided_rows`` ([B][M][N] views of a wider base),
``_strided_refs`` ([B][N] reference rows likewise), ``_window``, ``_windows``
(the (n0, n1) table), ``_ftan_tables`` (the per-ensemble windows, noise ranges
and scale range of the group-arrival calls) and ``_stats`` (the ``*_stats()``
dicts).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("TSPWS_LIB_PATH") or os.path.join(_HERE, "lib", "libtspws_hip.so")  # override: profiling builds only

time_t = C.c_long


class t_tsPWS(C.Structure):
    """include/ts_pws1f_lib.h (reference: src/ts_pws1f_lib.h:19-57)."""
    _fields_ = [
        ("type", C.c_int), ("uni", C.c_uint), ("J", C.c_uint), ("V", C.c_uint),
        ("s0", C.c_double), ("b0", C.c_double), ("w0", C.c_double), ("wu", C.c_double),
        ("fmin", C.c_double), ("Q", C.c_double), ("cycle", C.c_double),
        ("w0set", C.c_int), ("lrm", C.c_int), ("bin", C.c_int), ("lkinst", C.c_int),
        ("lVfix", C.c_int), ("ls0fix", C.c_int), ("lb0fix", C.c_int), ("verbose", C.c_int),
        ("fold", C.c_int), ("unbiased", C.c_int), ("convergence", C.c_int),
        ("subsmpl_N", C.c_uint), ("subsmpl_p", C.c_double),
        ("jackknife_n", C.c_uint), ("jackknife_d", C.c_uint), ("obin", C.c_uint),
        ("AllSteps", C.c_int), ("Nmax", C.c_uint), ("Kmax", C.c_uint),
        ("kinst", C.c_char_p), ("filein", C.c_char_p), ("fileout", C.c_char_p), ("fileconv", C.c_char_p),
    ]


class FrameInfo(C.Structure):
    """tspws_hip_frame_info (include/tspws_hip.h)."""
    _fields_ = [
        ("type", C.c_int), ("S", C.c_uint), ("V", C.c_uint), ("J", C.c_uint), ("N", C.c_uint),
        ("s0", C.c_double), ("b0", C.c_double), ("w0", C.c_double), ("Cpsi", C.c_double),
        ("ncoef", C.c_size_t), ("ntaps", C.c_size_t), ("device", C.c_int),
    ]


class InverseInfo(C.Structure):
    """tspws_hip_inverse_info_t (include/tspws_hip.h)."""
    _fields_ = [("items", C.c_uint), ("per_scale", C.c_uint), ("waves", C.c_uint), ("waves_lds", C.c_uint), ("waves_fast", C.c_uint),
                ("generic", C.c_uint)]


class TspwsError(RuntimeError):
    pass


def build(verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", _HERE, "all"], capture_output=True, text=True)
    if verbose or out.returncode:
        print(out.stdout + out.stderr)
    if out.returncode:
        raise TspwsError("building libtspws_hip.so failed")
    return LIB_PATH


_lib = None

# name -> (restype, argtypes); every symbol include/tspws_hip.h + ts_pws1f_lib.h declare
_vp, _u, _d, _sz, _i, _f = C.c_void_p, C.c_uint, C.c_double, C.c_size_t, C.c_int, C.c_float
SYMBOLS = {
    "tspws_main": (_i, [_vp, _vp, _vp]),
    "tspws_hip_device_count": (_i, []),
    "tspws_hip_last_error": (C.c_char_p, []),
    "tspws_hip_alloc": (_i, [C.POINTER(_vp), _sz, _i]),
    "tspws_hip_free": (_i, [_vp]),
    "tspws_hip_upload": (_i, [_vp, _vp, _sz, _vp]),
    "tspws_hip_download": (_i, [_vp, _vp, _sz, _vp]),
    "tspws_hip_zero": (_i, [_vp, _sz, _vp]),
    "tspws_hip_sync": (_i, [_vp]),
    "tspws_resolve_params": (None, [_vp, _u, _f]),
    "tspws_hip_plan_create": (_i, [C.POINTER(_vp), _i, _u, _u, _u, _d, _d, _d, _i, _i]),
    "tspws_hip_plan_destroy": (None, [_vp]),
    "tspws_hip_plan_info": (_i, [_vp, _vp]),
    "tspws_hip_plan_tables": (_i, [_vp] + [_vp] * 6),
    "tspws_hip_plan_taps": (_i, [_vp, _vp, _vp]),
    "tspws_hip_fold": (_i, [_vp, _sz, _sz, _sz, _vp]),
    "tspws_hip_remove_mean": (_i, [_vp, _sz, _sz, _sz, _vp]),
    "tspws_hip_partial_stacks": (_i, [_vp, _vp, _sz, _sz, _sz, _sz, _u, _vp, _sz, _vp]),
    "tspws_hip_partial_stacks_range": (_i, [_vp, _vp, _sz, _sz, _sz, _sz, _u, _u, _u, _vp, _sz, _vp]),
    "tspws_hip_forward_f64": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "tspws_hip_forward_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "tspws_hip_spectral_first_scale": (_u, [_vp, _u]),
    "tspws_hip_spectral_end_scale": (_u, [_vp]),
    "tspws_hip_spectral_transform_length": (_u, [_vp]),
    "tspws_hip_spectral_choice": (_u, [_vp, _sz]),
    "tspws_hip_forward_spectral_f64": (_i, [_vp, _vp, _sz, _sz, _vp, _u, _vp]),
    "tspws_hip_forward_spectral_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _u, _vp]),
    "tspws_hip_inverse": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "tspws_hip_inverse_info": (_i, [_vp, _vp]),
    "tspws_hip_inverse_bands": (_i, [_vp, _vp, _sz, _vp, _u, _vp, _vp, _vp]),
    "tspws_bands_from_frequencies": (_i, [_vp, _u, _d, _d, _vp, _vp, _u, _vp, _vp]),
    "tspws_hip_accumulate": (_i, [_vp, _vp, _sz, _vp, _vp, _i, _vp]),
    "tspws_hip_stacks_double": (_i, [_vp, _vp, _u, _sz, _vp, _vp, _vp]),
    "tspws_hip_stacks_float": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "tspws_hip_weight": (_i, [_vp, _vp, _vp, _vp, _u, _u, _d, _i, _vp]),
    "tspws_hip_epilogue": (_i, [_vp, _vp, _vp, _vp, _sz, _u, _vp]),
    "tspws_hip_stack_local": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "tspws_hip_reduce_buffer": (_i, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_sz)]),
    "tspws_hip_stack_finish": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "tspws_hip_stack_finish_range": (_i, [_vp, _vp, _sz, _u, _u, _vp]),
    "tspws_hip_stack_finish_tail": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "tspws_hip_stack": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "tspws_hip_stack_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _vp, _vp]),
    "tspws_hip_stack_batch_stats": (_i, [_vp, _vp]),
    "tspws_hip_stack_batch_bands": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _u, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_stack_batch_bands_stats": (_i, [_vp, _vp]),
    "tspws_hip_profile_begin": (_i, [_vp, _sz]),
    "tspws_hip_profile_read": (_i, [_vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "tspws_hip_profile_end": (_i, [_vp, C.POINTER(_d), C.POINTER(_sz)]),
    "tspws_hip_stream_launches": (_i, [_vp]),
    "tspws_jackknife_plan": (_i, [_vp, _vp, _sz, _u, _u, _u]),
    "tspws_hip_jackknife": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _u, _vp, _vp, _vp, _vp]),
    "tspws_hip_stack_jackknife": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _u, _vp, _vp, _vp, _vp]),
    "tspws_main_release": (None, []),
    "tspws_main_on": (_i, [_i, _vp, _vp, _vp]),
    "tspws_main_cached_devices": (C.c_ulonglong, []),
    "tspws_hip_finish_shard": (_i, [_vp, _vp, _sz, _u, _u, C.POINTER(_u), C.POINTER(_u)]),
    "tspws_hip_stack_finish_scales": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp]),
    "tspws_hip_jackknife_buffer": (_i, [_vp, _vp, _u, C.POINTER(_vp), C.POINTER(_sz)]),
    "tspws_hip_jackknife_local": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _u, _vp]),
    "tspws_hip_jackknife_finish": (_i, [_vp, _vp, _sz, _vp, _u, _u, _u, _vp, _vp, _vp, _vp]),
    "tspws_selection_classes": (_i, [_vp, _u, _sz, _vp, _vp, C.POINTER(_u)]),
    "tspws_hip_jackknife_single": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _u, _vp, _vp, _vp, _vp]),
    "tspws_hip_jackknife_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_jackknife_batch_stats": (_i, [_vp, _vp]),
    "tspws_hip_jackknife_batch_two_stage": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_jackknife_batch_two_stage_stats": (_i, [_vp, _vp]),
    "tspws_subsampling_plan": (_i, [_vp, _sz, _sz]),
    "tspws_hip_subsample": (_i, [_vp, _vp, _vp, _sz, _sz, _u, _vp, _vp, _vp]),
    "tspws_hip_subsample_sel": (_i, [_vp, _vp, _vp, _sz, _sz, _u, _vp, _vp, _vp, _vp]),
    "tspws_subsampling_plan_batch": (_i, [_vp, _vp, _u, _u, _d]),
    "tspws_hip_subsample_batch_sel": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _u, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_subsample_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _u, _vp, _vp, _vp, _vp]),
    "tspws_hip_subsample_batch_stats": (_i, [_vp, _vp]),
    "tspws_bootstrap_plan": (_i, [_vp, _sz]),
    "tspws_bootstrap_plan_batch": (_i, [_vp, _vp, _u, _u]),
    "tspws_hip_bootstrap_batch_cnt": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_bootstrap_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _u, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_bootstrap_batch_stats": (_i, [_vp, _vp]),
    "tspws_hip_weighted_stack_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_weighted_stack_batch_stats": (_i, [_vp, _vp]),
    "tspws_weights_from_scores": (_i, [_vp, _vp, _vp, _u, _i, _d]),
    "tspws_hip_replica_bands": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp, _u, _vp, _vp]),
    "tspws_hip_replica_bands_stats": (_i, [_vp, _vp]),
    "tspws_hip_trace_scores": (_i, [_vp, _vp, _sz, _vp, _u, _vp, _sz, _u, _sz, _sz, _vp, _vp, _vp]),
    "tspws_hip_trace_scores_stats": (_i, [_vp, _vp]),
    "tspws_selection_from_scores": (_i, [_vp, _vp, _vp, _vp, _u, _i, _d]),
    "tspws_hip_stretch_rows": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp, _sz, _d, _vp, _u, _vp, _u, _vp, _vp, _vp]),
    "tspws_hip_stretch_rows_stats": (_i, [_vp, _vp]),
    "tspws_stretch_grid": (_i, [_vp, _d, _u]),
    "tspws_hip_wxs_coef": (_i, [_vp, _vp, _vp, _vp, _sz, _u, _d, _vp, _u, _vp, _u, _i, _vp, _vp, _vp]),
    "tspws_hip_wxs_rows": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp, _sz, _d, _vp, _u, _vp, _u, _i, _vp, _vp, _vp]),
    "tspws_hip_wxs_rows_stats": (_i, [_vp, _vp]),
    "tspws_hip_mwcs_rows": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp, _sz, _d, _vp, _vp, _u, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_mwcs_rows_stats": (_i, [_vp, _vp]),
    "tspws_mwcs_bins": (_i, [_u, _d, _d, _d, _vp, _vp]),
    "tspws_hip_dtw_rows": (_i, [_vp, _vp, _sz, _u, _u, _vp, _vp, _sz, _d, _vp, _vp, _u, _vp, _vp, _vp]),
    "tspws_hip_dtw_rows_stats": (_i, [_vp, _vp]),
    "tspws_hip_ftan_coef": (_i, [_vp, _vp, _vp, _sz, _u, _d, _u, _u, _vp, _u, _vp, _u, _i, _vp, _vp, _vp]),
    "tspws_hip_ftan_rows": (_i, [_vp, _vp, _sz, _u, _u, _vp, _d, _u, _u, _vp, _u, _vp, _u, _i, _vp, _vp, _vp]),
    "tspws_hip_ftan_rows_stats": (_i, [_vp, _vp]),
    "tspws_ftan_windows": (_i, [_d, _d, _d, _d, _d, _sz, _i, _vp]),
    "tspws_ftan_periods": (_i, [_vp, _u, _d, _d, _vp]),
    "tspws_hip_filter_coef": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _u, _d, _i, _i, _vp, _vp]),
    "tspws_hip_filter_traces": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _sz, _u, _vp, _i, _vp, _sz, _vp]),
    "tspws_hip_filter_traces_stats": (_i, [_vp, _vp]),
    "tspws_mwcs_basis_size": (_sz, [_vp]),
    "tspws_mwcs_basis": (_i, [_vp, _vp]),
    "tspws_hip_selective_stack_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _i, _i, _d, _u, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_convergence": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_convergence_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tspws_hip_convergence_batch_stats": (_i, [_vp, _vp]),
    "tspws_hip_synth": (_i, [_vp, _sz, _sz, _sz, C.c_uint64, _sz, _vp]),
    # several devices of one process (csrc/comm.hip)
    "tspws_hip_comm_create": (_i, [C.POINTER(_vp), _i, _vp]),
    "tspws_hip_comm_destroy": (None, [_vp]),
    "tspws_hip_comm_size": (_i, [_vp]),
    "tspws_hip_comm_device": (_i, [_vp, _i]),
    "tspws_hip_comm_stream": (_vp, [_vp, _i]),
    "tspws_hip_comm_backend": (C.c_char_p, [_vp]),
    "tspws_hip_allreduce_f64": (_i, [_vp, _vp, _sz, _vp]),
    "tspws_hip_reduce_f64": (_i, [_vp, _vp, _sz, _i, _vp]),
    "tspws_shard_range": (None, [_sz, _u, _u, C.POINTER(_sz), C.POINTER(_sz)]),
    "tspws_hip_multi_create": (_i, [C.POINTER(_vp), _i, _vp, _i, _u, _u, _u, _d, _d, _d, _i]),
    "tspws_hip_multi_destroy": (None, [_vp]),
    "tspws_hip_multi_comm": (_vp, [_vp]),
    "tspws_hip_multi_plan": (_vp, [_vp, _i]),
    "tspws_hip_multi_upload": (_i, [_vp, _vp, _sz, _sz, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tspws_hip_multi_prologue": (_i, [_vp, _vp, _sz, _sz, _sz, _i, _i]),
    "tspws_hip_multi_stack": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "tspws_hip_multi_stack_jackknife": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _u, _vp, _vp, _vp]),
}


def load():
    """Load libtspws_hip.so and type its entry points.  Raises when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TspwsError(f"{LIB_PATH} is missing: run __graft_entry__.build() / make -C ts-pws_amd")
        # torch wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7) but request it by file
        # name; importing torch FIRST makes the loader hand that same runtime to this library, so a
        # process never ends up with two HIP runtimes (streams / events would not be shared).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the header promises a symbol the library lacks
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc, what=""):
    if rc:
        raise TspwsError(f"{what} failed with code {rc}: {load().tspws_hip_last_error().decode()}")


def _offsets(first, limit=None, rows="trace rows"):
    """(first as contiguous uint64, B, T) of B + 1 ensemble offsets, T = first[B] - first[0]; `limit` = how many `rows` they index into
    (None: no upper limit).  Converted offsets pass again unchanged."""
    import numpy as np
    f = np.asarray(first)
    if f.ndim != 1 or f.size < 1 or f.dtype.kind not in "iu":
        raise TspwsError("first must be a 1-D integer array of B + 1 ensemble offsets")
    if (f < 0).any() or (np.diff(f) < 0).any() or (limit is not None and int(f[-1]) > limit):
        raise TspwsError("first must be non-decreasing offsets" + (f" into the {limit} {rows}" if limit is not None else " >= 0"))
    f = np.ascontiguousarray(f, dtype=np.uint64)  # size_t
    return f, f.size - 1, int(f[-1] - f[0])


def _host_array(a, name, dtype, shape, optional=False):
    """`a` as a contiguous numpy array after checking its dtype and shape.  optional=True is the `mtr` of replica_bands / stretch_rows:
    None passes, and so does an array with strides (it is copied)."""
    import numpy as np
    if a is None and optional:
        return None
    if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape or not (optional or a.flags.c_contiguous):
        dims = f"of {shape[0]} entries" if len(shape) == 1 else "".join(f"[{n}]" for n in shape)
        raise TspwsError(f"{name} must be {'None or a' if optional else 'a contiguous'} {np.dtype(dtype).name} numpy array {dims}")
    return a if a.flags.c_contiguous else np.ascontiguousarray(a)


def _score_plane(score, T):
    """One plane of T scores (numpy, a sequence or a tensor anywhere) as contiguous float64 [T]."""
    import numpy as np
    if hasattr(score, "detach"):
        score = score.detach().cpu().numpy()
    sc = np.ascontiguousarray(score, dtype=np.float64)
    if sc.shape != (T,):
        raise TspwsError(f"score must be one plane of {T} scores, got {sc.shape}")
    return sc


def resolve(params, nsamp, dt=1.0):
    """Resolved copy of a t_tsPWS (tspws_resolve_params; reference ts_pws1f_lib.c:91-124)."""
    p = t_tsPWS.from_buffer_copy(params)
    load().tspws_resolve_params(C.byref(p), nsamp, dt)
    return p


def shard_range(mtr_global, rank, world):
    """Contiguous trace shard [first, first+count) of `rank` (the library's tspws_shard_range)."""
    first = rank * mtr_global // world
    last = (rank + 1) * mtr_global // world
    return first, last - first


class Plan:
    """Device-resident frame (taps, tables, scratch) for one resolved parameter set."""

    def __init__(self, params, N, device=0):
        self.lib = load()
        self.params = t_tsPWS.from_buffer_copy(params)
        h = C.c_void_p()
        p = self.params
        check(self.lib.tspws_hip_plan_create(C.byref(h), p.type, p.J, p.V, N, p.s0, p.b0, p.w0, int(p.uni), device), "plan_create")
        self.h = h
        info = FrameInfo()
        check(self.lib.tspws_hip_plan_info(self.h, C.byref(info)), "plan_info")
        self.info = info
        self.N, self.S, self.ncoef, self.ntaps, self.Cpsi = N, info.S, info.ncoef, info.ntaps, info.Cpsi
        self.device = device

    def tables(self):
        import numpy as np
        S = self.S
        t = dict(scale=np.zeros(S), L=np.zeros(S, np.uint32), c=np.zeros(S, np.int32), cd=np.zeros(S, np.int32),
                 D=np.zeros(S, np.uint32), Ns=np.zeros(S, np.uint32))
        check(self.lib.tspws_hip_plan_tables(self.h, *[t[k].ctypes.data for k in ("scale", "L", "c", "cd", "D", "Ns")]), "plan_tables")
        return t

    def taps(self):
        import numpy as np
        w = np.zeros(self.ntaps, np.complex128)
        wd = np.zeros(self.ntaps, np.complex128)
        check(self.lib.tspws_hip_plan_taps(self.h, w.ctypes.data, wd.ctypes.data), "plan_taps")
        return w, wd

    # ---- device-resident path on torch tensors -------------------------------------
    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reduce_buffer(self, mtr_global):
        """torch view (float64) of the buffer a multi-GPU caller all-reduces between the halves.

        The view aliases library scratch: it is the buffer of THIS (two-stage / single-stage, Kmax, mtr_global) shape.
        A later call that needs a larger buffer allocates a new block (the old one stays alive until the plan is
        destroyed, so an in-flight collective on it is safe) -- fetch the view again after changing the shape."""
        import torch
        ptr, n = C.c_void_p(), C.c_size_t()
        check(self.lib.tspws_hip_reduce_buffer(self.h, C.byref(self.params), mtr_global, C.byref(ptr), C.byref(n)), "reduce_buffer")
        return _as_tensor(ptr.value, n.value, torch.float64, self.device)

    def _traces(self, traces, dtype=None):
        """(rows, row stride) of a float32 [mtr][N] device tensor after checking what the C ABI cannot see."""
        import torch
        dtype = dtype or torch.float32
        if traces.dtype != dtype or traces.dim() != 2 or traces.shape[1] != self.N:
            raise TspwsError(f"traces must be {dtype} [mtr][{self.N}], got {traces.dtype} {tuple(traces.shape)}")
        if traces.shape[0] and traces.stride(1) != 1:
            raise TspwsError("traces must be contiguous along the samples (stride(1) == 1)")
        if not traces.is_cuda or (traces.device.index or 0) != self.device:
            raise TspwsError(f"traces live on {traces.device}, the plan on cuda:{self.device}")
        mtr = traces.shape[0]
        ld = traces.stride(0) if mtr > 1 else traces.shape[1]
        if ld < self.N:
            raise TspwsError("overlapping trace rows (stride(0) < N)")
        return mtr, ld

    def _need(self, t, name, dt, size, what="{} tensor", exact=False):
        """Raise unless `t` is a contiguous tensor of dtype `dt` ("float32" / "float64") on the plan's device, of exactly the shape `size` (a
        tuple) or of at least (exact=True: exactly) `size` elements (an int).  `what` words the size in the message; {} stands for `size`."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != getattr(torch, dt) or not t.is_contiguous() or not t.is_cuda or (t.device.index or 0) != self.device or \
                (tuple(t.shape) != size if isinstance(size, tuple) else t.numel() < size or (exact and t.numel() != size)):
            dims = "".join(f"[{n}]" for n in size) if isinstance(size, tuple) else size
            raise TspwsError(f"{name} must be a contiguous {dt} {what.format(dims)} on cuda:{self.device}")

    def _out(self, t, name):
        self._need(t, name, "float32", self.N, "tensor of >= {} samples")
        return t.data_ptr()

    def _refs(self, t, name, rows):
        """Data pointer of a reference array: contiguous float32 [rows][N] (or [N] for one row) on the plan's device."""
        one = rows == 1 and getattr(t, "ndim", 2) == 1
        self._need(t, name, "float32", (self.N,) if one else (rows, self.N), f"[{rows}][{self.N}] tensor")
        return t.data_ptr()

    def _rows_out(self, lead, device, ls_out, ts_out, mtr_out=None, counts=True, new="empty", what="{} tensor"):
        """ls_out / ts_out (float32 [*lead][N] on the plan's device) and mtr_out (uint32 numpy [*lead]; None with counts=False), each as
        given or new, and checked.  `new` = the torch constructor of a missing tensor ("empty" / "zeros"), or None: nothing may be missing."""
        import numpy as np
        import torch
        if new is not None:
            ls_out = getattr(torch, new)((*lead, self.N), dtype=torch.float32, device=device) if ls_out is None else ls_out
            ts_out = getattr(torch, new)((*lead, self.N), dtype=torch.float32, device=device) if ts_out is None else ts_out
            mtr_out = np.zeros(lead, np.uint32) if mtr_out is None and counts else mtr_out
        if counts:
            _host_array(mtr_out, "mtr_out", np.uint32, lead)
        self._need(ls_out, "ls_out", "float32", (*lead, self.N), what)
        self._need(ts_out, "ts_out", "float32", (*lead, self.N), what)
        return ls_out, ts_out, mtr_out

    def _coef_sets(self, Y, what):
        """(Y on the plan's device, whether it came as numpy) of the coefficient sets Y[`what`][ncoef]: a complex128 numpy array or a
        contiguous complex128 tensor on the plan's device."""
        import numpy as np
        import torch
        if not isinstance(Y, (np.ndarray, torch.Tensor)):
            raise TspwsError("Y must be a complex128 numpy array or device tensor")
        host = isinstance(Y, np.ndarray)
        if Y.dtype != (np.complex128 if host else torch.complex128) or Y.ndim != 2 or Y.shape[1] != self.ncoef or not Y.shape[0]:
            raise TspwsError(f"Y must be complex128 [{what} >= 1][{self.ncoef}], got {Y.dtype} {tuple(Y.shape)}")
        if host:
            return torch.as_tensor(np.ascontiguousarray(Y), device=f"cuda:{self.device}"), True
        if not Y.is_cuda or (Y.device.index or 0) != self.device or not Y.is_contiguous():
            raise TspwsError(f"Y must be a contiguous tensor on cuda:{self.device}, got {Y.device}")
        return Y, False

    def _strided_rows(self, t, name="rows", kind="", mid="M"):
        """(B, M, ld) of float32 [B][M][N] rows on the plan's device, contiguous or a [:, :, :N] view of one [B][M][ld] base.  The words of
        the messages: `name` of the argument, `kind` of rows ("replica ", "reference "), `mid` = the letter of the middle dimension."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != self.N:
            raise TspwsError(f"{name} must be a float32 [B][{mid}][{self.N}] tensor, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if not t.is_cuda or (t.device.index or 0) != self.device:
            raise TspwsError(f"{name} live on {t.device}, the plan on cuda:{self.device}")
        B, Mn = t.shape[0], t.shape[1]
        ld = t.stride(1) if Mn > 1 else (t.stride(0) if B > 1 else self.N)
        if B and Mn:
            if t.stride(2) != 1:
                raise TspwsError(f"{name} must be contiguous along the samples (stride(2) == 1)")
            if ld < self.N:
                raise TspwsError(f"overlapping {kind}rows (row stride < N)")
            if B > 1 and t.stride(0) != Mn * ld:
                raise TspwsError(f"{name} must be a [B][{mid}][N] view of one [B][{mid}][ld] base (stride(0) == {mid} * stride(1))")
        return B, Mn, ld

    def _strided_refs(self, ref, B):
        """The row stride of float32 [B][N] reference rows on the plan's device, contiguous or a [:, :N] view of one [B][ldr] base."""
        import torch
        if not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 or tuple(ref.shape) != (B, self.N):
            raise TspwsError(f"ref must be a float32 [{B}][{self.N}] tensor, got {getattr(ref, 'dtype', type(ref))} {tuple(getattr(ref, 'shape', ()))}")
        if not ref.is_cuda or (ref.device.index or 0) != self.device:
            raise TspwsError(f"ref lives on {ref.device}, the plan on cuda:{self.device}")
        ldr = ref.stride(0) if B > 1 else self.N
        if B and (ref.stride(1) != 1 or ldr < self.N):
            raise TspwsError("ref must be contiguous along the samples, its rows not overlapping")
        return ldr

    @staticmethod
    def _windows(windows):
        """`windows` as the C table: contiguous uint64 [W][2] of (n0, n1) pairs."""
        import numpy as np
        try:
            wa = np.ascontiguousarray(np.asarray(windows, dtype=np.int64))
        except (TypeError, ValueError):
            raise TspwsError("windows must be a sequence of (n0, n1) pairs of non-negative integers") from None
        if wa.ndim != 2 or wa.shape[1] != 2 or (wa < 0).any():
            raise TspwsError("windows must be a sequence of (n0, n1) pairs of non-negative integers")
        return np.ascontiguousarray(wa, dtype=np.uint64)  # size_t

    def _wxs_out(self, lead, sums, out, device):
        """(sums or None, fit) of a wavelet cross-spectrum call, given as `out` or new (NaN-filled): float64 tensors of at least
        prod(lead) 9 / prod(lead) 6 values."""
        import torch
        n = 1
        for k in lead:
            n *= k
        o_sums, o_fit = (out if sums else (None, out)) if out is not None else (None, None)
        if out is None:
            o_fit = torch.full((*lead, 6), float("nan"), dtype=torch.float64, device=device)
            o_sums = torch.full((*lead, 9), float("nan"), dtype=torch.float64, device=device) if sums else None
        self._need(o_fit, "out: fit", "float64", n * 6, "tensor of >= {} values")
        if sums:
            self._need(o_sums, "out: sums", "float64", n * 9, "tensor of >= {} values")
        return o_sums, o_fit

    def _stats(self, what, names):
        """dict(names -> counts) of tspws_hip_<what> (len(names) unsigned counters)."""
        st = (C.c_uint * len(names))()
        check(getattr(self.lib, "tspws_hip_" + what)(self.h, C.byref(st)), what)
        return dict(zip(names, list(st)))

    def stacks(self, traces):
        """The two FP64 planes of the rows of `traces` -- linear stack ST = sum Y_t and phase stack PS = sum Y_t / |Y_t| -- as complex128
        numpy arrays of ncoef: tspws_hip_stacks_float for float32 [mtr][N] rows, tspws_hip_stacks_double for float64 ones (the partial
        stacks of a two-stage call).  The device buffers hold NaN before the call (the entry points clear them: an unwritten coefficient
        shows); synchronises."""
        import numpy as np
        import torch
        if traces.dtype not in (torch.float32, torch.float64):
            raise TspwsError(f"traces must be float32 or float64 [mtr][{self.N}], got {traces.dtype}")
        mtr, ld = self._traces(traces, traces.dtype)
        if not mtr:
            raise TspwsError("stacks needs at least one row")
        fn = self.lib.tspws_hip_stacks_float if traces.dtype == torch.float32 else self.lib.tspws_hip_stacks_double
        ST = torch.full((2 * self.ncoef,), float("nan"), dtype=torch.float64, device=traces.device)
        PS = torch.full((2 * self.ncoef,), float("nan"), dtype=torch.float64, device=traces.device)
        check(fn(self.h, traces.data_ptr(), mtr, ld, ST.data_ptr(), PS.data_ptr(), self._stream()), "stacks")
        torch.cuda.synchronize(traces.device)
        return ST.cpu().numpy().view(np.complex128), PS.cpu().numpy().view(np.complex128)

    def inverse_info(self):
        """How tspws_hip_inverse launches this frame (tspws_hip_inverse_info): dict(items, per_scale, waves, waves_lds, waves_fast, generic)."""
        info = InverseInfo()
        check(self.lib.tspws_hip_inverse_info(self.h, C.byref(info)), "inverse_info")
        return {k: int(getattr(info, k)) for k, _ in InverseInfo._fields_}

    def inverse(self, Y):
        """Real part of the inverse frame transform of the coefficient sets Y[nrec][ncoef] in ONE tspws_hip_inverse call: a complex128 numpy
        array (returns float64 numpy [nrec][N]) or a contiguous complex128 tensor on the plan's device (returns a float64 tensor there).
        The output holds NaN before the call (an unwritten sample shows); synchronises."""
        import torch
        Yd, host = self._coef_sets(Y, "nrec")
        x = torch.full((Yd.shape[0], self.N), float("nan"), dtype=torch.float64, device=Yd.device)
        check(self.lib.tspws_hip_inverse(self.h, Yd.data_ptr(), Yd.shape[0], x.data_ptr(), self._stream()), "inverse")
        torch.cuda.synchronize(Yd.device)
        return x.cpu().numpy() if host else x

    def inverse_bands(self, Y, bands, quadrature=False):
        """Band rows of the coefficient sets Y[nset][ncoef] in ONE tspws_hip_inverse_bands call: `bands` = R half-open scale ranges
        (s_begin, s_end), which may overlap, cut an octave between voices or be empty.  Returns X[nset][R][N] (float64) -- row r = the sum of
        the reconstruction's scale rows s_begin <= s < s_end -- or, with quadrature=True, (X, Q): Q = the same rows of the set -i Y.  Y as for
        inverse (numpy in, numpy out; device tensor in, device tensors out).  The outputs hold NaN before the call; synchronises."""
        import torch
        bt = band_table(bands)
        Yd, host = self._coef_sets(Y, "nset")
        R = bt.shape[0]
        X = torch.full((Yd.shape[0], R, self.N), float("nan"), dtype=torch.float64, device=Yd.device)
        Q = torch.full_like(X, float("nan")) if quadrature else None
        check(self.lib.tspws_hip_inverse_bands(self.h, Yd.data_ptr(), Yd.shape[0], bt.ctypes.data, R, X.data_ptr(), Q.data_ptr() if quadrature else None,
                                               self._stream()), "inverse_bands")
        torch.cuda.synchronize(Yd.device)
        if host:
            X, Q = X.cpu().numpy(), (Q.cpu().numpy() if quadrature else None)
        return (X, Q) if quadrature else X

    def stack_local(self, traces, first=0, mtr_global=None):
        mtr, ld = self._traces(traces)
        mtr_global = mtr if mtr_global is None else mtr_global
        check(self.lib.tspws_hip_stack_local(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, first, mtr_global, self._stream()),
              "stack_local")

    def partial_stacks_range(self, traces, first, mtr_global, g_begin, g_end):
        """Two-stage only: stream the groups [g_begin, g_end) of this shard into rows of the reduce buffer."""
        mtr, ld = self._traces(traces)
        buf = self.reduce_buffer(mtr_global)
        check(self.lib.tspws_hip_partial_stacks_range(self.h, traces.data_ptr(), ld, mtr, first, mtr_global, self.params.Kmax, g_begin, g_end,
                                                      buf.data_ptr(), self.N, self._stream()), "partial_stacks_range")

    def stack_finish(self, mtr_global, ls, ts):
        check(self.lib.tspws_hip_stack_finish(self.h, C.byref(self.params), mtr_global, self._out(ls, "ls"), self._out(ts, "ts"), self._stream()),
              "stack_finish")

    def stack_finish_range(self, mtr_global, g_begin, g_end):
        """Two-stage: transform the reduced partial stacks [g_begin, g_end) and add them to the linear / phase stacks."""
        check(self.lib.tspws_hip_stack_finish_range(self.h, C.byref(self.params), mtr_global, g_begin, g_end, self._stream()),
              "stack_finish_range")

    def stack_finish_tail(self, mtr_global, ls, ts):
        """Weight, inverse transforms, epilogue (after every group went through stack_finish_range)."""
        check(self.lib.tspws_hip_stack_finish_tail(self.h, C.byref(self.params), mtr_global, self._out(ls, "ls"), self._out(ts, "ts"),
                                                   self._stream()), "stack_finish_tail")

    # ---- trace-sharded jackknife (see jackknife_sharded) ------------------------------
    @staticmethod
    def _sel(sel, width, noun=None, dims=None):
        """`sel` as contiguous int8 [rows][width].  With `noun` ("selection" / "masks"; `dims` = its shape in words) only a 2-D int8 / uint8 /
        bool numpy array passes; without, whatever converts to int8 (the sharded jackknife's callers)."""
        import numpy as np
        if noun and (not isinstance(sel, np.ndarray) or sel.ndim != 2 or sel.dtype not in (np.int8, np.uint8, np.bool_)):
            raise TspwsError(f"{noun} must be a 2-D int8 / uint8 / bool numpy array {dims}")
        rows = sel.shape[0]
        sel = np.ascontiguousarray(sel, dtype=np.int8)
        if sel.shape != (rows, width):
            raise TspwsError(f"selection must be [{rows}][{width}] (replica x trace of the WHOLE ensemble), got {sel.shape}")
        return sel

    def jackknife_buffer(self, C_):
        """torch view (float64, [C * Kmax * N]) of the replicas' partial-stack rows a multi-GPU caller reduces.  Like
        reduce_buffer the view aliases library scratch of THIS (C, Kmax) shape: an outgrown block stays alive until the plan is
        destroyed (an in-flight collective on it is safe), but later calls use the new block -- fetch the view again."""
        import torch
        ptr, n = C.c_void_p(), C.c_size_t()
        check(self.lib.tspws_hip_jackknife_buffer(self.h, C.byref(self.params), C_, C.byref(ptr), C.byref(n)), "jackknife_buffer")
        return _as_tensor(ptr.value, n.value, torch.float64, self.device)

    def jackknife_local(self, traces, first, mtr_global, sel):
        """One pass over the shard: its sums for the plain groups (reduce_buffer) and for every replica (jackknife_buffer)."""
        mtr, ld = self._traces(traces)
        sel = self._sel(sel, mtr_global)
        check(self.lib.tspws_hip_jackknife_local(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, first, mtr_global, sel.ctypes.data,
                                                 sel.shape[0], self._stream()), "jackknife_local")

    def jackknife_finish(self, mtr_global, sel, c_begin, c_end, ls_out, ts_out, mtr_out):
        """Replicas [c_begin, c_end) from the reduced rows into rows of the [C][N] float32 tensors; sizes into mtr_out (uint32 numpy)."""
        sel = self._sel(sel, mtr_global)
        self._rows_out((sel.shape[0],), None, ls_out, ts_out, mtr_out, new=None)
        check(self.lib.tspws_hip_jackknife_finish(self.h, C.byref(self.params), mtr_global, sel.ctypes.data, sel.shape[0], c_begin, c_end,
                                                  ls_out.data_ptr(), ts_out.data_ptr(), mtr_out.ctypes.data, self._stream()), "jackknife_finish")

    # ---- scale-sharded finish stage (see stack_sharded) --------------------------------
    def finish_shard(self, mtr_global, rank, world):
        """Scales [s_begin, s_end) that `rank` of `world` finishes, or None when this plan / parameter set has no sharded finish."""
        a, b = C.c_uint(), C.c_uint()
        rc = self.lib.tspws_hip_finish_shard(self.h, C.byref(self.params), mtr_global, rank, world, C.byref(a), C.byref(b))
        if rc == 1:
            return None
        check(rc, "finish_shard")
        return a.value, b.value

    def stack_finish_scales(self, mtr_global, s_begin, s_end, x2):
        """This rank's share of the finish stage: x2 (float64 [2 N], cuda) receives the partial reconstructions of the scales."""
        self._need(x2, "x2", "float64", 2 * self.N, "tensor of {} values", exact=True)
        check(self.lib.tspws_hip_stack_finish_scales(self.h, C.byref(self.params), mtr_global, s_begin, s_end, x2.data_ptr(), self._stream()),
              "stack_finish_scales")

    def epilogue(self, x2, mtr_global, ls, ts):
        """ls = (float)x2[N:] / mtr, ts = (float)x2[:N]  (reference epilogue, ts_pws1f_lib.c:233-241)."""
        self._need(x2, "x2", "float64", 2 * self.N, "tensor of {} values", exact=True)
        check(self.lib.tspws_hip_epilogue(self._out(ls, "ls"), self._out(ts, "ts"), x2.data_ptr() + 8 * self.N, x2.data_ptr(), self.N, mtr_global,
                                          self._stream()), "epilogue")

    def stack(self, traces, first=0, mtr_global=None, group=None):
        """ls, tsPWS (float32 cuda tensors) of a shard of HBM-resident traces; see stack_sharded."""
        return stack_sharded(self, traces, first, mtr_global, group)

    def stack_jackknife(self, traces, sel, ls=None, ts=None):
        """Two-stage stack AND its jackknife replicas from ONE pass over the traces (tspws_hip_stack_jackknife).
        `sel` = [C][mtr] int8 selection (tspws_jackknife_plan).  Returns ls, ts, ls_out[C][N], ts_out[C][N], mtr_out[C]."""
        import numpy as np
        import torch
        mtr, ld = self._traces(traces)
        sel = self._sel(sel, mtr)
        Cn = sel.shape[0]
        ls = torch.empty(self.N, dtype=torch.float32, device=traces.device) if ls is None else ls
        ts = torch.empty(self.N, dtype=torch.float32, device=traces.device) if ts is None else ts
        ls_out = torch.empty((Cn, self.N), dtype=torch.float32, device=traces.device)
        ts_out = torch.empty((Cn, self.N), dtype=torch.float32, device=traces.device)
        mtr_out = np.zeros(Cn, np.uint32)
        check(self.lib.tspws_hip_stack_jackknife(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, self._out(ls, "ls"), self._out(ts, "ts"),
                                                 sel.ctypes.data, Cn, ls_out.data_ptr(), ts_out.data_ptr(), mtr_out.ctypes.data, self._stream()),
              "stack_jackknife")
        return ls, ts, ls_out, ts_out, mtr_out

    def jackknife_single(self, traces, sel, ls_out=None, ts_out=None, mtr_out=None):
        """Single-stage jackknife replicas (tspws_hip_jackknife_single; the reference leaves these rows untouched).
        `sel` = [C][mtr] int8 selection (jackknife_selection).  Returns ls_out[C][N], ts_out[C][N] (float32 cuda), mtr_out[C] (uint32)."""
        mtr, ld = self._traces(traces)
        sel = self._sel(sel, mtr, "selection", "[C][mtr]")
        Cn = sel.shape[0]
        ls_out, ts_out, mtr_out = self._rows_out((Cn,), traces.device, ls_out, ts_out, mtr_out)
        check(self.lib.tspws_hip_jackknife_single(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, sel.ctypes.data, Cn, ls_out.data_ptr(),
                                                  ts_out.data_ptr(), mtr_out.ctypes.data, self._stream()), "jackknife_single")
        return ls_out, ts_out, mtr_out

    def profile_begin(self, max_calls):
        """Record HIP events inside the next `max_calls` stack_single calls (start, end of the streaming stage, end)."""
        check(self.lib.tspws_hip_profile_begin(self.h, max_calls), "profile_begin")

    def profile_read(self):
        """(stage_ms[], call_ms[]) of the recorded calls (numpy float64); synchronises the device."""
        import numpy as np
        n = C.c_size_t()
        check(self.lib.tspws_hip_profile_read(self.h, None, None, 0, C.byref(n)), "profile_read")
        st, ca = np.zeros(n.value), np.zeros(n.value)
        check(self.lib.tspws_hip_profile_read(self.h, st.ctypes.data, ca.ctypes.data, n.value, C.byref(n)), "profile_read")
        return st, ca

    def stack_single(self, traces, ls=None, ts=None):
        """Whole call on ONE GPU through tspws_hip_stack (stack_local + stack_finish in one C call)."""
        import torch
        mtr, ld = self._traces(traces)
        ls = torch.empty(self.N, dtype=torch.float32, device=traces.device) if ls is None else ls
        ts = torch.empty(self.N, dtype=torch.float32, device=traces.device) if ts is None else ts
        check(self.lib.tspws_hip_stack(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, self._out(ls, "ls"), self._out(ts, "ts"),
                                       self._stream()), "stack")
        return ls, ts

    def stack_batch(self, traces, first, ls=None, ts=None):
        """B ensembles of one trace array in ONE call (tspws_hip_stack_batch): ensemble b = rows [first[b], first[b+1]) of the float32
        [mtr][N] device tensor `traces`; `first` = B + 1 non-decreasing integer offsets (first[0] may be > 0).  Returns ls[B][N], ts[B][N]
        (float32 cuda): row b = what stack_single gives for ensemble b (an empty ensemble: zero rows)."""
        import torch
        mtr, ld = self._traces(traces)
        f, B, _ = _offsets(first, mtr)
        ls = torch.empty((B, self.N), dtype=torch.float32, device=traces.device) if ls is None else ls
        ts = torch.empty((B, self.N), dtype=torch.float32, device=traces.device) if ts is None else ts
        self._need(ls, "ls", "float32", (B, self.N))
        self._need(ts, "ts", "float32", (B, self.N))
        check(self.lib.tspws_hip_stack_batch(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, ls.data_ptr(), ts.data_ptr(),
                                             self._stream()), "stack_batch")
        return ls, ts

    def stack_batch_bands(self, traces, first, bands, envelope=False):
        """stack_batch with a band-limited finish (tspws_hip_stack_batch_bands): `bands` = R half-open scale ranges (bands_from_frequencies
        makes them from frequency edges).  Returns ls[B][R][N], ts[B][R][N] (float32 cuda) -- row (b, r) = band r's share of ensemble b's
        linear stack and ts-PWS -- and, with envelope=True, also ls_env, ts_env: the envelopes hypot(row, its quadrature).  B = 1 is the
        single-ensemble call.  Empty ensembles and empty bands give zero rows."""
        import torch
        mtr, ld = self._traces(traces)
        f, B, _ = _offsets(first, mtr)
        bt = band_table(bands)
        R = bt.shape[0]
        outs = [torch.full((B, R, self.N), float("nan"), dtype=torch.float32, device=traces.device) for _ in range(4 if envelope else 2)]
        ptr = [t.data_ptr() for t in outs] + [None] * (4 - len(outs))
        check(self.lib.tspws_hip_stack_batch_bands(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, bt.ctypes.data, R, *ptr,
                                                   self._stream()), "stack_batch_bands")
        return tuple(outs)

    def stack_batch_bands_stats(self):
        """The last stack_batch_bands call with B > 0 and R > 0 (tspws_hip_stack_batch_bands_stats): batch_stats' counts, the batches of
        sets of its band finish, the scales with work items and whether the quadrature ran."""
        return self._stats("stack_batch_bands_stats", ("single_pass", "two_stage_pass", "looped", "empty", "rounds", "pass_batches", "finish_batches", "scales", "quadrature"))

    def batch_stats(self):
        """How the last stack_batch call with B > 0 stacked its ensembles (tspws_hip_stack_batch_stats): dict of counts."""
        return self._stats("stack_batch_stats", ("single_pass", "two_stage_pass", "looped", "empty", "rounds", "pass_batches"))

    def _jackknife_batch(self, what, traces, first, sel, ls, ts, ls_out, ts_out, mtr_out, main):
        """Argument checks, output allocation and the call of the batched jackknives (tspws_hip_<what>)."""
        import torch
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        sel = self._sel(sel, T, "selection", "[C][T]")
        Cn = sel.shape[0]
        dev = traces.device
        ls_out, ts_out, mtr_out = self._rows_out((B, Cn), dev, ls_out, ts_out, mtr_out, what=f"{[B, Cn, self.N]} tensor")
        if main:
            ls = torch.empty((B, self.N), dtype=torch.float32, device=dev) if ls is None else ls
            ts = torch.empty((B, self.N), dtype=torch.float32, device=dev) if ts is None else ts
            self._need(ls, "ls", "float32", (B, self.N), f"{[B, self.N]} tensor")
            self._need(ts, "ts", "float32", (B, self.N), f"{[B, self.N]} tensor")
        elif ls is not None or ts is not None:
            raise TspwsError("main=False takes no ls / ts")
        check(getattr(self.lib, "tspws_hip_" + what)(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, sel.ctypes.data, Cn,
                                                     ls.data_ptr() if main else None, ts.data_ptr() if main else None, ls_out.data_ptr(),
                                                     ts_out.data_ptr(), mtr_out.ctypes.data, self._stream()), what)
        return ls, ts, ls_out, ts_out, mtr_out

    def jackknife_batch(self, traces, first, sel, ls=None, ts=None, ls_out=None, ts_out=None, mtr_out=None, main=True):
        """Single-stage jackknife of B ensembles of one trace array in ONE call (tspws_hip_jackknife_batch): ensemble b = rows
        [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`; `sel` = [C][T] int8 selection, T = first[B] - first[0], column
        i - first[0] for trace i (jackknife_selection_batch).  Returns ls[B][N], ts[B][N] (the plain stacks, as stack_batch; None with
        main=False), jk_ls[B][C][N], jk_ts[B][C][N] (float32 cuda) and jk_mtr[B][C] (uint32): block b = what jackknife_single gives for
        ensemble b alone (an empty ensemble: zero rows and counts)."""
        return self._jackknife_batch("jackknife_batch", traces, first, sel, ls, ts, ls_out, ts_out, mtr_out, main)

    def jackknife_batch_stats(self):
        """How the last jackknife_batch call with B > 0 and C > 0 went (tspws_hip_jackknife_batch_stats): dict of counts."""
        return self._stats("jackknife_batch_stats", ("shared", "looped", "empty", "rounds", "pass_batches", "classes"))

    def jackknife_batch_two_stage(self, traces, first, sel, ls=None, ts=None, ls_out=None, ts_out=None, mtr_out=None, main=True):
        """Two-stage jackknife of B ensembles of one trace array in ONE call (tspws_hip_jackknife_batch_two_stage); arguments and return
        tuple as jackknife_batch.  Block b of jk_ls / jk_ts / jk_mtr = what the two-stage tspws_hip_jackknife gives for ensemble b alone with
        its columns of `sel` (K_c = 0: zero rows, count 0), row b of ls / ts = what stack_batch gives for it (None with main=False).  Every
        non-empty ensemble must be two-stage (0 < Kmax <= its traces)."""
        return self._jackknife_batch("jackknife_batch_two_stage", traces, first, sel, ls, ts, ls_out, ts_out, mtr_out, main)

    def jackknife_batch_two_stage_stats(self):
        """How the last jackknife_batch_two_stage call with B > 0 and C > 0 went (tspws_hip_jackknife_batch_two_stage_stats): dict of counts."""
        return self._stats("jackknife_batch_two_stage_stats", ("shared", "looped", "empty", "rounds", "tiles", "rows"))

    def subsample_sel(self, traces, sel, prob=None, ls_out=None, ts_out=None):
        """The random subsamples of ONE ensemble with the masks given (tspws_hip_subsample_sel): `sel` = [M][mtr] int8 masks (1 = kept), every
        row with K = ceil(mtr * subsmpl_p) ones (`prob` replaces the plan's subsmpl_p for this call).  Returns ls_out[M][N], ts_out[M][N]
        (float32 cuda; given or new).  Synchronises."""
        mtr, ld = self._traces(traces)
        sel = self._sel(sel, mtr, "masks", "[M][mtr]")
        Mn = sel.shape[0]
        p = t_tsPWS.from_buffer_copy(self.params)
        if prob is not None:
            p.subsmpl_p = prob
        ls_out, ts_out, _ = self._rows_out((Mn,), traces.device, ls_out, ts_out, counts=False, new="zeros")
        check(self.lib.tspws_hip_subsample_sel(self.h, C.byref(p), traces.data_ptr(), ld, mtr, Mn, sel.ctypes.data, ls_out.data_ptr(), ts_out.data_ptr(),
                                               self._stream()), "subsample_sel")
        return ls_out, ts_out

    def subsample_batch(self, traces, first, sel, ls_out=None, ts_out=None, mtr_out=None):
        """M random subsamples of each of B ensembles of one trace array in ONE call (tspws_hip_subsample_batch_sel): ensemble b = rows
        [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`; `sel` = [M][T] int8 masks (1 = kept; any 0/1 matrix),
        T = first[B] - first[0], column i - first[0] for trace i (subsampling_selection_batch draws them).  Returns ls_out[B][M][N],
        ts_out[B][M][N] (float32 cuda) and mtr_out[B][M] (uint32, the traces every row keeps): block b = what subsample_sel gives for ensemble b
        alone (a row that keeps nothing and an empty ensemble: zero rows, count 0).  Synchronises."""
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        sel = self._sel(sel, T, "masks", "[M][T]")
        Mn = sel.shape[0]
        ls_out, ts_out, mtr_out = self._rows_out((B, Mn), traces.device, ls_out, ts_out, mtr_out)
        check(self.lib.tspws_hip_subsample_batch_sel(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, Mn, sel.ctypes.data,
                                                     ls_out.data_ptr(), ts_out.data_ptr(), mtr_out.ctypes.data, self._stream()), "subsample_batch_sel")
        return ls_out, ts_out, mtr_out

    def subsample_batch_stats(self):
        """How the last subsample_batch call with B > 0 and M > 0 went (tspws_hip_subsample_batch_stats): dict of counts."""
        return self._stats("subsample_batch_stats", ("single_shared", "two_stage_shared", "looped", "empty", "rounds", "rows"))

    def bootstrap_batch(self, traces, first, cnt, ls_out=None, ts_out=None, mtr_out=None, stats=False):
        """M bootstrap replicas of each of B single-stage ensembles of one trace array in ONE call (tspws_hip_bootstrap_batch_cnt): ensemble
        b = rows [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`; `cnt` = [M][T] uint8 counts, T = first[B] - first[0],
        cnt[m][i - first[0]] = how often trace i enters replica m (bootstrap_counts_batch draws them).  Returns ls_out[B][M][N],
        ts_out[B][M][N] (float32 cuda) and mtr_out[B][M] (uint32, the copies every row stacks): row [b][m] = the single-stage subsample of the
        expanded ensemble (trace i repeated cnt[m][i] times) with every copy kept (a row without copies and an empty ensemble: zero rows,
        count 0).  With stats=True a fourth value, float32 cuda [B][4][N]: per sample over the replicas with copies, the mean of ls_out, its
        bootstrap standard error, the mean of ts_out, its standard error.  Two-stage ensembles (0 < Kmax <= traces) are refused.
        Synchronises."""
        import numpy as np
        import torch
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        if not isinstance(cnt, np.ndarray) or cnt.ndim != 2 or cnt.dtype != np.uint8:
            raise TspwsError("counts must be a 2-D uint8 numpy array [M][T]")
        if cnt.shape[1] != T:
            raise TspwsError(f"counts must be [M][{T}] (replica x trace of the batch), got {cnt.shape}")
        cnt = np.ascontiguousarray(cnt)
        Mn = cnt.shape[0]
        ls_out, ts_out, mtr_out = self._rows_out((B, Mn), traces.device, ls_out, ts_out, mtr_out)
        st = torch.empty((B, 4, self.N), dtype=torch.float32, device=traces.device) if stats else None
        check(self.lib.tspws_hip_bootstrap_batch_cnt(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, Mn, cnt.ctypes.data,
                                                     ls_out.data_ptr(), ts_out.data_ptr(), mtr_out.ctypes.data, st.data_ptr() if stats else None,
                                                     self._stream()), "bootstrap_batch_cnt")
        return (ls_out, ts_out, mtr_out, st) if stats else (ls_out, ts_out, mtr_out)

    def bootstrap_batch_stats(self):
        """How the last bootstrap_batch call with B > 0 and M > 0 went (tspws_hip_bootstrap_batch_stats): dict of counts."""
        return self._stats("bootstrap_batch_stats", ("shared", "empty", "rounds", "rows", "max_count"))

    def weighted_stack_batch(self, traces, first, w, ls_out=None, ts_out=None, mtr_out=None):
        """M real-weighted stacks of each of B single-stage ensembles of one trace array in ONE call (tspws_hip_weighted_stack_batch): ensemble
        b = rows [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`; `w` = [M][T] float64 weights >= 0, T = first[B] -
        first[0], w[m][i - first[0]] = the weight of trace i in row m (weights_from_scores makes such rows).  Returns ls_out[B][M][N],
        ts_out[B][M][N] (float32 cuda), mtr_out[B][M] (uint32, the traces with a positive weight) and keff[B][M] (float64, the effective number
        of traces (sum w)^2 / sum w^2): ST = sum w Y, PS = sum w Y / |Y|, coherence |PS| / sum w, the unbiased weight with Keff.  A trace with
        weight 0 takes no part; a row without weight and an empty ensemble give zero rows, count 0 and keff 0; a 0/1 row is subsample_batch's
        row on that mask, bit for bit.  NaN, infinite and negative weights and two-stage ensembles (0 < Kmax <= traces) are refused.
        Synchronises."""
        import numpy as np
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        if not isinstance(w, np.ndarray) or w.ndim != 2 or w.dtype != np.float64:
            raise TspwsError("weights must be a 2-D float64 numpy array [M][T]")
        if w.shape[1] != T:
            raise TspwsError(f"weights must be [M][{T}] (row x trace of the batch), got {w.shape}")
        w = np.ascontiguousarray(w)
        Mn = w.shape[0]
        ls_out, ts_out, mtr_out = self._rows_out((B, Mn), traces.device, ls_out, ts_out, mtr_out)
        keff = np.zeros((B, Mn), np.float64)
        check(self.lib.tspws_hip_weighted_stack_batch(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, Mn, w.ctypes.data,
                                                      ls_out.data_ptr(), ts_out.data_ptr(), mtr_out.ctypes.data, keff.ctypes.data, self._stream()),
              "weighted_stack_batch")
        return ls_out, ts_out, mtr_out, keff

    def weighted_stack_batch_stats(self):
        """How the last weighted_stack_batch call with B > 0 and M > 0 went (tspws_hip_weighted_stack_batch_stats): dict of counts."""
        return self._stats("weighted_stack_batch_stats", ("shared", "empty", "rounds", "rows"))

    def replica_bands(self, rows, q, mtr=None, out=None):
        """Per sample, the quantiles `q` (a sequence of at most 8 probabilities in [0, 1]) over the replicas of each of B ensembles
        (tspws_hip_replica_bands): `rows` = float32 cuda [B][M][N] replica rows (ls_out / ts_out of the batched resampling calls), contiguous
        or with a row stride through a [B][M][ld] base; `mtr` = None or their uint32 [B][M] counts (mtr_out): replica (b, m) takes part iff
        mtr is None or mtr[b][m] > 0.  Returns float32 cuda [B][Q][N] (given as `out` or new): the "linear" quantile of the participating
        replicas, computed in FP64 from the exact order statistics; no participating replica gives zero bands.  Synchronises."""
        import numpy as np
        import torch
        B, Mn, ld = self._strided_rows(rows, kind="replica ")
        try:
            qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
        except (TypeError, ValueError):
            raise TspwsError("q must be a sequence of floats") from None
        if qa.ndim != 1:
            raise TspwsError("q must be a sequence of floats")
        Q = qa.size
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        out = torch.empty((B, Q, self.N), dtype=torch.float32, device=rows.device) if out is None else out
        self._need(out, "out", "float32", (B, Q, self.N))
        check(self.lib.tspws_hip_replica_bands(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, qa.ctypes.data, Q,
                                               out.data_ptr(), self._stream()), "replica_bands")
        return out

    def replica_bands_stats(self):
        """How the last replica_bands call with B, M, Q > 0 went (tspws_hip_replica_bands_stats): dict of counts; lds_max_rows = the largest
        M whose replicas are selected from LDS."""
        return self._stats("replica_bands_stats", ("lds", "global", "empty", "rounds", "lds_max_rows"))

    def _window(self, window):
        """(n0, n1) of a lag window: None = the whole trace, else n0 <= n < n1 (n1 == 0: the trace length)."""
        if window is None:
            return 0, 0
        n0, n1 = (int(v) for v in window)
        if n0 < 0 or n1 < 0:
            raise TspwsError("window must be (n0, n1) with 0 <= n0 < n1 <= N")
        return n0, n1

    def trace_scores(self, traces, first, refs, window=None, energy=False):
        """Similarity, misfit and dot product of every trace of B ensembles against the reference rows of its ensemble
        (tspws_hip_trace_scores): ensemble b = rows [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`; `refs` = float32
        cuda [B][R][N] (1 <= R <= 4) or [B][N] (R = 1), contiguous or a [:, :, :N] view of a wider base; `window` = None or (n0, n1), the
        samples n0 <= n < n1 every sum runs over.  Returns a float64 cuda tensor [R][3][T] -- planes sim, misfit, dot; T = first[B] - first[0],
        column i - first[0] for trace i; sim is NaN for a trace or a reference without energy -- and with energy=True also the traces'
        energies, float64 cuda [T].  The outputs hold NaN before the call (an unwritten entry shows).  Synchronises."""
        import torch
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        if not isinstance(refs, torch.Tensor) or refs.dtype != torch.float32 or refs.dim() not in (2, 3) or refs.shape[-1] != self.N or refs.shape[0] != B:
            raise TspwsError(f"refs must be a float32 [{B}][R][{self.N}] or [{B}][{self.N}] tensor, got {getattr(refs, 'dtype', type(refs))} "
                             f"{tuple(getattr(refs, 'shape', ()))}")
        if refs.dim() == 2:
            refs = refs.unsqueeze(1)
        R = refs.shape[1]
        if not 1 <= R <= 4:
            raise TspwsError(f"1 to 4 reference rows per ensemble, got {R}")
        _, _, ldr = self._strided_rows(refs, "refs", "reference ", "R")
        n0, n1 = self._window(window)
        scores = torch.full((R, 3, T), float("nan"), dtype=torch.float64, device=traces.device)
        en = torch.full((T,), float("nan"), dtype=torch.float64, device=traces.device) if energy else None
        if not T:  # no columns: nothing to call with (an empty tensor has no address)
            return (scores, en) if energy else scores
        check(self.lib.tspws_hip_trace_scores(self.h, traces.data_ptr(), ld, f.ctypes.data, B, refs.data_ptr(), ldr, R, n0, n1, scores.data_ptr(),
                                              en.data_ptr() if energy else None, self._stream()), "trace_scores")
        return (scores, en) if energy else scores

    def trace_scores_stats(self):
        """How the last trace_scores call with traces went (tspws_hip_trace_scores_stats): dict(vec, segments, rounds, empty)."""
        return self._stats("trace_scores_stats", ("vec", "segments", "rounds", "empty"))

    def selective_stack_batch(self, traces, first, against="ts", rule="mad", a=3.0, iters=2, window=None):
        """The selective stack of B ensembles (tspws_hip_selective_stack_batch): stack, score every trace against the ensemble's own
        `against` row ("ls" or "ts"), keep by `rule` ("threshold": sim >= a; "mad": sim >= median - a * 1.4826 * MAD of the ensemble's finite
        scores), restack; up to `iters` restacks, ending early when the mask no longer changes.  Returns (ls[B][N], ts[B][N]) float32 cuda --
        bit for bit the rows of subsample_batch(traces, first, sel[None]) --, sel int8 [T] (the last mask used), kept uint32 [B] and the
        number of restacks.  Synchronises."""
        import numpy as np
        import torch
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        if against not in AGAINST or rule not in RULES:
            raise TspwsError(f"against must be one of {tuple(AGAINST)} and rule one of {tuple(RULES)}, got {against!r}, {rule!r}")
        n0, n1 = self._window(window)
        ls = torch.empty((B, self.N), dtype=torch.float32, device=traces.device)
        ts = torch.empty((B, self.N), dtype=torch.float32, device=traces.device)
        sel = np.zeros(T, np.int8)
        kept = np.zeros(B, np.uint32)
        done = C.c_uint()
        check(self.lib.tspws_hip_selective_stack_batch(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, AGAINST[against],
                                                       RULES[rule], float(a), int(iters), n0, n1, ls.data_ptr(), ts.data_ptr(), sel.ctypes.data,
                                                       kept.ctypes.data, C.byref(done), self._stream()), "selective_stack_batch")
        return ls, ts, sel, kept, done.value

    def stretch_rows(self, rows, ref, z, eps, windows, mtr=None, cc=False, out=None):
        """dv/v by stretching (tspws_hip_stretch_rows): the correlation coefficient of every row of `rows` (float32 cuda [B][M][N], contiguous
        or a [:, :, :N] view of a [B][M][ld] base: ls_out / ts_out of the batched calls) with its ensemble's reference row `ref` (float32 cuda
        [B][N], contiguous or a [:, :N] view) evaluated at lag t (1 + eps), for the strictly increasing stretch factors `eps` (|eps| <= 0.5, at
        most 4096; see stretch_grid) over the 1 to 4 `windows` (n0, n1) of samples n0 <= n < n1; `z` = the zero-lag position in samples.
        `mtr` = None or the rows' uint32 [B][M] counts: row (b, m) takes part iff mtr is None or mtr[b][m] > 0.  Returns the fit plane, float64
        cuda [B][M][W][4] = eps_hat (dv/v), cc_hat, e*, edge; with cc=True the pair (cc [B][M][W][E], fit).  `out` = None, or the tensor(s)
        to write: a contiguous float64 cuda tensor of at least B M W 4 values (cc=True: the pair (cc, fit), cc of at least B M W E values),
        returned as given.  New outputs hold NaN before the call.  Synchronises."""
        import numpy as np
        import torch
        B, Mn, ld = self._strided_rows(rows)
        ldr = self._strided_refs(ref, B)
        try:
            ea = np.ascontiguousarray(np.asarray(eps, dtype=np.float64))
            wa = np.ascontiguousarray(np.asarray(windows, dtype=np.int64))
        except (TypeError, ValueError):
            raise TspwsError("eps must be a sequence of floats, windows a sequence of (n0, n1) pairs") from None
        if ea.ndim != 1 or wa.ndim != 2 or wa.shape[1] != 2 or (wa < 0).any():
            raise TspwsError("eps must be a sequence of floats, windows a sequence of (n0, n1) pairs of non-negative integers")
        wa = np.ascontiguousarray(wa, dtype=np.uint64)  # size_t
        E, W = ea.size, wa.shape[0]
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        o_cc, o_fit = (out if cc else (None, out)) if out is not None else (None, None)
        if out is None:
            o_fit = torch.full((B, Mn, W, 4), float("nan"), dtype=torch.float64, device=rows.device)
            o_cc = torch.full((B, Mn, W, E), float("nan"), dtype=torch.float64, device=rows.device) if cc else None
        self._need(o_fit, "out: fit", "float64", B * Mn * W * 4, "tensor of >= {} values")
        if cc:
            self._need(o_cc, "out: cc", "float64", B * Mn * W * E, "tensor of >= {} values")
        if B and Mn:  # (an empty tensor has no address)
            check(self.lib.tspws_hip_stretch_rows(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, ref.data_ptr(), ldr,
                                                  float(z), ea.ctypes.data, E, wa.ctypes.data, W, o_cc.data_ptr() if cc else None, o_fit.data_ptr(),
                                                  self._stream()), "stretch_rows")
        return (o_cc, o_fit) if cc else o_fit

    def stretch_rows_stats(self):
        """How the last stretch_rows call with B, M > 0 went (tspws_hip_stretch_rows_stats): dict(rounds, segments, rows, left_out, chunks)."""
        return self._stats("stretch_rows_stats", ("rounds", "segments", "rows", "left_out", "chunks"))

    def forward(self, rows):
        """The forward frame transform of float32 cuda rows [ntr][N] (contiguous along the samples; a row stride through a [:, :N] view is
        taken as it is) in ONE tspws_hip_forward_f32 call: the complex128 cuda tensor [ntr][ncoef].  The output holds NaN before the call;
        synchronises."""
        import torch
        ntr, ld = self._traces(rows)
        Y = torch.full((ntr, self.ncoef), complex(float("nan"), float("nan")), dtype=torch.complex128, device=rows.device)
        if ntr:
            check(self.lib.tspws_hip_forward_f32(self.h, rows.data_ptr(), ntr, ld, Y.data_ptr(), self._stream()), "forward")
            torch.cuda.synchronize(rows.device)
        return Y

    def wxs_coef(self, Yc, Yr, z, bands, windows, ens=None, skip_wrapped=False, sums=False, out=None):
        """dv/v per band from the wavelet cross-spectrum of coefficient sets (tspws_hip_wxs_coef): `Yc` [nrow][ncoef] against `Yr` [B][ncoef]
        (complex128, as for inverse: what forward returns), `ens` = None (nrow == B, row i against set i) or the uint32 [nrow] reference set of
        every row.  `z` = the zero-lag position in samples, `bands` = 1 to 64 scale ranges (s_begin, s_end), `windows` = 1 to 4 pairs (n0, n1);
        skip_wrapped leaves out the coefficients whose filter support wraps round the trace ends.  Returns the fit, float64 cuda
        [nrow][W][R][6] = eps_hat (dv/v), icpt, err, rms, coh, n; with sums=True the pair (sums [nrow][W][R][9], fit).  `out` as for
        stretch_rows.  New outputs hold NaN before the call.  Synchronises."""
        import numpy as np
        bt = band_table(bands)
        wa = self._windows(windows)
        Yc, _ = self._coef_sets(Yc, "nrow")
        Yr, _ = self._coef_sets(Yr, "B")
        nrow, B = Yc.shape[0], Yr.shape[0]
        ens = _host_array(ens, "ens", np.uint32, (nrow,), optional=True)
        if ens is None and nrow != B:
            raise TspwsError(f"without ens, Yc and Yr must hold as many sets ({nrow} and {B})")
        R, W = bt.shape[0], wa.shape[0]
        o_sums, o_fit = self._wxs_out((nrow, W, R), sums, out, Yc.device)
        check(self.lib.tspws_hip_wxs_coef(self.h, Yc.data_ptr(), Yr.data_ptr(), ens.ctypes.data if ens is not None else None, nrow, B, float(z),
                                          bt.ctypes.data, R, wa.ctypes.data, W, int(bool(skip_wrapped)), o_sums.data_ptr() if sums else None,
                                          o_fit.data_ptr(), self._stream()), "wxs_coef")
        return (o_sums, o_fit) if sums else o_fit

    def wxs_rows(self, rows, ref, z, bands, windows, mtr=None, skip_wrapped=False, sums=False, out=None):
        """dv/v per band from the wavelet cross-spectrum of rows (tspws_hip_wxs_rows): `rows`, `ref`, `z`, `windows` and `mtr` as for
        stretch_rows, `bands` = 1 to 64 scale ranges (s_begin, s_end) (see bands_from_frequencies).  The rows are transformed on the device in
        rounds of whole ensembles and never leave it.  Returns the fit, float64 cuda [B][M][W][R][6] = eps_hat (dv/v), icpt, err, rms, coh, n
        (rows left out: NaN and n = -1); with sums=True the pair (sums [B][M][W][R][9], fit).  `out` as for stretch_rows.  New outputs hold
        NaN before the call.  Synchronises."""
        import numpy as np
        B, Mn, ld = self._strided_rows(rows)
        ldr = self._strided_refs(ref, B)
        bt = band_table(bands)
        wa = self._windows(windows)
        R, W = bt.shape[0], wa.shape[0]
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        o_sums, o_fit = self._wxs_out((B, Mn, W, R), sums, out, rows.device)
        if B and Mn:  # (an empty tensor has no address)
            check(self.lib.tspws_hip_wxs_rows(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, ref.data_ptr(), ldr,
                                              float(z), bt.ctypes.data, R, wa.ctypes.data, W, int(bool(skip_wrapped)),
                                              o_sums.data_ptr() if sums else None, o_fit.data_ptr(), self._stream()), "wxs_rows")
        return (o_sums, o_fit) if sums else o_fit

    def wxs_rows_stats(self):
        """How the last wxs_rows / wxs_coef call that did work went (tspws_hip_wxs_rows_stats): dict(rounds, rows, left_out, items, scales)."""
        return self._stats("wxs_rows_stats", ("rounds", "rows", "left_out", "items", "scales"))

    def mwcs_rows(self, rows, ref, z, par, windows, mtr=None, win=False, spec=False):
        """dv/v by the moving-window cross-spectrum (tspws_hip_mwcs_rows): `rows`, `ref`, `z`, `windows` (the lag ranges) and `mtr` as for
        stretch_rows, `par` = the parameters (mwcs_par, or a dict of its arguments).  Returns the fit, float64 cuda [B][M][W][6] = eps_hat
        (dv/v), icpt, err_eps, eps0, err0, n (rows left out: NaN and n = -1).  With win=True and / or spec=True a dict: fit, win
        ([B][M][J][3] = delta, err, mcoh per window), spec ([B][M][J][Qx] complex128) and spec_ref ([B][J][Qx]).  New outputs hold NaN
        before the call.  Synchronises."""
        import numpy as np
        import torch
        B, Mn, ld = self._strided_rows(rows)
        ldr = self._strided_refs(ref, B)
        par = par if isinstance(par, MwcsPar) else mwcs_par(**par)
        wa = self._windows(windows)
        W = wa.shape[0]
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        J, Qx = mwcs_windows(par, wa).shape[0], mwcs_qrange(par)[2]
        nan = float("nan")
        o_fit = torch.full((B, Mn, W, 6), nan, dtype=torch.float64, device=rows.device)
        o_win = torch.full((B, Mn, J, 3), nan, dtype=torch.float64, device=rows.device) if win else None
        o_spec = torch.full((B, Mn, J, Qx), complex(nan, nan), dtype=torch.complex128, device=rows.device) if spec else None
        o_sref = torch.full((B, J, Qx), complex(nan, nan), dtype=torch.complex128, device=rows.device) if spec else None
        if B and Mn:  # (an empty tensor has no address)
            check(self.lib.tspws_hip_mwcs_rows(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, ref.data_ptr(), ldr,
                                               float(z), C.addressof(par), wa.ctypes.data, W, o_win.data_ptr() if win else None, o_fit.data_ptr(),
                                               o_spec.data_ptr() if spec else None, o_sref.data_ptr() if spec else None, self._stream()), "mwcs_rows")
        if not win and not spec:
            return o_fit
        return dict(fit=o_fit, win=o_win, spec=o_spec, spec_ref=o_sref)

    def mwcs_rows_stats(self):
        """How the last mwcs_rows call with B, M > 0 went (tspws_hip_mwcs_rows_stats): dict(rounds, rows, left_out, windows, bins)."""
        return self._stats("mwcs_rows_stats", ("rounds", "rows", "left_out", "windows", "bins"))

    def dtw_rows(self, rows, ref, z, par, ranges, mtr=None, lag=True):
        """dv/v by dynamic time warping (tspws_hip_dtw_rows): `rows`, `ref`, `z`, `ranges` (the lag ranges) and `mtr` as for stretch_rows,
        `par` = the parameters (dtw_par, or a dict of its arguments).  Returns a dict: fit, float64 cuda [B][M][W][6] = eps_hat (dv/v), icpt,
        err, rms, dist, clip (rows left out and dead (row, range)s: NaN and clip = -1), and lag, int32 cuda [B][M][T], the integer lag path
        of every range, range after range (INT_MIN where the fit is NaN); with lag=False only the fit.  New outputs hold NaN / INT_MIN
        before the call.  Synchronises."""
        import numpy as np
        import torch
        B, Mn, ld = self._strided_rows(rows)
        ldr = self._strided_refs(ref, B)
        par = par if isinstance(par, DtwPar) else dtw_par(**par)
        wa = self._windows(ranges)
        W = wa.shape[0]
        T = int((wa[:, 1].astype(np.int64) - wa[:, 0].astype(np.int64)).clip(0, 1 << 20).sum())  # (the library judges the ranges)
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        o_fit = torch.full((B, Mn, W, 6), float("nan"), dtype=torch.float64, device=rows.device)
        o_lag = torch.full((B, Mn, T), -2 ** 31, dtype=torch.int32, device=rows.device) if lag else None
        if B and Mn:  # (an empty tensor has no address)
            check(self.lib.tspws_hip_dtw_rows(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, ref.data_ptr(), ldr,
                                              float(z), C.addressof(par), wa.ctypes.data, W, o_lag.data_ptr() if lag else None, o_fit.data_ptr(),
                                              self._stream()), "dtw_rows")
        return dict(fit=o_fit, lag=o_lag) if lag else o_fit

    def dtw_rows_stats(self):
        """How the last dtw_rows call with B, M > 0 went (tspws_hip_dtw_rows_stats): dict(rounds, rows, left_out, lags, samples)."""
        return self._stats("dtw_rows_stats", ("rounds", "rows", "left_out", "lags", "samples"))

    def _ftan_tables(self, windows, noise, scales, B):
        """The host tables of a group-arrival call: (windows uint64 [B][W][2], noise uint64 [B][2] or None, s_begin, s_end).  A (W, 2) window
        array and a (q0, q1) noise pair are broadcast to all B ensembles; scales=None is every scale."""
        import numpy as np
        wa = np.asarray(windows)
        if wa.ndim == 3:
            if wa.shape[0] != B:
                raise TspwsError(f"windows must be (W, 2) or ({B}, W, 2) pairs (n0, n1), got {wa.shape}")
            wa = np.stack([self._windows(w) for w in wa]) if B else np.zeros((0,) + wa.shape[1:], np.uint64)
        else:
            one = self._windows(windows)
            wa = np.broadcast_to(one, (B,) + one.shape)
        wa = np.ascontiguousarray(wa, dtype=np.uint64)
        na = None
        if noise is not None:
            na = np.asarray(noise)
            if na.shape not in ((2,), (B, 2)) or na.dtype.kind not in "iu" or (na < 0).any():
                raise TspwsError(f"noise must be None, a pair (q0, q1) or ({B}, 2) pairs of non-negative integers")
            na = np.ascontiguousarray(np.broadcast_to(na, (B, 2)), dtype=np.uint64)
        try:
            s0, s1 = (0, self.S) if scales is None else (int(scales[0]), int(scales[1]))
        except (TypeError, ValueError, IndexError):
            raise TspwsError("scales must be None or a pair (s_begin, s_end)") from None
        if not 0 <= s0 <= 0xFFFFFFFF or not 0 <= s1 <= 0xFFFFFFFF:
            raise TspwsError("scales must be None or a pair (s_begin, s_end) of non-negative integers")
        return wa, na, s0, s1

    def _ftan_out(self, lead, W, Sx, P, noise, out, device):
        """(peaks, noise or None) of a group-arrival call, given as `out` or new (NaN-filled): float64 tensors of at least
        prod(lead) W Sx P 5 / prod(lead) Sx 2 values."""
        import torch
        n = 1
        for k in lead:
            n *= k
        Sx, P = max(Sx, 0), max(int(P), 0)
        o_peaks, o_noise = (out if noise else (out, None)) if out is not None else (None, None)
        if out is None:
            o_peaks = torch.full((*lead, W, Sx, P, 5), float("nan"), dtype=torch.float64, device=device)
            o_noise = torch.full((*lead, Sx, 2), float("nan"), dtype=torch.float64, device=device) if noise else None
        self._need(o_peaks, "out: peaks", "float64", n * W * Sx * P * 5, "tensor of >= {} values")
        if noise:
            self._need(o_noise, "out: noise", "float64", n * Sx * 2, "tensor of >= {} values")
        return o_peaks, o_noise

    def ftan_coef(self, Y, z, windows, scales=None, P=1, noise=None, ens=None, B=None, skip_wrapped=False, out=None):
        """Group arrivals per scale from coefficient sets (tspws_hip_ftan_coef): `Y` [nrow][ncoef] (complex128, as for inverse: what forward
        returns); `ens` = None (row i is ensemble i) or the uint32 [nrow] ensemble of every row, of `B` ensembles (None: max(ens) + 1).  `z` =
        the zero-lag position in samples; `windows` = 1 to 4 pairs (n0, n1) for all ensembles, or [B][W][2] (see ftan_windows); `scales` =
        (s_begin, s_end), None for all; `P` = 1 to 4 peaks; `noise` = None, a pair (q0, q1) or [B][2]; skip_wrapped leaves out the
        coefficients whose filter support wraps round the trace ends.  Returns the peaks, float64 cuda [nrow][W][Sx][P][5] = tg (the group
        arrival as a lag in samples), amp, re, im, k (unused slots: NaN and k = -1); with `noise` the pair (peaks, noise [nrow][Sx][2] = Q, n).
        `out` as for wxs_rows.  New outputs hold NaN before the call.  Synchronises."""
        import numpy as np
        Y, _ = self._coef_sets(Y, "nrow")
        nrow = Y.shape[0]
        ens = _host_array(ens, "ens", np.uint32, (nrow,), optional=True)
        B = (nrow if ens is None else int(ens.max()) + 1) if B is None else int(B)
        wa, na, s0, s1 = self._ftan_tables(windows, noise, scales, B)
        W = wa.shape[1]
        o_peaks, o_noise = self._ftan_out((nrow,), W, s1 - s0, P, na is not None, out, Y.device)
        check(self.lib.tspws_hip_ftan_coef(self.h, Y.data_ptr(), ens.ctypes.data if ens is not None else None, nrow, B, float(z), s0, s1, wa.ctypes.data, W,
                                           na.ctypes.data if na is not None else None, int(P), int(bool(skip_wrapped)), o_peaks.data_ptr(),
                                           o_noise.data_ptr() if na is not None else None, self._stream()), "ftan_coef")
        return (o_peaks, o_noise) if na is not None else o_peaks

    def ftan_rows(self, rows, z, windows, scales=None, P=1, noise=None, mtr=None, skip_wrapped=False, out=None):
        """Group arrivals per scale from rows (tspws_hip_ftan_rows): `rows`, `z` and `mtr` as for wxs_rows (the [B][M][N] rows the batched
        calls leave and their counts), the other arguments as for ftan_coef.  The rows are transformed on the device in rounds of whole
        ensembles and never leave it.  Returns the peaks, float64 cuda [B][M][W][Sx][P][5] = tg, amp, re, im, k (unused slots and rows left
        out: NaN and k = -1); with `noise` the pair (peaks, noise [B][M][Sx][2] = Q, n; rows left out: NaN and -1).  The M replicas of an
        ensemble give the arrival's spread.  `out` as for wxs_rows.  New outputs hold NaN before the call.  Synchronises."""
        import numpy as np
        B, Mn, ld = self._strided_rows(rows)
        wa, na, s0, s1 = self._ftan_tables(windows, noise, scales, B)
        W = wa.shape[1]
        mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
        o_peaks, o_noise = self._ftan_out((B, Mn), W, s1 - s0, P, na is not None, out, rows.device)
        if B and Mn:  # (an empty tensor has no address)
            check(self.lib.tspws_hip_ftan_rows(self.h, rows.data_ptr(), ld, B, Mn, mtr.ctypes.data if mtr is not None else None, float(z), s0, s1,
                                               wa.ctypes.data, W, na.ctypes.data if na is not None else None, int(P), int(bool(skip_wrapped)),
                                               o_peaks.data_ptr(), o_noise.data_ptr() if na is not None else None, self._stream()), "ftan_rows")
        return (o_peaks, o_noise) if na is not None else o_peaks

    def ftan_rows_stats(self):
        """How the last ftan_rows / ftan_coef call that did work went (tspws_hip_ftan_rows_stats): dict(rounds, rows, left_out, items, classes)."""
        return self._stats("ftan_rows_stats", ("rounds", "rows", "left_out", "items", "classes"))

    def filter_coef(self, Y, PS, K, ens=None, loo=False, out=None):
        """The stack's coherence weight applied to coefficient sets (tspws_hip_filter_coef): `Y` [nrow][ncoef] and `PS` [B][ncoef]
        (complex128, as for inverse), `K` = the uint32 [B] counts, `ens` = None (nrow == B, row i of ensemble i) or the uint32 [nrow] ensemble
        of every row; wu and unbiased are the plan's parameters.  loo=True filters row i with the weight of PS - u_i and K - 1.  Returns
        Y W as a complex128 cuda tensor [nrow][ncoef]: new (NaN before the call) or `out` as given; out=Y (the same device tensor) works in
        place.  Synchronises."""
        import numpy as np
        import torch
        Yd, _ = self._coef_sets(Y, "nrow")
        PSd, _ = self._coef_sets(PS, "B")
        nrow, B = Yd.shape[0], PSd.shape[0]
        K = _host_array(K, "K", np.uint32, (B,))
        ens = _host_array(ens, "ens", np.uint32, (nrow,), optional=True)
        if ens is None and nrow != B:
            raise TspwsError(f"without ens, Y and PS must hold as many sets ({nrow} and {B})")
        if out is not None and out is Y:  # in place: d_out == NULL
            o = None
        else:
            o = torch.full((nrow, self.ncoef), complex(float("nan"), float("nan")), dtype=torch.complex128, device=Yd.device) if out is None else out
            self._need(o, "out", "complex128", (nrow, self.ncoef))
        p = self.params
        check(self.lib.tspws_hip_filter_coef(self.h, Yd.data_ptr(), ens.ctypes.data if ens is not None else None, nrow, PSd.data_ptr(), K.ctypes.data, B,
                                             float(p.wu), int(p.unbiased), int(bool(loo)), o.data_ptr() if o is not None else None, self._stream()),
              "filter_coef")
        return Yd if o is None else o

    def filter_traces(self, traces, first, rows=None, mtr=None, loo=False, out=None):
        """The stack's coherence filter per trace (tspws_hip_filter_traces): x~_i = ICWT(Y_i W_b), W_b the weight that the stack of ensemble b
        = rows [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces` applies to its linear stack.  Targets: the ensembles' own
        traces -- returns float32 cuda [T][N], T = first[B] - first[0], row i - first[0] = trace i filtered --, or `rows` (float32 cuda
        [B][M][N] as for stretch_rows, with `mtr` = None or their uint32 [B][M] counts: a count of 0 leaves the row out) -- returns [B][M][N].
        loo=True (trace targets, single-stage ensembles): trace i is filtered without its own phasor.  Rows left out hold NaN.  `out` = None or
        the contiguous float32 cuda tensor of that shape to write; a new output holds NaN before the call.  The mean of an ensemble's filtered
        traces is its ts row of stack_batch.  Synchronises."""
        import numpy as np
        import torch
        ntr, ld = self._traces(traces)
        f, B, T = _offsets(first, ntr)
        if rows is None:
            if mtr is not None:
                raise TspwsError("mtr needs rows")
            shape, ldr, Mn = (T, self.N), 0, 0
        else:
            Br, Mn, ldr = self._strided_rows(rows)
            if Br != B:
                raise TspwsError(f"rows must hold the B = {B} ensembles of first, got {Br}")
            mtr = _host_array(mtr, "mtr", np.uint32, (B, Mn), optional=True)
            shape = (B, Mn, self.N)
        o = torch.full(shape, float("nan"), dtype=torch.float32, device=traces.device) if out is None else out
        self._need(o, "out", "float32", shape)
        if B and o.numel():  # (an empty tensor has no address)
            check(self.lib.tspws_hip_filter_traces(self.h, C.byref(self.params), traces.data_ptr() if ntr else None, ld, f.ctypes.data, B,
                                                   rows.data_ptr() if rows is not None else None, ldr, Mn, mtr.ctypes.data if mtr is not None else None,
                                                   int(bool(loo)), o.data_ptr(), self.N, self._stream()), "filter_traces")
        return o

    def filter_traces_stats(self):
        """How the last filter_traces / filter_coef call that did work went (tspws_hip_filter_traces_stats): dict(rounds, rows, left_out,
        single_stage, two_stage, empty, twice)."""
        return self._stats("filter_traces_stats", ("rounds", "rows", "left_out", "single_stage", "two_stage", "empty", "twice"))

    def convergence(self, traces, ref_ts, ref_ls, steps=False):
        """Convergence curves of ONE ensemble (tspws_hip_convergence) on device tensors: `traces` float32 [mtr][N], `ref_ts` / `ref_ls`
        float32 [N] references of the ts-PWS / linear curve.  Returns (ts_sim, ts_misfit, ls_sim, ls_misfit) as float64 numpy [mtr]; with
        steps=True also the [mtr][N] float32 cuda tensors of every step's ts-PWS and linear stack.  Synchronises."""
        import numpy as np
        import torch
        mtr, ld = self._traces(traces)
        r_ts, r_ls = self._refs(ref_ts, "ref_ts", 1), self._refs(ref_ls, "ref_ls", 1)
        cur = [np.full(mtr, np.nan) for _ in range(4)]
        st = [torch.full((mtr, self.N), float("nan"), dtype=torch.float32, device=traces.device) for _ in range(2)] if steps else [None, None]
        check(self.lib.tspws_hip_convergence(self.h, C.byref(self.params), traces.data_ptr(), ld, mtr, r_ts, r_ls, *[c.ctypes.data for c in cur],
                                             *[t.data_ptr() if steps else None for t in st], self._stream()), "convergence")
        return (*cur, *st) if steps else tuple(cur)

    def convergence_batch(self, traces, first, ref_ts=None, ref_ls=None, steps=False):
        """Convergence curves of B ensembles of one trace array in ONE call (tspws_hip_convergence_batch): ensemble b = rows
        [first[b], first[b+1]) of the float32 [mtr][N] device tensor `traces`, `first` = B + 1 non-decreasing integer offsets (first[0] may be
        > 0), T = first[B] - first[0].  `ref_ts` / `ref_ls`: float32 [B][N] cuda, row b = the reference of ensemble b; None (both): the rows of
        stack_batch(traces, first) -- every ensemble against its own final stacks.  Returns (ts_sim, ts_misfit, ls_sim, ls_misfit) as float64
        numpy [T], entry i - first[0] for trace i: what `convergence` gives for each ensemble alone; with steps=True also the two [T][N]
        float32 cuda tensors.  Arrays and tensors hold NaN before the call (an unwritten entry shows).  Synchronises."""
        import numpy as np
        import torch
        mtr, ld = self._traces(traces)
        f, B, T = _offsets(first, mtr)
        if (ref_ts is None) != (ref_ls is None):
            raise TspwsError("ref_ts and ref_ls are given together or not at all")
        if ref_ts is None:
            ref_ls, ref_ts = self.stack_batch(traces, f)
        r_ts, r_ls = self._refs(ref_ts, "ref_ts", B), self._refs(ref_ls, "ref_ls", B)
        cur = [np.full(T, np.nan) for _ in range(4)]
        st = [torch.full((T, self.N), float("nan"), dtype=torch.float32, device=traces.device) for _ in range(2)] if steps else [None, None]
        check(self.lib.tspws_hip_convergence_batch(self.h, C.byref(self.params), traces.data_ptr(), ld, f.ctypes.data, B, r_ts, r_ls,
                                                   *[c.ctypes.data for c in cur], *[t.data_ptr() if steps else None for t in st], self._stream()),
              "convergence_batch")
        return (*cur, *st) if steps else tuple(cur)

    def convergence_batch_stats(self):
        """How the last convergence_batch call with traces went (tspws_hip_convergence_batch_stats): dict of counts."""
        return self._stats("convergence_batch_stats", ("single_steps", "two_stage_steps", "rows", "rounds", "looped", "empty"))

    def close(self):
        if getattr(self, "h", None):
            self.lib.tspws_hip_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SCHEDULES = ("single", "split", "sharded-finish")
# tspws_selection_from_scores' rules and the selective stack's reference row, by name
RULES = {"threshold": 0, "mad": 1}
AGAINST = {"ls": 0, "ts": 1}


def stack_sharded(plan, traces, first=0, mtr_global=None, group=None, schedule=None):
    """One tspws_main-equivalent call over a trace-sharded ensemble.

    Every rank holds a contiguous shard `traces` whose first row is global trace `first` of
    `mtr_global`.  The shard-local half produces a sum over traces (two-stage: the Kmax partial
    stacks, group index taken from the GLOBAL trace index; single-stage: ST||PS); ONE all-reduce
    (RCCL over xGMI on GPUs, backend "nccl") adds the shards; every rank then finishes (K forward
    CWTs, weight, two inverses) redundantly -- that part is tiny.  With world_size 1 (or no process
    group) there is no collective at all.  `plan` only needs stack_local / reduce_buffer /
    stack_finish / N, so the CPU tests drive the same orchestration with an oracle-backed plan.

    `schedule` (N > 1, two-stage; default: $TSPWS_SCHEDULE or "single") -- three ways to place the one logical
    reduction of P[Kmax][N], selectable so that a multi-GPU node can A/B them (bench.py --schedule):
      "single"          north_star's wording: local half, ONE all-reduce of the whole buffer, redundant finish on every rank
                        (bit-identical to the one-GPU result when the shards add exactly);
      "split"           the groups in two pieces K/2 | K/2: the first reduction runs while the second piece is streamed, the
                        second while the first half of the groups is transformed (redundant finish in pieces);
      "sharded-finish"  pieces K-2 | 2, then every rank finishes only its share of the scales and a 2 N-double all-reduce adds
                        the partial reconstructions (falls back to "split" when the plan has no sharded finish)."""
    import torch
    import torch.distributed as dist
    mtr_global = traces.shape[0] if mtr_global is None else mtr_global
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    K = getattr(getattr(plan, "params", None), "Kmax", 0)
    schedule = schedule or os.environ.get("TSPWS_SCHEDULE") or "single"
    if schedule not in SCHEDULES:
        raise TspwsError(f"schedule must be one of {SCHEDULES}, got {schedule!r}")
    if distributed and schedule != "single" and callable(getattr(plan, "partial_stacks_range", None)) and K >= 2 and K <= mtr_global:
        # two-stage: the sum is row-separable, so the all-reduce of the first half of the groups runs (on the collective's
        # own stream) while the second half is still being streamed -- still one logical reduction of P[Kmax][N]
        shard = _finish_shard(plan, mtr_global, group) if schedule == "sharded-finish" else None
        half = split_groups(K, shard is not None)
        buf = plan.reduce_buffer(mtr_global).view(K, plan.N)
        plan.partial_stacks_range(traces, first, mtr_global, 0, half)
        w1 = dist.all_reduce(buf[:half], op=dist.ReduceOp.SUM, group=group, async_op=True)
        plan.partial_stacks_range(traces, first, mtr_global, half, K)
        w2 = dist.all_reduce(buf[half:], op=dist.ReduceOp.SUM, group=group, async_op=True)
        ls = torch.empty(plan.N, dtype=torch.float32, device=traces.device)
        ts = torch.empty(plan.N, dtype=torch.float32, device=traces.device)
        if shard is not None:
            # scale-sharded finish: every rank transforms / weights / reconstructs only its share of the scales of the
            # reduced partial stacks; the partial reconstructions (2 N doubles) are added and every rank ends with the outputs
            w1.wait()
            w2.wait()
            x2 = torch.empty(2 * plan.N, dtype=torch.float64, device=traces.device)
            plan.stack_finish_scales(mtr_global, shard[0], shard[1], x2)
            dist.all_reduce(x2, op=dist.ReduceOp.SUM, group=group)
            plan.epilogue(x2, mtr_global, ls, ts)
            return ls, ts
        w1.wait()
        if callable(getattr(plan, "stack_finish_range", None)):
            # the transforms of the first half of the groups run while the second half is still being reduced
            plan.stack_finish_range(mtr_global, 0, half)
            w2.wait()
            plan.stack_finish_range(mtr_global, half, K)
            plan.stack_finish_tail(mtr_global, ls, ts)
        else:
            w2.wait()
            plan.stack_finish(mtr_global, ls, ts)
        return ls, ts
    plan.stack_local(traces, first, mtr_global)
    if distributed:
        dist.all_reduce(plan.reduce_buffer(mtr_global), op=dist.ReduceOp.SUM, group=group)
    ls = torch.empty(plan.N, dtype=torch.float32, device=traces.device)
    ts = torch.empty(plan.N, dtype=torch.float32, device=traces.device)
    plan.stack_finish(mtr_global, ls, ts)
    return ls, ts


def jackknife_sharded(plan, traces, sel, first=0, mtr_global=None, group=None):
    """Two-stage stack AND its jackknife replicas over a trace-sharded ensemble ("Jackknife sharding").

    `sel` is the [C][mtr_global] selection of the whole ensemble (tspws_jackknife_plan), identical on every rank.  Each rank
    walks its shard ONCE (plan.jackknife_local): the sums of its traces for the Kmax plain groups and for the Kmax groups of
    every replica -- group indices come from the GLOBAL trace order, so the shards' rows simply add.  The plain rows are
    all-reduced and every rank finishes the stack (as in stack_sharded).  The replicas are SHARDED for the finish stage,
    which is where their time goes (Kmax transforms + an inverse each): rank r owns the contiguous block of replicas
    [r C / world, (r + 1) C / world), their rows are reduced to that rank only (one reduction per owner instead of one
    all-reduce of all C x Kmax rows on every rank), the owner finishes its block in one batched call, and one all-reduce of
    the [C][N] float outputs (zeros from the non-owners: exact) hands every rank all replicas.  Returns ls, ts, ls_out[C][N], ts_out[C][N], mtr_out[C]."""
    import numpy as np
    import torch
    import torch.distributed as dist
    mtr_global = traces.shape[0] if mtr_global is None else mtr_global
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    sel = np.ascontiguousarray(sel, dtype=np.int8)
    Cn = sel.shape[0]
    K, N = plan.params.Kmax, plan.N
    plan.jackknife_local(traces, first, mtr_global, sel)
    dev = traces.device
    ls = torch.empty(N, dtype=torch.float32, device=dev)
    ts = torch.empty(N, dtype=torch.float32, device=dev)
    ls_out = torch.zeros((Cn, N), dtype=torch.float32, device=dev)
    ts_out = torch.zeros((Cn, N), dtype=torch.float32, device=dev)
    mtr_out = np.zeros(Cn, np.uint32)
    # replica c belongs to the rank whose CONTIGUOUS block [r * C // world, (r + 1) * C // world) holds it: one reduction per
    # owner covers all its rows, and the owner finishes its block in one batched call (forward launch, inverses in pairs)
    def block(r):
        return r * Cn // world, (r + 1) * Cn // world
    works = []
    if distributed:
        rows = plan.jackknife_buffer(Cn).view(Cn, K * N)
        works.append(dist.all_reduce(plan.reduce_buffer(mtr_global), op=dist.ReduceOp.SUM, group=group, async_op=True))
        for r in range(world):
            c0, c1 = block(r)
            if c1 > c0:
                works.append(dist.reduce(rows[c0:c1], dst=dist.get_global_rank(group, r) if group is not None else r, op=dist.ReduceOp.SUM,
                                         group=group, async_op=True))
    for w in works[:1]:
        w.wait()
    plan.stack_finish(mtr_global, ls, ts)  # runs while the replicas' rows are still being reduced
    for w in works[1:]:
        w.wait()
    c0, c1 = block(rank)
    if c1 > c0:
        plan.jackknife_finish(mtr_global, sel, c0, c1, ls_out, ts_out, mtr_out)
    if distributed:
        dist.all_reduce(ls_out, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(ts_out, op=dist.ReduceOp.SUM, group=group)
        cnt = torch.from_numpy(mtr_out.astype(np.int64)).to(dev)
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
        mtr_out = cnt.cpu().numpy().astype(np.uint32)
    return ls, ts, ls_out, ts_out, mtr_out


def _finish_shard(plan, mtr_global, group=None):
    """This rank's share of the scales for the sharded finish stage, or None (plan without one, world 1, TSPWS_SHARD_FINISH=0).
    The decision is AGREED across the ranks: each one looks at its own environment and plan, so a rank that would not shard
    (a different TSPWS_SHARD_FINISH, a check-kernel switch) would otherwise issue a different sequence of collectives and
    hang the job -- one MIN all-reduce of a flag makes every rank take the redundant finish unless all of them can shard."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if world < 2:
        return None
    # agreed once per (group, ensemble size, frame): no collective in later calls.  The cache is module-level and keyed by the
    # frame's parameters, not by the plan object: a rank that rebuilds its plan hits the same entry as the ranks that kept
    # theirs, so the ranks cannot diverge into different collective sequences.
    pr = getattr(plan, "params", None)
    frame = (pr.type, pr.J, pr.V, pr.s0, pr.b0, pr.w0, int(pr.uni), pr.Kmax) if pr is not None else (id(plan),)
    # keyed on the process group AND on torch's count of groups created so far (it grows with every init_process_group / new_group, on
    # every rank alike): after destroy + init the id of the old group object may be reused, but the count has moved on, so all ranks miss
    # together and repeat the agreement collective -- no rank skips a collective that a peer still issues.  (No reference to the group is
    # kept: a process group held by a module-level table is torn down at interpreter exit with its threads still running.)
    try:
        gen = dist.distributed_c10d._world.group_count
    except Exception:
        gen = None
    key = (id(group) if group is not None else None, gen, world, dist.get_rank(group), mtr_global, getattr(plan, "N", 0), frame,
           os.environ.get("TSPWS_SHARD_FINISH", "1"))
    if gen is not None and key in _SHARD_AGREED:
        return _SHARD_AGREED[key]
    mine = None
    if os.environ.get("TSPWS_SHARD_FINISH", "1") != "0" and callable(getattr(plan, "finish_shard", None)):
        mine = plan.finish_shard(mtr_global, dist.get_rank(group), world)
    # the flag lives on the PLAN's device (not torch's current device: a caller that never ran torch.cuda.set_device would put
    # every rank's tensor on cuda:0 and RCCL would hang)
    dev = f"cuda:{getattr(plan, 'device', 0)}" if dist.get_backend(group) == "nccl" else "cpu"
    flag = torch.tensor([1 if mine is not None else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    agreed = mine if int(flag.item()) == 1 else None
    _SHARD_AGREED[key] = agreed
    return agreed


_SHARD_AGREED = {}


def split_groups(K, sharded_finish=False):
    """First piece of the two-piece streaming / reduction schedule.  Redundant finish: about half the groups -- the second
    reduction then hides behind the transforms of the first half.  Scale-sharded finish (nothing to hide behind): all but
    the last two groups, so that only a small reduction is left exposed.  EVEN when possible -- the streaming pass
    launches the groups two at a time (one workgroup per CU at N = 131072), so an odd piece would end on a launch that
    fills half the CUs."""
    half = K - 2 if (sharded_finish and K > 3) else K // 2
    if half >= 2 and half % 2:
        half -= 1
    return half


def _as_tensor(ptr, count, dtype, device):
    """Zero-copy torch view of library-owned device memory (via __cuda_array_interface__)."""
    import torch
    typestr = {torch.float64: "<f8", torch.float32: "<f4"}[dtype]

    class _Holder:
        __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}

    return torch.as_tensor(_Holder(), device=f"cuda:{device}")


def jackknife_selection(times, n, d):
    """Delete-d jackknife selection [C][mtr] (int8, 1 = kept), C = binomial(n, d), from trace start times (seconds since 1970;
    day-of-year bins, tspws_jackknife_plan).  Raises when there are no start times (times[0] == 0)."""
    import math
    import numpy as np
    times = np.ascontiguousarray(times, dtype=np.int64)
    if times.ndim != 1 or not times.size:
        raise TspwsError("times must be a non-empty 1-D array of start times")
    if not 0 < d < n:
        raise TspwsError(f"jackknife needs 0 < d < n, got n = {n}, d = {d}")
    Cn = math.comb(n, d)
    sel = np.zeros((Cn, times.size), np.int8)
    rc = load().tspws_jackknife_plan(sel.ctypes.data, times.ctypes.data, times.size, d, n, Cn)
    if rc:
        raise TspwsError("jackknife_selection: no trace start times" if rc == -2 else f"jackknife_selection failed with code {rc}")
    return sel


def jackknife_selection_batch(times, first, n, d):
    """Delete-d jackknife selection [C][T] (int8, 1 = kept) of B ensembles for Plan.jackknife_batch: times[i] = start time of trace i,
    ensemble b = traces [first[b], first[b+1]), T = first[B] - first[0]; the columns of every ensemble come from one tspws_jackknife_plan call
    on that ensemble's own start times (an empty ensemble has no columns).  Raises when an ensemble's first start time is 0."""
    import math
    import numpy as np
    times = np.ascontiguousarray(times, dtype=np.int64)
    if times.ndim != 1:
        raise TspwsError("times must be 1-D start times")
    f, _, _ = _offsets(first, times.size, "start times")
    if not 0 < d < n:
        raise TspwsError(f"jackknife needs 0 < d < n, got n = {n}, d = {d}")
    Cn = math.comb(n, d)
    f0 = int(f[0])
    sel = np.zeros((Cn, int(f[-1]) - f0), np.int8)
    for b in range(f.size - 1):
        a, e = int(f[b]), int(f[b + 1])
        if e > a:
            sel[:, a - f0:e - f0] = jackknife_selection(times[a:e], n, d)
    return sel


def subsampling_selection_batch(first, M, prob):
    """Random-subsampling masks of a batch (tspws_subsampling_plan_batch): int8 [M][T], T = first[-1] - first[0]; for every ensemble in order
    and every mask in order, ceil(M_b * prob) of the ensemble's columns of that row are 1, drawn with libc rand() in the order of a loop of
    single calls over the ensembles."""
    import numpy as np
    f, B, T = _offsets(first)
    if not 0 <= prob <= 1:
        raise TspwsError("prob must lie in [0, 1]")
    sel = np.zeros((int(M), T), np.int8)
    if load().tspws_subsampling_plan_batch(sel.ctypes.data, f.ctypes.data, B, int(M), float(prob)):
        raise TspwsError("tspws_subsampling_plan_batch refused its arguments")
    return sel


def bootstrap_counts_batch(first, M):
    """Bootstrap counts of a batch (tspws_bootstrap_plan_batch): uint8 [M][T], T = first[-1] - first[0]; for every ensemble in order and every
    replica in order, M_b draws with replacement among the ensemble's columns of that row (its counts sum to M_b), drawn with libc rand()
    in the order of a loop over the ensembles."""
    import numpy as np
    f, B, T = _offsets(first)
    cnt = np.zeros((int(M), T), np.uint8)
    if load().tspws_bootstrap_plan_batch(cnt.ctypes.data, f.ctypes.data, B, int(M)):
        raise TspwsError("tspws_bootstrap_plan_batch refused its arguments")
    return cnt


def selection_from_scores(score, first, rule, a):
    """One mask row from one plane of scores (tspws_selection_from_scores): `score` = float64 [T] (usually the sim plane of one reference,
    T = first[-1] - first[0]), `rule` = "threshold" / 0 (keep iff score >= a) or "mad" / 1 (per ensemble over its finite scores: keep iff
    score >= median - a * 1.4826 * MAD).  NaN is never kept.  Returns (sel int8 [T], kept uint32 [B])."""
    import numpy as np
    f, B, T = _offsets(first)
    sc = _score_plane(score, T)
    r = RULES.get(rule, rule)
    if r not in (0, 1):
        raise TspwsError(f"rule must be one of {tuple(RULES)} (or 0 / 1), got {rule!r}")
    sel = np.zeros(T, np.int8)
    kept = np.zeros(B, np.uint32)
    rc = load().tspws_selection_from_scores(sel.ctypes.data, kept.ctypes.data, sc.ctypes.data, f.ctypes.data, B, int(r), float(a))
    if rc:
        raise TspwsError(f"tspws_selection_from_scores refused its arguments (code {rc})")
    return sel, kept


def stretch_grid(eps_max, E):
    """The symmetric stretch grid of tspws_stretch_grid: float64 [E], eps[e] = (e - h) * (eps_max / h), h = (E - 1) / 2; E odd and >= 3,
    0 < eps_max <= 0.5.  The middle entry is exactly 0."""
    import numpy as np
    eps = np.zeros(max(int(E), 0), np.float64)
    rc = load().tspws_stretch_grid(eps.ctypes.data, float(eps_max), int(E)) if 0 <= int(E) < 2 ** 32 else 2
    if rc:
        raise TspwsError(f"tspws_stretch_grid refused its arguments (code {rc}): E odd and >= 3, 0 < eps_max <= 0.5")
    return eps


class MwcsPar(C.Structure):
    """tspws_mwcs_par"""
    _fields_ = [("L", C.c_uint), ("hop", C.c_uint), ("P", C.c_uint), ("q0", C.c_uint), ("q1", C.c_uint), ("h", C.c_uint), ("taper", C.c_double),
                ("min_coh", C.c_double), ("max_err", C.c_double), ("max_delta", C.c_double), ("err_floor", C.c_double)]


def mwcs_par(L, hop, P, q0, q1, h=0, taper=0.0, min_coh=0.0, max_err=float("inf"), max_delta=float("inf"), err_floor=1e-6):
    """The parameters of Plan.mwcs_rows (tspws_mwcs_par): window length, hop and DFT length in samples, the band [q0, q1) in DFT bins (see
    mwcs_bins), the smoothing half-width in bins, the taper fraction and the filters of the regression on the lag.  The library judges them."""
    try:
        return MwcsPar(int(L), int(hop), int(P), int(q0), int(q1), int(h), float(taper), float(min_coh), float(max_err), float(max_delta), float(err_floor))
    except (TypeError, ValueError, OverflowError):
        raise TspwsError("mwcs_par: L, hop, P, q0, q1, h must be non-negative integers below 2^32, the rest floats") from None


def mwcs_bins(P, dt, f_lo, f_hi):
    """(q0, q1) of tspws_mwcs_bins: the DFT bins of length P with f_lo <= q / (P dt) < f_hi, without bin 0 and below P / 2."""
    q0, q1 = C.c_uint(0), C.c_uint(0)
    rc = load().tspws_mwcs_bins(int(P), float(dt), float(f_lo), float(f_hi), C.byref(q0), C.byref(q1)) if 0 <= int(P) < 2 ** 32 else 2
    if rc:
        raise TspwsError(f"tspws_mwcs_bins refused its arguments (code {rc}): P a power of two in [16, 4096], dt > 0, 0 <= f_lo < f_hi, two bins or more")
    return q0.value, q1.value


def mwcs_qrange(par):
    """(qa, qb, Qx) of the parameters: the band with its smoothing margins, [max(0, q0 - h), min(P / 2 + 1, q1 + h))."""
    qa, qb = max(0, par.q0 - par.h), min(par.P // 2 + 1, par.q1 + par.h)
    return qa, qb, qb - qa


def mwcs_windows(par, windows):
    """The windows of the lag ranges, int64 [J][2] = (first sample, range): range w = (n0, n1) holds the windows n0 + j hop while they end
    at or before n1, numbered range after range."""
    import numpy as np
    out = [(n, w) for w, (n0, n1) in enumerate(np.asarray(windows, dtype=np.int64).reshape(-1, 2).tolist())
           for n in range(n0, n1 - par.L + 1, max(par.hop, 1))]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def mwcs_basis(par):
    """The table of tspws_mwcs_basis as a dict of float64 arrays: g [L], C and S [L][Qx], Tc and Ts [Qx], k [2 h + 1], v [Qx]."""
    import numpy as np
    par = par if isinstance(par, MwcsPar) else mwcs_par(**par)
    lib = load()
    n = lib.tspws_mwcs_basis_size(C.addressof(par))
    if not n:
        raise TspwsError("tspws_mwcs_basis refused the parameters")
    tab = np.empty(n, np.float64)
    rc = lib.tspws_mwcs_basis(C.addressof(par), tab.ctypes.data)
    if rc:
        raise TspwsError(f"tspws_mwcs_basis refused the parameters (code {rc})")
    L, Qx, nk = par.L, mwcs_qrange(par)[2], 2 * par.h + 1
    cuts = np.cumsum([0, L, L * Qx, L * Qx, Qx, Qx, nk, Qx])
    parts = [tab[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return dict(g=parts[0], C=parts[1].reshape(L, Qx), S=parts[2].reshape(L, Qx), Tc=parts[3], Ts=parts[4], k=parts[5], v=parts[6])


class DtwPar(C.Structure):
    """tspws_dtw_par"""
    _fields_ = [("Lmax", C.c_uint), ("b", C.c_uint)]


def dtw_par(Lmax, b=1):
    """The parameters of Plan.dtw_rows (tspws_dtw_par): the largest lag in samples (1 .. 127) and the strain limit (1 .. 8: the lag changes by
    at most one sample per b samples).  The library judges them."""
    try:
        return DtwPar(int(Lmax), int(b))
    except (TypeError, ValueError, OverflowError):
        raise TspwsError("dtw_par: Lmax and b must be non-negative integers below 2^32") from None


def band_table(bands):
    """The C band table (uint32 [R][2]: s_begin, s_end) of a sequence of (s_begin, s_end) pairs."""
    import numpy as np
    b = np.asarray(bands)
    if b.size == 0:
        return np.zeros((0, 2), np.uint32)
    if b.ndim != 2 or b.shape[1] != 2 or b.dtype.kind not in "iu" or (b < 0).any() or (b > 0xFFFFFFFF).any():
        raise TspwsError("bands must be a sequence of (s_begin, s_end) pairs of non-negative integers")
    return np.ascontiguousarray(b, dtype=np.uint32)


def bands_from_frequencies(plan_or_tables, dt, edges, w0=None):
    """Bands of centre frequencies (tspws_bands_from_frequencies, host only): fc_s = w0 / (2 pi dt scale_s), band r = the scales with
    f_lo <= fc_s < f_hi.  `plan_or_tables` = a Plan, or (scale[S], w0) / a dict with "scale" and "w0" (w0 may also be given by keyword);
    `edges` = a 1-D sequence of R + 1 increasing frequencies (R bands with shared edges, lowest band first: they partition the scales
    between the outer edges) or a sequence of R (f_lo, f_hi) pairs.  Returns (bands uint32 [R][2], fc[S])."""
    import numpy as np
    if isinstance(plan_or_tables, Plan):
        scale, w = plan_or_tables.tables()["scale"], plan_or_tables.info.w0
    elif isinstance(plan_or_tables, dict):
        scale, w = plan_or_tables["scale"], plan_or_tables.get("w0")
    else:
        scale, w = plan_or_tables
    w = w0 if w0 is not None else w
    if w is None:
        raise TspwsError("bands_from_frequencies needs w0")
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1 and e.size >= 1:
        lo, hi = e[:-1], e[1:]
    elif e.ndim == 2 and e.shape[1] == 2:
        lo, hi = e[:, 0], e[:, 1]
    else:
        raise TspwsError("edges must be R + 1 frequencies or R (f_lo, f_hi) pairs")
    lo, hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    bands = np.zeros((lo.size, 2), np.uint32)
    fc = np.zeros(scale.size, np.float64)
    check(load().tspws_bands_from_frequencies(scale.ctypes.data, scale.size, float(w), float(dt), lo.ctypes.data, hi.ctypes.data, lo.size,
                                             bands.ctypes.data, fc.ctypes.data), "bands_from_frequencies")
    return bands, fc


def ftan_windows(dist, vmin, vmax, dt, z, N, sides=1):
    """The windows of one station pair for Plan.ftan_rows (tspws_ftan_windows, host only): group velocities vmin .. vmax over the distance
    `dist` arrive at the lags dist / (vmax dt) .. dist / (vmin dt) samples behind `z`; sides=2 adds the mirrored acausal window.  Returns
    uint64 [sides][2]; an empty window after clipping to [0, N] is refused."""
    import numpy as np
    if sides not in (1, 2):
        raise TspwsError("ftan_windows: sides must be 1 or 2")
    win = np.zeros((sides, 2), np.uint64)
    check(load().tspws_ftan_windows(float(dist), float(vmin), float(vmax), float(dt), float(z), int(N), int(sides), win.ctypes.data), "ftan_windows")
    return win


def ftan_periods(plan_or_tables, dt, w0=None):
    """The period of every scale (tspws_ftan_periods, host only): T_s = 2 pi dt scale_s / w0, the inverse of bands_from_frequencies' fc.
    `plan_or_tables` as there.  Returns T[S]."""
    import numpy as np
    if isinstance(plan_or_tables, Plan):
        scale, w = plan_or_tables.tables()["scale"], plan_or_tables.info.w0
    elif isinstance(plan_or_tables, dict):
        scale, w = plan_or_tables["scale"], plan_or_tables.get("w0")
    else:
        scale, w = plan_or_tables
    w = w0 if w0 is not None else w
    if w is None:
        raise TspwsError("ftan_periods needs w0")
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    T = np.zeros(scale.size, np.float64)
    check(load().tspws_ftan_periods(scale.ctypes.data, scale.size, float(w), float(dt), T.ctypes.data), "ftan_periods")
    return T


# tspws_weights_from_scores' rules, by name
WEIGHT_RULES = {"power": 0, "inverse": 1}


def weights_from_scores(score, first, rule, a=1.0):
    """One weight row from one plane of scores (tspws_weights_from_scores): `score` = float64 [T] (T = first[-1] - first[0]), `rule` =
    "power" / 0 (a similarity plane: w = score ** a where score > 0, else 0) or "inverse" / 1 (the energy plane: w = 1 / score for a finite
    score > 0, else 0, divided by the ensemble's largest w; `a` is ignored).  NaN scores give weight 0.  Returns w float64 [T], one row of
    Plan.weighted_stack_batch's weights."""
    import numpy as np
    f, B, T = _offsets(first)
    sc = _score_plane(score, T)
    r = WEIGHT_RULES.get(rule, rule)
    if r not in (0, 1):
        raise TspwsError(f"rule must be one of {tuple(WEIGHT_RULES)} (or 0 / 1), got {rule!r}")
    w = np.zeros(T, np.float64)
    rc = load().tspws_weights_from_scores(w.ctypes.data, sc.ctypes.data, f.ctypes.data, B, int(r), float(a))
    if rc:
        raise TspwsError(f"tspws_weights_from_scores refused its arguments (code {rc})")
    return w


def selection_classes(sel):
    """(class_of_trace[mtr] uint32, kept[C][ncls] int8) of a selection [C][mtr]: traces with identical selection columns form a class,
    numbered in order of first appearance (tspws_selection_classes)."""
    import numpy as np
    sel = np.ascontiguousarray(sel, dtype=np.int8)
    if sel.ndim != 2:
        raise TspwsError("selection must be 2-D [C][mtr]")
    Cn, mtr = sel.shape
    cls = np.zeros(mtr, np.uint32)
    kept = np.zeros(Cn * max(mtr, 1), np.int8)
    n = C.c_uint()
    check(load().tspws_selection_classes(sel.ctypes.data, Cn, mtr, cls.ctypes.data, kept.ctypes.data, C.byref(n)), "selection_classes")
    return cls, kept[:Cn * n.value].reshape(Cn, n.value).copy()


def synth(mtr, N, seed=0, first=0, device=0, pad=0):
    """Seeded synthetic ensemble generated on the device: float32 [mtr][N] view of rows `N + pad` samples apart (pad > 0:
    the trace rows do not all start at the same offset of the memory interleave)."""
    import torch
    ld = N + pad
    buf = torch.empty((mtr, ld), dtype=torch.float32, device=f"cuda:{device}")
    check(load().tspws_hip_synth(buf.data_ptr(), mtr, N, ld, seed, first, Plan._stream()), "synth")
    return buf[:, :N] if pad else buf
