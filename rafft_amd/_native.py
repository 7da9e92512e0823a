"""ctypes binding of libraffthip.so (include/rafft_hip.h).  No CPU fallback: if the
HIP library or a GPU is missing every call raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAFFT_LIB") or os.path.join(_HERE, "libraffthip.so")      # (RAFFT_LIB: another build of the library, for A/B measurements)

OK, ERR_BAD_CHAR, ERR_EMPTY, ERR_TOO_LONG, ERR_TEMP, ERR_CAPACITY, ERR_PARAM, ERR_HIP, ERR_STRUCT, ERR_NO_DEVICE, ERR_INFEASIBLE = range(11)


class Params(C.Structure):
    _fields_ = [("nb_mode", C.c_int32), ("max_stack", C.c_int32), ("max_branch", C.c_int32), ("min_hp", C.c_int32),
                ("min_nrj", C.c_double), ("traj", C.c_int32), ("_pad", C.c_int32), ("temp", C.c_double),
                ("gc_wei", C.c_double), ("au_wei", C.c_double), ("gu_wei", C.c_double)]


class SeqResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_steps", C.c_int32), ("n_structs", C.c_int32),
                ("step_size", C.POINTER(C.c_int32)), ("step_off", C.POINTER(C.c_int32)),
                ("db", C.POINTER(C.c_char)), ("dcal", C.POINTER(C.c_int32))]


class Result(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("n_failed", C.c_int32), ("seq", C.POINTER(SeqResult)), ("_owner", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_expand", C.c_double), ("ms_expand_c1", C.c_double),
                ("ms_expand_c2", C.c_double), ("ms_expand_c3", C.c_double), ("ms_expand_wall", C.c_double), ("ms_beam", C.c_double),
                ("ms_materialize", C.c_double), ("ms_output", C.c_double),
                ("n_expand_launches", C.c_int64), ("n_steps", C.c_int64), ("n_node_expansions", C.c_int64),
                ("n_nodes_created", C.c_int64), ("n_nodes_aliased", C.c_int64),
                ("sum_node_len", C.c_int64), ("sum_lags", C.c_int64), ("n_structs", C.c_int64),
                ("n_children", C.c_int64), ("sum_struct_len", C.c_int64), ("alg_bytes", C.c_int64),
                ("alg_bytes_expand", C.c_int64), ("alg_bytes_expand_all", C.c_int64), ("n_regrows", C.c_int64),
                ("alg_bytes_expand_small", C.c_int64), ("alg_bytes_expand_c2", C.c_int64), ("alg_bytes_expand_c3", C.c_int64),
                ("alg_bytes_beam", C.c_int64), ("n_node_instances", C.c_int64), ("n_dE_evals", C.c_int64), ("n_dE_guessed", C.c_int64),
                ("n_kept_guessed", C.c_int64), ("n_regrows_prod", C.c_int64), ("n_waves_long_lists", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KinGraph(C.Structure):
    """rafft_kin_graph: one record per graph of rafft_kin_batch"""
    _fields_ = [("status", C.c_int32), ("n_rows", C.c_int32), ("row0", C.c_int32), ("n_unique", C.c_int32), ("n_edges", C.c_int32),
                ("_pad", C.c_int32)]


KIN_BATCH_MAX_STATES = 1024      # RAFFT_KIN_BATCH_MAX_STATES


class MfeSeq(C.Structure):
    """rafft_mfe_seq: one record per sequence of rafft_mfe_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("dcal", C.c_int32), ("n_pairs", C.c_int32)]


class MfeConSeq(C.Structure):
    """rafft_mfe_con_seq: one record per sequence of rafft_mfe_constrained_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("dcal", C.c_int32), ("n_pairs", C.c_int32), ("pseudo_dcal", C.c_int32),
                ("_pad", C.c_int32)]


class CofoldSeq(C.Structure):
    """rafft_cofold_seq: one record per sequence of rafft_cofold_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("dcal", C.c_int32), ("n_pairs", C.c_int32), ("cut", C.c_int32),
                ("n_inter", C.c_int32)]


MFE_MAX_LEN = 4096               # RAFFT_MFE_MAX_LEN
MFE_SOFT_MAX = 20000             # RAFFT_MFE_SOFT_MAX (dcal)
MFE_SPAN_MAX_LEN = 32768         # RAFFT_MFE_SPAN_MAX_LEN (RAFFT_MAX_LEN)


class PfSeq(C.Structure):
    """rafft_pf_seq: one record per sequence of rafft_pf_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("mfe_dcal", C.c_int32), ("n_pairs", C.c_int32), ("energy", C.c_double),
                ("mfe_frequency", C.c_double)]


PF_MAX_LEN = MFE_MAX_LEN         # RAFFT_PF_MAX_LEN


class MeaSeq(C.Structure):
    """rafft_mea_seq: one record per sequence of rafft_mea_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("mfe_dcal", C.c_int32), ("n_pairs", C.c_int32), ("dcal", C.c_int32),
                ("_pad", C.c_int32), ("energy", C.c_double), ("mea", C.c_double), ("diversity", C.c_double)]


class MeaProbsSeq(C.Structure):
    """rafft_mea_probs_seq: one record per matrix of rafft_mea_probs_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_pairs", C.c_int32), ("_pad", C.c_int32), ("mea", C.c_double),
                ("diversity", C.c_double)]


class SampleSeq(C.Structure):
    """rafft_sample_seq: one record per sequence of rafft_sample_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("mfe_dcal", C.c_int32), ("n_samples", C.c_int32), ("energy", C.c_double)]


SAMPLE_MAX = 1 << 20             # RAFFT_SAMPLE_MAX


class SuboptSeq(C.Structure):
    """rafft_subopt_seq: one record per sequence of a rafft_subopt_result"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("mfe_dcal", C.c_int32), ("n_structs", C.c_int32), ("n_reached", C.c_int64),
                ("db", C.POINTER(C.c_char)), ("dcal", C.POINTER(C.c_int32))]


class SuboptResult(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("n_failed", C.c_int32), ("seq", C.POINTER(SuboptSeq)), ("_owner", C.c_void_p)]


SUBOPT_MAX_LEN = MFE_MAX_LEN     # RAFFT_SUBOPT_MAX_LEN
SUBOPT_MAX_STRUCTS = 1 << 24     # RAFFT_SUBOPT_MAX_STRUCTS
SUBOPT_MAX_DELTA = 1000000       # RAFFT_SUBOPT_MAX_DELTA (dcal)

class FindpathRec(C.Structure):
    """rafft_findpath_rec: one record per problem of rafft_findpath_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("dist", C.c_int32), ("start_dcal", C.c_int32), ("end_dcal", C.c_int32),
                ("saddle_dcal", C.c_int32), ("saddle_step", C.c_int32), ("_pad", C.c_int32)]


FINDPATH_MAX_LEN = MFE_MAX_LEN           # RAFFT_FINDPATH_MAX_LEN
FINDPATH_MAX_WIDTH = 1024                # RAFFT_FINDPATH_MAX_WIDTH
FINDPATH_MAX_CANDIDATES = 1 << 20        # RAFFT_FINDPATH_MAX_CANDIDATES

class DescendSeq(C.Structure):
    """rafft_descend_seq: one record per sequence of rafft_descend_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_rows", C.c_int32), ("row0", C.c_int32)]


class DescendRow(C.Structure):
    """rafft_descend_row: one record per start row of rafft_descend_batch"""
    _fields_ = [("status", C.c_int32), ("n_steps", C.c_int32), ("start_dcal", C.c_int32), ("end_dcal", C.c_int32)]


DESCEND_MAX_LEN = MFE_MAX_LEN            # RAFFT_DESCEND_MAX_LEN

class BarriersMin(C.Structure):
    """rafft_barriers_min: one record per local minimum of a rafft_barriers_seq"""
    _fields_ = [("rank", C.c_int32), ("father", C.c_int32), ("saddle_rank", C.c_int32), ("dcal", C.c_int32), ("saddle_dcal", C.c_int32),
                ("basin_size", C.c_int32)]


class BarriersEdge(C.Structure):
    """rafft_barriers_edge: the direct saddle between two adjacent gradient basins"""
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("saddle_rank", C.c_int32)]


class BarriersSeq(C.Structure):
    """rafft_barriers_seq: one record per sequence of a rafft_barriers_result"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_rows", C.c_int32), ("n_minima", C.c_int32), ("n_edges", C.c_int32),
                ("_pad", C.c_int32), ("minima", C.POINTER(BarriersMin)), ("edges", C.POINTER(BarriersEdge)), ("basin", C.POINTER(C.c_int32))]


class BarriersResult(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("n_failed", C.c_int32), ("seq", C.POINTER(BarriersSeq)), ("_owner", C.c_void_p)]


BARRIERS_MAX_LEN = MFE_MAX_LEN           # RAFFT_BARRIERS_MAX_LEN
BARRIERS_MAX_ROWS = SUBOPT_MAX_STRUCTS   # RAFFT_BARRIERS_MAX_ROWS


class KinfoldSeq(C.Structure):
    """rafft_kinfold_seq: one record per sequence of rafft_kinfold_batch"""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_traj", C.c_int32), ("traj0", C.c_int32)]


class KinfoldTraj(C.Structure):
    """rafft_kinfold_traj: one record per trajectory of rafft_kinfold_batch"""
    _fields_ = [("status", C.c_int32), ("flags", C.c_int32), ("n_steps", C.c_int32), ("start_dcal", C.c_int32), ("end_dcal", C.c_int32),
                ("stop_index", C.c_int32), ("time", C.c_double)]


KINFOLD_MAX_LEN = DESCEND_MAX_LEN        # RAFFT_KINFOLD_MAX_LEN
KINFOLD_NW = 4096                        # RAFFT_KINFOLD_NW
KINFOLD_MAX_WATCH = 64                   # RAFFT_KINFOLD_MAX_WATCH
KINFOLD_DEFAULT_STEPS = 1 << 20          # RAFFT_KINFOLD_DEFAULT_STEPS
KF_TIME, KF_STOP, KF_ABSORBED, KF_MORE = 1, 2, 4, 8     # RAFFT_KINFOLD_*

EXPORTS = ["rafft_init", "rafft_fold_batch", "rafft_fold_submit", "rafft_fold_wait", "rafft_free_result", "rafft_last_error", "rafft_eval_structure",
           "rafft_eval_structures", "rafft_eval_structures_at", "rafft_expand_node", "rafft_get_stats", "rafft_version",
           "rafft_load_params", "rafft_load_params_text", "rafft_reset_params", "rafft_save_params", "rafft_params_info",
           "rafft_param_value", "rafft_kin_rate_matrix", "rafft_shutdown", "rafft_alloc_counters", "rafft_eval_structures_info", "rafft_params_unpinned",
           "rafft_landscape_distances", "rafft_landscape_mds", "rafft_landscape_surface", "rafft_landscape_counters",
           "rafft_score_rows", "rafft_score_result", "rafft_kin_batch", "rafft_mfe_batch", "rafft_mfe_lds_len", "rafft_pf_batch",
           "rafft_sample_batch", "rafft_subopt_batch", "rafft_subopt_free", "rafft_subopt_counters", "rafft_findpath_batch",
           "rafft_findpath_counters", "rafft_descend_batch", "rafft_descend_counters", "rafft_barriers_batch",
           "rafft_barriers_free", "rafft_barriers_counters", "rafft_kinfold_batch", "rafft_kinfold_weights", "rafft_kinfold_counters",
           "rafft_mea_batch", "rafft_mea_probs_batch", "rafft_mfe_span_batch", "rafft_pf_span_batch", "rafft_mfe_constrained_batch",
           "rafft_pf_constrained_batch", "rafft_cofold_batch", "rafft_cofold_duplex_init"]

_lib = None


class RafftError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libraffthip error {code}: {msg}")
        self.code = code


def _one_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's); if
    libraffthip.so pulled in the system one first, a later `import torch` would load a second runtime that finds no
    GPU ("No HIP GPUs are available" - measured).  So when torch is installed its runtime is loaded first and
    libraffthip.so binds to it; without torch the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the HIP library (building it is __graft_entry__.build()'s / rafft_amd.build's job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing - run `python -m rafft_amd.build` (hipcc, gfx950). "
                          "rafft_amd has no CPU fallback.")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.rafft_init.argtypes = [C.c_int]
    L.rafft_fold_batch.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int,
                                   C.POINTER(C.POINTER(Result))]
    L.rafft_fold_submit.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int,
                                    C.POINTER(C.c_void_p)]
    L.rafft_fold_wait.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Result))]
    L.rafft_free_result.argtypes = [C.POINTER(Result)]
    L.rafft_free_result.restype = None
    L.rafft_shutdown.restype = None
    L.rafft_shutdown.argtypes = []
    L.rafft_alloc_counters.restype = None
    L.rafft_alloc_counters.argtypes = [C.POINTER(C.c_ulonglong * 5)]
    L.rafft_last_error.restype = C.c_char_p
    L.rafft_version.restype = C.c_char_p
    L.rafft_eval_structure.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    L.rafft_eval_structures.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    L.rafft_expand_node.argtypes = [C.POINTER(Params), C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rafft_eval_structures_at.argtypes = [C.c_double] + L.rafft_eval_structures.argtypes
    L.rafft_eval_structures_info.argtypes = L.rafft_eval_structures.argtypes + [C.POINTER(C.c_int)]
    L.rafft_params_unpinned.argtypes = [C.POINTER(C.c_int * 3)]
    L.rafft_load_params.argtypes = [C.c_char_p]
    L.rafft_load_params_text.argtypes = [C.c_char_p, C.c_char_p]
    L.rafft_save_params.argtypes = [C.c_char_p]
    L.rafft_params_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.rafft_param_value.argtypes = [C.c_char_p, C.c_int, C.c_long, C.POINTER(C.c_int)]
    L.rafft_get_stats.argtypes = [C.POINTER(Stats)]
    L.rafft_kin_rate_matrix.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                        C.POINTER(C.c_double), C.c_double, C.c_void_p]
    L.rafft_landscape_distances.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    L.rafft_landscape_mds.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_void_p,
                                      C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.rafft_landscape_surface.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.rafft_landscape_counters.argtypes = [C.POINTER(C.c_longlong * 4)]
    L.rafft_score_rows.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                   C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
    L.rafft_score_result.argtypes = [C.POINTER(Result), C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
    L.rafft_kin_batch.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                  C.POINTER(C.c_void_p), C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                  C.c_longlong, C.POINTER(KinGraph), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                  C.POINTER(C.c_void_p)]
    L.rafft_mfe_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong, C.POINTER(MfeSeq),
                                  C.POINTER(C.c_void_p)]
    L.rafft_mfe_lds_len.argtypes = []
    L.rafft_mfe_constrained_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.POINTER(C.c_char_p),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(MfeConSeq),
                                              C.POINTER(C.c_void_p)]
    L.rafft_cofold_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong,
                                     C.POINTER(CofoldSeq), C.POINTER(C.c_void_p)]
    L.rafft_cofold_duplex_init.argtypes = [C.c_double, C.POINTER(C.c_int)]
    L.rafft_mfe_span_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong, C.POINTER(MfeSeq),
                                       C.POINTER(C.c_void_p)]
    L.rafft_pf_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_double, C.c_longlong, C.POINTER(PfSeq),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_pf_span_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_double, C.c_int, C.c_longlong,
                                      C.POINTER(PfSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_pf_constrained_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.POINTER(C.c_char_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double, C.c_longlong, C.POINTER(PfSeq),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_mea_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_double, C.c_longlong, C.c_double,
                                  C.POINTER(MeaSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_mea_probs_batch.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_double, C.c_longlong, C.POINTER(MeaProbsSeq),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_sample_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_double, C.c_longlong, C.c_int,
                                     C.POINTER(C.c_ulonglong), C.POINTER(SampleSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_subopt_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, C.c_longlong,
                                     C.POINTER(C.POINTER(SuboptResult))]
    L.rafft_subopt_free.argtypes = [C.POINTER(SuboptResult)]
    L.rafft_subopt_free.restype = None
    L.rafft_subopt_counters.argtypes = [C.POINTER(C.c_longlong * 7)]
    L.rafft_findpath_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_int), C.c_double, C.c_longlong, C.POINTER(FindpathRec), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]
    L.rafft_findpath_counters.argtypes = [C.POINTER(C.c_longlong * 4)]
    L.rafft_descend_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong, C.POINTER(DescendSeq), C.c_void_p,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_descend_counters.argtypes = [C.POINTER(C.c_longlong * 4)]
    L.rafft_barriers_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(C.POINTER(BarriersResult))]
    L.rafft_barriers_free.argtypes = [C.POINTER(BarriersResult)]
    L.rafft_barriers_free.restype = None
    L.rafft_barriers_counters.argtypes = [C.POINTER(C.c_longlong * 6)]
    L.rafft_kinfold_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                      C.POINTER(C.c_double), C.c_longlong, C.POINTER(KinfoldSeq), C.c_void_p, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rafft_kinfold_weights.argtypes = [C.c_double, C.c_double, C.c_void_p]
    L.rafft_kinfold_counters.argtypes = [C.POINTER(C.c_longlong * 4)]
    _lib = L
    return L


def seq_arrays(sequences, rows=False):
    """The ctypes arguments of a list of sequences: (enc, arr, lens) - the encoded strings (a character outside ASCII becomes '?',
    which the library reports as that sequence's bad character), the array of their pointers and the array of their lengths.
    rows=True adds (bufs, out): one output row of len + 1 bytes per sequence and the array of the rows' addresses."""
    n = len(sequences)
    enc = [s.encode("ascii", "replace") for s in sequences]
    arr = (C.c_char_p * n)(*enc)
    lens = (C.c_int * n)(*map(len, enc))
    if not rows:
        return enc, arr, lens
    bufs = [C.create_string_buffer(len(e) + 1) for e in enc]
    out = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    return enc, arr, lens, bufs, out


def check(rc):
    if rc:
        raise RafftError(rc, lib().rafft_last_error().decode())
