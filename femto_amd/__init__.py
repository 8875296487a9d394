"""femto_amd -- MI355X-native FM-index query engine reading femto (femto-dev/femto) index files.

This package is a thin ctypes binding over the C ABI in include/femto_amd.h (the product is the
shared library femto_amd/libfemto_amd.so: C++ host + hand-written HIP kernels for gfx950).  There
is NO CPU fallback: without the built library or without a HIP device every query call raises.

Host-side mirror of the reference's batch interface (src/main/femto_internal.h):
    Index.count(...)   <-> parallel_count   (src/main/femto.c:275)
    Index.locate(...)  <-> parallel_locate  (src/main/femto.c:331)
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

__all__ = ["Index", "Extractor", "FemtoAmdError", "lib", "ALPHA_SIZE", "CHARACTER_OFFSET", "Info", "class_patterns", "iupac_patterns"]

ALPHA_SIZE = 261
CHARACTER_OFFSET = 5
CLASS_SYMBOL = 0x8000     # FEMTO_AMD_CLASS_SYMBOL: a pattern symbol CLASS_SYMBOL | c names class c (Index.classes)
MAX_CLASSES = 4096        # FEMTO_AMD_MAX_CLASSES
QUERY_ICASE = 1           # FEMTO_AMD_QUERY_ICASE
ERR_NAMES = {0: "NOERR", 1: "MEM", 2: "IO", 3: "PARAM", 4: "FORMAT", 5: "BZ_DATA", 6: "INVALID",
             8: "MISSING", 10: "FULL", 11: "OVERWORKED", 12: "UNKNOWN"}
ERR_PARAM, ERR_INVALID, ERR_FULL, ERR_OVERWORKED = 3, 6, 10, 11
BUDGET_ALL = -2       # femto_amd_options_t::hbm_budget_bytes: whatever is free on the device (the default is a bound, include/femto_amd.h)


class FemtoAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"femto_amd error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


class Info(C.Structure):
    _fields_ = [("total_length", C.c_int64), ("number_of_blocks", C.c_int64), ("number_of_documents", C.c_int64),
                ("block_size", C.c_int32), ("bucket_size", C.c_int32), ("mark_period", C.c_int32),
                ("chunk_size", C.c_int32), ("text_size_bits", C.c_int32), ("total_buckets", C.c_int64),
                ("image_bytes", C.c_int64), ("table_bytes", C.c_int64)]


class Options(C.Structure):
    """femto_amd_options_t (include/femto_amd.h): every field -1 = auto after femto_amd_options_init"""
    _fields_ = [("struct_size", C.c_uint32), ("rank_mode", C.c_int32), ("hbm_budget_bytes", C.c_int64), ("packed_lines", C.c_int32),
                ("two_level_lines", C.c_int32), ("char_rank_lines", C.c_int32), ("text", C.c_int32), ("dense_arrays", C.c_int32),
                ("mark_every", C.c_int32), ("level_table", C.c_int32), ("level_table_syms", C.c_int32), ("level_table_bytes", C.c_int64),
                ("context_table", C.c_int32), ("context_syms", C.c_int32), ("context2_table", C.c_int32), ("context2_syms", C.c_int32),
                ("context2_bytes", C.c_int64), ("tail_min", C.c_int32), ("tail_ones", C.c_int32), ("tail_rows", C.c_int32),
                ("tail_row_cost", C.c_int32), ("sort_queries", C.c_int32), ("host_threads", C.c_int32), ("host_pipeline", C.c_int32),
                ("host_keys", C.c_int32), ("host_pipe_chunk_log2", C.c_int32), ("host_d2h_staged", C.c_int32),
                ("rank_units", C.c_int32), ("marks_32bit", C.c_int32), ("context_mid_table", C.c_int32), ("wavelet_lines", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().femto_amd_options_init(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise KeyError(k)
            setattr(self, k, int(v))


class SimilarResult(C.Structure):
    """femto_amd_similar_result_t"""
    _fields_ = [("n", C.c_int64), ("len", C.POINTER(C.c_int32)), ("ngroups", C.c_int64), ("g_len", C.POINTER(C.c_int32)),
                ("g_first", C.POINTER(C.c_int64)), ("g_last", C.POINTER(C.c_int64)), ("g_here", C.POINTER(C.c_int32)),
                ("g_min_start", C.POINTER(C.c_int64)), ("g_kept", C.POINTER(C.c_uint8)), ("index_numerator", C.c_int64),
                ("index_score", C.c_double), ("ndocs", C.c_int64), ("doc", C.POINTER(C.c_int64)),
                ("doc_numerator", C.POINTER(C.c_int64)), ("doc_seqs", C.POINTER(C.c_int32)), ("doc_score", C.POINTER(C.c_double))]


class MismatchResult(C.Structure):
    """femto_amd_mismatch_result_t"""
    _fields_ = [("npat", C.c_int64), ("total", C.c_int64), ("result_start", C.POINTER(C.c_int64)), ("first", C.POINTER(C.c_int64)),
                ("last", C.POINTER(C.c_int64)), ("cost", C.POINTER(C.c_int32)), ("sub_pos", C.POINTER(C.c_int32)),
                ("sub_sym", C.POINTER(C.c_uint16))]


class EditResult(C.Structure):
    """femto_amd_edit_result_t"""
    _fields_ = [("npat", C.c_int64), ("total", C.c_int64), ("result_start", C.POINTER(C.c_int64)), ("first", C.POINTER(C.c_int64)),
                ("last", C.POINTER(C.c_int64)), ("cost", C.POINTER(C.c_int32)), ("length", C.POINTER(C.c_int32))]


class ClassesResult(C.Structure):
    """femto_amd_classes_result_t"""
    _fields_ = [("npat", C.c_int64), ("total", C.c_int64), ("result_start", C.POINTER(C.c_int64)), ("first", C.POINTER(C.c_int64)),
                ("last", C.POINTER(C.c_int64))]


class HammingResult(C.Structure):
    """femto_amd_hamming_result_t"""
    _fields_ = [("npat", C.c_int64), ("total", C.c_int64), ("candidates", C.c_int64), ("result_start", C.POINTER(C.c_int64)),
                ("offset", C.POINTER(C.c_int64)), ("cost", C.POINTER(C.c_int32))]


class LevenResult(C.Structure):
    """femto_amd_leven_result_t"""
    _fields_ = [("npat", C.c_int64), ("total", C.c_int64), ("candidates", C.c_int64), ("raw", C.c_int64), ("result_start", C.POINTER(C.c_int64)),
                ("offset", C.POINTER(C.c_int64)), ("cost", C.POINTER(C.c_int32)), ("length", C.POINTER(C.c_int32))]


class Similar:
    """What Index.similar returns (numpy copies of femto_amd_similar_result_t): len[n]; the groups, longest first: g_len, g_first,
    g_last, g_here, g_min_start, g_kept; index_numerator, index_score; the documents with a score, best first: doc, doc_numerator,
    doc_seqs, doc_score"""

    def __init__(self, r):
        def arr(p, count, dtype):
            return np.ctypeslib.as_array(p, shape=(count,)).astype(dtype, copy=True) if count and p else np.zeros(0, dtype=dtype)
        self.n, self.ngroups, self.ndocs = int(r.n), int(r.ngroups), int(r.ndocs)
        self.len = arr(r.len, self.n, np.int32)
        self.g_len, self.g_here = arr(r.g_len, self.ngroups, np.int32), arr(r.g_here, self.ngroups, np.int32)
        self.g_first, self.g_last = arr(r.g_first, self.ngroups, np.int64), arr(r.g_last, self.ngroups, np.int64)
        self.g_min_start, self.g_kept = arr(r.g_min_start, self.ngroups, np.int64), arr(r.g_kept, self.ngroups, np.uint8)
        self.index_numerator, self.index_score = int(r.index_numerator), float(r.index_score)
        self.doc, self.doc_numerator = arr(r.doc, self.ndocs, np.int64), arr(r.doc_numerator, self.ndocs, np.int64)
        self.doc_seqs, self.doc_score = arr(r.doc_seqs, self.ndocs, np.int32), arr(r.doc_score, self.ndocs, np.float64)


def _dp(t):
    """a device address: a torch tensor's, or an int (0 / None = NULL)"""
    if t is None:
        return None
    return (t.data_ptr() if hasattr(t, "data_ptr") else int(t)) or None


def _u8(data):
    return np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)


def _copy_of(p, count, ct):
    """`count` elements of C type `ct` at the library's pointer `p`, as an array of our own"""
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(count,)).copy() if count else np.zeros(0, dtype=ct)


class NfaStruct(C.Structure):
    """femto_amd_nfa_t (include/femto_amd.h): the reference's nfa_description_t, flat"""
    _fields_ = [("num_nodes", C.c_int32), ("num_transitions", C.c_int32), ("trans_start", C.c_void_p),
                ("trans_char", C.c_void_p), ("trans_dest", C.c_void_p), ("is_start", C.c_void_p), ("is_final", C.c_void_p),
                ("cost_bound", C.c_int32), ("subst_cost", C.c_int32), ("delete_cost", C.c_int32), ("insert_cost", C.c_int32)]


class Nfa:
    """An epsilon-free automaton of the REVERSED pattern, as do_regexp_query simulates it (src/main/nfa.h:62-88): node i's
    transitions are entries trans_start[i] .. trans_start[i+1]-1 of trans_char (alpha codes) / trans_dest; settings =
    (cost_bound, subst_cost, delete_cost, insert_cost), cost_bound 1 = exact."""

    def __init__(self, trans_start, trans_char, trans_dest, is_start, is_final, settings=(1, 1, 1, 1)):
        self.trans_start = np.ascontiguousarray(trans_start, dtype=np.int32)
        self.trans_char = np.ascontiguousarray(trans_char, dtype=np.int32)
        self.trans_dest = np.ascontiguousarray(trans_dest, dtype=np.int32)
        self.is_start = np.ascontiguousarray(is_start, dtype=np.uint8)
        self.is_final = np.ascontiguousarray(is_final, dtype=np.uint8)
        self.settings = tuple(int(v) for v in settings)
        self.num_nodes = len(self.is_start)

    @classmethod
    def _of_handle(cls, h):
        """a copy of the automaton a femto_amd_regexp_t holds (femto_amd_regexp_nfa's view is valid until the handle is freed)"""
        v = lib().femto_amd_regexp_nfa(h).contents
        n, t = v.num_nodes, v.num_transitions
        return cls(_copy_of(v.trans_start, n + 1, C.c_int32), _copy_of(v.trans_char, t, C.c_int32), _copy_of(v.trans_dest, t, C.c_int32),
                   _copy_of(v.is_start, n, C.c_uint8), _copy_of(v.is_final, n, C.c_uint8),
                   (v.cost_bound, v.subst_cost, v.delete_cost, v.insert_cost))

    @classmethod
    def from_regex(cls, regex, approx=None):
        """femto_amd_regexp_compile: pattern text -> the position automaton of the reversed pattern; approx = (max_cost,
        subst_cost, delete_cost, insert_cost) as in QUERY_FORMAT.txt's APPROX"""
        rx = np.frombuffer(bytes(regex) + b"\0", dtype=np.uint8)
        k = (0, 1, 1, 1) if approx is None else tuple(int(v) for v in approx)
        h = C.c_void_p()
        _check(lib().femto_amd_regexp_compile(_ptr(rx), len(regex), k[0], k[1], k[2], k[3], C.byref(h)))
        try:
            return cls._of_handle(h)
        finally:
            lib().femto_amd_regexp_free(h)

    @classmethod
    def from_query(cls, query, icase=False, streamline=True):
        """femto_amd_query_compile: a whole femto_search query prepared as search_tool.cc prepares it (streamline_query,
        simplify_query, --icase).  Returns (Nfa, literal alpha codes or None, the query echoed as ast_to_string prints it)."""
        q = np.frombuffer(bytes(query) + b"\0", dtype=np.uint8)
        h = C.c_void_p()
        _check(lib().femto_amd_query_compile(_ptr(q), len(query), (1 if icase else 0) | (0 if streamline else 2), C.byref(h)))
        try:
            a = cls._of_handle(h)
            sp, sn = C.c_void_p(), C.c_int64(0)
            lit = None
            if lib().femto_amd_regexp_literal(h, C.byref(sp), C.byref(sn)):
                lit = _copy_of(sp, sn.value, C.c_uint16)
            return a, lit, lib().femto_amd_regexp_echo(h)
        finally:
            lib().femto_amd_regexp_free(h)

    def struct(self):
        return NfaStruct(self.num_nodes, len(self.trans_char), self.trans_start.ctypes.data, self.trans_char.ctypes.data,
                         self.trans_dest.ctypes.data, self.is_start.ctypes.data, self.is_final.ctypes.data, *self.settings)


class NfaBatch:
    """automata marshalled once into the C ABI's array of femto_amd_nfa_t (what a C caller holds anyway): timing
    Index.nfa_search_batch(NfaBatch) times the library call, not Python building 20 000 structs"""

    def __init__(self, nfas):
        self.nfas = list(nfas)          # keeps the numpy arrays the structs point into alive
        self.n = len(self.nfas)
        self.arr = (NfaStruct * max(1, self.n))(*[a.struct() for a in self.nfas])


_lib = None


def lib():
    """Load (never silently substitute) the HIP extension."""
    global _lib
    if _lib is None:
        if not os.path.exists(_build.LIB):
            raise ImportError(f"{_build.LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        # Load order matters in a process that also uses PyTorch-ROCm: torch ships its own libamdhip64, and two HIP runtimes
        # in one process do not see each other's devices.  Importing torch first makes this library resolve to the runtime
        # torch already loaded (observed on the GPU box: loading this library first made hipGetDeviceCount fail later).
        import sys
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(_build.LIB)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
        L.femto_amd_open.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
        L.femto_amd_close.argtypes = [vp]
        L.femto_amd_close.restype = None
        L.femto_amd_last_error.restype = C.c_char_p
        L.femto_amd_info.argtypes = [vp, C.POINTER(Info)]
        L.femto_amd_count_flat.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_count_bytes.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_locate_flat.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, i64, C.POINTER(i64)]
        L.femto_amd_locate_flat_alloc.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_parallel_locate_range.argtypes = [vp, i64, i64, vp]
        L.femto_amd_parallel_count.argtypes = [vp, i32, vp, vp, vp, vp]
        L.femto_amd_parallel_locate.argtypes = [vp, i32, vp, vp, i32, vp, vp]
        L.femto_amd_resolve_location.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64)]
        L.femto_amd_document_info.argtypes = [vp, i64, C.POINTER(C.c_char_p), C.POINTER(i64)]
        L.femto_amd_count_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
        L.femto_amd_locate_plan_device.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        L.femto_amd_locate_walk_device.argtypes = [vp, i64, vp, vp, i64, vp, vp]
        L.femto_amd_locate_device.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_locate_device_v2.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_pack_counts_device.argtypes = [vp, i64, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_trace_lines.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, C.POINTER(i64)]
        L.femto_amd_open_multi.argtypes = [C.c_char_p, i32, vp, C.POINTER(vp)]
        L.femto_amd_open_multi_striped.argtypes = [C.c_char_p, i32, vp, C.POINTER(vp)]
        L.femto_amd_striped_serve.argtypes = [vp, C.c_char_p, i32]
        L.femto_amd_open_striped_client.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.POINTER(vp)]
        L.femto_amd_multi_child.argtypes = [vp, i32, C.POINTER(vp)]
        L.femto_amd_device_count.argtypes = [vp]
        L.femto_amd_comm_unique_id.argtypes = [vp]
        L.femto_amd_comm_init.argtypes = [vp, vp, i32, i32]
        L.femto_amd_comm_gather.argtypes = [vp, vp, vp, i64, i32, vp]
        L.femto_amd_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        L.femto_amd_regexp_search.argtypes = [vp, vp, i64, i64, vp, vp, vp, C.POINTER(i64)]
        L.femto_amd_regexp_search_approx.argtypes = [vp, vp, i64, i32, i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(i64)]
        L.femto_amd_regexp_match.argtypes = [vp, i64, vp, i64]
        L.femto_amd_options_init.argtypes = [vp]
        L.femto_amd_options_init.restype = None
        L.femto_amd_open_opts.argtypes = [C.c_char_p, i32, vp, C.POINTER(vp)]
        L.femto_amd_host_pipeline_stats.argtypes = [vp, vp]
        L.femto_amd_key_format.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), vp]
        L.femto_amd_pack_keys_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
        L.femto_amd_locate_keys_device.argtypes = [vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_regexp_compile.argtypes = [vp, i64, i32, i32, i32, i32, C.POINTER(vp)]
        L.femto_amd_regexp_nfa.argtypes = [vp]
        L.femto_amd_regexp_nfa.restype = C.POINTER(NfaStruct)
        L.femto_amd_regexp_free.argtypes = [vp]
        L.femto_amd_regexp_free.restype = None
        L.femto_amd_nfa_search_batch.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
        L.femto_amd_nfa_stats.argtypes = [vp, vp]
        if hasattr(L, "femto_amd_lf_steps_device"):      # (absent from the older builds tools/ab_bench.sh loads beside this one)
            L.femto_amd_lf_steps_device.argtypes = [vp, i64, vp, vp, vp, vp]
        L.femto_amd_key_table_id.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.femto_amd_set_option.argtypes = [vp, C.c_char_p, i32]
        L.femto_amd_block_requests.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_kernel_time_ms.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(i64)]
        L.femto_amd_kernel_time_reset.argtypes = [vp]
        L.femto_amd_kernel_time_reset.restype = None
        L.femto_amd_kernel_time_enable.argtypes = [vp, i32]
        L.femto_amd_kernel_time_enable.restype = None
        L.femto_amd_build_index.argtypes = [C.c_char_p, i32, vp, vp, vp, C.c_char_p, i32]
        L.femto_amd_build_index_from_sa.argtypes = [C.c_char_p, i32, vp, vp, vp, C.c_char_p, vp]
        L.femto_amd_forward_steps.argtypes = [vp, i64, vp, vp, vp, vp]
        L.femto_amd_resolve_batch.argtypes = [vp, i64, vp, vp, vp]
        L.femto_amd_resolve_device.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_query_compile.argtypes = [vp, i64, i32, C.POINTER(vp)]
        L.femto_amd_regexp_literal.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_regexp_echo.argtypes = [vp]
        L.femto_amd_regexp_echo.restype = C.c_char_p
        L.femto_amd_query_echo.argtypes = [vp, i64, i32, i32, vp, i64]
        L.femto_amd_set_rank_mode.argtypes = [vp, i32]
        L.femto_amd_get_rank_mode.argtypes = [vp]
        L.femto_amd_pack_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i32)]
        L.femto_amd_structures.argtypes = [vp, vp, i32]
        L.femto_amd_flatten_index.argtypes = [C.c_char_p, C.c_char_p]
        L.femto_amd_bseq_encode.argtypes = [vp, i64, i32, vp, i64, C.POINTER(i64)]
        L.femto_amd_open_split.argtypes = [C.c_char_p, i32, i32, i32, C.POINTER(vp)]
        L.femto_amd_split_export.argtypes = [vp, vp]
        L.femto_amd_split_attach.argtypes = [vp, i32, vp]
        L.femto_amd_split_attach_local.argtypes = [vp, vp]
        L.femto_amd_split_commit.argtypes = [vp]
        L.femto_amd_split_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]
        L.femto_amd_extractor_open.argtypes = [vp, i32, i32, C.POINTER(vp)]
        L.femto_amd_extractor_free.argtypes = [vp]
        L.femto_amd_extractor_free.restype = None
        L.femto_amd_extractor_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_double)]
        L.femto_amd_extractor_eof_rows.argtypes = [vp, vp, i64]
        L.femto_amd_extract_device.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_context_device.argtypes = [vp, i64, vp, vp, vp, i32, i32, vp, vp, vp]
        L.femto_amd_extract.argtypes = [vp, i64, vp, vp, vp, vp]
        L.femto_amd_context.argtypes = [vp, i64, vp, vp, i32, i32, vp, vp]
        L.femto_amd_extract_document.argtypes = [vp, i64, C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_lines_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.femto_amd_line_bytes_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_line_groups_device.argtypes = [vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]
        L.femto_amd_lines.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_line_groups.argtypes = [vp, i64, vp, vp, vp, i32, vp, C.POINTER(i64)]
        L.femto_amd_doclist_info.argtypes = [C.POINTER(i32), C.POINTER(i32)]
        L.femto_amd_doclist_device.argtypes = [vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.femto_amd_docset_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_doclist.argtypes = [vp, i64, vp, vp, vp, i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_docset.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_docpos_info.argtypes = [C.POINTER(i32)]
        L.femto_amd_docpos_chunks.argtypes = []
        L.femto_amd_docpos_chunks.restype = i32
        L.femto_amd_docpos_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_docpos_documents_device.argtypes = [vp, i64, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_docpos.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_proximity.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_bquery_compile.argtypes = [vp, i64, i32, C.POINTER(vp)]
        L.femto_amd_bquery_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
        L.femto_amd_bquery_node.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(vp)]
        L.femto_amd_bquery_echo.argtypes = [vp]
        L.femto_amd_bquery_echo.restype = C.c_char_p
        L.femto_amd_bquery_free.argtypes = [vp]
        L.femto_amd_bquery_free.restype = None
        L.femto_amd_bquery_run_batch.argtypes = [vp, i64, vp, i32, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.femto_amd_match_stats_device.argtypes = [vp, i64, vp, i32, vp, vp, vp, vp]
        L.femto_amd_match_stats_steps_device.argtypes = [vp, i64, vp, i32, vp, vp]
        L.femto_amd_common_sequences_device.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp]
        L.femto_amd_common_groups_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.femto_amd_similar_documents_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, vp]
        L.femto_amd_similar.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, C.POINTER(SimilarResult)]
        L.femto_amd_similar_free.argtypes = [C.POINTER(SimilarResult)]
        L.femto_amd_similar_free.restype = None
        L.femto_amd_mismatch_device.argtypes = [vp, i64, i64, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.femto_amd_mismatch.argtypes = [vp, i64, vp, vp, i32, C.POINTER(MismatchResult)]
        L.femto_amd_mismatch_free.argtypes = [C.POINTER(MismatchResult)]
        L.femto_amd_mismatch_free.restype = None
        L.femto_amd_edit_device.argtypes = [vp, i64, i64, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
        L.femto_amd_edit.argtypes = [vp, i64, vp, vp, i32, C.POINTER(EditResult)]
        L.femto_amd_edit_free.argtypes = [C.POINTER(EditResult)]
        L.femto_amd_edit_free.restype = None
        L.femto_amd_classes_device.argtypes = [vp, i64, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
        L.femto_amd_classes.argtypes = [vp, i64, vp, vp, i64, vp, C.POINTER(ClassesResult)]
        L.femto_amd_classes_free.argtypes = [C.POINTER(ClassesResult)]
        L.femto_amd_classes_free.restype = None
        L.femto_amd_class_pattern_compile.argtypes = [vp, i64, i32, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64)]
        L.femto_amd_hamming_device.argtypes = [vp, i64, i64, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp]
        L.femto_amd_hamming.argtypes = [vp, i64, vp, vp, i32, C.POINTER(HammingResult)]
        L.femto_amd_hamming_free.argtypes = [C.POINTER(HammingResult)]
        L.femto_amd_hamming_free.restype = None
        L.femto_amd_leven_device.argtypes = [vp, i64, i64, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]
        L.femto_amd_leven.argtypes = [vp, i64, vp, vp, i32, C.POINTER(LevenResult)]
        L.femto_amd_leven_free.argtypes = [C.POINTER(LevenResult)]
        L.femto_amd_leven_free.restype = None
        _lib = L
    return _lib


def _libc_free(p):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)


def _check(rc):
    if rc:
        raise FemtoAmdError(rc, lib().femto_amd_last_error().decode(errors="replace"))


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def flatten(patterns):
    """list of uint16 alpha arrays -> (plen int32[n], flat uint16[sum], starts int64[n])"""
    plen = np.array([len(p) for p in patterns], dtype=np.int32)
    starts = np.zeros(len(patterns), dtype=np.int64)
    if len(patterns):
        starts[1:] = np.cumsum(plen[:-1], dtype=np.int64)
    flat = (np.concatenate([np.asarray(p, dtype=np.uint16) for p in patterns])
            if len(patterns) and plen.sum() else np.zeros(1, dtype=np.uint16))
    return plen, np.ascontiguousarray(flat), starts


def _class_words(members):
    """the four words of the class that holds the bytes `members`"""
    w = np.zeros(4, dtype=np.uint64)
    for b in members:
        w[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return w


def _merge_classes(per_query):
    """[(symbols uint16[], classes uint64[k, 4])] -> (patterns, classes uint64[n, 4]) with equal sets shared over all queries"""
    number, table, patterns = {}, [], []
    for syms, cls in per_query:
        syms = syms.copy()
        for i in np.nonzero(syms & CLASS_SYMBOL)[0]:
            words = cls[int(syms[i]) & ~CLASS_SYMBOL]
            key = words.tobytes()
            if key not in number:
                if len(table) >= MAX_CLASSES:
                    raise FemtoAmdError(ERR_PARAM, "more than %d different sets in one batch" % MAX_CLASSES)
                number[key] = len(table)
                table.append(words)
            syms[i] = CLASS_SYMBOL | number[key]
        patterns.append(syms)
    return patterns, (np.stack(table) if table else np.zeros((0, 4), dtype=np.uint64))


def class_patterns(queries, icase=False):
    """femto_amd_class_pattern_compile for every query text (bytes), the class tables merged: (patterns, classes uint64[n, 4]) as
    Index.classes and Index.classes_device take them.  A query that is not a concatenation of characters, strings, sets and periods
    raises FemtoAmdError with code ERR_INVALID"""
    per = []
    for q in queries:
        text = np.frombuffer(bytes(q) + b"\0", dtype=np.uint8)
        cap = len(q) + 1          # a symbol and a set take at least one byte of text each
        syms, cls = np.zeros(cap, dtype=np.uint16), np.zeros((cap, 4), dtype=np.uint64)
        ns, nc = C.c_int64(0), C.c_int64(0)
        _check(lib().femto_amd_class_pattern_compile(_ptr(text), len(q), QUERY_ICASE if icase else 0, _ptr(syms), cap, C.byref(ns),
                                                     _ptr(cls), cap, C.byref(nc)))
        per.append((syms[:ns.value], cls[:nc.value]))
    return _merge_classes(per)


# the IUPAC nucleotide codes beside A, C, G, T: class i of iupac_patterns' table holds the bases of IUPAC_CODES[i]
IUPAC_CODES = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def iupac_patterns(reads):
    """DNA reads (bytes or str over ACGT, the IUPAC codes RYSWKMBDHV and N, upper case) -> (patterns, classes uint64[11, 4]): a base
    is a literal, a code the class of its bases.  Any other character raises ValueError"""
    order = list(IUPAC_CODES)
    table = np.stack([_class_words([ord(b) for b in IUPAC_CODES[c]]) for c in order])
    sym = np.full(256, 0xffff, dtype=np.uint16)
    for b in b"ACGT":
        sym[b] = b + CHARACTER_OFFSET
    for i, c in enumerate(order):
        sym[ord(c)] = CLASS_SYMBOL | i
    patterns = []
    for r in reads:
        p = sym[np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), dtype=np.uint8)]
        if (p == 0xffff).any():
            raise ValueError("a read holds a character that is neither a base nor an IUPAC code")
        patterns.append(p)
    return patterns, table


class Index:
    """A femto index resident in the HBM of one GPU.  device=-1 parses only (host logic tests)."""

    def __init__(self, path, device=0, part=None, nparts=None, devices=None, striped=False, striped_socket=None, timeout_s=600,
                 _borrowed=None, options=None):
        self._h = C.c_void_p()
        self._peers = []   # range-split: the parts attached in-process must outlive this handle's use
        self._owner = None
        if _borrowed is not None:   # replica of a multi-device handle (femto_amd_multi_child): closed with its parent
            self._owner, self._h = _borrowed
        elif striped_socket is not None:   # striped index built by ANOTHER process (femto_amd_open_striped_client)
            _check(lib().femto_amd_open_striped_client(os.fsencode(path), os.fsencode(striped_socket), int(device), int(timeout_s),
                                                       C.byref(self._h)))
        elif devices is not None:     # one handle over several GPUs of this process (femto_amd_open_multi): host-pointer calls only
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            fn = lib().femto_amd_open_multi_striped if striped else lib().femto_amd_open_multi
            _check(fn(os.fsencode(path), len(devices), arr, C.byref(self._h)))
            device = list(devices)
        elif nparts is None and options is not None:    # femto_amd_open_opts: options = Options(...) or a dict of its fields
            o = options if isinstance(options, Options) else Options(**options)
            _check(lib().femto_amd_open_opts(os.fsencode(path), device, C.byref(o), C.byref(self._h)))
        elif nparts is None:
            _check(lib().femto_amd_open(os.fsencode(path), device, C.byref(self._h)))
        else:
            _check(lib().femto_amd_open_split(os.fsencode(path), device, int(part), int(nparts), C.byref(self._h)))
        self.device = device
        self.part, self.nparts = part, nparts
        self.info = Info()
        _check(lib().femto_amd_info(self._h, C.byref(self.info)))

    # ---- range-split index (femto_amd_open_split): part p holds blocks [nb*p/nparts, nb*(p+1)/nparts)
    def split_export(self):
        """128-byte blob (two hipIpcMemHandle_t) other PROCESSES pass to split_attach"""
        blob = C.create_string_buffer(128)
        _check(lib().femto_amd_split_export(self._h, blob))
        return blob.raw

    def split_attach(self, part, blob):
        _check(lib().femto_amd_split_attach(self._h, int(part), C.create_string_buffer(bytes(blob), 128)))

    def split_attach_local(self, owner):
        """attach a part opened in THIS process (same GPU, or another GPU with peer access)"""
        _check(lib().femto_amd_split_attach_local(self._h, owner._h))
        self._peers.append(owner)

    def split_commit(self):
        _check(lib().femto_amd_split_commit(self._h))

    def split_info(self):
        part, nparts, sb, ib = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        _check(lib().femto_amd_split_info(self._h, C.byref(part), C.byref(nparts), C.byref(sb), C.byref(ib)))
        return {"part": part.value, "nparts": nparts.value, "seg_bytes": sb.value, "image_bytes": ib.value}

    def striped_serve(self, socket_path, nclients):
        """striped handle (devices=[...], striped=True): hand the stripes to `nclients` other processes (blocks until all
        have attached; femto_amd_striped_serve)"""
        _check(lib().femto_amd_striped_serve(self._h, os.fsencode(socket_path), int(nclients)))

    def child(self, i):
        """replica i of a multi-device handle as a single-GPU Index (borrowed: valid until this handle is closed)"""
        h = C.c_void_p()
        _check(lib().femto_amd_multi_child(self._h, int(i), C.byref(h)))
        dev = self.device[i] if isinstance(self.device, (list, tuple)) else self.device
        return Index(None, device=dev, _borrowed=(self, h))

    def close(self):
        for ex in getattr(self, "_extractors", {}).values():   # before the handle they belong to
            ex.free()
        self._extractors = {}
        if self._owner is not None:
            self._h = C.c_void_p()
            self._owner = None
            return
        if self._h:
            lib().femto_amd_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- host-array API (numpy in, numpy out)
    def count_flat(self, plen, flat, starts):
        n = len(plen)
        plen = np.ascontiguousarray(plen, dtype=np.int32)
        flat = np.ascontiguousarray(flat, dtype=np.uint16)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        first = np.zeros(n, dtype=np.int64)
        last = np.zeros(n, dtype=np.int64)
        _check(lib().femto_amd_count_flat(self._h, n, _ptr(plen), _ptr(flat), _ptr(starts), _ptr(first), _ptr(last)))
        return first, last

    def count(self, patterns):
        return self.count_flat(*flatten(patterns))

    def locate_flat(self, plen, flat, starts, max_occs):
        n = len(plen)
        plen = np.ascontiguousarray(plen, dtype=np.int32)
        flat = np.ascontiguousarray(flat, dtype=np.uint16)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        noccs = np.zeros(n, dtype=np.int32)
        total = C.c_int64(0)
        buf = C.c_void_p()
        _check(lib().femto_amd_locate_flat_alloc(self._h, n, _ptr(plen), _ptr(flat), _ptr(starts), max_occs, _ptr(noccs), None,
                                                 C.byref(buf), C.byref(total)))
        if not total.value:
            return noccs, np.zeros(0, dtype=np.int64)
        try:
            offs = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int64)), shape=(total.value,)).copy()
        finally:
            _libc_free(buf)
        return noccs, offs

    def locate_flat_two_call(self, plen, flat, starts, max_occs):
        """femto_amd_locate_flat's sizing protocol: first call sizes, second fills a caller-provided buffer"""
        n = len(plen)
        plen = np.ascontiguousarray(plen, dtype=np.int32)
        flat = np.ascontiguousarray(flat, dtype=np.uint16)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        noccs = np.zeros(n, dtype=np.int32)
        ostarts = np.zeros(n + 1, dtype=np.int64)
        total = C.c_int64(0)
        _check(lib().femto_amd_locate_flat(self._h, n, _ptr(plen), _ptr(flat), _ptr(starts), max_occs, _ptr(noccs),
                                           _ptr(ostarts), None, 0, C.byref(total)))
        offs = np.zeros(max(1, total.value), dtype=np.int64)
        if total.value:
            _check(lib().femto_amd_locate_flat(self._h, n, _ptr(plen), _ptr(flat), _ptr(starts), max_occs,
                                               _ptr(noccs), _ptr(ostarts), _ptr(offs), total.value, C.byref(total)))
        return noccs, offs[:total.value]

    def locate_range(self, first, last):
        """text offsets of rows first..last (parallel_locate_range)"""
        out = np.zeros(max(0, last - first + 1), dtype=np.int64)
        _check(lib().femto_amd_parallel_locate_range(self._h, int(first), int(last), _ptr(out)))
        return out

    def locate(self, patterns, max_occs):
        return self.locate_flat(*flatten(patterns), max_occs)

    def pack_info(self):
        """small-alphabet packed lines (mode 3): {'available', 'bytes', 'build_ms', 'ktab_syms'}"""
        a, b, ms, k = C.c_int(0), C.c_int64(0), C.c_double(0), C.c_int(0)
        _check(lib().femto_amd_pack_info(self._h, C.byref(a), C.byref(b), C.byref(ms), C.byref(k)))
        return {"available": bool(a.value & 1), "available2": bool(a.value & 2), "level_table": bool(a.value & 4),
                "sa_full": bool(a.value & 8), "isa_full": bool(a.value & 16), "char_rank_lines": bool(a.value & 32), "context_table": bool(a.value & 64),
                "context_syms": (a.value >> 8) & 15, "context2_syms": (a.value >> 12) & 31, "context_mid_syms": (a.value >> 24) & 31, "rank_units": bool(a.value & (1 << 20)), "rank_units_marked": bool(a.value & (1 << 21)), "sa_32bit": bool(a.value & (1 << 22)),
                "bytes": b.value, "build_ms": ms.value, "ktab_syms": k.value}

    def structures(self):
        """femto_amd_structures: bytes of every structure the handle holds in HBM"""
        out = (C.c_int64 * 16)()
        _check(lib().femto_amd_structures(self._h, out, 16))
        names = ["image", "packed_lines", "marks", "rank_units", "level_table", "context_tables", "char_rank_lines", "text_sa_isa",
                 "two_level_lines", "derived_total", "mark_every", "level_table_syms", "mark_offset_bytes", "hbm_allocated", "hbm_budget",
                 "hbm_budget_is_default"]
        return {k: int(out[i]) for i, k in enumerate(names)}

    def document_info(self, doc):
        p, n = C.c_char_p(), C.c_int64(0)
        pv = C.c_void_p()
        _check(lib().femto_amd_document_info(self._h, int(doc), C.cast(C.byref(pv), C.POINTER(C.c_char_p)), C.byref(n)))
        return C.string_at(pv.value, n.value) if n.value else b""

    def block_requests(self, rows, ch_in=None, location=True):
        """block_request CHAR / OCCS / LOCATION per row: (L[row], occs in block, mark offset or -1); location=False asks for CHAR and
        OCCS only (off comes back None) -- in modes 3 / 4 such a call reads the derived lines alone"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n = len(rows)
        ch = np.zeros(n, dtype=np.uint16)
        occ = np.zeros(n, dtype=np.int32)
        off = np.zeros(n, dtype=np.int64) if location else None
        chin = np.ascontiguousarray(ch_in, dtype=np.uint16) if ch_in is not None else None
        _check(lib().femto_amd_block_requests(self._h, n, _ptr(rows), _ptr(chin), _ptr(ch), _ptr(occ), _ptr(off)))
        return ch, occ, off

    def forward_steps(self, rows):
        """do_forward_query per row: (ch, LF^-1 row or -1, mark offset or -1)"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n = len(rows)
        ch = np.zeros(n, dtype=np.uint16)
        nr = np.zeros(n, dtype=np.int64)
        off = np.zeros(n, dtype=np.int64)
        _check(lib().femto_amd_forward_steps(self._h, n, _ptr(rows), _ptr(ch), _ptr(nr), _ptr(off)))
        return ch, nr, off

    def resolve_location(self, offset):
        d, o = C.c_int64(), C.c_int64()
        _check(lib().femto_amd_resolve_location(self._h, offset, C.byref(d), C.byref(o)))
        return d.value, o.value

    def resolve_batch(self, offsets):
        """femto_amd_resolve_batch: (document int64[], offset in document int64[]) for host offsets, searched on the GPU"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        doc, off = np.zeros(len(offsets), dtype=np.int64), np.zeros(len(offsets), dtype=np.int64)
        _check(lib().femto_amd_resolve_batch(self._h, len(offsets), _ptr(offsets), _ptr(doc), _ptr(off)))
        return doc, off

    def resolve_device(self, d_offsets, n, d_doc=0, d_doc32=0, d_doc_offset=0, d_n=0, stream=0):
        """femto_amd_resolve_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_resolve_device(self._h, d_offsets, n, d_n or None, d_doc or None, d_doc32 or None, d_doc_offset or None,
                                              stream or None))

    # ---- extraction (femto_amd_extractor_*: do_context_query / do_extract_document_query)
    def extractor(self, sample_shift=-1, force_samples=False):
        """the handle's Extractor for these settings (made on first use, freed by close())"""
        if not hasattr(self, "_extractors"):
            self._extractors = {}
        key = (int(sample_shift), bool(force_samples))
        if key not in self._extractors:
            self._extractors[key] = Extractor(self, *key)
        return self._extractors[key]

    def extract(self, pos, lens, out_starts=None):
        return self.extractor().extract(pos, lens, out_starts)

    def extract_document(self, doc):
        return self.extractor().extract_document(doc)

    def context(self, rows=None, offsets=None, before=0, after=0):
        return self.extractor().context(rows=rows, offsets=offsets, before=before, after=after)

    def extract_device(self, n, d_pos, d_len, d_out_starts, d_out, stream=0):
        self.extractor().extract_device(n, d_pos, d_len, d_out_starts, d_out, stream)

    def context_device(self, n, d_rows=0, d_offsets=0, d_n=0, before=0, after=0, d_ctx=0, d_pos_out=0, stream=0):
        self.extractor().context_device(n, d_rows, d_offsets, d_n, before, after, d_ctx, d_pos_out, stream)

    # ---- common sequences (include/femto_amd.h "common sequences": src/main/similar_tool.c)
    def match_stats(self, data, max_len=0, ranges=True):
        """femto_amd_match_stats_device for host bytes: len int32[n] and, with ranges, (len, first int64[n], last int64[n]) -- for
        every end position j the longest data[j - len + 1 .. j] that occurs in the index and its range of rows"""
        import torch
        q = _u8(data)
        n = len(q)
        if n == 0:
            z = np.zeros(0, dtype=np.int64)
            return (np.zeros(0, dtype=np.int32), z, z.copy()) if ranges else np.zeros(0, dtype=np.int32)
        dev = "cuda:%d" % (self.device if isinstance(self.device, int) else self.device[0])
        buf = torch.zeros(n + 16, dtype=torch.uint8, device=dev)       # (8 bytes of slack on either side)
        buf[8:8 + n] = torch.from_numpy(q).to(dev)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_first = torch.zeros(n, dtype=torch.int64, device=dev) if ranges else None
        d_last = torch.zeros(n, dtype=torch.int64, device=dev) if ranges else None
        self.match_stats_device(n, buf.data_ptr() + 8, d_len, d_first, d_last, max_len=max_len)
        torch.cuda.synchronize()
        return (d_len.cpu().numpy(), d_first.cpu().numpy(), d_last.cpu().numpy()) if ranges else d_len.cpu().numpy()

    def similar(self, data, min_len=0, max_len=0, max_occs=0, not_indexes=()):
        """femto_amd_similar: the sequences `data` shares with the index, grouped, and the similarity scores (a Similar)"""
        q = _u8(data)
        nots = (C.c_void_p * max(1, len(not_indexes)))(*[ix._h for ix in not_indexes])
        r = SimilarResult()
        _check(lib().femto_amd_similar(self._h, _ptr(q) if len(q) else None, len(q), int(min_len), int(max_len), int(max_occs),
                                       len(not_indexes), nots if len(not_indexes) else None, C.byref(r)))
        try:
            return Similar(r)
        finally:
            lib().femto_amd_similar_free(C.byref(r))

    def match_stats_device(self, n, d_bytes, d_len, d_first=None, d_last=None, max_len=0, stream=0):
        """femto_amd_match_stats_device (torch tensors or raw device addresses; enqueue-only)"""
        _check(lib().femto_amd_match_stats_device(self._h, int(n), _dp(d_bytes), int(max_len), _dp(d_len), _dp(d_first), _dp(d_last), stream or None))

    def match_stats_steps_device(self, n, d_bytes, d_steps, max_len=0, stream=0):
        """femto_amd_match_stats_steps_device: d_steps[0] search steps, d_steps[1] those on a range of one row"""
        _check(lib().femto_amd_match_stats_steps_device(self._h, int(n), _dp(d_bytes), int(max_len), _dp(d_steps), stream or None))

    def common_sequences_device(self, n, d_len, d_first, d_last, d_seq_start, d_seq_len, d_seq_first, d_seq_last, capacity, d_total,
                                min_len=0, stream=0):
        """femto_amd_common_sequences_device (torch tensors or raw device addresses; enqueue-only)"""
        _check(lib().femto_amd_common_sequences_device(self._h, int(n), _dp(d_len), _dp(d_first), _dp(d_last), int(min_len), _dp(d_seq_start),
                                                       _dp(d_seq_len), _dp(d_seq_first), _dp(d_seq_last), int(capacity), _dp(d_total),
                                                       stream or None))

    def common_groups_device(self, capacity, d_total, d_seq_start, d_seq_len, d_seq_first, d_seq_last, d_group_of, d_g_len, d_g_first,
                             d_g_last, d_g_here, d_g_min_start, d_ngroups, stream=0):
        """femto_amd_common_groups_device (torch tensors or raw device addresses; enqueue-only)"""
        _check(lib().femto_amd_common_groups_device(self._h, int(capacity), _dp(d_total), _dp(d_seq_start), _dp(d_seq_len), _dp(d_seq_first),
                                                    _dp(d_seq_last), _dp(d_group_of), _dp(d_g_len), _dp(d_g_first), _dp(d_g_last),
                                                    _dp(d_g_here), _dp(d_g_min_start), _dp(d_ngroups), stream or None))

    def similar_documents_device(self, ngroups_capacity, d_ngroups, d_g_len, d_g_first, d_g_last, d_g_here, d_offsets, offsets_capacity,
                                 d_doc_score, d_doc_seqs, d_total, d_g_keep=None, max_occs=0, stream=0):
        """femto_amd_similar_documents_device (torch tensors or raw device addresses; enqueue-only)"""
        _check(lib().femto_amd_similar_documents_device(self._h, int(ngroups_capacity), _dp(d_ngroups), _dp(d_g_len), _dp(d_g_first),
                                                        _dp(d_g_last), _dp(d_g_here), _dp(d_g_keep), int(max_occs), _dp(d_offsets),
                                                        int(offsets_capacity), _dp(d_doc_score), _dp(d_doc_seqs), _dp(d_total),
                                                        stream or None))

    # ---- search with substitutions (include/femto_amd.h "search with substitutions")
    def mismatch(self, patterns, k):
        """femto_amd_mismatch: for every pattern (uint16 alpha codes) the variants with at most k substitutions that occur in the
        index.  Returns (result_start int64[n + 1], first int64[], last int64[], cost int32[], sub_pos int32[total, 2],
        sub_sym uint16[total, 2]): pattern i's results are entries result_start[i] .. result_start[i + 1] - 1, by first ascending;
        sub_pos = the substituted positions from the left, ascending, -1 for an unused slot; sub_sym = the substitutes"""
        plen, flat, _ = flatten(patterns)
        r = MismatchResult()
        _check(lib().femto_amd_mismatch(self._h, len(plen), _ptr(plen), _ptr(flat), int(k), C.byref(r)))
        try:
            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype=dtype)
            t = int(r.total)
            return (arr(r.result_start, int(r.npat) + 1, np.int64), arr(r.first, t, np.int64), arr(r.last, t, np.int64),
                    arr(r.cost, t, np.int32), arr(r.sub_pos, 2 * t, np.int32).reshape(t, 2), arr(r.sub_sym, 2 * t, np.uint16).reshape(t, 2))
        finally:
            lib().femto_amd_mismatch_free(C.byref(r))

    def mismatch_device(self, npat, nsyms, d_syms, d_starts, k, capacity, d_result_start, d_first, d_last, d_cost, d_sub_pos, d_sub_sym,
                        d_total, stream=0):
        """femto_amd_mismatch_device (torch tensors or raw device addresses; enqueue-only).  capacity = 0 with the five result arrays
        None: the counting form"""
        _check(lib().femto_amd_mismatch_device(self._h, int(npat), int(nsyms), _dp(d_syms), _dp(d_starts), int(k), int(capacity),
                                               _dp(d_result_start), _dp(d_first), _dp(d_last), _dp(d_cost), _dp(d_sub_pos), _dp(d_sub_sym),
                                               _dp(d_total), stream or None))

    # ---- search within edit distance (include/femto_amd.h "search within edit distance")
    def edit(self, patterns, k):
        """femto_amd_edit: for every pattern (uint16 alpha codes) the distinct strings within k substitutions, deletions and
        insertions of it that occur in the index.  Returns (result_start int64[n + 1], first int64[], last int64[], cost int32[],
        length int32[]): pattern i's results are entries result_start[i] .. result_start[i + 1] - 1, by first, then length ascending;
        cost = the fewest operations that reach the string, length = its symbols.  The ranges of one pattern may nest"""
        plen, flat, _ = flatten(patterns)
        r = EditResult()
        _check(lib().femto_amd_edit(self._h, len(plen), _ptr(plen), _ptr(flat), int(k), C.byref(r)))
        try:
            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype=dtype)
            t = int(r.total)
            return (arr(r.result_start, int(r.npat) + 1, np.int64), arr(r.first, t, np.int64), arr(r.last, t, np.int64),
                    arr(r.cost, t, np.int32), arr(r.length, t, np.int32))
        finally:
            lib().femto_amd_edit_free(C.byref(r))

    def edit_device(self, npat, nsyms, d_syms, d_starts, k, capacity, d_result_start, d_first, d_last, d_cost, d_length, d_total, stream=0):
        """femto_amd_edit_device (torch tensors or raw device addresses; enqueue-only).  capacity bounds the RAW records; capacity = 0
        with the result arrays None: the counting form.  d_total int64[3] = {distinct results, overflow, raw records}"""
        _check(lib().femto_amd_edit_device(self._h, int(npat), int(nsyms), _dp(d_syms), _dp(d_starts), int(k), int(capacity),
                                           _dp(d_result_start), _dp(d_first), _dp(d_last), _dp(d_cost), _dp(d_length), _dp(d_total),
                                           stream or None))

    # ---- search with character classes (include/femto_amd.h "search with character classes")
    def classes(self, patterns, classes):
        """femto_amd_classes: for every pattern (uint16 symbols: an alpha code, or CLASS_SYMBOL | c for class c) the distinct strings
        that occur in the index with the literal at every literal position and a member of the class at every class position.
        classes = uint64[n, 4]: bit b of word w of a class says that byte 64 w + b belongs to it (class_patterns and iupac_patterns
        make both).  Returns (result_start int64[n + 1], first int64[], last int64[]): pattern i's results are entries
        result_start[i] .. result_start[i + 1] - 1, by first ascending"""
        plen, flat, _ = flatten(patterns)
        table = np.ascontiguousarray(classes, dtype=np.uint64).reshape(-1, 4)
        r = ClassesResult()
        _check(lib().femto_amd_classes(self._h, len(plen), _ptr(plen), _ptr(flat), len(table), _ptr(table) if len(table) else None, C.byref(r)))
        try:
            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype=dtype)
            t = int(r.total)
            return arr(r.result_start, int(r.npat) + 1, np.int64), arr(r.first, t, np.int64), arr(r.last, t, np.int64)
        finally:
            lib().femto_amd_classes_free(C.byref(r))

    def classes_device(self, npat, nsyms, d_syms, d_starts, nclasses, d_classes, capacity, d_result_start, d_first, d_last, d_total, stream=0):
        """femto_amd_classes_device (torch tensors or raw device addresses; enqueue-only).  capacity = 0 with d_first and d_last None:
        the counting form"""
        _check(lib().femto_amd_classes_device(self._h, int(npat), int(nsyms), _dp(d_syms), _dp(d_starts), int(nclasses), _dp(d_classes),
                                              int(capacity), _dp(d_result_start), _dp(d_first), _dp(d_last), _dp(d_total), stream or None))

    # ---- occurrences within k substitutions (include/femto_amd.h "occurrences within k substitutions, by exact seeds")
    def hamming(self, patterns, k, sample_shift=-1, force_samples=False):
        """femto_amd_hamming through the handle's extractor: (result_start int64[n + 1], offset int64[], cost int32[], candidates)"""
        return self.extractor(sample_shift, force_samples).hamming(patterns, k)

    def hamming_device(self, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, d_offset, d_cost, d_total, stream=0,
                       sample_shift=-1, force_samples=False):
        """femto_amd_hamming_device through the handle's extractor"""
        self.extractor(sample_shift, force_samples).hamming_device(npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start,
                                                                   d_offset, d_cost, d_total, stream)

    def leven(self, patterns, k, sample_shift=-1, force_samples=False):
        """femto_amd_leven through the handle's extractor: (result_start int64[n + 1], offset int64[], cost int32[], length int32[],
        candidates, raw)"""
        return self.extractor(sample_shift, force_samples).leven(patterns, k)

    def leven_device(self, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, d_offset, d_cost, d_length, d_total, stream=0,
                     sample_shift=-1, force_samples=False):
        """femto_amd_leven_device through the handle's extractor"""
        self.extractor(sample_shift, force_samples).leven_device(npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start,
                                                                 d_offset, d_cost, d_length, d_total, stream)

    # ---- document listing (femto_amd_doclist*: results_create_sort_locations; femto_amd_docset*: AND / OR / NOT of the lists)
    def documents(self, patterns, max_occs):
        """femto_amd_doclist: (doc_starts int64[n + 1], docs int64[], hits int32[]) -- pattern i's distinct documents, ascending,
        and its located rows per document are entries doc_starts[i] .. doc_starts[i + 1] - 1"""
        plen, flat, starts = flatten(patterns)
        n = len(plen)
        doc_starts = np.zeros(n + 1, dtype=np.int64)
        pd, ph, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_doclist(self._h, n, _ptr(plen), _ptr(flat), _ptr(starts), int(max_occs), _ptr(doc_starts), C.byref(pd),
                                       C.byref(ph), C.byref(total)))
        if not total.value:
            return doc_starts, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        try:
            docs = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_int64)), shape=(total.value,)).copy()
            hits = np.ctypeslib.as_array(C.cast(ph, C.POINTER(C.c_int32)), shape=(total.value,)).copy()
        finally:
            _libc_free(pd)
            _libc_free(ph)
        return doc_starts, docs, hits

    def doclist_device(self, npats, d_out_starts, d_offsets, capacity, d_total, d_ndocs=0, d_docs=0, d_docs32=0, d_hits=0, d_pair_doc=0,
                       d_pair_off=0, d_doc_total=0, d_status=0, stream=0):
        """femto_amd_doclist_device on raw device addresses (0 = NULL): the arrays femto_amd_locate_device left -> per-pattern
        document lists in the rows' ragged layout; enqueue-only"""
        _check(lib().femto_amd_doclist_device(self._h, int(npats), d_out_starts or None, d_offsets or None, int(capacity), d_total or None,
                                              d_ndocs or None, d_docs or None, d_docs32 or None, d_hits or None, d_pair_doc or None,
                                              d_pair_off or None, d_doc_total or None, d_status or None, stream or None))

    def docset_device(self, npairs, d_docs_a, d_a_start, d_a_n, d_docs_b, d_b_start, d_b_n, d_op, d_res_starts, d_res_docs, res_capacity,
                      d_res_total, stream=0):
        """femto_amd_docset_device on raw device addresses: pair k = list a[k] op[k] list b[k] (DOCSET_AND / _OR / _NOT), packed"""
        _check(lib().femto_amd_docset_device(self._h, int(npairs), d_docs_a or None, d_a_start or None, d_a_n or None, d_docs_b or None,
                                             d_b_start or None, d_b_n or None, d_op or None, d_res_starts or None, d_res_docs or None,
                                             int(res_capacity), d_res_total or None, stream or None))

    def docset(self, a_lists, b_lists, ops):
        """femto_amd_docset on host lists (each ascending, no duplicates): (res_starts int64[n + 1], res_docs int64[])"""
        n = len(ops)

        def pack(lists):
            ln = np.array([len(x) for x in lists], dtype=np.int32)
            st = np.zeros(n, dtype=np.int64)
            if n:
                st[1:] = np.cumsum(ln[:-1], dtype=np.int64)
            flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if n and ln.sum() else np.zeros(1, dtype=np.int64)
            return np.ascontiguousarray(flat), st, ln

        (fa, sa, na), (fb, sb, nb) = pack(a_lists), pack(b_lists)
        op = np.ascontiguousarray(ops, dtype=np.int32)
        res_starts = np.zeros(n + 1, dtype=np.int64)
        pr, total = C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_docset(self._h, n, _ptr(fa), _ptr(sa), _ptr(na), _ptr(fb), _ptr(sb), _ptr(nb), _ptr(op), _ptr(res_starts),
                                      C.byref(pr), C.byref(total)))
        if not total.value:
            return res_starts, np.zeros(0, dtype=np.int64)
        try:
            return res_starts, np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_int64)), shape=(total.value,)).copy()
        finally:
            _libc_free(pr)

    # ---- positional operators (femto_amd_docpos*: thenResults / withinResults / unionResults on (document, offset) lists)
    @staticmethod
    def _pairs_back(n, res_starts, pd, po, total):
        if not total.value:
            return res_starts, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        try:
            return (res_starts, np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_int64)), shape=(total.value,)).copy(),
                    np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_int64)), shape=(total.value,)).copy())
        finally:
            _libc_free(pd)
            _libc_free(po)

    def docpos(self, a_lists, b_lists, ops, distances):
        """femto_amd_docpos on host lists, each an (n, 2) array of (document, offset) rows, strictly ascending: job k = a[k]
        ops[k] b[k] (DOCPOS_THEN / _WITHIN / _OR) at distances[k]; (res_starts int64[n + 1], res_doc int64[], res_off int64[])"""
        n = len(ops)

        def pack(lists):
            arrs = [np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in lists]
            ln = np.array([len(x) for x in arrs], dtype=np.int32)
            st = np.zeros(n, dtype=np.int64)
            if n:
                st[1:] = np.cumsum(ln[:-1], dtype=np.int64)
            flat = np.concatenate(arrs) if n and ln.sum() else np.zeros((1, 2), dtype=np.int64)
            return np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1]), st, ln

        (ad, ao, sa, na), (bd, bo, sb, nb) = pack(a_lists), pack(b_lists)
        op = np.ascontiguousarray(ops, dtype=np.int32)
        di = np.ascontiguousarray(distances, dtype=np.int32)
        res_starts = np.zeros(n + 1, dtype=np.int64)
        pd, po, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_docpos(self._h, n, _ptr(ad), _ptr(ao), _ptr(sa), _ptr(na), _ptr(bd), _ptr(bo), _ptr(sb), _ptr(nb), _ptr(op),
                                      _ptr(di), _ptr(res_starts), C.byref(pd), C.byref(po), C.byref(total)))
        return self._pairs_back(n, res_starts, pd, po, total)

    def proximity(self, left, right, ops, distances, max_occs):
        """femto_amd_proximity: pattern pair k = left[k] ops[k] right[k] at distances[k], over the rows located under the clamp
        max_occs; (res_starts int64[n + 1], res_doc int64[], res_off int64[])"""
        n = len(ops)
        lp, lf, ls = flatten(left)
        rp, rf, rs = flatten(right)
        op = np.ascontiguousarray(ops, dtype=np.int32)
        di = np.ascontiguousarray(distances, dtype=np.int32)
        res_starts = np.zeros(n + 1, dtype=np.int64)
        pd, po, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_proximity(self._h, n, _ptr(lp), _ptr(lf), _ptr(ls), _ptr(rp), _ptr(rf), _ptr(rs), _ptr(op), _ptr(di),
                                         int(max_occs), _ptr(res_starts), C.byref(pd), C.byref(po), C.byref(total)))
        return self._pairs_back(n, res_starts, pd, po, total)

    # ---- boolean queries (femto_amd_bquery*: the query language's AND OR NOT THEN WITHIN, a batch of trees at once)
    def bquery_run_batch(self, queries, max_occs):
        """femto_amd_bquery_run_batch over BooleanQuery objects: (res_starts int64[n + 1], res_type int32[n], res_doc int64[],
        res_off int64[]) -- query k's result is entries res_starts[k] .. res_starts[k + 1] - 1, documents (BQUERY_DOCUMENTS,
        offsets 0) or (document, offset) pairs (BQUERY_PAIRS)"""
        n = len(queries)
        handles = (C.c_void_p * max(1, n))(*[q._h for q in queries])
        res_starts = np.zeros(n + 1, dtype=np.int64)
        res_type = np.zeros(max(1, n), dtype=np.int32)
        pd, po, total = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_bquery_run_batch(self._h, n, C.cast(handles, C.c_void_p), int(max_occs), _ptr(res_starts), _ptr(res_type),
                                                C.byref(pd), C.byref(po), C.byref(total)))
        return (res_starts, res_type[:n]) + self._pairs_back(n, res_starts, pd, po, total)[1:]

    def docpos_device(self, npairs, d_a_doc, d_a_off, d_a_start, d_a_n, d_b_doc, d_b_off, d_b_start, d_b_n, d_op, d_distance, d_res_starts,
                      d_res_doc, d_res_off, res_capacity, d_res_total, stream=0):
        """femto_amd_docpos_device on raw device addresses: job k = list a[k] op[k] list b[k] at d_distance[k], packed; enqueue-only"""
        _check(lib().femto_amd_docpos_device(self._h, int(npairs), d_a_doc or None, d_a_off or None, d_a_start or None, d_a_n or None,
                                             d_b_doc or None, d_b_off or None, d_b_start or None, d_b_n or None, d_op or None,
                                             d_distance or None, d_res_starts or None, d_res_doc or None, d_res_off or None,
                                             int(res_capacity), d_res_total or None, stream or None))

    def docpos_documents_device(self, nlists, d_starts, d_pair_doc, d_doc_starts, d_docs, doc_capacity, d_total, stream=0):
        """femto_amd_docpos_documents_device on raw device addresses: the distinct documents of packed pair lists; enqueue-only"""
        _check(lib().femto_amd_docpos_documents_device(self._h, int(nlists), d_starts or None, d_pair_doc or None, d_doc_starts or None,
                                                       d_docs or None, int(doc_capacity), d_total or None, stream or None))

    # ---- device-pointer API (raw pointers, e.g. torch tensors' data_ptr())
    def count_device(self, npats, d_plen, d_pats, d_starts, d_first, d_last, stream=0):
        _check(lib().femto_amd_count_device(self._h, npats, d_plen, d_pats, d_starts, d_first, d_last or None,
                                            stream or None))

    def locate_plan_device(self, npats, d_plen, d_pats, d_starts, max_occs, d_first, d_last, d_noccs, d_out_starts,
                           stream=0):
        _check(lib().femto_amd_locate_plan_device(self._h, npats, d_plen, d_pats, d_starts, max_occs, d_first, d_last,
                                                  d_noccs, d_out_starts, stream or None))

    def pack_counts_device(self, npats, d_first, d_last, d_counts8, d_big, big_capacity, d_big_n, stream=0):
        """match counts as one byte per pattern + (pattern, count) pairs for counts >= 255 (femto_amd_pack_counts_device)"""
        _check(lib().femto_amd_pack_counts_device(self._h, npats, d_first, d_last, d_counts8, d_big or None, big_capacity, d_big_n,
                                                  stream or None))

    def locate_walk_device(self, npats, d_first, d_out_starts, total, d_offsets, stream=0):
        _check(lib().femto_amd_locate_walk_device(self._h, npats, d_first, d_out_starts, total, d_offsets,
                                                  stream or None))

    def locate_device(self, npats, d_plen, d_pats, d_starts, max_occs, d_first, d_last, d_noccs, d_out_starts, d_offsets,
                      capacity, d_total, stream=0):
        """count + clamp + prefix sum + locate walk in ONE enqueue-only call (femto_amd_locate_device_v2)"""
        _check(lib().femto_amd_locate_device_v2(self._h, npats, d_plen, d_pats, d_starts, max_occs, d_first, d_last, d_noccs,
                                             d_out_starts, d_offsets, capacity, d_total, stream or None))

    TRACE_REGIONS = ("pack_lines", "level_table", "suffix_array", "level1_lines", "level2_lines", "text", "isa", "rank_units", "char_rank_lines",
                     "context_table")

    def trace_lines(self, npats, d_plen, d_pats, d_starts, max_occs):
        """distinct 128-byte lines per derived array loaded by the count phase and by the locate phase of this batch"""
        cl = np.zeros(10, dtype=np.int64)
        ll = np.zeros(10, dtype=np.int64)
        rows = C.c_int64(0)
        _check(lib().femto_amd_trace_lines(self._h, npats, d_plen, d_pats, d_starts, max_occs, _ptr(cl), _ptr(ll), C.byref(rows)))
        return dict(zip(self.TRACE_REGIONS, cl.tolist())), dict(zip(self.TRACE_REGIONS, ll.tolist())), rows.value

    def trace_reads(self):
        """line READS (not only distinct lines) per derived array of the count / the locate phase of the last trace_lines call"""
        cr = np.zeros(10, dtype=np.int64)
        lr = np.zeros(10, dtype=np.int64)
        _check(lib().femto_amd_trace_reads(self._h, _ptr(cr), _ptr(lr)))
        return dict(zip(self.TRACE_REGIONS, cr.tolist())), dict(zip(self.TRACE_REGIONS, lr.tolist()))

    # ---- multi-process gather of device-resident results (RCCL send/recv, femto_amd_comm_*)
    @staticmethod
    def comm_unique_id():
        blob = C.create_string_buffer(128)
        _check(lib().femto_amd_comm_unique_id(blob))
        return blob.raw

    def comm_init(self, id128, nranks, rank):
        _check(lib().femto_amd_comm_init(self._h, C.create_string_buffer(bytes(id128), 128), int(nranks), int(rank)))

    def comm_info(self):
        """{'nranks', 'rank'} as the RCCL communicator reports them"""
        n, r = C.c_int(0), C.c_int(0)
        _check(lib().femto_amd_comm_info(self._h, C.byref(n), C.byref(r)))
        return {"nranks": n.value, "rank": r.value}

    def comm_gather(self, d_send, d_recv, bytes_per_rank, root=0, stream=0):
        _check(lib().femto_amd_comm_gather(self._h, d_send, d_recv or None, int(bytes_per_rank), int(root), stream or None))

    def key_format(self):
        """(bits per field, symbols per key, field_of_alpha uint8[261]) of femto_amd_key_format"""
        bits, syms = C.c_int32(), C.c_int32()
        table = np.zeros(261, dtype=np.uint8)
        _check(lib().femto_amd_key_format(self._h, C.byref(bits), C.byref(syms), _ptr(table)))
        return bits.value, syms.value, table

    def lf_steps_device(self, n, d_rows, d_next, d_off, stream=0):
        """femto_amd_lf_steps_device on raw device addresses: one step of the locate walk per row (offset if marked, else LF(row))"""
        _check(lib().femto_amd_lf_steps_device(self._h, int(n), d_rows, d_next, d_off, stream or None))

    def key_table_id(self):
        """identity of the key fields (femto_amd_key_table_id): keys built for one id are meaningless to a handle reporting another"""
        v = C.c_uint64(0)
        _check(lib().femto_amd_key_table_id(self._h, C.byref(v)))
        return v.value

    def pack_keys_device(self, npats, d_plen, d_pats, d_starts, d_keys, d_bad, stream=0):
        _check(lib().femto_amd_pack_keys_device(self._h, int(npats), d_plen, d_pats, d_starts, d_keys, d_bad, stream or None))

    def locate_keys_device(self, npats, d_keys, max_occs, d_ranges32, d_first, d_last, d_noccs, d_out_starts, d_offsets, capacity, d_total,
                           stream=0):
        """femto_amd_locate_keys_device on raw device addresses (0 / None = NULL)"""
        _check(lib().femto_amd_locate_keys_device(self._h, int(npats), d_keys, int(max_occs), d_ranges32 or None, d_first or None,
                                                  d_last or None, d_noccs or None, d_out_starts or None, d_offsets or None,
                                                  int(capacity), d_total or None, stream or None))

    def nfa_search_batch(self, nfas, max_results=1 << 20):
        """femto_amd_nfa_search_batch: do_regexp_query (src/main/server.c:1656) for a batch of automata on the GPU.
        Returns (result_start int64[n+1], first, last, match_len, cost, status int32[n]): automaton q's results are entries
        result_start[q] .. result_start[q+1]-1, in the order of the reference's sorted result list."""
        if isinstance(nfas, NfaBatch):
            n, arr = nfas.n, nfas.arr
        else:
            nfas = list(nfas)
            n = len(nfas)
            arr = (NfaStruct * max(1, n))(*[a.struct() for a in nfas])
        start = np.zeros(n + 1, dtype=np.int64)
        status = np.zeros(max(1, n), dtype=np.int32)
        m = max(0, int(max_results))      # 0: count only (result_start and the total; the result arrays come back empty)
        first, last = np.zeros(max(1, m), dtype=np.int64), np.zeros(max(1, m), dtype=np.int64)
        mlen, cost = np.zeros(max(1, m), dtype=np.int32), np.zeros(max(1, m), dtype=np.int32)
        tot = C.c_int64(0)
        self.last_total = 0
        try:
            _check(lib().femto_amd_nfa_search_batch(self._h, n, C.cast(arr, C.c_void_p), m, _ptr(start), _ptr(first), _ptr(last), _ptr(mlen),
                                                    _ptr(cost), _ptr(status), C.byref(tot)))
        finally:
            self.last_total = tot.value      # after ERR_FULL: the max_results to call again with
        k = tot.value if m else 0
        return start, first[:k], last[:k], mlen[:k], cost[:k], status[:n]

    def regexp_search_batch(self, regexes, max_results=1 << 20, approx=None):
        """compile every pattern (Nfa.from_regex) and search them as one batch"""
        return self.nfa_search_batch([Nfa.from_regex(r, approx) for r in regexes], max_results)

    def regexp_search(self, regex, max_results=1 << 20, approx=None):
        """the sorted result list of do_regexp_query for one byte regular expression -- or, approx=(max_cost, subst, delete,
        insert), its APPROX form: (first int64[], last int64[], match_len int32[][, cost int32[]]); a range whose string
        matches is a result and is not extended (the reference's rule), ranges inside another result are dropped"""
        rx = np.frombuffer(bytes(regex) + b"\0", dtype=np.uint8)
        k = (0, 1, 1, 1) if approx is None else tuple(int(v) for v in approx)
        n = C.c_int64(0)
        m = max(1, int(max_results))
        first, last = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        mlen, cost = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        _check(lib().femto_amd_regexp_search_approx(self._h, _ptr(rx), len(regex), k[0], k[1], k[2], k[3], m, _ptr(first), _ptr(last),
                                                    _ptr(mlen), _ptr(cost), C.byref(n)))
        if approx is None:
            return first[:n.value], last[:n.value], mlen[:n.value]
        return first[:n.value], last[:n.value], mlen[:n.value], cost[:n.value]

    def nfa_stats(self, thread=False):
        """the last automaton batch (thread=True: of the calling thread): pops, span, workgroup occupancy (femto_amd_nfa_stats)"""
        out = (C.c_double * 8)()
        _check(lib().femto_amd_nfa_stats(None if thread else self._h, out))
        keys = ("automata", "workgroups", "pops", "pops_longest", "busy_s", "span_s", "occupancy", "longest_waited_s")
        return dict(zip(keys, [float(v) for v in out]))

    def set_option(self, name, value):
        """'sort' (suffix-order batches of the wavelet-path kernels), 'regexp_max_iterations', 'regexp_stack_cap'"""
        _check(lib().femto_amd_set_option(self._h, name.encode(), int(value)))

    def set_rank_mode(self, mode):
        """3 / 4 = packed / two-level lines (the defaults where they exist), 1 = lane per query on femto's wavelet tree,
        0 = wavefront-per-query walk of femto's raw tables"""
        _check(lib().femto_amd_set_rank_mode(self._h, mode))

    @property
    def rank_mode(self):
        return lib().femto_amd_get_rank_mode(self._h)

    def kernel_time(self, name):
        ms, n = C.c_double(), C.c_int64()
        _check(lib().femto_amd_kernel_time_ms(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_enable(self, on=True):
        lib().femto_amd_kernel_time_enable(self._h, 1 if on else 0)

    def kernel_time_reset(self):
        lib().femto_amd_kernel_time_reset(self._h)


class Extractor:
    """femto_amd_extractor_t: text, documents and contexts of an Index (include/femto_amd.h "extraction").  Use
    Index.extractor(); it is freed by Index.close()."""

    PATH_TEXT, PATH_SAMPLES = 0, 1

    def __init__(self, index, sample_shift=-1, force_samples=False):
        self._h = C.c_void_p()
        self.index = index
        _check(lib().femto_amd_extractor_open(index._h, int(sample_shift), 1 if force_samples else 0, C.byref(self._h)))

    def free(self):
        if self._h:
            lib().femto_amd_extractor_free(self._h)
            self._h = C.c_void_p()

    def info(self):
        path, shift, nbytes, ms = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_double(0)
        _check(lib().femto_amd_extractor_info(self._h, C.byref(path), C.byref(shift), C.byref(nbytes), C.byref(ms)))
        return {"path": path.value, "sample_shift": shift.value, "bytes": nbytes.value, "build_ms": ms.value}

    def eof_rows(self):
        out = np.zeros(int(self.index.info.number_of_documents), dtype=np.int64)
        _check(lib().femto_amd_extractor_eof_rows(self._h, _ptr(out), len(out)))
        return out

    def extract(self, pos, lens, out_starts=None):
        """T[pos[i] : pos[i] + lens[i]] for every i (uint16); packed one after another unless out_starts is given (then an
        array of max(out_starts + lens) symbols, zero where nothing was written)"""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if out_starts is None:
            out = np.zeros(max(int(lens.astype(np.int64).clip(0).sum()), 1), dtype=np.uint16)
        else:
            out_starts = np.ascontiguousarray(out_starts, dtype=np.int64)
            out = np.zeros(max(int((out_starts + lens).max()) if len(lens) else 0, 1), dtype=np.uint16)
        _check(lib().femto_amd_extract(self._h, len(pos), _ptr(pos), _ptr(lens), _ptr(out_starts), _ptr(out)))
        return out[:int(lens.astype(np.int64).sum())] if out_starts is None else out

    def extract_document(self, doc):
        p, n = C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_extract_document(self._h, int(doc), C.byref(p), C.byref(n)))
        try:
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint16)), shape=(n.value,)).copy() if n.value else \
                np.zeros(0, dtype=np.uint16)
        finally:
            _libc_free(p)

    def context(self, rows=None, offsets=None, before=0, after=0):
        """(ctx uint16[n, before + after], p int64[n]) around rows (SA[row]) or text offsets"""
        a = np.ascontiguousarray(rows if rows is not None else offsets, dtype=np.int64)
        ctx = np.zeros((len(a), before + after), dtype=np.uint16)
        pos = np.zeros(len(a), dtype=np.int64)
        _check(lib().femto_amd_context(self._h, len(a), _ptr(a) if rows is not None else None, _ptr(a) if rows is None else None,
                                       int(before), int(after), C.c_void_p(ctx.ctypes.data) if ctx.size else None, _ptr(pos)))
        return ctx, pos

    def extract_device(self, n, d_pos, d_len, d_out_starts, d_out, stream=0):
        """femto_amd_extract_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_extract_device(self._h, n, d_pos, d_len, d_out_starts, d_out, stream or None))

    def context_device(self, n, d_rows=0, d_offsets=0, d_n=0, before=0, after=0, d_ctx=0, d_pos_out=0, stream=0):
        """femto_amd_context_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_context_device(self._h, n, d_rows or None, d_offsets or None, d_n or None, int(before), int(after),
                                              d_ctx or None, d_pos_out or None, stream or None))

    # ---- matching lines (include/femto_amd.h "matching lines": print_grep's rule over the document's bytes)
    LINE_BINARY, LINE_INVALID = 1, 2

    def lines(self, offsets, with_bytes=True):
        """the line around every text offset: (doc int64[n], line_pos int64[n], line_len int32[n], flags uint8[n]) and, with_bytes,
        (byte_starts int64[n + 1], bytes uint8[]) -- the lines packed one after another"""
        a = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(a)
        doc, pos = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        lens, flags = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        if not with_bytes:
            _check(lib().femto_amd_lines(self._h, n, _ptr(a), _ptr(doc), _ptr(pos), _ptr(lens), _ptr(flags), None, None, None))
            return doc, pos, lens, flags
        starts = np.zeros(n + 1, dtype=np.int64)
        p, total = C.c_void_p(), C.c_int64(0)
        _check(lib().femto_amd_lines(self._h, n, _ptr(a), _ptr(doc), _ptr(pos), _ptr(lens), _ptr(flags), _ptr(starts), C.byref(p), C.byref(total)))
        try:
            data = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total.value,)).copy() if total.value else \
                np.zeros(0, dtype=np.uint8)
        finally:
            _libc_free(p)
        return doc, pos, lens, flags, starts, data

    def line_groups(self, byte_starts, data, flags=None, hash_bits=0):
        """(group_first int64[n], number of distinct lines) of n packed lines: group_first[i] = the least j whose line has the
        bytes of line i, -1 where flags says LINE_INVALID.  hash_bits 1..63 keeps only that many bits of the hash (a diagnostic)"""
        starts = np.ascontiguousarray(byte_starts, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = len(starts) - 1
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        gf, ng = np.zeros(n, dtype=np.int64), C.c_int64(0)
        _check(lib().femto_amd_line_groups(self._h, n, _ptr(starts), _ptr(data) if len(data) else None, _ptr(fl), int(hash_bits), _ptr(gf),
                                           C.byref(ng)))
        return gf, ng.value

    def lines_device(self, n, d_offsets, d_n=0, d_doc=0, d_line_pos=0, d_line_len=0, d_flags=0, stream=0):
        """femto_amd_lines_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_lines_device(self._h, n, d_offsets or None, d_n or None, d_doc or None, d_line_pos or None, d_line_len or None,
                                            d_flags or None, stream or None))

    def line_bytes_device(self, n, d_line_pos, d_line_len, d_byte_starts, d_bytes, capacity, d_total, d_n=0, stream=0):
        """femto_amd_line_bytes_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_line_bytes_device(self._h, n, d_n or None, d_line_pos or None, d_line_len or None, d_byte_starts or None,
                                                 d_bytes or None, int(capacity), d_total or None, stream or None))

    def line_groups_device(self, n, d_byte_starts, d_bytes, d_group_first, d_ngroups, d_flags=0, d_n=0, hash_bits=0, stream=0):
        """femto_amd_line_groups_device (raw device pointers; enqueue-only)"""
        _check(lib().femto_amd_line_groups_device(self._h, n, d_n or None, d_byte_starts or None, d_bytes or None, d_flags or None, int(hash_bits),
                                                  d_group_first or None, d_ngroups or None, stream or None))

    # ---- occurrences within k substitutions (include/femto_amd.h "occurrences within k substitutions, by exact seeds")
    def hamming(self, patterns, k):
        """femto_amd_hamming: for every pattern (uint16 alpha codes of byte characters, more than k of them) the text offsets where it
        occurs with at most k substitutions.  Returns (result_start int64[n + 1], offset int64[], cost int32[], candidates): pattern
        i's results are entries result_start[i] .. result_start[i + 1] - 1, offsets ascending; candidates = the located pieces"""
        plen, flat, _ = flatten(patterns)
        r = HammingResult()
        _check(lib().femto_amd_hamming(self._h, len(plen), _ptr(plen), _ptr(flat), int(k), C.byref(r)))
        try:
            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype=dtype)
            t = int(r.total)
            return arr(r.result_start, int(r.npat) + 1, np.int64), arr(r.offset, t, np.int64), arr(r.cost, t, np.int32), int(r.candidates)
        finally:
            lib().femto_amd_hamming_free(C.byref(r))

    def hamming_device(self, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, d_offset, d_cost, d_total, stream=0):
        """femto_amd_hamming_device (torch tensors or raw device addresses; enqueue-only on the text path).  capacity = 0 with d_offset
        and d_cost None: the counting form.  d_total holds four words: results, their overflow, candidates, their overflow"""
        _check(lib().femto_amd_hamming_device(self._h, int(npat), int(nsyms), _dp(d_syms), _dp(d_starts), int(k), int(cand_capacity),
                                              int(capacity), _dp(d_result_start), _dp(d_offset), _dp(d_cost), _dp(d_total), stream or None))

    # ---- occurrences within k edits (include/femto_amd.h "occurrences within k edits, by exact seeds")
    def leven(self, patterns, k):
        """femto_amd_leven: for every pattern (uint16 alpha codes of byte characters, more than k of them) the text offsets where a
        string within Levenshtein distance k of it starts.  Returns (result_start int64[n + 1], offset int64[], cost int32[],
        length int32[], candidates, raw): pattern i's results are entries result_start[i] .. result_start[i + 1] - 1, offsets
        ascending, each with the least cost and the shortest length that reaches it; candidates = the located pieces, raw = the
        records before de-duplication"""
        plen, flat, _ = flatten(patterns)
        r = LevenResult()
        _check(lib().femto_amd_leven(self._h, len(plen), _ptr(plen), _ptr(flat), int(k), C.byref(r)))
        try:
            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype=dtype)
            t = int(r.total)
            return (arr(r.result_start, int(r.npat) + 1, np.int64), arr(r.offset, t, np.int64), arr(r.cost, t, np.int32),
                    arr(r.length, t, np.int32), int(r.candidates), int(r.raw))
        finally:
            lib().femto_amd_leven_free(C.byref(r))

    def leven_device(self, npat, nsyms, d_syms, d_starts, k, cand_capacity, capacity, d_result_start, d_offset, d_cost, d_length, d_total,
                     stream=0):
        """femto_amd_leven_device (torch tensors or raw device addresses; enqueue-only on the text path).  capacity = 0 with d_offset,
        d_cost and d_length None: the counting form.  d_total holds five words: distinct results, the raw records' overflow, raw
        records, candidates, their overflow"""
        _check(lib().femto_amd_leven_device(self._h, int(npat), int(nsyms), _dp(d_syms), _dp(d_starts), int(k), int(cand_capacity),
                                            int(capacity), _dp(d_result_start), _dp(d_offset), _dp(d_cost), _dp(d_length), _dp(d_total),
                                            stream or None))


DOCSET_AND, DOCSET_OR, DOCSET_NOT = 0, 1, 2


def doclist_info():
    """(wave_max, workgroup_max): the largest segment one wavefront / one workgroup lists (femto_amd_doclist_info)"""
    w, g = C.c_int(0), C.c_int(0)
    _check(lib().femto_amd_doclist_info(C.byref(w), C.byref(g)))
    return w.value, g.value


DOCPOS_THEN, DOCPOS_WITHIN, DOCPOS_OR = 0, 1, 2


def docpos_info():
    """tile: the merged positions one workgroup takes (femto_amd_docpos_info)"""
    t = C.c_int(0)
    _check(lib().femto_amd_docpos_info(C.byref(t)))
    return t.value


def docpos_chunks():
    """the chunks the tiles of one call are dealt into (femto_amd_docpos_chunks)"""
    return int(lib().femto_amd_docpos_chunks())


BQUERY_LEAF, BQUERY_AND, BQUERY_OR, BQUERY_NOT, BQUERY_THEN, BQUERY_WITHIN = 0, 1, 2, 3, 4, 5
BQUERY_DOCUMENTS, BQUERY_PAIRS = 0, 1


class BooleanQuery:
    """femto_amd_bquery_compile: a query with AND OR NOT THEN WITHIN as a typed tree.  nodes: the tree in postfix order, one
    dict per node -- op (BQUERY_*), distance, left, right (node numbers, -1 for a leaf) and, for a leaf, literal (alpha codes or
    None), settings (cost_bound, subst, delete, insert) and echo; result_type; echo (ast_to_string of the whole tree)."""

    def __init__(self, query, icase=False, streamline=True):
        q = np.frombuffer(bytes(query) + b"\0", dtype=np.uint8)
        self._h = C.c_void_p()
        _check(lib().femto_amd_bquery_compile(_ptr(q), len(query), (1 if icase else 0) | (0 if streamline else 2), C.byref(self._h)))
        nn, nl, rt = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(lib().femto_amd_bquery_info(self._h, C.byref(nn), C.byref(nl), C.byref(rt)))
        self.num_leaves, self.result_type = nl.value, rt.value
        self.echo = lib().femto_amd_bquery_echo(self._h)
        self.nodes = []
        for i in range(nn.value):
            op, di, le, ri, lf = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_void_p()
            _check(lib().femto_amd_bquery_node(self._h, i, C.byref(op), C.byref(di), C.byref(le), C.byref(ri), C.byref(lf)))
            node = {"op": op.value, "distance": di.value, "left": le.value, "right": ri.value}
            if op.value == BQUERY_LEAF:
                v = lib().femto_amd_regexp_nfa(lf).contents
                sp, sn = C.c_void_p(), C.c_int64(0)
                lit = None
                if lib().femto_amd_regexp_literal(lf, C.byref(sp), C.byref(sn)):
                    lit = (np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint16)), shape=(sn.value,)).copy() if sn.value
                           else np.zeros(0, dtype=np.uint16))
                node.update(literal=lit, settings=(v.cost_bound, v.subst_cost, v.delete_cost, v.insert_cost),
                            echo=lib().femto_amd_regexp_echo(lf))
            self.nodes.append(node)

    def free(self):
        if self._h:
            lib().femto_amd_bquery_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def regexp_match(regex, s):
    """test hook: the automaton built from `regex` accepts exactly the byte string s (None: syntax error)"""
    rx = np.frombuffer(bytes(regex) + b"\0", dtype=np.uint8)
    sb = np.frombuffer(bytes(s) + b"\0", dtype=np.uint8)
    r = lib().femto_amd_regexp_match(_ptr(rx), len(regex), _ptr(sb), len(s))
    return None if r < 0 else bool(r)


def query_echo(query, streamline=True, usequotes=False, simplify=False, icase=False, dump=False):
    """test hook: the query parsed, then streamline_query / simplify_query / icase_ast as asked (femto_search's order), printed
    back as ast_to_string prints it (None: syntax error); dump=True: the PARSED tree in the form oracle/ref_tool.c `ast` reads"""
    q = np.frombuffer(bytes(query) + b"\0", dtype=np.uint8)
    buf = C.create_string_buffer(64 * len(query) + 4096)
    flags = (1 if streamline else 0) | (2 if simplify else 0) | (4 if icase else 0)
    r = lib().femto_amd_query_echo(_ptr(q), len(query), flags, 2 if dump else int(usequotes), buf, len(buf))
    return None if r < 0 else buf.raw[:r]


def bseq_encode(raw_bytes, bitlen, force_type=0):
    """bseq_construct_forcetype-compatible encoding of a bit string (MSB-first bytes)."""
    raw = np.frombuffer(bytes(raw_bytes) + b"\0", dtype=np.uint8)
    n = C.c_int64(0)
    _check(lib().femto_amd_bseq_encode(_ptr(raw), bitlen, force_type, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint8)
    _check(lib().femto_amd_bseq_encode(_ptr(raw), bitlen, force_type, _ptr(out), n.value, C.byref(n)))
    return out


def _doc_args(docs, infos):
    docs = [np.ascontiguousarray(np.frombuffer(bytes(d), dtype=np.uint8) if not isinstance(d, np.ndarray) else d,
                                 dtype=np.uint8) for d in docs]
    n = len(docs)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data if len(d) else None for d in docs])
    lens = np.array([len(d) for d in docs], dtype=np.int64)
    infos = infos or [""] * n
    iarr = (C.c_char_p * n)(*[i.encode() if isinstance(i, str) else bytes(i) for i in infos])
    return docs, n, ptrs, lens, iarr


def build_index(out_dir, docs, params=None, infos=None, device=0):
    """GPU suffix sort + femto block-file writer (femto_amd_build_index)."""
    keep, n, ptrs, lens, iarr = _doc_args(docs, infos)
    _check(lib().femto_amd_build_index(os.fsencode(out_dir), n, ptrs, _ptr(lens), iarr,
                                       params.encode() if params else None, device))


def build_index_from_sa(out_dir, docs, sa, params=None, infos=None):
    """femto block-file writer from a caller-supplied suffix array of the prepared text."""
    keep, n, ptrs, lens, iarr = _doc_args(docs, infos)
    sa = np.ascontiguousarray(sa, dtype=np.int64)
    _check(lib().femto_amd_build_index_from_sa(os.fsencode(out_dir), n, ptrs, _ptr(lens), iarr,
                                               params.encode() if params else None, _ptr(sa)))


def flatten_index(index_dir, out_path):
    """flatten_index (src/main/index.c:2260): directory index -> single flattened file."""
    _check(lib().femto_amd_flatten_index(os.fsencode(index_dir), os.fsencode(out_path)))
