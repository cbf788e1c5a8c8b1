"""ctypes loader of the product library liblva_hip.so (C ABI: include/lva_decoder.h)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "liblva_hip.so"

MAX_DEVIATION_DEFAULT = 0xFFFFFFFF
ABI_VERSION = 5                # LVA_ABI_VERSION of include/lva_decoder.h
ERR_POST_TOO_SHORT = -6
ERR_BUSY = -13

ERRORS = {
    -1: "LVA_ERR_MEM_CONV", -2: "LVA_ERR_RATE", -3: "LVA_ERR_MSG_LEN", -4: "LVA_ERR_SYNC",
    -5: "LVA_ERR_TOO_MANY_STATES", -6: "LVA_ERR_POST_TOO_SHORT", -7: "LVA_ERR_MSG_TOO_LONG",
    -8: "LVA_ERR_NOMEM", -9: "LVA_ERR_HIP", -10: "LVA_ERR_ARG", -11: "LVA_ERR_NO_DEVICE",
    -12: "LVA_ERR_UNSUPPORTED", -13: "LVA_ERR_BUSY",
}

class LvaError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        name = ERRORS.get(code, "LVA_ERR_%d" % code)
        msg = name
        try:
            msg += ": " + load_library().lva_strerror(code).decode()
        except Exception:  # pragma: no cover
            pass
        if detail:
            msg += " (" + detail + ")"
        super().__init__(msg)


class Config(ctypes.Structure):
    _fields_ = [("mem_conv", ctypes.c_int32), ("rate", ctypes.c_int32), ("msg_len", ctypes.c_uint32),
                ("list_size", ctypes.c_uint32), ("max_deviation", ctypes.c_uint32),
                ("sync_marker", ctypes.c_char_p), ("sync_period", ctypes.c_uint32),
                ("device", ctypes.c_int32), ("max_slots", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("mem_budget_bytes", ctypes.c_uint64)]


class CodeInfoStruct(ctypes.Structure):
    _fields_ = [("nstate_pos", ctypes.c_uint32), ("nstate_conv", ctypes.c_uint32), ("oligo_len", ctypes.c_uint32),
                ("msg_words", ctypes.c_uint32), ("initial_state", ctypes.c_uint32), ("final_state", ctypes.c_uint32),
                ("g0", ctypes.c_uint32), ("g1", ctypes.c_uint32), ("pattern_len", ctypes.c_int32),
                ("pattern", ctypes.c_uint8 * 16)]


class Profile(ctypes.Structure):
    _fields_ = [("step_kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("step_launches", ctypes.c_uint64), ("read_steps", ctypes.c_uint64),
                ("algorithmic_bytes", ctypes.c_double), ("fixup_states", ctypes.c_uint64),
                ("fixup_reason", ctypes.c_uint64 * 4),
                ("slots", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("dominant_kernel_ms", ctypes.c_double), ("step_pair_ms", ctypes.c_double),
                ("timed_launches", ctypes.c_uint64), ("h2d_ms", ctypes.c_double), ("h2d_bytes", ctypes.c_uint64),
                ("overflow_steps", ctypes.c_uint64), ("working_bytes", ctypes.c_double)]


class KernelPlanInfo(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("dominant", ctypes.c_int32), ("fixup", ctypes.c_int32),
                ("lazy", ctypes.c_uint32), ("rec", ctypes.c_uint32), ("cmp", ctypes.c_uint32),
                ("ring_positions", ctypes.c_uint32), ("instance", ctypes.c_int32)]


class PayloadPos(ctypes.Structure):
    _fields_ = [("start_pos", ctypes.c_int32), ("end_pos", ctypes.c_int32), ("dist_start", ctypes.c_int32),
                ("dist_end", ctypes.c_int32), ("rc", ctypes.c_int32), ("ok", ctypes.c_int32)]


class ExperimentBarcodes(ctypes.Structure):
    _fields_ = [("start_barcode", ctypes.c_char_p), ("end_barcode", ctypes.c_char_p), ("min_len", ctypes.c_uint32)]


class DemuxPos(ctypes.Structure):
    _fields_ = [("pos", PayloadPos), ("experiment", ctypes.c_int32), ("reason", ctypes.c_int32),
                ("runner_up", ctypes.c_int32), ("runner_up_dist", ctypes.c_int32)]


class ListStat(ctypes.Structure):
    _fields_ = [("top_correct", ctypes.c_int32), ("list_correct", ctypes.c_int32), ("hamming", ctypes.c_int32),
                ("hamming8", ctypes.c_int32), ("hamming16", ctypes.c_int32), ("edit", ctypes.c_int32)]


_int, _vp, _cp = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
_i32, _u32, _u64, _u16 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint16
_code = [_i32, _i32, _u32, _i32, _cp, _u32]          # mem_conv, rate, msg_len, rc, sync_marker, sync_period
_decode_out = [_vp, _vp, _vp, _vp]                   # rc_flags, out_msgs, out_scores, out_counts
_demux = [_vp, _i32, _i32, _i32, _vp, _vp]           # exps, n_exps, max_dist, min_margin, out, all_out
_f32 = ctypes.c_float
# d, seed, first_read, n_reads, sub / del / ins thresholds, dwell_cdf, dwell_k, barcodes, flank_lo, flank_hi, rc_mode
_sim = [_vp, _u64, _u32, _i32, _u32, _u32, _u32, _vp, _i32, _cp, _cp, _u32, _u32, _i32]
_pool = [_vp, _i32, _vp]         # pool, n_pool, pool_cdf

# The C ABI, once: every function include/lva_decoder.h declares -> (restype, argtypes), in the header's order
# (tests/test_abi_table_host.py parses the header and holds this table and the structures above to it)
ABI = {
    "lva_version": (_cp, []),
    "lva_abi_version": (_int, []),
    "lva_strerror": (_cp, [_int]),
    "lva_last_hip_error": (_cp, []),
    "lva_code_describe": (_int, _code + [ctypes.POINTER(CodeInfoStruct)]),
    "lva_code_tables": (_int, _code + [_vp, _vp, _vp, _vp, _vp]),
    "lva_code_fingerprint": (_int, _code + [_vp, _u32, _vp]),
    "lva_band_table": (_int, _code + [_u32, _u32, _vp, _vp]),
    "lva_encode": (_int, [_i32, _i32, _u32, _vp, _i32, _vp]),
    "lva_algorithmic_bytes": (_int, _code + [_u32, _u32, _u32, ctypes.POINTER(ctypes.c_double)]),
    "lva_kernel_plan": (_int, [ctypes.POINTER(Config), ctypes.POINTER(KernelPlanInfo)]),
    "lva_decoder_create": (_int, [ctypes.POINTER(Config), ctypes.POINTER(_vp)]),
    "lva_decoder_destroy": (None, [_vp]),
    "lva_decode_batch": (_int, [_vp, _vp, _vp, _i32] + _decode_out),
    "lva_decode_batch_device": (_int, [_vp, _vp, _vp, _i32] + _decode_out),
    "lva_decode_windows_device": (_int, [_vp, _vp, _vp, _vp, _i32] + _decode_out),
    "lva_decoder_profile": (_int, [_vp, ctypes.POINTER(Profile)]),
    "lva_decoder_set_launch_events": (_int, [_vp, _i32]),
    "lva_stream_open": (_int, [_vp, _i32, ctypes.POINTER(_vp)]),
    "lva_stream_close": (_int, [_vp]),
    "lva_stream_submit": (_int, [_vp, _vp, ctypes.c_int64, _i32, _u64]),
    "lva_stream_poll": (_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32)]),
    "lva_stream_pending": (_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "lva_device_alloc": (_int, [_vp, _u64, ctypes.POINTER(_vp)]),
    "lva_device_free": (_int, [_vp, _vp]),
    "lva_device_upload": (_int, [_vp, _vp, _vp, _u64]),
    "lva_device_synchronize": (_int, [_vp]),
    "lva_device_download": (_int, [_vp, _vp, _vp, _u64]),
    "lva_transpost_batch": (_int, [_vp, _vp, _vp, _i32, _vp]),
    "lva_transpost_batch_device": (_int, [_vp, _vp, _vp, _i32, _vp]),
    "lva_basecall_batch": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "lva_basecall_batch_device": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "lva_find_barcode_batch": (_int, [_vp, _vp, _vp, _vp, _i32, _cp, _cp, _vp]),
    "lva_locate_payload_batch": (_int, [_vp, _vp, _vp, _i32, _cp, _cp, _u32, _vp]),
    "lva_locate_payload_batch_device": (_int, [_vp, _vp, _vp, _i32, _cp, _cp, _u32, _vp]),
    "lva_demux_batch": (_int, [_vp, _vp, _vp, _i32] + _demux),
    "lva_demux_batch_device": (_int, [_vp, _vp, _vp, _i32] + _demux),
    "lva_demux_bases_batch": (_int, [_vp, _vp, _vp, _vp, _i32] + _demux),
    "lva_rs_decode": (_int, [_i32, _vp, _i32, _i32, _i32, _vp, _i32, _u16, _u16, _vp, _vp]),
    "lva_rs_encode": (_int, [_i32, _vp, _i32, _i32, _i32, _u16, _vp]),
    "lva_rs_last_error": (_cp, []),
    "lva_list_filter": (_int, [_i32, _vp, _vp, _i32, _i32, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lva_list_consensus": (_int, [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lva_list_stats": (_int, [_i32, _vp, _vp, _vp, _i32, _i32, _u32, _vp]),
    "lva_rs_trials": (_int, [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, ctypes.c_int64, _vp, _i32, _u64, _u32, _i32, _i32, _vp, _vp, _vp]),
    "lva_simulate_plan": (_int, _sim + [_vp, _vp]),
    "lva_simulate_fill_device": (_int, _sim + [_f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lva_simulate_pool_plan": (_int, _sim + _pool + [_vp, _vp]),
    "lva_simulate_pool_fill_device": (_int, _sim + _pool + [_f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lva_align_profile": (_int, [_i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "lva_score_bases_device": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _vp]),
    "lva_score_bases": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _vp]),
    "lva_forward_bases_device": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _vp]),
    "lva_forward_bases": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _vp]),
    "lva_trace_bases_device": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _i32, _u64, _i32, _vp, _vp, _vp, _vp]),
    "lva_trace_bases": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _u32, _i32, _u64, _i32, _vp, _vp, _vp, _vp]),
    "lva_map_index_create_device": (_int, [_i32, _vp, _vp, _i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "lva_map_index_tables": (_int, [_vp, _vp, _vp, _vp]),
    "lva_map_index_create_pooled": (_int, [_vp, _vp, _i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "lva_map_reads_pooled": (_int, [_i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "lva_map_index_create": (_int, [_vp, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "lva_map_index_destroy": (None, [_vp]),
    "lva_map_index_info": (_int, [_vp, _vp, _vp, _vp]),
    "lva_map_reads": (_int, [_i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
}
EXPORTS = list(ABI)

_lib = None


def build_id():
    """The source hash the loaded library was built from (lva_version(): '... build <id>')."""
    return load_library().lva_version().decode().rsplit("build ", 1)[-1]


def library_path():
    # LVA_LIB_PATH: point at another build of the same library (kernel experiments)
    return os.environ.get("LVA_LIB_PATH") or os.path.join(_HERE, _LIB_NAME)


def load_library():
    """Load liblva_hip.so.  Raises if it has not been built: the product has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C nanopore_dna_storage_amd/csrc`" % path)
    L = ctypes.CDLL(path)
    if not hasattr(L, "lva_abi_version"):            # a library built before the ABI carried a version (round 4 and earlier)
        raise ImportError("%s has no lva_abi_version (ABI version < 5), this package was written for %d: rebuild it" % (path, ABI_VERSION))
    L.lva_abi_version.restype = ctypes.c_int
    if L.lva_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this package was written for %d (struct layouts of include/lva_decoder.h): rebuild it"
                          % (path, L.lva_abi_version(), ABI_VERSION))
    for name, (restype, argtypes) in ABI.items():    # entry points were added without a new ABI version: an older build lacks some
        if not hasattr(L, name):
            raise ImportError("%s has no %s: rebuild it" % (path, name))
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(status, detail="lva_last_hip_error"):
    """The one place a non-zero status of the library becomes an LvaError.  detail: the entry point that holds the text of
    what went wrong (lva_rs_last_error for the outer code), None for the host-only calls that leave none."""
    if status != 0:
        raise LvaError(status, getattr(load_library(), detail)().decode() if detail else "")
