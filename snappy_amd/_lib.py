"""ctypes binding of libsnaphash.so (include/snaphash.h).

The library is the product: HIP kernels for gfx950 behind a C ABI.  There is
no Python or CPU fallback -- if the shared object is missing this module
raises at import of the symbol table, and if no MI355X is visible
``Context()`` raises ``SnaphashError(EDEVICE)``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SNAPHASH_LIB: developer override to A/B another build of the same ABI (tools/ab_bench.sh)
LIB_PATH = os.environ.get("SNAPHASH_LIB") or os.path.join(_HERE, "libsnaphash.so")

OK, EINVAL, ENOMEM, EIO, EDEVICE, EMODE, ENAME, EPARSE, EMISMATCH = 0, -1, -2, -3, -4, -5, -6, -7, -8
EFORMAT, ECONTENT = -9, -10
KERNEL_AUTO, KERNEL_WIDE, KERNEL_SPLIT, KERNEL_PAIR, KERNEL_QUAD = 0, 1, 2, 3, 4
KERNEL_NAMES = {KERNEL_WIDE: "sha512_wide_kernel", KERNEL_SPLIT: "sha512_split_kernel<false>",
                KERNEL_PAIR: "sha512_split_kernel<true>", KERNEL_QUAD: "sha512_quad_kernel"}

# every symbol include/snaphash.h declares
EXPORTS = [
    "snaphash_init", "snaphash_destroy", "snaphash_abi_version",
    "snaphash_sha512_files", "snaphash_sha512_buffers", "snaphash_sha512_device", "snaphash_sync",
    "snaphash_tree", "snaphash_write_hashes", "snaphash_verify", "snaphash_free",
    "snaphash_files_equal", "snaphash_ranges_equal_device", "snaphash_dir_updated",
    "snaphash_walk", "snaphash_records_count", "snaphash_records_get", "snaphash_records_free",
    "snaphash_emit_yaml", "snaphash_parse_yaml", "snaphash_records_sha512_hex", "snaphash_mode_string", "snaphash_mode_parse", "snaphash_lpt_assign",
    "snaphash_fill_synthetic_device", "snaphash_strerror", "snaphash_last_error", "snaphash_get_stats",
    "snaphash_get_stats_ex", "snaphash_get_device_stats", "snaphash_tree_ex",
    "snaphash_batch_begin", "snaphash_batch_append", "snaphash_batch_end", "snaphash_batch_finish", "snaphash_batch_abort",
    "snaphash_tar_create", "snaphash_tar_create_fn", "snaphash_gzip_buffer", "snaphash_get_targz_stats",
    "snaphash_xz_buffer", "snaphash_xz_buffer_check", "snaphash_tar_create_xz",
    "snaphash_get_engine_info", "snaphash_numa_probe",
    "snaphash_get_engine_cpus", "snaphash_numa_slice", "snaphash_plan_streams", "snaphash_usable_cpus", "snaphash_cgroup_cpu_quota",
    "snaphash_shard_plan", "snaphash_shard_rows", "snaphash_shard_count", "snaphash_shard_streams", "snaphash_shard_bytes",
    "snaphash_shard_path", "snaphash_shard_hash", "snaphash_shard_emit", "snaphash_shard_free",
    # ABI 5
    "snaphash_shard_set_local_ranks", "snaphash_shard_fingerprint", "snaphash_get_plan_model", "snaphash_calib_observe_call",
    "snaphash_shard_list", "snaphash_shard_plan_from",
    "snaphash_calib_observe", "snaphash_calib_apply", "snaphash_get_calib",
    # the install side (row f5)
    "snaphash_gunzip_buffer", "snaphash_tar_unpack", "snaphash_get_unpack_stats", "snaphash_get_block_scan_stats",
    # data.tar.bz2
    "snaphash_bunzip2_buffer", "snaphash_tar_unpack_bz2",
    # data.tar.xz
    "snaphash_unxz_buffer", "snaphash_tar_unpack_xz", "snaphash_unxz_block_device", "snaphash_crc64_device",
    "snaphash_sha256_device", "snaphash_get_xz_check_stats",
    # the .snap itself: CRCs in HBM, the ar container, audit and unpack
    "snaphash_crc32_device", "snaphash_snap_open", "snaphash_snap_close", "snaphash_snap_members", "snaphash_snap_member_info",
    "snaphash_snap_control_member", "snaphash_snap_meta_member", "snaphash_snap_unpack", "snaphash_snap_audit",
    "snaphash_snap_get_stats",
    # the compressor's code construction alone
    "snaphash_deflate_codes_device",
    # the .xz encoder's kernels alone
    "snaphash_xzenc_stages_device",
    "snaphash_xzenc_stages_device_ex",
    # a SHA-512 kernel alone, over a caller's job table
    "snaphash_sha512_jobs_device",
    # the data.tar.bz2 producer, its BWT stage alone, and its stages on a caller's arrays
    "snaphash_bzip2_buffer", "snaphash_tar_create_bz2", "snaphash_bwt_device", "snaphash_bzenc_stages_device",
    # writing the .snap (ClickDeb.Build), and its self-check kernel alone
    "snaphash_snap_build", "snaphash_deflate_check_device",
    # the .xz producer with options and its self-check, and that check's kernel alone
    "snaphash_xz_buffer_ex", "snaphash_tar_create_xz_ex", "snaphash_get_xz_selfcheck_stats", "snaphash_lzma2_check_device",
    # .xz with a BCJ filter in front of LZMA2, both sides, and the filter kernels alone
    "snaphash_unxz_buffer_ex", "snaphash_tar_unpack_xz_ex", "snaphash_bcj_device", "snaphash_get_xz_filter_stats",
    # the .bz2 producer with options and its self-check, and that check's kernels alone
    "snaphash_bzip2_buffer_ex", "snaphash_tar_create_bz2_ex", "snaphash_get_bz2_selfcheck_stats", "snaphash_bz2_check_device",
    # the .snap session with ".xz" members routed to the .xz engine
    "snaphash_snap_open_ex",
    # every filter liblzma takes in front of LZMA2, the kernels alone
    "snaphash_xz_filter_device",
]
BUILD_NO_HASHES, BUILD_CHECK = 1, 2
SNAP_XZ = 1
DATA_CODECS = {"gz": 0, "bz2": 1, "xz": 2}  # snaphash_snap_build_options.data_codec
XZ_CHECK_NAMES = {"none": 0, "crc32": 1, "crc64": 4, "sha256": 10}
XZ_SELF_CHECK = 1
UNXZ_BCJ = 1
UNXZ_CHAINS = 4  # (2 is not a flag)
SNAP_XZ_CHAINS = 4
BCJ_X86, BCJ_ARM, BCJ_ARMTHUMB = 4, 7, 8  # the .xz format's filter ids
BCJ_NAMES = {"x86": BCJ_X86, "arm": BCJ_ARM, "armthumb": BCJ_ARMTHUMB}
XZ_FILTER_NAMES = dict(BCJ_NAMES, delta=3, powerpc=5, ia64=6, sparc=9)  # what snaphash_xz_filter_device takes


def bcj_filter(f):
    """A filter as the entry points take it: None / 0, an id (4, 7, 8) or a name ("x86", "arm", "armthumb")."""
    if not f:
        return 0
    return BCJ_NAMES[f] if isinstance(f, str) else int(f)

BZ2_SELF_CHECK = 1
JOB_FIRST, JOB_FINAL = 1, 2
CRC_GZIP, CRC_BZIP2 = 0, 1
FLAG_CHECK_GATHER, FLAG_NO_RCCL, FLAG_FORCE_GATHER, FLAG_GPU_ONLY, FLAG_NO_NUMA, FLAG_KEEP_RLIMIT = 1, 2, 4, 8, 16, 32
FLAG_SPLIT_BLOCKS = 64  # gunzip_buffer / tar_unpack: cut streams without flush points at their DEFLATE blocks too


class Config(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("staging_bytes", ctypes.c_uint64),
                ("kernel", ctypes.c_uint32), ("deflate_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p),
                # ABI 2
                ("devices", ctypes.POINTER(ctypes.c_int32)), ("n_devices", ctypes.c_uint32),
                ("host_threads", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved2", ctypes.c_uint32)]


class StatsEx(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_devices", ctypes.c_uint32), ("gather_kind", ctypes.c_uint32),
                ("gather_checked", ctypes.c_uint32), ("gather_ms", ctypes.c_double), ("gpu_bytes", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("host_streams", ctypes.c_uint64), ("reserved3", ctypes.c_uint64),
                ("host_ms", ctypes.c_double),
                # ABI 5: the plan's prediction beside what the call took
                ("planned_gpu_ms", ctypes.c_double), ("planned_host_ms", ctypes.c_double), ("planned_threads", ctypes.c_uint32),
                ("host_threads_run", ctypes.c_uint32), ("gpu_ms", ctypes.c_double), ("hash_ms", ctypes.c_double),
                ("plan_ms", ctypes.c_double)]


class EngineInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("numa_node", ctypes.c_int32),
                ("staging_node", ctypes.c_int32), ("fill_threads", ctypes.c_uint32), ("n_cpus", ctypes.c_uint32),
                ("pci_bus_id", ctypes.c_char * 32), ("pinned_bytes", ctypes.c_uint64), ("hbm_bytes", ctypes.c_uint64)]


class PlanModel(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_devices", ctypes.c_uint32), ("cpus", ctypes.c_uint32),
                ("fill_threads", ctypes.c_uint32), ("host_threads", ctypes.c_uint32), ("from_files", ctypes.c_uint32),
                ("host_rate", ctypes.c_double), ("gpu_stream_rate", ctypes.c_double), ("gpu_link", ctypes.c_double),
                ("gpu_latency", ctypes.c_double),
                ("gpu_seconds", ctypes.c_double), ("host_seconds", ctypes.c_double), ("host_streams", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("host_threads_used", ctypes.c_uint32), ("host_lane_gain_pct", ctypes.c_uint32),
                ("fill_rate", ctypes.c_double), ("fill_per_file", ctypes.c_double)]  # ABI 5


class PlanCalib(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_dma", ctypes.c_uint32), ("n_fill_mem", ctypes.c_uint32),
                ("n_fill_files", ctypes.c_uint32), ("dma", ctypes.c_double), ("fill_mem", ctypes.c_double),
                ("fill_files", ctypes.c_double), ("host_gain", ctypes.c_double), ("n_host", ctypes.c_uint32), ("n_fill_per_file", ctypes.c_uint32),
                ("fill_per_file", ctypes.c_double)]


class Stats(ctypes.Structure):
    _fields_ = [("bytes_hashed", ctypes.c_uint64), ("blocks", ctypes.c_uint64), ("streams", ctypes.c_uint64),
                ("launches", ctypes.c_uint32), ("kernel_used", ctypes.c_uint32), ("kernel_ms", ctypes.c_double),
                ("h2d_ms", ctypes.c_double), ("wall_ms", ctypes.c_double)]


class TargzStats(ctypes.Structure):
    _fields_ = [("tar_bytes", ctypes.c_uint64), ("gz_bytes", ctypes.c_uint64), ("members", ctypes.c_uint64),
                ("chunks", ctypes.c_uint64), ("stored_chunks", ctypes.c_uint64), ("deflate_ms", ctypes.c_double),
                ("fill_ms", ctypes.c_double), ("wall_ms", ctypes.c_double)]


class Sha512Job(ctypes.Structure):
    _fields_ = [("data", ctypes.c_uint64), ("nbytes", ctypes.c_uint64), ("total_prev", ctypes.c_uint64), ("idx", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class XzCheckStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("device_crc32", ctypes.c_uint64),
                ("device_crc64", ctypes.c_uint64), ("device_sha256", ctypes.c_uint64), ("host_checks", ctypes.c_uint64),
                ("device_check_ms", ctypes.c_double)]


class XzOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("block_size", ctypes.c_uint64),
                ("check", ctypes.c_uint32), ("filter", ctypes.c_uint32), ("level", ctypes.c_uint32), ("reserved2", ctypes.c_uint32)]


class XzOptionsChain(XzOptions):
    """snaphash_xz_options with the fields behind its first 32 bytes: the filter chain (struct_size 48)."""
    _fields_ = [("chain_len", ctypes.c_uint32), ("chain", ctypes.c_uint32 * 3)]


def xz_chain_words(chain):
    """[("delta", 4), "x86", 9] -> snaphash_xz_options.chain's words, id | param << 8"""
    out = []
    for f in chain:
        f, param = f if isinstance(f, tuple) else (f, 0)
        fid = XZ_FILTER_NAMES.get(f, f) if isinstance(f, str) else f
        if not isinstance(fid, int):
            raise ValueError("unknown .xz filter %r" % (f,))
        out.append(fid | int(param) << 8)
    return out


def xz_options(flags, block_size, check, filter, level, chain=None):
    """snaphash_xz_options: the 32-byte struct, or with a chain the 48-byte one"""
    if not chain:
        return XzOptions(ctypes.sizeof(XzOptions), flags, block_size, check, filter, level)
    words = xz_chain_words(chain)
    o = XzOptionsChain(ctypes.sizeof(XzOptionsChain), flags, block_size, check, filter, level)
    o.chain_len = len(words)
    for k, w in enumerate(words[:3]):
        o.chain[k] = w
    return o


class UnxzOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class XzFilterStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("filter", ctypes.c_uint32), ("device_blocks", ctypes.c_uint64),
                ("host_blocks", ctypes.c_uint64), ("device_ms", ctypes.c_double)]


class XzSelfCheckStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("chunks", ctypes.c_uint64), ("ms", ctypes.c_double)]


class Bz2Options(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("level", ctypes.c_uint32)]


class Bz2SelfCheckStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("blocks", ctypes.c_uint64), ("ms", ctypes.c_double)]


class UnpackStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("gz_bytes", ctypes.c_uint64),
                ("tar_bytes", ctypes.c_uint64), ("members", ctypes.c_uint64), ("segments", ctypes.c_uint64),
                ("gpu_segments", ctypes.c_uint64), ("host_bytes", ctypes.c_uint64), ("inflate_ms", ctypes.c_double),
                ("wall_ms", ctypes.c_double)]


class BlockScanStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("bits_scanned", ctypes.c_uint64),
                ("candidates", ctypes.c_uint64), ("linked", ctypes.c_uint64), ("unreached", ctypes.c_uint64),
                ("host_blocks", ctypes.c_uint64), ("scan_ms", ctypes.c_double)]


class SnapStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("data_decodes", ctypes.c_uint64),
                ("control_decodes", ctypes.c_uint64), ("device_crc_ranges", ctypes.c_uint64), ("host_crc_ranges", ctypes.c_uint64),
                ("device_crc_ms", ctypes.c_double)]


class SnapOpenOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class SnapBuildOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("mtime", ctypes.c_int64),
                ("data_codec", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("xz", ctypes.POINTER(XzOptions)),
                ("bz2", ctypes.POINTER(Bz2Options))]


class SnapBuildStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("snap_bytes", ctypes.c_uint64),
                ("data_bytes", ctypes.c_uint64), ("control_bytes", ctypes.c_uint64), ("tar_bytes", ctypes.c_uint64),
                ("members", ctypes.c_uint64), ("check_chunks", ctypes.c_uint64), ("check_ms", ctypes.c_double),
                ("data_ms", ctypes.c_double), ("control_ms", ctypes.c_double), ("ar_ms", ctypes.c_double), ("wall_ms", ctypes.c_double)]


class Mismatch(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("name", ctypes.c_char * 4096)]


class Record(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("st_mode", ctypes.c_uint32), ("is_regular", ctypes.c_int32),
                ("size", ctypes.c_int64), ("path", ctypes.c_char_p)]


class SnaphashError(Exception):
    def __init__(self, code, message=""):
        self.code = code
        super().__init__("snaphash error %d (%s)%s" % (code, strerror(code), (": " + message) if message else ""))


_lib = None


def lib():
    """Load libsnaphash.so; raises OSError loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: build it with `make -C snappy_amd/csrc` (or __graft_entry__.build())" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64, and a second runtime
    # loaded before it ends up without a device ("no ROCm-capable device is detected").  In the
    # Python mirror torch is always around (device memory, streams, torch.distributed), so load
    # it first and let libsnaphash.so bind to the runtime that is already in the process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    L.snaphash_init.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
    L.snaphash_destroy.argtypes = [vp]
    L.snaphash_destroy.restype = None
    L.snaphash_abi_version.argtypes = []
    L.snaphash_sha512_files.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), sz, vp, ctypes.POINTER(ctypes.c_int32)]
    L.snaphash_sha512_buffers.argtypes = [vp, ctypes.POINTER(vp), u64p, sz, vp]
    L.snaphash_sha512_device.argtypes = [vp, vp, vp, vp, sz, vp]
    L.snaphash_sync.argtypes = [vp]
    L.snaphash_tree.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_write_hashes.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    L.snaphash_verify.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.POINTER(Mismatch)]
    L.snaphash_files_equal.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), sz, vp]
    L.snaphash_ranges_equal_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
    L.snaphash_dir_updated.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp),
                                       ctypes.POINTER(sz)]
    L.snaphash_free.argtypes = [vp]
    L.snaphash_free.restype = None
    L.snaphash_walk.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.snaphash_records_count.argtypes = [vp]
    L.snaphash_records_count.restype = sz
    L.snaphash_records_get.argtypes = [vp, sz, ctypes.POINTER(Record)]
    L.snaphash_records_free.argtypes = [vp]
    L.snaphash_records_free.restype = None
    L.snaphash_emit_yaml.argtypes = [vp, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_parse_yaml.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(vp), ctypes.c_char_p]
    L.snaphash_records_sha512_hex.argtypes = [vp, sz]
    L.snaphash_records_sha512_hex.restype = ctypes.c_char_p
    L.snaphash_mode_string.argtypes = [ctypes.c_uint32, ctypes.c_char_p]
    L.snaphash_mode_parse.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    L.snaphash_lpt_assign.argtypes = [vp, sz, ctypes.c_int, vp]
    L.snaphash_fill_synthetic_device.argtypes = [vp, vp, vp, vp, vp, sz]
    L.snaphash_strerror.argtypes = [ctypes.c_int]
    L.snaphash_strerror.restype = ctypes.c_char_p
    L.snaphash_last_error.argtypes = [vp]
    L.snaphash_last_error.restype = ctypes.c_char_p
    L.snaphash_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.snaphash_get_stats.restype = None
    L.snaphash_get_stats_ex.argtypes = [vp, ctypes.POINTER(StatsEx)]
    L.snaphash_get_device_stats.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(Stats)]
    L.snaphash_tree_ex.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                   ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_batch_begin.argtypes = [vp, sz, ctypes.POINTER(vp)]
    L.snaphash_batch_append.argtypes = [vp, sz, vp, sz]
    L.snaphash_batch_end.argtypes = [vp, sz]
    L.snaphash_batch_finish.argtypes = [vp, vp]
    L.snaphash_batch_abort.argtypes = [vp]
    L.snaphash_batch_abort.restype = None
    L.snaphash_tar_create.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp),
                                      ctypes.POINTER(sz), ctypes.c_char_p]
    L.snaphash_gzip_buffer.argtypes = [vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_xz_buffer.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_create_xz.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp),
                                         ctypes.POINTER(sz), ctypes.c_char_p]
    L.snaphash_bzip2_buffer.argtypes = [vp, vp, sz, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_create_bz2.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp),
                                          ctypes.POINTER(sz), ctypes.c_char_p]
    L.snaphash_bwt_device.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    L.snaphash_bzenc_stages_device.argtypes = [vp, vp, vp, vp, sz] + [ctypes.c_uint32] * 4 + [vp] * 12 + [sz, u64p]
    L.snaphash_get_targz_stats.argtypes = [vp, ctypes.POINTER(TargzStats)]
    L.snaphash_deflate_codes_device.argtypes = [vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    L.snaphash_get_targz_stats.restype = None
    L.snaphash_gunzip_buffer.argtypes = [vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_unpack.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_get_unpack_stats.argtypes = [vp, ctypes.POINTER(UnpackStats)]
    L.snaphash_get_block_scan_stats.argtypes = [vp, ctypes.POINTER(BlockScanStats)]
    L.snaphash_bunzip2_buffer.argtypes = [vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_unpack_bz2.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_crc32_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, sz, vp]
    L.snaphash_unxz_buffer.argtypes = [vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_unpack_xz.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_crc64_device.argtypes = [vp, vp, vp, vp, sz, vp]
    L.snaphash_sha256_device.argtypes = [vp, vp, vp, vp, sz, vp]
    L.snaphash_get_xz_check_stats.argtypes = [vp, ctypes.POINTER(XzCheckStats)]
    L.snaphash_xz_buffer_check.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_unxz_block_device.argtypes = [vp, vp, sz, sz, vp, sz]
    L.snaphash_xzenc_stages_device.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, sz, u64p]
    L.snaphash_sha512_jobs_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(Sha512Job), sz, sz, vp, vp]
    L.snaphash_snap_open.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.snaphash_snap_open_ex.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(SnapOpenOptions), ctypes.POINTER(vp)]
    L.snaphash_snap_close.argtypes = [vp]
    L.snaphash_snap_close.restype = None
    L.snaphash_snap_members.argtypes = [vp]
    L.snaphash_snap_members.restype = sz
    L.snaphash_snap_member_info.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_char_p), u64p, u64p]
    L.snaphash_snap_control_member.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_snap_meta_member.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_snap_unpack.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_snap_audit.argtypes = [vp, ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_snap_get_stats.argtypes = [vp, ctypes.POINTER(SnapStats)]
    L.snaphash_snap_build.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(SnapBuildOptions), ctypes.c_char_p, ctypes.c_char_p,
                                      ctypes.POINTER(SnapBuildStats)]
    L.snaphash_deflate_check_device.argtypes = [vp, vp, sz, vp, u64p, sz, ctypes.c_int, vp]
    L.snaphash_xzenc_stages_device_ex.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, sz, u64p, ctypes.c_uint32]
    L.snaphash_xz_buffer_ex.argtypes = [vp, vp, sz, ctypes.POINTER(XzOptions), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_create_xz_ex.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(XzOptions), ctypes.POINTER(vp),
                                            ctypes.POINTER(sz), ctypes.c_char_p]
    L.snaphash_get_xz_selfcheck_stats.argtypes = [vp, ctypes.POINTER(XzSelfCheckStats)]
    L.snaphash_unxz_buffer_ex.argtypes = [vp, vp, sz, ctypes.POINTER(UnxzOptions), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_unpack_xz_ex.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.POINTER(UnxzOptions),
                                            ctypes.POINTER(Mismatch), ctypes.c_char_p]
    L.snaphash_bcj_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, vp, vp, vp, sz, ctypes.c_uint32]
    L.snaphash_xz_filter_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, vp, vp, vp, sz, ctypes.c_uint32]
    L.snaphash_get_xz_filter_stats.argtypes = [vp, ctypes.POINTER(XzFilterStats)]
    L.snaphash_lzma2_check_device.argtypes = [vp, vp, sz, ctypes.c_uint64, vp, sz, u64p, u64p, sz, ctypes.c_uint32, vp]
    L.snaphash_bzip2_buffer_ex.argtypes = [vp, vp, sz, ctypes.POINTER(Bz2Options), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_tar_create_bz2_ex.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(Bz2Options), ctypes.POINTER(vp),
                                             ctypes.POINTER(sz), ctypes.c_char_p]
    L.snaphash_get_bz2_selfcheck_stats.argtypes = [vp, ctypes.POINTER(Bz2SelfCheckStats)]
    L.snaphash_bz2_check_device.argtypes = [vp, vp, sz, u64p, u64p, vp, sz, u64p, u64p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, sz, vp]
    L.snaphash_get_engine_info.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(EngineInfo)]
    L.snaphash_numa_probe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), vp, sz, ctypes.POINTER(sz)]
    L.snaphash_shard_plan.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp)]
    for f in ("rows", "count", "streams"):
        getattr(L, "snaphash_shard_" + f).argtypes = [vp]
        getattr(L, "snaphash_shard_" + f).restype = sz
    L.snaphash_shard_bytes.argtypes = [vp]
    L.snaphash_shard_bytes.restype = ctypes.c_uint64
    L.snaphash_shard_path.argtypes = [vp, sz]
    L.snaphash_shard_path.restype = ctypes.c_char_p
    L.snaphash_shard_hash.argtypes = [vp, vp, vp]
    L.snaphash_shard_emit.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_shard_free.argtypes = [vp]
    L.snaphash_shard_free.restype = None
    L.snaphash_numa_slice.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, vp, sz, ctypes.POINTER(sz)]
    L.snaphash_get_engine_cpus.argtypes = [vp, ctypes.c_uint32, vp, sz, ctypes.POINTER(sz)]
    L.snaphash_plan_streams.argtypes = [u64p, sz, ctypes.POINTER(PlanModel), vp]
    L.snaphash_shard_list.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.snaphash_shard_plan_from.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                           ctypes.POINTER(vp)]
    L.snaphash_shard_set_local_ranks.argtypes = [vp, ctypes.c_uint32]
    L.snaphash_shard_fingerprint.argtypes = [vp]
    L.snaphash_shard_fingerprint.restype = ctypes.c_uint64
    L.snaphash_get_plan_model.argtypes = [vp, ctypes.c_int, ctypes.POINTER(PlanModel)]
    L.snaphash_calib_observe.argtypes = [ctypes.POINTER(PlanCalib), ctypes.c_int, ctypes.c_double, ctypes.c_double]
    L.snaphash_calib_observe_call.argtypes = [ctypes.POINTER(PlanCalib), ctypes.c_int] + [ctypes.c_double] * 5
    L.snaphash_calib_apply.argtypes = [ctypes.POINTER(PlanCalib), ctypes.POINTER(PlanModel)]
    L.snaphash_get_calib.argtypes = [vp, ctypes.POINTER(PlanCalib)]
    L.snaphash_usable_cpus.argtypes = []
    L.snaphash_usable_cpus.restype = ctypes.c_uint32
    L.snaphash_cgroup_cpu_quota.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.snaphash_cgroup_cpu_quota.restype = ctypes.c_uint32
    _lib = L
    return L


def plan_streams(lens, **model):
    """snaphash_plan_streams: what the planner decides for streams of these lengths (host-only, no device needed).
    Returns (on_host list of 0/1, dict of the model's outputs)."""
    n = len(lens)
    arr = (ctypes.c_uint64 * max(n, 1))(*[int(x) for x in lens])
    pm = PlanModel()
    pm.struct_size = ctypes.sizeof(PlanModel)
    for k, v in model.items():
        setattr(pm, k, v)
    flags = ctypes.create_string_buffer(max(n, 1))
    rc = lib().snaphash_plan_streams(arr, n, ctypes.byref(pm), flags)
    if rc:
        raise SnaphashError(rc)
    return list(flags.raw[:n]), {"gpu_seconds": pm.gpu_seconds, "host_seconds": pm.host_seconds, "host_streams": pm.host_streams,
                                 "host_bytes": pm.host_bytes, "host_threads": pm.host_threads_used}


def strerror(code):
    try:
        return lib().snaphash_strerror(code).decode()
    except OSError:
        return "?"


class Context:
    """One snaphash_ctx: one GPU (device=) or several (devices=[...], [-1] = all visible; the file list of a
    call is then LPT-sharded inside the library and the digests gathered over RCCL), one call in flight.
    host_threads: 0 = the library's default (a stream that would set the makespan of its batch all by itself -- the
    archive next to its tree -- is hashed on a host thread), N > 0 = N threads and the full planner;
    flags=FLAG_GPU_ONLY keeps every byte on the GPU (kernel parity tests, roofline runs)."""

    # flags a Context gets when the caller names none: 0 = the library's defaults.  The -m gpu suite sets it to
    # FLAG_GPU_ONLY (tests/conftest.py) so that every test exercises the HIP kernels unless it asks for the default.
    DEFAULT_FLAGS = 0

    def __init__(self, device=-1, staging_bytes=0, kernel=KERNEL_AUTO, stream=None, devices=None, host_threads=0, flags=None, deflate_depth=0):
        if flags is None:
            flags = Context.DEFAULT_FLAGS
        cfg = Config(ctypes.sizeof(Config), device, staging_bytes, kernel, deflate_depth, stream)
        if devices is not None:
            self._devs = (ctypes.c_int32 * len(devices))(*devices)
            cfg.devices = ctypes.cast(self._devs, ctypes.POINTER(ctypes.c_int32))
            cfg.n_devices = len(devices)
        cfg.host_threads = host_threads
        cfg.flags = flags
        h = ctypes.c_void_p()
        rc = lib().snaphash_init(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            raise SnaphashError(rc, "snaphash_init: " + lib().snaphash_last_error(None).decode(errors="replace"))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().snaphash_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise SnaphashError(rc, lib().snaphash_last_error(self._h).decode(errors="replace"))

    # ---- primitive -----------------------------------------------------------------
    def sha512_files(self, paths):
        """-> list of 64-byte digests; raises OSError(errno) for the first unreadable file."""
        n = len(paths)
        arr = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        out = ctypes.create_string_buffer(64 * max(n, 1))
        status = (ctypes.c_int32 * max(n, 1))()
        rc = lib().snaphash_sha512_files(self._h, arr, n, out, status)
        if rc == EIO:
            for i in range(n):
                if status[i]:
                    raise OSError(status[i], os.strerror(status[i]), os.fsdecode(paths[i]))
        self._check(rc)
        return [out.raw[64 * i:64 * i + 64] for i in range(n)]

    def sha512_buffers(self, bufs):
        n = len(bufs)
        keep = [bytes(b) if not isinstance(b, (bytes, bytearray)) else b for b in bufs]
        cbufs = [(ctypes.c_char * max(len(b), 1)).from_buffer_copy(b if len(b) else b"\0") for b in keep]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(c) for c in cbufs])
        lens = (ctypes.c_uint64 * max(n, 1))(*[len(b) for b in keep])
        out = ctypes.create_string_buffer(64 * max(n, 1))
        self._check(lib().snaphash_sha512_buffers(self._h, ptrs, lens, n, out))
        return [out.raw[64 * i:64 * i + 64] for i in range(n)]

    def sha512_device(self, d_base, offsets, lens, d_digests):
        """HBM-resident batch.  d_base / d_digests: device addresses (int);
        offsets / lens: contiguous numpy uint64 arrays.  Asynchronous: call sync()."""
        n = len(offsets)
        self._check(lib().snaphash_sha512_device(self._h, d_base, offsets.ctypes.data, lens.ctypes.data, n, d_digests))

    def sync(self):
        self._check(lib().snaphash_sync(self._h))

    def fill_synthetic_device(self, d_base, offsets, lens, file_index):
        self._check(lib().snaphash_fill_synthetic_device(self._h, d_base, offsets.ctypes.data, lens.ctypes.data,
                                                         file_index.ctypes.data, len(offsets)))

    # ---- pass ------------------------------------------------------------------------
    def tree(self, build_dir, data_tar):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().snaphash_tree(self._h, os.fsencode(build_dir), os.fsencode(data_tar), ctypes.byref(p),
                                        ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def write_hashes(self, build_dir, data_tar):
        self._check(lib().snaphash_write_hashes(self._h, os.fsencode(build_dir), os.fsencode(data_tar)))

    def tree_ex(self, build_dir, data_tar=None, archive_digest=None, write=False):
        """snaphash_tree_ex: the archive digest may be supplied by the caller (data_tar=None)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().snaphash_tree_ex(self._h, os.fsencode(build_dir), os.fsencode(data_tar) if data_tar else None,
                                           archive_digest, 1 if write else 0, ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def gzip_buffer(self, data):
        """One gzip member of `data`, DEFLATE on the GPU (row f3)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        buf = (ctypes.c_char * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        self._check(lib().snaphash_gzip_buffer(self._h, ctypes.addressof(buf), len(data), ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def xz_buffer(self, data, block_size=0, check=None, self_check=False, filter=None, level=0, chain=None):
        """One .xz Stream of `data`, a Block per `block_size` bytes (0: 1 MiB), LZMA2 on the GPU.  check: the Blocks'
        Check id -- 0 none, 1 CRC-32, 4 CRC-64, 10 SHA-256, each taken in HBM; None: CRC-64 through the entry point that
        takes no Check.  self_check: every LZMA2 chunk is walked against the bytes it was made from before it leaves HBM
        (snaphash_xz_buffer_ex with SNAPHASH_XZ_SELF_CHECK; xz_selfcheck_stats() tells what was walked); the bytes are
        the same.  filter: a BCJ filter in front of LZMA2 in every Block -- "x86", "arm", "armthumb" or the format's id
        (4, 7, 8), applied in HBM (snaphash_xz_buffer_ex; xz_filter_stats() tells what ran); None or 0: none.  level: 0 the
        greedy parse, 1 several candidates a position and a price-based parse (snaphash_xz_buffer_ex): a smaller file for
        more kernel time.  chain: up to three filters in front of LZMA2, the Block header's first filter first, e.g.
        [("delta", 4), "x86"] -- names or ids of "delta" (with its distance, 1 .. 256), "x86", "powerpc", "ia64", "arm",
        "armthumb", "sparc"; not together with filter.  unxz_buffer(chains=True) reads such a file back."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        buf = (ctypes.c_char * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        filter = bcj_filter(filter)
        if self_check or filter or level or chain:
            opt = xz_options(XZ_SELF_CHECK if self_check else 0, block_size, 4 if check is None else check, filter, level, chain)
            self._check(lib().snaphash_xz_buffer_ex(self._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n)))
        elif check is None:
            self._check(lib().snaphash_xz_buffer(self._h, ctypes.addressof(buf), len(data), block_size, ctypes.byref(p), ctypes.byref(n)))
        else:
            self._check(lib().snaphash_xz_buffer_check(self._h, ctypes.addressof(buf), len(data), block_size, check, ctypes.byref(p),
                                                       ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def bzip2_buffer(self, data, level=0, self_check=False, _ex=False):
        """One bzip2 stream of `data` at `level` (1..9; 0: 9), every block coded on the GPU; a block per 719 872 bytes of
        input at level 9 (79 872 at level 1).  The bytes are a function of (data, level) alone.  self_check: every block is
        decoded again in HBM and compared with the piece it was made from before it leaves the GPU
        (snaphash_bzip2_buffer_ex with SNAPHASH_BZ2_SELF_CHECK; bz2_selfcheck_stats() tells what was checked); the bytes
        are the same.  _ex: through the _ex entry also without the flag."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        buf = (ctypes.c_char * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        if self_check or _ex:
            opt = Bz2Options(ctypes.sizeof(Bz2Options), BZ2_SELF_CHECK if self_check else 0, level)
            self._check(lib().snaphash_bzip2_buffer_ex(self._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n)))
        else:
            self._check(lib().snaphash_bzip2_buffer(self._h, ctypes.addressof(buf), len(data), level, ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def tar_create_bz2(self, tarname, source_dir, exclude_prefix=None, with_hashes=False, level=0, self_check=False):
        """tar_create with the .bz2 producer: the format the install side reads and tarCreate refuses to write.  With the
        defaults: snaphash_tar_create_bz2 (level 9).  Anything else goes through snaphash_tar_create_bz2_ex: level and
        self_check as in bzip2_buffer.
        -> (yaml bytes or None, archive digest (64 bytes))."""
        if level == 0 and not self_check:
            return self.tar_create(tarname, source_dir, exclude_prefix, with_hashes, _entry="snaphash_tar_create_bz2")
        opt = Bz2Options(ctypes.sizeof(Bz2Options), BZ2_SELF_CHECK if self_check else 0, level)
        return self.tar_create(tarname, source_dir, exclude_prefix, with_hashes, _entry="snaphash_tar_create_bz2_ex", _opt=opt)

    def bz2_check_device(self, d_z, n_z, z_beg, z_end, d_in, n_in, in_off, in_len, crc, level):
        """The .bz2 self-check's four steps alone: d_z / d_in device addresses (ints) of the compressed bytes (n_z) and the
        staged stream (n_in); block k's bits are [z_beg[k], z_end[k]), its piece d_in[in_off[k] .. in_off[k] + in_len[k]), its
        CRC crc[k]; level: the stream's.  -> [(status, offset)] a block.  Synchronous."""
        nb = len(z_beg)
        assert len(z_end) == nb and len(in_off) == nb and len(in_len) == nb and len(crc) == nb
        arr = lambda t, v: (t * max(nb, 1))(*v)
        v = (ctypes.c_uint32 * (2 * max(nb, 1)))()
        self._check(lib().snaphash_bz2_check_device(self._h, d_z, n_z, arr(ctypes.c_uint64, z_beg), arr(ctypes.c_uint64, z_end), d_in, n_in,
                                                    arr(ctypes.c_uint64, in_off), arr(ctypes.c_uint64, in_len), arr(ctypes.c_uint32, crc), level, nb,
                                                    ctypes.cast(v, ctypes.c_void_p)))
        return [(v[2 * k], v[2 * k + 1]) for k in range(nb)]

    def bz2_selfcheck_stats(self):
        """The self-check of the last bzip2_buffer / tar_create_bz2 that went through an _ex entry, or of the data.tar.bz2 of
        the last snap_build: blocks decoded again, the check's kernels' milliseconds."""
        s = Bz2SelfCheckStats()
        s.struct_size = ctypes.sizeof(Bz2SelfCheckStats)
        self._check(lib().snaphash_get_bz2_selfcheck_stats(self._h, ctypes.byref(s)))
        return {"blocks": s.blocks, "ms": s.ms}

    def bwt_device(self, d_in, offsets, lens, d_last, d_orig_ptr):
        """The bzip2 encoder's BWT kernel alone over ranges resident in HBM.  d_in / d_last / d_orig_ptr: device addresses
        (int); offsets / lens: contiguous numpy uint64 arrays (each range 1..900 000 bytes).  d_last receives each range's
        last column at the range's offset, d_orig_ptr a uint32 per range."""
        self._check(lib().snaphash_bwt_device(self._h, d_in, offsets.ctypes.data, lens.ctypes.data, len(offsets), d_last, d_orig_ptr))

    def bzenc_stages_device(self, d_in, offsets, lens, level, cap, carry, carry_bits, arrays, out_words, from_last=None):
        """The .bz2 producer's sequence for one slot (CRCs, RLE1, BWT, MTF, coding, placement, concat) over ranges of d_in,
        every per-block array in the caller's HBM.  d_in: a device address (int); offsets / lens: contiguous numpy uint64
        arrays; arrays: the device addresses (ints) of d_rle, d_last, d_syms, d_maps, d_sel, d_slots, d_res, d_dst, d_out in
        that order, sized as snaphash.h states; from_last: None, or (rle_n, orig_ptr, crc), contiguous numpy uint32 arrays of
        a value a block -- then RLE1 and the BWT are not run and d_in / offsets / lens are not looked at.  -> the bit behind
        the last block in d_out."""
        total = ctypes.c_uint64()
        if from_last is None:
            head, nb, tail = (d_in, offsets.ctypes.data, lens.ctypes.data), len(offsets), (None, None, None)
        else:
            head, nb, tail = (None, None, None), len(from_last[0]), tuple(a.ctypes.data for a in from_last)
        self._check(lib().snaphash_bzenc_stages_device(self._h, *head, nb, level, cap, carry, carry_bits, *tail, *arrays, out_words,
                                                       ctypes.byref(total)))
        return total.value

    def tar_create_xz(self, tarname, source_dir, exclude_prefix=None, with_hashes=False, block_size=0, check=4, self_check=False, filter=None, level=0,
                      chain=None):
        """tarCreate's ".xz" branch (clickdeb/deb.go:272-273): tar_create with the .xz producer.  With the defaults:
        snaphash_tar_create_xz (1 MiB Blocks, CRC-64).  Anything else goes through snaphash_tar_create_xz_ex: block_size
        check, self_check, filter, level and chain as in xz_buffer (hashes.yaml and the Blocks' Checks are of the unfiltered
        bytes).
        -> (yaml bytes or None, archive digest (64 bytes))."""
        filter = bcj_filter(filter)
        if block_size == 0 and check == 4 and not self_check and not filter and not level and not chain:
            return self.tar_create(tarname, source_dir, exclude_prefix, with_hashes, _entry="snaphash_tar_create_xz")
        opt = xz_options(XZ_SELF_CHECK if self_check else 0, block_size, check, filter, level, chain)
        return self.tar_create(tarname, source_dir, exclude_prefix, with_hashes, _entry="snaphash_tar_create_xz_ex", _opt=opt)

    def tar_create(self, tarname, source_dir, exclude_prefix=None, with_hashes=False, _entry="snaphash_tar_create", _opt=None):
        """tarCreate (clickdeb/deb.go:261-344).  with_hashes: also hashes.yaml from the same read.
        -> (yaml bytes or None, archive digest (64 bytes))."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        dig = ctypes.create_string_buffer(64)
        extra = () if _opt is None else (ctypes.byref(_opt),)  # (the _ex entry's options)
        self._check(getattr(lib(), _entry)(self._h, os.fsencode(tarname), os.fsencode(source_dir),
                                              os.fsencode(exclude_prefix) if exclude_prefix else None, *extra,
                                              ctypes.byref(p) if with_hashes else None, ctypes.byref(n), dig))
        try:
            return (ctypes.string_at(p.value, n.value) if with_hashes else None), dig.raw
        finally:
            if with_hashes:
                lib().snaphash_free(p)

    def tar_create_fn(self, tarname, source_dir, keep=None, with_hashes=False):
        """tarCreate with the reference's own exclude function: keep(path) -> bool (clickdeb/deb.go:261, 295-299)."""
        KEEP = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p)
        cb = KEEP((lambda path, _u: 1 if keep(os.fsdecode(path)) else 0) if keep else 0)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        dig = ctypes.create_string_buffer(64)
        f = lib().snaphash_tar_create_fn
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, KEEP, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_char_p]
        self._check(f(self._h, os.fsencode(tarname), os.fsencode(source_dir), cb, None,
                      ctypes.cast(ctypes.byref(p), ctypes.c_void_p) if with_hashes else None,
                      ctypes.cast(ctypes.byref(n), ctypes.c_void_p), dig))
        try:
            return (ctypes.string_at(p.value, n.value) if with_hashes else None), dig.raw
        finally:
            if with_hashes:
                lib().snaphash_free(p)

    def gunzip_buffer(self, gz):
        """The inverse of gzip_buffer: every member of `gz` decoded, DEFLATE segments on the GPU (row f5)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        gz = bytes(gz)
        self._check(lib().snaphash_gunzip_buffer(self._h, ctypes.cast(ctypes.c_char_p(gz), ctypes.c_void_p), len(gz),
                                                 ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def tar_unpack(self, data_tar_gz, target_dir, yaml_bytes=None):
        """ClickDeb.Unpack of data.tar.gz into target_dir (clickdeb/deb.go:188-203); with yaml_bytes also the install-time
        Verify from the decoded bytes.  -> (None or (kind, name) of the first mismatch, archive digest (64 bytes))."""
        m = Mismatch()
        dig = ctypes.create_string_buffer(64)
        rc = lib().snaphash_tar_unpack(self._h, os.fsencode(data_tar_gz), os.fsencode(target_dir), yaml_bytes,
                                       len(yaml_bytes) if yaml_bytes is not None else 0, ctypes.byref(m), dig)
        if rc == EMISMATCH:
            return (m.kind, m.name.decode(errors="replace")), dig.raw
        self._check(rc)
        return None, dig.raw

    def bunzip2_buffer(self, bz):
        """Every stream of `bz` (bzip2) decoded, blocks side by side (host threads, or the GPU kernels with FLAG_GPU_ONLY)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        bz = bytes(bz)
        self._check(lib().snaphash_bunzip2_buffer(self._h, ctypes.cast(ctypes.c_char_p(bz), ctypes.c_void_p), len(bz),
                                                  ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def tar_unpack_bz2(self, data_tar_bz2, target_dir, yaml_bytes=None):
        """tar_unpack for a data.tar.bz2.  -> (None or (kind, name) of the first mismatch, archive digest (64 bytes))."""
        m = Mismatch()
        dig = ctypes.create_string_buffer(64)
        rc = lib().snaphash_tar_unpack_bz2(self._h, os.fsencode(data_tar_bz2), os.fsencode(target_dir), yaml_bytes,
                                           len(yaml_bytes) if yaml_bytes is not None else 0, ctypes.byref(m), dig)
        if rc == EMISMATCH:
            return (m.kind, m.name.decode(errors="replace")), dig.raw
        self._check(rc)
        return None, dig.raw

    def crc32_device(self, kind, d_base, offsets, lens):
        """CRC-32s (kind: CRC_GZIP / CRC_BZIP2) of byte ranges resident in HBM.  d_base: device address (int); offsets /
        lens: contiguous numpy uint64 arrays, any alignment.  -> numpy uint32 array."""
        import numpy as np
        n = len(offsets)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(lib().snaphash_crc32_device(self._h, kind, d_base, offsets.ctypes.data, lens.ctypes.data, n, out.ctypes.data))
        return out[:n]

    def deflate_codes_device(self, d_freq, n_tables, n_syms, max_bits, d_lens, d_codes, d_rounds):
        """The DEFLATE kernel's code construction alone, a wave per table.  Device addresses (int): d_freq -- n_tables x
        n_syms uint32 counts; d_lens -- as many bytes; d_codes -- as many uint32 (code << 8 | length); d_rounds -- n_tables
        uint32 (trees built before one fitted max_bits)."""
        self._check(lib().snaphash_deflate_codes_device(self._h, d_freq, n_tables, n_syms, max_bits, d_lens, d_codes, d_rounds))

    def unxz_buffer(self, xz, bcj=False, chains=False):
        """Every Stream of `xz` (.xz) decoded, Blocks side by side (host threads, or the GPU kernel with FLAG_GPU_ONLY).
        bcj: also take Blocks with an x86, ARM or ARM-Thumb filter in front of LZMA2 (snaphash_unxz_buffer_ex with
        SNAPHASH_UNXZ_BCJ); without it such a file is SNAPHASH_EINVAL.  chains: every chain liblzma reads, up to three of
        Delta, x86, PowerPC, IA64, ARM, ARM-Thumb, SPARC in front of LZMA2 (SNAPHASH_UNXZ_CHAINS)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        xz = bytes(xz)
        if bcj or chains:
            opt = UnxzOptions(ctypes.sizeof(UnxzOptions), (UNXZ_BCJ if bcj else 0) | (UNXZ_CHAINS if chains else 0))
            self._check(lib().snaphash_unxz_buffer_ex(self._h, ctypes.cast(ctypes.c_char_p(xz), ctypes.c_void_p), len(xz), ctypes.byref(opt),
                                                      ctypes.byref(p), ctypes.byref(n)))
        else:
            self._check(lib().snaphash_unxz_buffer(self._h, ctypes.cast(ctypes.c_char_p(xz), ctypes.c_void_p), len(xz),
                                                   ctypes.byref(p), ctypes.byref(n)))
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def tar_unpack_xz(self, data_tar_xz, target_dir, yaml_bytes=None, bcj=False, chains=False):
        """tar_unpack for a data.tar.xz; bcj and chains as in unxz_buffer (snaphash_tar_unpack_xz_ex).
        -> (None or (kind, name) of the first mismatch, archive digest (64 bytes))."""
        m = Mismatch()
        dig = ctypes.create_string_buffer(64)
        ylen = len(yaml_bytes) if yaml_bytes is not None else 0
        if bcj or chains:
            opt = UnxzOptions(ctypes.sizeof(UnxzOptions), (UNXZ_BCJ if bcj else 0) | (UNXZ_CHAINS if chains else 0))
            rc = lib().snaphash_tar_unpack_xz_ex(self._h, os.fsencode(data_tar_xz), os.fsencode(target_dir), yaml_bytes, ylen, ctypes.byref(opt),
                                                 ctypes.byref(m), dig)
        else:
            rc = lib().snaphash_tar_unpack_xz(self._h, os.fsencode(data_tar_xz), os.fsencode(target_dir), yaml_bytes, ylen, ctypes.byref(m), dig)
        if rc == EMISMATCH:
            return (m.kind, m.name.decode(errors="replace")), dig.raw
        self._check(rc)
        return None, dig.raw

    def unxz_block_device(self, xz, block, d_dst, dst_len):
        """Block `block` of the .xz file `xz` decoded by the GPU kernel to the device address d_dst (int), dst_len bytes:
        the Block's uncompressed size.  Its Check is not taken."""
        xz = bytes(xz)
        self._check(lib().snaphash_unxz_block_device(self._h, ctypes.cast(ctypes.c_char_p(xz), ctypes.c_void_p), len(xz), block, d_dst, dst_len))

    def xzenc_stages_device(self, d_in, n, block_size, launch_chunks, d_prev, d_cand, d_slots, d_res, d_dst, d_out, out_cap, level=None):
        """The .xz encoder's chain, chunk and concatenation kernels over d_in[0..n) in the caller's HBM (device addresses
        as ints; sizes as snaphash.h states them), the chunks in launches of launch_chunks (0: the producer's).  Block
        headers, padding and Checks are not written.  level: None for the plain entry; 0 or 1 for
        snaphash_xzenc_stages_device_ex (at level 1 d_cand holds 4 words a byte).  -> every Block's total bytes in d_out."""
        bs = block_size or 1 << 20
        tot = (ctypes.c_uint64 * max((n + bs - 1) // bs, 1))()
        if level is not None:
            self._check(lib().snaphash_xzenc_stages_device_ex(self._h, d_in, n, block_size, launch_chunks, d_prev, d_cand, d_slots, d_res, d_dst,
                                                              d_out, out_cap, tot, level))
            return list(tot[:(n + bs - 1) // bs])
        self._check(lib().snaphash_xzenc_stages_device(self._h, d_in, n, block_size, launch_chunks, d_prev, d_cand, d_slots, d_res, d_dst,
                                                       d_out, out_cap, tot))
        return list(tot[:(n + bs - 1) // bs])

    def sha512_jobs_device(self, kernel, jobs, n_rows, d_state, d_digests, staged=False):
        """One SHA-512 kernel (KERNEL_WIDE / _SPLIT / _PAIR; staged: PAIR under its second name) alone over a job table in
        the caller's order.  jobs: (device address, nbytes, total_prev, idx, flags) tuples, flags JOB_FIRST | JOB_FINAL;
        d_state / d_digests: device addresses (ints) of n_rows rows of 8 uint64 / 64 bytes.  Synchronous."""
        tab = (Sha512Job * max(len(jobs), 1))(*[Sha512Job(*j) for j in jobs])
        self._check(lib().snaphash_sha512_jobs_device(self._h, kernel, 1 if staged else 0, tab, len(jobs), n_rows, d_state, d_digests))

    def crc64_device(self, d_base, offsets, lens):
        """CRC-64/XZ of byte ranges resident in HBM.  d_base: device address (int); offsets / lens: contiguous numpy
        uint64 arrays, any alignment.  -> numpy uint64 array."""
        import numpy as np
        n = len(offsets)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(lib().snaphash_crc64_device(self._h, d_base, offsets.ctypes.data, lens.ctypes.data, n, out.ctypes.data))
        return out[:n]

    def bcj_device(self, filter, encode, d_base, offsets, lens, start_offset=0):
        """A BCJ filter in place over byte ranges resident in HBM, each range a Block of its own (snaphash_bcj_device).
        filter: "x86", "arm", "armthumb" or 4, 7, 8; encode: the producer's direction (False: the decoder's); d_base: device
        address (int); offsets / lens: contiguous numpy uint64 arrays, any alignment, no overlap.  stats() tells the
        kernels' milliseconds and their number."""
        n = len(offsets)
        self._check(lib().snaphash_bcj_device(self._h, bcj_filter(filter), 1 if encode else 0, d_base, offsets.ctypes.data if n else None,
                                              lens.ctypes.data if n else None, n, start_offset))

    def xz_filter_device(self, filter, encode, d_base, offsets, lens, start_offset=0, param=0):
        """Any filter liblzma takes in front of LZMA2, in place over byte ranges resident in HBM, each range a Block of its own
        (snaphash_xz_filter_device).  filter: "delta", "x86", "powerpc", "ia64", "arm", "armthumb", "sparc", a pair
        ("delta", distance), or an id 3 .. 9; param: Delta's distance, 1 .. 256; the rest as bcj_device."""
        if isinstance(filter, tuple):
            filter, param = filter
        fid = XZ_FILTER_NAMES.get(filter, filter) if isinstance(filter, str) else filter
        if not isinstance(fid, int):
            raise ValueError("unknown .xz filter %r" % (filter,))
        n = len(offsets)
        self._check(lib().snaphash_xz_filter_device(self._h, fid, param, 1 if encode else 0, d_base, offsets.ctypes.data if n else None,
                                                    lens.ctypes.data if n else None, n, start_offset))

    def xz_filter_stats(self):
        """What the BCJ filters did in the last .xz call of either side: the filter, Blocks filtered by the kernels and on
        host threads, the kernels' milliseconds."""
        s = XzFilterStats()
        s.struct_size = ctypes.sizeof(XzFilterStats)
        self._check(lib().snaphash_get_xz_filter_stats(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in XzFilterStats._fields_ if f[0] != "struct_size"}

    def sha256_device(self, d_base, offsets, lens):
        """SHA-256 of byte ranges resident in HBM.  d_base: device address (int); offsets / lens: contiguous numpy
        uint64 arrays, any alignment.  -> numpy uint8 array of shape (n, 32), a range's digest at its own index."""
        import numpy as np
        n = len(offsets)
        out = np.zeros((max(n, 1), 32), dtype=np.uint8)
        self._check(lib().snaphash_sha256_device(self._h, d_base, offsets.ctypes.data, lens.ctypes.data, n, out.ctypes.data))
        return out[:n]

    def xz_check_stats(self):
        """Who took the Blocks' Checks in the last unxz_buffer / tar_unpack_xz: Blocks per Check kernel, Blocks on host
        threads, the Check kernels' milliseconds."""
        s = XzCheckStats()
        s.struct_size = ctypes.sizeof(XzCheckStats)
        self._check(lib().snaphash_get_xz_check_stats(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in XzCheckStats._fields_ if f[0] not in ("struct_size", "reserved")}

    def snap_build(self, source_dir, snap_path, hashes=True, check=False, mtime=-1, codec="gz", **codec_options):
        """ClickDeb.Build with snappy.Build's callback: source_dir (with its DEBIAN/) -> the .snap at snap_path, every
        source file read once.  hashes=False is the reference's nil callback (no DEBIAN/hashes.yaml); check=True runs
        the self-check kernels over what is written (control.tar.gz's DEFLATE stream, and the data member's by its
        producer's own check); mtime < 0: now.  codec: the data member -- "gz" (data.tar.gz, what the reference writes),
        "xz" or "bz2" (or snaphash_snap_build_options.data_codec's number).  codec_options go to the member's producer as
        tar_create_xz / tar_create_bz2 take them: block_size, xz_check (the Blocks' Check: an id or "none", "crc32",
        "crc64", "sha256"), filter, chain and level for "xz"; level for "bz2"; self_check for either.  Options of a codec that
        is not chosen are refused by the library (EINVAL), as are the producers' own refusals.
        -> (archive digest, digest of the .snap written, stats dict)."""
        unknown = set(codec_options) - {"block_size", "xz_check", "filter", "chain", "level", "self_check"}
        if unknown:
            raise TypeError("snap_build: unknown codec option %s" % sorted(unknown))
        codec = DATA_CODECS.get(codec, codec)
        opt = SnapBuildOptions(ctypes.sizeof(SnapBuildOptions), (0 if hashes else BUILD_NO_HASHES) | (BUILD_CHECK if check else 0), int(mtime),
                               int(codec))
        xz_only = {k: codec_options[k] for k in ("block_size", "xz_check", "filter", "chain") if k in codec_options}
        shared = {k: codec_options[k] for k in ("level", "self_check") if k in codec_options}
        if xz_only or (shared and codec != DATA_CODECS["bz2"]):  # (with "gz" or an unknown codec too: the library refuses them)
            chk = xz_only.get("xz_check", 4)
            xo = xz_options(XZ_SELF_CHECK if shared.get("self_check") else 0, xz_only.get("block_size", 0),
                            XZ_CHECK_NAMES[chk] if isinstance(chk, str) else int(chk), bcj_filter(xz_only.get("filter")), shared.get("level", 0),
                            xz_only.get("chain"))
            opt.xz = ctypes.cast(ctypes.pointer(xo), ctypes.POINTER(XzOptions))  # (xo lives to the end of this call)
        elif shared:
            bo = Bz2Options(ctypes.sizeof(Bz2Options), BZ2_SELF_CHECK if shared.get("self_check") else 0, shared.get("level", 0))
            opt.bz2 = ctypes.pointer(bo)
        st = SnapBuildStats()
        st.struct_size = ctypes.sizeof(SnapBuildStats)
        adig, sdig = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        self._check(lib().snaphash_snap_build(self._h, os.fsencode(source_dir), os.fsencode(snap_path), ctypes.byref(opt), adig, sdig,
                                              ctypes.byref(st)))
        return adig.raw, sdig.raw, {f[0]: getattr(st, f[0]) for f in SnapBuildStats._fields_ if f[0] not in ("struct_size", "reserved")}

    def deflate_check_device(self, d_in, n_in, d_z, z_off, last_is_final=False):
        """deflate_check_kernel alone: d_in / d_z device addresses (ints) of the staged stream (n_in bytes) and the
        compressed bytes; z_off: the len(z_off) - 1 chunks' stretches.  -> [(status, offset)] a chunk.  Synchronous."""
        nch = len(z_off) - 1
        off = (ctypes.c_uint64 * (nch + 1))(*z_off)
        v = (ctypes.c_uint32 * (2 * max(nch, 1)))()
        self._check(lib().snaphash_deflate_check_device(self._h, d_in, n_in, d_z, off, nch, 1 if last_is_final else 0,
                                                        ctypes.cast(v, ctypes.c_void_p)))
        return [(v[2 * c], v[2 * c + 1]) for c in range(nch)]

    def lzma2_check_device(self, d_in, n_in, block_size, d_z, n_z, z_beg, z_end, launch_chunks=0):
        """lzma2_check_kernel alone: d_in / d_z device addresses (ints) of the staged stream (n_in bytes, Blocks of
        block_size) and the compressed bytes (n_z); chunk c's stretch is [z_beg[c], z_end[c]).  -> [(status, offset)] a
        chunk.  Synchronous."""
        nch = len(z_beg)
        assert len(z_end) == nch
        beg = (ctypes.c_uint64 * max(nch, 1))(*z_beg)
        end = (ctypes.c_uint64 * max(nch, 1))(*z_end)
        v = (ctypes.c_uint32 * (2 * max(nch, 1)))()
        self._check(lib().snaphash_lzma2_check_device(self._h, d_in, n_in, block_size, d_z, n_z, beg, end, nch, launch_chunks,
                                                      ctypes.cast(v, ctypes.c_void_p)))
        return [(v[2 * c], v[2 * c + 1]) for c in range(nch)]

    def xz_selfcheck_stats(self):
        """The self-check of the last xz_buffer / tar_create_xz that went through an _ex entry, or of the data.tar.xz of the
        last snap_build: chunks walked, the check kernel's milliseconds."""
        s = XzSelfCheckStats()
        s.struct_size = ctypes.sizeof(XzSelfCheckStats)
        self._check(lib().snaphash_get_xz_selfcheck_stats(self._h, ctypes.byref(s)))
        return {"chunks": s.chunks, "ms": s.ms}

    def snap_open(self, snap_path, xz=False, chains=False):
        """A session on a .snap file (ClickDeb.Open): see Snap.  xz: ".xz" members are read too (snaphash_snap_open_ex with
        SNAPHASH_SNAP_XZ); without it they are refused with the reference's "Can not handle" text.  chains (with xz): their
        Blocks may carry every chain unxz_buffer(chains=True) takes (SNAPHASH_SNAP_XZ_CHAINS)."""
        return Snap(self, snap_path, xz=xz, chains=chains)

    def unpack_stats(self):
        s = UnpackStats()
        s.struct_size = ctypes.sizeof(UnpackStats)
        self._check(lib().snaphash_get_unpack_stats(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in UnpackStats._fields_ if f[0] not in ("struct_size", "reserved")}

    def block_scan_stats(self):
        """What the block scan and the link did in the last gunzip_buffer / tar_unpack (FLAG_SPLIT_BLOCKS)."""
        s = BlockScanStats()
        s.struct_size = ctypes.sizeof(BlockScanStats)
        self._check(lib().snaphash_get_block_scan_stats(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in BlockScanStats._fields_ if f[0] not in ("struct_size", "reserved")}

    def targz_stats(self):
        s = TargzStats()
        lib().snaphash_get_targz_stats(self._h, ctypes.byref(s))
        return {f[0]: getattr(s, f[0]) for f in TargzStats._fields_}

    def batch(self, n_streams):
        """Streaming batch (row f2): feed chunks as another pass reads them."""
        return Batch(self, n_streams)

    def verify(self, inst_dir, yaml_bytes, data_tar=None):
        """-> None when the tree matches, else (kind, name) of the first mismatch."""
        m = Mismatch()
        rc = lib().snaphash_verify(self._h, os.fsencode(inst_dir), os.fsencode(data_tar) if data_tar else None,
                                   yaml_bytes, len(yaml_bytes), ctypes.byref(m))
        if rc == EMISMATCH:
            return (m.kind, m.name.decode(errors="replace"))
        self._check(rc)
        return None

    # ---- neighbouring scan: helpers.FilesAreEqual / DirUpdated ------------------------------
    def files_equal(self, pairs):
        """[(a, b)] -> [bool]; like helpers.FilesAreEqual any open/stat/read error means False."""
        n = len(pairs)
        a = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p[0]) for p in pairs])
        b = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p[1]) for p in pairs])
        out = ctypes.create_string_buffer(max(n, 1))
        self._check(lib().snaphash_files_equal(self._h, a, b, n, out))
        return [bool(x) for x in out.raw[:n]]

    def ranges_equal_device(self, d_a, off_a, d_b, off_b, lens, d_equal):
        self._check(lib().snaphash_ranges_equal_device(self._h, d_a, off_a.ctypes.data, d_b, off_b.ctypes.data,
                                                       lens.ctypes.data, len(lens), d_equal))

    def dir_updated(self, dir_a, dir_b, pfx=""):
        """helpers.DirUpdated -> {name: True} like the Go map."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().snaphash_dir_updated(self._h, os.fsencode(dir_a), os.fsencode(dir_b), pfx.encode(),
                                               ctypes.byref(p), ctypes.byref(n)))
        try:
            names, addr = {}, p.value
            for _ in range(n.value):
                s_ = ctypes.string_at(addr)
                names[s_.decode(errors="surrogateescape")] = True
                addr += len(s_) + 1
            return names
        finally:
            lib().snaphash_free(p)

    def stats(self):
        s = Stats()
        lib().snaphash_get_stats(self._h, ctypes.byref(s))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def stats_ex(self):
        s = StatsEx(ctypes.sizeof(StatsEx))
        self._check(lib().snaphash_get_stats_ex(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in StatsEx._fields_}

    def plan_model(self, from_files):
        """snaphash_get_plan_model: what this ctx plans a call with right now (calibrated link and fill rates included);
        its fields are keyword arguments of plan_streams()."""
        pm = PlanModel(ctypes.sizeof(PlanModel))
        self._check(lib().snaphash_get_plan_model(self._h, 1 if from_files else 0, ctypes.byref(pm)))
        return {k: getattr(pm, k) for k in ("n_devices", "cpus", "fill_threads", "host_threads", "from_files", "host_rate",
                                            "gpu_stream_rate", "gpu_link", "gpu_latency", "host_lane_gain_pct", "fill_rate", "fill_per_file")}

    def calib(self):
        c = PlanCalib(ctypes.sizeof(PlanCalib))
        self._check(lib().snaphash_get_calib(self._h, ctypes.byref(c)))
        return {f[0]: getattr(c, f[0]) for f in PlanCalib._fields_ if f[0] != "struct_size"}

    def engine_info(self, i):
        e = EngineInfo(ctypes.sizeof(EngineInfo))
        self._check(lib().snaphash_get_engine_info(self._h, i, ctypes.byref(e)))
        out = {f[0]: getattr(e, f[0]) for f in EngineInfo._fields_}
        out["pci_bus_id"] = e.pci_bus_id.decode()
        return out

    def engine_cpus(self, i):
        n = ctypes.c_size_t()
        self._check(lib().snaphash_get_engine_cpus(self._h, i, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_int32 * max(n.value, 1))()
        self._check(lib().snaphash_get_engine_cpus(self._h, i, buf, n.value, ctypes.byref(n)))
        return list(buf[:n.value])

    def device_stats(self, i):
        s, d = Stats(), ctypes.c_int32()
        self._check(lib().snaphash_get_device_stats(self._h, i, ctypes.byref(d), ctypes.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in Stats._fields_}
        out["device"] = d.value
        return out


class Snap:
    """snaphash_snap_*: one .snap file read once, its ar members, and its two tars decoded at most once each."""

    def __init__(self, ctx, snap_path, xz=False, _opt=None, chains=False):
        self._ctx = ctx
        h = ctypes.c_void_p()
        if xz or chains or _opt is not None:  # (_opt: a SnapOpenOptions as it is, for the tests of the entry's refusals)
            flags = (SNAP_XZ if xz else 0) | (SNAP_XZ_CHAINS if chains else 0)
            opt = _opt if _opt is not None else SnapOpenOptions(ctypes.sizeof(SnapOpenOptions), flags)
            ctx._check(lib().snaphash_snap_open_ex(ctx._h, os.fsencode(snap_path), ctypes.byref(opt), ctypes.byref(h)))
        else:
            ctx._check(lib().snaphash_snap_open(ctx._h, os.fsencode(snap_path), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().snaphash_snap_close(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def members(self):
        """-> [(name, offset of the data in the file, size)] in file order."""
        out = []
        name, off, size = ctypes.c_char_p(), ctypes.c_uint64(), ctypes.c_uint64()
        for i in range(lib().snaphash_snap_members(self._h)):
            self._ctx._check(lib().snaphash_snap_member_info(self._h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(size)))
            out.append((name.value.decode(errors="surrogateescape"), off.value, size.value))
        return out

    def _member(self, fn, name):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._ctx._check(fn(self._h, os.fsencode(name), ctypes.byref(p), ctypes.byref(n)))
        if not p.value:
            return None
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)

    def control_member(self, name):
        """ClickDeb.ControlMember -> bytes, or None when control.tar.* has no such member."""
        return self._member(lib().snaphash_snap_control_member, name)

    def meta_member(self, name):
        """ClickDeb.MetaMember -> bytes of meta/<name> in data.tar.*, or None."""
        return self._member(lib().snaphash_snap_meta_member, name)

    def _verdict(self, rc, m, dig):
        if rc == EMISMATCH:
            return (m.kind, m.name.decode(errors="replace")), dig.raw
        self._ctx._check(rc)
        return None, dig.raw

    def unpack(self, target_dir, verify=True):
        """ClickDeb.Unpack into target_dir; verify: also the install-time Verify against the package's own hashes.yaml.
        -> (None or (kind, name) of the first mismatch, SHA-512 of the data.tar.* member (64 bytes))."""
        m, dig = Mismatch(), ctypes.create_string_buffer(64)
        return self._verdict(lib().snaphash_snap_unpack(self._h, os.fsencode(target_dir), 1 if verify else 0, ctypes.byref(m), dig), m, dig)

    def audit(self):
        """Every check the package carries, nothing written.  -> (None or (kind, name), SHA-512 of the data.tar.* member)."""
        m, dig = Mismatch(), ctypes.create_string_buffer(64)
        return self._verdict(lib().snaphash_snap_audit(self._h, ctypes.byref(m), dig), m, dig)

    def stats(self):
        s = SnapStats(ctypes.sizeof(SnapStats))
        self._ctx._check(lib().snaphash_snap_get_stats(self._h, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SnapStats._fields_ if f[0] not in ("struct_size", "reserved")}


class Batch:
    """snaphash_batch_*: hash.Hash-style appends into many streams, digests at finish()."""

    def __init__(self, ctx, n_streams):
        self._ctx, self.n = ctx, n_streams
        h = ctypes.c_void_p()
        ctx._check(lib().snaphash_batch_begin(ctx._h, n_streams, ctypes.byref(h)))
        self._h = h

    def append(self, stream, data):
        buf = (ctypes.c_char * len(data)).from_buffer_copy(data) if len(data) else None
        self._ctx._check(lib().snaphash_batch_append(self._h, stream, ctypes.addressof(buf) if buf is not None else None, len(data)))

    def append_ptr(self, stream, addr, n):
        self._ctx._check(lib().snaphash_batch_append(self._h, stream, addr, n))

    def end(self, stream):
        self._ctx._check(lib().snaphash_batch_end(self._h, stream))

    def finish(self):
        out = ctypes.create_string_buffer(64 * max(self.n, 1))
        h, self._h = self._h, None
        self._ctx._check(lib().snaphash_batch_finish(h, out))
        return [out.raw[64 * i:64 * i + 64] for i in range(self.n)]

    def abort(self):
        if self._h:
            lib().snaphash_batch_abort(self._h)
            self._h = None


# ---- host-only entry points (no device) ----------------------------------------------

def walk(build_dir):
    """filepath.Walk as writeHashes drives it -> list of dicts in walk order."""
    h = ctypes.c_void_p()
    rc = lib().snaphash_walk(os.fsencode(build_dir), ctypes.byref(h))
    if rc:
        raise SnaphashError(rc, build_dir)
    try:
        out = []
        r = Record()
        for i in range(lib().snaphash_records_count(h)):
            lib().snaphash_records_get(h, i, ctypes.byref(r))
            out.append({"name": r.name.decode(errors="surrogateescape"), "st_mode": r.st_mode,
                        "is_regular": bool(r.is_regular), "size": r.size,
                        "path": r.path.decode(errors="surrogateescape")})
        return out
    finally:
        lib().snaphash_records_free(h)


def emit_yaml(build_dir, archive_digest, file_digests):
    """yaml.Marshal(hashesYaml) for the tree at build_dir with the given raw digests."""
    h = ctypes.c_void_p()
    rc = lib().snaphash_walk(os.fsencode(build_dir), ctypes.byref(h))
    if rc:
        raise SnaphashError(rc, build_dir)
    try:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        blob = b"".join(file_digests)
        rc = lib().snaphash_emit_yaml(h, archive_digest, blob if blob else None, ctypes.byref(p), ctypes.byref(n))
        if rc:
            raise SnaphashError(rc)
        try:
            return ctypes.string_at(p.value, n.value)
        finally:
            lib().snaphash_free(p)
    finally:
        lib().snaphash_records_free(h)


def parse_yaml(text):
    """yaml.Unmarshal into hashesYaml -> (archive_hex, [record dicts])."""
    h = ctypes.c_void_p()
    arch = ctypes.create_string_buffer(129)
    rc = lib().snaphash_parse_yaml(text, len(text), ctypes.byref(h), arch)
    if rc:
        raise SnaphashError(rc)
    try:
        out = []
        r = Record()
        for i in range(lib().snaphash_records_count(h)):
            lib().snaphash_records_get(h, i, ctypes.byref(r))
            out.append({"name": r.name.decode(errors="surrogateescape"), "st_mode": r.st_mode,
                        "is_regular": bool(r.is_regular), "size": r.size,
                        "sha512": lib().snaphash_records_sha512_hex(h, i).decode()})
        return arch.value.decode(), out
    finally:
        lib().snaphash_records_free(h)


def numa_probe(sysfs_root, pci_bus_id):
    """The engines' topology probe on any sysfs tree -> (node, [cpus])."""
    node, n = ctypes.c_int32(), ctypes.c_size_t()
    cpus = (ctypes.c_int32 * 4096)()
    rc = lib().snaphash_numa_probe(os.fsencode(sysfs_root), pci_bus_id.encode(), ctypes.byref(node), cpus, 4096, ctypes.byref(n))
    if rc:
        raise SnaphashError(rc)
    return node.value, list(cpus[:min(n.value, 4096)])


def mode_string(st_mode):
    buf = ctypes.create_string_buffer(11)
    rc = lib().snaphash_mode_string(st_mode, buf)
    if rc:
        raise SnaphashError(rc)
    return buf.value.decode()


def mode_parse(s):
    m = ctypes.c_uint32()
    rc = lib().snaphash_mode_parse(s.encode(), ctypes.byref(m))
    if rc:
        raise SnaphashError(rc)
    return m.value


def lpt_assign(lens, nshards):
    import numpy as np
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.empty(len(lens), dtype=np.int32)
    rc = lib().snaphash_lpt_assign(lens.ctypes.data, len(lens), nshards, out.ctypes.data)
    if rc:
        raise SnaphashError(rc)
    return out
