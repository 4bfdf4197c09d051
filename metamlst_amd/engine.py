"""ctypes binding of libmlst_hip.so (include/mlst.h) -- the only compute path of the package.

There is no CPU fallback: if the HIP library is missing or no GPU is present the
constructor raises.  The oracle under oracle/ is test infrastructure and is never
imported from here.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from .index import AlleleIndex
from .typing import SampleStats

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLST_LIB", os.path.join(_HERE, "libmlst_hip.so"))   # MLST_LIB: profiling builds only

MLST_CNT_N = 8
CNT_TOTAL_RECORDS, CNT_IGNORED, CNT_READS_SEEN, CNT_CANDIDATES, CNT_RETAINED, CNT_ITEMS, CNT_DP_PAIRS = range(7)
KERNELS = ("sieve", "seed", "extend", "banded_sw", "accumulate", "pileup", "pack", "sieve_inkernel", "sieve_wg_longest",
           "sieve_route", "sieve_probe", "sieve_verify", "extend_prep")
SIEVE_KINDS = ("lds", "global", "binned (round 1, removed)", "routed")


class MlstParams(C.Structure):
    """struct mlst_params (include/mlst.h)."""
    _fields_ = [("minscore", C.c_int32), ("max_xm", C.c_int32), ("min_read_len", C.c_int32),
                ("minqual", C.c_int32), ("mincov", C.c_int32), ("match_bonus", C.c_int32),
                ("mm_max", C.c_int32), ("mm_min", C.c_int32), ("n_penalty", C.c_int32),
                ("gap_open", C.c_int32), ("gap_ext", C.c_int32), ("gbar", C.c_int32),
                ("band_w", C.c_int32), ("gap_trigger_mm", C.c_int32), ("xm_field_quirk", C.c_int32),
                ("gap_trigger_clip", C.c_int32), ("minscore_const", C.c_double), ("minscore_coef", C.c_double),
                ("max_retained_reads", C.c_uint64), ("max_items", C.c_uint64), ("max_pair_results", C.c_uint64)]


class MlstItem(C.Structure):
    """struct mlst_item (include/mlst.h)."""
    _fields_ = [("read_index", C.c_uint64), ("locus", C.c_uint32), ("diag", C.c_int32),
                ("strand", C.c_uint16), ("votes", C.c_uint16), ("reserved", C.c_uint32)]


def default_params() -> MlstParams:
    """Defaults of mlst_policy.h, usable without loading the library (tests, oracle)."""
    p = MlstParams()
    p.minscore, p.max_xm, p.min_read_len, p.minqual, p.mincov = 80, 5, 50, 20, 1
    p.match_bonus, p.mm_max, p.mm_min, p.n_penalty = 2, 6, 2, 1
    p.gap_open, p.gap_ext, p.gbar, p.band_w = 5, 3, 4, 8
    p.gap_trigger_mm, p.xm_field_quirk, p.gap_trigger_clip = 12, 1, 8
    p.minscore_const, p.minscore_coef = 20.0, 8.0
    p.max_retained_reads = p.max_items = p.max_pair_results = 0
    return p


class MlstError(RuntimeError):
    pass


@dataclasses.dataclass
class Alignments:
    """The records of Engine.export_alignments (mlst_alignments_fetch, include/mlst.h): one entry per record in read_index ..
    flags (bit 0 strand, bit 1 used_dp); cigar (len << 4 | op) and seq / qual (ASCII on the reference strand, raw Phred) delimited
    by cigar_off / seq_off[n_rec + 1]."""
    read_index: np.ndarray
    allele: np.ndarray
    pos0: np.ndarray
    as_: np.ndarray
    xm: np.ndarray
    diag: np.ndarray
    flags: np.ndarray
    cigar_off: np.ndarray
    cigar: np.ndarray
    seq_off: np.ndarray
    seq: np.ndarray
    qual: np.ndarray

    def __len__(self) -> int:
        return len(self.read_index)

    def pileup_arrays(self) -> tuple:
        """the arrays Engine.pileup_alignments takes behind `chosen`, in its order"""
        return (self.allele, self.pos0, self.as_, self.xm, self.cigar_off, self.cigar, self.seq_off, self.seq, self.qual)


class BgzfCrcMismatch(MlstError):
    """The library's "CRC mismatch in BGZF block <n> ..." (mlst_set_bgzf_verify): file = 1 / 2 on the paired entry, else None.
    The one place that reads the library's text for it (Engine._check); callers go by the type."""

    def __init__(self, text: str, file: int | None):
        super().__init__(text)
        self.file = file


class HostPathNeeded(MlstError):
    """The library's "host path needed: <reason> at record <n>" (mlst_submit_bam_bgzf, mlst_submit_sam_text): the BAM or the SAM
    text holds a record the device does not treat; the caller runs samin.AlignmentSample on the file, which raises or answers as
    the reference would.  Also "... at byte
    <n>" (mlst_submit_fasta): a sequence line only Python's strip() treats; the caller tiles the file with fastq.tile_fasta."""


class CorruptInput(Exception):
    """a BGZF block of the file `path` does not have the CRC-32 of its trailer: the device's report or the host's, with the file's name"""

    def __init__(self, path: str, message: str):
        super().__init__("%s: %s" % (path, message))
        self.path = path


def crc_checked(paths, fn):
    """fn(), with a CRC mismatch of a BGZF block -- the library's (BgzfCrcMismatch) or the host's for the blocks it inflates itself
    (fastq.BgzfCrcError) -- turned into CorruptInput naming the file (the paired entry says which of the two)"""
    from .fastq import BgzfCrcError
    try:
        return fn()
    except BgzfCrcMismatch as e:
        raise CorruptInput(paths[1] if e.file == 2 else paths[0], str(e)) from e
    except BgzfCrcError as e:
        raise CorruptInput(paths[0], str(e)) from e


_lib = None


def load_library(path: str | None = None):
    """Load libmlst_hip.so and declare every prototype of include/mlst.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # The PyTorch ROCm wheel bundles its own HIP / HSA runtime, this library links the system one.  Both can live in
    # one process only if torch's runtime initialises first ("No HIP GPUs are available" otherwise), so when torch
    # is installed it is imported before the engine is loaded.  torch is not needed by the engine itself.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(path):
        raise MlstError("HIP engine library not built: %s is missing (run __graft_entry__.build()); "
                        "there is no CPU fallback" % path)
    lib = C.CDLL(path)
    vp, u8p, u64p, u32p, i32p, i64p, u16p = (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    H = C.c_void_p
    sig = {
        "mlst_default_params": (None, [C.POINTER(MlstParams)]),
        "mlst_create": (C.c_int, [C.c_int, C.POINTER(MlstParams), C.POINTER(H)]),
        "mlst_destroy": (None, [H]),
        "mlst_last_error": (C.c_char_p, [H]),
        "mlst_load_reference": (C.c_int, [H, u8p, u64p, u32p, u32p, i32p, C.c_uint32]),
        "mlst_set_reference_cache": (C.c_int, [C.c_char_p]),
        "mlst_submit_reads": (C.c_int, [H, u8p, u8p, u64p, C.c_uint64, C.c_int]),
        "mlst_submit_fastq": (C.c_int, [H, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
        "mlst_submit_fasta": (C.c_int, [H, u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_submit_fastq_bgzf": (C.c_int, [H, u8p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_submit_fastq_bgzf_pair": (C.c_int, [H, u8p, C.c_uint64, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]),
        "mlst_selftest_inflate": (C.c_int, [u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_selftest_inflate_canon": (C.c_int, [u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
        "mlst_debug_bgzf_walk": (C.c_int, [u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
        "mlst_selftest_inflate_device": (C.c_int, [H, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "mlst_selftest_bgzf_crc": (C.c_int, [H, u8p, C.c_uint64, u32p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "mlst_debug_inflate_paths": (C.c_int, [H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_set_bgzf_verify": (C.c_int, [H, C.c_int]),
        "mlst_get_bgzf_verify": (C.c_int, [H, C.POINTER(C.c_int)]),
        "mlst_set_read_tiling": (C.c_int, [H, C.c_uint32, C.c_uint32]),
        "mlst_get_read_tiling": (C.c_int, [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "mlst_get_read_tiling_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_names": (C.c_int, [H, C.c_int]),
        "mlst_get_read_names": (C.c_int, [H, C.POINTER(C.c_int)]),
        "mlst_set_read_prep": (C.c_int, [H, C.POINTER(C.c_uint32)]),      # (mlst_read_prep: four uint32_t)
        "mlst_get_read_prep": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "mlst_read_prep_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_adapters": (C.c_int, [H, C.c_char_p, C.c_uint32, C.c_uint32]),
        "mlst_get_read_adapters": (C.c_int, [H, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "mlst_get_read_adapters_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_stats": (C.c_int, [H, C.c_int]),
        "mlst_get_read_stats": (C.c_int, [H, C.POINTER(C.c_int)]),
        "mlst_set_read_stats_side": (C.c_int, [H, C.c_int]),
        "mlst_read_stats_fetch": (C.c_int, [H, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64]),
        "mlst_read_stats_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_dedup": (C.c_int, [H, C.c_int]),
        "mlst_get_read_dedup": (C.c_int, [H, C.POINTER(C.c_int)]),
        "mlst_read_dedup_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_pair_overlap": (C.c_int, [H, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]),
        "mlst_get_read_pair_overlap": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "mlst_read_pair_overlap_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_read_pair_overlap_hist": (C.c_int, [H, C.POINTER(C.c_uint64), C.c_uint64]),
        "mlst_set_read_filter": (C.c_int, [H, C.POINTER(C.c_uint32)]),      # (mlst_read_filter: six uint32_t)
        "mlst_get_read_filter": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "mlst_read_filter_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_read_window": (C.c_int, [H, C.POINTER(C.c_uint32)]),      # (mlst_read_window: six uint32_t)
        "mlst_get_read_window": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "mlst_read_window_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_set_export_md": (C.c_int, [H, C.c_int]),
        "mlst_get_export_md": (C.c_int, [H, C.POINTER(C.c_int)]),
        "mlst_read_names_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_read_names_fetch": (C.c_int, [H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]),
        "mlst_submit_reads_device": (C.c_int, [H, u8p, u8p, u64p, C.c_uint64, C.c_uint32, C.c_int]),
        "mlst_pack_reads_device": (C.c_int, [H, u8p, u8p, u64p, C.c_uint64, u32p, u8p, u16p, C.c_uint32, C.c_uint32]),
        "mlst_submit_packed_device": (C.c_int, [H, u32p, u8p, u16p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]),
        "mlst_pack_fastq_host": (C.c_int, [u8p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u8p, u16p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]),
        "mlst_submit_packed_host": (C.c_int, [H, u32p, u8p, u16p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]),
        "mlst_alloc_host": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
        "mlst_free_host": (C.c_int, [C.c_void_p]),
        "mlst_get_allele_stats": (C.c_int, [H, i64p, u32p, u64p, u64p, u64p]),
        "mlst_stats_flat_sizes": (C.c_int, [H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_export_stats_device": (C.c_int, [H, i64p, i64p]),
        "mlst_import_stats_device": (C.c_int, [H, i64p, i64p]),
        "mlst_pileup": (C.c_int, [H, u32p, C.c_uint32, u32p]),
        "mlst_set_depth_cap": (C.c_int, [H, C.c_uint32]),
        "mlst_pileup_device": (C.c_int, [H, u32p, C.c_uint32, u32p, C.POINTER(C.c_uint64)]),
        "mlst_consensus": (C.c_int, [H, u32p, C.c_uint32, C.c_uint32, C.c_char, u8p, u32p]),
        "mlst_consensus_from_counts_device": (C.c_int, [H, u32p, C.c_uint64, C.c_uint32, C.c_char, u8p]),
        "mlst_pileup_alignments": (C.c_int, [H, u32p, C.c_uint32, C.c_uint64, u32p, i32p, i32p, i32p, u64p, u32p, u64p, u8p, u8p,
                                             C.c_int32, C.c_int32, C.c_int32, u32p]),
        "mlst_alignments_export": (C.c_int, [H, u32p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_alignments_fetch": (C.c_int, [H, u64p, u32p, i32p, i32p, i32p, i32p, u8p, u64p, u32p, u64p, u8p, u8p]),
        "mlst_alignments_text_open": (C.c_int, [H, u8p, u64p, C.c_int, C.c_uint64]),
        "mlst_alignments_text_next": (C.c_int, [H, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
        "mlst_alignments_text_close": (C.c_int, [H]),
        "mlst_reads_text_open": (C.c_int, [H, C.c_int, C.c_uint64]),
        "mlst_reads_text_next": (C.c_int, [H, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
        "mlst_reads_text_close": (C.c_int, [H]),
        "mlst_typing_layout": (C.c_int, [H, u64p, C.POINTER(C.c_uint64)]),
        "mlst_typing_enqueue": (C.c_int, [H, C.c_int32, C.c_uint32, C.c_char]),
        "mlst_typing_choose_pileup": (C.c_int, [H, C.c_int32, u32p]),
        "mlst_typing_finish": (C.c_int, [H, C.c_uint32, C.c_char, u32p]),
        "mlst_typing_choose_pileup_compact": (C.c_int, [H, C.c_int32, u32p, C.c_uint64]),
        "mlst_typing_finish_compact": (C.c_int, [H, C.c_uint32, C.c_char, u32p]),
        "mlst_typing_compact_info": (C.c_int, [H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "mlst_set_stream": (C.c_int, [H, C.c_void_p]),
        "mlst_set_cu_partition": (C.c_int, [H, C.c_uint32, C.c_uint32]),
        "mlst_get_stream": (C.c_int, [H, C.POINTER(C.c_void_p)]),
        "mlst_busy": (C.c_int, [H]),
        "mlst_export_stats_device_async": (C.c_int, [H, i64p, i64p]),
        "mlst_import_stats_device_async": (C.c_int, [H, i64p, i64p]),
        "mlst_typing_fetch": (C.c_int, [H, i64p, u32p, u64p, u64p, u64p, i32p, u8p]),
        "mlst_typing_wait": (C.c_int, [H]),
        "mlst_typing_fetch_waited": (C.c_int, [H, i64p, u32p, u64p, u64p, u64p, i32p, u8p]),
        "mlst_round_tenths": (C.c_longlong, [C.c_longlong, C.c_uint32]),
        "mlst_hamming_le": (C.c_int, [H, C.c_uint32, u8p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
        "mlst_hamming_all": (C.c_int, [H, C.c_uint32, u8p, C.c_uint32, u32p]),
        "mlst_msa_align": (C.c_int, [H, u8p, u64p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "mlst_msa_fetch": (C.c_int, [H, u8p]),
        "mlst_reset_sample": (C.c_int, [H]),
        "mlst_set_read_index_base": (C.c_int, [H, C.c_uint64]),
        "mlst_get_items": (C.c_int, [H, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_set_profiling": (C.c_int, [H, C.c_int]),
        "mlst_get_kernel_time": (C.c_int, [H, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "mlst_reset_kernel_time": (C.c_int, [H]),
        "mlst_get_index_bytes": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_get_sieve_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_get_extend_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_release_index_cache": (None, []),
        "mlst_submit_fastq_stream": (C.c_int, [H, u8p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
        "mlst_submit_fastq_pair": (C.c_int, [H, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_get_route_trace": (C.c_int, [H, u64p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_debug_route_realloc": (C.c_int, [H, C.c_uint64]),
        "mlst_debug_route_probe": (C.c_int, [H, C.POINTER(C.c_uint64), u32p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_bam_open": (C.c_int, [H, C.c_int, i32p, i32p, u8p, C.c_uint32, C.c_uint32, u32p, C.c_uint32]),
        "mlst_submit_bam_bgzf": (C.c_int, [H, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mlst_bam_set_capacity": (C.c_int, [H, C.c_uint64]),
        "mlst_bam_pileup_fetch": (C.c_int, [H, u32p]),
        "mlst_debug_bam_split": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint64)]),
        "mlst_sam_open": (C.c_int, [H, C.c_int, u8p, u64p, i32p, i32p, u8p, C.c_uint32, u32p, C.c_uint32]),
        "mlst_submit_sam_text": (C.c_int, [H, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
        "mlst_bam_reads_open": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_int]),
        "mlst_bam_reads_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_debug_last_packed": (C.c_int, [H, u32p, C.c_uint64, u8p, C.c_uint64, u16p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "mlst_debug_fasta_info": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "mlst_synchronize": (C.c_int, [H]),
    }
    tolerant = bool(os.environ.get("MLST_LIB_ALLOW_MISSING"))      # A/B runs against an older build (profiles/ab.sh)
    for name, (res, args) in sig.items():
        if tolerant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)          # AttributeError here = the library does not export the ABI
        fn.restype, fn.argtypes = res, args
    lib._mlst_symbols = tuple(sig)
    if path == LIB_PATH:
        _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def pack_fastq_host(text, read_len_max: int = 160, threads: int = 0):
    """FASTQ text (bytes / uint8 array of whole records) -> (packed, qrows, lens, n_reads, words_per_read, qual_stride): the engine's
    resident read format made on the host by all its threads (mlst_pack_fastq_host), for Engine.submit_packed_host."""
    lib = load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    wpr = ((int(read_len_max) + 31) // 32) * 2
    qstride = (int(read_len_max) + 7) // 8 * 8
    cap = int(buf.size // 8 + 64)                       # a record is at least 8 bytes
    cap = min(cap, int(np.count_nonzero(buf[:1 << 20] == 10) * (buf.size / max(1, min(buf.size, 1 << 20))) / 4 * 1.1) + 4096)
    packed = np.zeros(((cap + 63) // 64) * 64 * wpr, np.uint32)
    qrows = np.empty((cap, qstride), np.uint8)
    lens = np.empty(cap, np.uint16)
    n = C.c_uint64()
    rc = lib.mlst_pack_fastq_host(_ptr(buf), buf.size, wpr, qstride, _ptr(packed), _ptr(qrows), _ptr(lens), cap, C.byref(n), int(threads))
    if rc == -4:                                        # MLST_E_CAPACITY: the estimate from the first megabyte was too low
        cap = int(buf.size // 8 + 64)
        packed = np.zeros(((cap + 63) // 64) * 64 * wpr, np.uint32); qrows = np.empty((cap, qstride), np.uint8); lens = np.empty(cap, np.uint16)
        rc = lib.mlst_pack_fastq_host(_ptr(buf), buf.size, wpr, qstride, _ptr(packed), _ptr(qrows), _ptr(lens), cap, C.byref(n), int(threads))
    if rc != 0:
        raise MlstError("mlst_pack_fastq_host failed (%d): not whole 4-line FASTQ records, or a read longer than %d bases" % (rc, read_len_max))
    return packed, qrows, lens, int(n.value), wpr, qstride


def pinned_array(n_bytes: int) -> np.ndarray:
    """uint8 array of n_bytes in page-locked host memory (mlst_alloc_host); the memory is released when the array is collected.
    Needs the GPU runtime: raises MlstError where there is none."""
    import weakref
    lib = load_library()
    p = C.c_void_p()
    rc = lib.mlst_alloc_host(int(n_bytes), C.byref(p))
    if rc != 0 or not p.value:
        raise MlstError("mlst_alloc_host(%d) failed (%d)" % (n_bytes, rc))
    arr = np.frombuffer((C.c_uint8 * int(n_bytes)).from_address(p.value), np.uint8)
    weakref.finalize(arr, lib.mlst_free_host, C.c_void_p(p.value)).atexit = False      # (at interpreter exit the runtime may be gone: the OS takes the pages)
    return arr


def pair_file_cuts(size1: int, size2: int, chunk_bytes: int) -> list[tuple[int, int, int, int]]:
    """Byte ranges (lo1, hi1, lo2, hi2) of two mate files, one per call of Engine.submit_fastq_bgzf_pair_files: together about
    chunk_bytes a call, the same fraction of each file (so both files reach the same record at about the same call however
    differently they compress), the first call a quarter of the others.  The ranges of a file follow each other without gaps."""
    total = size1 + size2
    if total == 0:
        return [(0, 0, 0, 0)]
    chunk = max(1, int(chunk_bytes))
    marks = [0.0]
    step = min(1.0, chunk / 4 / total)
    while marks[-1] < 1.0:
        marks.append(min(1.0, marks[-1] + step))
        step = min(1.0, chunk / total)
    cuts = []
    for a, b in zip(marks, marks[1:]):
        cuts.append((int(size1 * a), int(size1 * b) if b < 1.0 else size1, int(size2 * a), int(size2 * b) if b < 1.0 else size2))
    return cuts


class Engine:
    """One GPU's typing engine.  Mirrors the reference's per-sample flow:
    load_reference (index) -> submit_reads* (alignment + hit accumulation) -> stats ->
    pileup (consensus counts) -> hamming_le (allele match)."""

    def __init__(self, device: int = 0, params: MlstParams | None = None):
        self.lib = load_library()
        self.params = params or default_params()
        self._h = C.c_void_p()
        rc = self.lib.mlst_create(int(device), C.byref(self.params), C.byref(self._h))
        if rc != 0:
            msg = self.lib.mlst_last_error(None)
            raise MlstError("mlst_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.device = device
        self.depth_cap = 0
        self.index: AlleleIndex | None = None

    def close(self):
        if self._h:
            self.lib.mlst_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.mlst_last_error(self._h)
            text = msg.decode() if msg else "?"
            if rc == -1 and text.startswith("CRC mismatch in BGZF block"):      # MLST_E_INVALID with k_bgzf_crc's report (include/mlst.h)
                raise BgzfCrcMismatch("%s failed (%d): %s" % (what, rc, text), 1 if " of file 1 " in text else 2 if " of file 2 " in text else None)
            if rc == -1 and text.startswith("host path needed"):
                raise HostPathNeeded("%s: %s" % (what, text))
            raise MlstError("%s failed (%d): %s" % (what, rc, text))

    # ---- reference ----
    def load_reference(self, index: AlleleIndex, cache_path: str | None = None):
        """cache_path: where the built host index is kept between runs (mlst_set_reference_cache: `<database>.mlstref` next to the
        database, as the reference keeps `<idx>.1.bt2`, metamlst-index.py:224-225); None leaves the process-wide setting alone."""
        self.index = index
        if cache_path is not None:
            self.lib.mlst_set_reference_cache(cache_path.encode() if cache_path else None)
        self._check(self.lib.mlst_load_reference(self._h, _ptr(index.ascii_concat), _ptr(index.off), _ptr(index.locus_id),
                                                 _ptr(index.species_id), _ptr(index.allele_no), index.n_alleles),
                    "mlst_load_reference")

    # ---- pass 1 ----
    def submit_reads(self, bases: np.ndarray, quals: np.ndarray, off: np.ndarray, paired: bool = False):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        self._check(self.lib.mlst_submit_reads(self._h, _ptr(bases), _ptr(quals), _ptr(off), len(off) - 1, int(paired)),
                    "mlst_submit_reads")

    def submit_fastq(self, text, paired: bool = False) -> int:
        """Pass 1 straight from FASTQ text (bytes / bytearray / uint8 array holding whole 4-line records); parsed on the GPU."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_fastq(self._h, _ptr(buf) if buf.size else None, buf.size, int(paired), C.byref(n)), "mlst_submit_fastq")
        return int(n.value)

    def submit_fasta(self, text, read_len: int = 150, stride: int = 25, min_len: int = 50) -> tuple[int, int]:
        """Pass 1 from FASTA text that holds whole contigs (bytes / bytearray / uint8 array): cut into the reads of
        fastq.tile_fasta and packed on the GPU (mlst_submit_fasta; the rules: include/mlst.h).  Returns (contigs, reads).
        HostPathNeeded: a sequence line with white space inside or a CR without its LF; nothing of the call was submitted."""
        for v in (read_len, stride, min_len):
            if not 0 <= int(v) < (1 << 32):
                raise ValueError("read_len, stride and min_len are unsigned 32-bit numbers")
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        nc, nr = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_submit_fasta(self._h, _ptr(buf) if buf.size else None, buf.size, int(read_len), int(stride), int(min_len),
                                               C.byref(nc), C.byref(nr)), "mlst_submit_fasta")
        return int(nc.value), int(nr.value)

    def submit_fasta_file(self, path: str, read_len: int = 150, stride: int = 25, min_len: int = 50, chunk_bytes: int = 64 << 20) -> tuple[int, int]:
        """submit_fasta over a FASTA file in whole-contig chunks (fastq.fasta_chunks: plain files through pooled read buffers; .gz
        and bgzip'd files are inflated on the host -- a compressed genome is a few dozen BGZF blocks).  Returns (contigs, reads).
        After HostPathNeeded the chunks before the refused one have been submitted: reset_sample() before the host path."""
        from .fastq import fasta_chunks, prefetch, release_buffers
        ring: list = []
        nc = nr = 0
        try:
            for chunk in prefetch(fasta_chunks(path, chunk_bytes, reuse=True, ring=ring)):
                c, r = self.submit_fasta(chunk, read_len, stride, min_len)      # (returns when the chunk has left the host buffer)
                nc += c
                nr += r
        finally:
            release_buffers(ring)
        return nc, nr

    def submit_fastq_bgzf(self, data, final: bool, paired: bool = False) -> int:
        """Pass 1 from BGZF-compressed FASTQ: a run of whole BGZF blocks (fastq.bgzf_chunks), inflated and parsed on the GPU.
        final marks the last chunk of the file.  Returns the number of records completed by this chunk."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_fastq_bgzf(self._h, _ptr(buf) if buf.size else None, buf.size, int(final), int(paired), C.byref(n), None),
                    "mlst_submit_fastq_bgzf")
        return int(n.value)

    def _submit_bgzf_pieces(self, path: str, lo: int, hi: int, chunk_bytes: int, paired: bool, final_last: bool) -> int:
        """Compressed bytes [lo, hi) of a BGZF file (whole blocks from lo on) into mlst_submit_fastq_bgzf, piece by piece: a
        reader thread stays two pieces ahead (fastq.raw_chunks: positional reads of a few threads into pooled buffers), the
        library takes the whole blocks of a piece and says how many bytes that was, and the cut-off block is copied in front
        of the next piece (the buffers keep a margin for it).  Until round 4 every piece went through f.read() and
        `carry + block`: ~0.15 s of one host thread per 256 MB piece against ~0.04 s of GPU work."""
        from .fastq import prefetch, raw_chunks, release_buffers
        margin = 1 << 17
        total, carry = 0, None
        n, used = C.c_uint64(), C.c_uint64()
        ring: list = []
        at = lo
        if hi <= lo:
            self._check(self.lib.mlst_submit_fastq_bgzf(self._h, None, 0, int(final_last), int(paired), C.byref(n), None), "mlst_submit_fastq_bgzf")
            return int(n.value)
        for buf, got in prefetch(raw_chunks(path, chunk_bytes, lo, hi, margin, reuse=True, ring=ring)):
            at += got
            c = 0 if carry is None else carry.size
            if c > margin:
                raise MlstError("a BGZF block of more than %d bytes?" % margin)
            if c:
                buf[margin - c:margin] = carry
            view = buf[margin - c:margin + got]
            last = at >= hi
            self._check(self.lib.mlst_submit_fastq_bgzf(self._h, _ptr(view), view.size, int(last and final_last), int(paired),
                                                        C.byref(n), None if last else C.byref(used)), "mlst_submit_fastq_bgzf")
            total += int(n.value)
            carry = None if last else view[int(used.value):].copy()      # (a cut-off block: under 64 KB)
        release_buffers(ring)
        return total

    def submit_fastq_bgzf_file(self, path: str, paired: bool = False, chunk_bytes: int = (512 << 20) - (1 << 18)) -> int:
        """A whole bgzip'd FASTQ file (see _submit_bgzf_pieces).  Chunks of just under 512 MB compressed (~44 k BGZF blocks; with the
        reader's margin a chunk fills a 512 MB page-locked buffer, four of them per walk): one pass of the inflate kernels with
        three waves per CU (k_inflate_tok2 holds four: 65,536 blocks a turn), and the chunk behind it is copied and inflated
        meanwhile; the library cuts a first chunk's head and a last chunk's tail off as pieces of their own (mlst_submit_fastq_bgzf)."""
        return self._submit_bgzf_pieces(path, 0, os.path.getsize(path), chunk_bytes, paired, True)

    # ---- BGZF BAM (ready-made alignments) ----
    def bam_open(self, which: int, ref_allele, ref_locus, ref_flags, skip_bytes: int = 0, chosen=None) -> None:
        """Open a BAM stream (mlst_bam_open): which = 1 accumulates, 2 piles the records of `chosen` up; the three tables come
        from the BAM header (samin.bam_ref_table), skip_bytes from samin.read_bam_header."""
        ra, rl, rf = np.ascontiguousarray(ref_allele, np.int32), np.ascontiguousarray(ref_locus, np.int32), np.ascontiguousarray(ref_flags, np.uint8)
        ch = np.ascontiguousarray([] if chosen is None else chosen, np.uint32)
        self._check(self.lib.mlst_bam_open(self._h, int(which), _ptr(ra), _ptr(rl), _ptr(rf), ra.size, int(skip_bytes), _ptr(ch) if ch.size else None, ch.size),
                    "mlst_bam_open")

    def submit_bam_bgzf(self, data, final: bool, partial: bool = False):
        """One chunk of the open BAM stream: whole BGZF blocks (partial: the buffer may end inside one).  Returns (records
        completed by the call, bytes taken)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n, used = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_submit_bam_bgzf(self._h, _ptr(buf) if buf.size else None, buf.size, int(final), C.byref(n), C.byref(used) if partial else None),
                    "mlst_submit_bam_bgzf")
        return int(n.value), int(used.value) if partial else buf.size

    def _bam_stream_file(self, path: str, lo: int, chunk_bytes: int) -> int:
        """Compressed bytes [lo, end) of a BAM into the open stream, piece by piece (the reader ring of _submit_bgzf_pieces)."""
        from .fastq import prefetch, raw_chunks, release_buffers
        margin, hi = 1 << 17, os.path.getsize(path)
        total, carry, at = 0, None, lo
        n, used = C.c_uint64(), C.c_uint64()
        if hi <= lo:
            self._check(self.lib.mlst_submit_bam_bgzf(self._h, None, 0, 1, C.byref(n), None), "mlst_submit_bam_bgzf")
            return int(n.value)
        ring: list = []
        try:
            for buf, got in prefetch(raw_chunks(path, chunk_bytes, lo, hi, margin, reuse=True, ring=ring)):
                at += got
                c = 0 if carry is None else carry.size
                if c > margin:
                    raise MlstError("a BGZF block of more than %d bytes?" % margin)
                if c:
                    buf[margin - c:margin] = carry
                view = buf[margin - c:margin + got]
                last = at >= hi
                self._check(self.lib.mlst_submit_bam_bgzf(self._h, _ptr(view), view.size, int(last), C.byref(n), None if last else C.byref(used)),
                            "mlst_submit_bam_bgzf")
                total += int(n.value)
                carry = None if last else view[int(used.value):].copy()
        finally:
            release_buffers(ring)
        return total

    def submit_bam_file(self, path: str, species_filter: str | None = None, chunk_bytes: int = 64 << 20) -> int:
        """Pass 1 over a BGZF BAM (hit accumulation, metamlst.py:101-130) on the device; returns the number of records.  The
        statistics are the engine's (stats(), typing_*).  HostPathNeeded: a record only the host reader treats.  With set_bgzf_verify
        on, the blocks of the header are checked on the host (fastq.BgzfCrcError), those of the records on the device."""
        from .samin import bam_ref_table, read_bam_header
        names, lo, skip = read_bam_header(path, self.bgzf_verify)      # (the header's blocks are the host's to check)
        self.bam_open(1, *bam_ref_table(self.index, names, species_filter), skip_bytes=skip)
        return self._bam_stream_file(path, lo, chunk_bytes)

    def pileup_bam_file(self, path: str, chosen, chunk_bytes: int = 64 << 20) -> dict[int, np.ndarray]:
        """Pass 2 over a BGZF BAM: {allele idx: uint32[len, 4]} of the chosen contigs, counted on the device from the records in
        place (true AS / XM by name, the engine's minscore / max_xm / minqual)."""
        from .samin import bam_ref_table, read_bam_header
        names, lo, skip = read_bam_header(path, self.bgzf_verify)      # (the header's blocks are the host's to check)
        ch = np.ascontiguousarray(chosen, np.uint32)
        self.bam_open(2, *bam_ref_table(self.index, names, None), skip_bytes=skip, chosen=ch)
        self._bam_stream_file(path, lo, chunk_bytes)
        lens = [int(self.index.off[a + 1] - self.index.off[a]) for a in ch]
        counts = np.zeros((max(1, sum(lens)), 4), np.uint32)
        self._check(self.lib.mlst_bam_pileup_fetch(self._h, _ptr(counts)), "mlst_bam_pileup_fetch")
        out, at = {}, 0
        for a, L in zip(ch, lens):
            out[int(a)] = counts[at:at + L]
            at += L
        return out

    # ---- SAM text (ready-made alignments) ----
    def sam_open(self, which: int, names, ref_allele, ref_locus, ref_flags, chosen=None) -> None:
        """Open a stream of SAM text (mlst_sam_open): which = 1 accumulates, 2 piles the records of `chosen` up; names are the
        SN: names of the file's @SQ lines (samin.read_sam_header), the three tables samin.bam_ref_table's for them."""
        enc = [n.encode("utf-8", "surrogateescape") if isinstance(n, str) else bytes(n) for n in names]
        off = np.zeros(len(enc) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in enc], dtype=np.uint64)
        arena = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        ra, rl, rf = np.ascontiguousarray(ref_allele, np.int32), np.ascontiguousarray(ref_locus, np.int32), np.ascontiguousarray(ref_flags, np.uint8)
        if not ra.size == rl.size == rf.size == len(enc):
            raise ValueError("one (allele, locus, flags) triple per name")
        ch = np.ascontiguousarray([] if chosen is None else chosen, np.uint32)
        self._check(self.lib.mlst_sam_open(self._h, int(which), _ptr(arena), _ptr(off), _ptr(ra), _ptr(rl), _ptr(rf), len(enc),
                                           _ptr(ch) if ch.size else None, ch.size), "mlst_sam_open")

    def submit_sam_text(self, text, final: bool) -> int:
        """One chunk of the open SAM stream (bytes / bytearray / uint8 array), cut anywhere; returns the record lines it completed."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_sam_text(self._h, _ptr(buf) if buf.size else None, buf.size, int(final), C.byref(n)), "mlst_submit_sam_text")
        return int(n.value)

    def _sam_stream_file(self, path: str, chunk_bytes: int) -> int:
        """The bytes of a SAM file into the open stream, chunk by chunk: a plain file through the reader ring and the pooled
        (page-locked) buffers of _bam_stream_file; a gzip file (plain or bgzip'd) inflated by the host's gzip, a chunk ahead."""
        from .fastq import prefetch, raw_chunks, release_buffers
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        chunk_bytes = min(int(chunk_bytes), (1 << 30) - 1)
        with open(path, "rb") as f:
            zipped = f.read(2) == b"\x1f\x8b"
        total = 0
        if zipped:
            import gzip

            def pieces():
                with gzip.open(path, "rb") as z:
                    while True:
                        piece = z.read(chunk_bytes)
                        if not piece:
                            return
                        yield piece
            for piece in prefetch(pieces()):
                total += self.submit_sam_text(piece, False)
            return total + self.submit_sam_text(b"", True)
        size = os.path.getsize(path)
        if size == 0:
            return self.submit_sam_text(b"", True)
        ring: list = []
        at = 0
        try:
            for buf, got in prefetch(raw_chunks(path, chunk_bytes, 0, size, 0, reuse=True, ring=ring)):
                at += got
                total += self.submit_sam_text(buf[:got], at >= size)      # (returns when the chunk has left the host buffer)
        finally:
            release_buffers(ring)
        return total

    def submit_sam_file(self, path: str, species_filter: str | None = None, chunk_bytes: int = 64 << 20) -> int:
        """Pass 1 over SAM text, plain or .gz (hit accumulation, metamlst.py:101-130), parsed on the device; returns the number of
        records.  The statistics are the engine's (stats(), typing_*).  HostPathNeeded: a line only the host reader treats."""
        from .samin import bam_ref_table, read_sam_header
        names = read_sam_header(path)
        self.sam_open(1, names, *bam_ref_table(self.index, names, species_filter))
        return self._sam_stream_file(path, chunk_bytes)

    def pileup_sam_file(self, path: str, chosen, chunk_bytes: int = 64 << 20) -> dict[int, np.ndarray]:
        """Pass 2 over SAM text: {allele idx: uint32[len, 4]} of the chosen contigs, counted on the device from the lines in
        place (true AS / XM by name, the engine's minscore / max_xm / minqual)."""
        from .samin import bam_ref_table, read_sam_header
        names = read_sam_header(path)
        ch = np.ascontiguousarray(chosen, np.uint32)
        self.sam_open(2, names, *bam_ref_table(self.index, names, None), chosen=ch)
        self._sam_stream_file(path, chunk_bytes)
        lens = [int(self.index.off[a + 1] - self.index.off[a]) for a in ch]
        counts = np.zeros((max(1, sum(lens)), 4), np.uint32)
        self._check(self.lib.mlst_bam_pileup_fetch(self._h, _ptr(counts)), "mlst_bam_pileup_fetch")
        out, at = {}, 0
        for a, L in zip(ch, lens):
            out[int(a)] = counts[at:at + L]
            at += L
        return out

    # ---- BGZF BAM (its records taken as reads) ----
    def bam_reads_open(self, n_ref: int, skip_bytes: int = 0, paired: bool = False) -> None:
        """Open a reads stream (mlst_bam_reads_open); the data follows through submit_bam_bgzf."""
        self._check(self.lib.mlst_bam_reads_open(self._h, int(n_ref), int(skip_bytes), int(paired)), "mlst_bam_reads_open")

    def submit_bam_reads_file(self, path: str, paired: bool = False, chunk_bytes: int = 64 << 20) -> int:
        """Pass 1 over the READS of a BGZF BAM (the rules of `samtools fastq`, include/mlst.h): inflated, chosen, strand-corrected
        and packed on the device; returns the reads submitted (bam_reads_info() has the records skipped).  paired: the reads kept
        come as neighbours with one QNAME and are submitted as pairs.  With set_read_tiling on and paired False, a read longer
        than the tile is cut into windows on the device (the rule: samin.bam_reads_fastq, then fastq.tile_fastq); the count
        returned is then windows plus uncut reads, read_tiling_info() has the reads cut.  With set_bgzf_verify on, the blocks of the header are
        checked on the host (fastq.BgzfCrcError), those of the records on the device."""
        from .samin import read_bam_header
        names, lo, skip = read_bam_header(path, self.bgzf_verify)      # (the header's blocks are the host's to check)
        self.bam_reads_open(len(names), skip, paired)
        self._bam_stream_file(path, lo, chunk_bytes)
        return self.bam_reads_info()[0]

    def bam_reads_info(self) -> tuple[int, int, int, int]:
        """(reads submitted, records skipped as secondary / supplementary, skipped as empty, cells of the record split walked
        again) of the reads stream just finished or still open (mlst_bam_reads_info)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_bam_reads_info(self._h, out), "mlst_bam_reads_info")
        return tuple(int(x) for x in out)

    def debug_last_packed(self):
        """Test hook (mlst_debug_last_packed): (packed, qrows, lens, words_per_read, qual_stride) of the last submission made from
        FASTQ text, from the reads of a BAM or from tiled contigs, copied from the device."""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.mlst_debug_last_packed(self._h, None, 0, None, 0, None, 0, out), "mlst_debug_last_packed")
        n, wpr, qs = (int(x) for x in out)
        packed = np.zeros(((n + 63) // 64) * 64 * wpr, np.uint32); qrows = np.zeros((n, qs), np.uint8); lens = np.zeros(n, np.uint16)
        if n:
            self._check(self.lib.mlst_debug_last_packed(self._h, _ptr(packed), packed.size, _ptr(qrows), qrows.size, _ptr(lens), lens.size, out),
                        "mlst_debug_last_packed")
        return packed, qrows, lens, wpr, qs

    def fasta_info(self) -> tuple[int, int, int, int]:
        """Test hook (mlst_debug_fasta_info): (cells, contigs, entries of the contig tables, passes over them: 1 or 2) of the last
        submit_fasta call that reached the device."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_debug_fasta_info(self._h, out), "mlst_debug_fasta_info")
        return tuple(int(x) for x in out)

    def bam_set_capacity(self, max_entries: int) -> None:
        self._check(self.lib.mlst_bam_set_capacity(self._h, int(max_entries)), "mlst_bam_set_capacity")

    def debug_bam_split(self, force_miss_every: int = 0) -> int:
        """Test hook (mlst_debug_bam_split): returns the cells the last BAM stream walked again."""
        n = C.c_uint64()
        self._check(self.lib.mlst_debug_bam_split(self._h, int(force_miss_every), C.byref(n)), "mlst_debug_bam_split")
        return int(n.value)

    def submit_fastq_bgzf_pair(self, data1, data2, final: bool) -> int:
        """Pass 1 from the two bgzip'd files of a paired-end sample: whole BGZF blocks of file 1 and of file 2 (any number of
        records of either), inflated and paired on the GPU (record k of one file is the mate of record k of the other, across
        calls).  final marks the last call.  Returns the number of reads completed by this call (2 x pairs)."""
        b1 = np.frombuffer(data1, dtype=np.uint8) if not isinstance(data1, np.ndarray) else np.ascontiguousarray(data1, np.uint8)
        b2 = np.frombuffer(data2, dtype=np.uint8) if not isinstance(data2, np.ndarray) else np.ascontiguousarray(data2, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_fastq_bgzf_pair(self._h, _ptr(b1) if b1.size else None, b1.size, _ptr(b2) if b2.size else None, b2.size,
                                                         int(final), C.byref(n), None, None), "mlst_submit_fastq_bgzf_pair")
        return int(n.value)

    def submit_fastq_bgzf_pair_files(self, path1: str, path2: str, chunk_bytes: int = (512 << 20) - (1 << 18)) -> int:
        """Two bgzip'd mate files (mlst_submit_fastq_bgzf_pair), read as _submit_bgzf_pieces reads one: a reader thread stays two
        calls ahead (fastq.raw_chunks into pooled page-locked buffers), and each file's cut-off block goes in front of its next
        piece.  A call takes about chunk_bytes compressed bytes of the two files together, the same fraction of each file's
        size, so that the records one file is ahead by -- which wait on the device for their mates -- stay few even when the
        two files compress differently.  The first call takes a quarter of that: its inflate has nothing to hide behind."""
        from .fastq import prefetch, raw_chunks, release_buffers
        margin = 1 << 17
        s1, s2 = os.path.getsize(path1), os.path.getsize(path2)
        n, used1, used2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if s1 + s2 == 0:
            self._check(self.lib.mlst_submit_fastq_bgzf_pair(self._h, None, 0, None, 0, 1, C.byref(n), None, None), "mlst_submit_fastq_bgzf_pair")
            return int(n.value)
        cuts = pair_file_cuts(s1, s2, chunk_bytes)
        ring1: list = []
        ring2: list = []

        def span(path, lo, hi, ring):
            for buf, got in raw_chunks(path, hi - lo, lo, hi, margin, reuse=True, ring=ring):      # (one piece: [lo, hi))
                return buf, got
            return None, 0

        def pieces():
            for a1, b1, a2, b2 in cuts:
                yield span(path1, a1, b1, ring1), span(path2, a2, b2, ring2)

        total = 0
        carry = [None, None]
        for k, (p1, p2) in enumerate(prefetch(pieces())):
            last = k == len(cuts) - 1
            views = []
            for f, (buf, got) in enumerate((p1, p2)):
                c = 0 if carry[f] is None else carry[f].size
                if c > margin:
                    raise MlstError("a BGZF block of more than %d bytes?" % margin)
                if buf is None:
                    views.append(carry[f] if c else np.empty(0, np.uint8))
                    continue
                if c:
                    buf[margin - c:margin] = carry[f]
                views.append(buf[margin - c:margin + got])
            v1, v2 = views
            self._check(self.lib.mlst_submit_fastq_bgzf_pair(self._h, _ptr(v1) if v1.size else None, v1.size, _ptr(v2) if v2.size else None, v2.size,
                                                             int(last), C.byref(n), None if last else C.byref(used1), None if last else C.byref(used2)),
                        "mlst_submit_fastq_bgzf_pair")
            total += int(n.value)
            if not last:
                carry = [v1[int(used1.value):].copy(), v2[int(used2.value):].copy()]      # (cut-off blocks: under 64 KB each)
        release_buffers(ring1)
        release_buffers(ring2)
        return total

    def inflate_bgzf(self, data) -> bytes:
        """Test hook: whole BGZF blocks -> their text, inflated by the device kernel."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        room, off = 0, 0                             # the blocks' ISIZE fields added up; anything odd: the format's bound (the library checks)
        while off + 18 <= buf.size:
            size = int(buf[off + 16]) + (int(buf[off + 17]) << 8) + 1
            plain = buf[off:off + 16].tobytes() == b"\x1f\x8b\x08\x04" + buf[off + 4:off + 10].tobytes() + b"\x06\x00BC\x02\x00"      # (XLEN = 6: the BC subfield alone)
            if not plain or size < 26 or off + size > buf.size:
                room = (buf.size // 18 + 1) * 65536
                break
            room += min(int.from_bytes(buf[off + size - 4:off + size].tobytes(), "little"), 65536)
            off += size
        if off != buf.size:
            room = (buf.size // 18 + 1) * 65536
        out = np.empty(max(1, room), np.uint8)
        n, ms = C.c_uint64(), C.c_double()
        self._check(self.lib.mlst_selftest_inflate_device(self._h, _ptr(buf), buf.size, _ptr(out), out.size, C.byref(n), C.byref(ms)), "mlst_selftest_inflate_device")
        self.last_inflate_ms = float(ms.value)
        return out[:int(n.value)].tobytes()

    def inflate_paths(self):
        """Test hook (mlst_debug_inflate_paths): (BGZF blocks with data of the last inflate_bgzf call, how many of them phase 1 of
        the two-kernel inflate left to k_inflate)."""
        n, left = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_debug_inflate_paths(self._h, C.byref(n), C.byref(left)), "mlst_debug_inflate_paths")
        return int(n.value), int(left.value)

    def bgzf_block_crcs(self, data) -> np.ndarray:
        """Test hook: whole BGZF blocks -> the CRC-32 the device computes of every block with data (uint32, file order), whatever
        the trailers say.  last_crc_ms: the CRC kernel alone."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        out = np.zeros(max(1, buf.size // 26 + 1), np.uint32)      # (a block is at least 26 bytes)
        n, ms = C.c_uint64(), C.c_double()
        self._check(self.lib.mlst_selftest_bgzf_crc(self._h, _ptr(buf), buf.size, _ptr(out), out.size, C.byref(n), C.byref(ms)), "mlst_selftest_bgzf_crc")
        self.last_crc_ms = float(ms.value)
        return out[:int(n.value)].copy()

    def set_bgzf_verify(self, on: bool) -> None:
        """Check the CRC-32 of every BGZF block on the GPU before its reads are typed (mlst_set_bgzf_verify; off by default,
        MLST_BGZF_CRC=1 switches it on for new engines).  Only while no stream is open."""
        self._check(self.lib.mlst_set_bgzf_verify(self._h, int(bool(on))), "mlst_set_bgzf_verify")

    def set_read_tiling(self, read_len: int = 150, stride: int = 25) -> None:
        """Cut FASTQ records and BAM reads longer than read_len bases into windows of read_len bases every stride bases on the GPU,
        each with its slice of the qualities (mlst_set_read_tiling; the rule: fastq.tile_fastq, for a BAM applied to the reads
        samin.bam_reads_fastq writes).  0, 0 = off, the default.  Unpaired submit_fastq / submit_fastq_stream / submit_fastq_bgzf
        and unpaired BAM reads streams (bam_reads_open, submit_bam_reads_file) only; may change only while no stream is open on
        the handle."""
        self._check(self.lib.mlst_set_read_tiling(self._h, int(read_len), int(stride)), "mlst_set_read_tiling")

    def get_read_tiling(self) -> tuple[int, int]:
        """(read_len, stride) of set_read_tiling; (0, 0) = off"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.mlst_get_read_tiling(self._h, C.byref(a), C.byref(b)), "mlst_get_read_tiling")
        return int(a.value), int(b.value)

    def read_tiling_info(self) -> dict:
        """Since the last reset_sample: records (FASTQ records, kept BAM reads) seen by tiled submissions, records cut, windows made of
        them, bases of the longest record"""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_get_read_tiling_info(self._h, out), "mlst_get_read_tiling_info")
        return {"records": int(out[0]), "cut": int(out[1]), "windows": int(out[2]), "longest": int(out[3])}

    def set_read_names(self, on: bool = True) -> None:
        """Keep the name of every retained read, copied out of the FASTQ text on the GPU (mlst_set_read_names; off by default; the
        rule: samout.read_qname).  export_sam_text / write_sam_all then write it as QNAME, read_names() gives samout.write_sam its
        map.  FASTQ text and BGZF entries only -- every other way of adding reads is refused while it is on; may change only while
        the sample holds no reads and no stream is open.  reset_sample empties the names and keeps the switch."""
        self._check(self.lib.mlst_set_read_names(self._h, int(bool(on))), "mlst_set_read_names")

    def get_read_names(self) -> bool:
        on = C.c_int()
        self._check(self.lib.mlst_get_read_names(self._h, C.byref(on)), "mlst_get_read_names")
        return bool(on.value)

    def read_names_info(self) -> dict:
        """Since the last reset_sample: retained reads with a kept name, the bytes of those names, retained reads whose name is no
        legal QNAME (they keep r<k>), the longest kept name.  All zero with the switch off."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_read_names_info(self._h, out), "mlst_read_names_info")
        return {"named": int(out[0]), "bytes": int(out[1]), "fallbacks": int(out[2]), "longest": int(out[3])}

    def read_names(self) -> dict:
        """{read index: name (bytes)} of the retained reads with a kept name (mlst_read_names_fetch)"""
        info = self.read_names_info()
        n = info["named"]
        ridx = np.zeros(max(n, 1), np.uint64); off = np.zeros(n + 1, np.uint64); data = np.zeros(max(info["bytes"], 1), np.uint8)
        self._check(self.lib.mlst_read_names_fetch(self._h, ridx.ctypes.data_as(C.POINTER(C.c_uint64)), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   data.ctypes.data_as(C.POINTER(C.c_uint8))), "mlst_read_names_fetch")
        raw = data.tobytes()
        return {int(ridx[i]): raw[int(off[i]):int(off[i + 1])] for i in range(n)}

    def set_read_prep(self, trim5: int = 0, trim3: int = 0, trim_qual: int = 0, phred64: bool = False) -> None:
        """Prepare every read of FASTQ text on the GPU before it is packed (mlst_set_read_prep; off by default; the rule:
        fastq.prep_fastq): Phred base 64, bowtie2's fixed trims -5 / -3, then a 3' quality trim (cutadapt -q).  The engine then behaves
        as if it had been given prep_fastq's text.  FASTQ text and BGZF entries only -- every other way of adding reads is refused
        while it is on; may change only while the sample holds no reads and no stream is open.  All defaults: off."""
        for v in (trim5, trim3, trim_qual):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("set_read_prep: %r is no unsigned 32-bit value" % (v,))
        p = (C.c_uint32 * 4)(int(trim5), int(trim3), int(trim_qual), 64 if phred64 else 33)
        self._check(self.lib.mlst_set_read_prep(self._h, p), "mlst_set_read_prep")

    def get_read_prep(self) -> dict:
        p = (C.c_uint32 * 4)()
        self._check(self.lib.mlst_get_read_prep(self._h, p), "mlst_get_read_prep")
        return {"trim5": int(p[0]), "trim3": int(p[1]), "trim_qual": int(p[2]), "phred64": int(p[3]) == 64}

    def read_prep_info(self) -> dict:
        """Since the last reset_sample: reads whose length changed, bases removed, reads of length >= 1 left without a base.  All zero
        with the switch off."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_read_prep_info(self._h, out), "mlst_read_prep_info")
        return {"shortened": int(out[0]), "bases_removed": int(out[1]), "emptied": int(out[2])}

    def set_read_adapters(self, adapters=None, min_overlap: int = 3, error_permille: int = 100) -> None:
        """Remove a 3' adapter from every read of FASTQ text on the GPU before it is packed (mlst_set_read_adapters; off by default;
        the rule: fastq.adapter_cut, modelled on `cutadapt -a ADAPTER --no-indels`), behind set_read_prep's steps.  The engine then
        behaves as if it had been given fastq.trim_adapters' text.  adapters: one str / bytes with commas between the adapters or a
        sequence of them (1 to 8, 1 to 64 letters of ACGTN each); None, "" or an empty sequence: off.  FASTQ text and BGZF entries only
        -- every other way of adding reads is refused while it is on; may change only while the sample holds no reads and no stream is
        open."""
        if adapters is not None and not isinstance(adapters, (str, bytes, bytearray)):
            adapters = b",".join(a.encode() if isinstance(a, str) else bytes(a) for a in adapters)
        if isinstance(adapters, str):
            adapters = adapters.encode()
        for v in (min_overlap, error_permille):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("set_read_adapters: %r is no unsigned 32-bit value" % (v,))
        if adapters and b"\0" in bytes(adapters):
            raise ValueError("set_read_adapters: a zero byte among the adapters")
        self._check(self.lib.mlst_set_read_adapters(self._h, bytes(adapters) if adapters else None, int(min_overlap), int(error_permille)), "mlst_set_read_adapters")

    def get_read_adapters(self) -> dict:
        """{"adapters": [upper-case str], "min_overlap", "error_permille"}; no adapters and 0, 0 with the switch off"""
        buf = C.create_string_buffer(8 * 65)
        mo, pm = C.c_uint32(), C.c_uint32()
        self._check(self.lib.mlst_get_read_adapters(self._h, buf, len(buf), C.byref(mo), C.byref(pm)), "mlst_get_read_adapters")
        text = buf.value.decode()
        return {"adapters": text.split(",") if text else [], "min_overlap": int(mo.value), "error_permille": int(pm.value)}

    def read_adapters_info(self) -> dict:
        """Since the last reset_sample: reads cut, bases removed, reads of length >= 1 cut at 0, reads cut per adapter.  All zero (and
        no adapter) with the switch off.  Separate from read_prep_info()."""
        out = (C.c_uint64 * 12)()
        self._check(self.lib.mlst_get_read_adapters_info(self._h, out), "mlst_get_read_adapters_info")
        return {"trimmed": int(out[0]), "bases_removed": int(out[1]), "emptied": int(out[2]), "per_adapter": [int(out[4 + k]) for k in range(int(out[3]))]}

    def set_read_stats(self, on: bool = True) -> None:
        """Count per-cycle quality and base tables of every read of FASTQ text on the GPU, next to the parser (mlst_set_read_stats; off
        by default; the rule: fastq.read_stats).  Typing is untouched.  FASTQ text and BGZF entries only -- every other way of adding
        reads is refused while it is on; may change only while the sample holds no reads and no stream is open."""
        self._check(self.lib.mlst_set_read_stats(self._h, 1 if on else 0), "mlst_set_read_stats")

    def get_read_stats(self) -> bool:
        on = C.c_int()
        self._check(self.lib.mlst_get_read_stats(self._h, C.byref(on)), "mlst_get_read_stats")
        return bool(on.value)

    def set_read_stats_side(self, side: int) -> None:
        """The side (0 or 1) unpaired submissions count into from here on (mlst_set_read_stats_side): 1 in front of a mate file that
        goes in as unpaired text.  Refused while a stream is open; 0 again behind reset_sample."""
        self._check(self.lib.mlst_set_read_stats_side(self._h, int(side)), "mlst_set_read_stats_side")

    def read_stats(self) -> dict:
        """{"raw": [side 0, side 1], "prepared": [side 0, side 1]}: the tables since the last reset_sample as dicts shaped as
        fastq.read_stats': reads, bases, clamped_low (int), len_hist (321), base (320 x 5), qual (320 x 94), gc_hist (101),
        readqual_hist (94) as numpy int64.  With neither a trim nor an adapter set "prepared" is the raw block.  All zero with the
        switch off."""
        from .fastq import RS_BASE, RS_GC, RS_LEN, RS_QUAL, RS_READQUAL, RS_WORDS
        out = {}
        for stage, name in enumerate(("raw", "prepared")):
            out[name] = []
            for side in (0, 1):
                w = np.zeros(RS_WORDS, np.uint64)
                self._check(self.lib.mlst_read_stats_fetch(self._h, stage, side, w.ctypes.data_as(C.POINTER(C.c_uint64)), RS_WORDS), "mlst_read_stats_fetch")
                w = w.astype(np.int64)
                out[name].append({"reads": int(w[0]), "bases": int(w[1]), "clamped_low": int(w[2]), "len_hist": w[RS_LEN:RS_BASE].copy(),
                                  "base": w[RS_BASE:RS_QUAL].reshape(320, 5).copy(), "qual": w[RS_QUAL:RS_GC].reshape(320, 94).copy(),
                                  "gc_hist": w[RS_GC:RS_READQUAL].copy(), "readqual_hist": w[RS_READQUAL:RS_WORDS].copy()})
        out["phred_base"] = 64 if self.get_read_prep()["phred64"] else 33      # (what fastq.read_stats_text and fastq.phred_hint ask for)
        out["prepared_counted"] = self.read_stats_info()["prepared_launches"] > 0
        return out

    def read_stats_info(self) -> dict:
        """Launches of the counting kernel per stage since the last reset_sample and the bytes of the tables on the device; all zero
        with the switch off (nothing is queued or allocated)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_read_stats_info(self._h, out), "mlst_read_stats_info")
        return {"raw_launches": int(out[0]), "prepared_launches": int(out[1]), "table_bytes": int(out[2])}

    def set_read_dedup(self, on: bool = True) -> None:
        """Empty every read (in a paired submission: every pair) of FASTQ text that repeats an earlier one of the sample, on the GPU
        before it is packed (mlst_set_read_dedup; off by default; the rule: fastq.dedup_fastq), behind set_read_prep's steps and
        set_read_adapters' cut.  The engine then behaves as if it had been given the deduplicated text.  FASTQ text and BGZF entries
        only -- every other way of adding reads is refused while it is on; may change only while the sample holds no reads and no
        stream is open.  reset_sample empties the table of keys and keeps the switch."""
        self._check(self.lib.mlst_set_read_dedup(self._h, 1 if on else 0), "mlst_set_read_dedup")

    def get_read_dedup(self) -> bool:
        on = C.c_int()
        self._check(self.lib.mlst_get_read_dedup(self._h, C.byref(on)), "mlst_get_read_dedup")
        return bool(on.value)

    def read_dedup_info(self) -> dict:
        """Since the last reset_sample, fastq.dedup_fastq's counters -- reads, units (reads or pairs that took part), duplicates,
        reads_removed, bases_removed, distinct, levels (eight: keys that occur 1, 2, 3, 4, 5-9, 10-49, 50-499, >= 500 times) -- and
        clashes (units kept because only the first 64 bits of their key met another's) and slots (of the table on the device).  All
        zero with the switch off."""
        out = (C.c_uint64 * 16)()
        self._check(self.lib.mlst_read_dedup_info(self._h, out), "mlst_read_dedup_info")
        return {"reads": int(out[0]), "units": int(out[1]), "duplicates": int(out[2]), "reads_removed": int(out[3]), "bases_removed": int(out[4]),
                "distinct": int(out[5]), "clashes": int(out[6]), "slots": int(out[7]), "levels": [int(out[8 + k]) for k in range(8)]}

    def set_read_pair_overlap(self, on: bool = True, min_overlap: int = 30, max_mismatches: int = 5, error_permille: int = 200) -> None:
        """Cut adapter read-through from both mates of every pair of FASTQ text where the overlap of the mates says the insert ends, on
        the GPU before the reads are packed (mlst_set_read_pair_overlap; off by default; the rule: fastq.pair_overlap /
        fastq.trim_pair_overlap), behind set_read_prep's steps and set_read_adapters' cut, in front of set_read_dedup.  The engine then
        behaves as if it had been given the cut text.  Paired FASTQ text and BGZF entries only -- every other way of adding reads is
        refused while it is on; may change only while the sample holds no reads and no stream is open.  reset_sample zeroes the
        counters and keeps the switch."""
        self._check(self.lib.mlst_set_read_pair_overlap(self._h, 1 if on else 0, int(min_overlap), int(max_mismatches), int(error_permille)), "mlst_set_read_pair_overlap")

    def get_read_pair_overlap(self) -> dict:
        on, mo, mm, pm = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.mlst_get_read_pair_overlap(self._h, C.byref(on), C.byref(mo), C.byref(mm), C.byref(pm)), "mlst_get_read_pair_overlap")
        return {"on": bool(on.value), "min_overlap": int(mo.value), "max_mismatches": int(mm.value), "error_permille": int(pm.value)}

    def read_pair_overlap_info(self) -> dict:
        """Since the last reset_sample, fastq.trim_pair_overlap's counters -- pairs, overlapping, trimmed_pairs, reads_trimmed,
        bases_removed, emptied -- and insert_hist (1,024 bins: the fragment length of every overlapping pair in the file's
        coordinates, the last bin holding the longer ones).  All zero with the switch off."""
        out = (C.c_uint64 * 8)()
        self._check(self.lib.mlst_read_pair_overlap_info(self._h, out), "mlst_read_pair_overlap_info")
        hist = (C.c_uint64 * 1024)()
        self._check(self.lib.mlst_read_pair_overlap_hist(self._h, hist, 1024), "mlst_read_pair_overlap_hist")
        return {"pairs": int(out[0]), "overlapping": int(out[1]), "trimmed_pairs": int(out[2]), "reads_trimmed": int(out[3]), "bases_removed": int(out[4]),
                "emptied": int(out[5]), "insert_hist": [int(v) for v in hist]}

    def set_read_filter(self, poly="", poly_min: int = 10, min_length: int = 0, max_n=None, complexity: int = 0, mean_qual: int = 0) -> None:
        """Trim poly-G / poly-X tails from the 3' end of every read of FASTQ text and empty the reads that fail a filter, on the GPU before
        the reads are packed (mlst_set_read_filter; off by default; the rule: fastq.poly_tail / fastq.read_fails / fastq.filter_fastq,
        modelled on fastp), behind set_read_prep's steps, set_read_adapters' cut and set_read_pair_overlap's, in front of set_read_dedup.
        The engine then behaves as if it had been given filter_fastq's text.  poly: the tail letters ("G": two-colour chemistry; "ACGT":
        every letter; "": no tail trim), poly_min: the shortest tail; min_length, max_n (None: no limit), complexity (percent of
        neighbouring bases that differ), mean_qual: the filters, 0 / None = off.  FASTQ text and BGZF entries only -- every other way of
        adding reads is refused while it is on; may change only while the sample holds no reads and no stream is open.  All defaults: off."""
        letters = (poly.encode() if isinstance(poly, str) else bytes(poly)).upper()
        if letters.strip(b"ACGT"):
            raise ValueError("set_read_filter: tail letters %r: only A, C, G and T are taken" % letters.decode("latin-1"))
        vals = [sum(1 << b"ACGT".index(c) for c in set(letters)), poly_min, min_length, 0xFFFFFFFF if max_n is None else max_n, complexity, mean_qual]
        for v in vals:
            if int(v) != v or not 0 <= int(v) < 1 << 32:
                raise ValueError("set_read_filter: %r is no unsigned 32-bit value" % (v,))
        if max_n is not None and int(max_n) == 0xFFFFFFFF:
            raise ValueError("set_read_filter: max_n %r stands for no limit: give None" % (max_n,))
        self._check(self.lib.mlst_set_read_filter(self._h, (C.c_uint32 * 6)(*[int(v) for v in vals])), "mlst_set_read_filter")

    def get_read_filter(self) -> dict:
        """{"poly": the tail letters, "poly_min", "min_length", "max_n" (None: no limit), "complexity", "mean_qual"}"""
        p = (C.c_uint32 * 6)()
        self._check(self.lib.mlst_get_read_filter(self._h, p), "mlst_get_read_filter")
        return {"poly": "".join(c for k, c in enumerate("ACGT") if (int(p[0]) >> k) & 1), "poly_min": int(p[1]), "min_length": int(p[2]),
                "max_n": None if int(p[3]) == 0xFFFFFFFF else int(p[3]), "complexity": int(p[4]), "mean_qual": int(p[5])}

    def read_filter_info(self) -> dict:
        """Since the last reset_sample, fastq.filter_fastq's counters: tail_trimmed, tail_bases, per_letter (A, C, G, T), tail_emptied,
        failed_short, failed_n, failed_complexity, failed_quality, filtered_bases.  All zero with the switch off."""
        out = (C.c_uint64 * 16)()
        self._check(self.lib.mlst_read_filter_info(self._h, out), "mlst_read_filter_info")
        return {"tail_trimmed": int(out[0]), "tail_bases": int(out[1]), "per_letter": [int(out[2 + k]) for k in range(4)], "tail_emptied": int(out[6]),
                "failed_short": int(out[7]), "failed_n": int(out[8]), "failed_complexity": int(out[9]), "failed_quality": int(out[10]),
                "filtered_bases": int(out[11])}

    def set_read_window(self, front=None, right=None, tail=None) -> None:
        """Cut every read of FASTQ text by sliding-window mean quality on the GPU before the reads are packed (mlst_set_read_window; off by
        default; the rule: fastq.window_cut / fastq.cut_windows, modelled on fastp's cut_front / cut_right / cut_tail), directly behind
        set_read_prep's steps and in front of set_read_adapters' cut.  The engine then behaves as if it had been given cut_windows' text.
        Each operation is (W, Q) -- a window of 1..320 values whose mean must reach Q, 1..93 -- or None = off: front drops bases from the
        5' end up to the first passing window, right cuts at the first failing window behind that (its leading bases >= Q stay), tail
        drops bases from the 3' end down to the last passing window.  W = 1 is Trimmomatic's LEADING / TRAILING, right=(4, 15) its
        SLIDINGWINDOW:4:15.  A front cut is refused together with set_read_pair_overlap.  FASTQ text and BGZF entries only -- every other
        way of adding reads is refused while it is on; may change only while the sample holds no reads and no stream is open."""
        from .fastq import check_read_window
        try:
            vals = check_read_window(front, right, tail)
        except ValueError as e:
            raise ValueError("set_read_window: %s" % e) from None
        self._check(self.lib.mlst_set_read_window(self._h, (C.c_uint32 * 6)(*vals)), "mlst_set_read_window")

    def get_read_window(self) -> dict:
        """{"front", "right", "tail"}: each [W, Q], or None for an operation that is off"""
        p = (C.c_uint32 * 6)()
        self._check(self.lib.mlst_get_read_window(self._h, p), "mlst_get_read_window")
        return {name: [int(p[2 * k]), int(p[2 * k + 1])] if int(p[2 * k]) else None for k, name in enumerate(("front", "right", "tail"))}

    def read_window_info(self) -> dict:
        """Since the last reset_sample, fastq.cut_windows' counters: shortened, front_reads, front_bases, right_reads, right_bases,
        tail_reads, tail_bases, emptied.  All zero with the switch off."""
        from .fastq import WINDOW_COUNTERS
        out = (C.c_uint64 * 8)()
        self._check(self.lib.mlst_read_window_info(self._h, out), "mlst_read_window_info")
        return {name: int(out[k]) for k, name in enumerate(WINDOW_COUNTERS)}

    def set_export_md(self, on: bool = True) -> None:
        """export_sam_text / write_sam_all write bowtie2's MD:Z field between NM:i and YT:Z, formatted on the GPU (mlst_set_export_md; off
        by default; the rule: samout.md_text).  Read when an export is opened and refused while one is open; no part of the sample's
        state, so it may change at any other time."""
        self._check(self.lib.mlst_set_export_md(self._h, int(bool(on))), "mlst_set_export_md")

    def get_export_md(self) -> bool:
        on = C.c_int()
        self._check(self.lib.mlst_get_export_md(self._h, C.byref(on)), "mlst_get_export_md")
        return bool(on.value)

    @property
    def bgzf_verify(self) -> bool:
        on = C.c_int()
        self._check(self.lib.mlst_get_bgzf_verify(self._h, C.byref(on)), "mlst_get_bgzf_verify")
        return bool(on.value)

    @bgzf_verify.setter
    def bgzf_verify(self, on: bool) -> None:
        self.set_bgzf_verify(on)

    def submit_fastq_stream(self, text, final: bool, paired: bool = False) -> int:
        """One chunk of an open FASTQ stream (cut anywhere; a partial record at its end is completed by the next chunk, text or
        BGZF); final marks the last one.  Returns the number of records completed."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_fastq_stream(self._h, _ptr(buf) if buf.size else None, buf.size, int(final), int(paired), C.byref(n)),
                    "mlst_submit_fastq_stream")
        return int(n.value)

    def submit_fastq_pair(self, text1, text2) -> int:
        """Two FASTQ chunks with the same number of whole records (fastq.pair_chunks): mates are interleaved on the GPU and
        submitted as pairs.  Returns the number of reads."""
        b1 = np.frombuffer(text1, dtype=np.uint8) if not isinstance(text1, np.ndarray) else np.ascontiguousarray(text1, np.uint8)
        b2 = np.frombuffer(text2, dtype=np.uint8) if not isinstance(text2, np.ndarray) else np.ascontiguousarray(text2, np.uint8)
        n = C.c_uint64()
        self._check(self.lib.mlst_submit_fastq_pair(self._h, _ptr(b1) if b1.size else None, b1.size, _ptr(b2) if b2.size else None, b2.size, C.byref(n)),
                    "mlst_submit_fastq_pair")
        return int(n.value)

    def submit_fastq_bgzf_range(self, path: str, lo: int, hi: int, chunk_bytes: int = 256 << 20, verify_crc: bool = False) -> int:
        """The records of a bgzip'd FASTQ that start in the BGZF blocks starting in compressed bytes [lo, hi): the boundary
        blocks are inflated on the host to find the record boundaries (fastq.bgzf_range_plan), everything between goes to
        the GPU compressed.  N ranks given consecutive ranges read every record exactly once.  verify_crc: the host checks the
        CRC-32 of the blocks it inflates (ValueError); the blocks between are the device's (set_bgzf_verify)."""
        from .fastq import bgzf_range_plan
        plan = bgzf_range_plan(path, lo, hi, verify_crc)
        total = 0
        first, end = plan["mid"]
        if plan["head"]:
            total += self.submit_fastq_stream(plan["head"], final=(first >= end and not plan["tail"]))
        if end > first:
            total += self._submit_bgzf_pieces(path, first, end, chunk_bytes, False, not plan["tail"])
        if plan["tail"]:
            total += self.submit_fastq_stream(plan["tail"], final=True)
        return total

    def submit_reads_device(self, d_bases: int, d_quals: int, d_off: int, n_reads: int, max_len: int, paired: bool = False):
        self._check(self.lib.mlst_submit_reads_device(self._h, d_bases, d_quals, d_off, n_reads, max_len, int(paired)),
                    "mlst_submit_reads_device")

    def pack_reads_device(self, d_bases: int, d_quals: int, d_off: int, n_reads: int, d_packed: int, d_qual_rows: int,
                          d_lens: int, words_per_read: int, qual_stride: int):
        self._check(self.lib.mlst_pack_reads_device(self._h, d_bases, d_quals, d_off, n_reads, d_packed, d_qual_rows, d_lens,
                                                    words_per_read, qual_stride), "mlst_pack_reads_device")

    def submit_packed_device(self, d_packed: int, d_qual_rows: int, d_lens: int, n_reads: int, words_per_read: int,
                             qual_stride: int, paired: bool = False):
        self._check(self.lib.mlst_submit_packed_device(self._h, d_packed, d_qual_rows, d_lens, n_reads, words_per_read,
                                                       qual_stride, int(paired)), "mlst_submit_packed_device")

    def submit_packed_host(self, packed: np.ndarray, qrows: np.ndarray, lens: np.ndarray, n_reads: int, words_per_read: int, qual_stride: int,
                           paired: bool = False):
        """Pass 1 from host-packed arrays (pack_fastq_host): bases and lengths cross the link, Phred rows of the sieve's
        candidates only."""
        self._check(self.lib.mlst_submit_packed_host(self._h, _ptr(packed), _ptr(qrows), _ptr(lens), int(n_reads), int(words_per_read),
                                                     int(qual_stride), 1 if paired else 0), "mlst_submit_packed_host")

    def stats(self) -> SampleStats:
        nA, nL = self.index.n_alleles, self.index.n_loci
        s = SampleStats(np.zeros(nA, np.int64), np.zeros(nA, np.uint32), np.zeros(nL, np.uint64),
                        np.zeros(nL, np.uint64), np.zeros(MLST_CNT_N, np.uint64))
        self._check(self.lib.mlst_get_allele_stats(self._h, _ptr(s.sum_score), _ptr(s.n_hits), _ptr(s.locus_len_sum),
                                                   _ptr(s.locus_first), _ptr(s.counters)), "mlst_get_allele_stats")
        return s

    def pileup_alignments(self, chosen, rec_allele, rec_pos0, rec_as, rec_xm, cigar_off, cigar, seq_off, seq, qual,
                          minscore: int = 80, max_xm: int = 5, minqual: int = 20) -> dict[int, np.ndarray]:
        """Pass 2 over ready-made alignment records (metamlst_amd.samin); {allele idx: uint32[len, 4]}."""
        ch = np.ascontiguousarray(chosen, np.uint32)
        lens = [int(self.index.off[a + 1] - self.index.off[a]) for a in ch]
        counts = np.zeros((max(1, sum(lens)), 4), np.uint32)
        arr = [np.ascontiguousarray(x, t) for x, t in ((rec_allele, np.uint32), (rec_pos0, np.int32), (rec_as, np.int32), (rec_xm, np.int32),
                                                       (cigar_off, np.uint64), (cigar, np.uint32), (seq_off, np.uint64), (seq, np.uint8), (qual, np.uint8))]
        self._check(self.lib.mlst_pileup_alignments(self._h, _ptr(ch), len(ch), len(arr[0]), *[_ptr(x) for x in arr],
                                                    int(minscore), int(max_xm), int(minqual), _ptr(counts)), "mlst_pileup_alignments")
        out, at = {}, 0
        for a, L in zip(ch, lens):
            out[int(a)] = counts[at:at + L]
            at += L
        return out

    def export_alignments(self, chosen) -> Alignments:
        """The engine's alignments of the sample's work items to the chosen alleles (allele indices, one per locus at the most), as
        records: what the pile-up of `chosen` piles up, the records that fail its AS / XM filter included (mlst_alignments_export /
        mlst_alignments_fetch).  Reads the sample's state and changes none of it."""
        ch = np.ascontiguousarray(chosen, np.uint32)
        nr, nc, ns = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_alignments_export(self._h, _ptr(ch) if len(ch) else None, len(ch), C.byref(nr), C.byref(nc), C.byref(ns)),
                    "mlst_alignments_export")
        nr, nc, ns = int(nr.value), int(nc.value), int(ns.value)
        a = Alignments(np.zeros(nr, np.uint64), np.zeros(nr, np.uint32), np.zeros(nr, np.int32), np.zeros(nr, np.int32), np.zeros(nr, np.int32),
                       np.zeros(nr, np.int32), np.zeros(nr, np.uint8), np.zeros(nr + 1, np.uint64), np.zeros(nc, np.uint32),
                       np.zeros(nr + 1, np.uint64), np.zeros(ns, np.uint8), np.zeros(ns, np.uint8))
        self._check(self.lib.mlst_alignments_fetch(self._h, *[_ptr(getattr(a, f.name)) for f in dataclasses.fields(a)]), "mlst_alignments_fetch")
        return a

    def export_sam_text(self, idx, paired: bool = False, round_bytes: int = 0, md: bool = False):
        """Every alignment of the sample as SAM records, formatted on the device (mlst_alignments_text_open / _next / _close; the
        rule: samout's docstring): a generator of `bytes`, whole lines, one per round of at most round_bytes of bounded text
        (0: 256 MiB).  idx: the loaded AlleleIndex (its labels are the RNAMEs); paired: the sample was submitted as pairs.  The
        rounds leave the device through one page-locked buffer; the export is closed on exhaustion and on error.  Reads the
        sample's state and changes none of it.  md=True: the records of this export carry MD:Z -- the switch of
        set_export_md is set for it and put back when the export is closed; md=False leaves the switch as it stands."""
        labels = [idx.label(a).encode() for a in range(idx.n_alleles)]
        name_off = np.zeros(len(labels) + 1, np.uint64)
        name_off[1:] = np.cumsum([len(x) for x in labels], dtype=np.uint64)
        names = np.frombuffer(b"".join(labels) or b"\0", np.uint8)
        set_md = bool(md) and not self.get_export_md()      # (md=False asks the library nothing)
        if set_md:
            self.lib.mlst_alignments_text_close(self._h)      # (an export left open: the open below would close it, the switch refuses it)
            self.set_export_md(True)
        try:
            self._check(self.lib.mlst_alignments_text_open(self._h, _ptr(names), _ptr(name_off), int(bool(paired)), int(round_bytes)), "mlst_alignments_text_open")
            buf = None
            nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()
            while True:
                # the size of the round that comes next, then the round itself
                self._check(self.lib.mlst_alignments_text_next(self._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done)), "mlst_alignments_text_next")
                if done.value:
                    break
                need = int(nb.value)
                if buf is None or len(buf) < need:
                    buf = pinned_array(max(need, 1 << 16))
                self._check(self.lib.mlst_alignments_text_next(self._h, _ptr(buf), len(buf), C.byref(nb), C.byref(nr), C.byref(done)), "mlst_alignments_text_next")
                if nb.value:      # (a round whose reads have no record gives no text)
                    yield buf[:int(nb.value)].tobytes()
                if done.value:
                    break
        finally:
            self.lib.mlst_alignments_text_close(self._h)
            if set_md:
                self.set_export_md(False)

    def export_reads_text(self, paired: bool = False, round_bytes: int = 0):
        """The reads that have at least one record in the full export, as FASTQ text formatted on the device (mlst_reads_text_open /
        _next / _close; the rule: samout.reads_fastq_rule): a generator of `bytes`, whole four-line records in ascending read index,
        one per round of at most round_bytes (0: 256 MiB) of bounded text and tables.  paired: the sample was submitted as pairs
        (names r<pair>/1, /2).  With set_read_names the names are the reads' own.  The export is closed on exhaustion, on error and
        when the generator is abandoned.  Reads the sample's state and changes none of it."""
        try:
            self._check(self.lib.mlst_reads_text_open(self._h, int(bool(paired)), int(round_bytes)), "mlst_reads_text_open")
            buf = None
            nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()
            while True:
                # the size of the round that comes next, then the round itself
                self._check(self.lib.mlst_reads_text_next(self._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done)), "mlst_reads_text_next")
                if done.value:
                    break
                need = int(nb.value)
                if buf is None or len(buf) < need:
                    buf = pinned_array(max(need, 1 << 16))
                self._check(self.lib.mlst_reads_text_next(self._h, _ptr(buf), len(buf), C.byref(nb), C.byref(nr), C.byref(done)), "mlst_reads_text_next")
                if nb.value:
                    yield buf[:int(nb.value)].tobytes()
                if done.value:
                    break
        finally:
            self.lib.mlst_reads_text_close(self._h)

    # ---- typing tail on the device ----
    def typing_enqueue(self, penalty: int = 100, mincov: int = 1, none_char: str = "N"):
        """Queue allele choice + pileup + consensus + host copies behind the submitted pass 1 (returns at once)."""
        self._check(self.lib.mlst_typing_enqueue(self._h, int(penalty), int(mincov), none_char.encode()), "mlst_typing_enqueue")

    def typing_choose_pileup(self, penalty: int = 100, d_counts: int = 0):
        self._check(self.lib.mlst_typing_choose_pileup(self._h, int(penalty), d_counts or None), "mlst_typing_choose_pileup")

    def typing_finish(self, mincov: int = 1, none_char: str = "N", d_counts: int = 0):
        self._check(self.lib.mlst_typing_finish(self._h, int(mincov), none_char.encode(), d_counts or None), "mlst_typing_finish")

    def typing_choose_pileup_compact(self, penalty: int, d_counts: int, cap_cols: int):
        """Allele choice + pileup into the compact layout (loci with a chosen allele only) of a buffer of cap_cols columns."""
        self._check(self.lib.mlst_typing_choose_pileup_compact(self._h, int(penalty), d_counts, int(cap_cols)), "mlst_typing_choose_pileup_compact")

    def typing_finish_compact(self, mincov: int, none_char: str, d_counts: int):
        self._check(self.lib.mlst_typing_finish_compact(self._h, int(mincov), none_char.encode(), d_counts), "mlst_typing_finish_compact")

    def typing_compact_info(self) -> tuple[int, bool]:
        """After typing_fetch: (columns the compact layout needed, True when they did not fit the buffer)."""
        need, over = C.c_uint64(), C.c_uint32()
        self._check(self.lib.mlst_typing_compact_info(self._h, C.byref(need), C.byref(over)), "mlst_typing_compact_info")
        return int(need.value), bool(over.value)

    def typing_total_cols(self) -> int:
        tot = C.c_uint64()
        self._check(self.lib.mlst_typing_layout(self._h, None, C.byref(tot)), "mlst_typing_layout")
        return int(tot.value)

    def set_stream(self, stream: int = 0):
        """Run the engine on a caller's HIP stream (e.g. torch.cuda.Stream.cuda_stream); 0 = its own stream again."""
        self._check(self.lib.mlst_set_stream(self._h, stream or None), "mlst_set_stream")

    def set_cu_partition(self, part: int, n_parts: int):
        """The engine's own stream on share `part` of `n_parts` equal shares of the CUs (n_parts = 1: the whole device)."""
        self._check(self.lib.mlst_set_cu_partition(self._h, int(part), int(n_parts)), "mlst_set_cu_partition")

    def own_stream(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.mlst_get_stream(self._h, C.byref(p)), "mlst_get_stream")
        return int(p.value or 0)

    def busy(self) -> bool:
        rc = self.lib.mlst_busy(self._h)
        if rc < 0:
            self._check(rc, "mlst_busy")
        return rc == 1

    def export_stats_device_async(self, d_sum: int, d_min: int):
        self._check(self.lib.mlst_export_stats_device_async(self._h, d_sum, d_min), "mlst_export_stats_device_async")

    def import_stats_device_async(self, d_sum: int, d_min: int):
        self._check(self.lib.mlst_import_stats_device_async(self._h, d_sum, d_min), "mlst_import_stats_device_async")

    def typing_wait(self):
        """Wait for the queued typing step; its results stay in the engine (typing_fetch(waited=True)) while the next step is queued."""
        self._check(self.lib.mlst_typing_wait(self._h), "mlst_typing_wait")

    def typing_fetch(self, per_allele: bool = True, waited: bool = False):
        """-> (SampleStats, {locus: chosen allele idx}, {allele idx: consensus bytes}) of the last typing_enqueue.
        per_allele=False leaves sum_score / n_hits out (empty arrays): a caller that takes choice and consensus from the
        device needs the per-locus figures only, and 12 bytes per allele of a large database are 4 MB to copy per sample."""
        nA, nL = self.index.n_alleles, self.index.n_loci
        if getattr(self, "_colbase", None) is None or len(self._colbase) != nL + 1:
            self._colbase = np.zeros(nL + 1, np.uint64)
            tot = C.c_uint64()
            self._check(self.lib.mlst_typing_layout(self._h, _ptr(self._colbase), C.byref(tot)), "mlst_typing_layout")
            self._cb_list = [int(x) for x in self._colbase]
        nA_out = nA if per_allele else 0
        s = SampleStats(np.empty(nA_out, np.int64), np.empty(nA_out, np.uint32), np.empty(nL, np.uint64),
                        np.empty(nL, np.uint64), np.empty(MLST_CNT_N, np.uint64))
        chosen = np.empty(nL, np.int32)
        letters = np.empty(self._cb_list[-1], np.uint8)
        fn = self.lib.mlst_typing_fetch_waited if waited else self.lib.mlst_typing_fetch
        self._check(fn(self._h, _ptr(s.sum_score) if per_allele else None, _ptr(s.n_hits) if per_allele else None,
                       _ptr(s.locus_len_sum), _ptr(s.locus_first), _ptr(s.counters), _ptr(chosen), _ptr(letters)), "mlst_typing_fetch")
        raw = letters.tobytes()
        ch, let = {}, {}
        off = self.index.off
        for l in np.nonzero(chosen >= 0)[0].tolist():
            a = int(chosen[l]); ch[l] = a
            b = self._cb_list[l]
            let[a] = raw[b:b + int(off[a + 1] - off[a])]
        return s, ch, let

    def flat_sizes(self) -> tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_stats_flat_sizes(self._h, C.byref(a), C.byref(b)), "mlst_stats_flat_sizes")
        return int(a.value), int(b.value)

    def export_stats_device(self, d_sum: int, d_min: int):
        self._check(self.lib.mlst_export_stats_device(self._h, d_sum, d_min), "mlst_export_stats_device")

    def import_stats_device(self, d_sum: int, d_min: int):
        self._check(self.lib.mlst_import_stats_device(self._h, d_sum, d_min), "mlst_import_stats_device")

    # ---- pass 2 ----
    def set_depth_cap(self, cap: int) -> None:
        """Policy MLST_DEPTH_CAP as a switch (pysam max_depth, metaMLST_functions.py:255-259): 0 = off; n = a column sees
        the first n records that span it in (read index, strand) order.  Every pile-up that follows."""
        self._check(self.lib.mlst_set_depth_cap(self._h, int(cap)), "mlst_set_depth_cap")
        self.depth_cap = int(cap)

    def pileup(self, chosen: list[int]) -> dict[int, np.ndarray]:
        """{allele idx: uint32[len, 4]} for the chosen alleles (A,C,G,T columns)."""
        ch = np.ascontiguousarray(chosen, dtype=np.uint32)
        if any(int(a) >= self.index.n_alleles for a in chosen):
            raise MlstError("mlst_pileup: chosen allele out of range")
        lens = [int(self.index.off[a + 1] - self.index.off[a]) for a in chosen]
        counts = np.zeros((sum(lens), 4), np.uint32)
        self._check(self.lib.mlst_pileup(self._h, _ptr(ch), len(chosen), _ptr(counts)), "mlst_pileup")
        out, at = {}, 0
        for a, L in zip(chosen, lens):
            out[int(a)] = counts[at:at + L]
            at += L
        return out

    def consensus(self, chosen: list[int], mincov: int = 1, none_char: str = "N") -> dict[int, bytes]:
        """{allele idx: consensus bytes}: what cmseq's reference_free_consensus returns per contig (majority base,
        none_char below mincov), computed on the GPU from the pileup."""
        ch = np.ascontiguousarray(chosen, dtype=np.uint32)
        if any(int(a) >= self.index.n_alleles for a in chosen):
            raise MlstError("mlst_consensus: chosen allele out of range")
        lens = [int(self.index.off[a + 1] - self.index.off[a]) for a in chosen]
        out = np.zeros(max(1, sum(lens)), np.uint8)
        self._check(self.lib.mlst_consensus(self._h, _ptr(ch), len(chosen), int(mincov), none_char.encode(), _ptr(out), None), "mlst_consensus")
        res, at = {}, 0
        buf = out.tobytes()
        for a, L in zip(chosen, lens):
            res[int(a)] = buf[at:at + L]
            at += L
        return res

    def consensus_from_counts_device(self, d_counts: int, n_cols: int, mincov: int = 1, none_char: str = "N") -> bytes:
        out = np.zeros(max(1, n_cols), np.uint8)
        self._check(self.lib.mlst_consensus_from_counts_device(self._h, d_counts, n_cols, int(mincov), none_char.encode(), _ptr(out)),
                    "mlst_consensus_from_counts_device")
        return out.tobytes()[:n_cols]

    def pileup_device(self, chosen: list[int], d_counts: int) -> int:
        ch = np.ascontiguousarray(chosen, dtype=np.uint32)
        n = C.c_uint64()
        self._check(self.lib.mlst_pileup_device(self._h, _ptr(ch), len(chosen), d_counts, C.byref(n)), "mlst_pileup_device")
        return int(n.value)

    # ---- allele match ----
    def hamming_le(self, locus: int, query: bytes, z: int) -> tuple[int, int]:
        q = np.frombuffer(query, dtype=np.uint8)
        first, nw = C.c_int32(), C.c_uint32()
        self._check(self.lib.mlst_hamming_le(self._h, locus, _ptr(q) if len(q) else None, len(q), z, C.byref(first), C.byref(nw)),
                    "mlst_hamming_le")
        return int(first.value), int(nw.value)

    def hamming_all(self, locus: int, query: bytes) -> np.ndarray:
        q = np.frombuffer(query, dtype=np.uint8)
        if not 0 <= locus < self.index.n_loci:
            raise MlstError("mlst_hamming_all: locus %d out of range" % locus)
        d = np.zeros(int(self.index.locus_count[locus]), np.uint32)
        self._check(self.lib.mlst_hamming_all(self._h, locus, _ptr(q) if len(q) else None, len(q), _ptr(d)), "mlst_hamming_all")
        return d

    # ---- misc ----
    def align_center_star(self, seqs) -> tuple[int, list[bytes]]:
        """Centre-star alignment of `seqs` (bytes each) on the GPU: (index of the centre, the rows), byte for byte what
        metamlst_amd.msa.center_star returns (mlst_msa_align / mlst_msa_fetch).  Raises MlstError for what that statement refuses."""
        seqs = [bytes(q) for q in seqs]
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
        flat = np.frombuffer(b"".join(seqs) or b"\0", np.uint8)
        center, width = C.c_uint32(), C.c_uint32()
        self._check(self.lib.mlst_msa_align(self._h, _ptr(flat), _ptr(off), len(seqs), C.byref(center), C.byref(width)), "mlst_msa_align")
        rows = np.empty((len(seqs), width.value), np.uint8)
        self._check(self.lib.mlst_msa_fetch(self._h, _ptr(rows)), "mlst_msa_fetch")
        return int(center.value), [r.tobytes() for r in rows]

    def reset_sample(self):
        self._check(self.lib.mlst_reset_sample(self._h), "mlst_reset_sample")

    def set_read_index_base(self, base: int):
        self._check(self.lib.mlst_set_read_index_base(self._h, int(base)), "mlst_set_read_index_base")

    def items(self, cap: int = 1 << 20) -> np.ndarray:
        buf = (MlstItem * cap)()
        n = C.c_uint64()
        self._check(self.lib.mlst_get_items(self._h, C.cast(buf, C.c_void_p), cap, C.byref(n)), "mlst_get_items")
        k = min(cap, int(n.value))
        return np.array([(b.read_index, b.locus, b.strand, b.diag, b.votes) for b in buf[:k]], dtype=np.int64).reshape(-1, 5)

    def set_profiling(self, on):
        """0 / False = off, 1 / True = HIP events + sieve window, 2 = sieve window only (hipGraph replay stays on)."""
        self._check(self.lib.mlst_set_profiling(self._h, int(on)), "mlst_set_profiling")

    def kernel_time(self, which: int | str) -> tuple[float, int]:
        w = KERNELS.index(which) if isinstance(which, str) else which
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.lib.mlst_get_kernel_time(self._h, w, C.byref(ms), C.byref(n)), "mlst_get_kernel_time")
        return float(ms.value), int(n.value)

    def reset_kernel_time(self):
        self._check(self.lib.mlst_reset_kernel_time(self._h), "mlst_reset_kernel_time")

    def index_bytes(self) -> list[int]:
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_get_index_bytes(self._h, out), "mlst_get_index_bytes")
        return [int(x) for x in out]

    def sieve_info(self) -> dict:
        """{kind, n_seeds, longest_chain, buckets} of the loaded database's seed sieve."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mlst_get_sieve_info(self._h, out), "mlst_get_sieve_info")
        return {"kind": SIEVE_KINDS[int(out[0])], "n_seeds": int(out[1]), "longest_chain": int(out[2]), "buckets": int(out[3])}

    def extend_info(self) -> dict:
        """The block-haplotype tables of the loaded database (mlst_get_extend_info)."""
        out = (C.c_uint64 * 8)()
        self._check(self.lib.mlst_get_extend_info(self._h, out), "mlst_get_extend_info")
        keys = ("haplotypes", "bytes", "loci", "window6", "window11", "lds_bytes_160", "lds_bytes_320", "threads")
        return {k: int(v) for k, v in zip(keys, out)}

    def route_trace(self):
        """Diagnostics of the routed sieve's last submission (None until the trace, switched on by the first call, has
        seen one): {P, arena, packed, khz, cap, filter, flags, arena_entries, wg: uint64[P + 256][4]}."""
        n = C.c_uint64()
        self._check(self.lib.mlst_get_route_trace(self._h, None, 0, C.byref(n)), "mlst_get_route_trace")
        if not n.value:
            return None
        out = np.zeros(int(n.value), np.uint64)
        self._check(self.lib.mlst_get_route_trace(self._h, _ptr(out), out.size, C.byref(n)), "mlst_get_route_trace")
        keys = ("P", "arena", "packed", "khz", "cap", "filter", "flags", "arena_entries")
        d = {k: int(out[i]) for i, k in enumerate(keys)}
        d["wg"] = out[8:].reshape(-1, 4)
        return d

    def debug_route_realloc(self, pad_bytes: int = 0):
        """pad_bytes = -1: keep the old arena allocated (the new one is other memory for certain)."""
        self._check(self.lib.mlst_debug_route_realloc(self._h, int(pad_bytes) & 0xFFFFFFFFFFFFFFFF), "mlst_debug_route_realloc")

    def debug_route_probe(self, with_candidates: bool = True) -> tuple[int, np.ndarray | None]:
        """Test hook (mlst_debug_route_probe): (blocks of parked entries that found the consumer's LDS ring full during the sample,
        the sorted candidate list of the last submission or None)."""
        full, n = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mlst_debug_route_probe(self._h, C.byref(full), None, 0, C.byref(n)), "mlst_debug_route_probe")
        if not with_candidates:
            return int(full.value), None
        cand = np.zeros(max(int(n.value), 1), np.uint32)
        self._check(self.lib.mlst_debug_route_probe(self._h, C.byref(full), _ptr(cand), cand.size, C.byref(n)), "mlst_debug_route_probe")
        return int(full.value), np.sort(cand[:int(n.value)])

    def synchronize(self):
        self._check(self.lib.mlst_synchronize(self._h), "mlst_synchronize")
