"""fastq.dedup_fastq, the rule mlst_set_read_dedup applies on the device (include/mlst.h; csrc/read_dedup.h), pinned by hand; the refusals
of `cli type --dedup`, each with its reason and before any GPU use; the three symbols in header, library and engine.py; the command's
line on fixed counters.  No GPU is needed."""
import ctypes as C
import os

import pytest

from metamlst_amd import cli
from metamlst_amd import engine as eng_mod
from metamlst_amd.fastq import DEDUP_LEVELS, dedup_fastq, dedup_level
from test_gpu_pair_bgzf import bgzf_blocks


def rec(name: str, seq: bytes, eol: bytes = b"\n", qual: bytes = None) -> bytes:
    return b"@" + name.encode() + eol + seq + eol + b"+" + eol + (qual if qual is not None else b"I" * len(seq)) + eol


def kept(text: bytes) -> list:
    """per record: the sequence line is not empty"""
    lines = text.split(b"\n")
    return [len(lines[k + 1]) > 0 for k in range(0, len(lines) - 1, 4)]


def info_of(**kv) -> dict:
    out = {"reads": 0, "units": 0, "duplicates": 0, "reads_removed": 0, "bases_removed": 0, "distinct": 0, "levels": [0] * 8}
    out.update(kv)
    return out


def test_case_folding_n_against_r_a_prefix_and_empty_reads():
    seqs = [b"ACGTACGT",      # 0 the first occurrence
            b"acgtAcGt",      # 1 a copy in another case
            b"ACGTACG",       # 2 a prefix: another length, another key
            b"ACGNACGT",      # 3
            b"ACGRACGT",      # 4 R folds to N: a copy of 3
            b"ACG.acgt",      # 5 so does every other byte
            b"ACGAACGT",      # 6 A is not N
            b"",              # 7 an empty read: neither a copy ...
            b"",              # 8 ... nor a first occurrence
            b"ACGTACGT",      # 9 a third copy of 0
            b"ACGTACGA"]      # 10 differs in the last base
    text = b"".join(rec("r%d" % k, s, qual=bytes(40 + (k + j) % 30 for j in range(len(s)))) for k, s in enumerate(seqs))
    out, info = dedup_fastq(text)
    assert kept(out) == [True, False, True, True, False, False, True, False, False, False, True]
    assert info == info_of(reads=11, units=9, duplicates=4, reads_removed=4, bases_removed=32, distinct=5, levels=[3, 0, 2, 0, 0, 0, 0, 0])
    # a duplicate stays a record: header and '+' line untouched, two empty lines; everything else is the text's bytes
    lines_in, lines_out = text.split(b"\n"), out.split(b"\n")
    assert len(lines_in) == len(lines_out)
    for k, keep in enumerate(kept(out)):
        want = lines_in[4 * k:4 * k + 4] if keep or not seqs[k] else [lines_in[4 * k], b"", lines_in[4 * k + 2], b""]
        assert lines_out[4 * k:4 * k + 4] == want, k
    assert dedup_fastq(out)[0] == out and dedup_fastq(out)[1]["duplicates"] == 0      # (the text it writes holds none)
    assert dedup_fastq(b"") == (b"", info_of())


def test_qualities_and_names_play_no_part_and_a_reverse_complement_is_no_duplicate():
    text = rec("a", b"AACCGGTTAC", qual=b"IIIIIIIIII") + rec("b", b"AACCGGTTAC", qual=b"##########") + rec("c", b"GTAACCGGTT")
    out, info = dedup_fastq(text)
    assert kept(out) == [True, False, True] and info["duplicates"] == 1 and info["distinct"] == 2


def test_crlf_text():
    text = rec("a", b"ACGTT", b"\r\n") + rec("b", b"ACGTT", b"\r\n") + rec("c", b"ACGTA", b"\r\n")
    out, info = dedup_fastq(text)
    assert out == rec("a", b"ACGTT") + rec("b", b"") + rec("c", b"ACGTA")      # line ends LF
    assert info == info_of(reads=3, units=2 + 1, duplicates=1, reads_removed=1, bases_removed=5, distinct=2, levels=[1, 1, 0, 0, 0, 0, 0, 0])
    mixed = rec("a", b"ACGTT", b"\r\n") + rec("b", b"ACGTT")
    assert kept(dedup_fastq(mixed)[0]) == [True, False]      # (the CR is no letter)


def test_pairs():
    pairs = [(b"AAAACCCC", b"GGGGTTTT"),      # 0
             (b"AAAACCCC", b"GGGGTTTA"),      # 1 the same mate 1, another mate 2
             (b"GGGGTTTT", b"AAAACCCC"),      # 2 pair 0 with the mates swapped
             (b"aaaacccc", b"GGGGTTTT"),      # 3 a copy of pair 0
             (b"AAAACCCC", b""),              # 4 one empty mate: takes part as it is
             (b"", b"AAAACCCC"),              # 5 the other mate empty: another key
             (b"AAAACCCC", b""),              # 6 a copy of pair 4
             (b"", b""),                      # 7 both empty: takes no part
             (b"", b""),                      # 8
             (b"AAAACCC", b"CGGGGTTTT"),      # 9 the same letters end to end as pair 0, the lengths differ
             (b"", b"AAAACCCC")]              # 10 a copy of pair 5
    text = b"".join(rec("p%d/1" % k, a) + rec("p%d/2" % k, b) for k, (a, b) in enumerate(pairs))
    out, info = dedup_fastq(text, paired=True)
    gone = {3, 6, 10}
    want = []
    for k, (a, b) in enumerate(pairs):
        want += [bool(a) and k not in gone, bool(b) and k not in gone]
    assert kept(out) == want
    assert info == info_of(reads=22, units=9, duplicates=3, reads_removed=6, bases_removed=16 + 8 + 8, distinct=6, levels=[3, 3, 0, 0, 0, 0, 0, 0])
    # unpaired, the same text is another sample: every mate on its own
    out1, info1 = dedup_fastq(text)
    assert info1["units"] == 22 - 8 and info1["distinct"] == 5 and out1 != out
    with pytest.raises(ValueError, match="not whole pairs"):
        dedup_fastq(text[:len(text) - len(rec("p10/2", b"AAAACCCC"))], paired=True)
    with pytest.raises(ValueError, match="4-line records"):
        dedup_fastq(b"@r\nACGT\n+\n")
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        dedup_fastq(b"@r\nACGT\n+\nIII\n")


def test_the_levels_bin_edges():
    assert DEDUP_LEVELS == (1, 2, 3, 4, 5, 10, 50, 500)
    assert [dedup_level(c) for c in (1, 2, 3, 4, 5, 9, 10, 49, 50, 499, 500, 10 ** 6)] == [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    counts = [1, 2, 3, 4, 5, 9, 10, 49, 50, 499, 500, 501]
    letters = b"ACGT"
    reads = []
    for k, c in enumerate(counts):
        seq = bytes(letters[(k >> (2 * j)) & 3] for j in range(4)) + b"ACGT" * 5
        reads += [seq] * c
    # (interleave the copies: the order of the records plays no part in the counters)
    reads = reads[::2] + reads[1::2]
    out, info = dedup_fastq(b"".join(rec("r%d" % k, s) for k, s in enumerate(reads)))
    assert info["levels"] == [1, 1, 1, 1, 2, 2, 2, 2] and info["distinct"] == len(counts)
    assert info["units"] == info["reads"] == sum(counts) and info["duplicates"] == sum(counts) - len(counts) == info["reads_removed"]
    assert info["bases_removed"] == 24 * info["duplicates"] and sum(kept(out)) == len(counts)


# ------------------------------------------------------------------ the command
def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    os.makedirs(tmp_path / "in")
    for k in range(2):
        (tmp_path / "in" / ("f%d.fastq" % k)).write_bytes(b"@r\nACGT\n+\nIIII\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    head = "duplicate removal (--dedup): "
    tail = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]
    for args, why in ((["s.fastq", "--alignments"], "with --alignments the file holds alignments, not reads to compare"),
                      (["c.fa", "--contigs"], "--contigs cuts assemblies into windows"),
                      (["s.fastq", "--long-reads"], "--long-reads cuts reads into windows, and the windows of a read would be compared, not the read"),
                      ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts reads into windows, and the windows of a read would be compared, not the read"),
                      ([str(bam)], "the reads of a BAM are not compared: FASTQ input only"),
                      (["s.fastq", "t.fastq"], "one table of keys per engine: several samples or a folder are typed without it"),
                      (["in"], "one table of keys per engine: several samples or a folder are typed without it"),
                      (["s.fastq", "--gpus", "2"], "a rank of --gpus N sees only its byte range, and duplicates across ranks would be missed")):
        monkeypatch.chdir(tmp_path)
        assert cli.main(["type"] + args + ["--dedup"] + tail) == 1, args
        assert head + why in capsys.readouterr().out, args
    # the flag alone, and with what it goes with, gets past the checks
    for args in (["s.fastq"], ["s.fastq,t.fastq"], ["s.fastq", "-2", "t.fastq"],
                 ["s.fastq", "--trim5", "1", "--trim-qual", "20", "--phred64", "--adapter", "illumina", "--read-stats", "--write-sam", "--write-sam-all", "--write-reads", "--read-names"]):
        assert cli.main(["type"] + args + ["--dedup"] + tail) == 1
        assert capsys.readouterr().out.startswith("Failed to connect to the database"), args
    assert not os.path.exists(tmp_path / "o")


def test_the_commands_line_on_fixed_counters():
    info = {"reads": 2000, "units": 1000, "duplicates": 333, "reads_removed": 666, "bases_removed": 99900, "distinct": 667, "clashes": 0, "slots": 4194304,
            "levels": [500, 100, 50, 10, 4, 2, 1, 0]}
    assert cli.read_dedup_line(info, paired=True) == ("duplicate removal: 1000 pairs, 333 duplicates (33.3 %), 99900 bases removed; distinct 667: "
                                                      "x1 500, x2 100, x3 50, x4 10, x5-9 4, x10-49 2, x50-499 1, x500+ 0")
    info.update(units=3, duplicates=2, clashes=7)
    assert cli.read_dedup_line(info).startswith("duplicate removal: 3 reads, 2 duplicates (66.7 %), ")      # (2000 / 3 = 666.67 tenths of a percent: half up)
    assert cli.read_dedup_line(info).endswith("x500+ 0; 7 kept on a 64-bit clash")
    info.update(units=2000, duplicates=1)
    assert "1 duplicates (0.1 %)" in cli.read_dedup_line(info)      # (0.05 %: half up)
    info.update(units=0, duplicates=0, clashes=0)
    assert "0 reads, 0 duplicates (0.0 %)" in cli.read_dedup_line(info)
    # dedup_fastq's counters carry no "clashes": the line takes them too
    assert cli.read_dedup_line(dedup_fastq(rec("a", b"ACGT") * 2)[1]) == ("duplicate removal: 2 reads, 1 duplicates (50.0 %), 4 bases removed; distinct 1: "
                                                                         "x1 0, x2 1, x3 0, x4 0, x5-9 0, x10-49 0, x50-499 0, x500+ 0")


# ------------------------------------------------------------------ the C ABI
def test_the_three_symbols_are_in_header_library_and_engine():
    lib = eng_mod.load_library()
    want = {"mlst_set_read_dedup": [C.c_int], "mlst_get_read_dedup": [C.POINTER(C.c_int)], "mlst_read_dedup_info": [C.POINTER(C.c_uint64)]}
    for name, args in want.items():
        fn = getattr(lib, name)                                                          # AttributeError: the symbol is missing
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes[1:]) == args, (name, fn.argtypes)
    root = os.path.dirname(os.path.dirname(os.path.abspath(eng_mod.__file__)))
    text = open(os.path.join(root, "include", "mlst.h")).read()
    for line in ("int mlst_set_read_dedup(mlst_handle* h, int on);", "int mlst_get_read_dedup(mlst_handle* h, int* on);", "int mlst_read_dedup_info(mlst_handle* h, uint64_t out[16]);"):
        assert line in text
    assert "#define MLST_DEDUP_KEY        128" in open(os.path.join(root, "include", "mlst_policy.h")).read()
    for name in ("set_read_dedup", "get_read_dedup", "read_dedup_info"):
        assert callable(getattr(eng_mod.Engine, name))
