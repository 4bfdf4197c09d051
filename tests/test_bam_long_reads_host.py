"""The builders of tests/bam_long_reads.py against restatements of the rule (long_reads.window_starts, a reverse complement written
out here), their figures, and the refusals of `cli type --long-bam-reads`.  No GPU."""
import gzip
import struct

import numpy as np
import pytest

import bam_long_reads as bl
import bam_reads_zoo as bz
import fixtures as fx
import long_reads as lr
from metamlst_amd import synth

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ------------------------------------------------------------------ the builders' figures
@pytest.mark.parametrize("tile", lr.TILES)
def test_window_counts_and_the_reverse_strand_slice(tmp_path, tile):
    read_len, stride = tile
    for n in lr.edge_lengths(*tile) + [321, bl.LONGEST]:
        assert len(lr.window_starts(n, read_len, stride)) == lr.fa_windows_of(n, read_len, stride)
    lengths = [n for n in lr.edge_lengths(*tile) if n and n < 32_000] + [321, 2001, 2000]      # (window by window in Python: short ones)
    seqs = lr.random_records(lengths)
    path = bl.write(tmp_path / "e.bam", bl.records(lengths))
    counts = {}
    text, yard = bl.yardstick(path, tile, counts)
    assert counts["reads"] == len(lengths) and counts["secondary"] + counts["empty"] == len(range(0, len(lengths), 3)) + 1
    reads, wins = lr.parse(text), lr.parse(yard)
    assert [s for _, s, _ in reads] == seqs and [q for _, _, q in reads] == [lr.quals(n, r) for r, n in enumerate(lengths)]
    starts, _, flags, lseqs = bz.layout(path)
    raw = gzip.open(path, "rb").read()
    kept_at = [int(s) for s, k in zip(starts, bz.kept_mask(flags, lseqs)) if k]
    at = 0
    for r, (n, s) in enumerate(zip(lengths, seqs)):
        st_list = lr.window_starts(n, read_len, stride)
        assert len(st_list) == lr.fa_windows_of(n, read_len, stride)
        # the stored SEQ of the record, nibble by nibble
        rec = kept_at[r]
        flag = struct.unpack_from("<H", raw, rec + 18)[0]
        seq_at = rec + 36 + raw[rec + 12] + 4 * struct.unpack_from("<H", raw, rec + 16)[0]
        nib = np.frombuffer(raw[seq_at:seq_at + (n + 1) // 2], np.uint8)
        stored = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)[np.stack((nib >> 4, nib & 15), 1).reshape(-1)[:n]].tobytes()
        assert bool(flag & 16) == bool(r % 2) and (stored == s) != bool(flag & 16)
        for st in st_list:
            ln = min(n, read_len)
            assert wins[at][1] == s[st:st + ln] and wins[at][2] == lr.quals(n, r)[st:st + ln]
            if flag & 16:      # window st of the read: bases n - 1 - st ... n - st - len of SEQ, complemented
                assert wins[at][1] == stored[n - st - ln:n - st][::-1].translate(_COMP)
            at += 1
        if flag & 16 and n > read_len:      # the flush window of the read lies at the FRONT of the stored SEQ
            assert wins[at - 1][1] == stored[:read_len][::-1].translate(_COMP)
    assert at == len(wins)


def test_the_writer_writes_the_longest_record(tmp_path):
    seq = lr.random_records([bl.LONGEST])[0]
    path = bl.write(tmp_path / "big.bam", [bz.unmapped("r698000", seq.decode(), lr.quals(bl.LONGEST, 0).decode("latin1"))])
    starts, end, flags, lseqs = bz.layout(path)
    assert len(starts) == 1 and end - int(starts[0]) == 1_047_044 < (1 << 20) - 64 and int(lseqs[0]) == bl.LONGEST
    (_, s, q), = lr.parse(bl.reads_text(path))
    assert s == seq and q == lr.quals(bl.LONGEST, 0)


def test_the_long_read_sample_as_a_bam(tmp_path):
    """the 1,800 reads of tests/test_gpu_long_reads.py's `sample` as a BAM, every other one reverse-mapped"""
    db, idx = fx.ecoli_small(80)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][11], size=100_000)
    text = lr.genome_reads(g, 1800)
    path = bl.write(tmp_path / "s.bam", bl.from_fastq(text))
    back, yard = bl.yardstick(path, (150, 25))
    assert [r[1:] for r in lr.parse(back)] == [r[1:] for r in lr.parse(text)]
    assert yard.count(b"\n") // 4 == 114_284
    assert int((bz.layout(path)[2] & 16 != 0).sum()) == 900


# ------------------------------------------------------------------ the command
def _reads_bam(tmp_path, name="long.bam", flag=None):
    seq = lr.random_records([400])[0]
    return bl.write(tmp_path / name, [bz.skipped("secondary", 0), bl.kept(0, seq, False, flag=flag)])


@pytest.mark.parametrize("extra, said", [(["-2", "OTHER"], "it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N"),
                                         (["--alignments"], "it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N"),
                                         (["--contigs"], "it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N"),
                                         (["--long-reads"], "it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N"),
                                         (["--gpus", "2"], "it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N"),
                                         (["OTHER"], "--long-bam-reads takes BAM files"),
                                         (["--tile", "150"], "--tile LEN,STEP takes two positive numbers"),
                                         (["--tile", "0,25"], "--tile LEN,STEP takes two positive numbers"),
                                         (["--tile", "321,25"], "at most 320 bases")])
def test_refusals_of_the_command(tmp_path, capsys, extra, said):
    from metamlst_amd.cli import main
    f = _reads_bam(tmp_path)
    other = str(tmp_path / "other.fastq")
    open(other, "wb").write(lr.record(0, b"ACGT" * 100))
    more = [other] if extra == ["OTHER"] else []      # (a second READS file: a FASTQ among the BAMs)
    extra = [] if more else [other if x == "OTHER" else x for x in extra]
    assert main(["type", f] + more + ["--long-bam-reads", "-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "o")] + extra) == 1
    out = capsys.readouterr().out
    assert said in out and len(out.strip().splitlines()) == 1


def test_a_paired_bam_is_refused(tmp_path, capsys):
    from metamlst_amd.cli import main
    f = _reads_bam(tmp_path, "paired.bam", flag=1 | 4 | 8 | 64)
    assert main(["type", f, "--long-bam-reads", "-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "o")]) == 1
    out = capsys.readouterr().out
    assert "--long-bam-reads takes unpaired reads" in out and "FLAG 0x1" in out and len(out.strip().splitlines()) == 1


def test_long_reads_still_refuses_a_bam_and_names_the_new_switch(tmp_path, capsys):
    from metamlst_amd.cli import main
    f = _reads_bam(tmp_path)
    assert main(["type", f, "--long-reads", "-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "o")]) == 1
    out = capsys.readouterr().out
    assert "--long-reads takes FASTQ" in out and "--long-bam-reads" in out and "samtools" not in out
