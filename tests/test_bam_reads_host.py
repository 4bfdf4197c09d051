"""The reads of a BAM on the host (samin.bam_reads_fastq, the yardstick of the device path of tests/test_gpu_bam_reads.py): the
rules of include/mlst.h against hand-written expectations, and the figures of the record zoo the device tests type -- properties
of the input, checked here without a device."""
import numpy as np
import pytest

import bam_reads_zoo as bz
from metamlst_amd import samin


def fastq_of(tmp_path, recs, paired=False, counts=None):
    path = bz.write(tmp_path / "t.bam", recs)
    return b"".join(samin.bam_reads_fastq(path, paired=paired, counts=counts))


def test_forward_record(tmp_path):
    assert fastq_of(tmp_path, [bz.unmapped("r1", "ACGTA", "IIII#")]) == b"@r1\nACGTA\n+\nIIII#\n"


def test_reverse_record_of_odd_length_is_reverse_complemented_and_its_filler_nibble_ignored(tmp_path):
    rec = ("r2", 16, "chrHost", 7, 30, "5M", "AACGT", "ABCDE", [])
    assert fastq_of(tmp_path, [rec]) == b"@r2\nACGTT\n+\nEDCBA\n"
    # (bam_writer's filler nibble is 0, '=': it would read as a sixth base if it were taken)
    assert fastq_of(tmp_path, [("r3", 16, "chrHost", 7, 30, "1M", "C", "5", [])]) == b"@r3\nG\n+\n5\n"


def test_n_and_iupac_letters(tmp_path):
    assert fastq_of(tmp_path, [bz.unmapped("f", "ANRC", "IIII")]) == b"@f\nANRC\n+\nIIII\n"
    # R = A|G -> complement Y = T|C; the order is reversed
    assert fastq_of(tmp_path, [("r", 16, "chrHost", 1, 9, "4M", "ANRC", "1234", [])]) == b"@r\nGYNT\n+\n4321\n"


def test_record_without_qualities_gets_phred_1(tmp_path):
    assert fastq_of(tmp_path, [bz.unmapped("nq", "ACGTAC", "*")]) == b'@nq\nACGTAC\n+\n""""""\n'


def test_quality_bytes_are_clamped_to_127_and_only_a_first_byte_of_255_means_no_qualities(tmp_path):
    raw = (128, 200, 254, 127, 0, 255)
    rec = bz.unmapped("hq", "ACGTAC", "".join(chr(33 + q) for q in raw))
    assert fastq_of(tmp_path, [rec]) == b"@hq\nACGTAC\n+\n" + bytes([160, 160, 160, 160, 33, 160]) + b"\n"
    rev = ("hr", 16, "chrHost", 1, 9, "3M", "AAC", "".join(chr(33 + q) for q in (200, 255, 3)), [])
    assert fastq_of(tmp_path, [rev]) == b"@hr\nGTT\n+\n" + bytes([36, 160, 160]) + b"\n"


def test_secondary_supplementary_and_empty_records_are_skipped_and_counted(tmp_path):
    counts = {}
    recs = [bz.skipped("secondary", 1), bz.unmapped("a", "ACGT", "IIII"), bz.skipped("supplementary", 2), bz.skipped("empty", 3),
            ("both", 256, "*", 0, 0, "*", "*", "*", []), bz.unmapped("b", "TT", "##"), bz.skipped("empty", 4)]
    assert fastq_of(tmp_path, recs, counts=counts) == b"@a\nACGT\n+\nIIII\n@b\nTT\n+\n##\n"
    assert counts == {"reads": 2, "secondary": 3, "empty": 2}      # (secondary and empty: counts as secondary)
    assert samin.bam_first_read_flags(bz.write(tmp_path / "f.bam", recs)) == 4
    assert samin.bam_first_read_flags(bz.write(tmp_path / "g.bam", recs[2:4])) is None


def test_mate_suffixes_and_paired_names(tmp_path):
    recs = [bz.unmapped("q", "ACGT", "IIII", flag=77), bz.skipped("empty", 0), bz.unmapped("q", "GGCC", "JJJJ", flag=141)]
    assert fastq_of(tmp_path, recs) == b"@q/1\nACGT\n+\nIIII\n@q/2\nGGCC\n+\nJJJJ\n"
    assert fastq_of(tmp_path, recs, paired=True) == b"@q\nACGT\n+\nIIII\n@q\nGGCC\n+\nJJJJ\n"
    assert samin.bam_first_read_flags(bz.write(tmp_path / "p.bam", recs)) == 77
    with pytest.raises(ValueError, match="record 0 has no mate next to it"):
        fastq_of(tmp_path, recs[:2], paired=True)
    with pytest.raises(ValueError, match="record 0 has no mate next to it"):
        fastq_of(tmp_path, [recs[0], bz.unmapped("other", "GGCC", "JJJJ", flag=141)], paired=True)
    with pytest.raises(ValueError, match="record 2 has no mate next to it"):
        fastq_of(tmp_path, [recs[0], recs[1], bz.unmapped("q", "GGCC", "JJJJ", flag=4)], paired=True)


# ------------------------------------------------------------------ the zoo of tests/test_gpu_bam_reads.py
@pytest.mark.parametrize("n_kept", [63, 64, 65, 6000])
def test_zoo_counts(tmp_path, n_kept):
    recs = bz.zoo(n_kept)
    path = bz.write(tmp_path / "z.bam", recs)
    counts = {}
    text = b"".join(samin.bam_reads_fastq(path, counts=counts))
    assert counts["reads"] == n_kept == text.count(b"\n") // 4
    assert counts["secondary"] == sum(1 for r in recs if r[1] & 0x900) and counts["empty"] == sum(1 for r in recs if not r[1] & 0x900 and r[6] == "*")
    assert counts["secondary"] >= 3 and counts["empty"] >= 3
    assert not bz.is_kept(recs[0]) and not bz.is_kept(recs[-1])      # skipped records as the first and the last of the file
    lens = sorted({len(r[6]) for r in recs if bz.is_kept(r)})
    assert set(bz.EDGE_LENGTHS) <= set(lens) and max(lens) == 320


def test_zoo_has_kept_records_across_block_boundaries_and_a_tag_longer_than_a_cell_of_heads(tmp_path):
    path = bz.write(tmp_path / "z.bam", bz.zoo(6000))
    starts, end, flags, lseqs = bz.layout(path)
    assert end > 10 * bz.BLOCK
    ends = np.append(starts[1:], end)
    straddles = (starts // bz.BLOCK != (ends - 1) // bz.BLOCK) & bz.kept_mask(flags, lseqs)
    assert straddles.sum() >= 5
    assert (ends - starts).max() > 20000


@pytest.mark.parametrize("blocks_per_call", [1, 2])
def test_paired_zoo_has_pieces_that_end_on_an_odd_kept_count(tmp_path, blocks_per_call):
    recs = bz.zoo_paired(3000)
    path = bz.write(tmp_path / "p.bam", recs)
    text = b"".join(samin.bam_reads_fastq(path, paired=True))
    assert text.count(b"\n") // 4 == 6000
    starts, end, flags, lseqs = bz.layout(path)
    ends = np.append(starts[1:], end)
    kept = bz.kept_mask(flags, lseqs)
    # a call of n blocks ends at a multiple of n * BLOCK inflated bytes (the header is shorter than a block): the records complete
    # by then hold an odd number of reads -> the piece hands its last kept record on
    cuts = np.arange(blocks_per_call * bz.BLOCK, end, blocks_per_call * bz.BLOCK)
    odd = [int(kept[ends <= c].sum()) & 1 for c in cuts]
    assert len(cuts) >= 4 and sum(odd) >= 1 and sum(odd) < len(odd)
    # mates are neighbours among the kept records, with skipped records between the mates of some pairs
    names = [r[0] for r in recs if bz.is_kept(r)]
    assert names[0::2] == names[1::2]
    between = sum(1 for k in range(1, len(recs) - 1) if not bz.is_kept(recs[k]) and bz.is_kept(recs[k - 1]) and bz.is_kept(recs[k + 1]) and recs[k - 1][0] == recs[k + 1][0])
    assert between >= 10
