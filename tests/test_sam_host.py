"""samin.read_sam_header: the names table of the device path for SAM text (mlst_sam_open), from plain and gzip files.  No device needed."""
import gzip
import os

import numpy as np
import pytest

import golden_util as gu
from metamlst_amd import samin
from metamlst_amd.index import load_index
from test_bam_gpu import write, zoo

RECORD = "r1\t0\t%s\t1\t255\t4M\t*\t0\t0\tACGT\tIIII\tAS:i:8\tXN:i:0\tXM:i:0\tXO:i:0\n"


def both(tmp_path, name, text: bytes):
    """the text as a plain file and gzipped"""
    plain = tmp_path / name
    plain.write_bytes(text)
    with gzip.open(str(plain) + ".gz", "wb") as z:
        z.write(text)
    return str(plain), str(plain) + ".gz"


def test_three_thousand_long_names_and_the_triples_of_the_bam_header(tmp_path):
    idx = load_index(gu.golden_db())
    refs = [("spLong_gene%04d_%d" % (k, k) + "x" * 40, 1000 + k) for k in range(3000)] + [(idx.label(0), 10), ("a_b", 5)]
    text = ("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:bowtie2\n" + RECORD % refs[5][0]).encode()
    assert len(text) > 3 * 60000
    _, recs = zoo(idx, 20)
    recs = [(r[0], r[1], refs[k % len(refs)][0], r[3], r[4], r[5], r[6], r[7], r[8]) for k, r in enumerate(recs)]
    bam_names = samin.read_bam_header(write(tmp_path / "h.bam", refs, recs))[0]
    sp = idx.loci[0][0]
    for path in both(tmp_path, "h.sam", text):
        names = samin.read_sam_header(path)
        assert names == [r[0] for r in refs] == bam_names
        for filt in (None, sp, "nobody"):
            for got, want in zip(samin.bam_ref_table(idx, names, filt), samin.bam_ref_table(idx, bam_names, filt)):
                assert np.array_equal(got, want) and got.dtype == want.dtype
        ra, rl, rf = samin.bam_ref_table(idx, names, None)
        assert ra[-2] == 0 and rl[-2] == int(idx.locus_id[0]) and rf[-2] == 1 and rf[-1] == 2 and ra[0] == -1
        assert samin.is_sam_text(path)
    assert not samin.is_sam_text(str(tmp_path / "h.bam"))


@pytest.mark.parametrize("header, want", [
    ("", []),                                                                                      # no header at all
    ("@HD\tVN:1.0\n", []),
    ("@SQ\tLN:5\n@SQ\tSN:a_b_1\tLN:7\n@SQ\tLN:9\tAS:x\n", ["a_b_1"]),                              # @SQ lines without SN:
    ("@SQ\tSN:a_b_1\tLN:7\n@CO\tSN:no_t_1\n@CO\t@SQ\tSN:no_t_2\n@SQ\tLN:3\tSN:a_b_2\n", ["a_b_1", "a_b_2"]),      # @CO lines between them
    ("@SQ\tSN:a_b_1\tLN:7\r\n@SQ\tSN:a_b_2\r\n", ["a_b_1", "a_b_2"]),                              # CRLF
    ("@SQ\tSN:\tLN:7\n@SQ\tSN:a_b_1\tSN:zz\n", ["", "a_b_1"]),                                     # an empty name; the first SN: of a line
], ids=["none", "hd-only", "sq-without-sn", "co-between", "crlf", "empty-and-first"])
def test_header_shapes(tmp_path, header, want):
    # an @SQ line behind the first record is no part of the header
    text = (header + RECORD % "a_b_1" + "@SQ\tSN:late_x_1\tLN:4\n" + RECORD % "a_b_2").encode()
    for path in both(tmp_path, "s.sam", text):
        assert samin.read_sam_header(path) == want
        assert len(list(samin.read_alignments(path))) == 2      # (the host reader passes over '@' lines wherever they stand)


def test_empty_file_and_a_last_header_line_without_lf(tmp_path):
    for path in both(tmp_path, "e.sam", b""):
        assert samin.read_sam_header(path) == []
    for path in both(tmp_path, "l.sam", b"@SQ\tSN:a_b_1\tLN:7\n@SQ\tSN:a_b_2"):
        assert samin.read_sam_header(path) == ["a_b_1", "a_b_2"]


def test_names_keep_their_bytes(tmp_path):
    raw = b"sp\xff_g_1"
    for path in both(tmp_path, "b.sam", b"@SQ\tSN:" + raw + b"\tLN:7\n@SQ\tSN:sp\xc3\xa9_g_2\n"):
        names = samin.read_sam_header(path)
        assert [n.encode("utf-8", "surrogateescape") for n in names] == [raw, b"sp\xc3\xa9_g_2"] and names[1] == "spé_g_2"


def test_golden_inputs_carry_no_sq_lines():
    # (the device tests give them the header bowtie2 writes; as they are, their first record goes to the host path)
    for case in sorted(os.listdir(os.path.join(gu.GOLD, "typing"))):
        assert samin.read_sam_header(os.path.join(gu.GOLD, "typing", case, "input.sam")) == []
