"""fastq.read_stats / read_stats_text / phred_hint: the rule mlst_set_read_stats counts by on the device (csrc/read_stats.h), stated
once in Python, the report file of `cli type --read-stats` and the Phred hint.  The hand cases are worked out on paper from the rule in
include/mlst.h, not taken from the function.  Then the command's refusals and the new symbols in header, library and engine.py."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from metamlst_amd import cli, engine
from metamlst_amd import fastq as fq
from metamlst_amd.fastq import phred_hint, prep_fastq, read_stats, read_stats_text, trim_adapters
from test_read_prep_host import HAND, phred, rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cells(a) -> dict:
    """{index tuple: count} of the non-zero cells"""
    return {tuple(int(x) for x in i): int(a[tuple(i)]) for i in np.argwhere(a)}


def test_lengths_0_and_1_letters_and_qualities_by_hand():
    text = (rec(b"e", b"", b"")                       # length 0: reads and len_hist[0] only
            + rec(b"o", b"g", b"I")                   # length 1: GC 100 %, mean quality 40
            + rec(b"m", b"AcgTNnRy.-", b"!~\x90?I+5@#\x7f"))
    s = read_stats(text)
    assert s[1]["reads"] == 0 and not s[1]["len_hist"].any()
    t = s[0]
    assert (t["reads"], t["bases"], t["clamped_low"]) == (3, 11, 0)
    assert cells(t["len_hist"]) == {(0,): 1, (1,): 1, (10,): 1}
    # cycle 0: g and A; then c, g, T; N n R y . - are "other": every byte that is none of ACGT in either case
    assert cells(t["base"]) == {(0, 2): 1, (0, 0): 1, (1, 1): 1, (2, 2): 1, (3, 3): 1, (4, 4): 1, (5, 4): 1, (6, 4): 1, (7, 4): 1, (8, 4): 1, (9, 4): 1}
    # '!' 0, '~' 93, 0x90 = 144 -> 111 -> bin 93, '?' 30, 'I' 40, '+' 10, '5' 20, '@' 31, '#' 2, 0x7f = 127 -> 94 -> bin 93
    assert cells(t["qual"]) == {(0, 40): 1, (0, 0): 1, (1, 93): 1, (2, 93): 1, (3, 30): 1, (4, 40): 1, (5, 10): 1, (6, 20): 1, (7, 31): 1, (8, 2): 1, (9, 93): 1}
    # GC: 1 of 1 -> 100; c and g of 10 -> 20.  Mean quality: 40; (0 + 93 + 93 + 30 + 40 + 10 + 20 + 31 + 2 + 93) // 10 = 412 // 10 = 41
    assert cells(t["gc_hist"]) == {(100,): 1, (20,): 1}
    assert cells(t["readqual_hist"]) == {(40,): 1, (41,): 1}
    assert t["qual"].shape == (320, 94) and t["base"].shape == (320, 5) and len(t["len_hist"]) == 321 and len(t["gc_hist"]) == 101 and len(t["readqual_hist"]) == 94


def test_base_64_and_the_characters_below_it():
    text = rec(b"r", b"ACGT", b"@h5\x90")      # '@' 0, 'h' 40, '5' = 53 < 64: clamped to 0 and counted, 0x90 = 144 -> 80
    t = read_stats(text, phred64=True)[0]
    assert cells(t["qual"]) == {(0, 0): 1, (1, 40): 1, (2, 0): 1, (3, 80): 1} and t["clamped_low"] == 1
    assert cells(t["readqual_hist"]) == {(30,): 1}      # 120 // 4
    t33 = read_stats(text)[0]
    assert cells(t33["qual"]) == {(0, 31): 1, (1, 71): 1, (2, 20): 1, (3, 93): 1} and t33["clamped_low"] == 0
    assert read_stats(rec(b"r", b"A", b" "))[0]["clamped_low"] == 1      # a blank is below '!'


def test_crlf_line_ends_and_a_last_record_without_a_newline():
    lf = rec(b"a", b"ACGTT", b"IIII5") + rec(b"b", b"GG", b"??")
    crlf = rec(b"a", b"ACGTT", b"IIII5", b"\r\n") + rec(b"b", b"GG", b"??", b"\r\n")
    want = read_stats(lf)
    assert want[0]["bases"] == 7
    for other in (crlf, lf[:-1]):
        got = read_stats(other)
        assert all(fq.read_stats_equal(g, w) for g, w in zip(got, want))


def test_paired_sides_and_the_current_side():
    r = [rec(b"p0/1", b"AAAA", b"IIII"), rec(b"p0/2", b"CC", b"55"), rec(b"p1/1", b"GGG", b"???"), rec(b"p1/2", b"T", b"!")]
    s = read_stats(b"".join(r), paired=True)
    assert (s[0]["reads"], s[0]["bases"], s[1]["reads"], s[1]["bases"]) == (2, 7, 2, 3)
    assert cells(s[0]["base"]) == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1, (0, 2): 1, (1, 2): 1, (2, 2): 1}
    assert cells(s[1]["base"]) == {(0, 1): 1, (1, 1): 1, (0, 3): 1}
    assert cells(s[1]["qual"]) == {(0, 20): 1, (1, 20): 1, (0, 0): 1}
    # the same records as two unpaired texts, the second counted into side 1
    one, two = read_stats(r[0] + r[2], side=0), read_stats(r[1] + r[3], side=1)
    assert one[1]["reads"] == 0 and two[0]["reads"] == 0
    assert fq.read_stats_equal(one[0], s[0]) and fq.read_stats_equal(two[1], s[1])
    both = fq.read_stats_sum(one[0], two[1])
    assert fq.read_stats_equal(both, read_stats(b"".join(r))[0])
    with pytest.raises(ValueError, match="whole pairs"):
        read_stats(b"".join(r[:3]), paired=True)
    with pytest.raises(ValueError, match="side"):
        read_stats(r[0], side=2)
    with pytest.raises(ValueError, match="longer than 320"):
        read_stats(rec(b"l", b"A" * 321, b"I" * 321))
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        read_stats(rec(b"l", b"AC", b"I"))


def test_prepared_is_the_rule_on_the_prepared_text():
    """the hand cases of test_read_prep_host.py: what remains under T = 20 is what the prepared stage counts, cycle 0 at the first
    remaining base"""
    text = b"".join(rec(b"r%d" % k, (b"ACGT" * 4)[:len(q)], phred(q, 64)) for k, (q, _) in enumerate(HAND))
    t = read_stats(prep_fastq(text, trim_qual=20, phred64=True)[0])[0]
    assert t["reads"] == len(HAND) and t["bases"] == sum(w for _, w in HAND) and t["clamped_low"] == 0
    want_len = {}
    for _, w in HAND:
        want_len[(w,)] = want_len.get((w,), 0) + 1
    assert cells(t["len_hist"]) == want_len
    want_q = {}
    for q, w in HAND:
        for c, v in enumerate(q[:w]):
            want_q[(c, v)] = want_q.get((c, v), 0) + 1
    assert cells(t["qual"]) == want_q
    # trim5 moves cycle 0; an adapter cut ends the read: ACGTAC + adapter TAC at 3
    one = rec(b"r", b"ACGTACGG", phred([30, 31, 32, 33, 34, 35, 36, 37]))
    t = read_stats(trim_adapters(prep_fastq(one, trim5=1)[0], "TACGG", 3, 0)[0])[0]
    assert cells(t["base"]) == {(0, 1): 1, (1, 2): 1} and cells(t["qual"]) == {(0, 31): 1, (1, 32): 1} and cells(t["len_hist"]) == {(2,): 1}


FIXED = rec(b"a", b"ACGTN", b"IIII!") + rec(b"b", b"acg", b"5?+") + rec(b"c", b"", b"")
FIXED_TSV = b"""#metamlst-readstats\t1
#sample\ts1
#phred_base\t33
#stages\traw
#columns\ttable\tstage\tside\tindex\tvalues
total\traw\t0\t0\t3\t8\t0
len\traw\t0\t0\t1
len\traw\t0\t3\t1
len\traw\t0\t5\t1
base\traw\t0\t0\t2\t0\t0\t0\t0
base\traw\t0\t1\t0\t2\t0\t0\t0
base\traw\t0\t2\t0\t0\t2\t0\t0
base\traw\t0\t3\t0\t0\t0\t1\t0
base\traw\t0\t4\t0\t0\t0\t0\t1
qual\traw\t0\t0\t%s
qual\traw\t0\t1\t%s
qual\traw\t0\t2\t%s
qual\traw\t0\t3\t%s
qual\traw\t0\t4\t%s
gc\traw\t0\t40\t1
gc\traw\t0\t66\t1
readqual\traw\t0\t20\t1
readqual\traw\t0\t32\t1
"""


def qrow(*at) -> bytes:
    """41 columns (Phred 0 .. 40, the highest bin in use), a 1 at each of `at`"""
    return b"\t".join(b"1" if v in at else b"0" for v in range(41))


def test_report_bytes_on_a_fixed_input():
    s = read_stats(FIXED)
    stats = {"raw": s, "prepared": s, "phred_base": 33, "prepared_counted": False}
    # qualities: cycle 0: I 40, 5 20; 1: I, ? 30; 2: I, + 10; 3: I; 4: ! 0.  Means: 160 // 5 = 32, 60 // 3 = 20
    want = FIXED_TSV % (qrow(40, 20), qrow(40, 30), qrow(40, 10), qrow(40), qrow(0))
    got = read_stats_text(stats, "s1")
    assert got == want
    assert read_stats_text({"raw": s, "prepared": s}, "s1", phred64=False, prepared=False) == want
    # both stages and a second side
    p = read_stats(rec(b"a", b"ACG", b"III") + rec(b"m", b"TT", b"55"), paired=True)
    two = read_stats_text({"raw": p, "prepared": p, "phred_base": 64, "prepared_counted": True}, "x").decode().split("\n")
    assert two[2:4] == ["#phred_base\t64", "#stages\traw,prepared"]
    assert [l.split("\t")[:3] for l in two if l.startswith("total")] == [["total", "raw", "0"], ["total", "raw", "1"], ["total", "prepared", "0"], ["total", "prepared", "1"]]
    assert "base\tprepared\t1\t1\t0\t0\t0\t1\t0" in two and not any(l.startswith("base\tprepared\t1\t2") for l in two)
    assert all(re.fullmatch(r"#.*|[a-z]+\t(raw|prepared)\t[01](\t\d+)+", l) for l in two[:-1]) and two[-1] == ""
    # the docstring states the format
    doc = read_stats_text.__doc__
    for word in ("#metamlst-readstats", "#sample", "#phred_base", "#stages", "#columns", "total", "len", "base", "qual", "gc", "readqual", "project's own"):
        assert word in doc, word


def test_phred_hint_in_both_directions_and_silent_otherwise():
    def stats_of(text, phred64=False):
        s = read_stats(text, phred64=phred64)
        return {"raw": s, "prepared": s, "phred_base": 64 if phred64 else 33, "prepared_counted": False}

    seq = b"ACGT" * 25
    p64 = b"".join(rec(b"r%d" % k, seq, phred([2 + (k + c) % 39 for c in range(100)], 64)) for k in range(10))      # 1,000 bases, Phred 2 .. 40 at +64
    hint = phred_hint(stats_of(p64))
    assert hint and "looks like Phred+64" in hint and "--phred64" in hint and "1000 bases" in hint
    assert phred_hint(stats_of(p64, phred64=True)) is None                            # typed with the flag: nothing to say
    assert phred_hint(stats_of(p64[:len(p64) // 10 * 9])) is None                     # 900 bases: fewer than 1,000
    normal = b"".join(rec(b"r%d" % k, seq, phred([2 + (k + c) % 39 for c in range(100)])) for k in range(10))
    assert phred_hint(stats_of(normal)) is None
    one_low = p64 + rec(b"x", b"A", b"?")                                             # one character below '@'
    assert phred_hint(stats_of(one_low)) is None
    back = phred_hint(stats_of(normal, phred64=True))
    assert back and "does not look like Phred+64" in back and "without --phred64" in back
    # both sides count
    s = read_stats(p64[:len(p64) // 2], side=0)
    s[1] = read_stats(p64[len(p64) // 2:], side=1)[1]
    assert phred_hint({"raw": s, "prepared": s, "phred_base": 33}) is not None


def test_the_lines_of_the_command():
    s = read_stats(rec(b"a", b"ACGTN", b"IIII!") + rec(b"b", b"GGGCC", b"?????"))
    lines = cli.read_stats_lines({"raw": s, "prepared": s, "prepared_counted": False})
    assert lines == ["read statistics (raw, side 0): 2 reads, 10 bases, mean length 5.0, >= Q20 90.0 %, >= Q30 90.0 %, GC 70.0 %, non-ACGT 10.00 %"]


def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    from test_gpu_pair_bgzf import bgzf_blocks
    (tmp_path / "s.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    os.makedirs(tmp_path / "in")
    for k in range(2):
        (tmp_path / "in" / ("f%d.fastq" % k)).write_bytes(b"@r\nACGT\n+\nIIII\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    for args, why in ((["s.fastq", "--alignments"], "with --alignments the file holds alignments, not the reads of a FASTQ file"),
                      (["c.fa", "--contigs"], "--contigs cuts assemblies into windows, and an assembly has neither cycles nor qualities"),
                      (["s.fastq", "--long-reads"], "--long-reads cuts reads into windows, and the tables hold the 320 cycles of a short read"),
                      ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts reads into windows, and the tables hold the 320 cycles of a short read"),
                      ([str(bam)], "the reads of a BAM are not counted: FASTQ input only"),
                      (["s.fastq", "t.fastq"], "it reports one sample: several samples or a folder are typed without it"),
                      (["in"], "it reports one sample: several samples or a folder are typed without it"),
                      (["s.fastq", "--gpus", "2"], "the tables are one GPU's: a rank of --gpus N counts its own share of the reads only")):
        monkeypatch.chdir(tmp_path)
        assert cli.main(["type"] + args + ["--read-stats", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]) == 1
        assert "--read-stats: " + why in capsys.readouterr().out, args
    assert not os.path.exists(tmp_path / "o")


def test_new_symbols_in_header_library_and_engine():
    ge.build()
    lib = engine.load_library()
    header = open(os.path.join(ROOT, "include", "mlst.h")).read()
    for name in ("mlst_set_read_stats", "mlst_get_read_stats", "mlst_set_read_stats_side", "mlst_read_stats_fetch", "mlst_read_stats_info"):
        assert re.search(r"^int %s\(mlst_handle\* h" % name, header, re.M), name
        assert hasattr(lib, name) and name in lib._mlst_symbols, name
    for meth in ("set_read_stats", "get_read_stats", "set_read_stats_side", "read_stats", "read_stats_info"):
        assert callable(getattr(engine.Engine, meth)), meth
    consts = {k: int(v) for k, v in re.findall(r"^#define MLST_RS_([A-Z_]+) (\d+)$", header, re.M)}
    assert consts == {"READS": 0, "BASES": 1, "CLAMPED_LOW": 2, "LEN": fq.RS_LEN, "BASE": fq.RS_BASE, "QUAL": fq.RS_QUAL, "GC": fq.RS_GC,
                      "READQUAL": fq.RS_READQUAL, "WORDS": fq.RS_WORDS}
    assert (fq.RS_BASE - fq.RS_LEN, fq.RS_QUAL - fq.RS_BASE, fq.RS_GC - fq.RS_QUAL, fq.RS_READQUAL - fq.RS_GC, fq.RS_WORDS - fq.RS_READQUAL) == (321, 1600, 320 * 94, 101, 94)
