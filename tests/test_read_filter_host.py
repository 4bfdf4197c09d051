"""fastq.poly_tail / fastq.read_fails / fastq.filter_fastq, the rule mlst_set_read_filter applies on the device (include/mlst.h;
csrc/read_filter.h), pinned by hand; the refusals of `cli type --trim-poly-g / --trim-poly-x / --min-length / --max-n / --low-complexity
/ --min-mean-qual`, each with its reason and before any GPU use; the three symbols in header, library and engine.py; the command's line on
fixed counters.  No GPU is needed.  The rule is the project's own (modelled on fastp); nothing here claims fastp's bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from metamlst_amd import cli
from metamlst_amd import engine as eng_mod
from metamlst_amd.fastq import check_read_filter, filter_fastq, poly_tail, read_fails
from test_gpu_pair_bgzf import bgzf_blocks

B = b"ACT" * 10      # a front of 30 bases without a G: no tail of G reaches into it, and it is no tail of another letter


def tail(L: int, m: int) -> bytes:
    """L bases that begin on a G, then m bases that are no G, then G to the end"""
    return b"G" + b"A" * m + b"G" * (L - 1 - m)


G5 = {"letters": b"G", "poly_min": 5}
G10 = {"letters": b"G"}
X10 = {"letters": b"ACGT"}
# (sequence, quality characters or None for all 'I', the arguments of filter_fastq, bases the tail trim leaves, the tail's letter or -1,
#  the reason the read then fails or 0) -- every number written by hand, none produced by the rule
KNOWN = [
    # the shortest tail
    (B + b"G" * 9, None, G10, 39, -1, 0),
    (B + b"G" * 10, None, G10, 30, 2, 0),
    (B + b"G" * 4, None, G5, 34, -1, 0),
    (B + b"G" * 5, None, G5, 30, 2, 0),
    # the budget min(5, L // 8), at it and one over: one over, what is cut is the run of G behind the other bases (when it is long enough)
    (B + tail(7, 0), None, G5, 30, 2, 0),         # L 7: budget 0
    (B + tail(7, 1), None, G5, 32, 2, 0),         # ... one mismatch: the five G behind it
    (B + tail(8, 1), None, G5, 30, 2, 0),         # L 8: budget 1
    (B + tail(8, 2), None, G5, 33, 2, 0),
    (B + tail(15, 1), None, G5, 30, 2, 0),        # L 15: budget 1
    (B + tail(15, 2), None, G5, 33, 2, 0),
    (B + tail(16, 2), None, G5, 30, 2, 0),        # L 16: budget 2
    (B + tail(16, 3), None, G5, 34, 2, 0),
    (B + tail(39, 4), None, G5, 30, 2, 0),        # L 39: budget 4
    (B + tail(39, 5), None, G5, 36, 2, 0),
    (B + tail(40, 5), None, G5, 30, 2, 0),        # L 40: budget 5
    (B + tail(40, 6), None, G5, 37, 2, 0),        # the sixth mismatch
    (B + tail(47, 5), None, G5, 30, 2, 0),        # L 47: budget 5
    (B + tail(47, 6), None, G5, 37, 2, 0),
    (B + tail(48, 5), None, G5, 30, 2, 0),        # L 48: 48 // 8 = 6, the cap is 5
    (B + tail(48, 6), None, G5, 37, 2, 0),
    (B + tail(8, 2), None, {"letters": b"G", "poly_min": 6}, 38, -1, 0),      # ... and the run behind is shorter than the minimum
    # where the tail begins
    (B + b"A" + b"G" * 9, None, G10, 40, -1, 0),                              # ten bases that begin on a mismatch are no tail
    (B + b"GT" + b"G" * 10, None, G10, 30, 2, 0),                             # it steps over one mismatch onto an earlier G
    (b"ACGT" * 10 + b"G" * 10, None, G10, 38, 2, 0),                          # the over-step example: 38, not 40
    (b"G" * 20, None, G10, 0, 2, 0),                                          # the whole read is the tail
    (b"G" * 9, None, G10, 9, -1, 0),
    # letters
    (B + b"g" * 10, None, G10, 30, 2, 0),                                     # lower case
    (B.lower() + b"GgGgGgGgGg", None, G10, 30, 2, 0),
    (B + b"GGGGNGGGGGGG", None, G10, 30, 2, 0),                               # an N inside the tail is a mismatch: twelve bases, budget 1
    (B + b"GNNGGGGGGGGG", None, G10, 42, -1, 0),                              # two of them: over the budget, and nine G are too few
    (B + b"G.GGGGGGGGGG", None, G10, 30, 2, 0),
    (b"CGT" * 10 + b"A" * 10, None, X10, 30, 0, 0),                           # all four letters
    (b"AGT" * 10 + b"C" * 10, None, X10, 30, 1, 0),
    (b"ACT" * 10 + b"G" * 10, None, X10, 30, 2, 0),
    (b"ACG" * 10 + b"T" * 10, None, X10, 30, 3, 0),
    (b"ACG" * 10 + b"T" * 10, None, G10, 40, -1, 0),                          # G alone leaves a tail of T
    (b"ACG" * 10 + b"T" * 10, None, {"letters": b"AT"}, 30, 3, 0),
    (b"ACG" * 10 + b"N" * 10, None, X10, 40, -1, 0),                          # N is no letter
    # n = 0, 1, 2
    (b"", None, G10, 0, -1, 0),
    (b"", None, {"letters": b"ACGT", "poly_min": 1, "min_length": 5, "max_n": 0, "complexity": 100, "mean_qual": 93}, 0, -1, 0),      # a read of length 0 fails nothing
    (b"G", None, G10, 1, -1, 0),
    (b"G", None, {"letters": b"G", "poly_min": 1}, 0, 2, 0),
    (b"GG", None, {"letters": b"G", "poly_min": 2}, 0, 2, 0),
    (b"AG", None, {"letters": b"G", "poly_min": 1}, 1, 2, 0),
    (b"GA", None, {"letters": b"G", "poly_min": 1}, 2, -1, 0),
    (b"A", None, {"complexity": 100}, 1, -1, 0),                              # complexity applies from two bases on
    (b"AA", None, {"complexity": 1}, 2, -1, 3),
    (b"AC", None, {"complexity": 100}, 2, -1, 0),
    # too short
    (b"ACGT" * 7 + b"A", None, {"min_length": 30}, 29, -1, 1),
    (b"ACGT" * 7 + b"AC", None, {"min_length": 30}, 30, -1, 0),
    (B + b"G" * 10, None, {"letters": b"G", "min_length": 31}, 30, 2, 1),     # judged as the tail trim leaves it
    (B + b"G" * 10, None, {"letters": b"G", "min_length": 30}, 30, 2, 0),
    # too many N: every byte that is none of ACGT in either case
    (b"ACGTNNNacgt", None, {"max_n": 3}, 11, -1, 0),
    (b"ACGTNNNacgtN", None, {"max_n": 3}, 12, -1, 2),
    (b"ACGTN.nacgt", None, {"max_n": 3}, 11, -1, 0),
    (b"ACGTN.nacgtR", None, {"max_n": 3}, 12, -1, 2),
    (b"ACGTACGT", None, {"max_n": 0}, 8, -1, 0),
    (b"ACGTACGN", None, {"max_n": 0}, 8, -1, 2),
    (B + b"GGGGNGGGGGGG", None, {"letters": b"G", "max_n": 0}, 30, 2, 0),     # the N went with the tail
    # low complexity: eleven bases, ten neighbours; 100 d against pct * 10
    (b"AAAACCCGGTT", None, {"complexity": 30}, 11, -1, 0),                    # d 3: 300 == 300 passes
    (b"AAAAACCCGGG", None, {"complexity": 30}, 11, -1, 3),                    # d 2
    (b"AAAAA.N-nXX", None, {"complexity": 10}, 11, -1, 0),                    # every other byte is N: d 1, 100 == 100
    (b"AAAAA.N-nXX", None, {"complexity": 11}, 11, -1, 3),
    (b"aAaAaAcCcCc", None, {"complexity": 10}, 11, -1, 0),                    # folded: d 1
    (b"ACACACACACA", None, {"complexity": 100}, 11, -1, 0),                   # d 10: a dinucleotide repeat is not caught by this measure
    (b"ACACACACAAA", None, {"complexity": 100}, 11, -1, 3),
    # low quality: ten bases at Q 20 need a sum of 200
    (b"ACGTACGTAC", b"IIIII!!!!!", {"mean_qual": 20}, 10, -1, 0),             # 5 * 40
    (b"ACGTACGTAC", b"IIIIH!!!!!", {"mean_qual": 20}, 10, -1, 4),             # 199
    (b"ACGTACGTAC", b"55555 5555", {"mean_qual": 18}, 10, -1, 0),             # a character below '!' counts 0: 9 * 20 = 180
    (b"ACGTACGTAC", b"55555 5554", {"mean_qual": 18}, 10, -1, 4),
    (b"ACGTACGTAC", b"~~~~~~~~~~", {"mean_qual": 93}, 10, -1, 0),
    # the first reason that holds
    (b"NNNN", None, {"min_length": 10, "max_n": 0}, 4, -1, 1),
    (b"N" * 12, None, {"max_n": 0, "complexity": 50}, 12, -1, 2),
    (b"A" * 10, b"!" * 10, {"complexity": 30, "mean_qual": 20}, 10, -1, 3),
    (b"N" * 12, b"!" * 12, {"min_length": 12, "max_n": 12, "complexity": 0, "mean_qual": 1}, 12, -1, 4),
]


def qual_of(seq: bytes, qual) -> bytes:
    return b"I" * len(seq) if qual is None else qual


def rec(name: str, seq: bytes, qual=None, eol: bytes = b"\n") -> bytes:
    return b"@" + name.encode() + eol + seq + eol + b"+" + eol + qual_of(seq, qual) + eol


def zero_info(**kw) -> dict:
    return dict({"tail_trimmed": 0, "tail_bases": 0, "per_letter": [0, 0, 0, 0], "tail_emptied": 0, "failed_short": 0, "failed_n": 0, "failed_complexity": 0,
                 "failed_quality": 0, "filtered_bases": 0}, **kw)


def brute_tail(seq: bytes, letters: bytes, min_len: int):
    """the definition, every L of every letter"""
    s = seq.upper()
    n = len(s)
    best = (0, -1)
    for x, X in enumerate(b"ACGT"):
        if X not in letters.upper():
            continue
        for L in range(max(1, min_len), n + 1):
            mism = sum(c != X for c in s[n - L:])
            if s[n - L] == X and mism <= min(5, L // 8) and L > best[0]:
                best = (L, x)
    return n - best[0], best[1]


# ------------------------------------------------------------------ the rule
def test_known_answers():
    for k, (seq, qual, kw, left, letter, why) in enumerate(KNOWN):
        q = qual_of(seq, qual)
        filters = {key: v for key, v in kw.items() if key not in ("letters", "poly_min")}
        if kw.get("letters"):
            assert poly_tail(seq, kw["letters"], kw.get("poly_min", 10)) == (left, letter), (k, seq)
        else:
            assert (left, letter) == (len(seq), -1), k
        assert read_fails(seq[:left], q[:left], **filters) == why, (k, seq)
        text, info = filter_fastq(rec("r", seq, q), **kw)
        end = 0 if why else left
        assert text == rec("r", seq[:end], q[:end]), (k, seq)
        want = zero_info(filtered_bases=left if why else 0)
        if letter >= 0:
            want.update(tail_trimmed=1, tail_bases=len(seq) - left, tail_emptied=int(left == 0))
            want["per_letter"][letter] = 1
        if why:
            want[("failed_short", "failed_n", "failed_complexity", "failed_quality")[why - 1]] = 1
        assert info == want, (k, seq, info)


def test_the_table_covers_what_it_says():
    for L, budget in ((7, 0), (8, 1), (15, 1), (16, 2), (39, 4), (40, 5), (47, 5), (48, 5)):
        assert min(5, L // 8) == budget
        for m in (budget, budget + 1):
            assert any(seq == B + tail(L, m) and kw == G5 for seq, _, kw, _, _, _ in KNOWN), (L, m)
    assert {letter for _, _, _, _, letter, _ in KNOWN} == {-1, 0, 1, 2, 3} and {why for *_, why in KNOWN} == {0, 1, 2, 3, 4}
    assert {len(seq) for seq, *_ in KNOWN} >= {0, 1, 2}


def test_the_rule_against_the_definition():
    rng = np.random.default_rng(41)
    cut = 0
    for k in range(400):
        n = int(rng.choice([0, 1, 2, 9, 10, 11, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100, 150]))
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes())
        L = int(rng.integers(0, n + 1)) if k % 2 else 0
        X = int(rng.choice(list(b"ACGTg")))
        for i in range(n - L, n):
            s[i] = X
        for _ in range(int(rng.integers(0, 8))):
            if n:
                s[int(rng.integers(0, n))] = int(rng.choice(list(b"ACGTNacgtn.")))
        letters = [b"G", b"ACGT", b"CT", b"a"][k % 4]
        min_len = int(rng.choice([1, 5, 10, 10, 20]))
        got = poly_tail(bytes(s), letters, min_len)
        assert got == brute_tail(bytes(s), letters, min_len), (k, bytes(s), letters, min_len)
        cut += got[1] >= 0
    assert cut > 60


def test_random_reads_are_rarely_cut():
    rng = np.random.default_rng(5)
    reads = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=150)].tobytes() for _ in range(3000)]
    assert sum(poly_tail(r, b"G")[1] >= 0 for r in reads) <= 2
    assert sum(poly_tail(r, b"ACGT")[1] >= 0 for r in reads) <= 4


def test_the_counters_of_a_small_text():
    recs = [("a", B + b"G" * 12, None),                    # a tail of 12 G
            ("b", b"G" * 15, None),                        # one tail: emptied by the trim, fails nothing
            ("c", b"CGT" * 10 + b"A" * 20, None),          # a tail of 20 A
            ("d", B[:20], None),                           # 20 bases: too short
            ("e", B + b"NNNN", None),                      # 4 N
            ("f", b"A" * 29 + b"C" + b"T" * 10, None),     # a tail of 10 T, then 30 bases with one change: low complexity
            ("g", B, b"#" * 30),                           # Q 2
            ("h", B + b"ACGTAC", None),                    # passes
            ("i", b"", None)]
    text = b"".join(rec(n, s, q) for n, s, q in recs)
    out, info = filter_fastq(text, letters=b"ACGT", poly_min=10, min_length=25, max_n=3, complexity=30, mean_qual=20)
    left = [B, b"", b"CGT" * 10, b"", b"", b"", b"", B + b"ACGTAC", b""]
    assert out == b"".join(rec(n, l, None if q is None else q[:len(l)]) for (n, _, q), l in zip(recs, left))
    assert info == {"tail_trimmed": 4, "tail_bases": 12 + 15 + 20 + 10, "per_letter": [1, 0, 2, 1], "tail_emptied": 1, "failed_short": 1, "failed_n": 1,
                    "failed_complexity": 1, "failed_quality": 1, "filtered_bases": 20 + 34 + 30 + 30}
    # line ends: CRLF in, LF out; mates are filtered file by file
    assert filter_fastq(b"".join(rec(n, s, q, b"\r\n") for n, s, q in recs), letters=b"ACGT", poly_min=10, min_length=25, max_n=3, complexity=30, mean_qual=20) == (out, info)
    assert filter_fastq(text) == (text, zero_info())
    with pytest.raises(ValueError, match="not a whole number of 4-line records"):
        filter_fastq(b"@a\nACGT\n+\n")
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        filter_fastq(rec("a", b"ACGT", b"II"))


def test_the_settings_that_are_refused():
    for bad, why in (({"letters": b"GX"}, "only A, C, G and T are taken"), ({"letters": b"N"}, "only A, C, G and T are taken"),
                     ({"letters": b"G", "poly_min": 0}, "poly_min 0 is outside 1..320"), ({"letters": b"G", "poly_min": 321}, "poly_min 321 is outside 1..320"),
                     ({"min_length": -1}, "min_length -1 is outside 0..320"), ({"min_length": 321}, "min_length 321 is outside 0..320"),
                     ({"max_n": -1}, "max_n -1 is outside"), ({"complexity": 101}, "complexity 101 is outside 0..100"), ({"complexity": -1}, "complexity -1 is outside 0..100"),
                     ({"mean_qual": 94}, "mean_qual 94 is outside 0..93"), ({"mean_qual": 1.5}, "mean_qual 1.5 is outside 0..93")):
        with pytest.raises(ValueError, match=why):
            check_read_filter(**bad)
        with pytest.raises(ValueError, match=why):
            filter_fastq(rec("a", b"ACGT"), **bad)
    assert check_read_filter() == 0 and check_read_filter(b"", poly_min=0) == 0      # (poly_min is looked at only with letters)
    assert check_read_filter("g") == 4 and check_read_filter(b"TTCA", 320, 320, 0, 100, 93) == 0b1011
    with pytest.raises(ValueError, match="poly_min 0"):
        poly_tail(b"ACGT", b"G", 0)


# ------------------------------------------------------------------ the command
HEAD = "read filter (--trim-poly-g, --trim-poly-x, --min-length, --max-n, --low-complexity, --min-mean-qual): "


def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r 1\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r 2\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    os.makedirs(tmp_path / "in")
    for k in range(2):
        (tmp_path / "in" / ("f%d.fastq" % k)).write_bytes(b"@r\nACGT\n+\nIIII\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    monkeypatch.chdir(tmp_path)
    tail_ = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]
    for flags in (["--trim-poly-g"], ["--trim-poly-x"], ["--min-length", "30"], ["--max-n", "5"], ["--low-complexity", "30"], ["--min-mean-qual", "20"]):
        for args, why in ((["s.fastq", "--alignments"], "with --alignments the records are what they are: the file holds alignments, not reads to trim or remove"),
                          (["c.fa", "--contigs"], "--contigs cuts assemblies into windows, and an assembly has neither tails nor qualities"),
                          (["s.fastq", "--long-reads"], "--long-reads cuts reads into windows, and a window is cut from the record as it stands"),
                          ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"),
                          ([str(bam)], "the reads of a BAM are taken as they are stored: FASTQ input only")):
            assert cli.main(["type"] + args + flags + tail_) == 1, (args, flags)
            assert HEAD + why in capsys.readouterr().out, (args, flags)
    for flags, why in ((["--trim-poly-g", "--trim-poly-x"], "--trim-poly-x trims G tails too: give one of the two"),
                       (["--poly-min", "12"], "--poly-min belongs to --trim-poly-g / --trim-poly-x"),
                       (["--poly-min", "12", "--min-length", "30"], "--poly-min belongs to --trim-poly-g / --trim-poly-x"),
                       (["--trim-poly-g", "--poly-min", "0"], "--poly-min takes a number from 1 to 320, not 0"),
                       (["--trim-poly-x", "--poly-min", "321"], "--poly-min takes a number from 1 to 320, not 321"),
                       (["--min-length", "0"], "--min-length takes a number from 1 to 320, not 0"),
                       (["--min-length", "321"], "--min-length takes a number from 1 to 320, not 321"),
                       (["--max-n", "4294967295"], "--max-n takes a number from 0 to 4294967294, not 4294967295"),
                       (["--low-complexity", "101"], "--low-complexity takes a number from 1 to 100, not 101"),
                       (["--low-complexity", "0"], "--low-complexity takes a number from 1 to 100, not 0"),
                       (["--min-mean-qual", "94"], "--min-mean-qual takes a number from 1 to 93, not 94")):
        assert cli.main(["type", "s.fastq"] + flags + tail_) == 1, flags
        assert why in capsys.readouterr().out, flags
    # a plain switch does not swallow the READS argument; the flags get past the checks where --adapter does: a folder, several samples, -2, --gpus
    every = ["--poly-min", "5", "--min-length", "320", "--max-n", "0", "--low-complexity", "100", "--min-mean-qual", "93"]
    for args in (["--trim-poly-g", "s.fastq"], ["--trim-poly-x", "s.fastq"] + every, ["s.fastq", "--trim-poly-g"] + every, ["in", "--trim-poly-g"], ["s.fastq", "t.fastq", "--max-n", "0"],
                 ["s.fastq", "-2", "t.fastq", "--trim-poly-x", "--pair-overlap", "--trim5", "1", "--trim-qual", "20", "--phred64", "--adapter", "illumina", "--read-stats", "--dedup",
                  "--write-sam", "--write-sam-all", "--write-reads", "--read-names"]):
        assert cli.main(["type"] + args + tail_) == 1, args
        assert capsys.readouterr().out.startswith("Failed to connect to the database"), args
    import argparse
    assert cli._read_filter_of(argparse.Namespace(trim_poly_x=True, max_n=0)) == {"poly": "ACGT", "poly_min": 10, "min_length": 0, "max_n": 0, "complexity": 0, "mean_qual": 0}
    assert cli._read_filter_of(argparse.Namespace(trim_poly_g=True, poly_min=7, min_mean_qual=20)) == {"poly": "G", "poly_min": 7, "min_length": 0, "max_n": None, "complexity": 0, "mean_qual": 20}
    assert cli._read_filter_of(argparse.Namespace()) is None
    assert not os.path.exists(tmp_path / "o")


def test_the_commands_line_on_fixed_counters():
    info = {"tail_trimmed": 1000, "tail_bases": 43210, "per_letter": [1, 2, 990, 7], "tail_emptied": 3, "failed_short": 40, "failed_n": 30, "failed_complexity": 20,
            "failed_quality": 10, "filtered_bases": 9876}
    assert cli.read_filter_line(info) == ("read filter: 1000 poly tails trimmed (A 1, C 2, G 990, T 7), 43210 bases removed, 3 reads left without a base; 100 reads removed "
                                          "(40 too short, 30 with too many N, 20 of low complexity, 10 of low quality), 9876 bases")
    assert cli.read_filter_line(zero_info()) == ("read filter: 0 poly tails trimmed (A 0, C 0, G 0, T 0), 0 bases removed, 0 reads left without a base; 0 reads removed "
                                                 "(0 too short, 0 with too many N, 0 of low complexity, 0 of low quality), 0 bases")
    assert cli._sum_filter_infos([info, info, zero_info()]) == {k: [2 * x for x in v] if isinstance(v, list) else 2 * v for k, v in info.items()}
    assert cli._sum_filter_infos([]) == zero_info()


def test_the_three_symbols_are_in_header_library_and_engine():
    lib = eng_mod.load_library()
    want = {"mlst_set_read_filter": [C.POINTER(C.c_uint32)], "mlst_get_read_filter": [C.POINTER(C.c_uint32)], "mlst_read_filter_info": [C.POINTER(C.c_uint64)]}
    for name, args in want.items():
        fn = getattr(lib, name)                                                          # AttributeError: the symbol is missing
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes[1:]) == args, (name, fn.argtypes)
    root = os.path.dirname(os.path.dirname(os.path.abspath(eng_mod.__file__)))
    text = open(os.path.join(root, "include", "mlst.h")).read()
    for line in ("typedef struct { uint32_t poly_mask, poly_min, min_length, max_n, complexity_pct, mean_qual; } mlst_read_filter;",
                 "int mlst_set_read_filter(mlst_handle* h, const mlst_read_filter* f);", "int mlst_get_read_filter(mlst_handle* h, mlst_read_filter* out);",
                 "int mlst_read_filter_info(mlst_handle* h, uint64_t out[16]);", "#define MLST_RF_NO_LIMIT 0xFFFFFFFFu"):
        assert line in text
    for name in ("set_read_filter", "get_read_filter", "read_filter_info"):
        assert callable(getattr(eng_mod.Engine, name))
