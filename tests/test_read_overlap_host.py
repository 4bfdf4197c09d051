"""fastq.pair_overlap / fastq.trim_pair_overlap, the rule mlst_set_read_pair_overlap applies on the device (include/mlst.h;
csrc/read_overlap.h), pinned by hand; the refusals of `cli type --pair-overlap`, each with its reason and before any GPU use; the four
symbols in header, library and engine.py; the command's line on fixed counters.  No GPU is needed."""
import ctypes as C
import os

import numpy as np
import pytest

from metamlst_amd import cli
from metamlst_amd import engine as eng_mod
from metamlst_amd.fastq import check_pair_overlap, pair_overlap, pair_overlap_median, trim_pair_overlap
from test_gpu_pair_bgzf import bgzf_blocks

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def letters(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


_rng = np.random.default_rng(2027)
FRAG = letters(_rng, 400)                  # a genome to cut fragments from
AD1, AD2 = letters(_rng, 340), letters(_rng, 340)      # what follows the insert on either mate (two different adapters)


def mates(insert: int, n1: int = 150, n2: int = 150, at: int = 0):
    """the mates of the fragment FRAG[at : at + insert]: the read runs through the insert into the adapter"""
    frag = FRAG[at:at + insert]
    return (frag + AD1)[:n1], (revcomp(frag) + AD2)[:n2]


def mutate(s: bytes, places) -> bytes:
    out = bytearray(s)
    for p in places:
        out[p:p + 1] = bytes(out[p:p + 1]).translate(bytes.maketrans(b"ACGT", b"CGTA"))
    return bytes(out)


def rec(name: str, seq: bytes, eol: bytes = b"\n", qual: bytes = None) -> bytes:
    return b"@" + name.encode() + eol + seq + eol + b"+" + eol + (qual if qual is not None else b"I" * len(seq)) + eol


def pair_text(m1: bytes, m2: bytes, eol: bytes = b"\n") -> bytes:
    return rec("p/1", m1, eol) + rec("p/2", m2, eol)


def seqs(text: bytes) -> list:
    return text.split(b"\n")[1::4]


def zero_info(**kw):
    out = {"pairs": 0, "overlapping": 0, "trimmed_pairs": 0, "reads_trimmed": 0, "bases_removed": 0, "emptied": 0, "insert_hist": [0] * 1024}
    hist = kw.pop("hist", {})
    out.update(kw)
    for k, v in hist.items():
        out["insert_hist"][k] = v
    return out


def brute(seq1: bytes, seq2: bytes, min_overlap=30, max_mismatches=5, error_permille=200):
    """the rule letter by letter"""
    fold = lambda s: bytes(c & 0xDF if (c & 0xDF) in b"ACGT" else 78 for c in s)      # noqa: E731
    s1, c2 = fold(seq1), fold(seq2).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    n1, n2 = len(s1), len(c2)
    best = None
    for o in range(-(n2 - min_overlap), n1 - min_overlap + 1):
        a, b = max(0, o), min(n1, o + n2)
        if b - a < min_overlap:
            continue
        m = sum(s1[p] == c2[p - o] and s1[p] != 78 for p in range(a, b))
        mism = (b - a) - m
        if mism <= max_mismatches and mism <= ((b - a) * error_permille) // 1000 and (best is None or m > best[1]):
            best = (o, m)
    return best


# ------------------------------------------------------------------ the offset
def test_a_pair_at_every_insert_of_one_150_base_fragment():
    """inserts 0 .. 330 of 150 / 150 mates: o = insert - 150; below min_overlap nothing is seen; from 271 on the mates no longer overlap
    over 30 bases"""
    for insert in range(0, 331):
        m1, m2 = mates(insert)
        got = pair_overlap(m1, m2)
        if 30 <= insert <= 270:
            L = min(insert, 150) - max(0, insert - 150)
            assert got == (insert - 150, L), (insert, got)
        else:
            assert got is None, (insert, got)
        out, info = trim_pair_overlap(pair_text(m1, m2))
        keep = min(150, insert) if 30 <= insert <= 270 else 150
        assert [len(s) for s in seqs(out)] == [keep, keep], insert
        assert seqs(out) == [m1[:keep], m2[:keep]]
        cut = 30 <= insert < 150
        assert info == zero_info(pairs=1, overlapping=int(30 <= insert <= 270), trimmed_pairs=int(cut), reads_trimmed=2 * cut,
                                 bases_removed=2 * (150 - insert) * cut, hist={insert: 1} if 30 <= insert <= 270 else {}), insert


def test_a_tail_of_one_base_is_found():
    m1, m2 = mates(149)
    out, info = trim_pair_overlap(pair_text(m1, m2))
    assert [len(s) for s in seqs(out)] == [149, 149] and info["bases_removed"] == 2


def test_the_overlap_length_at_29_30_31():
    for L, seen in ((29, False), (30, True), (31, True)):
        m1, m2 = mates(300 - L)                      # 150 / 150 mates of an insert of 300 - L overlap over L bases
        assert (pair_overlap(m1, m2) == (150 - L, L)) is seen and (pair_overlap(m1, m2) is None) is not seen, L
        m1, m2 = mates(L)                            # an insert of L bases: L letters of either mate
        assert (pair_overlap(m1, m2) == (L - 150, L)) is seen, L
    assert pair_overlap(FRAG[:29], revcomp(FRAG[:29])) is None      # a mate shorter than min_overlap has no candidate
    assert pair_overlap(FRAG[:30], revcomp(FRAG[:30])) == (0, 30)
    assert pair_overlap(FRAG[:29], revcomp(FRAG[:150])) is None and pair_overlap(FRAG[:150], revcomp(FRAG[:29])) is None


def test_five_and_six_mismatches_at_an_overlap_of_30():
    m1, m2 = mates(30)
    assert (30 * 200) // 1000 == 6                   # the permille bound allows six: the count decides
    assert pair_overlap(mutate(m1, (1, 6, 11, 16, 21)), m2) == (-120, 25)
    assert pair_overlap(mutate(m1, (1, 6, 11, 16, 21, 26)), m2) is None
    assert pair_overlap(m1, mutate(m2, (0, 5, 10, 20, 29))) == (-120, 25)
    assert pair_overlap(m1, mutate(m2, (0, 5, 10, 15, 20, 29))) is None
    assert pair_overlap(mutate(m1, (1, 6, 11, 16, 21, 26)), m2, max_mismatches=6) == (-120, 24)


def test_the_permille_bound_decides_at_an_overlap_of_10():
    m1, m2 = mates(10, 40, 40)
    assert (10 * 200) // 1000 == 2
    assert pair_overlap(mutate(m1, (2, 7)), m2, min_overlap=10) == (-30, 8)
    assert pair_overlap(mutate(m1, (2, 5, 7)), m2, min_overlap=10) is None          # three of ten: within max_mismatches, over the permille bound
    assert pair_overlap(mutate(m1, (2, 5, 7)), m2, min_overlap=10, error_permille=300) == (-30, 7)
    assert pair_overlap(mutate(m1, (2,)), m2, min_overlap=10, error_permille=99) is None      # 990 // 1000 = 0
    assert pair_overlap(m1, m2, min_overlap=10, error_permille=0, max_mismatches=0) == (-30, 10)


def test_an_n_on_either_mate_is_a_mismatch_and_so_is_n_against_n():
    m1, m2 = mates(60)

    def put(s, p, c=b"N"):
        return s[:p] + c + s[p + 1:]
    assert pair_overlap(m1, m2) == (-90, 60)
    assert pair_overlap(put(m1, 10), m2) == (-90, 59)
    assert pair_overlap(m1, put(m2, 10)) == (-90, 59)
    assert pair_overlap(put(m1, 10), put(m2, 49)) == (-90, 59)                      # base 10 of mate 1 lies on base 59 - 10 of mate 2: N against N
    assert pair_overlap(put(m1, 10, b"R"), put(m2, 49, b".")) == (-90, 59)          # every other byte is N
    assert pair_overlap(put(m1, 10), put(m2, 10)) == (-90, 58)
    assert pair_overlap(put(m1, 100), put(m2, 100)) == (-90, 60)                    # outside the overlap: no part
    six = m1
    for p in (3, 9, 20, 31, 32, 59):
        six = put(six, p)
    assert pair_overlap(six, m2) is None


def test_lower_case():
    m1, m2 = mates(100)
    assert pair_overlap(m1.lower(), m2) == pair_overlap(m1, m2.lower()) == pair_overlap(m1.lower(), m2.lower()) == (-50, 100)
    out, _ = trim_pair_overlap(pair_text(m1.lower(), m2))
    assert seqs(out) == [m1.lower()[:100], m2[:100]]                                # the letters stay what they are


def test_two_equally_good_offsets_the_smaller_wins():
    unit = b"ACGGTCATTGCA" * 20                      # a period of 12 whose reverse complement is another word
    m1, m2 = unit[:60], revcomp(unit[:60])
    got = pair_overlap(m1, m2, min_overlap=30)
    assert got == (0, 60)                            # the whole overlap beats the shifted ones
    m1, m2 = unit[:48], revcomp(unit[12:72])         # c2 = unit[12:72]: offsets -12 (36 matches) ... and every 12 bases
    by_hand = brute(m1, m2)
    assert pair_overlap(m1, m2) == by_hand
    same = b"AC" * 40                                # period 2: every even offset is exact, the longest overlap has the most matches
    assert pair_overlap(same[:50], revcomp(same[:50])) == (0, 50)
    # two offsets with the same number of matches: mate 1 = X Y X (X 40 letters), c2 = X -- o = 0 and o = 50 both match 40
    x, y = FRAG[200:240], FRAG[250:260]
    m1 = x + y + x
    assert pair_overlap(m1, revcomp(x)) == (0, 40) and brute(m1, revcomp(x)) == (0, 40)
    assert pair_overlap(mutate(m1, (5,)), revcomp(x)) == (50, 40)                   # one mismatch at the first: the second has more matches


def test_unequal_mate_lengths():
    for n1, n2, insert in ((150, 100, 120), (100, 150, 120), (320, 97, 200), (97, 320, 200), (320, 97, 60), (151, 149, 150), (33, 320, 33)):
        m1, m2 = mates(insert, n1, n2)
        got = pair_overlap(m1, m2)
        L = min(n1, insert) - max(0, insert - n2)
        assert got == (insert - n2, L) == brute(m1, m2), (n1, n2, insert)
        out, info = trim_pair_overlap(pair_text(m1, m2))
        assert [len(s) for s in seqs(out)] == [min(n1, insert), min(n2, insert)]
        assert info["reads_trimmed"] == (insert < n1) + (insert < n2) and info["insert_hist"][insert] == 1


def test_a_quality_trimmed_mate_2_lying_inside_mate_1():
    """an insert of 200, mate 2 trimmed to 60 bases: its reverse complement lies on bases 140 .. 199 of the fragment, of which mate 1
    holds 140 .. 149 -- too few; at an insert of 120 it lies on bases 60 .. 119, inside mate 1, and mate 1 is cut"""
    m1, m2 = mates(200, 150, 60)
    assert pair_overlap(m1, m2) is None
    m1, m2 = mates(120, 150, 60)
    assert pair_overlap(m1, m2) == (60, 60)
    out, info = trim_pair_overlap(pair_text(m1, m2))
    assert seqs(out) == [m1[:120], m2] and info == zero_info(pairs=1, overlapping=1, trimmed_pairs=1, reads_trimmed=1, bases_removed=30, hist={120: 1})
    m1, m2 = mates(300, 320, 40)                     # ... in the middle of a long mate 1: nothing to cut
    out, info = trim_pair_overlap(pair_text(m1, m2))
    assert pair_overlap(m1, m2) == (260, 40) and seqs(out) == [m1[:300], m2] and info["bases_removed"] == 20


def test_mates_that_overlap_in_their_middles_stay():
    m1, m2 = mates(220)
    out, info = trim_pair_overlap(pair_text(m1, m2))
    assert out == pair_text(m1, m2)
    assert info == zero_info(pairs=1, overlapping=1, hist={220: 1})


def test_trim5_lands_on_the_true_insert_end():
    """both mates lost six bases in front (--trim5 6): the cut is where the insert ends in the prepared mates"""
    for insert in (42, 90, 149):
        m1, m2 = mates(insert)
        p1, p2 = m1[6:], m2[6:]
        got = pair_overlap(p1, p2)
        assert got == (insert - 12 - 144, insert - 12)
        out, info = trim_pair_overlap(pair_text(p1, p2), trim5=6)
        assert seqs(out) == [m1[6:insert], m2[6:insert]], insert                    # the insert's own bases, none of the adapter
        assert info["insert_hist"][insert] == 1 and sum(info["insert_hist"]) == 1   # the fragment length in the file's coordinates
        assert info["bases_removed"] == 2 * (150 - insert)
        short, _ = trim_pair_overlap(pair_text(p1, p2))                             # without it the cut falls six bases short
        assert seqs(short) == [m1[6:insert - 6], m2[6:insert - 6]]


def test_an_empty_mate():
    m1, _ = mates(100)
    for a, b in ((m1, b""), (b"", m1), (b"", b"")):
        assert pair_overlap(a, b) is None
        out, info = trim_pair_overlap(pair_text(a, b))
        assert out == pair_text(a, b) and info == zero_info(pairs=1)


def test_crlf_text():
    m1, m2 = mates(100)
    out, info = trim_pair_overlap(pair_text(m1, m2, b"\r\n"))
    assert out == pair_text(m1[:100], m2[:100])      # line ends LF, sequence and quality lines both cut
    assert info["bases_removed"] == 100
    with pytest.raises(ValueError, match="not whole pairs"):
        trim_pair_overlap(rec("a", m1))
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        trim_pair_overlap(rec("a", m1, qual=b"II") + rec("b", m2))


def test_the_histogram_index_and_its_clamp():
    text = b"".join(pair_text(*mates(i)) for i in (30, 100, 100, 270, 20, 280))
    info = trim_pair_overlap(text)[1]
    assert info["pairs"] == 6 and info["overlapping"] == 4
    assert {k: v for k, v in enumerate(info["insert_hist"]) if v} == {30: 1, 100: 2, 270: 1}
    assert len(info["insert_hist"]) == 1024
    m1, m2 = mates(120)
    info = trim_pair_overlap(pair_text(m1[40:], m2[40:]), trim5=40)[1]               # o + n2 + 2 trim5 = the insert
    assert info["insert_hist"][120] == 1 and sum(info["insert_hist"]) == 1
    m1, m2 = mates(100)
    info = trim_pair_overlap(pair_text(m1, m2), trim5=461)[1]                        # 100 + 922 = 1022
    assert info["insert_hist"][1022] == 1
    for t5 in (462, 500, 60000):                     # 1023 and beyond: the last bin
        info = trim_pair_overlap(pair_text(m1, m2), trim5=t5)[1]
        assert info["insert_hist"][1023] == 1 and sum(info["insert_hist"]) == 1
    assert pair_overlap_median([0] * 1024) == 0
    assert pair_overlap_median(trim_pair_overlap(text)[1]["insert_hist"]) == 100
    hist = [0] * 1024
    hist[50], hist[60] = 2, 2
    assert pair_overlap_median(hist) == 50           # the lower median


def test_the_settings_that_are_refused():
    for bad, why in (({"min_overlap": 7}, "min_overlap 7 is outside 8..320"), ({"min_overlap": 321}, "min_overlap 321 is outside 8..320"),
                     ({"max_mismatches": -1}, "max_mismatches -1 is outside 0..64"), ({"max_mismatches": 65}, "max_mismatches 65 is outside 0..64"),
                     ({"error_permille": 501}, "error_permille 501 is outside 0..500"), ({"error_permille": -1}, "error_permille -1 is outside 0..500")):
        with pytest.raises(ValueError, match=why):
            check_pair_overlap(**bad)
        with pytest.raises(ValueError, match=why):
            pair_overlap(b"ACGT", b"ACGT", **bad)
    check_pair_overlap(8, 0, 0)
    check_pair_overlap(320, 64, 500)
    m1, m2 = mates(320, 320, 320)
    assert pair_overlap(m1, m2, min_overlap=320) == (0, 320)


def test_the_rule_against_a_letter_by_letter_walk():
    rng = np.random.default_rng(77)
    seen = 0
    for k in range(150):
        n1, n2 = (int(v) for v in rng.choice([0, 1, 29, 30, 31, 32, 33, 63, 64, 65, 97, 128, 150, 160, 320], size=2))
        insert = int(rng.integers(8, 400))
        m1, m2 = (bytearray(m) for m in mates(insert, n1, n2, at=int(rng.integers(0, 20)) if insert < 380 else 0))
        for m in (m1, m2):
            for _ in range(int(rng.choice([0, 0, 1, 3, 7]))):
                if m:
                    m[int(rng.integers(0, len(m)))] = int(rng.choice(list(b"ACGTNacgtn.")))
        setting = {"min_overlap": int(rng.choice([8, 10, 30, 30, 64])), "max_mismatches": int(rng.choice([0, 5, 5, 64])), "error_permille": int(rng.choice([0, 200, 200, 500]))}
        got = pair_overlap(bytes(m1), bytes(m2), **setting)
        assert got == brute(bytes(m1), bytes(m2), **setting), (k, n1, n2, insert, setting)
        seen += got is not None
    assert seen > 15


# ------------------------------------------------------------------ the command
def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r 1\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r 2\nACGT\n+\nIIII\n")
    (tmp_path / "u.fastq").write_bytes(b"@other 2\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    os.makedirs(tmp_path / "in")
    for k in range(2):
        (tmp_path / "in" / ("f%d.fastq" % k)).write_bytes(b"@r\nACGT\n+\nIIII\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    head = "--pair-overlap: "
    tail = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]
    for args, why in ((["s.fastq"], "it lays the mates of a pair on each other: give the second file with -2"),
                      (["s.fastq", "-2", "u.fastq"], "the records of s.fastq and u.fastq do not share their names, so the files go in as two unpaired texts and no read has a mate"),
                      (["s.fastq", "--alignments"], "with --alignments the file holds alignments, not mates to lay on each other"),
                      (["c.fa", "--contigs"], "--contigs cuts assemblies into windows, and a window has no mate"),
                      (["s.fastq", "--long-reads"], "--long-reads cuts unpaired reads into windows, and a window has no mate"),
                      ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts unpaired reads into windows, and a window has no mate"),
                      ([str(bam)], "the mates of a BAM are taken as they are stored: FASTQ input with -2 only"),
                      (["s.fastq", "t.fastq"], "several samples or a folder are typed without it"),
                      (["in"], "several samples or a folder are typed without it"),
                      (["s.fastq", "-2", "t.fastq", "--gpus", "2"], "one GPU: the counters of the ranks of --gpus N are not summed yet"),
                      (["s.fastq,t.fastq", "-2", "t.fastq"], "it takes one file of first mates and one of second mates (-2), not `a.fq,b.fq`")):
        monkeypatch.chdir(tmp_path)
        assert cli.main(["type"] + args + ["--pair-overlap"] + tail) == 1, args
        assert head + why in capsys.readouterr().out, args
    for flags, why in ((["--pair-overlap-min", "20"], "--pair-overlap-min belongs to --pair-overlap"),
                       (["--pair-overlap-diff", "2"], "--pair-overlap-diff belongs to --pair-overlap"),
                       (["--pair-overlap-rate", "0.1"], "--pair-overlap-rate belongs to --pair-overlap"),
                       (["--pair-overlap", "--pair-overlap-min", "7"], "--pair-overlap: min_overlap 7 is outside 8..320"),
                       (["--pair-overlap", "--pair-overlap-min", "321"], "--pair-overlap: min_overlap 321 is outside 8..320"),
                       (["--pair-overlap", "--pair-overlap-diff", "65"], "--pair-overlap: max_mismatches 65 is outside 0..64"),
                       (["--pair-overlap", "--pair-overlap-rate", "0.6"], "--pair-overlap: --pair-overlap-rate takes a number from 0 to 0.5, not 0.6")):
        assert cli.main(["type", "s.fastq", "-2", "t.fastq"] + flags + tail) == 1
        assert why in capsys.readouterr().out, flags
    # the flag with -2, and with what it goes with, gets past the checks
    for args in ([], ["--pair-overlap-min", "8", "--pair-overlap-diff", "0", "--pair-overlap-rate", "0.5"],
                 ["--trim5", "1", "--trim-qual", "20", "--phred64", "--adapter", "illumina", "--read-stats", "--dedup", "--write-sam", "--write-sam-all", "--write-reads", "--read-names"]):
        assert cli.main(["type", "s.fastq", "-2", "t.fastq", "--pair-overlap"] + args + tail) == 1
        assert capsys.readouterr().out.startswith("Failed to connect to the database"), args
    assert not os.path.exists(tmp_path / "o")


def test_the_commands_line_on_fixed_counters():
    hist = [0] * 1024
    hist[120], hist[140], hist[1023] = 200, 132, 1
    info = {"pairs": 1000, "overlapping": 333, "trimmed_pairs": 300, "reads_trimmed": 590, "bases_removed": 12345, "emptied": 0, "insert_hist": hist}
    assert cli.read_pair_overlap_line(info) == ("mate overlap trimming: 1000 pairs, 333 overlapping (33.3 %), 300 pairs cut (590 reads), 12345 bases removed, "
                                                "0 reads left without a base; median insert of the overlapping pairs 120")
    info.update(pairs=3, overlapping=2)
    assert "3 pairs, 2 overlapping (66.7 %)" in cli.read_pair_overlap_line(info)      # (2000 / 3 = 666.67 tenths of a percent: half up)
    info.update(pairs=0, overlapping=0, insert_hist=[0] * 1024)
    assert cli.read_pair_overlap_line(info) == "mate overlap trimming: 0 pairs, 0 overlapping (0.0 %), 300 pairs cut (590 reads), 12345 bases removed, 0 reads left without a base"
    text = b"".join(pair_text(*mates(i)) for i in (30, 100, 100, 270, 20, 280))
    assert cli.read_pair_overlap_line(trim_pair_overlap(text)[1]) == ("mate overlap trimming: 6 pairs, 4 overlapping (66.7 %), 3 pairs cut (6 reads), 440 bases removed, "
                                                                    "0 reads left without a base; median insert of the overlapping pairs 100")


def test_the_four_symbols_are_in_header_library_and_engine():
    lib = eng_mod.load_library()
    U32, P64 = C.c_uint32, C.POINTER(C.c_uint64)
    want = {"mlst_set_read_pair_overlap": [C.c_int, U32, U32, U32],
            "mlst_get_read_pair_overlap": [C.POINTER(C.c_int), C.POINTER(U32), C.POINTER(U32), C.POINTER(U32)],
            "mlst_read_pair_overlap_info": [P64], "mlst_read_pair_overlap_hist": [P64, C.c_uint64]}
    for name, args in want.items():
        fn = getattr(lib, name)                                                          # AttributeError: the symbol is missing
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes[1:]) == args, (name, fn.argtypes)
    root = os.path.dirname(os.path.dirname(os.path.abspath(eng_mod.__file__)))
    text = open(os.path.join(root, "include", "mlst.h")).read()
    for line in ("int mlst_set_read_pair_overlap(mlst_handle* h, int on, uint32_t min_overlap, uint32_t max_mismatches, uint32_t error_permille);",
                 "int mlst_get_read_pair_overlap(mlst_handle* h, int* on, uint32_t* min_overlap, uint32_t* max_mismatches, uint32_t* error_permille);",
                 "int mlst_read_pair_overlap_info(mlst_handle* h, uint64_t out[8]);",
                 "int mlst_read_pair_overlap_hist(mlst_handle* h, uint64_t* out, uint64_t cap);", "#define MLST_PO_HIST 1024"):
        assert line in text
    for name in ("set_read_pair_overlap", "get_read_pair_overlap", "read_pair_overlap_info"):
        assert callable(getattr(eng_mod.Engine, name))
