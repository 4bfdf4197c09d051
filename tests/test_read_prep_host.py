"""fastq.prep_fastq: the rule mlst_set_read_prep applies on the device (csrc/read_prep.h), stated once in Python -- Phred base, bowtie2's
fixed trims, the 3' quality trim of cutadapt -q / bwa aln -q, a read without a base stays a read.  The hand cases here are worked out
on paper from the rule in include/mlst.h, not taken from the function."""
import pytest

from metamlst_amd.fastq import prep_fastq, qtrim_len

ZERO = {"shortened": 0, "bases_removed": 0, "emptied": 0}

# (Phred values, how many remain with T = 20)
HAND = [
    ([30, 30, 10, 30, 10, 10], 4),          # sums 10, 20, 10, 20 (a tie: the cut stays), 10, 0
    ([30, 30, 10, 10, 30, 10, 10], 2),      # 10, 20, 10, 20, 30 (the sum dips and recovers), 20, 10
    ([5, 40, 40, 10], 3),                   # 10, then -10: the walk ends, the 5 in front is never seen
    ([20, 25, 40, 20], 4),                  # all >= 20: the sum never rises above 0
    ([19, 0, 3, 19], 0),                    # all < 20: the sum rises all the way
    ([], 0),
    ([19], 0),
    ([20], 1),
]


def phred(q, base=33) -> bytes:
    return bytes(v + base for v in q)


def rec(name: bytes, seq: bytes, qual: bytes, eol: bytes = b"\n") -> bytes:
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


@pytest.mark.parametrize("q,want", HAND)
def test_the_quality_trim_by_hand(q, want):
    assert qtrim_len(q, 20) == want
    assert qtrim_len(q, 0) == len(q)
    seq = (b"ACGT" * 4)[:len(q)]
    text, info = prep_fastq(rec(b"r", seq, phred(q)), trim_qual=20)
    assert text == rec(b"r", seq[:want], phred(q[:want]))
    assert info == {"shortened": int(want != len(q)), "bases_removed": len(q) - want, "emptied": int(want == 0 and len(q) > 0)}
    # the same values under Phred+64 come out as Phred+33 characters
    text64, info64 = prep_fastq(rec(b"r", seq, phred(q, 64)), trim_qual=20, phred64=True)
    assert text64 == text and info64 == info


def test_the_quality_trim_sees_what_the_fixed_trims_leave():
    q = [30, 30, 10, 30, 10, 10]
    # trim3 = 2 removes the two 10s; of [30, 30, 10, 30] nothing more goes: the sum starts at -10
    assert prep_fastq(rec(b"r", b"ACGTAC", phred(q)), trim3=2, trim_qual=20)[0] == rec(b"r", b"ACGT", phred(q[:4]))
    # trim5 = 3 leaves [30, 10, 10]: sums 10, 20, 10 -> one base remains, base 3 of the read
    text, info = prep_fastq(rec(b"r", b"ACGTAC", phred(q)), trim5=3, trim_qual=20)
    assert text == rec(b"r", b"T", phred([30])) and info == {"shortened": 1, "bases_removed": 5, "emptied": 0}


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 40])
def test_fixed_trim_arithmetic(n):
    seq, q = (b"ACGTTGCA" * 5)[:n], list(range(2, 2 + n))
    for t5, t3 in [(0, 0), (3, 0), (0, 3), (3, 4), (n, 0), (0, n), (n + 5, 0), (0, n + 5)] + [(a, s - a) for s in (n - 1, n, n + 1) if s >= 0 for a in (0, s // 2, s)]:
        a, n1 = min(t5, n), max(0, n - t5 - t3)
        text, info = prep_fastq(rec(b"x y", seq, phred(q)), trim5=t5, trim3=t3)
        assert text == rec(b"x y", seq[a:a + n1], phred(q[a:a + n1])), (t5, t3)
        assert info == {"shortened": int(n1 != n), "bases_removed": n - n1, "emptied": int(n1 == 0 and n > 0)}, (t5, t3)
    # trim5 + trim3 = n - 1 leaves exactly one base, at index trim5
    if n >= 1:
        for t5 in range(n):
            assert prep_fastq(rec(b"x", seq, phred(q)), trim5=t5, trim3=n - 1 - t5)[0] == rec(b"x", seq[t5:t5 + 1], phred(q[t5:t5 + 1]))


def test_trim5_larger_than_the_read_alone():
    text, info = prep_fastq(rec(b"a", b"ACGTA", b"IIIII") + rec(b"b", b"ACGTACGTAC", b"IIIIIIIIII"), trim5=7)
    assert text == rec(b"a", b"", b"") + rec(b"b", b"TAC", b"III")
    assert info == {"shortened": 2, "bases_removed": 12, "emptied": 1}


def test_phred64_and_the_clamp_below_the_base():
    qual = bytes([64, 66, 104, 63, 33, 59, 126, 127, 200, 255])      # '@' B h, three bytes below '@', '~', DEL, two high bytes
    want = [0, 2, 40, 0, 0, 0, 62, 63, 127, 127]
    text, info = prep_fastq(rec(b"r", b"ACGTACGTAC", qual), phred64=True)
    assert text == rec(b"r", b"ACGTACGTAC", bytes(v + 33 for v in want)) and info == ZERO
    # under Phred+33 the same bytes: 31 more each, clamped at 127; a byte below '!' is Phred 0
    text33, _ = prep_fastq(rec(b"r", b"ACG", bytes([32, 10 + 33, 161])))
    assert text33 == rec(b"r", b"ACG", bytes([33, 43, 160]))
    # a Q2 tail ('B' under Phred+64) goes under --trim-qual with the right base and stays with the wrong one
    r = rec(b"r", b"ACGTACGT", b"hhhhhBBB")
    assert prep_fastq(r, trim_qual=20, phred64=True)[0] == rec(b"r", b"ACGTA", b"IIIII")
    assert prep_fastq(r, trim_qual=20)[0] == r


def test_crlf_input_and_a_last_record_without_a_newline():
    q = [30, 30, 10, 30, 10, 10]
    lf = rec(b"a 1", b"ACGTAC", phred(q)) + rec(b"b", b"", b"") + rec(b"c", b"GGGTTT", phred(q))
    crlf = rec(b"a 1", b"ACGTAC", phred(q), b"\r\n") + rec(b"b", b"", b"", b"\r\n") + rec(b"c", b"GGGTTT", phred(q), b"\r\n")
    want = rec(b"a 1", b"CGT", phred(q[1:4])) + rec(b"b", b"", b"") + rec(b"c", b"GGT", phred(q[1:4]))
    for text in (lf, crlf, lf[:-1], crlf[:-2], crlf[:-1]):
        got, info = prep_fastq(text, trim5=1, trim_qual=20)
        assert got == want and info == {"shortened": 2, "bases_removed": 6, "emptied": 0}
    assert prep_fastq(b"") == (b"", ZERO)
    with pytest.raises(ValueError):
        prep_fastq(b"@a\nACGT\n+\nIII\n")
    with pytest.raises(ValueError):
        prep_fastq(b"@a\nACGT\n+\n")


def test_header_and_plus_line_are_not_touched():
    text = b"@name with spaces\tand a TAB 1:N:0\nACGTN\n+name again\nIIII#\n"
    assert prep_fastq(text, trim5=1, trim3=1)[0] == b"@name with spaces\tand a TAB 1:N:0\nCGT\n+name again\nIII\n"


def test_counters_over_a_file():
    recs = [(b"ACGTACGTAC", [40] * 10), (b"ACG", [40] * 3), (b"", []), (b"ACGTACGT", [40, 40, 40, 40, 40, 2, 2, 2]), (b"AC", [2, 2]), (b"ACGTA", [40] * 5)]
    text = b"".join(rec(b"r%d" % k, s, phred(q)) for k, (s, q) in enumerate(recs))
    got, info = prep_fastq(text, trim5=2, trim3=1, trim_qual=20)
    # lengths 10 -> 7, 3 -> 0, 0 -> 0 (unchanged: neither shortened nor emptied), 8 -> 5 - 2 = 3 (the Q2 tail), 2 -> 0, 5 -> 2
    want = [7, 0, 0, 3, 0, 2]
    assert got == b"".join(rec(b"r%d" % k, s[2:2 + n], phred(q[2:2 + n])) for k, ((s, q), n) in enumerate(zip(recs, want)))
    assert info == {"shortened": 5, "bases_removed": 10 + 3 + 8 + 2 + 5 - sum(want), "emptied": 2}
    assert prep_fastq(text) == (text, ZERO)


def test_prepared_text_is_a_fixed_point_of_the_defaults():
    q = [0, 2, 40, 41, 62, 20, 19, 2, 2, 2]
    text = rec(b"a", b"ACGTNACGTA", phred(q, 64), b"\r\n") + rec(b"b", b"ACG", bytes([50, 63, 64]), b"\r\n")
    once, _ = prep_fastq(text, phred64=True)
    assert once != text and prep_fastq(once) == (once, ZERO)
    trimmed, _ = prep_fastq(text, trim5=1, trim3=1, trim_qual=20, phred64=True)
    assert prep_fastq(trimmed) == (trimmed, ZERO)
    # and preparing the prepared text with the same trims' quality step changes nothing more: the rule leaves no tail it would cut
    assert prep_fastq(trimmed, trim_qual=20)[0] == trimmed


def test_negative_settings_are_refused():
    for kw in ({"trim5": -1}, {"trim3": -1}, {"trim_qual": -1}):
        with pytest.raises(ValueError):
            prep_fastq(b"", **kw)
