"""fastq.adapter_cut / trim_adapters: the rule mlst_set_read_adapters applies on the device (csrc/read_adapt.h), stated once in Python --
a 3' adapter inside the read or hanging over its 3' end, the start with the most matches within an integer error budget, one adapter per
read.  The rule is modelled on `cutadapt -a ADAPTER --no-indels`, is the project's own and claims none of cutadapt's bytes.  The known
answers here are worked out from the rule in include/mlst.h, and once more by a letter-by-letter walk, not taken from the function."""
import random

import pytest

from metamlst_amd.fastq import ADAPTER_NAMES, adapter_cut, check_adapters, prep_fastq, trim_adapters

INS = b"CTGACCGTTAGGCATTCAGGACCTTGAAACGTTGCAGTAC"
A = b"AGATCGGAAGAGC"
T = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
assert len(INS) == 40 and len(A) == 13 and len(T) == 33

# (read, adapters, new length, adapter or -1), all with min_overlap 3 and error_permille 100
KNOWN = [
    (INS + A + b"TTGCA", [A], 40, 0),
    (INS + b"AGA", [A], 40, 0),
    (INS + b"AG", [A], 42, -1),                                   # under min_overlap
    (INS + b"AGATCGCAAGAGC" + b"TT", [A], 40, 0),                 # 1 mismatch, L = 13, budget 1
    (INS + b"AGTTCGCAAGAGC" + b"TT", [A], 55, -1),                # 2 mismatches
    (INS + b"AGATCGCAA", [A], 49, -1),                            # L = 9, budget 0
    (INS + b"AGATCGCAAG", [A], 40, 0),                            # L = 10, budget 1
    (INS + b"AGATCGNAAGAGC", [A], 40, 0),                         # a read N is a mismatch, budget 1
    (INS + b"AGATCGNAA", [A], 49, -1),                            # budget 0
    (INS + b"AGATCGTAA", [b"AGATCGNAAGAGC"], 40, 0),              # an adapter N matches anything
    ((INS + A).lower(), [A], 40, 0),
    (A + INS, [A], 0, 0),                                         # emptied
    (INS[:10] + A + INS[10:20] + A, [A], 10, 0),                  # two exact ones: the leftmost
    (INS + b"AGATCGG", [b"AGATCGGTT", b"AGATCGGAA"], 40, 0),      # a tie goes to the first adapter
    (INS + T[:20], [A, T], 40, 1),                                # more matches
    (b"AGATCGCAAGAGC" + b"TTTT" + A, [A], 17, 0),                 # the exact one beats the leftmost
    (b"", [A], 0, -1),
    (b"AG", [A], 2, -1),
]


def walk(seq: bytes, adapters, min_overlap=3, error_permille=100):
    """the rule, letter by letter"""
    s = seq.upper()
    n = len(s)
    found = None      # (matches, p, k)
    for k, a in enumerate(adapters):
        for p in range(0, n - min(min_overlap, len(a)) + 1):
            L = min(len(a), n - p)
            matches = 0
            for i in range(L):
                if a[i:i + 1] == b"N" or (s[p + i:p + i + 1] in (b"A", b"C", b"G", b"T") and s[p + i] == a[i]):
                    matches += 1
            if L - matches <= (L * error_permille) // 1000:
                if found is None or matches > found[0] or (matches == found[0] and (p, k) < (found[1], found[2])):
                    found = (matches, p, k)
    return (n, -1) if found is None else (found[1], found[2])


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_the_known_answers(case):
    read, adapters, want_len, want_k = KNOWN[case]
    assert adapter_cut(read, adapters) == (want_len, want_k)
    assert walk(read, adapters) == (want_len, want_k)
    assert adapter_cut(read, b",".join(adapters).decode().lower()) == (want_len, want_k)      # one string, either case


def test_random_reads_against_the_walk():
    rng = random.Random(11)
    pick = lambda n, alpha: bytes(rng.choice(alpha) for _ in range(n))
    cut = 0
    for _ in range(1500):
        ads = []
        for _ in range(rng.choice([1, 1, 2, 3])):
            a = pick(rng.choice([1, 3, 5, 13, 33, 64]), b"ACGTACGTACGTN")
            ads.append(a if a.strip(b"N") else b"C" + a[1:])
        n = rng.choice([0, 1, 2, 3, 16, 40, 64, 65, 90])
        r = bytearray(pick(n, b"ACGTACGTACGTNacgtR"))
        if n and rng.random() < 0.7:
            a = bytearray(rng.choice(ads).replace(b"N", b"G"))
            for _ in range(rng.choice([0, 0, 1, 2])):
                a[rng.randrange(len(a))] = rng.choice(b"ACGTN")
            p = rng.randrange(n)
            r[p:p + len(a)] = a
            r = r[:n]
        mo, pm = rng.choice([1, 3, 3, 8, 64]), rng.choice([0, 100, 100, 250, 500])
        got = adapter_cut(bytes(r), ads, mo, pm)
        assert got == walk(bytes(r), ads, mo, pm), (bytes(r), ads, mo, pm)
        cut += got[1] >= 0
    assert 300 < cut < 1400


def rec(name: bytes, seq: bytes, qual: bytes, eol: bytes = b"\n") -> bytes:
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


def test_the_counters_and_the_text():
    reads = [r for r, ads, _, _ in KNOWN if ads == [A]]
    text = b"".join(rec(b"r%d extra" % k, r, bytes(33 + (7 * k + j) % 40 for j in range(len(r)))) for k, r in enumerate(reads))
    got, info = trim_adapters(text, [A])
    cuts = [adapter_cut(r, [A]) for r in reads]
    assert info == {"trimmed": sum(k >= 0 for _, k in cuts), "bases_removed": sum(len(r) - n for r, (n, _) in zip(reads, cuts)),
                    "emptied": 1, "per_adapter": [sum(k >= 0 for _, k in cuts)]}
    assert info["trimmed"] == 9 and info["bases_removed"] == 18 + 3 + 15 + 10 + 13 + 13 + 53 + 36 + 13      # (by hand, from KNOWN)
    assert got == b"".join(rec(b"r%d extra" % k, r[:n], bytes(33 + (7 * k + j) % 40 for j in range(n))) for k, (r, (n, _)) in enumerate(zip(reads, cuts)))
    # two adapters: the counts per adapter
    both = rec(b"a", INS + T[:20], b"I" * 60) + rec(b"b", INS + b"CTGTCTC", b"I" * 47) + rec(b"c", INS, b"I" * 40)
    got, info = trim_adapters(both, [ADAPTER_NAMES["illumina"], ADAPTER_NAMES["nextera"], T])
    assert info == {"trimmed": 2, "bases_removed": 27, "emptied": 0, "per_adapter": [0, 1, 1]}
    assert got == rec(b"a", INS, b"I" * 40) + rec(b"b", INS, b"I" * 40) + rec(b"c", INS, b"I" * 40)
    assert ADAPTER_NAMES == {"illumina": "AGATCGGAAGAGC", "nextera": "CTGTCTCTTATA", "smallrna": "TGGAATTCTCGG"}


def test_crlf_text_and_an_empty_read():
    text = rec(b"x", INS + A, b"F" * 53, b"\r\n") + rec(b"e", b"", b"", b"\r\n") + rec(b"y", A, b"#" * 13, b"\r\n")
    got, info = trim_adapters(text, [A])
    assert got == rec(b"x", INS, b"F" * 40) + rec(b"e", b"", b"") + rec(b"y", b"", b"")
    assert info == {"trimmed": 2, "bases_removed": 26, "emptied": 1, "per_adapter": [2]}
    assert trim_adapters(b"", [A]) == (b"", {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0]})
    with pytest.raises(ValueError, match="not a whole number of 4-line records"):
        trim_adapters(b"@r\nACGT\n+\n", [A])
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        trim_adapters(b"@r\nACGT\n+\nIII\n", [A])


def test_behind_the_quality_trim_the_cut_changes():
    """Phred base, fixed trims, quality trim, then adapters: a quality trim that removes half an adapter leaves an overlap whose error
    budget is smaller"""
    read = INS + b"AGATCGCAAGAGC" + b"TT"                  # one mismatch in 13: found on the whole read (budget 1)
    qual = [40] * 46 + [2] * 9                             # the quality trim leaves INS + AGATCG: L = 6, no mismatch, budget 0
    text = rec(b"r", read, bytes(v + 33 for v in qual))
    assert trim_adapters(text, [A])[0] == rec(b"r", INS, b"I" * 40)
    prepared, pinfo = prep_fastq(text, trim_qual=20)
    assert prepared == rec(b"r", read[:46], b"I" * 46) and pinfo["bases_removed"] == 9
    got, info = trim_adapters(prepared, [A])
    assert got == rec(b"r", INS, b"I" * 40) and info["bases_removed"] == 6
    qual = [40] * 49 + [2] * 6                             # ... leaves INS + AGATCGCAA: L = 9, one mismatch, budget 0 -- nothing is cut
    text = rec(b"r", read, bytes(v + 33 for v in qual))
    prepared, _ = prep_fastq(text, trim_qual=20)
    assert prepared == rec(b"r", read[:49], b"I" * 49)
    assert trim_adapters(prepared, [A]) == (prepared, {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0]})
    assert trim_adapters(text, [A])[1]["bases_removed"] == 15      # without the quality trim the adapter goes whole


def test_about_two_percent_of_random_reads_lose_bases_by_chance():
    """min_overlap 3, cutadapt's default and its known price: an exact 3-letter overlap at the 3' end alone has probability 1 / 64, and
    the longer ones add 1 / 256 + ...: about 1 / 48 of the reads.  Of 2,000 reads that is 42 +- 6.4 (one standard deviation)."""
    rng = random.Random(2026)
    hit = sum(adapter_cut(bytes(rng.choice(b"ACGT") for _ in range(150)), [A])[1] >= 0 for _ in range(2000))
    assert 20 <= hit <= 65, hit


@pytest.mark.parametrize("adapters,mo,pm,why", [
    (["AGAX"], 3, 100, "outside ACGTN"),
    (["AGA", "AC-GT"], 3, 100, "outside ACGTN"),
    (["NNNN"], 3, 100, "only N"),
    ([""], 3, 100, "1 to 64"),
    ("AGA,,ACG", 3, 100, "1 to 64"),
    (["A" * 65], 3, 100, "1 to 64"),
    (["ACGT"] * 9, 3, 100, "1 to 8"),
    ([], 3, 100, "1 to 8"),
    (["ACGT"], 0, 100, "min_overlap"),
    (["ACGT"], 65, 100, "min_overlap"),
    (["ACGT"], 3, 501, "error_permille"),
    (["ACGT"], 3, -1, "error_permille"),
])
def test_every_invalid_setting_is_a_value_error(adapters, mo, pm, why):
    for call in (lambda: check_adapters(adapters, mo, pm), lambda: adapter_cut(INS, adapters, mo, pm), lambda: trim_adapters(rec(b"r", INS, b"I" * 40), adapters, mo, pm)):
        with pytest.raises(ValueError, match=why):
            call()


def test_the_limits_are_taken():
    assert check_adapters(["a" * 64, "n" * 63 + "c"] + ["ACGTN"] * 6, 64, 500) == [b"A" * 64, b"N" * 63 + b"C"] + [b"ACGTN"] * 6
    assert check_adapters(b"acg,TTN", 1, 0) == [b"ACG", b"TTN"]
    assert adapter_cut(INS + b"A" * 64, ["A" * 64], 64, 0) == (40, 0)
    assert adapter_cut(INS + b"A" * 63, ["A" * 64], 64, 0) == (103, -1)      # the adapter must lie on 64 bases
