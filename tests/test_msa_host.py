"""metamlst_amd.msa.center_star, the written rule of the engine's centre-star alignment (include/mlst.h, mlst_msa_align): its properties,
hand-written cases with one optimum, the tie rule in homopolymers, its refusals, and write_sequences(..., aligner=...) on a tiny
database whose species has a locus with alleles of different lengths (the branch that needed MUSCLE)."""
import pytest

import msa_cases as mc
from metamlst_amd import merge
from metamlst_amd.msa import center_star, pick_center

A = b"GATTACAGCTC"        # no base repeats next to the places the cases below cut or fill, so every case has one optimum


def statement_aligner(seqs):
    """The statement with _muscle's contract: [(id, sequence)] -> {id: aligned sequence}."""
    _, rows = center_star([q.encode() for _, q in seqs])
    return dict((i, r.decode()) for (i, _), r in zip(seqs, rows))


def test_properties_on_a_family():
    seqs = mc.family(40, 120, seed=7) + [b"acgtn" * 20, b"N" * 30]
    c, rows = center_star(seqs)
    assert len(set(map(len, rows))) == 1
    assert [r.replace(b"-", b"") for r in rows] == seqs             # letters and case kept
    assert c == pick_center(seqs) and rows[c].replace(b"-", b"") == seqs[c]
    m = len(seqs[c])
    assert len(rows[0]) >= m and any(len(q) != m for q in seqs)


def test_identical_sequences_get_no_gaps():
    assert center_star([A, A, A]) == (0, [A, A, A])
    assert center_star([A]) == (0, [A])                             # n = 1: the sequence itself
    assert center_star([A.lower(), A]) == (0, [A.lower(), A])       # lower case matches its upper case


def test_centre_rule():
    assert pick_center([b"ACG", b"ACGT", b"TCGT", b"AC"]) == 1      # most frequent length, first of it in input order
    assert pick_center([b"AC", b"GT", b"ACG", b"ACT"]) == 2         # lengths 2 and 3 come twice each: the greater
    assert pick_center([b"ACGT", b"ACGTA"]) == 1                    # every length once: the greatest
    assert pick_center([b"ACGTA", b"ACGT", b"ACGTC"]) == 0
    assert center_star([b"ACGT", b"ACGTA"])[0] == 1


@pytest.mark.parametrize("seqs, want", [
    # a G filled in between A and C
    ([A, b"GATTAGCAGCTC", A], [b"GATTA-CAGCTC", b"GATTAGCAGCTC", b"GATTA-CAGCTC"]),
    # the A between T and C cut out
    ([A, b"GATTCAGCTC", A], [b"GATTACAGCTC", b"GATT-CAGCTC", b"GATTACAGCTC"]),
    # an insertion in front of the first column, and one behind the last
    ([A, b"T" + A, A], [b"-" + A, b"T" + A, b"-" + A]),
    ([A, A + b"GG", A], [A + b"--", A + b"GG", A + b"--"]),
    # two rows fill the same slot with one and with two bases: stacked from the left, not aligned to each other
    ([A, b"GATTAGGCAGCTC", b"GATTATCAGCTC", A], [b"GATTA--CAGCTC", b"GATTAGGCAGCTC", b"GATTAT-CAGCTC", b"GATTA--CAGCTC"]),
    # a deletion and an insertion in one row, apart
    ([A, b"GTTACAGAACTC", A], [b"GATTACAG--CTC", b"G-TTACAGAACTC", b"GATTACAG--CTC"]),
])
def test_cases_with_one_optimum(seqs, want):
    assert center_star(seqs) == (0, want)


def test_ties_in_a_homopolymer():
    # AAA against the centre AAAA: every placement of the one gap scores 3 * 5 - 11 = 4.  At [3][4] M = 5 + H[2][3] = 4 and D = M[3][3] - 11
    # = 4: M is listed first and ends the path.  On the way back H[2][3] and H[1][2] are ties of M and D too (both -1, both -6) and
    # M wins again, until M[1][2] = 5 + H[0][1], whose only real source is the border's D[0][1]: the gap lands on column 1.
    assert center_star([b"AAAA", b"AAA"]) == (0, [b"AAAA", b"-AAA"])
    # AAAA against the centre AAA, the mirror image: M wins the ties down to M[2][1] = 5 + H[1][0], the border's I[1][0]: the spare A
    # is the insertion in front of column 1.
    assert center_star([b"AAA", b"AAAA", b"AAA"]) == (0, [b"-AAA", b"AAAA", b"-AAA"])


def test_n_matches_nothing():
    # N on N costs a mismatch, as N on A does: one N is a mismatch column, not a gap (-4 against -22)
    assert center_star([b"GATNACA", b"GATNACA"]) == (0, [b"GATNACA", b"GATNACA"])
    # a run of 14 N against itself: 14 mismatches cost 56, a deletion and an insertion of 14 cost 24 + 24, and mismatching k of them
    # only adds 2 k.  Deletion first or insertion first score the same: the M of the first C takes max(M, I, D)[19][19], where I (the
    # path that ends with the insertion) is listed before D.  So the row's N fill the slot behind column 19, its columns 6..19 are gaps.
    q = b"AAAAA" + b"N" * 14 + b"CCCCC"
    assert center_star([q, q]) == (0, [b"AAAAA" + b"N" * 14 + b"-" * 14 + b"CCCCC", b"AAAAA" + b"-" * 14 + b"N" * 14 + b"CCCCC"])


@pytest.mark.parametrize("seqs", [[], [b""], [A, b""], [b"A" * 4096], [b"AC-T"], [b"AC T"], [b"AC1T"], [b"ACGT\n"], [A, b"AC*T"]])
def test_refusals(seqs):
    with pytest.raises(ValueError):
        center_star(seqs)


def test_longest_sequence_is_taken():
    q = mc.rand_seq(4095, 5)
    assert center_star([q])[1] == [q]


def test_write_sequences_with_an_aligner(tmp_path):
    """Format A on a species with a length-variant locus, without MUSCLE: every record has the same length and is, without its gaps,
    the concatenation of its profile's allele sequences."""
    tables, records = mc.merge_tiny(str(tmp_path), statement_aligner)
    want = mc.expected_concatenations(tables)
    assert len(records) == 3 and len(set(len(s) for _, s in records)) == 1
    assert len(records[0][1]) == 60 + (72 + 5) + 66 and sum("-" in s for _, s in records) == 2      # g2: its 72 columns and the one slot of 5
    seen = set()
    for rid, seq in records:
        st = int(rid.split("_ST")[1].split("_")[0])
        assert seq.replace("-", "") == want[st], rid
        seen.add(st)
    assert {3, 4} < seen and len(seen) == 3                                                  # two known STs and the sample's new profile


def test_without_an_aligner_the_branch_still_asks_for_muscle(tmp_path, monkeypatch):
    monkeypatch.setattr(merge.shutil, "which", lambda name: None)
    with pytest.raises(RuntimeError, match="MUSCLE is needed"):
        mc.merge_tiny(str(tmp_path), None)


def test_cli_merge_has_the_aligner_switch():
    import argparse

    from metamlst_amd import cli
    p = cli._merge_parser(argparse.ArgumentParser().add_subparsers())
    assert p.parse_args(["out", "-d", "db"]).aligner == "auto"
    assert [p.parse_args(["out", "-d", "db", "--aligner", k]).aligner for k in ("gpu", "muscle", "auto")] == ["gpu", "muscle", "auto"]
    with pytest.raises(SystemExit):
        p.parse_args(["out", "-d", "db", "--aligner", "clustal"])
