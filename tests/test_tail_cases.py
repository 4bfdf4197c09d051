"""The crafted inputs of the typing tail (tests/tail_cases.py) on the CPU: the database has the loci it was built for at the
positions it was built for, every statistics case puts its winner, its tie partners and its largest depth where it says (in that
wave and turn of k_choose), and the two host statements of the allele choice agree on every case they can both read."""
import numpy as np
import pytest

import tail_cases as tc
from metamlst_amd.typing import consensus_from_counts


@pytest.fixture(scope="module")
def cp():
    return tc.corpus()


def test_database_has_its_loci_where_the_kernels_turn(cp):
    ix = cp.idx
    assert ix.n_loci == tc.N_LOCI == 1024 + 6
    for pos, (tag, n, length) in tc.NAMED.items():
        l = ix.locus_index(tc.SPA, tc.gene_name(pos))
        assert l == pos == cp.position(tag)                       # positions come from the loaded index
        assert int(ix.locus_count[l]) == n and int(ix.locus_maxlen[l]) == length, tag
    assert {0, 1023, 1024} <= set(tc.NAMED) and cp.position("dup") == tc.DUP_POS == ix.n_loci - 1
    assert {int(ix.locus_count[p]) for p in tc.NAMED} == {1, 3, 8, 63, 64, 65, 255, 256, 257, 513, 1025}
    assert {40, 255, 256, 257, 600} == {int(x) for x in ix.locus_maxlen}
    l = cp.position("ragged")
    b = int(ix.locus_begin[l])
    lens = {int(ix.allele_no[a]): int(ix.off[a + 1] - ix.off[a]) for a in range(b, b + int(ix.locus_count[l]))}
    assert lens == tc.RAGGED_LEN and min(lens.values()) == 40 and max(lens.values()) == 600
    for pos in tc.WIDE_FILLERS:
        assert int(ix.locus_maxlen[pos]) == 257 and int(ix.locus_count[pos]) == 2


def test_the_repeated_number_sits_in_threads_255_and_0(cp):
    """Rows in (number, row) order: numbers 1..255, 256 twice, 257..512 -- the pair at rows 255 and 256, so the higher index is in
    the LOWER thread of k_choose."""
    ix = cp.idx_dup
    assert ix.n_loci == 1 and int(ix.locus_count[0]) == tc.DUP_ROWS >= 513
    assert tc.numbers(ix, 0) == list(range(1, 256)) + [256, 256] + list(range(257, 513))
    k1, k2 = tc.duplicate_pair(ix, 0)
    assert (k1, k2) == (255, 256) and k2 % 256 < k1 % 256
    assert tc.where(k1) == (3, 0) and tc.where(k2) == (0, 1)
    case = tc.dup_case(ix, 0)
    assert tc.choice_fast(ix, case, 100) == {0: k1}               # the first visited: the lower index
    l = cp.position("dup")                                         # the same rows inside the whole database, in similarity order
    assert sorted(tc.numbers(cp.idx, l)) == sorted(tc.numbers(ix, 0)) and tc.has_duplicates(cp.idx, l)
    assert [m for m in range(cp.idx.n_loci) if tc.has_duplicates(cp.idx, m)] == [l]


def test_the_cases_are_the_ones_asked_for(cp):
    names = [c.name for c in cp.cases]
    for at in tc.WINNER_AT:
        assert "winner_at_%s" % at in names
    for place in tc.PLACEMENTS:
        for order in ("lower_number_first", "lower_number_second"):
            assert "tie/%s/%s" % (place, order) in names
    for pattern in tc.PRESENCE:
        assert "presence/%s" % pattern in names
    for name in ("tie/three_waves/lowest_in_0", "tie/three_waves/lowest_in_1", "tie/three_waves/lowest_in_2", "mx_in_wave3", "mx_in_last_turn",
                 "hits_only_from_256_on", "single_hit_allele", "alternating/even", "alternating/odd", "extremes/positive", "extremes/negative",
                 "duplicate_number_tie"):
        assert name in names
    assert [c.name for c in cp.cases if c.dup] == ["duplicate_number_tie"]
    for c in cp.cases:                                             # the sentinel exactly where a locus has no hit
        hit = np.add.reduceat(c.n_hits, cp.idx.locus_begin.astype(np.intp)) > 0
        assert np.array_equal(c.locus_first != tc.SENTINEL, hit), c.name
        assert int(c.n_hits.max(initial=0)) <= tc.M32 and int(np.abs(c.sum_score).max(initial=0)) <= max(1 << 44, 10 ** 9 + 2000)


def test_unique_winners_sit_in_every_wave_and_turn(cp):
    ix = cp.idx
    for at in tc.WINNER_AT:
        case = cp.case("winner_at_%s" % at)
        want = {l for l in range(ix.n_loci) if at == "last" or int(ix.locus_count[l]) > at}
        assert set(case.expect) == want and want
        for l, e in case.expect.items():
            k = int(ix.locus_count[l]) - 1 if at == "last" else at
            assert e["winner"] == k and tc.where(k) == (k % 256 // 64, k // 256)
    seen = {tc.where(e["winner"]) for at in tc.WINNER_AT for e in cp.case("winner_at_%s" % at).expect.values()}
    assert {(w, 0) for w in range(4)} | {(0, 1), (3, 1), (0, 2), (0, 4)} <= seen
    # indices 0 .. 512 exist in the loci of 513 and 1,025 alleles; n - 1 of the latter is the fifth turn
    assert cp.case("winner_at_512").expect.keys() == {cp.position("n513"), cp.position("n1025"), cp.position("dup")}
    assert cp.case("winner_at_last").expect[cp.position("n1025")]["winner"] == 1024


def test_tie_partners_sit_where_the_case_says(cp):
    ix = cp.idx
    for place in tc.PLACEMENTS:
        for order in ("lower_number_first", "lower_number_second"):
            case = cp.case("tie/%s/%s" % (place, order))
            for l, e in case.expect.items():
                no = tc.numbers(ix, l)
                i, j = e["partners"]
                (wi, ti), (wj, tj) = tc.where(i), tc.where(j)
                assert i < j and no[i] != no[j] and (no[i] < no[j]) == (order == "lower_number_first")
                assert e["winner"] == (i if no[i] < no[j] else j)
                b = int(ix.locus_begin[l])
                assert case.n_hits[b + i] == case.n_hits[b + j] == 100 and {int(case.sum_score[b + i]), int(case.sum_score[b + j])} == {30010, 30014}
                if place == "same_thread_two_turns":
                    assert i % 256 == j % 256 and tj == ti + 1
                elif place == "two_lanes_of_one_wave":
                    assert (wi, ti) == (wj, tj) and i % 64 != j % 64
                elif place == "wave0_vs_wave3":
                    assert (wi, wj) == (0, 3) and ti == tj
                else:
                    assert (ti, tj) == (0, 4) and int(ix.locus_count[l]) == 1025
    both = [set(cp.case("tie/%s/%s" % (place, o)).expect) for place in tc.PLACEMENTS for o in ("lower_number_first", "lower_number_second")]
    n513, n1025 = cp.position("n513"), cp.position("n1025")
    assert all(n1025 in s for s in both) and all(n513 in s for s in both[:6])           # both orders exist where it matters
    assert any(tc.where(cp.case("tie/wave0_vs_wave3/lower_number_first").expect[l]["partners"][0])[1] == 1 for l in (n513, n1025))
    for lowest in (0, 1, 2):
        case = cp.case("tie/three_waves/lowest_in_%d" % lowest)
        assert {n513, n1025, cp.position("n255"), cp.position("n256"), cp.position("n257")} <= set(case.expect)
        for l, e in case.expect.items():
            no = tc.numbers(ix, l)
            waves = [tc.where(k)[0] for k in e["partners"]]
            assert len(set(waves)) == 3 and waves[0] == 0 and waves[1] == 1
            assert min(e["partners"], key=lambda k: no[k]) == e["partners"][lowest] == e["winner"]


def test_the_largest_depth_is_far_from_the_winner(cp):
    ix = cp.idx
    for name in ("mx_in_wave3", "mx_in_last_turn"):
        case = cp.case(name)
        assert case.expect
        want100, want3 = tc.choice_fast(ix, case, 100), tc.choice_fast(ix, case, 3)
        for l, e in case.expect.items():
            b, n = int(ix.locus_begin[l]), int(ix.locus_count[l])
            mx = e["mx"]
            assert int(case.n_hits[b:b + n].argmax()) == mx and int(case.n_hits[b + mx]) == 1000
            assert (tc.where(mx)[0] == 3) if name == "mx_in_wave3" else (tc.where(mx)[1] == (n - 1) // 256 >= 1)
            assert want100[l] == b + e["winner_at_100"] != b + mx and tc.where(e["winner_at_100"]) == (0, 0)
            assert want3[l] == b + 70 and tc.where(70) == (1, 0)                # without the full penalty the allele in wave 1 wins
            local = case.sum_score[b:b + n] - (1000 - case.n_hits[b:b + n]) * 100
            assert int((local[case.n_hits[b:b + n] > 0] < 0).sum()) >= n // 3 - 2    # the floor-division branch of round_tenths


def test_both_host_statements_agree_on_every_case(cp):
    """compile_cel + pick_alleles (the literal restatement of metamlst.py:133-151, 244) and pick_alleles_fast give the same
    label for every locus, on every case and locus the literal one can read: it keys the alleles of a locus by their number
    (geneInfo[str(no)]), so two rows of one number are one entry to it, and the locus of the repeated number is left out."""
    ix = cp.idx
    rep = cp.position("dup")
    for case in cp.cases:
        if case.dup:
            continue
        for penalty in tc.PENALTIES:
            fast = tc.choice_fast(ix, case, penalty)
            literal = tc.choice_literal(ix, case, penalty)
            assert set(fast) == set(literal)
            assert {l: ix.label(a) for l, a in fast.items() if l != rep} == {l: v for l, v in literal.items() if l != rep}, (case.name, penalty)
            assert sorted(fast) == case.chosen_loci()
            for l, e in case.expect.items():
                if l != "missing" and "winner" in e:
                    assert fast[l] == int(ix.locus_begin[l]) + e["winner"], (case.name, penalty, l)
        if "missing" in case.expect:
            assert set(range(ix.n_loci)) - set(case.chosen_loci()) == case.expect["missing"]


def test_presence_patterns(cp):
    n = cp.idx.n_loci
    assert tc.missing_loci("none_missing", n) == set() and tc.missing_loci("all_missing", n) == set(range(n))
    for k in (0, 1023, 1024, 1029):
        assert tc.missing_loci("missing_%d" % k, n) == {k}
    assert tc.missing_loci("missing_first_turn", n) == set(range(1024)) and tc.missing_loci("missing_second_turn", n) == set(range(1024, 1030))
    assert tc.missing_loci("missing_even", n) | tc.missing_loci("missing_odd", n) == set(range(n))


def test_compact_model_reproduces_the_fixed_layout_when_every_locus_is_chosen(cp):
    ix = cp.idx
    cb = tc.fixed_colbase(ix)
    base, need = tc.compact_layout(cb, range(ix.n_loci))
    assert need == int(cb[-1]) == int(ix.locus_maxlen.sum()) and [base[l] for l in range(ix.n_loci)] == [int(x) for x in cb[:-1]]
    assert np.array_equal(tc.compact_counts(tc.counts_fixed(), cb, range(ix.n_loci)), tc.counts_fixed())
    base, need = tc.compact_layout(cb, [5, 1024, 700])
    assert base == {5: 0, 700: 40, 1024: 640} and need == 680
    assert tc.compact_layout(cb, []) == ({}, 0)
    some = tc.compact_counts(tc.counts_fixed(), cb, [700, 1024])
    assert np.array_equal(some[:600], tc.counts_fixed()[int(cb[700]):int(cb[701])]) and len(some) == 640


def test_every_counts_pattern_lands_on_both_sides_of_column_256(cp):
    ix = cp.idx
    pats = tc.count_patterns()
    names = [n for n, _ in pats]
    assert len(pats) <= len(tc.WIDE_FILLERS)
    for want in ["zero"] + ["single_" + b for b in "ACGT"] + ["tie_" + t for t in ("AC", "AG", "AT", "CG", "CT", "GT", "ACG", "ACT", "AGT", "CGT", "ACGT")] \
            + ["total_1", "total_2", "total_7999", "total_8000"] + ["max_" + b for b in "ACGT"] + ["sum_max_G", "sum_max_T"]:
        assert want in names
    by = dict(pats)
    assert sum(by["total_7999"]) == 7999 and sum(by["total_8000"]) == 8000 and sum(by["total_1"]) == 1 and sum(by["total_2"]) == 2
    assert sum(by["sum_max_G"]) == sum(by["sum_max_T"]) == tc.M32 and max(sum(p) for p in by.values()) == tc.M32      # never 2^32 or more
    assert "".join(consensus_from_counts(np.array([by["tie_ACGT"], by["tie_CGT"], by["tie_GT"], by["sum_max_T"]], np.uint32))) == "ACGT"
    cb = tc.fixed_colbase(ix)
    counts = tc.counts_fixed()
    at = {"below": set(), 255: set(), 256: set(), "above": set()}
    for l in range(ix.n_loci):
        w = int(cb[l + 1] - cb[l])
        for c in range(w):
            p = tc.pattern_of_column(l, c, len(pats))
            at["below" if c < 255 else "above" if c > 256 else c].add(p)
        assert tuple(int(x) for x in counts[int(cb[l]) + w - 1]) == pats[tc.pattern_of_column(l, w - 1, len(pats))][1]
    assert all(s == set(range(len(pats))) for s in at.values()), {k: len(s) for k, s in at.items()}


def test_letters_model_pieces(cp):
    ix = cp.idx
    cb = tc.fixed_colbase(ix)
    for mincov, none_char in ((0, "N"), (1, "-"), (8000, "N")):
        chosen = [0, 700, 1029]
        want = tc.letters_model(tc.counts_fixed(), cb, chosen, mincov, none_char)
        assert np.array_equal(tc.letters_of_corpus(chosen, mincov, none_char), want)
        empty = want[int(cb[1]):int(cb[2])]                        # a locus without a chosen allele: what zero counts give
        assert set(empty.tolist()) == ({ord("A")} if mincov == 0 else {ord(none_char)})


def test_hamming_queries(cp):
    ix = cp.idx
    assert set(tc.NAMED) | {tc.DUP_POS} <= set(tc.hamming_loci(ix))
    for l in tc.hamming_loci(ix):
        b, n = int(ix.locus_begin[l]), int(ix.locus_count[l])
        lens = [int(ix.off[a + 1] - ix.off[a]) for a in range(b, b + n)]
        q = dict(tc.hamming_queries(ix, l))
        assert [len(q["len_" + k]) for k in ("0", "1", "shortest-1", "shortest", "shortest+1", "longest+1", "limit")] == \
            [0, 1, min(lens) - 1, min(lens), min(lens) + 1, max(lens) + 1, tc.HAMMING_LIMIT]
        for name, a in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            d = [int(tc.hamming_model(ix, l, q["%s/%s" % (name, kind)])[a]) for kind in ("exact", "one_changed", "two_changed", "all_changed", "lower_case")]
            assert d == [0, 1, 2 if lens[a] > 1 else 1, lens[a], lens[a]]
        assert not tc.hamming_model(ix, l, b"").any()
    assert tc.string_diff(b"ACGT", b"AGGTTT") == 1 and tc.string_diff(b"", b"ACGT") == 0
    assert tc.hamming_le_model(np.array([3, 1, 1, 0], np.uint32), 10, 1) == (11, 3) and tc.hamming_le_model(np.array([3], np.uint32), 10, 2) == (-1, 0)
