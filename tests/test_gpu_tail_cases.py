"""The crafted inputs of the typing tail (tests/tail_cases.py) on the GPU: k_choose, k_layout_compact, k_consensus,
k_consensus_expand, k_hamming and k_export / k_import against the plain models of tail_cases, with no reads at all -- statistics are
imported, pile-up counts are written into a buffer the test owns.  Every comparison is exact.  One engine for the module."""
import ctypes as C

import numpy as np
import pytest

import tail_cases as tc
from metamlst_amd.engine import MLST_CNT_N, Engine, MlstError, _ptr
from metamlst_amd.typing import NO_READ, SampleStats, pick_alleles_fast

pytestmark = pytest.mark.gpu

# columns of slack behind the fixed layout in the counts buffer: cap_cols = need + 1 is one column more than the fixed layout when
# every locus is chosen, and the engine zeroes cap_cols columns
SLACK_COLS = 16


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    try:
        e.load_reference(tc.corpus().idx)
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def colbase(eng):
    """mlst_typing_layout's column bases: the models lay their letters and counts out by these."""
    ix = tc.corpus().idx
    cb, tot = np.zeros(ix.n_loci + 1, np.uint64), C.c_uint64()
    eng._check(eng.lib.mlst_typing_layout(eng._h, _ptr(cb), C.byref(tot)), "mlst_typing_layout")
    assert int(tot.value) == int(cb[-1]) == eng.typing_total_cols()
    assert np.array_equal(cb, tc.fixed_colbase(ix))                # one slot of the longest allele per locus, in locus order
    return cb


def to_device(torch, a: np.ndarray):
    """A device copy of a numpy array (as int64 / int32 words: the engine reads the bytes)."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def import_case(torch, eng, case, keep):
    """Statistics of a case into the engine; `keep` holds the device tensors until the test is over."""
    n_sum, n_min = eng.flat_sizes()
    assert n_min == len(case.locus_first) and n_sum == 2 * len(case.sum_score) + n_min + MLST_CNT_N
    t_flat, t_first = to_device(torch, case.flat(n_sum)), to_device(torch, case.locus_first)
    keep += [t_flat, t_first]
    eng.import_stats_device(t_flat.data_ptr(), t_first.data_ptr())


def fetch_raw(eng):
    """mlst_typing_fetch as it is: (statistics, chosen int32[n_loci], the WHOLE fixed-layout letter array) -- Engine.typing_fetch
    trims the letters to the chosen alleles."""
    ix = eng.index
    nA, nL = ix.n_alleles, ix.n_loci
    s = SampleStats(np.empty(nA, np.int64), np.empty(nA, np.uint32), np.empty(nL, np.uint64), np.empty(nL, np.uint64), np.empty(MLST_CNT_N, np.uint64))
    chosen, letters = np.empty(nL, np.int32), np.full(eng.typing_total_cols(), 0xFF, np.uint8)
    eng._check(eng.lib.mlst_typing_fetch(eng._h, _ptr(s.sum_score), _ptr(s.n_hits), _ptr(s.locus_len_sum), _ptr(s.locus_first), _ptr(s.counters),
                                         _ptr(chosen), _ptr(letters)), "mlst_typing_fetch")
    return s, chosen, letters


def assert_stats_are(s, case):
    want = case.stats()
    assert np.array_equal(s.sum_score, want.sum_score), (case.name, "sum_score")
    assert np.array_equal(s.n_hits, want.n_hits), (case.name, "n_hits")
    assert np.array_equal(s.locus_first, want.locus_first), (case.name, "locus_first")
    assert not s.locus_len_sum.any(), (case.name, "locus_len_sum")


def chosen_array(ix, case, penalty) -> np.ndarray:
    want = np.full(ix.n_loci, -1, np.int32)
    for l, a in tc.choice_fast(ix, case, penalty).items():
        want[l] = a
    return want


def first_differences(got: np.ndarray, want: np.ndarray, ix) -> str:
    bad = np.nonzero(got != want)[0][:6].tolist()
    return ", ".join("locus %d (%d alleles): index %d, model %d" % (l, int(ix.locus_count[l]), int(got[l]) - int(ix.locus_begin[l]),
                                                                   int(want[l]) - int(ix.locus_begin[l])) for l in bad)


# ---- 1. choice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("penalty", tc.PENALTIES)
def test_choice_equals_the_host_statement_on_every_case(torch, eng, penalty):
    """import, mlst_typing_enqueue, mlst_typing_fetch: the statistics come back unchanged and chosen[] is pick_alleles_fast's allele
    INDEX for every locus.  All cases run under one (penalty, mincov, none_char): from the third on the typing graph is a replay,
    and it must read the statistics imported after its capture."""
    cp = tc.corpus()
    ix, keep = cp.idx, []
    eng.reset_sample()
    for case in cp.cases:
        import_case(torch, eng, case, keep)
        eng.typing_enqueue(penalty=penalty, mincov=1, none_char="N")
        s, chosen, _ = fetch_raw(eng)
        assert_stats_are(s, case)
        want = chosen_array(ix, case, penalty)
        assert np.array_equal(chosen, want), "%s, penalty %d: %s" % (case.name, penalty, first_differences(chosen, want, ix))
        assert {l: int(a) for l, a in enumerate(chosen) if a >= 0} == pick_alleles_fast(ix, s, penalty)      # ... and from the statistics handed back
    eng.reset_sample()


def test_rows_of_one_number_that_tie_go_to_the_lower_index():
    """Rows 255 and 256 of one locus carry the same number and tie: thread 255 holds the lower index, thread 0 (second turn) the
    higher.  The host statement keeps the first it visits; the device's answer must not depend on its thread layout."""
    import torch
    ix = tc.corpus().idx_dup
    case = tc.dup_case(ix, 0)
    k1, k2 = tc.duplicate_pair(ix, 0)
    assert (k1, k2) == (255, 256)
    e = Engine(0)
    try:
        e.load_reference(ix)
        keep = []
        for penalty in tc.PENALTIES:
            import_case(torch, e, case, keep)
            e.typing_enqueue(penalty=penalty)
            s, chosen, _ = fetch_raw(e)
            assert_stats_are(s, case)
            assert chosen.tolist() == [k1] == [tc.choice_fast(ix, case, penalty)[0]], (penalty, chosen.tolist())
    finally:
        e.close()


# ---- 2. consensus: three routes, one answer ------------------------------------------------------------------------------------------
_COUNTS = {}


def counts_of_pattern(pattern: str) -> np.ndarray:
    """Fixed-layout counts: the crafted patterns in the slots of the loci the presence case chooses, zeros elsewhere."""
    if pattern not in _COUNTS:
        ix = tc.corpus().idx
        mask = np.zeros(ix.n_loci, bool)
        mask[tc.corpus().case("presence/" + pattern).chosen_loci()] = True
        a = np.where(np.repeat(mask, ix.locus_maxlen)[:, None], tc.counts_fixed(), np.uint32(0)).astype(np.uint32)
        a.setflags(write=False)
        _COUNTS[pattern] = a
    return _COUNTS[pattern]


def write_counts(torch, eng, d_counts, counts: np.ndarray):
    """After the engine's own zero-fill and (empty) pile-up have finished: the crafted counts into the front of the buffer."""
    eng.synchronize()
    if len(counts):
        d_counts[:counts.size].copy_(torch.from_numpy(counts.view(np.int32).reshape(-1).copy()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("none_char", tc.NONE_CHARS)
@pytest.mark.parametrize("mincov", tc.MINCOVS)
def test_consensus_by_three_routes(torch, eng, colbase, mincov, none_char):
    """Fixed layout (k_consensus over the caller's buffer), the bare kernel entry (mlst_consensus_from_counts_device) and the
    compact layout (k_layout_compact + k_consensus_expand): the WHOLE fixed-layout letter array equals the model each time --
    columns of a slot beyond the chosen allele's length and slots of loci without a chosen allele included."""
    cp = tc.corpus()
    ix, keep = cp.idx, []
    total = int(colbase[-1])
    d_counts = torch.zeros((total + SLACK_COLS) * 4, dtype=torch.int32, device="cuda:0")      # the full fixed layout, whatever cap_cols
    torch.cuda.synchronize()
    eng.reset_sample()
    for pattern in tc.PRESENCE:
        case = cp.case("presence/" + pattern)
        loci = case.chosen_loci()
        counts = counts_of_pattern(pattern)
        want = tc.letters_of_corpus(loci, mincov, none_char)
        want_chosen = chosen_array(ix, case, 100)
        assert sorted(np.nonzero(want_chosen >= 0)[0].tolist()) == loci
        import_case(torch, eng, case, keep)

        eng.typing_choose_pileup(100, d_counts.data_ptr())
        write_counts(torch, eng, d_counts, counts)
        eng.typing_finish(mincov, none_char, d_counts.data_ptr())
        s, chosen, letters = fetch_raw(eng)
        assert_stats_are(s, case)
        assert np.array_equal(chosen, want_chosen), (pattern, "choice")
        assert np.array_equal(letters, want), (pattern, "fixed layout", np.nonzero(letters != want)[0][:8])

        got = np.frombuffer(eng.consensus_from_counts_device(d_counts.data_ptr(), total, mincov, none_char), np.uint8)
        assert np.array_equal(got, want), (pattern, "consensus_from_counts_device", np.nonzero(got != want)[0][:8])

        compact = tc.compact_counts(counts, colbase, loci)
        need = tc.compact_layout(colbase, loci)[1]
        eng.typing_choose_pileup_compact(100, d_counts.data_ptr(), max(need, 1))
        write_counts(torch, eng, d_counts, compact)
        eng.typing_finish_compact(mincov, none_char, d_counts.data_ptr())
        s, chosen, letters = fetch_raw(eng)
        assert eng.typing_compact_info() == (need, False), pattern
        assert np.array_equal(chosen, want_chosen), (pattern, "choice, compact")
        assert np.array_equal(letters, want), (pattern, "compact layout", np.nonzero(letters != want)[0][:8])
    eng.reset_sample()


# ---- 3. compact layout ---------------------------------------------------------------------------------------------------------------
def test_compact_layout_need_and_overflow(torch, eng, colbase):
    """mlst_typing_compact_info returns the model's need for every pattern of chosen loci; need and need + 1 columns fit, need - 1
    reports overflow with the same need, and the repeat with need columns gives the right letters with statistics and choice untouched."""
    cp = tc.corpus()
    ix, keep = cp.idx, []
    total = int(colbase[-1])
    d_counts = torch.zeros((total + SLACK_COLS) * 4, dtype=torch.int32, device="cuda:0")      # ALWAYS the full fixed layout: a wrong layout must
    torch.cuda.synchronize()                                                                   # show as wrong letters, never outside the buffer
    eng.reset_sample()
    needs = set()
    for pattern in tc.PRESENCE:
        case = cp.case("presence/" + pattern)
        loci = case.chosen_loci()
        compact = tc.compact_counts(counts_of_pattern(pattern), colbase, loci)
        need = tc.compact_layout(colbase, loci)[1]
        assert need == len(compact) <= total
        needs.add(need)
        want = tc.letters_of_corpus(loci, 1, "N")
        want_chosen = chosen_array(ix, case, 100)
        import_case(torch, eng, case, keep)
        for cap in ([need + 1, need - 1, need] if need else [1]):
            eng.typing_choose_pileup_compact(100, d_counts.data_ptr(), cap)
            write_counts(torch, eng, d_counts, compact)
            eng.typing_finish_compact(1, "N", d_counts.data_ptr())
            s, chosen, letters = fetch_raw(eng)
            assert eng.typing_compact_info() == (need, cap < need), (pattern, cap)
            assert_stats_are(s, case)
            assert np.array_equal(chosen, want_chosen), (pattern, cap)
            if cap >= need:
                assert np.array_equal(letters, want), (pattern, cap, np.nonzero(letters != want)[0][:8])
    assert 0 in needs and total in needs and len(needs) >= 6
    with pytest.raises(MlstError, match=r"\(-1\)"):                 # a buffer of no columns is refused (MLST_E_INVALID)
        eng.typing_choose_pileup_compact(100, d_counts.data_ptr(), 0)
    eng.reset_sample()


# ---- 4. Hamming ----------------------------------------------------------------------------------------------------------------------
def test_hamming_equals_string_diff(eng):
    """mlst_hamming_all = stringDiff against every allele for every query (zip() semantics: the shorter of the two bounds it; the
    compare is by byte); mlst_hamming_le = the first allele in index order and the count."""
    ix = tc.corpus().idx
    for l in tc.hamming_loci(ix):
        b = int(ix.locus_begin[l])
        for name, q in tc.hamming_queries(ix, l):
            want = tc.hamming_model(ix, l, q)
            got = eng.hamming_all(l, q)
            assert np.array_equal(got, want), (l, name, np.nonzero(got != want)[0][:8])
            lo, hi = int(want.min()), int(want.max())
            for z in sorted({0, lo, hi} | ({lo - 1} if lo > 0 else set())):
                assert eng.hamming_le(l, q, z) == tc.hamming_le_model(want, b, z), (l, name, z)


def test_hamming_all_on_every_locus(eng):
    ix = tc.corpus().idx
    for l in range(ix.n_loci):
        for name, q in tc.hamming_queries(ix, l):
            want = tc.hamming_model(ix, l, q)
            got = eng.hamming_all(l, q)
            assert np.array_equal(got, want), (l, name, np.nonzero(got != want)[0][:8])


def test_hamming_query_limit(eng):
    ix = tc.corpus().idx
    for l in (tc.corpus().position("n1"), tc.corpus().position("n1025"), tc.corpus().position("w600")):
        q = dict(tc.hamming_queries(ix, l))
        ok = q["len_limit"]
        assert len(ok) == tc.HAMMING_LIMIT
        with pytest.raises(MlstError, match=r"\(%d\)" % tc.MLST_E_LIMIT):
            eng.hamming_all(l, ok + b"A")
        with pytest.raises(MlstError, match=r"\(%d\)" % tc.MLST_E_LIMIT):
            eng.hamming_le(l, ok + b"A", 0)
        assert np.array_equal(eng.hamming_all(l, ok), tc.hamming_model(ix, l, ok))             # a good query right after it
        assert np.array_equal(eng.hamming_all(l, q["first/exact"]), tc.hamming_model(ix, l, q["first/exact"]))


# ---- 5. export / import --------------------------------------------------------------------------------------------------------------
def test_export_of_import_is_the_identity(torch, eng):
    ix = tc.corpus().idx
    nA, nL = ix.n_alleles, ix.n_loci
    n_sum, n_min = eng.flat_sizes()
    assert (n_sum, n_min) == (2 * nA + nL + MLST_CNT_N, nL)
    dev = torch.device("cuda", 0)

    def export():
        t_sum, t_min = torch.full((n_sum,), -7, dtype=torch.int64, device=dev), torch.full((n_min,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        eng.export_stats_device(t_sum.data_ptr(), t_min.data_ptr())
        return t_sum.cpu().numpy(), t_min.cpu().numpy()
    eng.reset_sample()
    empty = export()
    assert not empty[0].any() and (empty[1] == tc.SENTINEL).all()
    vectors = tc.export_vectors(nA, nL, n_sum)
    assert {0, 1, 1 << 40, 1 << 62, tc.SENTINEL} == set(np.concatenate([f for _, _, f in vectors]).tolist())
    assert any((v[:nA] < 0).all() for _, v, _ in vectors) and any((v[nA:2 * nA] == tc.M32).all() for _, v, _ in vectors)
    assert all((v[2 * nA + nL:] != 0).all() for _, v, _ in vectors)                         # non-zero counters
    for name, flat, first in vectors:
        t_flat, t_first = to_device(torch, flat), to_device(torch, first)
        eng.import_stats_device(t_flat.data_ptr(), t_first.data_ptr())
        got = export()
        assert np.array_equal(got[0], flat), (name, np.nonzero(got[0] != flat)[0][:8])
        assert np.array_equal(got[1], first), (name, np.nonzero(got[1] != first)[0][:8])
        eng.reset_sample()
        again = export()
        assert np.array_equal(again[0], empty[0]) and np.array_equal(again[1], empty[1]), name
    s = eng.stats()                                                 # and the host entry sees the empty state too
    assert not s.sum_score.any() and not s.n_hits.any() and (s.locus_first == NO_READ).all()
