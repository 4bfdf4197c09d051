"""The crafted alignment cases (tests/align_cases.py) on the GPU: the HIP engine against the oracle, one submission per group so
that a difference names its group, in every configuration that changes which extension kernel or which pass takes a pair."""
import contextlib
import functools
import os

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
from metamlst_amd import synth
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.typing import consensus_from_counts, pick_alleles_fast

pytestmark = pytest.mark.gpu

CAP = 1 << 16
# name -> (environment while the reference is loaded, parameters, loci the haplotype kernel must take: None = all)
CONFIGS = {
    "default": ({}, {}, None),
    "pairs_kernel": ({"MLST_EXT_HAP_MAX": "0"}, {}, 0),
    "hap_max_64": ({"MLST_EXT_HAP_MAX": "64"}, {}, 64),                 # the 64-allele locus is the last one k_extend takes
    "threads_256": ({"MLST_EXT_THREADS": "256"}, {}, None),
    "two_additions": ({}, {"max_items": 1 << 24}, None),
    "always_banded": ({}, {"gap_trigger_mm": -1}, None),
    "no_quirk": ({}, {"xm_field_quirk": 0}, None),
}


def params_of(over):
    p = default_params()
    for k, v in over.items():
        setattr(p, k, v)
    return p


@contextlib.contextmanager
def engine_for(env, over, idx=None):
    """An engine with the reference loaded under `env`, closed on the way out whether the test passed or not."""
    eng = _engine_for(env, over, idx)
    try:
        yield eng
    finally:
        eng.close()


def _engine_for(env, over, idx=None):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(0, params_of(over))
        eng.load_reference(idx if idx is not None else ac.corpus().idx)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return eng


@functools.lru_cache(maxsize=None)
def submission(what, order="forward"):
    """(bases, quals, off, cases): a group, or the whole corpus in case order / reversed."""
    cp = ac.corpus()
    cases = cp.of(what) if what != "all" else list(cp.cases)
    if order == "reversed":
        cases = cases[::-1]
    fb, fq, off, _ = cp.layout(cases, lanes=None if what != "all" else False)
    return fb, fq, off, cases


@functools.lru_cache(maxsize=None)
def oracle_says(what, order, trig, quirk):
    """The specification's answer for a submission, computed once per (submission, parameters) and shared."""
    cp = ac.corpus()
    orc = oracle_lib.Oracle(cp.idx, params_of({"gap_trigger_mm": trig, "xm_field_quirk": quirk}))
    fb, fq, off, _ = submission(what, order)
    orc.submit_reads(fb, fq, off)
    so, items = orc.stats(want_items=CAP)
    chosen = sorted(pick_alleles_fast(cp.idx, so, 100).values())
    return so, fx.sorted_items(items), chosen, (orc.pileup(chosen) if chosen else {})


def spec(what, order, over):
    p = params_of(over)
    return oracle_says(what, order, int(p.gap_trigger_mm), int(p.xm_field_quirk))


def check(eng, what, order, over, tail=True):
    cp = ac.corpus()
    fb, fq, off, _ = submission(what, order)
    so, items_o, chosen_o, po = spec(what, order, over)
    eng.reset_sample()
    eng.submit_reads(fb, fq, off)
    s = eng.stats()
    fx.assert_stats_equal(s, so)
    assert np.array_equal(fx.sorted_items(eng.items(CAP)), items_o), "items differ"
    chosen = sorted(pick_alleles_fast(cp.idx, s, 100).values())
    assert chosen == chosen_o
    if chosen:
        pc, cons = eng.pileup(chosen), eng.consensus(chosen)
        for a in chosen:
            assert np.array_equal(pc[a], po[a]), "pileup differs for allele %d (chosen %s)" % (a, chosen)
            assert cons[a].decode() == "".join(consensus_from_counts(po[a])), "consensus differs for allele %d (chosen %s)" % (a, chosen)
        if tail:                                                          # k_choose against the host's choice
            eng.reset_sample()
            eng.submit_reads(fb, fq, off)
            eng.typing_enqueue(penalty=100)
            st, dev_chosen, _ = eng.typing_fetch()
            fx.assert_stats_equal(st, so)
            assert dev_chosen == pick_alleles_fast(cp.idx, st, 100), "k_choose differs from the host choice"


def first_differing_case(eng, what, over):      # (eng: the engine of the failed check, still open)
    """After a MISMATCH (never after a fault): the group's cases one by one, the first whose sums or items differ."""
    cp = ac.corpus()
    p = params_of(over)
    orc = oracle_lib.Oracle(cp.idx, p)
    for c in cp.of(what) if what != "all" else cp.cases:
        fb, fq, off, _ = cp.layout([c], lanes=False)
        eng.reset_sample()
        eng.submit_reads(fb, fq, off)
        orc.submit_reads(fb, fq, off)
        s = eng.stats()
        so, items = orc.stats(want_items=64)
        try:
            fx.assert_stats_equal(s, so)
            assert np.array_equal(fx.sorted_items(eng.items(64)), fx.sorted_items(items))
        except AssertionError as e:
            alleles = np.nonzero((s.sum_score != so.sum_score) | (s.n_hits != so.n_hits))[0][:8].tolist()
            return "%s (alleles %s): %s" % (c.name, alleles, str(e)[:300])
    return "no single case differs on its own"


def run_groups(eng, over, groups, tail=True):
    for g in groups:
        try:
            check(eng, g, "forward", over, tail)
        except AssertionError as e:
            raise AssertionError("group %s: %s; first differing case: %s" % (g, str(e)[:400], first_differing_case(eng, g, over))) from None


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_group_equals_the_oracle(config):
    env, over, hap_max = CONFIGS[config]
    cp = ac.corpus()
    with engine_for(env, over) as eng:
        info = eng.extend_info()
        counts = [int(x) for x in cp.idx.locus_count]
        assert info["loci"] == sum(1 for n in counts if hap_max is None or n <= hap_max), (config, info)      # the loci k_extend is meant to take
        if "MLST_EXT_THREADS" in env:
            assert info["threads"] == int(env["MLST_EXT_THREADS"])
        run_groups(eng, over, ac.GROUPS)


@pytest.mark.parametrize("kind", ["lds", "routed", "global"])
def test_seeding_groups_under_every_sieve(kind, monkeypatch):
    monkeypatch.setenv("MLST_SIEVE", kind)
    with engine_for({}, {}) as eng:
        assert eng.sieve_info()["kind"] == kind
        run_groups(eng, {}, ("lengths", "votes"), tail=False)


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_whole_corpus_in_one_submission(order):
    with engine_for({}, {}) as eng:
        try:
            check(eng, "all", order, {})
        except AssertionError as e:
            raise AssertionError("%s; first differing case: %s" % (str(e)[:400], first_differing_case(eng, "all", {}))) from None


def test_whole_corpus_twice_replays_the_graph():
    fb, fq, off, _ = submission("all")
    so, items_o, _, _ = spec("all", "forward", {})
    with engine_for({}, {}) as eng:
        for _ in range(2):
            eng.reset_sample()
            eng.submit_reads(fb, fq, off)
            fx.assert_stats_equal(eng.stats(), so)
            assert np.array_equal(fx.sorted_items(eng.items(CAP)), items_o)


def test_a_locus_beyond_the_pending_additions_of_an_item_takes_the_slow_pass():
    """n_alleles > acc_cap: k_extend keeps at most 16,384 pending additions of an item in LDS; a locus of 16,512 alleles that the
    haplotype kernel is made to take (MLST_EXT_HAP_MAX raised) must go pair by pair there and still equal the oracle."""
    idx, reads = ac.wide_locus()
    assert int(idx.locus_count[0]) == ac.WIDE_B0 * ac.WIDE_B1 > 16384
    fb, fq, off = synth.ragged_reads(reads, [b"I" * len(r) for r in reads])
    orc = oracle_lib.Oracle(idx)
    orc.submit_reads(fb, fq, off)
    so, items_o = orc.stats(want_items=64)
    assert int(so.counters[0]) > 16384 and len(items_o) == len(reads)
    with engine_for({"MLST_EXT_HAP_MAX": "100000"}, {}, idx) as eng:
        assert eng.extend_info()["loci"] == 1                      # the haplotype kernel has the locus
        for _ in range(2):
            eng.reset_sample()
            eng.submit_reads(fb, fq, off)
            s = eng.stats()
            fx.assert_stats_equal(s, so)
            assert np.array_equal(fx.sorted_items(eng.items(64)), fx.sorted_items(items_o))
        chosen = sorted(pick_alleles_fast(idx, s, 100).values())
        pc, po = eng.pileup(chosen), orc.pileup(chosen)
        for a in chosen:
            assert np.array_equal(pc[a], po[a])


# name -> parameters under which a read of 320 bases could exceed a packed field: the 10-bit score, the 8-bit xm, the 7-bit xo
OVER_LIMIT = {
    "score_1280": {"match_bonus": 4, "mm_min": 2, "mm_max": 6, "n_penalty": 1, "gap_open": 8, "gap_ext": 3},
    "xm_free_n": {"n_penalty": 0},
    "xm_free_mismatch": {"mm_min": 0},
    "xm_cheap_mismatch": {"match_bonus": 3, "mm_min": 1, "mm_max": 6, "n_penalty": 0},
    "xo_cheap_gaps": {"gap_open": 2, "gap_ext": 2},
}


@pytest.mark.parametrize("name", list(OVER_LIMIT))
def test_scoring_that_could_overflow_a_packed_field_is_refused(name):
    with pytest.raises(MlstError, match=r"\(-5\)"):                  # MLST_E_LIMIT
        Engine(0, params_of(OVER_LIMIT[name]))


def test_the_widest_scoring_inside_the_limits_is_accepted():
    """match_bonus 3 (score 960 < 1,024), cheapest mismatch 1 (3 <= 4 * 1), one-base gap of 8 (15 <= 16): accepted, and a
    perfect 320-base read and one with N at every third base equal the oracle."""
    over = {"match_bonus": 3, "mm_min": 1, "mm_max": 6, "n_penalty": 1, "gap_open": 5, "gap_ext": 3}
    cp = ac.corpus()
    cases = [c for c in cp.of("score_limits") if "perfect320" in c.name or "N_every" in c.name]
    fb, fq, off, _ = cp.layout(cases, lanes=False)
    orc = oracle_lib.Oracle(cp.idx, params_of(over))
    orc.submit_reads(fb, fq, off)
    so, items_o = orc.stats(want_items=64)
    assert int(so.sum_score.max()) >= 960
    with engine_for({}, over) as eng:
        eng.submit_reads(fb, fq, off)
        fx.assert_stats_equal(eng.stats(), so)
        assert np.array_equal(fx.sorted_items(eng.items(64)), fx.sorted_items(items_o))
