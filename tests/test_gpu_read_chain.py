"""The read chain as a whole (csrc/read_chain.h, chain_apply): raw statistics, quality trim, adapter cut, mate overlap, prepared
statistics, duplicate removal.  The tests of the single switches cover each stage alone, all of them together and overlap beside the
statistics; here every subset of {preparation, adapters, mate overlap, dedup} runs with the statistics off and on, through both callers
of the chain (the single-text parser and the mate-file parser), and unpaired.  The yardstick is that of the other read tests: the engine
with the switches ON and the RAW text must leave what it leaves with every switch OFF and the text the rules of metamlst_amd.fastq
compose in chain order -- the packed rows byte for byte, the typed statistics, every stage's counters, the launches per stage.  Then the
order in which the switches close the entries that take no prepared reads (chain_refuse)."""
import functools
import itertools

import numpy as np
import pytest

import test_gpu_read_dedup as dd
import test_gpu_read_overlap as po
import test_gpu_read_prep as rp
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import dedup_fastq, prep_fastq, read_stats, read_stats_equal, trim_adapters, trim_pair_overlap
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks

pytestmark = pytest.mark.gpu

ADAPTERS = {"adapters": [po.ADAPTER], "min_overlap": 8, "error_permille": 100}
RA_ZERO = {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": []}
SUBSETS = list(itertools.product((False, True), repeat=4))      # (prep, adapter, overlap, dedup)


def subset_id(s) -> str:
    return "+".join(n for n, on in zip(("prep", "adapter", "overlap", "dedup"), s) if on) or "none"


@functools.lru_cache(maxsize=None)
def raw_text(prep: bool, paired: bool) -> bytes:
    """the 399 pairs of chain_sample() interleaved (Phred+64 under the preparation), or their first mates alone"""
    t1, _, inter = po.texts_of(po.chain_sample()[1], 64 if prep else 33)
    return inter if paired else t1


@functools.lru_cache(maxsize=None)
def shortened(prep: bool, adapter: bool, overlap: bool, paired: bool):
    """(the text in front of the duplicates' removal, {stage: the rule's counters}); every step is computed once"""
    if overlap:
        text, info = shortened(prep, adapter, False, paired)
        text, oinfo = trim_pair_overlap(text, trim5=po.PREP["trim5"] if prep else 0, **po.DEFAULT)
        return text, dict(info, overlap=oinfo)
    if adapter:
        text, info = shortened(prep, False, False, paired)
        text, ainfo = trim_adapters(text, [po.ADAPTER], 8, 100)
        return text, dict(info, adapter=ainfo)
    if prep:
        text, pinfo = prep_fastq(raw_text(True, paired), **po.PREP)
        return text, {"prep": pinfo}
    return raw_text(False, paired), {}


@functools.lru_cache(maxsize=None)
def rule(subset, paired: bool = True):
    """(the text in front of dedup, the text the engine must behave as if given, {stage: counters})"""
    prep, adapter, overlap, dedup = subset
    before, info = shortened(prep, adapter, overlap, paired)
    if not dedup:
        return before, before, info
    text, dinfo = dedup_fastq(before, paired=paired)
    return before, text, dict(info, dedup=dinfo)


def test_no_stage_passes_vacuously():
    """on the host: every enabled stage acts on more than 10 reads or pairs of this input, in every subset"""
    for paired in (True, False):
        for s in SUBSETS:
            if s[2] and not paired:
                continue
            info = rule(s, paired)[2]
            acted = {"prep": lambda i: i["shortened"], "adapter": lambda i: i["trimmed"], "overlap": lambda i: i["trimmed_pairs"], "dedup": lambda i: i["duplicates"]}
            assert sorted(info) == sorted(n for n, on in zip(("prep", "adapter", "overlap", "dedup"), s) if on)
            assert all(acted[k](v) > 10 for k, v in info.items()), (subset_id(s), paired, {k: acted[k](v) for k, v in info.items()})


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(po.chain_sample()[0])
    e.set_profiling(1)
    yield e
    e.close()


def begin(eng, subset=(False, False, False, False), stats: bool = False):
    prep, adapter, overlap, dedup = subset
    eng.reset_sample()
    eng.reset_kernel_time()
    eng.set_read_prep(**(po.PREP if prep else {}))
    eng.set_read_adapters(**(ADAPTERS if adapter else {"adapters": None}))
    eng.set_read_stats(stats)
    eng.set_read_dedup(dedup)
    eng.set_read_pair_overlap(overlap, **po.DEFAULT)


_plain = {}


def plain(eng, text: bytes, paired: bool):
    """what the engine leaves of a text with every switch off: (packed rows, typed statistics); once per text"""
    key = (text, paired)
    if key not in _plain:
        begin(eng)
        eng.submit_fastq(text, paired=paired)
        _plain[key] = (eng.debug_last_packed(), typed(eng))
        assert eng.read_prep_info() == rp.ZERO and eng.read_adapters_info() == RA_ZERO and eng.read_pair_overlap_info() == po.ZERO and eng.read_dedup_info() == dd.ZERO
        assert all(eng.kernel_time(k)[1] == 0 for k in range(18, 23))
    return _plain[key]


def assert_chain(eng, subset, stats: bool, paired: bool, pieces: int):
    """the counters, the launches and the tables behind a sample that went through chain_apply `pieces` times"""
    prep, adapter, overlap, dedup = subset
    before, _, info = rule(subset, paired)
    shortens = prep or adapter or overlap
    what = (subset_id(subset), stats, paired)
    assert eng.read_prep_info() == info.get("prep", rp.ZERO), what
    assert eng.read_adapters_info() == info.get("adapter", RA_ZERO), what
    assert eng.read_pair_overlap_info() == info.get("overlap", po.ZERO), what
    got_dd = eng.read_dedup_info()
    assert (dd.rule_part(got_dd) == info["dedup"] and got_dd["clashes"] == 0) if dedup else got_dd == dd.ZERO, what
    want_launches = {18: pieces * prep, 19: pieces * adapter, 20: pieces * (1 + shortens) * stats, 21: pieces * dedup, 22: pieces * overlap}
    got_launches = {k: eng.kernel_time(k)[1] for k in want_launches}
    print(what, "launches", got_launches)
    assert got_launches == want_launches, what
    sinfo = eng.read_stats_info()
    assert sinfo["raw_launches"] == pieces * stats and sinfo["prepared_launches"] == pieces * (stats and shortens), what
    if stats:
        tables = eng.read_stats()
        assert tables["prepared_counted"] == bool(shortens), what
        for stage, text, phred64 in (("raw", raw_text(prep, paired), prep), ("prepared", before, False)):      # (prep_fastq writes Phred+33)
            want = read_stats(text, phred64=phred64, paired=paired)
            assert all(read_stats_equal(tables[stage][side], want[side]) for side in (0, 1)), what + (stage,)


# ------------------------------------------------------------------ the single-text parser
@pytest.mark.parametrize("stats", (False, True), ids=("stats off", "stats on"))
@pytest.mark.parametrize("subset", SUBSETS, ids=subset_id)
def test_every_subset_of_the_chain_on_one_paired_chunk(eng, subset, stats):
    raw, want_text = raw_text(subset[0], True), rule(subset)[1]
    want = plain(eng, want_text, True)
    begin(eng, subset, stats)
    assert eng.submit_fastq(raw, paired=True) == 798
    assert_chain(eng, subset, stats, True, 1)
    rp.assert_packed_equal(eng.debug_last_packed(), want[0])
    assert_typed_equal(typed(eng), want[1])
    assert int(want[1][0].n_hits.sum()) > 100, "the statistics are empty"


# ------------------------------------------------------------------ the mate-file parser
def last_records(text: bytes, n: int) -> bytes:
    return text[dd.record_starts(text)[-n]:]


@pytest.mark.parametrize("subset", SUBSETS, ids=subset_id)
def test_every_subset_of_the_chain_through_bgzip_mate_files(eng, subset):
    raw, want_text = raw_text(subset[0], True), rule(subset)[1]
    want = plain(eng, want_text, True)
    b1, b2 = (bgzf_blocks(t, sizes)[:-1] for t, sizes in zip(po.split_mates(raw), ((3001, 4507), (2777, 3999))))
    eof = bgzf_blocks(b"")[-1]
    calls = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    assert len(calls) > 3
    begin(eng, subset, True)
    done = [eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls)]
    assert sum(done) == 798
    pieces = sum(n > 0 for n in done)      # (a piece that completes no pair never reaches the chain)
    assert pieces > 1
    assert_chain(eng, subset, True, True, pieces)
    assert_typed_equal(typed(eng), want[1])
    # the packed rows are those of the last piece that held a pair: the tail of the expected text
    last = [n for n in done if n][-1]
    got_rows = eng.debug_last_packed()
    begin(eng)
    assert eng.submit_fastq(last_records(want_text, last), paired=True) == last
    rp.assert_packed_equal(got_rows, eng.debug_last_packed())


# ------------------------------------------------------------------ unpaired
@pytest.mark.parametrize("subset", [s for s in SUBSETS if not s[2]], ids=subset_id)
def test_every_subset_without_the_overlap_on_unpaired_text(eng, subset):
    raw, want_text = raw_text(subset[0], False), rule(subset, False)[1]
    want = plain(eng, want_text, False)
    begin(eng, subset, True)
    assert eng.submit_fastq(raw) == 399
    assert_chain(eng, subset, True, False, 1)
    rp.assert_packed_equal(eng.debug_last_packed(), want[0])
    assert_typed_equal(typed(eng), want[1])
    # with the overlap on as well an unpaired submission is refused, and the handle stays usable
    begin(eng, subset[:2] + (True,) + subset[3:], True)
    with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: an unpaired FASTQ submission"):
        eng.submit_fastq(raw)
    begin(eng, subset, True)
    assert eng.submit_fastq(raw) == 399
    assert_typed_equal(typed(eng), want[1])


# ------------------------------------------------------------------ the order of the refusals
SENTENCES = (("rn", r"read names are on \(mlst_set_read_names\)"), ("rp", r"read preparation is on \(mlst_set_read_prep\)"),
             ("ra", r"adapter removal is on \(mlst_set_read_adapters\)"), ("rs", r"read statistics are on \(mlst_set_read_stats\)"),
             ("dd", r"duplicate removal is on \(mlst_set_read_dedup\)"), ("po", r"mate overlap trimming is on \(mlst_set_read_pair_overlap\)"))


def test_the_first_switch_that_is_on_closes_the_seven_entries():
    idx, reads = rp.sample()
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        fb = np.frombuffer(reads[0][0], np.uint8); fq = np.frombuffer(bytes(v + 33 for v in reads[0][1]), np.uint8); off = np.array([0, len(fb)], np.uint64)
        calls = {
            "mlst_submit_reads": lambda: eng.submit_reads(fb, fq, off),
            "mlst_submit_reads_device": lambda: eng.submit_reads_device(0, 0, 0, 1, 150),
            "mlst_submit_packed_device": lambda: eng.submit_packed_device(0, 0, 0, 1, 10, 152),
            "mlst_submit_packed_host": lambda: eng._check(eng.lib.mlst_submit_packed_host(eng._h, None, None, None, 1, 10, 152, 0), "mlst_submit_packed_host"),
            "mlst_submit_fasta": lambda: eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n"),
            "mlst_bam_reads_open": lambda: eng.bam_reads_open(0),
            "mlst_set_read_tiling": lambda: eng.set_read_tiling(150, 25),
        }
        off_switch = {"rn": lambda: eng.set_read_names(False), "rp": lambda: eng.set_read_prep(), "ra": lambda: eng.set_read_adapters(None),
                      "rs": lambda: eng.set_read_stats(False), "dd": lambda: eng.set_read_dedup(False), "po": lambda: eng.set_read_pair_overlap(False)}
        eng.set_read_names(True); eng.set_read_prep(**po.PREP); eng.set_read_adapters(**ADAPTERS)
        eng.set_read_stats(True); eng.set_read_dedup(True); eng.set_read_pair_overlap(True)
        for stage, sentence in SENTENCES:
            for entry, call in calls.items():
                with pytest.raises(MlstError, match=r"\(-1\): %s: %s" % (entry, sentence)):
                    call()
            off_switch[stage]()
        assert eng.get_read_tiling() == (0, 0)
        # with every switch off every entry is open: none answers with a switch's sentence (the device entries are handed no
        # buffers and refuse those, or are given no reads)
        calls["mlst_submit_reads_device"] = lambda: eng.submit_reads_device(0, 0, 0, 0, 150)
        for entry, call in calls.items():
            try:
                call()
            except MlstError as e:
                assert " is on (mlst_set_read_" not in str(e) and " are on (mlst_set_read_" not in str(e), (entry, str(e))
                assert entry in ("mlst_submit_packed_device", "mlst_submit_packed_host"), (entry, str(e))
            eng.reset_sample()
        assert eng.get_read_tiling() == (150, 25)
    finally:
        eng.close()
