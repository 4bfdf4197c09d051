"""mlst_set_read_pair_overlap (csrc/read_overlap.h): adapter read-through cut from the overlap of the mates on the device before the reads
are packed.  The yardstick is that of test_gpu_read_adapters.py: the engine with the switch ON and the RAW text must leave what the same
engine leaves with the switch OFF and the text fastq.trim_pair_overlap(fastq.trim_adapters(fastq.prep_fastq(...))) writes -- the packed
rows byte for byte (mlst_debug_last_packed), the typed statistics, the counters, the histogram -- through all five paired entries; then
the combinations with --dedup, --read-stats and an export, the life cycle, the refusals and `cli type --pair-overlap`.  pair_overlap itself
is pinned by hand in test_read_overlap_host.py.  The rule is the project's own (modelled on fastp's overlap analysis); nothing here claims
fastp's bytes."""
import functools
import gzip
import os

import numpy as np
import pytest

import test_gpu_read_dedup as dd
import test_gpu_read_prep as rp
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import dedup_fastq, pair_overlap, prep_fastq, read_stats, read_stats_equal, trim_adapters, trim_pair_overlap
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_read_overlap_host import letters, mutate, revcomp

pytestmark = pytest.mark.gpu

DEFAULT = {"min_overlap": 30, "max_mismatches": 5, "error_permille": 200}
SETTINGS = [DEFAULT, {"min_overlap": 10, "max_mismatches": 5, "error_permille": 200}, {"min_overlap": 64, "max_mismatches": 0, "error_permille": 0}]
LENGTHS = [0, 1, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 319, 320]
EDGES = (15, 16, 17, 63, 64, 65, 255, 256, 257)      # units at wave, workgroup and 64-read group edges that must carry a cut
ADAPTER = "AGATCGGAAGAGC"
ZERO = {"pairs": 0, "overlapping": 0, "trimmed_pairs": 0, "reads_trimmed": 0, "bases_removed": 0, "emptied": 0, "insert_hist": [0] * 1024}

_rng = np.random.default_rng(4242)
GENOME = letters(_rng, 900)
AD1, AD2 = ADAPTER.encode() + letters(_rng, 330), letters(_rng, 340)      # what follows the insert on mate 1 (the Illumina adapter first) and on mate 2


def ids(s):
    return "min=%d diff=%d permille=%d" % (s["min_overlap"], s["max_mismatches"], s["error_permille"])


def mates_of(frag: bytes, n1: int, n2: int):
    """the mates of a fragment: each read runs through the insert into its adapter"""
    return (frag + AD1)[:n1], (revcomp(frag) + AD2)[:n2]


def mates(insert: int, n1: int = 150, n2: int = 150, at: int = 0):
    return mates_of(GENOME[at:at + insert], n1, n2)


def put(s: bytes, p: int, c: bytes = b"N") -> bytes:
    return s[:p] + c + s[p + 1:]


def crafted_pairs() -> list:
    """[(mate 1, mate 2, note)]: the pairs by hand"""
    out = []
    for k, n in enumerate(LENGTHS):                            # equal lengths: read-through by one base, the whole read, half of it
        for insert in (n - 1, n, n // 2 + 15):
            out.append(mates(max(insert, 0), n, n, at=k) + ("%d / %d, insert %d" % (n, n, insert),))
    for k, n in enumerate(LENGTHS):                            # crossed lengths
        m = LENGTHS[-1 - k]
        for insert in (min(n, m) - 1, max(n, m) - 1, (n + m) // 2):
            out.append(mates(max(insert, 0), n, m, at=k + 20) + ("%d / %d, insert %d" % (n, m, insert),))
    for insert in range(30, 271):                              # every offset of one 150 / 150 pair
        out.append(mates(insert, at=40) + ("150 / 150 at o = %d" % (insert - 150),))
    for insert in range(30, 388):                              # every offset of one 320 / 97 pair: o = insert - 97 = -67 .. 290
        out.append(mates(insert, 320, 97, at=41) + ("320 / 97 at o = %d" % (insert - 97),))
    for insert in (96, 97, 98, 127, 128, 129, 320, 352, 353):  # ... and some of the other way round
        out.append(mates(insert, 97, 320, at=42) + ("97 / 320, insert %d" % insert,))
    m1, m2 = mates(30, at=43)                                  # the budget edges at L = 30 ...
    for places in ((1, 6, 11, 16, 21), (1, 6, 11, 16, 21, 26), (0, 29), (0, 7, 14, 21, 28, 29)):
        out.append((mutate(m1, places), m2, "L 30, %d mismatches on mate 1" % len(places)))
        out.append((m1, mutate(m2, places), "L 30, %d mismatches on mate 2" % len(places)))
    m1, m2 = mates(10, 40, 40, at=44)                          # ... and at L = 10, where the permille bound decides (SETTINGS[1])
    for places in ((2, 7), (2, 5, 7), (0,), (9,)):
        out.append((mutate(m1, places), m2, "L 10, %d mismatches" % len(places)))
    m1, m2 = mates(200, at=45)                                 # L = 100: 5 and 6 mismatches spread over four words
    for places in ((51, 63, 64, 95, 149), (51, 63, 64, 95, 96, 149)):
        out.append((mutate(m1, places), m2, "L 100, %d mismatches" % len(places)))
    m1, m2 = mates(60, at=46)                                  # N on either mate, N against N, other bytes, lower case
    out += [(put(m1, 10), m2, "N on mate 1"), (m1, put(m2, 10), "N on mate 2"), (put(m1, 10), put(m2, 49), "N against N"),
            (put(m1, 10, b"R"), put(m2, 49, b"."), "other bytes against each other"), (put(m1, 100), put(m2, 100), "N outside the overlap"),
            (put(put(put(put(put(put(m1, 3), 9), 20), 31), 32), 59), m2, "six Ns"), (m1.lower(), m2, "lower-case mate 1"), (m1, m2.lower(), "lower-case mate 2"),
            (m1.lower(), m2.lower(), "both in lower case"), (b"N" * 150, b"N" * 150, "only N"), (b"A" * 150, b"T" * 150, "one letter"),
            ((b"AC" * 80)[:150], revcomp((b"AC" * 80)[:150]), "period 2")]
    x, y = GENOME[600:640], GENOME[650:660]
    out += [(x + y + x, revcomp(x), "two equally good offsets"), (mutate(x + y + x, (5,)), revcomp(x), "the second has more matches")]
    out += [mates(120, 150, 60, at=47) + ("a trimmed mate 2 inside mate 1",), mates(200, 150, 60, at=47) + ("a trimmed mate 2 beyond mate 1",),
            mates(300, 320, 40, at=48) + ("a short mate 2 in the middle of a long mate 1",), mates(220, at=49) + ("overlapping in their middles",)]
    return out


@functools.lru_cache(maxsize=None)
def sample():
    """(index, [(mate 1, mate 2)] as (bases, [Phred])): the crafted pairs; 250 unrelated random pairs; 300 pairs cut from reads of an
    isolate (on and off the loci), 150 / 150 mates of inserts of 36 - 320 bases; pairs with read-through planted at EDGES and in the
    last unit"""
    idx, reads = rp.sample()
    rng = np.random.default_rng(99)
    pairs = [(m1, m2) for m1, m2, _ in crafted_pairs()]
    pairs += [(letters(rng, 150), letters(rng, 150)) for _ in range(250)]
    pairs += [mates_of(b.upper(), 150, 150) for b, _ in reads[5:1500:5]]
    order = rng.permutation(len(pairs))
    pairs = [pairs[int(k)] for k in order]
    for k, at in enumerate(EDGES):
        pairs.insert(at, mates(100 + k, at=60 + k))
    pairs.append(mates(77, at=80))
    assert len(pairs) <= 2500
    out = []
    for m1, m2 in pairs:
        out.append(((m1, [int(v) for v in rng.integers(30, 42, size=len(m1))]), (m2, [int(v) for v in rng.integers(30, 42, size=len(m2))])))
    return idx, out


def texts_of(pairs, base: int = 33):
    """(file 1, file 2, interleaved)"""
    t1 = rp.fastq_text([p[0] for p in pairs], base, header=rp.mate_header(0))
    t2 = rp.fastq_text([p[1] for p in pairs], base, header=rp.mate_header(1))
    inter = b"".join(rp.mate_header(f)(k) + b"\n" + r[0] + b"\n+\n" + bytes(v + base for v in r[1]) + b"\n" for k, p in enumerate(pairs) for f, r in enumerate(p))
    return t1, t2, inter


def split_mates(inter: bytes):
    """interleaved text -> (file 1, file 2)"""
    lines = inter.split(b"\n")[:-1]
    recs = [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines), 4)]
    return b"".join(recs[0::2]), b"".join(recs[1::2])


@functools.lru_cache(maxsize=None)
def raw_texts():
    return texts_of(sample()[1])


@functools.lru_cache(maxsize=None)
def expected(which: int):
    """(the text the engine must behave as if given, the counters) for SETTINGS[which]; computed once"""
    return trim_pair_overlap(raw_texts()[2], **SETTINGS[which])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(sample()[0])
    yield e
    e.close()


def begin(eng, setting=None, prep=None, adapters=None, stats: bool = False, dedup: bool = False):
    eng.reset_sample()
    eng.set_read_prep(**(prep or {}))
    eng.set_read_adapters(**(adapters or {"adapters": None}))
    eng.set_read_stats(stats)
    eng.set_read_dedup(dedup)
    if setting is None:
        eng.set_read_pair_overlap(False)
        assert eng.get_read_pair_overlap()["on"] is False
    else:
        eng.set_read_pair_overlap(True, **setting)
        assert eng.get_read_pair_overlap() == dict(setting, on=True)


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_pair_overlap_info()


# ------------------------------------------------------------------ one whole chunk
@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_one_whole_chunk_equals_the_cut_text(eng, which):
    idx, pairs = sample()
    _, _, raw = raw_texts()
    want_text, want_info = expected(which)
    assert want_info["pairs"] == len(pairs) and want_info["trimmed_pairs"] > 100 and want_info["overlapping"] > want_info["trimmed_pairs"]
    begin(eng, SETTINGS[which])
    assert eng.submit_fastq(raw, paired=True) == 2 * len(pairs)
    got = left_behind(eng)
    begin(eng)
    assert eng.submit_fastq(want_text, paired=True) == 2 * len(pairs)
    want = left_behind(eng)
    assert want[2] == ZERO
    assert {k: v for k, v in got[2].items() if k != "insert_hist"} == {k: v for k, v in want_info.items() if k != "insert_hist"}
    assert got[2]["insert_hist"] == want_info["insert_hist"]
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert int(got[1][0].n_hits.sum()) > 100, "the statistics are empty"
    # the guard: the raw text without the switch is another sample
    begin(eng)
    eng.submit_fastq(raw, paired=True)
    assert not np.array_equal(eng.debug_last_packed()[2], got[0][2])


def test_the_crafted_chunk_holds_what_it_says():
    """on the host: the plants are what their notes say, under the default setting"""
    idx, pairs = sample()
    want_text, info = expected(0)
    lens = dd.seq_lens(want_text)
    for k, at in enumerate(EDGES):                             # the edges carry a cut
        assert lens[2 * at:2 * at + 2] == [100 + k, 100 + k], at
    assert lens[-2:] == [77, 77]
    crafted = crafted_pairs()
    hit = {note: pair_overlap(m1, m2) for m1, m2, note in crafted}
    for o in range(-120, 121):
        assert hit["150 / 150 at o = %d" % o][0] == o
    for o in range(-67, 291):
        assert hit["320 / 97 at o = %d" % o][0] == o
    assert hit["L 30, 5 mismatches on mate 1"] == (-120, 25) and hit["L 30, 6 mismatches on mate 1"] is None
    assert hit["L 30, 5 mismatches on mate 2"] == (-120, 25) and hit["L 30, 6 mismatches on mate 2"] is None
    assert hit["L 100, 5 mismatches"] == (50, 95) and hit["L 100, 6 mismatches"] is None
    assert hit["L 10, 2 mismatches"] is None                  # (below the default minimum)
    assert pair_overlap(*crafted_by("L 10, 2 mismatches"), min_overlap=10) == (-30, 8) and pair_overlap(*crafted_by("L 10, 3 mismatches"), min_overlap=10) is None
    assert hit["N against N"] == (-90, 59) and hit["six Ns"] is None and hit["only N"] is None and hit["both in lower case"] == (-90, 60)
    assert hit["two equally good offsets"] == (0, 40) and hit["the second has more matches"] == (50, 40)
    assert hit["a trimmed mate 2 inside mate 1"] == (60, 60) and hit["a trimmed mate 2 beyond mate 1"] is None
    for n in LENGTHS:
        want = (-1, n - 1) if n - 1 >= 30 else None
        assert hit["%d / %d, insert %d" % (n, n, n - 1)] == want, n
    # the unrelated random pairs stay untouched
    rng = np.random.default_rng(99)
    assert sum(pair_overlap(letters(rng, 150), letters(rng, 150)) is not None for _ in range(250)) == 0


def crafted_by(note: str):
    return next((m1, m2) for m1, m2, n in crafted_pairs() if n == note)


# ------------------------------------------------------------------ the other four paired entries
def test_two_mate_texts(eng):
    idx, pairs = sample()
    t1, t2, _ = raw_texts()
    want_text, want_info = expected(0)
    begin(eng, DEFAULT)
    assert eng.submit_fastq_pair(t1, t2) == 2 * len(pairs)
    got = left_behind(eng)
    begin(eng)
    assert eng.submit_fastq_pair(*split_mates(want_text)) == 2 * len(pairs)
    want = left_behind(eng)
    assert got[2] == want_info and want[2] == ZERO
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])


def test_a_stream_cut_behind_every_pair_of_a_small_text(eng):
    idx, pairs = sample()
    few = pairs[240:300]                                      # (EDGES 255 - 257 among them)
    _, _, raw = texts_of(few)
    want_text, want_info = trim_pair_overlap(raw)
    assert want_info["trimmed_pairs"] > 10
    begin(eng)
    assert eng.submit_fastq(want_text, paired=True) == 2 * len(few)
    want_typed = typed(eng)
    starts = dd.record_starts(raw)
    begin(eng, DEFAULT)
    lens, n = dd.feed_stream(eng, raw, starts[2::2], paired=True)
    assert n == 2 * len(few) and lens == dd.seq_lens(want_text)
    assert eng.read_pair_overlap_info() == want_info
    assert_typed_equal(typed(eng), want_typed)
    # a paired chunk cut behind a first mate is refused
    begin(eng, DEFAULT)
    with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: a paired chunk holds 3 records"):
        eng.submit_fastq_stream(raw[:starts[3]], final=False, paired=True)
    eng.reset_sample()


def test_bgzip_with_blocks_cut_inside_records(eng):
    idx, pairs = sample()
    few = pairs[:700]
    t1, t2, raw = texts_of(few)
    want_text, want_info = trim_pair_overlap(raw)
    sizes = (4099, 6007, 9001, 2503)
    assert dd.cuts_inside_sequence_lines(raw, sizes) > 5
    blocks = bgzf_blocks(raw, sizes)
    begin(eng)
    eng.submit_fastq(want_text, paired=True)
    want_typed = typed(eng)
    for per_call in (1, 7, len(blocks)):
        begin(eng, DEFAULT)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks), paired=True) for k in range(0, len(blocks), per_call))
        assert n == 2 * len(few), per_call
        assert eng.read_pair_overlap_info() == want_info, per_call
        assert_typed_equal(typed(eng), want_typed)
    # bgzip'd mates with one file ahead
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    assert len(b1) > 12 and len(b2) > 45
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])), (b"".join(b1[9:10]), b"".join(b2[1:30])), (b"", b"".join(b2[30:40])), (b"".join(b1[10:]) + eof, b"".join(b2[40:]) + eof)]
    step = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    for what, calls in (("one file ahead", ahead), ("three blocks of each per call", step)):
        begin(eng, DEFAULT)
        n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
        assert n == 2 * len(few), what
        assert eng.read_pair_overlap_info() == want_info, what
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ the combinations
@functools.lru_cache(maxsize=None)
def chain_sample():
    """pairs for the whole chain: Phred+64 text whose mates carry six extra bases in front (--trim5 6 removes them), a decayed tail
    on every third mate 2, read-through on most pairs, and every fifth pair a copy of an earlier one (for --dedup)"""
    idx, reads = rp.sample()
    rng = np.random.default_rng(17)
    pairs = []
    for k, (b, _) in enumerate(reads[7:2400:6]):
        frag = b.upper()
        m1, m2 = mates_of(frag, 6 + 144, 6 + 144)
        q1, q2 = [int(v) for v in rng.integers(30, 42, size=len(m1))], [int(v) for v in rng.integers(30, 42, size=len(m2))]
        if k % 3 == 0:
            q2[-25:] = [2] * 25
        pairs.append(((m1, q1), (m2, q2)))
    for k in range(4, len(pairs), 5):
        pairs[k] = pairs[k - 3]
    return idx, pairs


PREP = {"trim5": 6, "trim_qual": 20, "phred64": True}


def test_behind_the_preparation_in_front_of_dedup_beside_the_read_statistics(eng):
    idx, pairs = chain_sample()
    _, _, raw = texts_of(pairs, 64)
    prepared, pinfo = prep_fastq(raw, **PREP)
    cut, ainfo = trim_adapters(prepared, [ADAPTER], 8, 100)
    over, oinfo = trim_pair_overlap(cut, trim5=6, **DEFAULT)
    want_text, dinfo = dedup_fastq(over, paired=True)
    assert pinfo["shortened"] == 2 * len(pairs) and ainfo["trimmed"] > 50 and oinfo["trimmed_pairs"] > 50 and dinfo["duplicates"] > 50
    assert oinfo != trim_pair_overlap(cut, **DEFAULT)[1] and oinfo != trim_pair_overlap(prepared, trim5=6, **DEFAULT)[1]      # the order and trim5 matter
    begin(eng, DEFAULT, PREP, {"adapters": [ADAPTER], "min_overlap": 8, "error_permille": 100}, stats=True, dedup=True)
    assert eng.submit_fastq(raw, paired=True) == 2 * len(pairs)
    got = left_behind(eng)
    stats = eng.read_stats()
    assert got[2] == oinfo and eng.read_prep_info() == pinfo and eng.read_adapters_info() == ainfo
    assert dd.rule_part(eng.read_dedup_info()) == dinfo
    begin(eng)
    assert eng.submit_fastq(want_text, paired=True) == 2 * len(pairs)
    want = left_behind(eng)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert int(got[1][0].n_hits.sum()) > 100
    # the prepared stage of the read statistics shows the cut reads (in front of the duplicates' removal), the raw stage the file's
    assert stats["prepared_counted"]
    for stage, text in (("raw", raw), ("prepared", over)):
        rule = read_stats(text, phred64=(stage == "raw"), paired=True)
        assert all(read_stats_equal(stats[stage][side], rule[side]) for side in (0, 1)), stage
    # the switch alone beside the statistics: the prepared stage is counted all the same
    _, _, raw33 = texts_of(pairs)
    over33, info33 = trim_pair_overlap(raw33, **DEFAULT)
    begin(eng, DEFAULT, stats=True)
    eng.submit_fastq(raw33, paired=True)
    stats = eng.read_stats()
    assert eng.read_pair_overlap_info() == info33 and stats["prepared_counted"] and eng.read_stats_info()["prepared_launches"] == 1
    rule = read_stats(over33, paired=True)
    assert all(read_stats_equal(stats["prepared"][side], rule[side]) for side in (0, 1))
    assert not read_stats_equal(stats["prepared"][0], stats["raw"][0])


def test_rows_are_as_wide_as_the_cut_text_when_every_longest_read_is_cut(eng):
    pairs = [mates(90 + k % 7, 320, 300, at=k) for k in range(40)] + [mates(400, 120, 110, at=k) for k in range(40)]
    pairs = [((m1, [40] * len(m1)), (m2, [40] * len(m2))) for m1, m2 in pairs]
    _, _, raw = texts_of(pairs)
    want_text, info = trim_pair_overlap(raw)
    assert max(dd.seq_lens(want_text)) == 120 and info["trimmed_pairs"] == 40
    begin(eng, DEFAULT)
    eng.submit_fastq(raw, paired=True)
    got = left_behind(eng)
    begin(eng)
    eng.submit_fastq(want_text, paired=True)
    want = left_behind(eng)
    assert got[0][3:] == want[0][3:] == (8, 120)
    rp.assert_packed_equal(got[0], want[0])


def test_export_bytes_are_those_of_the_cut_text(eng):
    idx, pairs = sample()
    _, _, raw = raw_texts()
    want_text, _ = expected(0)
    begin(eng)
    eng.submit_fastq(want_text, paired=True)
    off = b"".join(eng.export_reads_text(paired=True))
    sam_off = b"".join(eng.export_sam_text(idx, md=True))
    begin(eng, DEFAULT)
    eng.submit_fastq(raw, paired=True)
    on = b"".join(eng.export_reads_text(paired=True))
    assert on == off and on.count(b"\n") > 200
    assert b"".join(eng.export_sam_text(idx, md=True)) == sam_off
    begin(eng)
    eng.submit_fastq(raw, paired=True)
    assert b"".join(eng.export_reads_text(paired=True)) != off             # without the switch the adapter tails are exported


# ------------------------------------------------------------------ refusals and life cycle
def test_refusals_and_life_cycle():
    idx, pairs = sample()
    _, _, text = texts_of(pairs[:200])
    want_info = trim_pair_overlap(text)[1]
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        assert eng.get_read_pair_overlap() == dict(DEFAULT, on=False) and eng.read_pair_overlap_info() == ZERO
        for bad, why in (({"min_overlap": 7}, "min_overlap 7 is outside 8..320"), ({"min_overlap": 321}, "min_overlap 321 is outside 8..320"),
                         ({"max_mismatches": 65}, "max_mismatches 65 is outside 0..64"), ({"error_permille": 501}, "error_permille 501 is outside 0..500")):
            with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: " + why):
                eng.set_read_pair_overlap(True, **bad)
        assert eng.get_read_pair_overlap()["on"] is False
        eng.set_read_pair_overlap(True, 320, 64, 500)                         # the limits are taken
        eng.set_read_pair_overlap(True, 8, 0, 0)
        assert eng.get_read_pair_overlap() == {"on": True, "min_overlap": 8, "max_mismatches": 0, "error_permille": 0}
        eng.set_read_pair_overlap(False, 1, 999, 999)                         # off, whatever the numbers: the setting stays
        assert eng.get_read_pair_overlap() == {"on": False, "min_overlap": 8, "max_mismatches": 0, "error_permille": 0}
        # off: nothing is queued, nothing is allocated
        eng.set_profiling(1)
        eng.submit_fastq(text, paired=True)
        assert eng.kernel_time(22) == (0.0, 0) and eng.read_pair_overlap_info() == ZERO
        eng.reset_sample()
        eng.reset_kernel_time()
        eng.set_read_pair_overlap(True)
        assert eng.get_read_pair_overlap() == dict(DEFAULT, on=True)
        reads = rp.sample()[1]
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
        for entry, call in calls.items():
            with pytest.raises(MlstError, match=r"\(-1\): %s: mate overlap trimming is on \(mlst_set_read_pair_overlap\)" % entry):
                call()
        assert eng.get_read_tiling() == (0, 0)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: an unpaired FASTQ submission"):
            eng.submit_fastq(text)
        eng.reset_sample()
        assert eng.submit_fastq(text, paired=True) == 400                      # the handle stays usable
        ms, launches = eng.kernel_time(22)
        assert launches == 1 and ms > 0 and eng.kernel_time(6)[0] >= ms      # k_po_cut alone, inside 6
        eng.set_profiling(0)
        assert eng.read_pair_overlap_info() == want_info and want_info["trimmed_pairs"] > 10
        for change in (lambda: eng.set_read_pair_overlap(False), lambda: eng.set_read_pair_overlap(True, 31)):
            with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_pair_overlap"):
                change()
        eng.set_read_pair_overlap(True, **DEFAULT)                            # (no change: accepted)
        assert eng.submit_fastq(text, paired=True) == 400                      # the counters add up over the sample's chunks
        twice = eng.read_pair_overlap_info()
        assert twice["pairs"] == 400 and twice["bases_removed"] == 2 * want_info["bases_removed"] and twice["insert_hist"] == [2 * v for v in want_info["insert_hist"]]
        eng.reset_sample()                                                     # keeps the switch, zeroes the counters
        assert eng.get_read_pair_overlap() == dict(DEFAULT, on=True) and eng.read_pair_overlap_info() == ZERO
        eng.submit_fastq_stream(text[:1000], final=False, paired=True)         # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_pair_overlap(False)
        eng.reset_sample()
        eng.set_read_pair_overlap(False)
        eng.submit_reads(fb, fq, off)                                          # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_pair_overlap(True)
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: mlst_set_read_tiling is on"):
            eng.set_read_pair_overlap(True)
        eng.set_read_pair_overlap(False)                                       # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_pair_overlap(True)
        eng.submit_fastq(text, paired=True)
        eng.reset_sample()
        eng.set_read_pair_overlap(False)
        eng.submit_fastq(text, paired=True)
        got = left_behind(eng)
        fresh = Engine(0, default_params())
        try:
            fresh.load_reference(idx)
            fresh.submit_fastq(text, paired=True)
            want = left_behind(fresh)
        finally:
            fresh.close()
        assert got[2] == want[2] == ZERO
        rp.assert_packed_equal(got[0], want[0])
        assert_typed_equal(got[1], want[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ the command
@functools.lru_cache(maxsize=None)
def command_pairs():
    """fragments of 50 - 260 bases tiled over the alleles of the planted ST, 100 / 100 mates at Phred 40: the shorter ones run into
    the adapters"""
    db, idx = dd.command_db()
    pairs = []
    for a in rp.true_alleles(db, idx):
        seq = idx.sequence(a).encode().upper()
        for k, s in enumerate(range(0, len(seq) - 260, 3)):
            m1, m2 = mates_of(seq[s:s + 50 + (37 * k) % 211], 100, 100)
            pairs.append(((m1, [40] * 100), (m2, [40] * 100)))
    return pairs


def test_cli_pair_overlap_types_read_through_as_the_cut_text(tmp_path, monkeypatch, capsys):
    pairs = command_pairs()
    _, _, inter = texts_of(pairs)
    rule_text, info = trim_pair_overlap(inter)
    assert info["trimmed_pairs"] > len(pairs) // 6 and info["overlapping"] > info["trimmed_pairs"]
    eof = bgzf_blocks(b"")[-1]
    for d, text in (("raw", inter), ("rule", rule_text)):
        os.makedirs(tmp_path / d)
        for f, t in enumerate(split_mates(text)):
            (tmp_path / d / ("m_%d.fastq" % (f + 1))).write_bytes(t)
            (tmp_path / d / ("g_%d.fastq.gz" % (f + 1))).write_bytes(gzip.compress(t, 1))
            (tmp_path / d / ("b_%d.fastq.gz" % (f + 1))).write_bytes(b"".join(bgzf_blocks(t, (30011, 20201))))
    for stem in ("m_%d.fastq", "g_%d.fastq.gz", "b_%d.fastq.gz"):
        args = [stem % 1, "-2", stem % 2]
        tag = stem[0]
        dd.run_type(monkeypatch, capsys, tmp_path / "rule", args + ["--quiet"], tmp_path / (tag + "_rule"))
        said = dd.run_type(monkeypatch, capsys, tmp_path / "raw", args + ["--pair-overlap"], tmp_path / (tag + "_raw"))
        want, got = rp.written(tmp_path / (tag + "_rule")), rp.written(tmp_path / (tag + "_raw"))
        assert got == want and len(want) == 2 and all(len(v) > 0 for v in want.values()), stem
        assert cli.read_pair_overlap_line(info) in said and dd.names_the_planted_st(said), (stem, said[-400:])
    quiet = dd.run_type(monkeypatch, capsys, tmp_path / "raw", ["m_1.fastq", "-2", "m_2.fastq", "--pair-overlap", "--quiet"], tmp_path / "o_quiet")
    assert "mate overlap trimming" not in quiet and rp.written(tmp_path / "o_quiet") == rp.written(tmp_path / "m_rule")
    # with the other steps of the chain and the exports: they carry the cut SEQ / QUAL, and the prepared statistics show the cut reads
    flags = ["--pair-overlap", "--pair-overlap-min", "20", "--pair-overlap-diff", "3", "--pair-overlap-rate", "0.1"]
    chain_text, chain_info = trim_pair_overlap(inter, 20, 3, 100)
    for f, t in enumerate(split_mates(chain_text)):
        (tmp_path / "rule" / ("c_%d.fastq" % (f + 1))).write_bytes(t)
        (tmp_path / "raw" / ("c_%d.fastq" % (f + 1))).write_bytes(split_mates(inter)[f])
    more = ["--write-sam", "--write-sam-all", "--write-reads", "--md", "--read-names", "--dedup"]
    dd.run_type(monkeypatch, capsys, tmp_path / "rule", ["c_1.fastq", "-2", "c_2.fastq", "--quiet"] + more, tmp_path / "c_rule")
    said = dd.run_type(monkeypatch, capsys, tmp_path / "raw", ["c_1.fastq", "-2", "c_2.fastq", "--read-stats"] + more + flags, tmp_path / "c_raw")
    want, got = rp.written(tmp_path / "c_rule"), rp.written(tmp_path / "c_raw")
    assert cli.read_pair_overlap_line(chain_info) in said, said[-600:]
    assert sorted(got) == sorted(list(want) + ["c_1.readstats.tsv"]) and len(want) == 5
    assert all(got[k] == want[k] for k in want) and want["c_1.all.sam"].count(b"\n") > 500
    rule = read_stats(chain_text, paired=True)
    assert b"prepared" in got["c_1.readstats.tsv"]
    assert "read statistics (prepared, side 0): %d reads, %d bases," % (rule[0]["reads"], rule[0]["bases"]) in said, said[-800:]
    assert "read statistics (prepared, side 1): %d reads, %d bases," % (rule[1]["reads"], rule[1]["bases"]) in said
