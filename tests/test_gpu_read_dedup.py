"""mlst_set_read_dedup (csrc/read_dedup.h): exact duplicate reads emptied on the device before they are packed.  The yardstick everywhere:
the engine with the switch ON and the RAW text must leave what the same engine leaves with the switch OFF and the text
fastq.dedup_fastq writes -- the packed rows byte for byte (mlst_debug_last_packed), the typed statistics, the counters -- through every
entry that takes FASTQ text, however the text is cut into chunks; then the table's growth, the clash path (MLST_DEDUP_TAG_BITS), the
exports, the refusals and the life cycle, and `cli type --dedup`.  dedup_fastq itself is pinned by hand in test_read_dedup_host.py."""
import functools
import os
import re

import numpy as np
import pytest

import fixtures as fx
import read_names_cases as rc
import test_gpu_read_prep as rp
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import dedup_fastq, prep_fastq, read_stats_equal, trim_adapters
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_sam_all import assert_rule_bytes, export

pytestmark = pytest.mark.gpu

RULE_KEYS = ("reads", "units", "duplicates", "reads_removed", "bases_removed", "distinct", "levels")
ZERO = {"reads": 0, "units": 0, "duplicates": 0, "reads_removed": 0, "bases_removed": 0, "distinct": 0, "clashes": 0, "slots": 0, "levels": [0] * 8}
FOLD = bytes(c if c in b"ACGT" else (c & 0xDF if (c & 0xDF) in b"ACGT" else 78) for c in range(256))
ADAPTER = "AGATCGGAAGAGC"


@functools.lru_cache(maxsize=None)
def distinct_reads():
    """(index, 300 reads of 36 - 320 bases with 300 different keys, some with non-ACGT bases)"""
    idx, reads = rp.sample()
    seen, out = set(), []
    for b, q in reads[:260] + reads[2350:]:      # (short reads, then long ones)
        key = b.translate(FOLD)
        if len(b) >= 36 and key not in seen:
            seen.add(key)
            out.append((b, q))
        if len(out) == 300:
            break
    assert len(out) == 300 and any(b"N" in b for b, _ in out) and max(len(b) for b, _ in out) == 320
    return idx, out


@functools.lru_cache(maxsize=None)
def corpus():
    """1,100 units of the 300 reads, five workgroups of 256 threads: copies in the same wave, in different waves of a workgroup, in
    different workgroups, and at units 63, 64, 65, 255, 256, 257 of the launch; two empty reads; the rest filled with the other reads
    in turn, so that every one of them occurs three or four times"""
    idx, d = distinct_reads()
    units = [None] * 1100
    for k, where in enumerate(((3, 7), (5, 6), (10, 100, 200), (20, 300, 700, 1050), (63, 64), (65, 255), (256, 257), (1, 62, 254, 258), (511, 512), (767, 768, 1023, 1024))):
        for u in where:
            units[u] = d[k]
    units[40] = units[900] = (b"", [])
    rest = iter(d[10:] * 5)
    units = [u if u is not None else next(rest) for u in units]
    lower = {7, 100, 300, 64}      # (a copy in the other case is a copy)
    return idx, [(b.lower(), q) if k in lower else (b, q) for k, (b, q) in enumerate(units)]


def record_starts(text: bytes) -> list:
    """the byte at which every record of FASTQ text starts"""
    out, at = [], 0
    for k, line in enumerate(text.split(b"\n")[:-1]):
        if k % 4 == 0:
            out.append(at)
        at += len(line) + 1
    return out


def seq_lens(text: bytes) -> list:
    return [len(x) for x in text.split(b"\n")[1::4]]


def got_lens(eng) -> list:
    return [int(v) & 0x7FFF for v in eng.debug_last_packed()[2]]


def rule_part(info: dict) -> dict:
    return {k: info[k] for k in RULE_KEYS}


def load(idx):
    e = Engine(0, default_params())
    e.load_reference(idx)
    return e


@pytest.fixture(scope="module")
def eng():
    e = load(rp.sample()[0])
    yield e
    e.close()


def begin(eng, on: bool, prep=None, adapters=None, stats: bool = False):
    eng.reset_sample()
    eng.set_read_prep(**(prep or {}))
    eng.set_read_adapters(adapters)
    eng.set_read_stats(stats)
    eng.set_read_dedup(on)
    assert eng.get_read_dedup() is on


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_dedup_info()


def assert_equals_the_rule(eng, raw: bytes, paired: bool = False, submit=None):
    """one whole chunk: ON and raw against OFF and the rule's text; -> what ON left behind"""
    submit = submit or (lambda e, t: e.submit_fastq(t, paired=paired))
    want_text, want_info = dedup_fastq(raw, paired)
    begin(eng, True)
    n = submit(eng, raw)
    got = left_behind(eng)
    begin(eng, False)
    assert eng.submit_fastq(want_text, paired=paired) == n == want_info["reads"]
    want = left_behind(eng)
    assert want[2] == ZERO
    assert rule_part(got[2]) == want_info and got[2]["clashes"] == 0, (got[2], want_info)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    return got


# ------------------------------------------------------------------ one whole chunk
def test_one_whole_chunk_equals_the_rules_text(eng):
    idx, units = corpus()
    raw = rp.fastq_text(units)
    want_info = dedup_fastq(raw)[1]
    assert want_info["distinct"] == 300 and want_info["units"] == 1098 and want_info["duplicates"] == 798 and want_info["levels"][2] + want_info["levels"][3] > 280
    got = assert_equals_the_rule(eng, raw)
    lens = [int(v) & 0x7FFF for v in got[0][2]]
    for first, copies in ((3, (7,)), (5, (6,)), (10, (100, 200)), (20, (300, 700, 1050)), (63, (64,)), (65, (255,)), (256, (257,)), (1, (62, 254, 258)), (511, (512,)), (767, (768, 1023, 1024))):
        assert lens[first] == len(units[first][0]) > 0 and all(lens[c] == 0 for c in copies), first
    assert got[2]["slots"] == 1 << 22 and int(got[1][0].n_hits.sum()) > 50, "the statistics are empty"
    # the raw text without the switch is another sample: the test would pass on an engine that ignored the switch otherwise
    begin(eng, False)
    eng.submit_fastq(raw)
    assert got_lens(eng) == [len(b) for b, _ in units] != lens


LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 319, 320)      # the 16-byte load edges and the 32-base word edges
ROT = bytes.maketrans(b"ACGT", b"CGTA")


def one_place_pairs():
    """[(n, what, first read, second read, is the second a copy)]"""
    rng = np.random.default_rng(77)
    out = []
    for n in LENGTHS:
        def fresh():
            return bytes(b"ACGT"[v] for v in rng.integers(0, 4, size=n))
        b = fresh(); out.append((n, "last base", b, b[:-1] + b[-1:].translate(ROT), False))
        b = fresh(); out.append((n, "first base", b, b[:1].translate(ROT) + b[1:], False))
        if n > 1:
            b = fresh(); out.append((n, "a prefix", b, b[:-1], False))
        b = fresh(); out.append((n, "case", b, b.lower(), True))
        for at in (n - 1, 0, n // 2):
            b = fresh(); out.append((n, "N against R at %d" % at, b[:at] + b"N" + b[at + 1:], b[:at] + b"R" + b[at + 1:], True))
            b = fresh(); out.append((n, "N against . at %d" % at, b[:at] + b"n" + b[at + 1:], b[:at] + b"." + b[at + 1:], True))
            b = fresh(); out.append((n, "N against A at %d" % at, b[:at] + b"N" + b[at + 1:], b[:at] + b"A" + b[at + 1:], False))
    return out


def test_reads_that_differ_in_one_place_only(eng):
    cases = one_place_pairs()
    reads = []
    for n, what, a, b, dup in cases:
        assert seq_lens(dedup_fastq(rp.fastq_text([(a, [40] * len(a)), (b, [40] * len(b))]))[0]) == [len(a), 0 if dup else len(b)], (n, what)      # the rule on the two alone
        reads += [(a, [40] * len(a)), (b, [40] * len(b))]
    got = assert_equals_the_rule(eng, rp.fastq_text(reads))
    lens = [int(v) & 0x7FFF for v in got[0][2]]
    for k, (n, what, a, b, dup) in enumerate(cases):
        if n >= 15:      # (at one base the cases meet each other: the rule's text above holds them)
            assert lens[2 * k] == len(a) and lens[2 * k + 1] == (0 if dup else len(b)), (n, what)


# ------------------------------------------------------------------ across chunks
def feed_stream(eng, text: bytes, cuts, paired: bool = False):
    """the text in pieces cut at the bytes `cuts`; -> (lengths of all reads, reads counted)"""
    lens, n, at = [], 0, 0
    for cut in list(cuts) + [len(text)]:
        k = eng.submit_fastq_stream(text[at:cut], final=cut == len(text), paired=paired)
        if k:
            lens += got_lens(eng)
        n += k
        at = cut
    return lens, n


def test_the_same_text_in_one_chunk_and_in_many(eng):
    idx, units = corpus()
    raw = rp.fastq_text(units)
    want_text, want_info = dedup_fastq(raw)
    starts = record_starts(raw)
    assert len(starts) == len(units)
    inside_64 = starts[64] + len(rc.illumina(64)) + 1 + 30      # inside the sequence line of the copy of unit 63
    feeds = {"one chunk": [], "first occurrence and copy apart": [inside_64], "between units 256 and 257": [starts[257]],
             "about 20 chunks": [len(raw) * k // 20 for k in range(1, 20)], "a chunk per 64 reads": starts[64::64]}
    assert starts[20] < feeds["about 20 chunks"][0] < starts[300]
    begin(eng, False)
    eng.submit_fastq(want_text)
    want_typed = typed(eng)
    for what, cuts in feeds.items():
        begin(eng, True)
        lens, n = feed_stream(eng, raw, cuts)
        assert n == len(units) and lens == seq_lens(want_text), what
        info = eng.read_dedup_info()
        assert rule_part(info) == want_info and info["clashes"] == 0, what
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ growth
@functools.lru_cache(maxsize=None)
def growth_text():
    idx, reads = rp.sample()
    rng = np.random.default_rng(5)
    pick = rng.integers(0, 1500, size=5000)
    units = [(reads[k][0][:60], reads[k][1][:60]) for k in pick]
    return rp.fastq_text(units), len(units)


def test_the_table_grows_by_rehashing(eng, monkeypatch):
    raw, n_units = growth_text()
    want_text, want_info = dedup_fastq(raw)
    assert want_info["duplicates"] > 3000 and want_info["distinct"] > 1000
    starts = record_starts(raw)
    cuts = [starts[k] for k in (20, 50, 110, 230, 470, 950, 1900, 3000, 4000)]      # 64 slots hold 32 units: every cut but the last two doubles them
    begin(eng, True)
    lens_default, _ = feed_stream(eng, raw, cuts)
    info_default, typed_default = eng.read_dedup_info(), typed(eng)
    assert info_default["slots"] == 1 << 22 and lens_default == seq_lens(want_text) and rule_part(info_default) == want_info
    monkeypatch.setenv("MLST_DEDUP_SLOTS", "64")
    small = load(rp.sample()[0])
    try:
        small.set_read_dedup(True)
        lens, at, sizes = [], 0, []
        for cut in cuts + [len(raw)]:
            assert small.submit_fastq_stream(raw[at:cut], final=cut == len(raw)) > 0
            lens += got_lens(small)
            sizes.append(small.read_dedup_info()["slots"])
            at = cut
        assert sizes[0] == 64 and sizes[-1] == 16384 and len(set(sizes)) - 1 >= 6, sizes      # at least six rehashes
        assert lens == lens_default
        info = small.read_dedup_info()
        assert dict(info, slots=0) == dict(info_default, slots=0)
        assert_typed_equal(typed(small), typed_default)
        # the table keeps its size behind a reset, and is empty
        small.reset_sample()
        assert small.submit_fastq(raw) == n_units and got_lens(small) == lens_default
        assert small.read_dedup_info() == info
    finally:
        small.close()
    for bad in ("100", "32", "0", "-64"):
        monkeypatch.setenv("MLST_DEDUP_SLOTS", bad)
        other = load(rp.sample()[0])
        try:
            other.set_read_dedup(True)
            with pytest.raises(MlstError, match=r"\(-1\): MLST_DEDUP_SLOTS is %s: a power of two" % bad):
                other.submit_fastq(raw[:starts[10]])
        finally:
            other.close()


# ------------------------------------------------------------------ the clash path
def test_clash_path_with_no_tag_bits_every_unit_meets_one_slot(monkeypatch):
    """the outcome needs no knowledge of the hash: the later copies of the very first non-empty unit go, every other unit is kept"""
    idx, units = corpus()
    units = [(b"", [])] + units      # (the very first unit is empty: it takes no part)
    raw = rp.fastq_text(units)
    first = units[1][0].translate(FOLD)
    copies = [k for k, (b, _) in enumerate(units) if k > 1 and b.translate(FOLD) == first]
    assert len(copies) == 3
    monkeypatch.setenv("MLST_DEDUP_TAG_BITS", "0")
    e = load(idx)
    try:
        e.set_read_dedup(True)
        starts = record_starts(raw)
        for cuts in ([], starts[100::100]):
            e.reset_sample()
            lens, n = feed_stream(e, raw, cuts)
            assert n == len(units) and lens == [0 if k in copies else len(b) for k, (b, _) in enumerate(units)]
            n_units = sum(len(b) > 0 for b, _ in units)
            assert e.read_dedup_info() == {"reads": len(units), "units": n_units, "duplicates": 3, "reads_removed": 3, "bases_removed": 3 * len(first), "distinct": 1,
                                           "clashes": n_units - 4, "slots": 1 << 22, "levels": [0, 0, 0, 1, 0, 0, 0, 0]}
    finally:
        e.close()


def test_clash_path_with_four_tag_bits_never_removes_a_first_occurrence(monkeypatch):
    idx, units = corpus()
    raw = rp.fastq_text(units)
    rule = seq_lens(dedup_fastq(raw)[0])
    starts = record_starts(raw)
    monkeypatch.setenv("MLST_DEDUP_TAG_BITS", "4")
    e = load(idx)
    try:
        e.set_read_dedup(True)
        runs = []
        for cuts in ([], [], starts[50::50], [len(raw) * k // 20 for k in range(1, 20)]):
            e.reset_sample()
            lens, n = feed_stream(e, raw, cuts)
            info = e.read_dedup_info()
            runs.append((lens, info))
            assert n == len(units)
            gone = [k for k, (b, _) in enumerate(units) if len(b) and not lens[k]]
            assert all(rule[k] == 0 for k in gone), "a read that is no duplicate was removed"
            assert all(lens[k] in (0, len(b)) for k, (b, _) in enumerate(units))
            assert 0 < len(gone) == info["duplicates"] < 798 and info["clashes"] > 0 and info["distinct"] <= 16
            assert info["units"] == 1098 and info["duplicates"] + info["clashes"] + info["distinct"] == info["units"]
        assert all(r == runs[0] for r in runs[1:])
    finally:
        e.close()


# ------------------------------------------------------------------ pairs
@functools.lru_cache(maxsize=None)
def pair_texts():
    idx, d = distinct_reads()
    e = (b"", [])
    A, B, C = d[0], d[1], d[2]
    pairs = [(A, B), (A, C), (B, A), ((A[0].lower(), A[1]), B), (A, e), (e, A), (A, e), (e, e), (e, e), (e, A), (A, B)]
    rng = np.random.default_rng(11)
    pool = [(d[int(a)], d[int(b)]) for a, b in rng.integers(3, 300, size=(300, 2))]
    pairs += [pool[int(k)] for k in rng.integers(0, 300, size=700)]
    m1, m2 = [p[0] for p in pairs], [p[1] for p in pairs]
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    inter = b"".join(rp.mate_header(f)(k) + b"\n" + r[0] + b"\n+\n" + bytes(v + 33 for v in r[1]) + b"\n" for k, p in enumerate(pairs) for f, r in enumerate(p))
    return pairs, t1, t2, inter


def test_pairs_through_every_paired_entry(eng):
    pairs, t1, t2, inter = pair_texts()
    want_text, want_info = dedup_fastq(inter, paired=True)
    lens = seq_lens(want_text)
    A, B, C = pairs[0][0][0], pairs[0][1][0], pairs[1][1][0]
    assert lens[:22] == [len(A), len(B), len(A), len(C), len(B), len(A), 0, 0, len(A), 0, 0, len(A), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert want_info["units"] == len(pairs) - 2 and want_info["duplicates"] > 300 and want_info["reads_removed"] == 2 * want_info["duplicates"]
    got = assert_equals_the_rule(eng, inter, paired=True)
    # the same pairs typed as unpaired reads are another sample
    assert dedup_fastq(inter)[1]["duplicates"] != want_info["duplicates"]
    assert_equals_the_rule(eng, inter, paired=True, submit=lambda e, t: e.submit_fastq_pair(t1, t2))
    # an interleaved stream cut between pairs
    starts = record_starts(inter)
    begin(eng, True)
    got_l, n = feed_stream(eng, inter, starts[200::200], paired=True)
    assert n == 2 * len(pairs) and got_l == lens and rule_part(eng.read_dedup_info()) == want_info
    assert_typed_equal(typed(eng), got[1])
    # bgzip'd mates with one file ahead
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    assert len(b1) > 12 and len(b2) > 45
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])), (b"".join(b1[9:10]), b"".join(b2[1:30])), (b"", b"".join(b2[30:40])), (b"".join(b1[10:]) + eof, b"".join(b2[40:]) + eof)]
    step = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    for what, calls in (("one file ahead", ahead), ("three blocks of each per call", step)):
        begin(eng, True)
        n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
        assert n == 2 * len(pairs), what
        info = eng.read_dedup_info()
        assert rule_part(info) == want_info and info["clashes"] == 0, what
        assert_typed_equal(typed(eng), got[1])


# ------------------------------------------------------------------ bgzip
def cuts_inside_sequence_lines(text: bytes, sizes) -> int:
    kind, at = {}, 0
    for k, line in enumerate(text.split(b"\n")):
        kind[at] = (k % 4, at + len(line))
        at += len(line) + 1
    starts = sorted(kind)
    n, cut, j = 0, 0, 0
    while cut + sizes[j % len(sizes)] < len(text):
        cut += sizes[j % len(sizes)]
        j += 1
        s = starts[np.searchsorted(starts, cut, side="right") - 1]
        n += kind[s][0] == 1 and s < cut < kind[s][1]
    return n


def test_bgzip_pieces_row_by_row(eng):
    """a block per call, the rows of every piece: reads whose sequence line is cut by a block end are compared once and whole"""
    idx, units = corpus()
    few = units[:400]
    raw = rp.fastq_text(few)
    sizes = (1201, 2203, 777)
    assert cuts_inside_sequence_lines(raw, sizes) > 10
    blocks = bgzf_blocks(raw, sizes)
    want_text, want_info = dedup_fastq(raw)
    begin(eng, False)
    eng.submit_fastq(want_text)
    want_reads, want_typed = rp.reads_of(eng), typed(eng)
    begin(eng, True)
    got, seen = [], 0
    for k, b in enumerate(blocks):
        eng.submit_fastq_bgzf(b, final=k == len(blocks) - 1)
        eng.synchronize()                    # (finishes the piece in flight)
        total = int(eng.stats().counters[2])
        if total > seen:                     # this call's piece completed records: the last pack is theirs
            piece = rp.reads_of(eng)
            assert len(piece) == total - seen, k
            got += piece
            seen = total
    assert seen == len(few) and got == want_reads
    assert rule_part(eng.read_dedup_info()) == want_info and want_info["duplicates"] > 100
    assert_typed_equal(typed(eng), want_typed)
    for per_call in (7, len(blocks)):
        begin(eng, True)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == len(few) and rule_part(eng.read_dedup_info()) == want_info, per_call
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ behind the preparation
def test_behind_the_preparation_and_beside_the_read_statistics(eng):
    idx, reads = rp.sample()
    rng = np.random.default_rng(3)
    body, body2 = rp.locus_bases(idx, 100, 4), rp.locus_bases(idx, 80, 9)

    def junk(n):
        return bytes(b"ACGT"[v] for v in rng.integers(0, 4, size=n))
    crafted = [(body + junk(20), [40] * 100 + [3] * 20), (body + junk(20), [40] * 100 + [3] * 20),                      # they differ in the tail --trim-qual removes
               (body2 + ADAPTER.encode() + junk(12), [40] * 105), (body2 + ADAPTER.encode() + junk(30), [40] * 123)]      # ... and behind the adapter
    few = reads[:300] + crafted[:1] + reads[300:600] + crafted[2:3] + reads[:150] + crafted[1:2] + crafted[3:]
    raw = rp.fastq_text(few)
    prep = {"trim_qual": 20}
    cut_text = trim_adapters(prep_fastq(raw, **prep)[0], [ADAPTER])[0]
    want_text, want_info = dedup_fastq(cut_text)
    assert seq_lens(want_text)[300] == 100 and seq_lens(want_text)[601] == 80 and seq_lens(want_text)[-3:] == [0, 0, 0] and seq_lens(dedup_fastq(raw)[0])[-2:] == [120, 123]
    begin(eng, True, prep, [ADAPTER])
    assert eng.submit_fastq(raw) == len(few)
    got = left_behind(eng)
    begin(eng, False)
    eng.submit_fastq(want_text)
    want = left_behind(eng)
    assert rule_part(got[2]) == want_info and want_info["duplicates"] > 100
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    # the read statistics are counted in front of the duplicates' removal: the tables are those without the switch
    tables = []
    for on in (False, True):
        begin(eng, on, prep, [ADAPTER], stats=True)
        eng.submit_fastq(raw)
        tables.append(eng.read_stats())
    for stage in ("raw", "prepared"):
        assert all(read_stats_equal(tables[0][stage][side], tables[1][stage][side]) for side in (0, 1)), stage
    assert tables[1]["prepared_counted"] and tables[1]["prepared"][0]["reads"] == len(few)
    assert rule_part(eng.read_dedup_info()) == want_info
    # alone beside the statistics (neither a trim nor an adapter): one raw launch, the duplicates still go
    begin(eng, True, stats=True)
    eng.submit_fastq(raw)
    assert rule_part(eng.read_dedup_info()) == dedup_fastq(raw)[1] and eng.read_stats_info()["prepared_launches"] == 0


# ------------------------------------------------------------------ the longest length
def test_a_chunk_whose_only_longest_read_is_a_duplicate_has_narrow_rows(eng):
    idx, d = distinct_reads()
    long_ = next(r for r in d if len(r[0]) == 320)
    short = [(b[:100], q[:100]) for b, q in d[5:205]]
    first, second = [long_] + short[:100], short[100:150] + [long_] + short[150:]
    raw = rp.fastq_text(first + second)
    want_text = dedup_fastq(raw)[0]
    cut = record_starts(raw)[len(first)]
    begin(eng, True)
    eng.submit_fastq(raw[:cut])
    assert eng.debug_last_packed()[3:] == (20, 320)
    eng.submit_fastq(raw[cut:])
    got = eng.debug_last_packed()
    begin(eng, False)
    eng.submit_fastq(want_text[:cut])
    eng.submit_fastq(want_text[cut:])      # (the rule's text is shorter by the duplicate's lines only behind the cut)
    want = eng.debug_last_packed()
    assert got[3:] == want[3:] == (8, 104)
    rp.assert_packed_equal(got, want)
    assert [int(v) for v in got[2]][50] == 0


# ------------------------------------------------------------------ the exports
def test_export_bytes_are_those_of_the_rules_text(eng, tmp_path):
    idx, units = corpus()
    raw = rp.fastq_text(units)
    want_text = dedup_fastq(raw)[0]
    begin(eng, False)
    eng.submit_fastq(want_text)
    recs_off, body_off = export(eng, idx, tmp_path / "off.all.sam")
    reads_off = b"".join(eng.export_reads_text())
    begin(eng, True)
    eng.submit_fastq(raw)
    recs_on, body_on = export(eng, idx, tmp_path / "on.all.sam")
    assert body_on == body_off and len(recs_on) > 50
    assert_rule_bytes(idx, recs_on, body_on)
    assert b"".join(eng.export_reads_text()) == reads_off and reads_off.count(b"\n") >= 4 * 20
    begin(eng, False)
    eng.submit_fastq(raw)
    assert b"".join(eng.export_reads_text()) != reads_off      # (without the switch the copies are exported too)
    # with the reads' own names: the header lines are not touched, so the names are the file's
    other = load(idx)
    try:
        out = []
        for on, text in ((True, raw), (False, want_text)):
            other.reset_sample()
            other.set_read_dedup(on)
            other.set_read_names(True)
            other.submit_fastq(text)
            out.append((b"".join(other.export_sam_text(idx, md=True)), b"".join(other.export_reads_text()), other.read_names()))
        assert out[0] == out[1] and len(out[0][2]) >= 20
        heads = rc.yardstick([raw])
        assert all(heads[ri].startswith(b"@" + nm) for ri, nm in out[0][2].items())
    finally:
        other.close()


# ------------------------------------------------------------------ refusals and life cycle
def test_refusals_and_life_cycle():
    idx, units = corpus()
    text = rp.fastq_text(units[:400])
    want_info = dedup_fastq(text)[1]
    eng = load(idx)
    try:
        assert eng.get_read_dedup() is False and eng.read_dedup_info() == ZERO
        b0, q0 = units[0]
        fb = np.frombuffer(b0, np.uint8); fq = np.frombuffer(bytes(v + 33 for v in q0), np.uint8); off = np.array([0, len(fb)], np.uint64)
        calls = {
            "mlst_submit_reads": lambda: eng.submit_reads(fb, fq, off),
            "mlst_submit_reads_device": lambda: eng.submit_reads_device(0, 0, 0, 1, 150),
            "mlst_submit_packed_device": lambda: eng.submit_packed_device(0, 0, 0, 1, 10, 152),
            "mlst_submit_packed_host": lambda: eng._check(eng.lib.mlst_submit_packed_host(eng._h, None, None, None, 1, 10, 152, 0), "mlst_submit_packed_host"),
            "mlst_submit_fasta": lambda: eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n"),
            "mlst_bam_reads_open": lambda: eng.bam_reads_open(0),
            "mlst_set_read_tiling": lambda: eng.set_read_tiling(150, 25),
        }
        eng.set_read_dedup(True)
        assert eng.read_dedup_info() == ZERO      # (nothing is allocated before the first submission)
        for entry, call in calls.items():
            with pytest.raises(MlstError, match=r"\(-1\): %s: duplicate removal is on \(mlst_set_read_dedup\) and only the FASTQ text and BGZF entries apply it" % entry):
                call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text) == 400                                 # the handle stays usable
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_dedup"):
            eng.set_read_dedup(False)
        eng.set_read_dedup(True)                                             # (no change: accepted)
        assert rule_part(eng.read_dedup_info()) == want_info
        eng.reset_sample()                                                   # keeps the switch, zeroes counters and table
        assert eng.get_read_dedup() is True
        assert eng.read_dedup_info() == dict(ZERO, slots=1 << 22)
        assert eng.submit_fastq(text) == 400                                 # the same text again: the same counters, not all duplicates
        assert rule_part(eng.read_dedup_info()) == want_info and want_info["duplicates"] < 300
        lens = got_lens(eng)
        assert eng.submit_fastq(text) == 400                                 # and without a reset: every unit is a copy
        again = eng.read_dedup_info()
        assert again["duplicates"] == want_info["duplicates"] + want_info["units"] and again["distinct"] == want_info["distinct"] and not any(got_lens(eng))
        eng.reset_sample()
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_dedup(False)
        eng.reset_sample()
        cut = record_starts(text)[3]
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_dedup: a paired chunk holds 3 records"):
            eng.submit_fastq_stream(text[:cut], final=False, paired=True)
        eng.reset_sample()
        eng.set_read_dedup(False)
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_dedup(True)
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_dedup: mlst_set_read_tiling is on"):
            eng.set_read_dedup(True)
        eng.set_read_dedup(False)                                            # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_dedup(True)
        eng.submit_fastq(text)
        assert got_lens(eng) == lens
        eng.reset_sample()
        eng.set_read_dedup(False)
        eng.submit_fastq(text)
        got = left_behind(eng)
        fresh = load(idx)
        try:
            fresh.submit_fastq(text)
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
def command_db():
    """the small fixture database without indel alleles: error-free reads of an ST's alleles are typed as that ST"""
    return fx.ecoli_small(40, 0)


def run_type(monkeypatch, capsys, cwd, args, out):
    """test_gpu_read_prep.run_type on command_db()"""
    monkeypatch.chdir(cwd)
    got = cli.main(["type"] + args + ["-d", command_db()[0].path, "--min_accuracy", "0", "--nloci", "0", "--log", "-o", str(out)])
    said = capsys.readouterr().out
    assert got == 0, said
    return said


@functools.lru_cache(maxsize=None)
def command_sample():
    """reads tiled over the alleles of the planted ST every second base (100 bases, no error), every read written one to three times, the
    copies spread over the file"""
    db, idx = command_db()
    reads = []
    for a in rp.true_alleles(db, idx):
        seq = idx.sequence(a).encode().upper()
        reads += [(seq[s:s + 100], [40] * 100) for s in range(0, len(seq) - 100 + 1, 2)]
    rng = np.random.default_rng(8)
    out = [r for k, r in enumerate(reads) for _ in range(1 + k % 3)]
    order = rng.permutation(len(out))
    return [out[int(k)] for k in order]


def names_the_planted_st(said: str) -> bool:
    db, _ = command_db()
    return all(re.search(r"(?m)^\s+%s\s+%d\s" % (re.escape(g), int(a)), said) for (g, _), a in zip(db.loci["ecoli"], db.profiles["ecoli"][3]))


def test_cli_dedup_types_the_copies_as_the_rules_text(tmp_path, monkeypatch, capsys):
    reads = command_sample()
    raw = rp.fastq_text(reads)
    want_text, info = dedup_fastq(raw)
    assert info["duplicates"] > len(reads) // 3 and min(info["levels"][:3]) > 300
    for d, text in (("raw", raw), ("rule", want_text)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / "s.fastq").write_bytes(text)
    said_rule = run_type(monkeypatch, capsys, tmp_path / "rule", ["s.fastq"], tmp_path / "o_rule")
    said = run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--dedup"], tmp_path / "o_raw")
    want, got = rp.written(tmp_path / "o_rule"), rp.written(tmp_path / "o_raw")
    assert sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert got == want
    assert cli.read_dedup_line(info) in said and "duplicate removal" not in said_rule, said[-400:]
    assert "clash" not in said and names_the_planted_st(said), said
    quiet = run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--dedup", "--quiet"], tmp_path / "o_quiet")
    assert "duplicate removal" not in quiet and rp.written(tmp_path / "o_quiet") == want
    # mates: the pair is the unit
    n = len(reads) // 2
    pairs = [(reads[2 * (k % 700)], reads[2 * (k % 700) + 1]) if k % 3 == 0 else (reads[2 * k], reads[2 * k + 1]) for k in range(n)]
    inter = b"".join(rp.mate_header(f)(k) + b"\n" + r[0] + b"\n+\n" + bytes(v + 33 for v in r[1]) + b"\n" for k, p in enumerate(pairs) for f, r in enumerate(p))
    rule_inter, pinfo = dedup_fastq(inter, paired=True)
    assert pinfo["duplicates"] > 200 and pinfo["reads_removed"] == 2 * pinfo["duplicates"]
    for d, text in (("raw", inter), ("rule", rule_inter)):
        lines = text.split(b"\n")[:-1]
        recs = [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines), 4)]
        (tmp_path / d / "m_1.fastq").write_bytes(b"".join(recs[0::2]))
        (tmp_path / d / "m_2.fastq").write_bytes(b"".join(recs[1::2]))
    run_type(monkeypatch, capsys, tmp_path / "rule", ["m_1.fastq", "-2", "m_2.fastq", "--quiet"], tmp_path / "p_rule")
    said = run_type(monkeypatch, capsys, tmp_path / "raw", ["m_1.fastq", "-2", "m_2.fastq", "--dedup"], tmp_path / "p_raw")
    want, got = rp.written(tmp_path / "p_rule"), rp.written(tmp_path / "p_raw")
    assert got == want and sorted(want) == ["m_1.nfo", "m_1.out"] and len(want["m_1.nfo"]) > 0
    assert cli.read_dedup_line(pinfo, paired=True) in said and names_the_planted_st(said), said[-400:]
