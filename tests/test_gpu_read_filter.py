"""mlst_set_read_filter (csrc/read_filter.h): poly-G / poly-X tails trimmed and reads filtered on the device before the reads are packed.
The yardstick is that of test_gpu_read_adapters.py: the engine with the switch ON and the RAW text must leave what the same engine leaves
with every switch OFF and the text fastq.filter_fastq(...) writes -- the packed rows byte for byte (mlst_debug_last_packed), the typed
statistics, the counters -- through every entry that takes FASTQ text; then the whole chain, the exports, the refusals and the life
cycle, and the command.  poly_tail and read_fails are pinned by hand in test_read_filter_host.py.  The rule is the project's own
(modelled on fastp); nothing here claims fastp's bytes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import read_names_cases as rc
import test_gpu_read_dedup as dd
import test_gpu_read_overlap as ro
import test_gpu_read_prep as rp
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import dedup_fastq, filter_fastq, prep_fastq, read_stats, read_stats_equal, trim_adapters, trim_pair_overlap
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_read_adapters import cuts_inside_sequence_lines, row_width
from test_gpu_sam_all import assert_rule_bytes, export
from test_read_filter_host import KNOWN, qual_of, zero_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFF = {"poly": "", "poly_min": 10, "min_length": 0, "max_n": None, "complexity": 0, "mean_qual": 0}
ALL = {"poly": "ACGT", "poly_min": 10, "min_length": 40, "max_n": 2, "complexity": 30, "mean_qual": 20}
SETTINGS = [{"poly": "G"}, {"poly": "ACGT", "poly_min": 5}, {"min_length": 60}, {"max_n": 2}, {"complexity": 30}, {"mean_qual": 20}, ALL]
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320]
FAILED = ("failed_short", "failed_n", "failed_complexity", "failed_quality")


def ids(s):
    return " ".join("%s=%s" % kv for kv in s.items())


def full(setting):
    """what get_read_filter answers under the setting"""
    out = dict(OFF, **(setting or {}))
    if not out["poly"]:
        out["poly_min"] = 10
    return out


def rule_kw(setting) -> dict:
    """the arguments of fastq.filter_fastq for the arguments of Engine.set_read_filter"""
    s = full(setting)
    return {"letters": s["poly"].encode(), "poly_min": s["poly_min"], "min_length": s["min_length"], "max_n": s["max_n"], "complexity": s["complexity"], "mean_qual": s["mean_qual"]}


def add_infos(*infos):
    return cli._sum_filter_infos(list(infos))


def letters(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def planted_tail(rng, t: int, letter: int, mism: int) -> bytes:
    """t bases of one letter that begin on it, `mism` of the others replaced by another letter"""
    out = bytearray(b"ACGT"[letter:letter + 1] * t)
    for _ in range(mism if t > 1 else 0):
        out[int(rng.integers(1, t))] = b"ACGT"[(letter + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(out)


def crafted_reads(idx) -> list:
    """[(bases, [Phred])]: the reads by hand"""
    lb = rp.locus_bases
    out = [(seq, [max(c - 33, -1) for c in qual_of(seq, qual)]) for seq, qual, *_ in KNOWN]
    for k, n in enumerate(LENGTHS):                              # total lengths: plain, ending in twelve G, one tail
        t = min(n, 12)
        for b in (lb(idx, n, k), lb(idx, n - t, k + 20) + b"G" * t, b"T" * n):
            out.append((b, [40] * n))
    for o in range(34):                                          # a tail that starts at every offset from the 3' end: the 16-byte load edges
        out.append((lb(idx, 150 - o, o) + b"G" * o, [40] * 150))
        if o >= 3:
            out.append((lb(idx, 150 - o, o + 40) + b"CA" + b"C" * (o - 2), [40] * 150))      # ... and one that steps over a mismatch
    for n in (20, 150, 320):                                     # whole-read tails
        out += [(b"G" * n, [40] * n), (b"a" * n, [38] * n)]
    return out


@functools.lru_cache(maxsize=None)
def sample():
    """(index, [(bases, [Phred])]): test_gpu_read_prep's sample -- about 3,000 reads of 36 - 320 bases on and off the loci --, one read in
    three with a planted tail of 5 - 60 bases of one letter with 0 - 3 mismatches, some reads turned into dinucleotide repeats and runs of
    one letter, some N-rich, some of low quality, some cut short; the crafted reads spread through every group of 64"""
    idx, base = rp.sample()
    rng = np.random.default_rng(23)
    reads = []
    for k, (b, q) in enumerate(base):
        n = len(b)
        q = list(q)
        if k % 3 == 1:
            t = min(int(rng.integers(5, 61)), n)
            b = b[:n - t] + planted_tail(rng, t, 2 if k % 2 else (k // 6) % 4, int(rng.integers(0, 4)))
        elif k % 24 == 0:
            b = (b"AC" * n)[:n]                                  # a dinucleotide repeat: every neighbour differs, the measure lets it pass
        elif k % 24 == 3:
            b = b"".join(bytes([c]) * 9 for c in b[:n // 9 + 1])[:n]      # runs of nine: one neighbour in nine differs
        elif k % 24 == 6:
            b = bytearray(b)
            for at in rng.integers(0, n, size=int(rng.integers(1, 9))):
                b[int(at)] = ord("Nn.R"[int(at) % 4])
            b = bytes(b)
        elif k % 24 == 9:
            q = [int(v) for v in rng.integers(2, 30, size=n)]
        elif k % 24 == 12:
            m = int(rng.integers(20, 70))
            b, q = b[:m], q[:m]
        reads.append((b, q))
    crafted = crafted_reads(idx)
    total = len(reads) + len(crafted)
    for k, c in enumerate(crafted):      # evenly over the file: every group of 64 reads holds some
        reads.insert(k * total // len(crafted), c)
    return idx, reads


@functools.lru_cache(maxsize=None)
def raw_text(base: int = 33) -> bytes:
    return rp.fastq_text(sample()[1], base)


@functools.lru_cache(maxsize=None)
def expected(which: int):
    """(the text the engine must behave as if given, the counters) for SETTINGS[which]; computed once"""
    return filter_fastq(raw_text(), **rule_kw(SETTINGS[which]))


def moved(setting, info) -> list:
    """the counters the setting can move"""
    s = full(setting)
    out = []
    if s["poly"]:
        out += [info["tail_trimmed"], info["tail_bases"]] + [info["per_letter"]["ACGT".index(c)] for c in s["poly"]]
    out += [info[name] for name, on in zip(FAILED, (s["min_length"], s["max_n"] is not None, s["complexity"], s["mean_qual"])) if on]
    if s["min_length"] or s["max_n"] is not None or s["complexity"] or s["mean_qual"]:
        out.append(info["filtered_bases"])
    return out


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(sample()[0])
    yield e
    e.close()


def begin(eng, setting=None, prep=None, adapters=None, overlap=None, stats: bool = False, dedup: bool = False):
    eng.reset_sample()
    eng.set_read_prep(**(prep or {}))
    eng.set_read_adapters(**(adapters or {"adapters": None}))
    eng.set_read_stats(stats)
    eng.set_read_dedup(dedup)
    if overlap is None:
        eng.set_read_pair_overlap(False)
    else:
        eng.set_read_pair_overlap(True, **overlap)
    eng.set_read_filter(**(setting or {}))
    assert eng.get_read_filter() == full(setting)


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_filter_info()


# ------------------------------------------------------------------ the sample says what it is meant to
@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_the_sample_moves_every_counter(which):
    """from the rule alone, before the device is asked"""
    info = expected(which)[1]
    assert all(v > 20 for v in moved(SETTINGS[which], info)), (SETTINGS[which], info)
    s = full(SETTINGS[which])
    if s["poly"]:
        assert info["tail_emptied"] >= 1
    if which == len(SETTINGS) - 1:
        assert all(info[name] >= 1 for name in FAILED) and all(v > 20 for v in info["per_letter"])


# ------------------------------------------------------------------ one whole chunk
@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_one_whole_chunk_equals_the_filtered_text(eng, which):
    setting = SETTINGS[which]
    idx, reads = sample()
    raw = raw_text()
    want_text, want_info = expected(which)
    begin(eng, setting)
    assert eng.submit_fastq(raw) == len(reads)
    got = left_behind(eng)
    begin(eng)
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert want[2] == zero_info() and got[2] == want_info, (got[2], want_info)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2]
    assert int(got[1][0].n_hits.sum()) > 100 and len(got[1][1]) > 100, "the statistics are empty"
    # the guard: the raw text without the switch is another sample -- an engine that ignored the setting would pass otherwise
    begin(eng)
    eng.submit_fastq(raw)
    plain = eng.debug_last_packed()
    assert not np.array_equal(plain[2], lens)


def test_the_known_answers_on_the_device(eng):
    """the table of test_read_filter_host.py, the lengths by hand, without filter_fastq in between"""
    groups = {}
    for row in KNOWN:
        groups.setdefault(tuple(sorted(row[2].items())), []).append(row)
    assert len(groups) > 10
    for key, rows in groups.items():
        kw = dict(key)
        setting = {"poly": kw.get("letters", b"").decode(), "poly_min": kw.get("poly_min", 10), **{k: v for k, v in kw.items() if k not in ("letters", "poly_min")}}
        begin(eng, setting)
        assert eng.submit_fastq(b"".join(b"@r%d\n%s\n+\n%s\n" % (k, seq, qual_of(seq, qual)) for k, (seq, qual, *_) in enumerate(rows))) == len(rows)
        lens = eng.debug_last_packed()[2]
        assert [int(v) & 0x7FFF for v in lens] == [0 if why else left for *_, left, _, why in rows], kw
        cut = [(len(seq) - left, left, letter) for seq, _, _, left, letter, _ in rows if letter >= 0]
        assert eng.read_filter_info() == zero_info(
            tail_trimmed=len(cut), tail_bases=sum(c[0] for c in cut), per_letter=[sum(c[2] == x for c in cut) for x in range(4)], tail_emptied=sum(c[1] == 0 for c in cut),
            filtered_bases=sum(left for *_, left, _, why in rows if why), **{name: sum(why == k + 1 for *_, why in rows) for k, name in enumerate(FAILED)}), kw


# ------------------------------------------------------------------ a stream
def test_a_stream_cut_at_every_byte_of_a_sequence_and_a_quality_line(eng):
    idx, reads = sample()
    few = [(b[:90], q[:90]) for b, q in reads[400:520]]
    victim = 60
    few[victim] = (b"ACT" * 20 + b"G" * 30, [40] * 60 + [12] * 30)      # cut to 60, which pass at a mean of 40
    raw = rp.fastq_text(few)
    want_text, want_info = filter_fastq(raw, **rule_kw(ALL))
    begin(eng)
    assert eng.submit_fastq(want_text) == len(few)
    want_reads, want_typed = rp.reads_of(eng), typed(eng)
    assert want_reads[victim][0] & 0x7FFF == 60 and want_info["tail_trimmed"] > 20 and sum(want_info[k] for k in FAILED) > 5
    start = sum(len(rc.illumina(k)) + 2 * len(b) + 5 for k, (b, _) in enumerate(few[:victim])) + len(rc.illumina(victim)) + 1
    assert raw[start:start + 90] == few[victim][0] and raw[start + 93:start + 183] == bytes(v + 33 for v in few[victim][1])
    for cut in range(start - 1, start + 183 + 2):      # in front of the sequence line ... behind the quality line's LF
        begin(eng, ALL)
        n = eng.submit_fastq_stream(raw[:cut], final=False)
        got = rp.reads_of(eng) if n else []
        n += eng.submit_fastq_stream(raw[cut:], final=True)
        got += rp.reads_of(eng)
        assert n == len(few) and got == want_reads, cut
        assert eng.read_filter_info() == want_info, cut
    assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ mates
def mate_reads(n_pairs: int):
    """test_gpu_read_prep's mates of different lengths (every fifth first mate holds 20 bases, every third second mate 30: too short)"""
    return rp.mate_reads(sample()[1], n_pairs)


def test_mates_of_different_lengths_where_one_mate_is_filtered(eng):
    m1, m2 = mate_reads(600)
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    (p1, i1), (p2, i2) = filter_fastq(t1, **rule_kw(ALL)), filter_fastq(t2, **rule_kw(ALL))
    assert i1["failed_short"] >= 600 // 5 - 20 and i2["failed_short"] >= 600 // 3 - 40 and i1["tail_trimmed"] + i2["tail_trimmed"] > 100
    begin(eng)
    assert eng.submit_fastq_pair(p1, p2) == 1200
    want = left_behind(eng)
    begin(eng, ALL)
    assert eng.submit_fastq_pair(t1, t2) == 1200
    got = left_behind(eng)
    assert got[2] == add_infos(i1, i2) and want[2] == zero_info()
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2] & 0x7FFF
    assert ((lens[0::2] == 0) & (lens[1::2] > 0)).any() and ((lens[0::2] > 0) & (lens[1::2] == 0)).any() and len(got[1][1]) > 20      # the partner of a filtered mate stays
    # bgzip'd, one file ahead of the other
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    assert len(b1) > 12 and len(b2) > 45
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])),                           # file 1 nine blocks ahead: its records wait for their mates
             (b"".join(b1[9:10]), b"".join(b2[1:30])),                       # then file 2 overtakes
             (b"", b"".join(b2[30:40])),
             (b"".join(b1[10:]) + eof, b"".join(b2[40:]) + eof)]
    begin(eng, ALL)
    n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(ahead) - 1)) for k, (c1, c2) in enumerate(ahead))
    assert n == 1200 and eng.read_filter_info() == add_infos(i1, i2)
    assert_typed_equal(typed(eng), want[1])


# ------------------------------------------------------------------ bgzip
def test_bgzip_with_blocks_cut_inside_sequence_lines(eng):
    """with all four preparation flags on: Phred+64 text, the trims, then the filter (which reads the qualities at base 64)"""
    idx, reads = sample()
    few = reads[:1300]
    raw = rp.fastq_text(few, 64)
    sizes = (4099, 6007, 9001, 2503)
    assert cuts_inside_sequence_lines(raw, sizes) > 10
    blocks = bgzf_blocks(raw, sizes)
    prepared, pinfo = prep_fastq(raw, **rp.ALL4)
    want_text, want_info = filter_fastq(prepared, **rule_kw(ALL))
    assert want_info["tail_trimmed"] > 100 and want_info["failed_quality"] > 5 and want_info != filter_fastq(rp.fastq_text(few), **rule_kw(ALL))[1]
    begin(eng)
    eng.submit_fastq(want_text)
    want_typed = typed(eng)
    for per_call in (1, 7, len(blocks)):
        begin(eng, ALL, rp.ALL4)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == len(few), per_call
        assert eng.read_filter_info() == want_info and eng.read_prep_info() == pinfo, per_call
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ the row width
def test_rows_are_as_wide_as_the_filtered_text_when_every_longest_read_goes(eng):
    """every longest read (147 bases) loses a tail of 47 or fails the quality filter: the rows are those of 100 bases, through the text
    parse and through the pair-records parse (the longest length is fed by the last kernel that shortens alone)"""
    idx, _ = sample()
    reads = []
    for k in range(320):
        if k % 4 == 0:
            b = rp.locus_bases(idx, 99, k) + b"A" + b"G" * 47
        elif k % 4 == 1:
            b = rp.locus_bases(idx, 147, k)
        else:
            b = rp.locus_bases(idx, 36 + (k * 7) % 65, k) + b"T"
        reads.append((b, [5 if k % 4 == 1 else 40] * len(b)))
    setting = {"poly": "G", "mean_qual": 20}
    raw = rp.fastq_text(reads)
    want_text, want_info = filter_fastq(raw, **rule_kw(setting))
    assert row_width(raw) == (10, 152) and row_width(want_text) == (8, 104) and want_info["tail_trimmed"] >= 80 and want_info["failed_quality"] == 80
    begin(eng)
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert want[0][3:] == (8, 104)
    begin(eng, setting)
    assert eng.submit_fastq(raw) == len(reads)
    got = left_behind(eng)
    assert got[0][3:] == (8, 104), got[0][3:]
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert got[2] == want_info
    # mates, bgzip'd: the pair-records parse
    m1, m2 = reads[0::2], reads[1::2]
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    c1, c2 = (filter_fastq(t, **rule_kw(setting))[0] for t in (t1, t2))
    assert max(row_width(c1), row_width(c2)) == (8, 104) and row_width(t1) == (10, 152)
    begin(eng)
    assert eng.submit_fastq_pair(c1, c2) == len(reads)
    want = left_behind(eng)
    begin(eng, setting)
    assert eng.submit_fastq_bgzf_pair(b"".join(bgzf_blocks(t1, (7001,))), b"".join(bgzf_blocks(t2, (5003,))), final=True) == len(reads)
    got = left_behind(eng)
    assert len(got[0][2]) == len(reads) and got[0][3:] == (8, 104), got[0][3:]
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])


# ------------------------------------------------------------------ the whole chain
@functools.lru_cache(maxsize=None)
def chain_pairs():
    """test_gpu_read_overlap's chain sample; about every second first mate ends in a tail of G of high quality, about every seventh second
    mate is N-rich -- chosen by the mates' own letters, so that the copies the sample holds for --dedup stay copies"""
    idx, pairs = ro.chain_sample()
    out = []
    for (m1, q1), (m2, q2) in pairs:
        if sum(m1[6:14]) % 2 == 1:
            t = 12 + sum(m1[6:16]) % 40
            m1 = m1[:len(m1) - t] + b"G" * t
        if sum(m2[6:14]) % 7 == 2:
            m2 = bytes(ord("N") if i % 11 == 0 else c for i, c in enumerate(m2))
        out.append(((m1, q1), (m2, q2)))
    return idx, out


CHAIN = {"poly": "G", "min_length": 50, "max_n": 5, "complexity": 20, "mean_qual": 25}
ADAPT = {"adapters": [ro.ADAPTER], "min_overlap": 8, "error_permille": 100}


def test_the_whole_chain_prep_adapters_overlap_filter_dedup_statistics(eng):
    idx, pairs = chain_pairs()
    _, _, raw = ro.texts_of(pairs, 64)
    prepared, pinfo = prep_fastq(raw, **ro.PREP)
    cut, ainfo = trim_adapters(prepared, [ro.ADAPTER], 8, 100)
    over, oinfo = trim_pair_overlap(cut, trim5=6, **ro.DEFAULT)
    filt, finfo = filter_fastq(over, **rule_kw(CHAIN))
    want_text, dinfo = dedup_fastq(filt, paired=True)
    assert pinfo["shortened"] == 2 * len(pairs) and ainfo["trimmed"] > 50 and oinfo["trimmed_pairs"] > 50 and dinfo["duplicates"] > 30
    assert finfo["tail_trimmed"] > 50 and finfo["failed_n"] > 20 and finfo["failed_short"] > 5
    assert finfo != filter_fastq(cut, **rule_kw(CHAIN))[1] and dinfo != dedup_fastq(over, paired=True)[1]      # the order matters
    eng.set_profiling(1)
    try:
        begin(eng, CHAIN, ro.PREP, ADAPT, ro.DEFAULT, stats=True, dedup=True)
        eng.reset_kernel_time()
        assert eng.submit_fastq(raw, paired=True) == 2 * len(pairs)
        ms, launches = eng.kernel_time(23)
        assert launches == 1 and ms > 0 and eng.kernel_time(6)[0] >= ms      # k_rf_filter alone, inside 6
    finally:
        eng.set_profiling(0)
    got = left_behind(eng)
    stats = eng.read_stats()
    assert got[2] == finfo and eng.read_prep_info() == pinfo and eng.read_adapters_info() == ainfo and eng.read_pair_overlap_info() == oinfo
    assert dd.rule_part(eng.read_dedup_info()) == dinfo
    begin(eng)
    assert eng.submit_fastq(want_text, paired=True) == 2 * len(pairs)
    want = left_behind(eng)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert int(got[1][0].n_hits.sum()) > 100
    # the prepared stage of the read statistics shows the filtered reads (in front of the duplicates' removal), the raw stage the file's
    assert stats["prepared_counted"]
    for stage, text in (("raw", raw), ("prepared", filt)):
        rule = read_stats(text, phred64=(stage == "raw"), paired=True)
        assert all(read_stats_equal(stats[stage][side], rule[side]) for side in (0, 1)), stage
    # the filter alone beside the statistics: the prepared stage is counted all the same
    _, _, raw33 = ro.texts_of(pairs)
    filt33, info33 = filter_fastq(raw33, **rule_kw(CHAIN))
    begin(eng, CHAIN, stats=True)
    eng.submit_fastq(raw33, paired=True)
    stats = eng.read_stats()
    assert eng.read_filter_info() == info33 and stats["prepared_counted"] and eng.read_stats_info()["prepared_launches"] == 1
    rule = read_stats(filt33, paired=True)
    assert all(read_stats_equal(stats["prepared"][side], rule[side]) for side in (0, 1))
    assert not read_stats_equal(stats["prepared"][0], stats["raw"][0])


# ------------------------------------------------------------------ the exports
def test_export_bytes_are_those_of_the_filtered_text(eng, tmp_path):
    idx, reads = sample()
    raw = raw_text()
    want_text = expected(len(SETTINGS) - 1)[0]
    begin(eng)
    eng.submit_fastq(want_text)
    recs_off, body_off = export(eng, idx, tmp_path / "off.all.sam")
    md_off = b"".join(eng.export_sam_text(idx, md=True))
    begin(eng, ALL)
    eng.submit_fastq(raw)
    recs_on, body_on = export(eng, idx, tmp_path / "on.all.sam")
    assert body_on == body_off and len(recs_on) > 100
    assert_rule_bytes(idx, recs_on, body_on)
    assert b"".join(eng.export_sam_text(idx, md=True)) == md_off
    # once with the reads' own names: the header lines are not touched, so the names are the file's; a filtered read is in no export
    gone = {k for k, (a, b) in enumerate(zip(raw.split(b"\n")[1::4], want_text.split(b"\n")[1::4])) if a and not b}
    other = Engine(0, default_params())
    try:
        other.load_reference(idx)
        out = []
        for setting, text in ((ALL, raw), ({}, want_text)):
            other.reset_sample()
            other.set_read_filter(**setting)
            other.set_read_names(True)
            other.submit_fastq(text)
            out.append((b"".join(other.export_sam_text(idx, md=True)), other.read_names()))
        assert out[0] == out[1] and len(out[0][1]) > 100
        heads = rc.yardstick([raw])
        assert all(heads[ri].startswith(b"@" + nm) for ri, nm in out[0][1].items())
        assert len(gone) > 100 and not gone & set(out[0][1])
    finally:
        other.close()


# ------------------------------------------------------------------ refusals and life cycle
def test_every_other_way_of_adding_reads_is_refused():
    idx, reads = sample()
    text = rp.fastq_text(reads[:400])
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        assert eng.get_read_filter() == OFF and eng.read_filter_info() == zero_info()
        for bad, why in (({"poly": "G", "poly_min": 0}, "poly_min 0 is outside 1..320"), ({"poly": "G", "poly_min": 321}, "poly_min 321 is outside 1..320"),
                         ({"min_length": 321}, "min_length 321 is outside 0..320"), ({"complexity": 101}, "complexity_pct 101 is outside 0..100"),
                         ({"mean_qual": 94}, "mean_qual 94 is outside 0..93")):
            with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_filter: " + why):
                eng.set_read_filter(**bad)
        import ctypes as C
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_filter: poly_mask 16 is outside 0..15"):
            eng._check(eng.lib.mlst_set_read_filter(eng._h, (C.c_uint32 * 6)(16, 10, 0, 0xFFFFFFFF, 0, 0)), "mlst_set_read_filter")
        with pytest.raises(ValueError, match="only A, C, G and T"):
            eng.set_read_filter("GN")
        assert eng.get_read_filter() == OFF
        eng.set_read_filter("tgca", 320, 320, 0, 100, 93)                    # the limits are taken
        assert eng.get_read_filter() == {"poly": "ACGT", "poly_min": 320, "min_length": 320, "max_n": 0, "complexity": 100, "mean_qual": 93}
        assert eng.lib.mlst_set_read_filter(eng._h, None) == 0 and eng.get_read_filter() == OFF      # NULL: off
        eng.set_read_filter(min_length=5, poly_min=0)                       # (poly_min is looked at only with letters)
        assert eng.get_read_filter() == dict(OFF, min_length=5)
        eng.set_read_filter()                                               # all off: off
        assert eng.get_read_filter() == OFF
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
        # off: nothing is queued, nothing is allocated
        eng.set_profiling(1)
        eng.submit_fastq(text)
        assert eng.kernel_time(23) == (0.0, 0) and eng.read_filter_info() == zero_info()
        eng.reset_sample()
        eng.reset_kernel_time()
        for setting in ({"min_length": 60}, ALL):                           # every switch that turns the stage on closes the other entries
            eng.set_read_filter(**setting)
            for entry, call in calls.items():
                with pytest.raises(MlstError, match=r"\(-1\): %s: the read filter is on \(mlst_set_read_filter\) and only the FASTQ text and BGZF entries apply it" % entry):
                    call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text) == 400                                 # the handle stays usable
        ms, launches = eng.kernel_time(23)
        assert launches == 1 and ms > 0 and eng.kernel_time(6)[0] >= ms      # k_rf_filter alone, inside 6
        eng.set_profiling(0)
        want_info = filter_fastq(text, **rule_kw(ALL))[1]
        for change in (lambda: eng.set_read_filter(), lambda: eng.set_read_filter(**dict(ALL, poly_min=11))):
            with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_filter"):
                change()
        eng.set_read_filter(**dict(ALL, poly="tgca"))                       # (no change: accepted)
        assert eng.get_read_filter() == ALL and eng.read_filter_info() == want_info and want_info["tail_trimmed"] > 50
        eng.reset_sample()                                                   # keeps the setting, zeroes the counters
        assert eng.get_read_filter() == ALL and eng.read_filter_info() == zero_info()
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_filter()
        eng.reset_sample()
        eng.set_read_filter()
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_filter("G")
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_filter: mlst_set_read_tiling is on and a window is cut from the record as it stands"):
            eng.set_read_filter("G")
        eng.set_read_filter()                                                # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_filter(**ALL)
        eng.submit_fastq(text)
        eng.reset_sample()
        eng.set_read_filter()
        eng.submit_fastq(text)
        got = left_behind(eng)
        fresh = Engine(0, default_params())
        try:
            fresh.load_reference(idx)
            fresh.submit_fastq(text)
            want = left_behind(fresh)
        finally:
            fresh.close()
        assert got[2] == want[2] == zero_info()
        rp.assert_packed_equal(got[0], want[0])
        assert_typed_equal(got[1], want[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ the command
@functools.lru_cache(maxsize=None)
def command_sample():
    """(the reads with planted tails, the text the rule leaves of them, the counters): test_gpu_read_prep's planted sample, two reads in
    three followed by 10 - 40 G at Phred 38 (what a two-colour machine writes behind a short insert); every ninth read cut to 25 bases"""
    rng = np.random.default_rng(8)
    raw = []
    for k, (b, q) in enumerate(rp.planted_sample()):
        if k % 9 == 4:
            b, q = b[:25], list(q)[:25]
        elif k % 3:
            t = min(int(rng.integers(10, 41)), 320 - len(b))
            b, q = b + b"G" * t, list(q) + [38] * t
        raw.append((b, q))
    text, info = filter_fastq(rp.fastq_text(raw), letters=b"G", min_length=30)
    assert info["tail_trimmed"] >= 0.5 * len(raw) and info["failed_short"] >= len(raw) // 10
    return raw, text, info


FLAGS = ["--trim-poly-g", "--min-length", "30"]


def test_cli_trim_poly_g_types_planted_tails_as_the_filtered_text(tmp_path, monkeypatch, capsys):
    raw, clean_text, info = command_sample()
    for d, text in (("raw", rp.fastq_text(raw)), ("clean", clean_text)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / "s.fastq").write_bytes(text)
    rp.run_type(monkeypatch, capsys, tmp_path / "clean", ["s.fastq", "--quiet"], tmp_path / "o_clean")
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq"] + FLAGS, tmp_path / "o_raw")
    rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--quiet"], tmp_path / "o_noflag")
    want, got, wrong = rp.written(tmp_path / "o_clean"), rp.written(tmp_path / "o_raw"), rp.written(tmp_path / "o_noflag")
    assert sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert got == want
    assert cli.read_filter_line(info) in said, said[-400:]
    assert wrong != want                                                     # without the flag the tails are typed
    quiet = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--quiet"] + FLAGS, tmp_path / "o_quiet")
    assert "read filter" not in quiet and rp.written(tmp_path / "o_quiet") == want
    # between the adapter line and the overlap line
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--adapter", "illumina", "--trim-poly-x", "--poly-min", "12", "--max-n", "3", "--low-complexity", "30", "--min-mean-qual", "15"], tmp_path / "o_x")
    want_x = filter_fastq(trim_adapters(rp.fastq_text(raw), ["AGATCGGAAGAGC"])[0], letters=b"ACGT", poly_min=12, max_n=3, complexity=30, mean_qual=15)[1]
    assert cli.read_filter_line(want_x) in said and said.index("adapter removal:") < said.index("read filter:")


def test_cli_read_filter_on_a_folder_and_mates(tmp_path, monkeypatch, capsys):
    raw, _, _ = command_sample()
    raw_dir, cut_dir = tmp_path / "raw", tmp_path / "cut"
    for d in (raw_dir, cut_dir):
        os.makedirs(d / "in")
    n = len(raw) // 2
    m1, m2 = raw[0:2 * n:2], raw[1:2 * n:2]
    texts = {"m_1.fastq": rp.fastq_text(m1, header=rp.mate_header(0)), "m_2.fastq": rp.fastq_text(m2, header=rp.mate_header(1))}
    third = len(raw) // 3
    texts.update({"in/f%d.fastq" % k: rp.fastq_text(raw[k * third:(k + 1) * third] + raw[:400]) for k in range(3)})
    infos = {}
    for name, text in texts.items():
        (raw_dir / name).write_bytes(text)
        cut, infos[name] = filter_fastq(text, letters=b"G", min_length=30)
        (cut_dir / name).write_bytes(cut)
    for what, args, names in (("folder", ["in"], ["in/f0.fastq", "in/f1.fastq", "in/f2.fastq"]), ("mates", ["m_1.fastq", "-2", "m_2.fastq"], ["m_1.fastq", "m_2.fastq"])):
        said = rp.run_type(monkeypatch, capsys, raw_dir, args + FLAGS, tmp_path / ("o_raw_" + what))
        rp.run_type(monkeypatch, capsys, cut_dir, args + ["--quiet"], tmp_path / ("o_cut_" + what))
        got, want = rp.written(tmp_path / ("o_raw_" + what)), rp.written(tmp_path / ("o_cut_" + what))
        assert got == want and len(want) == 2 * (3 if what == "folder" else 1) and all(len(v) > 0 for v in want.values()), what
        total = add_infos(*(infos[f] for f in names))
        assert cli.read_filter_line(total) in said and total["tail_trimmed"] > 500, (what, said[-400:])


def test_cli_two_ranks_equal_one_process(tmp_path):
    """in the manner of test_gpu_multirank.py: two ranks on the one GPU, gloo collectives"""
    raw, clean_text, info = command_sample()
    db, _ = fx.ecoli_small(40, 5)
    (tmp_path / "s.fastq").write_bytes(rp.fastq_text(raw))
    os.makedirs(tmp_path / "p")
    (tmp_path / "p" / "s.fastq").write_bytes(clean_text)
    env = dict(os.environ, MLST_FASTQ_CHUNK=str(256 << 10), MLST_ONE_GPU="1", MLST_BACKEND="gloo")      # several chunks per rank
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    tail = ["-d", db.path, "--min_accuracy", "0", "--nloci", "0", "--log"]
    outs = []
    for cwd, args in ((tmp_path, FLAGS + ["--gpus", "2", "-o", str(tmp_path / "two")]), (tmp_path / "p", ["--quiet", "-o", str(tmp_path / "one")])):
        r = subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "type", "s.fastq"] + tail + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    got, want = rp.written(tmp_path / "two"), rp.written(tmp_path / "one")
    assert got == want and sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert [l for l in outs[0].splitlines() if l.startswith("read filter:")] == [cli.read_filter_line(info)]
