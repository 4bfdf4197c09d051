"""mlst_set_read_window (csrc/read_window.h): sliding-window quality cuts on the device before the reads are packed.  The yardstick is
that of test_gpu_read_filter.py: the engine with the switch ON and the RAW text must leave what the same engine leaves with every switch
OFF and the text fastq.cut_windows(...) writes -- the packed rows byte for byte (mlst_debug_last_packed), the typed statistics, the
counters -- through every entry that takes FASTQ text; then the whole chain, the exports, the refusals and the life cycle, and the
command.  window_cut is pinned by hand in test_read_window_host.py.  The rule is the project's own (modelled on fastp's cut_front /
cut_right / cut_tail); nothing here claims fastp's or Trimmomatic's bytes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import read_names_cases as rc
import test_gpu_read_dedup as dd
import test_gpu_read_overlap as ro
import test_gpu_read_prep as rp
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import cut_windows, dedup_fastq, filter_fastq, prep_fastq, read_stats, read_stats_equal, trim_adapters, trim_pair_overlap
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_read_adapters import cuts_inside_sequence_lines, row_width
from test_gpu_sam_all import assert_rule_bytes, export
from test_read_window_host import KNOWN, bases, info_of, zero_info

pytestmark = pytest.mark.gpu

OFF = {"front": None, "right": None, "tail": None}
ALL = {"front": (2, 20), "right": (33, 25), "tail": (15, 30)}
RECIPE = {"front": (1, 3), "right": (4, 15), "tail": (1, 3)}      # LEADING:3 SLIDINGWINDOW:4:15 TRAILING:3
WIDTHS = (1, 2, 4, 15, 16, 17, 33, 320)      # the lagging load at every alignment against the leading one, and W > n
SETTINGS = ([{op: (w, q)} for op, q in (("front", 20), ("right", 20), ("tail", 25)) for w in WIDTHS] +      # (the walk down has its own lagging load)
            [RECIPE, ALL, {"front": (320, 20), "right": (16, 22), "tail": (64, 33)}])
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320]
OPS = ("front", "right", "tail")


def ids(s):
    return " ".join("%s=%d,%d" % (k, *v) for k, v in s.items())


def full(setting):
    """what get_read_window answers under the setting"""
    return {k: list(v) if v else None for k, v in dict(OFF, **(setting or {})).items()}


def add_infos(*infos):
    return {k: sum(i[k] for i in infos) for k in infos[0]}


def crafted_reads(idx) -> list:
    """[(bases, [Phred])]: the reads by hand"""
    lb = rp.locus_bases
    out = [(lb(idx, len(q), k), list(q)) for k, (q, *_) in enumerate(KNOWN)]
    for k, n in enumerate(LENGTHS):      # every length: all good, all bad, the last window alone fails (W 4), the first alone
        m = min(n, 3)
        for q in ([40] * n, [2] * n, [40] * (n - m) + [2] * m, [2] * m + [40] * (n - m)):
            out.append((lb(idx, n, k + len(out)), q))
    for o in range(34):                  # one bad window that starts at every offset from the 5' end and from the 3' end: the 16-byte load edges
        for n, w in ((150, 4), (97, 4), (150, 40)):
            q = [40] * n
            q[o:o + w] = [2] * w
            out.append((lb(idx, n, o + len(out)), q))
            q = [40] * n
            q[n - o - w:n - o] = [2] * w
            out.append((lb(idx, n, o + len(out)), q))
    return out


@functools.lru_cache(maxsize=None)
def sample():
    """(index, [(bases, [Phred])]): test_gpu_read_prep's sample -- about 3,000 reads of 36 - 320 bases on and off the loci, one in three
    with a decayed tail --, the qualities reshaped: one read in four with a dip of 3 - 12 bad bases in its middle, one in four with a bad
    5' end of 1 - 20 bases, one in eight with a bad 3' end of 1 - 30 bases, one in eight with one or two bad last bases (which a window of four tolerates), one in fifty bad all over; the crafted reads spread through every group of 64"""
    idx, base = rp.sample()
    rng = np.random.default_rng(24)
    reads = []
    for k, (b, q) in enumerate(base):
        n, q = len(b), list(q)
        if n >= 36:
            if k % 4 == 0:
                a, L = int(rng.integers(10, n - 12)), int(rng.integers(3, 13))
                q[a:a + L] = [int(v) for v in rng.integers(2, 11, size=L)]
            elif k % 4 == 1:
                t = int(rng.integers(1, 21))
                q[:t] = [int(v) for v in rng.integers(2, 11, size=t)]
            elif k % 8 == 2:
                t = int(rng.integers(1, 31))
                q[n - t:] = [int(v) for v in rng.integers(2, 11, size=t)]
            elif k % 8 == 6:
                t = int(rng.integers(1, 3))
                q[n - t:] = [2] * t
            if k % 50 == 7:
                q = [int(v) for v in rng.integers(2, 12, size=n)]
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
    return cut_windows(raw_text(), **SETTINGS[which])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(sample()[0])
    yield e
    e.close()


def begin(eng, setting=None, prep=None, adapters=None, overlap=None, filt=None, stats: bool = False, dedup: bool = False):
    eng.reset_sample()
    eng.set_read_window()      # (off first: a front cut and the mates' overlap do not meet on the way)
    eng.set_read_prep(**(prep or {}))
    eng.set_read_adapters(**(adapters or {"adapters": None}))
    eng.set_read_stats(stats)
    eng.set_read_dedup(dedup)
    if overlap is None:
        eng.set_read_pair_overlap(False)
    else:
        eng.set_read_pair_overlap(True, **overlap)
    eng.set_read_filter(**(filt or {}))
    eng.set_read_window(**(setting or {}))
    assert eng.get_read_window() == full(setting)


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_window_info()


# ------------------------------------------------------------------ the sample says what it is meant to
def test_the_sample_holds_what_it_says():
    """from the text alone: every length, quality lines that start at every residue mod 16, crafted reads in every group of 64"""
    idx, reads = sample()
    assert {len(b) for b, _ in reads} >= set(LENGTHS) and 3000 < len(reads) < 3700
    text, at, starts = raw_text(), 0, set()
    for k, (b, _) in enumerate(reads):
        at += len(rc.illumina(k)) + 1 + len(b) + 3
        assert text[at - 3:at] == b"\n+\n"
        starts.add(at % 16)
        at += len(b) + 1
    assert at == len(text) and starts == set(range(16))
    crafted = {(b, tuple(q)) for b, q in crafted_reads(idx)}
    assert all(any((b, tuple(q)) in crafted for b, q in reads[g:g + 64]) for g in range(0, len(reads) - 63, 64))


@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_the_sample_moves_every_counter(which):
    """from the rule alone, before the device is asked"""
    info = expected(which)[1]
    moved = [info["shortened"]] + [info[op + x] for op in OPS if op in SETTINGS[which] for x in ("_reads", "_bases")]
    assert all(v > 20 for v in moved) and info["emptied"] >= 1, (SETTINGS[which], info)


# ------------------------------------------------------------------ one whole chunk
@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_one_whole_chunk_equals_the_cut_text(eng, which):
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
    assert int(got[1][0].n_hits.sum()) > 100 and len(got[1][1]) > 100, "the statistics are empty"
    # the guard: the raw text without the switch is another sample -- an engine that ignored the setting would pass otherwise
    begin(eng)
    eng.submit_fastq(raw)
    assert not np.array_equal(eng.debug_last_packed()[2], got[0][2])


def test_the_known_answers_on_the_device(eng):
    """the table of test_read_window_host.py, lengths and bases by hand, without cut_windows in between"""
    groups = {}
    for row in KNOWN:
        groups.setdefault(tuple(row[1:4]), []).append(row)
    assert len(groups) >= 8
    for (front, right, tail), rows in groups.items():
        begin(eng, {k: v for k, v in zip(OPS, (front, right, tail)) if v})
        assert eng.submit_fastq(b"".join(b"@r%d\n%s\n+\n%s\n" % (k, bases(len(q)), bytes(v + 33 for v in q)) for k, (q, *_) in enumerate(rows))) == len(rows)
        got = [(entry & 0x7FFF, b) for entry, b, _ in rp.reads_of(eng)]
        assert got == [(e - f, bases(len(q))[f:e]) for q, _, _, _, f, _, e in rows], (front, right, tail)
        assert eng.read_window_info() == info_of(rows), (front, right, tail)


def test_phred64_text_with_no_other_preparation(eng):
    """the Phred base alone starts no k_rp_qtrim: the window kernel takes the base as a value"""
    idx, reads = sample()
    want_text, want_info = cut_windows(raw_text(64), phred64=True, **ALL)
    assert want_info == expected(SETTINGS.index(ALL))[1] and want_text == expected(SETTINGS.index(ALL))[0]
    begin(eng)
    eng.submit_fastq(want_text)
    want = left_behind(eng)
    begin(eng, ALL, {"phred64": True})
    assert eng.submit_fastq(raw_text(64)) == len(reads)
    got = left_behind(eng)
    assert got[2] == want_info and eng.read_prep_info() == rp.ZERO
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])


# ------------------------------------------------------------------ a stream
def test_a_stream_cut_at_every_byte_of_a_sequence_and_a_quality_line(eng):
    idx, reads = sample()
    few = [(b[:90], q[:90]) for b, q in reads[400:520]]
    victim = 60
    few[victim] = (few[victim][0] if len(few[victim][0]) == 90 else rp.locus_bases(idx, 90, 5), [2] * 5 + [40] * 45 + [2] * 40)
    raw = rp.fastq_text(few)
    want_text, want_info = cut_windows(raw, **ALL)
    begin(eng)
    assert eng.submit_fastq(want_text) == len(few)
    want_reads, want_typed = rp.reads_of(eng), typed(eng)
    # front: 4, then 42 at s = 4; right: a window of 33 needs 20 values of 40 (38 x + 66 >= 825), the one at s = 31 holds 19, and they stay
    assert want_reads[victim][0] & 0x7FFF == 46 and all(want_info[op + "_reads"] > 5 for op in OPS)
    b = few[victim][0]
    start = sum(len(rc.illumina(k)) + 2 * len(b_) + 5 for k, (b_, _) in enumerate(few[:victim])) + len(rc.illumina(victim)) + 1
    assert raw[start:start + 90] == b and raw[start + 93:start + 183] == bytes(v + 33 for v in few[victim][1])
    for cut in range(start - 1, start + 183 + 2):      # in front of the sequence line ... behind the quality line's LF
        begin(eng, ALL)
        n = eng.submit_fastq_stream(raw[:cut], final=False)
        got = rp.reads_of(eng) if n else []
        n += eng.submit_fastq_stream(raw[cut:], final=True)
        got += rp.reads_of(eng)
        assert n == len(few) and got == want_reads, cut
        assert eng.read_window_info() == want_info, cut
    assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ mates
def test_mates_of_different_lengths_each_cut_on_its_own(eng):
    m1, m2 = rp.mate_reads(sample()[1], 600)
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    (p1, i1), (p2, i2) = cut_windows(t1, **ALL), cut_windows(t2, **ALL)
    assert all(i[op + "_reads"] > 20 for i in (i1, i2) for op in OPS) and i1 != i2
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
    assert ((lens[0::2] == 0) & (lens[1::2] > 0)).any() and ((lens[0::2] > 0) & (lens[1::2] == 0)).any() and len(got[1][1]) > 20      # the partner of an emptied mate stays
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
    assert n == 1200 and eng.read_window_info() == add_infos(i1, i2)
    assert_typed_equal(typed(eng), want[1])


# ------------------------------------------------------------------ bgzip
def test_bgzip_with_blocks_cut_inside_sequence_lines(eng):
    """with all four preparation flags on: Phred+64 text, the trims (which move the reads' starts first), then the windows at base 64"""
    idx, reads = sample()
    few = reads[:1300]
    raw = rp.fastq_text(few, 64)
    sizes = (4099, 6007, 9001, 2503)
    assert cuts_inside_sequence_lines(raw, sizes) > 10
    blocks = bgzf_blocks(raw, sizes)
    prepared, pinfo = prep_fastq(raw, **rp.ALL4)
    want_text, want_info = cut_windows(prepared, **ALL)
    assert all(want_info[op + "_reads"] > 20 for op in OPS) and want_info != cut_windows(rp.fastq_text(few), **ALL)[1]
    begin(eng)
    eng.submit_fastq(want_text)
    want_typed = typed(eng)
    for per_call in (1, 7, len(blocks)):
        begin(eng, ALL, rp.ALL4)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == len(few), per_call
        assert eng.read_window_info() == want_info and eng.read_prep_info() == pinfo, per_call
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ the row width
def test_rows_are_as_wide_as_the_cut_text_when_every_longest_read_is_shortened(eng):
    """every longest read (147 bases) is cut to 100 at a dip or is bad all over: the rows are those of 100 bases, through the text parse
    and through the pair-records parse (the longest length is fed by the last kernel that shortens alone)"""
    idx, _ = sample()
    reads = []
    for k in range(320):
        if k % 4 == 0:
            b, q = rp.locus_bases(idx, 147, k), [40] * 100 + [2] * 4 + [40] * 43      # 122, 84, then 46 at s = 99: one base of that window stays
        elif k % 4 == 1:
            b, q = rp.locus_bases(idx, 147, k), [5] * 147
        else:
            b = rp.locus_bases(idx, 36 + (k * 7) % 65, k)
            q = [40] * len(b)
        reads.append((b, q))
    setting = {"right": (4, 20)}
    raw = rp.fastq_text(reads)
    want_text, want_info = cut_windows(raw, **setting)
    assert row_width(raw) == (10, 152) and row_width(want_text) == (8, 104) and want_info == zero_info(shortened=160, right_reads=160, right_bases=80 * 47 + 80 * 147, emptied=80)
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
    c1, c2 = (cut_windows(t, **setting)[0] for t in (t1, t2))
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
    """test_gpu_read_overlap's chain sample; about every third first mate has a dip of six bad bases in its middle, about every fourth
    second mate two bad bases in front of its last one, about every second first mate a tail of G -- chosen by the mates' own letters, so that the
    copies the sample holds for --dedup stay copies"""
    idx, pairs = ro.chain_sample()
    out = []
    for (m1, q1), (m2, q2) in pairs:
        q1, q2 = list(q1), list(q2)
        if sum(m1[6:14]) % 3 == 0:
            a = 50 + sum(m1[6:16]) % 60
            q1[a:a + 6] = [3] * 6
        if sum(m2[6:14]) % 4 == 1 and q2[-1] >= 30:
            q2[-3:] = [5, 5, 40]      # (--trim-qual leaves at the good last base; a window of two does not)
        if sum(m1[6:14]) % 2 == 1:
            t = 12 + sum(m1[6:16]) % 40
            m1 = m1[:len(m1) - t] + b"G" * t
        out.append(((m1, q1), (m2, q2)))
    return idx, out


CHAIN = {"right": (4, 20), "tail": (2, 25)}      # (no front cut: it does not combine with the mates' overlap)
FILT = {"poly": "G", "min_length": 50, "max_n": 5}
FILT_RULE = {"letters": b"G", "min_length": 50, "max_n": 5}
ADAPT = {"adapters": [ro.ADAPTER], "min_overlap": 8, "error_permille": 100}


@functools.lru_cache(maxsize=None)
def chain_rule():
    """the composition the engine must equal, every step computed once: (raw, [(text, counters)] of prep, windows, adapters, overlap, filter, dedup)"""
    idx, pairs = chain_pairs()
    _, _, raw = ro.texts_of(pairs, 64)
    steps = [prep_fastq(raw, **ro.PREP)]
    steps.append(cut_windows(steps[-1][0], **CHAIN))
    steps.append(trim_adapters(steps[-1][0], [ro.ADAPTER], 8, 100))
    steps.append(trim_pair_overlap(steps[-1][0], trim5=6, **ro.DEFAULT))
    steps.append(filter_fastq(steps[-1][0], **FILT_RULE))
    steps.append(dedup_fastq(steps[-1][0], paired=True))
    return raw, steps


def test_the_chain_sample_moves_every_stage():
    """from the rules alone"""
    idx, pairs = chain_pairs()
    (_, pinfo), (cut, winfo), (_, ainfo), (_, oinfo), (_, finfo), (_, dinfo) = chain_rule()[1]
    assert pinfo["shortened"] == 2 * len(pairs) and winfo["right_reads"] > 50 and winfo["tail_reads"] > 20 and ainfo["trimmed"] > 50
    assert oinfo["trimmed_pairs"] > 50 and finfo["tail_trimmed"] > 50 and finfo["failed_short"] > 5 and dinfo["duplicates"] > 30
    assert ainfo != trim_adapters(chain_rule()[1][0][0], [ro.ADAPTER], 8, 100)[1]      # the order matters: the windows stand in front of the adapters


def test_the_whole_chain_prep_windows_adapters_overlap_filter_dedup_statistics(eng):
    idx, pairs = chain_pairs()
    raw, steps = chain_rule()
    (_, pinfo), (_, winfo), (_, ainfo), (_, oinfo), (filt, finfo), (want_text, dinfo) = steps
    eng.set_profiling(1)
    try:
        begin(eng, CHAIN, ro.PREP, ADAPT, ro.DEFAULT, FILT, stats=True, dedup=True)
        eng.reset_kernel_time()
        assert eng.submit_fastq(raw, paired=True) == 2 * len(pairs)
        ms, launches = eng.kernel_time(24)
        assert launches == 1 and ms > 0 and eng.kernel_time(6)[0] >= ms      # k_rw_cut alone, inside 6
    finally:
        eng.set_profiling(0)
    got = left_behind(eng)
    stats = eng.read_stats()
    assert got[2] == winfo and eng.read_prep_info() == pinfo and eng.read_adapters_info() == ainfo and eng.read_pair_overlap_info() == oinfo
    assert eng.read_filter_info() == finfo and dd.rule_part(eng.read_dedup_info()) == dinfo
    begin(eng)
    assert eng.submit_fastq(want_text, paired=True) == 2 * len(pairs)
    want = left_behind(eng)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert int(got[1][0].n_hits.sum()) > 100
    # the prepared stage of the read statistics shows the reads in front of the duplicates' removal, the raw stage the file's
    assert stats["prepared_counted"]
    for stage, text in (("raw", raw), ("prepared", filt)):
        rule = read_stats(text, phred64=(stage == "raw"), paired=True)
        assert all(read_stats_equal(stats[stage][side], rule[side]) for side in (0, 1)), stage
    # the windows alone beside the statistics: the prepared stage is counted all the same
    _, _, raw33 = ro.texts_of(pairs)
    cut33, info33 = cut_windows(raw33, **CHAIN)
    begin(eng, CHAIN, stats=True)
    eng.submit_fastq(raw33, paired=True)
    stats = eng.read_stats()
    assert eng.read_window_info() == info33 and stats["prepared_counted"] and eng.read_stats_info()["prepared_launches"] == 1
    rule = read_stats(cut33, paired=True)
    assert all(read_stats_equal(stats["prepared"][side], rule[side]) for side in (0, 1))
    assert not read_stats_equal(stats["prepared"][0], stats["raw"][0])


# ------------------------------------------------------------------ the exports
def test_export_bytes_are_those_of_the_cut_text(eng, tmp_path):
    idx, reads = sample()
    raw = raw_text()
    want_text = expected(SETTINGS.index(ALL))[0]
    begin(eng)
    eng.submit_fastq(want_text)
    recs_off, body_off = export(eng, idx, tmp_path / "off.all.sam")
    md_off = b"".join(eng.export_sam_text(idx, md=True))
    reads_off = b"".join(eng.export_reads_text())
    begin(eng, ALL)
    eng.submit_fastq(raw)
    recs_on, body_on = export(eng, idx, tmp_path / "on.all.sam")
    assert body_on == body_off and len(recs_on) > 100
    assert_rule_bytes(idx, recs_on, body_on)
    assert b"".join(eng.export_sam_text(idx, md=True)) == md_off
    assert b"".join(eng.export_reads_text()) == reads_off and reads_off.count(b"\n") > 400      # --write-reads: the cut SEQ / QUAL
    # once with the reads' own names: the header lines are not touched, so the names are the file's and survive a front cut
    fronted = {k for k, (a, b) in enumerate(zip(raw.split(b"\n")[1::4], want_text.split(b"\n")[1::4])) if b and not a.startswith(b)}
    other = Engine(0, default_params())
    try:
        other.load_reference(idx)
        out = []
        for setting, text in ((ALL, raw), ({}, want_text)):
            other.reset_sample()
            other.set_read_window(**setting)
            other.set_read_names(True)
            other.submit_fastq(text)
            out.append((b"".join(other.export_sam_text(idx, md=True)), other.read_names()))
        assert out[0] == out[1] and len(out[0][1]) > 100
        heads = rc.yardstick([raw])
        assert all(heads[ri].startswith(b"@" + nm) for ri, nm in out[0][1].items())
        assert len(fronted) > 100 and len(fronted & set(out[0][1])) > 10
    finally:
        other.close()


# ------------------------------------------------------------------ refusals and life cycle
def raw_set(eng, *six):
    eng._check(eng.lib.mlst_set_read_window(eng._h, (C.c_uint32 * 6)(*six)), "mlst_set_read_window")


def test_every_other_way_of_adding_reads_is_refused():
    idx, reads = sample()
    text = rp.fastq_text(reads[:400])
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        assert eng.get_read_window() == OFF and eng.read_window_info() == zero_info()
        for six, why in (((321, 20, 0, 0, 0, 0), "front_w 321 is outside 0..320"), ((4, 0, 0, 0, 0, 0), "front_q 0 is outside 1..93"), ((0, 0, 4, 94, 0, 0), "right_q 94 is outside 1..93"),
                         ((0, 0, 0, 0, 400, 20), "tail_w 400 is outside 0..320"), ((1, 1, 1, 1, 1, 0), "tail_q 0 is outside 1..93")):
            with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_window: " + why):
                raw_set(eng, *six)
        with pytest.raises(ValueError, match="set_read_window: front window 0 is outside 1..320"):
            eng.set_read_window(front=(0, 20))
        assert eng.get_read_window() == OFF
        eng.set_read_window((320, 93), (1, 1), (320, 1))                     # the limits are taken
        assert eng.get_read_window() == {"front": [320, 93], "right": [1, 1], "tail": [320, 1]}
        assert eng.lib.mlst_set_read_window(eng._h, None) == 0 and eng.get_read_window() == OFF      # NULL: off
        raw_set(eng, 0, 99, 0, 0, 0, 7)                                      # (w = 0: the operation is off and its q is not looked at)
        assert eng.get_read_window() == OFF
        eng.set_read_window(tail=(4, 20))
        assert eng.get_read_window() == dict(OFF, tail=[4, 20])
        eng.set_read_window()                                                # all off: off
        assert eng.get_read_window() == OFF
        # a front cut and the mates' overlap, in both orders; right and tail go with it
        sentence = r"a front cut \(mlst_set_read_window, front_w != 0\) and mate overlap trimming \(mlst_set_read_pair_overlap\) do not combine.*true insert bases"
        eng.set_read_pair_overlap(True)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_window: " + sentence):
            eng.set_read_window(front=(4, 20))
        eng.set_read_window(right=(4, 20), tail=(1, 3))
        assert eng.get_read_window() == {"front": None, "right": [4, 20], "tail": [1, 3]} and eng.get_read_pair_overlap()["on"]
        eng.set_read_pair_overlap(False)
        eng.set_read_window(**ALL)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_pair_overlap: " + sentence):
            eng.set_read_pair_overlap(True)
        assert not eng.get_read_pair_overlap()["on"] and eng.get_read_window() == full(ALL)
        eng.set_read_pair_overlap(False)                                     # (off beside a front cut: nothing to refuse)
        eng.set_read_window()
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
        assert eng.kernel_time(24) == (0.0, 0) and eng.read_window_info() == zero_info()
        eng.reset_sample()
        eng.reset_kernel_time()
        for setting in ({"front": (1, 3)}, {"right": (4, 15)}, {"tail": (1, 3)}, ALL):      # every operation turns the stage on and closes the other entries
            eng.set_read_window(**setting)
            for entry, call in calls.items():
                with pytest.raises(MlstError, match=r"\(-1\): %s: the quality windows are on \(mlst_set_read_window\) and only the FASTQ text and BGZF entries apply them" % entry):
                    call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text) == 400                                 # the handle stays usable
        ms, launches = eng.kernel_time(24)
        assert launches == 1 and ms > 0 and eng.kernel_time(6)[0] >= ms      # k_rw_cut alone, inside 6
        eng.set_profiling(0)
        want_info = cut_windows(text, **ALL)[1]
        for change in (lambda: eng.set_read_window(), lambda: eng.set_read_window(**dict(ALL, tail=(15, 31)))):
            with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_window"):
                change()
        eng.set_read_window(**{k: list(v) for k, v in ALL.items()})          # (no change: accepted)
        assert eng.get_read_window() == full(ALL) and eng.read_window_info() == want_info and want_info["shortened"] > 50
        eng.reset_sample()                                                   # keeps the setting, zeroes the counters
        assert eng.get_read_window() == full(ALL) and eng.read_window_info() == zero_info()
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_window()
        eng.reset_sample()
        eng.set_read_window()
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_window(right=(4, 20))
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_window: mlst_set_read_tiling is on and a window is cut from the record as it stands"):
            eng.set_read_window(right=(4, 20))
        eng.set_read_window()                                                # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_window(**ALL)
        eng.submit_fastq(text)
        eng.reset_sample()
        eng.set_read_window()
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
    """(the reads, the text the rule leaves of them, the counters): test_gpu_read_prep's planted sample with its planted letters at full
    quality behind four bad bases -- a window cut drops them, without it they out-vote the right letter --, every fifth read with a bad
    5' end of 1 - 9 bases and every seventh with a bad 3' end of 1 - 3"""
    idx, reads = rp.sample()
    rng = np.random.default_rng(9)
    raw = []
    for k, (b, q) in enumerate(rp.planted_sample()):
        q = list(q)
        low = [i for i, v in enumerate(q) if v == 2]
        if len(q) == 100 and low and low[0] >= 10:
            for i in low:
                q[i] = 40
            q[low[0] - 6:low[0] - 2] = [2] * 4
        if k % 5 == 0:
            t = int(rng.integers(1, 10))
            q[:t] = [2] * t
        if k % 7 == 0:
            t = int(rng.integers(1, 4))
            q[len(q) - t:] = [2] * t
        raw.append((b, q))
    text, info = cut_windows(rp.fastq_text(raw), **RECIPE)
    assert all(info[op + "_reads"] > 100 for op in OPS), info
    return raw, text, info


FLAGS = ["--cut-front", "1,3", "--cut-tail", "1,3", "--cut-right", "4,15"]


def test_cli_quality_windows_type_a_file_as_the_cut_text(tmp_path, monkeypatch, capsys):
    raw, clean_text, info = command_sample()
    for d, text in (("raw", rp.fastq_text(raw)), ("clean", clean_text)):
        os.makedirs(tmp_path / d / "in")
        (tmp_path / d / "s.fastq").write_bytes(text)
        (tmp_path / d / "in" / "f0.fastq").write_bytes(text[:text.index(b"\n@", 4000) + 1])
    rp.run_type(monkeypatch, capsys, tmp_path / "clean", ["s.fastq", "--quiet"], tmp_path / "o_clean")
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq"] + FLAGS, tmp_path / "o_raw")
    rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--quiet"], tmp_path / "o_noflag")
    want, got, wrong = rp.written(tmp_path / "o_clean"), rp.written(tmp_path / "o_raw"), rp.written(tmp_path / "o_noflag")
    assert sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert got == want
    assert cli.read_window_line(info) in said, said[-400:]
    assert wrong != want                                                     # without the flags the planted letters are typed
    quiet = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--quiet"] + FLAGS, tmp_path / "o_quiet")
    assert "quality windows" not in quiet and rp.written(tmp_path / "o_quiet") == want
    # between the preparation's line and the adapter line
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--trim3", "1", "--adapter", "illumina", "--min-length", "36"] + FLAGS, tmp_path / "o_x")
    want_x = cut_windows(prep_fastq(rp.fastq_text(raw), trim3=1)[0], **RECIPE)[1]
    assert cli.read_window_line(want_x) in said and said.index("read preparation:") < said.index("quality windows:") < said.index("adapter removal:") < said.index("read filter:")
    # a folder is refused, with the reason, before anything is written
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["in", "s.fastq"] + FLAGS, tmp_path / "o_many", rc_want=1)
    assert "quality windows (--cut-front, --cut-right, --cut-tail): several samples or a folder are typed without them" in said and not os.path.exists(tmp_path / "o_many")


def test_cli_quality_windows_on_mates(tmp_path, monkeypatch, capsys):
    raw, _, _ = command_sample()
    raw_dir, cut_dir = tmp_path / "raw", tmp_path / "cut"
    n = len(raw) // 2
    m1, m2 = raw[0:2 * n:2], raw[1:2 * n:2]
    texts = {"m_1.fastq": rp.fastq_text(m1, header=rp.mate_header(0)), "m_2.fastq": rp.fastq_text(m2, header=rp.mate_header(1))}
    infos = {}
    for d in (raw_dir, cut_dir):
        os.makedirs(d)
    for name, text in texts.items():
        (raw_dir / name).write_bytes(text)
        cut, infos[name] = cut_windows(text, **RECIPE)
        (cut_dir / name).write_bytes(cut)
    args = ["m_1.fastq", "-2", "m_2.fastq"]
    said = rp.run_type(monkeypatch, capsys, raw_dir, args + FLAGS, tmp_path / "o_raw")
    rp.run_type(monkeypatch, capsys, cut_dir, args + ["--quiet"], tmp_path / "o_cut")
    got, want = rp.written(tmp_path / "o_raw"), rp.written(tmp_path / "o_cut")
    assert got == want and len(want) == 2 and all(len(v) > 0 for v in want.values())
    total = add_infos(*infos.values())
    assert cli.read_window_line(total) in said and total["shortened"] > 500, said[-400:]
