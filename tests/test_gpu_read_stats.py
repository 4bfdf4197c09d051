"""mlst_set_read_stats (csrc/read_stats.h): per-cycle quality and base tables counted on the device next to the FASTQ parser.  The
yardstick everywhere is fastq.read_stats, the rule in Python (pinned by hand in test_read_stats_host.py): stage "raw" equals the rule on
the text as given, stage "prepared" the rule on the text fastq.prep_fastq / fastq.trim_adapters write -- every comparison exact integer
equality -- through every entry that takes FASTQ text; then the edges of the kernel's mapping, the life cycle, the refusals and
`cli type --read-stats`."""
import functools
import os

import numpy as np
import pytest

import read_names_cases as rc
import test_gpu_read_prep as rp
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import ADAPTER_NAMES, phred_hint, prep_fastq, read_stats, read_stats_empty, read_stats_sum, read_stats_text, trim_adapters
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks

pytestmark = pytest.mark.gpu

ADAPT = {"adapters": [ADAPTER_NAMES["illumina"]], "min_overlap": 3, "error_permille": 100}
KEYS = ("reads", "bases", "clamped_low", "len_hist", "base", "qual", "gc_hist", "readqual_hist")


def assert_side(got: dict, want: dict, what, skip=()):
    for k in KEYS:
        if k not in skip:
            assert np.array_equal(got[k], want[k]), (what, k, got[k] if np.ndim(got[k]) == 0 else np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:8], want[k] if np.ndim(want[k]) == 0 else None)


def assert_stats(got: dict, raw, prepared, what=""):
    """got: Engine.read_stats(); raw / prepared: [side 0, side 1] of the rule.  prepared None: no trim and no adapter ran, the engine
    reports the raw block (clamped_low included)"""
    for side in (0, 1):
        assert_side(got["raw"][side], raw[side], (what, "raw", side))
        assert_side(got["prepared"][side], (prepared or raw)[side], (what, "prepared", side))
    assert got["prepared_counted"] == (prepared is not None), what


def prepared_text(text: bytes, setting=None, adapters=None) -> bytes:
    t = prep_fastq(text, **setting)[0] if setting else text
    return trim_adapters(t, **adapters)[0] if adapters else t


@functools.lru_cache(maxsize=None)
def corpus(base: int = 33):
    """(text, the rule on it): computed once, shared, left unchanged"""
    text = rp.fastq_text(rp.sample()[1], base)
    return text, read_stats(text, phred64=base == 64)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(rp.sample()[0])
    e.set_read_stats(True)
    yield e
    e.close()


def begin(eng, setting=None, adapters=None, on=True):
    eng.reset_sample()
    eng.set_read_prep(**(setting or rp.OFF))
    eng.set_read_adapters(**(adapters or {}))
    eng.set_read_stats(on)
    assert eng.get_read_stats() == on


# ------------------------------------------------------------------ one whole chunk
def test_no_trims_one_launch_and_prepared_is_raw(eng):
    text, want = corpus()
    begin(eng)
    assert eng.submit_fastq(text) == len(rp.sample()[1])
    assert_stats(eng.read_stats(), want, None)
    info = eng.read_stats_info()
    assert info["raw_launches"] == 1 and info["prepared_launches"] == 0 and info["table_bytes"] == 4 * 32200 * 8
    t = want[0]
    assert t["reads"] > 2800 and t["len_hist"][0] >= 3 and t["len_hist"][320] > 100 and t["base"][:, 4].sum() > 100 and not want[1]["reads"]


@pytest.mark.parametrize("setting", rp.SETTINGS + [None], ids=lambda s: rp.ids(s) if s else "adapter alone")
def test_each_setting_raw_and_prepared(eng, setting):
    adapters = None if setting else ADAPT
    base = rp.base_of(setting or {})
    text, want_raw = corpus(base)
    trims = bool(adapters) or any(setting.get(k) for k in ("trim5", "trim3", "trim_qual"))
    want_prep = read_stats(prepared_text(text, setting, adapters)) if trims else None
    if adapters:
        assert trim_adapters(text, **adapters)[1]["trimmed"] > 20
    begin(eng, setting, adapters)
    eng.submit_fastq(text)
    assert_stats(eng.read_stats(), want_raw, want_prep, setting)
    if trims:
        assert want_prep[0]["bases"] < want_raw[0]["bases"] and want_prep[0]["reads"] == want_raw[0]["reads"]
        assert want_prep[0]["clamped_low"] == 0 and eng.read_stats_info()["prepared_launches"] == 1


# ------------------------------------------------------------------ the five entries, trims and an adapter and Phred+64 at once
ALL = dict(rp.ALL4)


def test_text_stream_cut_mid_record(eng):
    text, want_raw = corpus(64)
    want_prep = read_stats(prepared_text(text, ALL, ADAPT))
    cut = len(text) // 2
    while text[cut - 1:cut] == b"\n":      # inside a line
        cut += 1
    begin(eng, ALL, ADAPT)
    n = eng.submit_fastq_stream(text[:cut], final=False)
    n += eng.submit_fastq_stream(text[cut:], final=True)
    assert n == want_raw[0]["reads"]
    assert_stats(eng.read_stats(), want_raw, want_prep)
    assert eng.read_stats_info()["raw_launches"] == 2 == eng.read_stats_info()["prepared_launches"]


def mates(base=64, n_pairs=700):
    m1, m2 = rp.mate_reads(rp.sample()[1], n_pairs)
    return rp.fastq_text(m1, base, header=rp.mate_header(0)), rp.fastq_text(m2, base, header=rp.mate_header(1))


@functools.lru_cache(maxsize=None)
def mates_rule(odd: bool = False):
    t1, t2 = mates(n_pairs=699 if odd else 700)
    raw = [read_stats(t1, phred64=True, side=0)[0], read_stats(t2, phred64=True, side=1)[1]]
    prep = [read_stats(prepared_text(t1, ALL, ADAPT), side=0)[0], read_stats(prepared_text(t2, ALL, ADAPT), side=1)[1]]
    return t1, t2, raw, prep


@pytest.mark.parametrize("odd", [False, True], ids=["700 pairs", "an odd pair count"])
def test_mate_files_as_text(eng, odd):
    t1, t2, raw, prep = mates_rule(odd)
    begin(eng, ALL, ADAPT)
    assert eng.submit_fastq_pair(t1, t2) == (1398 if odd else 1400)
    assert_stats(eng.read_stats(), raw, prep)
    assert raw[1]["reads"] == raw[0]["reads"] and not np.array_equal(raw[0]["len_hist"], raw[1]["len_hist"])


def test_interleaved_pairs_in_one_text(eng):
    reads = rp.sample()[1][:601 * 2]
    text = rp.fastq_text(reads)
    want = read_stats(text, paired=True)
    begin(eng)
    assert eng.submit_fastq(text, paired=True) == len(reads)
    assert_stats(eng.read_stats(), want, None)
    assert want[0]["reads"] == want[1]["reads"] == 601


def test_bgzip(eng):
    text, want_raw = corpus(64)
    want_prep = read_stats(prepared_text(text, ALL, ADAPT))
    blocks = bgzf_blocks(text, (4099, 6007, 9001, 2503))
    for per_call in (7, len(blocks)):
        begin(eng, ALL, ADAPT)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == want_raw[0]["reads"]
        assert_stats(eng.read_stats(), want_raw, want_prep, per_call)      # (the fetch finishes the piece in flight)


def test_bgzipd_mates(eng):
    t1, t2, raw, prep = mates_rule()
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    calls = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    begin(eng, ALL, ADAPT)
    n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
    assert n == 1400
    assert_stats(eng.read_stats(), raw, prep)


# ------------------------------------------------------------------ the edges of the mapping
# A lane holds 4 cycles (edges 3, 4, 5), a wave's first load 256 (63, 64, 65 lanes' worth is 252 / 256 / 260 bases; 255, 256, 257), the
# second load cycles 256 .. 319 (319, 320); a wave takes a batch of 64 reads (63, 64, 65), a workgroup 16 batches a turn (1023, 1024,
# 1025) and the grid grows by a workgroup per 4096 reads (4096, 4097).
EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 251, 252, 253, 255, 256, 257, 259, 260, 261, 318, 319, 320]


def edge_reads(rng, lengths):
    letters = np.frombuffer(b"ACGTacgtNnRY.-", np.uint8)
    return [(rng.choice(letters, n, p=[.2, .2, .2, .2] + [.02] * 10).tobytes(), [int(v) for v in rng.integers(0, 94, n)]) for n in lengths]


def edge_text(reads, base=33) -> bytes:
    """header k holds k % 16 + 1 letters: sequence and quality lines start at every residue mod 16 of the text offset"""
    return rp.fastq_text(reads, base, header=lambda k: b"@" + b"h" * (k % 16 + (1 if k % 32 < 16 else 2)))


def line_offsets(text: bytes):
    at, seq, qual = 0, set(), set()
    for k, line in enumerate(text.split(b"\n")):
        if k % 4 == 1:
            seq.add(at % 16)
        if k % 4 == 3:
            qual.add(at % 16)
        at += len(line) + 1
    return seq, qual


def test_every_length_edge_at_every_offset(eng):
    rng = np.random.default_rng(11)
    reads = edge_reads(rng, [n for n in EDGE_LENGTHS for _ in range(34)])
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    # written at +33 (characters 33 .. 126) and at +64 (64 .. 157: some of 128 and above), each read under either base: characters
    # below the base under 64, bin 93 for 128 and above under 33
    for written, p64 in ((33, False), (33, True), (64, False), (64, True)):
        text = edge_text(reads, written)
        seq, qual = line_offsets(text)
        assert seq == set(range(16)) == qual
        want = read_stats(text, phred64=p64)
        begin(eng, {"phred64": p64})
        eng.submit_fastq(text)
        assert_stats(eng.read_stats(), want, None, (written, p64))
        assert (want[0]["clamped_low"] > 0) == (written == 33 and p64)
        if written == 64:
            continue
        # and the prepared stage with cycle 0 moved by one, two, three bases: the loads start at every residue behind the trim
        for t5 in (1, 2, 3):
            setting = {"trim5": t5, "phred64": p64}
            begin(eng, setting)
            eng.submit_fastq(text)
            assert_stats(eng.read_stats(), want, read_stats(prep_fastq(text, **setting)[0]), (p64, t5))


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097])
def test_chunks_at_the_batch_workgroup_and_grid_edges(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    reads = edge_reads(rng, [int(v) for v in rng.choice([0, 1, 5, 9, 33], n_reads)])
    reads[-1] = edge_reads(rng, [320])[0]      # the last read of the last batch is a whole one
    text = edge_text(reads)
    want = read_stats(text)
    begin(eng)
    assert eng.submit_fastq(text) == n_reads
    assert_stats(eng.read_stats(), want, None)


@pytest.mark.parametrize("n_pairs", [1, 33, 63, 65, 2049])
def test_paired_chunks_with_odd_pair_counts(eng, n_pairs):
    rng = np.random.default_rng(n_pairs)
    reads = edge_reads(rng, [int(v) for v in rng.choice([0, 2, 6, 40, 300], 2 * n_pairs)])
    text = edge_text(reads)
    want = read_stats(text, paired=True)
    begin(eng)
    assert eng.submit_fastq(text, paired=True) == 2 * n_pairs
    assert_stats(eng.read_stats(), want, None)


def test_4000_identical_reads_and_4000_that_differ_at_cycle_0(eng):
    same = [(b"ACGTN" * 30, [30 + (c % 11) for c in range(150)])] * 4000      # every add of a cycle lands on one cell
    text = rp.fastq_text(same)
    want = read_stats(text)
    assert want[0]["qual"][0, 30] == 4000 and want[0]["base"][4, 4] == 4000 and want[0]["readqual_hist"][34] == 4000
    begin(eng)
    eng.submit_fastq(text)
    assert_stats(eng.read_stats(), want, None, "identical")
    differ = [(b"ACGT"[k % 4:k % 4 + 1] + b"G" * 99, [k % 94] + [40] * 99) for k in range(4000)]      # 94 cells of cycle 0, one cell behind it
    text = rp.fastq_text(differ)
    want = read_stats(text)
    assert (want[0]["qual"][0] > 0).all() and want[0]["qual"][1, 40] == 4000
    begin(eng)
    eng.submit_fastq(text)
    assert_stats(eng.read_stats(), want, None, "different at cycle 0")


# ------------------------------------------------------------------ the sample's life
def test_three_submissions_add_up_reset_zeroes_and_the_setting_is_refused_mid_sample(eng):
    reads = rp.sample()[1]
    parts = [rp.fastq_text(reads[a:b], first=a) for a, b in ((0, 700), (700, 1500), (1500, 2100))]
    whole = b"".join(parts)
    setting = {"trim_qual": 20}
    want_raw, want_prep = read_stats(whole), read_stats(prep_fastq(whole, **setting)[0])
    begin(eng, setting)
    for p in parts:
        eng.submit_fastq(p)
    assert_stats(eng.read_stats(), want_raw, want_prep)
    assert eng.read_stats_info()["raw_launches"] == 3
    with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_stats"):
        eng.set_read_stats(False)
    eng.set_read_stats(True)                                                 # (no change: accepted)
    eng.set_read_stats_side(1)                                               # the side may change between submissions
    eng.reset_sample()                                                       # keeps the switch, zeroes the tables and the side
    assert eng.get_read_stats() is True
    zero = [read_stats_empty(), read_stats_empty()]
    assert_stats(eng.read_stats(), zero, None)
    assert eng.read_stats_info()["raw_launches"] == 0
    eng.submit_fastq(parts[0])
    assert_stats(eng.read_stats(), read_stats(parts[0]), read_stats(prep_fastq(parts[0], **setting)[0]), "side 0 again behind the reset")
    eng.reset_sample()
    eng.submit_fastq_stream(parts[0][:1000], final=False)                    # a stream is open
    with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
        eng.set_read_stats(False)
    with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
        eng.set_read_stats_side(1)
    eng.reset_sample()
    with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_stats_side: side is 2, not 0 or 1"):
        eng.set_read_stats_side(2)


def test_the_side_switch_reports_two_unpaired_texts_apart(eng):
    t1, t2 = mates(33, 300)
    want = [read_stats(t1)[0], read_stats(t2, side=1)[1]]
    begin(eng)
    eng.submit_fastq(t1)
    eng.set_read_stats_side(1)
    eng.submit_fastq(t2)
    assert_stats(eng.read_stats(), want, None)
    eng.set_read_stats_side(0)
    eng.submit_fastq(t2)
    want[0] = read_stats_sum(want[0], read_stats(t2)[0])
    assert_stats(eng.read_stats(), want, None, "back on side 0")


def test_typing_is_untouched_by_the_switch(eng):
    text, _ = corpus(64)
    left = []
    for on in (True, False):
        begin(eng, ALL, ADAPT, on=on)
        eng.submit_fastq(text)
        left.append((eng.debug_last_packed(), typed(eng), eng.read_prep_info(), eng.read_adapters_info()))
    rp.assert_packed_equal(left[0][0], left[1][0])
    assert_typed_equal(left[0][1], left[1][1])
    assert left[0][2:] == left[1][2:] and left[0][2]["shortened"] > 0 and left[0][3]["trimmed"] > 0
    assert len(left[0][1][1]) > 100, "the statistics are empty"
    eng.reset_sample()
    eng.set_read_stats(True)


def test_switch_off_nothing_is_queued_or_allocated():
    idx = rp.sample()[0]
    text, _ = corpus()
    e = Engine(0, default_params())
    try:
        e.load_reference(idx)
        assert e.get_read_stats() is False
        e.submit_fastq(text)
        assert e.read_stats_info() == {"raw_launches": 0, "prepared_launches": 0, "table_bytes": 0}
        got = e.read_stats()
        assert_stats(got, [read_stats_empty(), read_stats_empty()], None)
    finally:
        e.close()


def test_every_other_way_of_adding_reads_is_refused():
    idx, reads = rp.sample()
    e = Engine(0, default_params())
    try:
        e.load_reference(idx)
        e.set_read_stats(True)
        fb = np.frombuffer(reads[0][0], np.uint8); fq = np.frombuffer(bytes(v + 33 for v in reads[0][1]), np.uint8); off = np.array([0, len(fb)], np.uint64)
        calls = {
            "mlst_submit_reads": lambda: e.submit_reads(fb, fq, off),
            "mlst_submit_reads_device": lambda: e.submit_reads_device(0, 0, 0, 1, 150),
            "mlst_submit_packed_device": lambda: e.submit_packed_device(0, 0, 0, 1, 10, 152),
            "mlst_submit_packed_host": lambda: e._check(e.lib.mlst_submit_packed_host(e._h, None, None, None, 1, 10, 152, 0), "mlst_submit_packed_host"),
            "mlst_submit_fasta": lambda: e.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n"),
            "mlst_bam_reads_open": lambda: e.bam_reads_open(0),
            "mlst_set_read_tiling": lambda: e.set_read_tiling(150, 25),
        }
        for entry, call in calls.items():
            with pytest.raises(MlstError, match=r"\(-1\): %s: read statistics are on \(mlst_set_read_stats\) and only the FASTQ text and BGZF entries count their reads" % entry):
                call()
        assert e.get_read_tiling() == (0, 0)
        text = rp.fastq_text(reads[:400])
        assert e.submit_fastq(text) == 400                                   # the handle stays usable
        assert_stats(e.read_stats(), read_stats(text), None)
        e.reset_sample()
        e.set_read_stats(False)
        e.submit_reads(fb, fq, off)                                          # off again: every entry is open
        e.reset_sample()
        e.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_stats: mlst_set_read_tiling is on"):
            e.set_read_stats(True)
        e.set_read_tiling(0, 0)
    finally:
        e.close()


def test_a_malformed_chunk_is_refused_as_before_and_not_counted(eng):
    reads = rp.sample()[1]
    good = rp.fastq_text(reads[:300])
    bad = rp.fastq_text(reads[300:400]).replace(b"\n+\n", b"\n+\nII", 1)      # one quality line two characters longer than its sequence
    begin(eng, {"trim_qual": 20})
    eng.submit_fastq(good)
    with pytest.raises(MlstError, match="malformed FASTQ"):
        eng.submit_fastq(bad)
    # (the kernel leaves at once on the parser's error bits: nothing of the chunk is counted.  The sample is not typed, and the
    # command reads no table behind the error)
    assert_stats(eng.read_stats(), read_stats(good), read_stats(prep_fastq(good, trim_qual=20)[0]))
    begin(eng)
    eng.submit_fastq(good)
    assert_stats(eng.read_stats(), read_stats(good), None, "the handle stays usable")


# ------------------------------------------------------------------ the command
def test_cli_report_file_and_the_nfo(tmp_path, monkeypatch, capsys):
    text, want = corpus()
    (tmp_path / "s.fastq").write_bytes(text)
    said = rp.run_type(monkeypatch, capsys, tmp_path, ["s.fastq", "--read-stats", "--trim-qual", "20"], tmp_path / "on")
    rp.run_type(monkeypatch, capsys, tmp_path, ["s.fastq", "--quiet", "--trim-qual", "20"], tmp_path / "off")
    got, plain = rp.written(tmp_path / "on"), rp.written(tmp_path / "off")
    assert sorted(got) == ["s.nfo", "s.out", "s.readstats.tsv"] and sorted(plain) == ["s.nfo", "s.out"]
    assert got["s.nfo"] == plain["s.nfo"] and got["s.out"] == plain["s.out"] and len(plain["s.nfo"]) > 0
    rule = {"raw": want, "prepared": read_stats(prep_fastq(text, trim_qual=20)[0]), "phred_base": 33, "prepared_counted": True}
    assert got["s.readstats.tsv"] == read_stats_text(rule, "s")
    lines = [l for l in said.splitlines() if l.startswith("read statistics")]
    assert len(lines) == 2 and lines[0].startswith("read statistics (raw, side 0): %d reads, %d bases" % (want[0]["reads"], want[0]["bases"]))
    assert lines[1].startswith("read statistics (prepared, side 0): %d reads, %d bases" % (rule["prepared"][0]["reads"], rule["prepared"][0]["bases"]))
    assert phred_hint(rule) is None and "Phred+64" not in said


def test_cli_mates_with_different_names_and_the_phred64_hint(tmp_path, monkeypatch, capsys):
    m1, m2 = rp.mate_reads(rp.sample()[1], 400)
    t1, t2 = rp.fastq_text(m1, 64), rp.fastq_text(m2, 64, header=lambda k: b"@other%d" % k)      # names differ: two unpaired texts
    (tmp_path / "m_1.fastq").write_bytes(t1)
    (tmp_path / "m_2.fastq").write_bytes(t2)
    said = rp.run_type(monkeypatch, capsys, tmp_path, ["m_1.fastq", "-2", "m_2.fastq", "--read-stats"], tmp_path / "o")
    want = [read_stats(t1)[0], read_stats(t2, side=1)[1]]
    rule = {"raw": want, "prepared": want, "phred_base": 33, "prepared_counted": False}
    assert rp.written(tmp_path / "o")["m_1.readstats.tsv"] == read_stats_text(rule, "m_1")
    assert phred_hint(rule) in said and "looks like Phred+64" in said and "--phred64" in said
    assert sum(l.startswith("read statistics (raw, side") for l in said.splitlines()) == 2
    # `a.fq,b.fq` stays side 0, and with --phred64 nothing is hinted
    said = rp.run_type(monkeypatch, capsys, tmp_path, ["m_1.fastq,m_2.fastq", "--read-stats", "--phred64"], tmp_path / "o2")
    both = [read_stats_sum(read_stats(t1, phred64=True)[0], read_stats(t2, phred64=True)[0]), read_stats_empty()]
    rule = {"raw": both, "prepared": both, "phred_base": 64, "prepared_counted": False}
    assert rp.written(tmp_path / "o2")["m_1.readstats.tsv"] == read_stats_text(rule, "m_1")
    assert "Phred+64" not in said
