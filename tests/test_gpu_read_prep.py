"""mlst_set_read_prep (csrc/read_prep.h): reads trimmed and re-based on the device before they are packed.  The yardstick everywhere:
the engine with the switch ON and the RAW text must leave what the same engine leaves with the switch OFF and the text
fastq.prep_fastq writes -- the packed rows byte for byte (mlst_debug_last_packed), the typed statistics, the counters -- through every
entry that takes FASTQ text; then the exports, the refusals and the life cycle, and `cli type --trim5 / --trim3 / --trim-qual /
--phred64`.  prep_fastq itself is pinned by hand in test_read_prep_host.py."""
import ctypes
import functools
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import read_names_cases as rc
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import prep_fastq
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_sam_all import assert_rule_bytes, export

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFF = {"trim5": 0, "trim3": 0, "trim_qual": 0, "phred64": False}
ZERO = {"shortened": 0, "bases_removed": 0, "emptied": 0}
ALL4 = {"trim5": 7, "trim3": 5, "trim_qual": 20, "phred64": True}
SETTINGS = [{"trim5": 7}, {"trim3": 5}, {"trim_qual": 20}, {"phred64": True}, ALL4, {"trim5": 200, "trim3": 200}]      # the last: more than every read holds
HAND = [[30, 30, 10, 30, 10, 10], [30, 30, 10, 10, 30, 10, 10], [5, 40, 40, 10], [20, 25, 40, 20], [19, 0, 3, 19]]      # test_read_prep_host.py


def ids(s):
    return " ".join("%s=%s" % kv for kv in s.items())


def locus_bases(idx, n: int, k: int) -> bytes:
    """n bases of the allele sequences, from a different place for every k"""
    seq = idx.sequence(k % idx.n_alleles).encode().upper()
    at = (37 * k) % len(seq)
    return (seq[at:] + seq * (n // len(seq) + 1))[:n]


@functools.lru_cache(maxsize=None)
def sample():
    """(index, [(bases, [Phred])]): about 3,000 reads of 36 - 320 bases -- reads of an isolate (on and off the loci) cut to varying
    lengths, one in three with a decayed tail; between them the crafted ones: every length at a 16-byte step, the hand cases alone and
    behind a good front, walks that end at a 16-byte step, non-ACGT bases inside and outside what is trimmed"""
    idx, short = rc.sample(5000, 150)
    _, long_ = rc.sample(1200, 320)
    rng = np.random.default_rng(2026)
    reads = []
    for k, (b, _) in enumerate(short[:2300] + long_[:500]):
        n = int(rng.integers(36, len(b) + 1)) if k % 4 else len(b)
        q = rng.integers(30, 42, size=n)
        if k % 3 == 0:      # a decayed tail, a good base or two inside it
            t = int(rng.integers(1, min(n, 60)))
            q[n - t:] = rng.integers(2, 26, size=t)
            q[n - 1 - t // 2] = 40
        if k % 17 == 0:     # a bad 5' end as well (it stays: the rule trims the 3' end only)
            q[:5] = 2
        b = bytearray(b[:n])
        if k % 29 == 0:
            b[2] = ord("N")                  # inside --trim5 7 only
        if k % 31 == 0:
            b[n - 2] = ord("n")              # inside --trim3 5 only
        if k % 37 == 0:
            b[n // 2] = ord("N")             # in the middle: it stays unless the quality trim reaches it
        if k % 3 == 0 and k % 41 == 0:
            b[n - 1 - (t // 4)] = ord("R")   # in the decayed tail
        reads.append((bytes(b), [int(v) for v in q]))
    crafted = []
    for k, n in enumerate([0, 1, 15, 16, 17, 31, 32, 33, 319, 320]):
        crafted.append((locus_bases(idx, n, k), [40] * n))
        crafted.append((locus_bases(idx, n, k + 50), [40] * (n - n // 3) + [3] * (n // 3)))
        crafted.append((locus_bases(idx, n, k + 90), [2] * n))
    for k, h in enumerate(HAND):
        crafted.append((locus_bases(idx, len(h), k), list(h)))
        crafted.append((locus_bases(idx, 60 + len(h), k + 7), [40] * 60 + list(h)))
        crafted.append((locus_bases(idx, 12 + len(h), k + 9), [25] * 12 + list(h)))      # (all4: the 5' trim reaches into some of them)
    for n in (48, 50, 64, 45):      # the walk over a whole number of 16-byte steps, and where it leaves
        crafted.append((locus_bases(idx, n, n), [40] * (n - 16) + [2] * 16))                     # cut at n - 16
        crafted.append((locus_bases(idx, n, n + 1), [40] * (n - 16) + [40] + [19] * 15))          # negative at byte n - 16: the lowest byte of the first step
        crafted.append((locus_bases(idx, n, n + 2), [40] * (n - 17) + [40] + [19] * 16))          # negative at byte n - 17: the highest byte of the second step
        crafted.append((locus_bases(idx, n, n + 3), [21] * (n - 32) + [19] * 32))                 # the sum is lost one by one: two whole steps, then on
    every = len(reads) // len(crafted)
    for k, c in enumerate(crafted):      # spread over the file: every workgroup of 256 reads and most groups of 64 hold some
        reads.insert(k * every + 5, c)
    return idx, reads


def fastq_text(reads, base: int = 33, eol: bytes = b"\n", header=rc.illumina, first: int = 0) -> bytes:
    return b"".join(header(first + k) + eol + b + eol + b"+" + eol + bytes(v + base for v in q) + eol for k, (b, q) in enumerate(reads))


def base_of(setting) -> int:
    return 64 if setting.get("phred64") else 33


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(sample()[0])
    yield e
    e.close()


def begin(eng, setting):
    eng.reset_sample()
    eng.set_read_prep(**setting)
    assert eng.get_read_prep() == dict(OFF, **setting)


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_prep_info()


def assert_packed_equal(got, want, what=""):
    assert got[3:] == want[3:], (what, "wpr / qstride", got[3:], want[3:])
    assert np.array_equal(got[2], want[2]), (what, "lens", np.nonzero(got[2] != want[2])[0][:10])
    assert np.array_equal(got[1], want[1]), (what, "qrows", np.nonzero((got[1] != want[1]).any(axis=1))[0][:10])
    assert np.array_equal(got[0], want[0]), (what, "packed bases")


def reads_of(eng) -> list:
    """[(lens entry, bases, Phred bytes)] of the last pack, decoded from the resident layout (word w of read i of a 64-read group is
    word (w >> 1) << 7 | i << 1 | w & 1 of the group; base t of a word at bits 2 t): what a sample that arrives in pieces is compared by"""
    packed, qrows, lens, wpr, _ = eng.debug_last_packed()
    g = packed.reshape(-1, 64 * wpr) if len(lens) else packed
    out = []
    for r in range(len(lens)):
        n, i = int(lens[r]) & 0x7FFF, r & 63
        words = [int(g[r >> 6, ((w >> 1) << 7) | (i << 1) | (w & 1)]) for w in range((n + 15) // 16)]
        out.append((int(lens[r]), bytes(b"ACGT"[(words[t >> 4] >> (2 * (t & 15))) & 3] for t in range(n)), qrows[r, :n].tobytes()))
    return out


# ------------------------------------------------------------------ one whole chunk
@pytest.mark.parametrize("setting", SETTINGS, ids=ids)
def test_one_whole_chunk_equals_the_prepared_text(eng, setting):
    idx, reads = sample()
    raw = fastq_text(reads, base_of(setting))
    want_text, want_info = prep_fastq(raw, **setting)
    assert want_info["shortened"] > 0 or setting == {"phred64": True}
    begin(eng, setting)
    assert eng.submit_fastq(raw) == len(reads)
    got = left_behind(eng)
    begin(eng, OFF)
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert want[2] == ZERO and got[2] == want_info, (got[2], want_info)
    assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2]
    if max(setting.get("trim5", 0), setting.get("trim3", 0)) < 200:
        assert int(got[1][0].n_hits.sum()) > 100 and len(got[1][1]) > 100, "the statistics are empty"
        assert (lens & 0x8000).any() and int((lens & 0x7FFF).max()) == 320 - setting.get("trim5", 0) - setting.get("trim3", 0)
    else:
        assert not lens.any() and got[0][3:] == (2, 8) and want_info["emptied"] == len(reads) - 3 and len(got[1][1]) == 0
    # the raw text without the switch is another sample: the test would pass on an engine that ignored the setting otherwise
    begin(eng, OFF)
    eng.submit_fastq(raw)
    plain = eng.debug_last_packed()
    assert not (np.array_equal(plain[2], lens) and plain[1].shape == got[0][1].shape and np.array_equal(plain[1], got[0][1]))
    if setting.get("trim5") == 7 and "trim3" not in setting:      # a non-ACGT base inside the trimmed part only: bit 15 is the prepared read's
        assert int(((plain[2] & 0x8000) != 0).sum()) > int(((lens & 0x8000) != 0).sum())


def test_the_hand_cases_on_the_device(eng):
    """the lengths by hand, without prep_fastq in between"""
    idx, _ = sample()
    want = [4, 2, 3, 4, 0]
    reads = [(locus_bases(idx, len(h), k), h) for k, h in enumerate(HAND)] + [(locus_bases(idx, 60 + len(h), k), [40] * 60 + h) for k, h in enumerate(HAND)]
    for base in (33, 64):
        begin(eng, {"trim_qual": 20, "phred64": base == 64})
        assert eng.submit_fastq(fastq_text(reads, base)) == 10
        lens = eng.debug_last_packed()[2]
        assert [int(v) for v in lens] == want + [60 + w for w in want]
        assert eng.read_prep_info() == {"shortened": 8, "bases_removed": 2 * (2 + 5 + 1 + 4), "emptied": 1}


# ------------------------------------------------------------------ a stream
def test_a_stream_cut_at_every_byte_of_a_sequence_and_a_quality_line(eng):
    idx, reads = sample()
    few = [(b[:90], q[:90]) for b, q in reads[400:520]]
    victim = 60                                                              # a read with a decayed tail in the middle of the file
    few[victim] = (locus_bases(idx, 90, 5), [40] * 70 + [3] * 20)
    raw = fastq_text(few, 64)
    begin(eng, OFF)
    assert eng.submit_fastq(prep_fastq(raw, **ALL4)[0]) == len(few)
    want_reads, want_typed = reads_of(eng), typed(eng)
    want_info = prep_fastq(raw, **ALL4)[1]
    assert want_reads[victim][0] & 0x7FFF < 90 - 12
    start = sum(len(rc.illumina(k)) + 2 * len(b) + 5 for k, (b, _) in enumerate(few[:victim])) + len(rc.illumina(victim)) + 1
    assert raw[start:start + 90] == few[victim][0]
    for cut in range(start - 1, start + 90 + 3 + 90 + 2):      # in front of the sequence line ... behind the quality line's LF
        begin(eng, ALL4)
        n = eng.submit_fastq_stream(raw[:cut], final=False)
        got = reads_of(eng) if n else []
        n += eng.submit_fastq_stream(raw[cut:], final=True)
        got += reads_of(eng)
        assert n == len(few) and got == want_reads, cut
        assert eng.read_prep_info() == want_info, cut
    assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ mates as text
def mate_reads(reads, n_pairs: int):
    """mates of different lengths: every third second mate holds 30 bases, every fifth first mate 20"""
    m1 = [reads[2 * k] if k % 5 else (reads[2 * k][0][:20], reads[2 * k][1][:20]) for k in range(n_pairs)]
    m2 = [reads[2 * k + 1] if k % 3 else (reads[2 * k + 1][0][:30], reads[2 * k + 1][1][:30]) for k in range(n_pairs)]
    return m1, m2


def mate_header(f: int):
    return lambda k: rc.illumina(2 * k).split(b" ")[0] + b" %d:N:0:ACGT" % (f + 1)


PAIR_SETTING = {"trim5": 20, "trim3": 15, "trim_qual": 20}


def test_mates_of_different_lengths_where_one_mate_empties(eng):
    idx, reads = sample()
    m1, m2 = mate_reads(reads, 700)
    t1, t2 = fastq_text(m1, header=mate_header(0)), fastq_text(m2, header=mate_header(1))
    (p1, i1), (p2, i2) = prep_fastq(t1, **PAIR_SETTING), prep_fastq(t2, **PAIR_SETTING)
    assert i1["emptied"] >= 700 // 5 and i2["emptied"] >= 700 // 3
    begin(eng, PAIR_SETTING)
    assert eng.submit_fastq_pair(t1, t2) == 1400
    got = left_behind(eng)
    begin(eng, OFF)
    assert eng.submit_fastq_pair(p1, p2) == 1400
    want = left_behind(eng)
    assert got[2] == {k: i1[k] + i2[k] for k in i1}
    assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2] & 0x7FFF
    assert ((lens[0::2] == 0) & (lens[1::2] > 0)).any() and ((lens[0::2] > 0) & (lens[1::2] == 0)).any() and len(got[1][1]) > 20


# ------------------------------------------------------------------ bgzip
def cuts_inside_quality_lines(text: bytes, sizes) -> int:
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
        n += kind[s][0] == 3 and s < cut < kind[s][1]
    return n


def test_bgzip_with_blocks_cut_inside_quality_lines(eng):
    idx, reads = sample()
    few = reads[:1300]
    raw = fastq_text(few, 64)
    sizes = (4099, 6007, 9001, 2503)
    assert cuts_inside_quality_lines(raw, sizes) > 20
    blocks = bgzf_blocks(raw, sizes)
    want_text, want_info = prep_fastq(raw, **ALL4)
    begin(eng, OFF)
    eng.submit_fastq(want_text)
    want_typed = typed(eng)
    for per_call in (1, 7, len(blocks)):
        begin(eng, ALL4)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == len(few), per_call
        assert eng.read_prep_info() == want_info, per_call
        assert_typed_equal(typed(eng), want_typed)


def test_bgzip_pieces_row_by_row(eng):
    """a block per call, the rows of every piece: reads whose quality line is cut by a block end are prepared once and whole"""
    idx, reads = sample()
    few = reads[:300]
    raw = fastq_text(few, 64)
    sizes = (1201, 2203, 777)
    assert cuts_inside_quality_lines(raw, sizes) > 10
    blocks = bgzf_blocks(raw, sizes)
    begin(eng, OFF)
    eng.submit_fastq(prep_fastq(raw, **ALL4)[0])
    want_reads = reads_of(eng)
    begin(eng, ALL4)
    got, seen = [], 0
    for k, b in enumerate(blocks):
        eng.submit_fastq_bgzf(b, final=k == len(blocks) - 1)
        eng.synchronize()                    # (finishes the piece in flight)
        total = int(eng.stats().counters[2])
        if total > seen:                     # this call's piece completed records: the last pack is theirs
            piece = reads_of(eng)
            assert len(piece) == total - seen, k
            got += piece
            seen = total
    assert seen == len(few) and got == want_reads


def test_bgzipd_mates_with_one_file_ahead(eng):
    idx, reads = sample()
    m1, m2 = mate_reads(reads, 600)
    t1, t2 = fastq_text(m1, 64, header=mate_header(0)), fastq_text(m2, 64, header=mate_header(1))
    setting = dict(PAIR_SETTING, phred64=True)
    (p1, i1), (p2, i2) = prep_fastq(t1, **setting), prep_fastq(t2, **setting)
    begin(eng, OFF)
    assert eng.submit_fastq_pair(p1, p2) == 1200
    want_typed = typed(eng)
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    assert len(b1) > 12 and len(b2) > 45
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])),                           # file 1 nine blocks ahead: its records wait for their mates
             (b"".join(b1[9:10]), b"".join(b2[1:30])),                       # then file 2 overtakes
             (b"", b"".join(b2[30:40])),
             (b"".join(b1[10:]) + eof, b"".join(b2[40:]) + eof)]
    step = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    for what, calls in (("one file ahead", ahead), ("three blocks of each per call", step)):
        begin(eng, setting)
        n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
        assert n == 1200, what
        assert eng.read_prep_info() == {k: i1[k] + i2[k] for k in i1}, what
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ the exports
def test_export_bytes_are_those_of_the_prepared_text(eng, tmp_path):
    idx, reads = sample()
    raw = fastq_text(reads, 64)
    want_text, _ = prep_fastq(raw, **ALL4)
    begin(eng, OFF)
    eng.submit_fastq(want_text)
    recs_off, body_off = export(eng, idx, tmp_path / "off.all.sam")
    md_off = b"".join(eng.export_sam_text(idx, md=True))
    begin(eng, ALL4)
    eng.submit_fastq(raw)
    recs_on, body_on = export(eng, idx, tmp_path / "on.all.sam")
    assert body_on == body_off and len(recs_on) > 100
    assert_rule_bytes(idx, recs_on, body_on)
    assert b"".join(eng.export_sam_text(idx, md=True)) == md_off
    # once with the reads' own names and MD:Z: the header lines are not touched, so the names are the file's
    other = Engine(0, default_params())
    try:
        other.load_reference(idx)
        out = []
        for setting, text in ((ALL4, raw), (OFF, want_text)):
            other.reset_sample()
            other.set_read_prep(**setting)
            other.set_read_names(True)
            other.submit_fastq(text)
            out.append((b"".join(other.export_sam_text(idx, md=True)), other.read_names()))
        assert out[0] == out[1] and len(out[0][1]) > 100
        heads = rc.yardstick([raw])
        assert all(heads[ri].startswith(b"@" + nm) for ri, nm in out[0][1].items())
        assert out[0][0] != md_off and len(out[0][0].splitlines()) == len(md_off.splitlines())
    finally:
        other.close()


# ------------------------------------------------------------------ refusals and life cycle
def test_every_other_way_of_adding_reads_is_refused():
    idx, reads = sample()
    text = fastq_text(reads[:400])
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        assert eng.get_read_prep() == OFF and eng.read_prep_info() == ZERO
        for bad in ({"trim_qual": 94}, {"trim5": 65536}, {"trim3": 65536}):
            with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_prep"):
                eng.set_read_prep(**bad)
        assert eng.lib.mlst_set_read_prep(eng._h, (ctypes.c_uint32 * 4)(0, 0, 0, 48)) == -1
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_prep: phred_base is 48, not 33 or 64"):
            eng._check(-1, "mlst_set_read_prep")
        assert eng.get_read_prep() == OFF
        eng.set_read_prep(trim_qual=93, trim5=65535, trim3=65535)
        assert eng.lib.mlst_set_read_prep(eng._h, None) == 0 and eng.get_read_prep() == OFF      # NULL: off
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
        for setting in ({"phred64": True}, {"trim3": 1}):
            eng.set_read_prep(**setting)
            for entry, call in calls.items():
                with pytest.raises(MlstError, match=r"\(-1\): %s: read preparation is on \(mlst_set_read_prep\) and only the FASTQ text and BGZF entries apply it" % entry):
                    call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text) == 400                                 # the handle stays usable
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_prep"):
            eng.set_read_prep()
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_prep"):
            eng.set_read_prep(trim3=2)
        eng.set_read_prep(trim3=1)                                           # (no change: accepted)
        assert eng.get_read_prep() == dict(OFF, trim3=1) and eng.read_prep_info() == prep_fastq(text, trim3=1)[1]
        eng.reset_sample()                                                   # keeps the setting, zeroes the counters
        assert eng.get_read_prep() == dict(OFF, trim3=1) and eng.read_prep_info() == ZERO
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_prep()
        eng.reset_sample()
        eng.set_read_prep()
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_prep(phred64=True)
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_prep: mlst_set_read_tiling is on"):
            eng.set_read_prep(trim5=1)
        eng.set_read_prep()                                                  # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_prep(**ALL4)
        eng.submit_fastq(fastq_text(reads[:400], 64))
        eng.reset_sample()
        eng.set_read_prep()
        eng.submit_fastq(text)
        got = left_behind(eng)
        fresh = Engine(0, default_params())
        try:
            fresh.load_reference(idx)
            fresh.submit_fastq(text)
            want = left_behind(fresh)
        finally:
            fresh.close()
        assert got[2] == want[2] == ZERO
        assert_packed_equal(got[0], want[0])
        assert_typed_equal(got[1], want[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ the command
def true_alleles(db, idx, st_row: int = 3) -> list:
    """the allele indices of the isolate rc.sample() reads"""
    want = {g: int(a) for (g, _), a in zip(db.loci["ecoli"], db.profiles["ecoli"][st_row])}
    return [a for a in range(idx.n_alleles) if want.get(idx.loci[int(idx.locus_id[a])][1]) == int(idx.allele_no[a])]


def planted_sample():
    """reads of the isolate plus reads tiled over its alleles every second base; two thirds of the tiled reads carry the wrong letter
    at the two middle columns of their locus, at Phred 2: not counted by the pile-up (minqual 20) when the qualities are read with the
    right base, out-voting the right letter when every quality is read 31 too high"""
    idx, reads = sample()
    db, _ = fx.ecoli_small(40, 5)
    out = [r for r in reads if 100 <= len(r[0])][:1500]
    rot = bytes.maketrans(b"ACGT", b"CGTA")
    for a in true_alleles(db, idx):
        seq = idx.sequence(a).encode().upper()
        cols = (len(seq) // 2, len(seq) // 2 + 1)
        for j, s in enumerate(range(0, len(seq) - 100 + 1, 2)):
            b, q = bytearray(seq[s:s + 100]), [40] * 100
            if j % 3:
                for c in cols:
                    if s <= c < s + 100:
                        b[c - s:c - s + 1] = bytes(b[c - s:c - s + 1]).translate(rot)
                        q[c - s] = 2
            out.append((bytes(b), q))
    return out


def run_type(monkeypatch, capsys, cwd, args, out, rc_want=0):
    monkeypatch.chdir(cwd)
    db, _ = fx.ecoli_small(40, 5)
    got = cli.main(["type"] + args + ["-d", db.path, "--min_accuracy", "0", "--nloci", "0", "--log", "-o", str(out)])
    said = capsys.readouterr().out
    assert got == rc_want, said
    return said


def written(out) -> dict:
    """{file name without the --log table's time stamp: bytes}"""
    return {re.sub(r"_\d+\.out$", ".out", os.path.basename(f)): open(f, "rb").read() for f in sorted(glob.glob(str(out) + "/*")) if os.path.isfile(f)}


def test_cli_phred64_types_a_phred64_copy_as_the_original(tmp_path, monkeypatch, capsys):
    reads = planted_sample()
    for d, base in (("p33", 33), ("p64", 64)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / "s.fastq").write_bytes(fastq_text(reads, base))
    run_type(monkeypatch, capsys, tmp_path / "p33", ["s.fastq", "--quiet"], tmp_path / "o33")
    said = run_type(monkeypatch, capsys, tmp_path / "p64", ["s.fastq", "--phred64"], tmp_path / "o64")
    run_type(monkeypatch, capsys, tmp_path / "p64", ["s.fastq", "--quiet"], tmp_path / "o64_noflag")
    want, got, wrong = written(tmp_path / "o33"), written(tmp_path / "o64"), written(tmp_path / "o64_noflag")
    assert sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert got == want
    assert "read preparation: 0 reads shortened, 0 bases removed, 0 reads left without a base" in said
    assert wrong["s.nfo"] != want["s.nfo"] and wrong["s.out"] != want["s.out"]


CLI_TRIMS = ["--trim5", "7", "--trim3", "5", "--trim-qual", "20"]
CLI_SETTING = {"trim5": 7, "trim3": 5, "trim_qual": 20}


def test_cli_trims_on_a_file_a_folder_and_mates(tmp_path, monkeypatch, capsys):
    idx, reads = sample()
    raw_dir, prep_dir = tmp_path / "raw", tmp_path / "prep"
    infos = {}
    for d in (raw_dir, prep_dir):
        os.makedirs(d / "in")
    m1, m2 = mate_reads(reads, 900)
    texts = {"s.fastq": fastq_text(reads), "m_1.fastq": fastq_text(m1, header=mate_header(0)), "m_2.fastq": fastq_text(m2, header=mate_header(1))}
    texts.update({"in/f%d.fastq" % k: fastq_text(reads[k * 900:(k + 1) * 900 + 300]) for k in range(3)})
    for name, text in texts.items():
        (raw_dir / name).write_bytes(text)
        prepared, infos[name] = prep_fastq(text, **CLI_SETTING)
        (prep_dir / name).write_bytes(prepared)
    for what, args, names in (("file", ["s.fastq"], ["s.fastq"]), ("folder", ["in"], ["in/f0.fastq", "in/f1.fastq", "in/f2.fastq"]),
                              ("mates", ["m_1.fastq", "-2", "m_2.fastq"], ["m_1.fastq", "m_2.fastq"])):
        said = run_type(monkeypatch, capsys, raw_dir, args + CLI_TRIMS, tmp_path / ("o_raw_" + what))
        run_type(monkeypatch, capsys, prep_dir, args + ["--quiet"], tmp_path / ("o_prep_" + what))
        got, want = written(tmp_path / ("o_raw_" + what)), written(tmp_path / ("o_prep_" + what))
        assert got == want and len(want) == 2 * (3 if what == "folder" else 1) and all(len(v) > 0 for v in want.values()), what
        n, m, k = (sum(infos[f][key] for f in names) for key in ("shortened", "bases_removed", "emptied"))
        assert "read preparation: %d reads shortened, %d bases removed, %d reads left without a base" % (n, m, k) in said, (what, said[-300:])
    # and the exports carry the prepared SEQ / QUAL
    run_type(monkeypatch, capsys, raw_dir, ["s.fastq", "--quiet", "--write-sam", "--write-sam-all", "--md", "--read-names"] + CLI_TRIMS, tmp_path / "x_raw")
    run_type(monkeypatch, capsys, prep_dir, ["s.fastq", "--quiet", "--write-sam", "--write-sam-all", "--md", "--read-names"], tmp_path / "x_prep")
    got, want = written(tmp_path / "x_raw"), written(tmp_path / "x_prep")
    assert got == want and sorted(want) == ["s.all.sam", "s.nfo", "s.out", "s.sam"] and want["s.all.sam"].count(b"\n") > 500


def test_cli_two_ranks_equal_one_process(tmp_path):
    """in the manner of test_gpu_multirank.py: two ranks on the one GPU, gloo collectives"""
    idx, reads = sample()
    db, _ = fx.ecoli_small(40, 5)
    text = fastq_text(reads, 64)
    (tmp_path / "s.fastq").write_bytes(text)
    os.makedirs(tmp_path / "p")
    (tmp_path / "p" / "s.fastq").write_bytes(prep_fastq(text, **ALL4)[0])
    info = prep_fastq(text, **ALL4)[1]
    env = dict(os.environ, MLST_FASTQ_CHUNK=str(256 << 10), MLST_ONE_GPU="1", MLST_BACKEND="gloo")      # ~0.9 MB of text: several chunks per rank
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    tail = ["-d", db.path, "--min_accuracy", "0", "--nloci", "0", "--log"]
    flags = ["--trim5", "7", "--trim3", "5", "--trim-qual", "20", "--phred64"]
    outs = []
    for cwd, args in ((tmp_path, flags + ["--gpus", "2", "-o", str(tmp_path / "two")]), (tmp_path / "p", ["--quiet", "-o", str(tmp_path / "one")])):
        r = subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "type", "s.fastq"] + tail + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    got, want = written(tmp_path / "two"), written(tmp_path / "one")
    assert got == want and sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    lines = [l for l in outs[0].splitlines() if l.startswith("read preparation:")]
    assert lines == ["read preparation: %d reads shortened, %d bases removed, %d reads left without a base" % (info["shortened"], info["bases_removed"], info["emptied"])]


def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    head = "read preparation (--trim5, --trim3, --trim-qual, --phred64): "
    for args, why in ((["s.fastq", "--alignments"], "with --alignments the records are what they are"),
                      (["c.fa", "--contigs"], "--contigs cuts assemblies into windows"),
                      (["s.fastq", "--long-reads"], "--long-reads cuts reads into windows"),
                      ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts reads into windows"),
                      ([str(bam)], "a reads BAM stores raw Phred and its own strand")):
        for flags in (["--trim5", "3"], ["--trim3", "3"], ["--trim-qual", "20"], ["--phred64"]):
            monkeypatch.chdir(tmp_path)
            assert cli.main(["type"] + args + flags + ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]) == 1
            assert head + why in capsys.readouterr().out, (args, flags)
    for flags, why in ((["--trim-qual", "94"], "--trim-qual takes a number from 0 to 93, not 94"), (["--trim5", "70000"], "--trim5 takes a number from 0 to 65535, not 70000"),
                       (["--trim3=-1"], "--trim3 takes a number from 0 to 65535, not -1")):
        assert cli.main(["type", "s.fastq"] + flags + ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]) == 1
        assert why in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "o")
