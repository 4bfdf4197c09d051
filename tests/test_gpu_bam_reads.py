"""The reads of a BGZF BAM typed on the device (mlst_bam_reads_open / mlst_submit_bam_bgzf, csrc/bam_reads.h) against the rules
applied on the host (samin.bam_reads_fastq) followed by the FASTQ text path: the same packed rows, statistics, work items, chosen
alleles and consensus letters.  The inputs are the record zoo of tests/bam_reads_zoo.py (its figures: tests/test_bam_reads_host.py)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bam_reads_zoo as bz
import fixtures as fx
from metamlst_amd import samin

pytestmark = pytest.mark.gpu


def make_engine(verify=False):
    from metamlst_amd.engine import Engine
    eng = Engine(0)
    eng.load_reference(fx.ecoli_small()[1])
    eng.set_bgzf_verify(verify)
    return eng


def typed(eng):
    """what a sample leaves behind: statistics, sorted work items, chosen alleles and consensus letters"""
    st, items = eng.stats(), fx.sorted_items(eng.items())
    eng.typing_enqueue()
    _, chosen, letters = eng.typing_fetch()
    return st, items, chosen, letters


def assert_typed_equal(got, want):
    fx.assert_stats_equal(got[0], want[0])
    assert int(got[0].counters[2]) == int(want[0].counters[2])      # reads seen
    assert np.array_equal(got[1], want[1]), "work items differ"
    assert got[2] == want[2], "chosen alleles differ"
    assert got[3].keys() == want[3].keys() and all(bytes(got[3][a]) == bytes(want[3][a]) for a in got[3]), "consensus letters differ"


def feed(eng, path, paired=False, blocks_per_call=None, cut_inside=False, empty_final=False):
    """the records' blocks of a BAM into a reads stream: calls of blocks_per_call BGZF blocks (None: one call), or one buffer that
    ends inside a block and a second with the rest (n_consumed_out); empty_final: no call with data is marked final, a call
    without data closes the stream; -> records counted by the calls"""
    names, lo, skip = samin.read_bam_header(path)
    raw = open(path, "rb").read()[lo:]
    eng.bam_reads_open(len(names), skip, paired)
    if cut_inside:
        blocks = bz.bgzf_blocks(raw)
        at = blocks[len(blocks) // 2][0] + blocks[len(blocks) // 2][1] // 2
        n1, used = eng.submit_bam_bgzf(raw[:at], final=False, partial=True)
        assert used == blocks[len(blocks) // 2][0]
        return n1 + eng.submit_bam_bgzf(raw[used:], final=True)[0]
    if blocks_per_call is None:
        return eng.submit_bam_bgzf(raw, final=True)[0]
    blocks, n = bz.bgzf_blocks(raw), 0
    for k in range(0, len(blocks), blocks_per_call):
        hi = blocks[min(k + blocks_per_call, len(blocks)) - 1]
        n += eng.submit_bam_bgzf(raw[blocks[k][0]:hi[0] + hi[1]], final=not empty_final and k + blocks_per_call >= len(blocks))[0]
    if empty_final:
        n += eng.submit_bam_bgzf(b"", final=True)[0]
    return n


def host_counts(path, paired=False):
    counts = {}
    text = b"".join(samin.bam_reads_fastq(path, paired=paired, counts=counts))
    return text, counts


@pytest.fixture(scope="module")
def eng():
    return make_engine()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """the zoo of ~6,000 reads: its file, the yardstick text and counts, and what the text path makes of it (computed once)"""
    d = tmp_path_factory.mktemp("bamreads")
    recs = bz.zoo(6000)
    path = bz.write(d / "zoo.bam", recs)
    text, counts = host_counts(path)
    ref = make_engine()
    assert ref.submit_fastq(text) == 6000
    want = typed(ref)
    assert int((want[0].n_hits > 0).sum()) >= 7 and len(want[1]) >= 100      # some hundred reads land on loci
    return {"path": path, "text": text, "counts": counts, "want": want, "n_records": len(recs), "dir": d}


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bampairs")
    recs = bz.zoo_paired(3000)
    path = bz.write(d / "pairs.bam", recs)
    text, counts = host_counts(path, paired=True)
    t1, t2 = bz.split_fastq(text)
    ref = make_engine()
    assert ref.submit_fastq_pair(t1, t2) == 6000
    want = typed(ref)
    ref.reset_sample(); ref.submit_fastq(text)
    unpaired = ref.stats()
    return {"path": path, "text": text, "mates": (t1, t2), "counts": counts, "want": want, "unpaired": unpaired, "n_records": len(recs), "dir": d}


# ------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("n_kept", [63, 64, 65, 6000])
def test_packed_rows_equal_the_host_pack_of_the_yardstick_text(eng, tmp_path, n_kept):
    from metamlst_amd.engine import pack_fastq_host
    path = bz.write(tmp_path / "z.bam", bz.zoo(n_kept))
    text, counts = host_counts(path)
    eng.reset_sample()
    assert eng.submit_bam_reads_file(path) == n_kept
    packed, qrows, lens, wpr, qs = eng.debug_last_packed()
    h_packed, h_qrows, h_lens, n, h_wpr, h_qs = pack_fastq_host(text, read_len_max=320)
    assert (n, h_wpr, h_qs) == (n_kept, wpr, qs) and lens.size == n_kept
    assert np.array_equal(lens, h_lens[:n]), np.nonzero(lens != h_lens[:n])[0][:10]
    assert np.array_equal(qrows, h_qrows[:n]), np.unique(np.nonzero(qrows != h_qrows[:n])[0])[:10]
    assert np.array_equal(packed, h_packed[:packed.size]), np.nonzero(packed != h_packed[:packed.size])[0][:10]
    assert packed.size == ((n + 63) // 64) * 64 * wpr
    assert eng.bam_reads_info()[:3] == (n_kept, counts["secondary"], counts["empty"])
    assert (lens & 0x8000).any() and (qrows & 0x80).any()      # reads with non-ACGT bases are among them


# ------------------------------------------------------------------ 2. typing equals the text path
@pytest.mark.parametrize("mode", ["file", "one_call", "one_block", "two_blocks", "cut_inside_a_block", "serial", "force_miss"])
def test_typing_equals_the_text_path(eng, big, mode, monkeypatch):
    e = eng
    if mode == "serial":      # (the switch is read once per handle)
        monkeypatch.setenv("MLST_BGZF_PIPE", "0")
        e = make_engine()
    e.reset_sample()
    if mode == "force_miss":
        e.debug_bam_split(3)
    try:
        if mode == "file":
            assert e.submit_bam_reads_file(big["path"]) == 6000
        else:
            n = feed(e, big["path"], blocks_per_call={"one_block": 1, "two_blocks": 2}.get(mode), cut_inside=mode == "cut_inside_a_block")
            assert n == big["n_records"]
        info = e.bam_reads_info()
    finally:
        if mode == "force_miss":
            e.debug_bam_split(0)
    assert info[:3] == (6000, big["counts"]["secondary"], big["counts"]["empty"])
    assert info[3] > 0 or mode != "force_miss"      # k_bam_link walked cells again
    assert_typed_equal(typed(e), big["want"])


# ------------------------------------------------------------------ 3. pairs
@pytest.mark.parametrize("blocks_per_call", [None, 1])
def test_paired_stream_equals_submit_fastq_pair(eng, pairs, blocks_per_call):
    eng.reset_sample()
    assert feed(eng, pairs["path"], paired=True, blocks_per_call=blocks_per_call) == pairs["n_records"]
    assert eng.bam_reads_info()[:3] == (6000, pairs["counts"]["secondary"], pairs["counts"]["empty"])
    got = typed(eng)
    assert_typed_equal(got, pairs["want"])
    assert not np.array_equal(got[0].locus_len_sum, pairs["unpaired"].locus_len_sum)      # pairing is what changes this figure


def test_paired_stream_closed_by_a_call_without_data(eng, pairs, tmp_path):
    """no data call is marked final: what the last piece handed on (a whole kept record, a partial record, nothing) is judged by a
    closing piece that holds the carry alone"""
    from metamlst_amd.engine import MlstError
    eng.reset_sample()
    assert feed(eng, pairs["path"], paired=True, blocks_per_call=1, empty_final=True) == pairs["n_records"]
    assert_typed_equal(typed(eng), pairs["want"])
    # an odd kept count: the last kept record waits in the carry for a mate that never comes
    recs = bz.zoo_paired(400)
    recs.insert(len(recs) - 1, bz.unmapped("single", *bz.isolate()[5], flag=77))
    odd = bz.write(tmp_path / "odd.bam", recs)
    eng.reset_sample()
    with pytest.raises(MlstError, match="record %d has no mate next to it" % (len(recs) - 2)):
        feed(eng, odd, paired=True, blocks_per_call=1, empty_final=True)
    # the file cut inside a record
    cut = bz.reblock(gzip.open(pairs["path"], "rb").read()[:-30], tmp_path / "cut.bam")
    eng.reset_sample()
    with pytest.raises(MlstError, match="truncated BAM"):
        feed(eng, cut, paired=True, blocks_per_call=1, empty_final=True)
    eng.reset_sample()
    assert feed(eng, pairs["path"], paired=True) == pairs["n_records"]
    fx.assert_stats_equal(eng.stats(), pairs["want"][0])


def test_paired_errors_leave_the_handle_usable(eng, pairs, big, tmp_path):
    from metamlst_amd.engine import MlstError
    a, b = bz.isolate()[0], bz.isolate()[1]
    good = [bz.unmapped("p0", *a, flag=77), bz.unmapped("p0", *b, flag=141)]
    bad = {"names": (good + [bz.unmapped("p1", *a, flag=77), bz.skipped("empty", 0), bz.unmapped("p2", *b, flag=141)], 2),
           "flag": (good + [bz.skipped("secondary", 0), bz.unmapped("p1", *a, flag=77), bz.unmapped("p1", *b, flag=4)], 4),
           "odd": (good + [bz.unmapped("p1", *a, flag=77), bz.skipped("empty", 1)], 2)}
    for name, (recs, at) in bad.items():
        path = bz.write(tmp_path / (name + ".bam"), recs)
        with pytest.raises(ValueError, match="record %d has no mate next to it" % at):
            b"".join(samin.bam_reads_fastq(path, paired=True))
        eng.reset_sample()
        with pytest.raises(MlstError, match=r"record %d has no mate next to it \(a paired BAM must be collated by name\)" % at):
            eng.submit_bam_reads_file(path, paired=True)
        eng.reset_sample()
        assert feed(eng, pairs["path"], paired=True) == pairs["n_records"]
        fx.assert_stats_equal(eng.stats(), pairs["want"][0])
    eng.reset_sample()      # ... and a FASTQ sample behind it sees nothing of the BAM samples
    eng.submit_fastq(big["text"])
    assert_typed_equal(typed(eng), big["want"])


# ------------------------------------------------------------------ 4. limits and damage
def test_limits_damage_and_stream_exclusion(eng, big, tmp_path):
    from metamlst_amd.engine import CorruptInput, MlstError, crc_checked
    from test_bam_gpu import flip_in_block
    seq = "ACGT" * 81
    long_ = bz.write(tmp_path / "long.bam", bz.zoo(63) + [bz.unmapped("r321", seq[:321], "I" * 321)])
    eng.reset_sample()
    with pytest.raises(MlstError, match=r"\(-5\).*a BAM read is longer than 320 bases"):
        eng.submit_bam_reads_file(long_)
    # the file cut inside its last record (whole BGZF blocks all the same)
    text = gzip.open(big["path"], "rb").read()[:-40]
    cut = bz.reblock(text, tmp_path / "cut.bam")
    eng.reset_sample()
    with pytest.raises(MlstError, match="truncated BAM"):
        eng.submit_bam_reads_file(cut)
    # one byte of a block's text changed, its length kept: only the CRC-32 tells
    flipped = str(tmp_path / "flip.bam")
    open(flipped, "wb").write(flip_in_block(open(big["path"], "rb").read(), 3))
    eng.reset_sample()
    eng.set_bgzf_verify(True)
    try:
        with pytest.raises(CorruptInput, match="flip.bam.*CRC mismatch in BGZF block"):
            crc_checked([flipped], lambda: eng.submit_bam_reads_file(flipped))
        eng.reset_sample()
        assert eng.submit_bam_reads_file(big["path"]) == 6000      # the intact file passes the check
    finally:
        eng.reset_sample()
        eng.set_bgzf_verify(False)
    # a reads stream excludes the FASTQ entries and the other way round
    names, lo, skip = samin.read_bam_header(big["path"])
    eng.bam_reads_open(len(names), skip)
    with pytest.raises(MlstError, match="BAM stream is open"):
        eng.submit_fastq(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(MlstError, match="BAM stream is open"):
        eng.bam_reads_open(len(names), skip)
    eng.reset_sample()
    part = np.frombuffer(b"@r\nACGT\n+\nIIII\n@r2\nAC", np.uint8)
    n = C.c_uint64()
    assert eng.lib.mlst_submit_fastq_stream(eng._h, part.ctypes.data_as(C.c_void_p), part.size, 0, 0, C.byref(n)) == 0
    with pytest.raises(MlstError, match="FASTQ stream is open"):
        eng.bam_reads_open(len(names), skip)
    eng.reset_sample()
    assert eng.submit_bam_reads_file(big["path"]) == 6000
    assert_typed_equal(typed(eng), big["want"])


# ------------------------------------------------------------------ 5. CLI
def _cli(args):
    from metamlst_amd.cli import main
    return main(args)


def _nfo(out, name="smp"):
    p = os.path.join(out, name + ".nfo")
    return open(p, "rb").read() if os.path.exists(p) else None


def test_cli_types_the_reads_of_a_bam(big, pairs, tmp_path, capsys):
    import shutil
    dbp = fx.ecoli_small()[0].path
    d = {k: str(tmp_path / k) for k in ("bam", "fq", "pbam", "pfq", "two")}
    for k in d:
        os.mkdir(d[k])
    shutil.copy(big["path"], d["bam"] + "/smp.bam"); open(d["fq"] + "/smp.fastq", "wb").write(big["text"])
    shutil.copy(pairs["path"], d["pbam"] + "/smp.bam")
    open(d["pfq"] + "/smp.fastq", "wb").write(pairs["mates"][0]); open(d["pfq"] + "/mates.fastq", "wb").write(pairs["mates"][1])
    assert _cli(["type", d["bam"] + "/smp.bam", "-d", dbp, "-o", d["bam"] + "/out"]) == 0
    said = capsys.readouterr().out
    assert "6000 reads taken, %d secondary / supplementary and %d empty records skipped" % (big["counts"]["secondary"], big["counts"]["empty"]) in said
    assert _cli(["type", d["fq"] + "/smp.fastq", "-d", dbp, "-o", d["fq"] + "/out", "--quiet"]) == 0
    single = _nfo(d["bam"] + "/out")
    assert single is not None and single == _nfo(d["fq"] + "/out")
    # a name-collated paired BAM: as -2 on the two mate texts
    loose = ["--min_accuracy", "0.3", "--nloci", "50"]      # (a third of these pairs are one fragment read twice: the loci are covered with holes)
    assert _cli(["type", d["pbam"] + "/smp.bam", "-d", dbp, "-o", d["pbam"] + "/out"] + loose) == 0
    assert "6000 reads taken as pairs" in capsys.readouterr().out
    assert _cli(["type", d["pfq"] + "/smp.fastq", "-2", d["pfq"] + "/mates.fastq", "-d", dbp, "-o", d["pfq"] + "/out", "--quiet"] + loose) == 0
    paired = _nfo(d["pbam"] + "/out")
    assert paired is not None and paired == _nfo(d["pfq"] + "/out")
    # -2 and --gpus N do not go with a BAM
    assert _cli(["type", d["bam"] + "/smp.bam", "-2", d["pfq"] + "/mates.fastq", "-d", dbp, "-o", d["two"] + "/x"]) == 1
    assert _cli(["type", d["bam"] + "/smp.bam", "--gpus", "2", "-d", dbp, "-o", d["two"] + "/x"]) == 1
    assert "applies to FASTQ input" in capsys.readouterr().out and not os.path.exists(d["two"] + "/x")
    # two BAMs on one command line are two samples
    shutil.copy(big["path"], d["two"] + "/one.bam"); shutil.copy(pairs["path"], d["two"] + "/other.bam")
    assert _cli(["type", d["two"] + "/one.bam", d["two"] + "/other.bam", "-d", dbp, "-o", d["two"] + "/out"] + loose) == 0
    said = capsys.readouterr().out      # the line on what was taken, once per BAM
    assert "one.bam: 6000 reads taken, " in said and "other.bam: 6000 reads taken as pairs, " in said
    assert _cli(["type", d["bam"] + "/smp.bam", "-d", dbp, "-o", d["bam"] + "/out_loose", "--quiet"] + loose) == 0
    single = _nfo(d["bam"] + "/out_loose")
    assert single is not None
    assert _nfo(d["two"] + "/out", "one") == single.replace(b"smp", b"one") and _nfo(d["two"] + "/out", "other") == paired.replace(b"smp", b"other")


def test_cli_alignments_switch_still_takes_the_alignment_path(tmp_path, capsys):
    import golden_util as gu
    from test_bam_gpu import CASES, sam_to_bam
    import glob
    import json
    dbp = gu.golden_db()
    argv = [a for a in json.load(open(os.path.join(CASES[0], "args.json"))) if a != "--log"]      # (the case's own thresholds)
    sam, bam = str(tmp_path / "smp.sam"), str(tmp_path / "smp.bam")
    open(sam, "wb").write(open(os.path.join(CASES[0], "input.sam"), "rb").read())
    sam_to_bam(sam, bam)
    assert _cli(["type", sam, "--alignments", "-d", dbp, "-o", str(tmp_path / "o_sam"), "--quiet", "--log"] + argv) == 0
    assert _cli(["type", bam, "--alignments", "-d", dbp, "-o", str(tmp_path / "o_bam"), "--log"] + argv) == 0
    assert "reads taken" not in capsys.readouterr().out
    assert _nfo(str(tmp_path / "o_bam")) == _nfo(str(tmp_path / "o_sam"))
    # the --log table of the accumulation of metamlst.py:101-130 (a table of alignment records, which the reads path does not write like this)
    logs = [glob.glob(str(tmp_path / o) + "/smp_*.out") for o in ("o_bam", "o_sam")]
    assert len(logs[0]) == len(logs[1]) == 1
    tables = [open(l[0], "rb").read().split(b"\r\n", 1)[1] for l in logs]
    assert tables[0] == tables[1] and len(tables[0]) > 100
