"""FASTQ records longer than the tile cut into windows on the device (mlst_set_read_tiling, csrc/fastq_tile.h) against the text
fastq.tile_fastq writes followed by the FASTQ text path with tiling off: the same packed rows byte for byte, and -- by every route a
text can take -- the same statistics, read indices, chosen alleles and consensus letters; the refusals; the command.  The builders and
the comparison are tests/long_reads.py (its figures: tests/test_long_reads_host.py)."""
import glob
import gzip
import os

import numpy as np
import pytest

import fixtures as fx
import long_reads as lr
from metamlst_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return fx.ecoli_small(80)


def make_engine(ref):
    from metamlst_amd.engine import Engine
    eng = Engine(0)
    eng.load_reference(ref[1])
    return eng


@pytest.fixture(scope="module")
def eng(ref):
    return make_engine(ref)


N_READS = 1800      # of 400 .. 3,000 bases over 100,000: ~30 reads over every base, about half of them with Phred >= 20 there


def typed(eng):
    st = eng.stats()
    eng.typing_enqueue()
    _, chosen, letters = eng.typing_fetch()
    return st, chosen, letters


def assert_typed_equal(got, want):
    fx.assert_stats_equal(got[0], want[0])      # (locus_first among them: the read indices)
    assert int(got[0].counters[2]) == int(want[0].counters[2])
    assert got[1] == want[1]
    assert got[2].keys() == want[2].keys() and all(bytes(got[2][a]) == bytes(want[2][a]) for a in got[2])


# ------------------------------------------------------------------ 1. rows byte for byte
@pytest.mark.parametrize("tile", lr.TILES)
def test_rows_of_every_edge_length_in_one_chunk(eng, tile):
    lengths = lr.edge_lengths(*tile)      # 32,768 and 100,003 bases: lengths a 16-bit field with bit 15 taken cannot hold
    want = sum(lr.fa_windows_of(n, *tile) for n in lengths)
    assert lr.assert_rows_equal(eng, lr.text_of(lr.random_records(lengths)), tile) == want


@pytest.mark.parametrize("eol, final_eol", [(b"\r\n", True), (b"\n", False), (b"\r\n", False)])
def test_rows_with_crlf_and_without_the_last_newline(eng, eol, final_eol):
    seqs = lr.random_records([400, 150, 0, 151, 7, 1000, 333])      # (the last record is cut: its quality line ends the text)
    lr.assert_rows_equal(eng, lr.text_of(seqs, eol, final_eol), (150, 25))


def test_rows_of_reads_with_scattered_n_and_lower_case(eng):
    rng = np.random.default_rng(lr.SEED + 1)
    seqs = []
    for k, n in enumerate([400, 900, 151, 150, 2000, 320, 321]):
        s = bytearray(lr.bases(rng, n))
        if k % 2 == 0:
            s[n // 2] = ord("N")                      # one N: the windows over the middle hold it, the others do not
        s[n // 3:n // 3 + 11] = bytes(s[n // 3:n // 3 + 11]).lower()
        if k == 4:
            s[0] = ord("n"); s[n - 1] = ord("R")      # the first window's first base, the last window's last
        seqs.append(bytes(s))
    for tile in ((150, 25), (320, 1)):
        lr.assert_rows_equal(eng, lr.text_of(seqs), tile)
    lens = eng.debug_last_packed()[2]
    assert (lens & 0x8000).any() and not (lens & 0x8000).all()


# ------------------------------------------------------------------ 2. edges of the new kernels
def mixed(n_records):
    """n_records records whose lengths cycle through uncut and cut ones (0, 1, 2, 3, 11 and 1 windows at 150,25)"""
    cyc = (100, 150, 151, 176, 0, 400, 37)
    return lr.random_records([cyc[k % len(cyc)] for k in range(n_records)], lr.SEED + n_records)


@pytest.mark.parametrize("n_records", [1023, 1024, 1025, 2049])      # workgroups of 1,024 records: one short of one, one, two, and a third
def test_record_counts_at_the_workgroup_edges(eng, n_records):
    lr.assert_rows_equal(eng, lr.text_of(mixed(n_records)), (150, 25))


@pytest.mark.parametrize("total", [63, 64, 65])      # k_pack_text's groups of 64 reads
def test_window_totals_at_the_pack_group_edges(eng, total):
    seqs = lr.random_records([120] * 30 + [150 + 25 * (total - 60 - 1)] + [90] * 30)      # 60 uncut records and one of total - 60 windows
    assert lr.assert_rows_equal(eng, lr.text_of(seqs), (150, 25)) == total


@pytest.mark.parametrize("where", ["first", "last", "only"])
def test_the_only_cut_record_is_the_first_or_the_last(eng, where):
    short = [100, 150, 1, 0, 149] * 300
    lengths = {"first": [777] + short, "last": short + [777], "only": [777]}[where]
    lr.assert_rows_equal(eng, lr.text_of(lr.random_records(lengths)), (150, 25))


def test_a_chunk_without_a_long_record_takes_the_path_of_the_switch_off(eng):
    text = lr.text_of(lr.random_records([(150, 100, 0, 36, 149)[k % 5] for k in range(3000)]))
    eng.reset_sample()
    eng.set_read_tiling(0, 0)
    assert eng.get_read_tiling() == (0, 0) and eng.submit_fastq(text) == 3000
    off = eng.debug_last_packed()
    assert eng.read_tiling_info() == {"records": 0, "cut": 0, "windows": 0, "longest": 0}
    assert lr.assert_rows_equal(eng, text, (150, 25)) == 3000
    on = eng.debug_last_packed()
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3])) and on[3:] == off[3:]
    assert eng.read_tiling_info() == {"records": 3000, "cut": 0, "windows": 0, "longest": 150}


# ------------------------------------------------------------------ 3. every route gives the same sample
@pytest.fixture(scope="module")
def sample(ref):
    """reads of 400 .. 3,000 bases from a genome with a planted ST; what the text path with tiling off makes of tile_fastq's text"""
    db, idx = ref
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][11], size=100_000)
    text = lr.genome_reads(g, N_READS)
    yard = lr.yardstick(text, (150, 25))
    e = make_engine(ref)
    assert e.get_read_tiling() == (0, 0)
    n = e.submit_fastq(yard)
    want = typed(e)
    assert len(want[1]) == 7 and n == yard.count(b"\n") // 4
    return text, yard, n, want


def test_one_tiled_submission(eng, sample):
    text, yard, n, want = sample
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    assert eng.submit_fastq(text) == n
    assert_typed_equal(typed(eng), want)
    info = eng.read_tiling_info()
    assert info["records"] == N_READS and info["cut"] == N_READS and info["windows"] == n and 400 <= info["longest"] <= 3000


def test_a_stream_cut_inside_a_sequence_line_and_inside_a_quality_line(eng, sample):
    text, yard, n, want = sample
    lines = text.split(b"\n")
    start = np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines[:-1]])])
    cuts = [int(start[4 * 100 + 1]) + 211, int(start[4 * 250 + 3]) + 1, int(start[4 * 250 + 3]) + 390, int(start[4 * 400 + 1]) + len(lines[4 * 400 + 1]) - 1]
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    got, at = 0, 0
    for c in cuts + [len(text)]:
        got += eng.submit_fastq_stream(text[at:c], final=c == len(text))
        at = c
    assert got == n
    assert_typed_equal(typed(eng), want)


def test_the_bgzipped_text(eng, sample):
    text, yard, n, want = sample
    data = lr.bgzip(text)
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    assert eng.submit_fastq_bgzf(data, final=True) == n
    assert_typed_equal(typed(eng), want)
    # in two calls, cut between blocks (in the middle of a record)
    from bam_writer import _bgzf_block
    half = len(b"".join(_bgzf_block(text[i:i + 65280]) for i in range(0, 10 * 65280, 65280)))
    eng.reset_sample()
    assert eng.submit_fastq_bgzf(data[:half], final=False) + eng.submit_fastq_bgzf(data[half:], final=True) == n
    assert_typed_equal(typed(eng), want)


# ------------------------------------------------------------------ 4. rounds
def test_rounds_of_64_windows(ref, sample, monkeypatch):
    text, _, _, _ = sample
    recs = text.split(b"@rec")[1:]
    body, total = [], 0
    for r in recs:      # long reads up to 960 windows at most, then 150-base reads IN FRONT of them up to 1,000: the last round is cut from long reads
        w = lr.fa_windows_of(len(r.split(b"\n")[1]), 150, 25)
        if total + w > 960:
            break
        body.append(b"@rec" + r)
        total += w
    pads = [lr.record(5000 + k, recs[k].split(b"\n")[1][:150]) for k in range(1000 - total)]
    case = b"".join(pads + body)
    yard = lr.yardstick(case, (150, 25))
    names = [r[0] for r in lr.parse(yard)]
    assert len(names) == 1000 and total >= 900 and max(len(r.split(b"\n")[1]) for r in body) > 64 * 25 + 150      # a record of more than 64 windows
    one = make_engine(ref)
    one.set_read_tiling(150, 25)
    assert one.submit_fastq(case) == 1000
    lr.compare_rows(one.debug_last_packed(), lr.host_rows(yard), names)
    want = typed(one)
    monkeypatch.setenv("MLST_TILE_ROUND", "64")
    many = make_engine(ref)
    monkeypatch.delenv("MLST_TILE_ROUND")
    many.set_read_tiling(150, 25)
    assert many.submit_fastq(case) == 1000
    tail = b"".join(b"\n".join((n, s, b"+", q)) + b"\n" for n, s, q in lr.parse(yard)[1000 - 1000 % 64:])
    got = many.debug_last_packed()
    assert got[2].size == 1000 % 64
    lr.compare_rows(got, lr.host_rows(tail), names, first=1000 - 1000 % 64)      # (every round's rows are as wide as the chunk's longest read: 150 here too)
    assert_typed_equal(typed(many), want)
    assert many.read_tiling_info() == one.read_tiling_info()


# ------------------------------------------------------------------ 5. refusals and the unchanged default
def test_setter_refusals_and_the_default(ref):
    from metamlst_amd.engine import Engine, MlstError
    e = Engine(0)
    assert e.get_read_tiling() == (0, 0)      # a fresh engine: off
    for tile, code in (((0, 25), -1), ((150, 0), -1), ((321, 25), -5), ((4000, 1), -5)):
        with pytest.raises(MlstError, match=r"\(%d\)" % code):
            e.set_read_tiling(*tile)
        assert e.get_read_tiling() == (0, 0)
    e.set_read_tiling(320, 1)
    assert e.get_read_tiling() == (320, 1)
    e.set_read_tiling(0, 0)
    assert e.get_read_tiling() == (0, 0)


def test_the_setter_while_a_stream_is_open(eng):
    from metamlst_amd.engine import MlstError
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    assert eng.submit_fastq_stream(b"@r\nACGT\n+\nIIII\n@s\nAC", final=False) == 1
    for tile in ((0, 0), (300, 150)):
        with pytest.raises(MlstError, match="a FASTQ stream is open"):
            eng.set_read_tiling(*tile)
    assert eng.get_read_tiling() == (150, 25)
    eng.reset_sample()
    eng.set_read_tiling(300, 150)
    assert eng.get_read_tiling() == (300, 150)


def test_paired_submissions_are_not_tiled(eng):
    from metamlst_amd.engine import MlstError
    long_rec, short_rec = lr.record(0, b"ACGT" * 80 + b"A"), lr.record(1, b"ACGT" * 30)
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    with pytest.raises(MlstError, match="longer than 320"):
        eng.submit_fastq(long_rec + short_rec, paired=True)
    eng.reset_sample()
    with pytest.raises(MlstError, match="longer than 320"):
        eng.submit_fastq_pair(short_rec, long_rec)
    eng.reset_sample()
    assert eng.submit_fastq(long_rec + short_rec) == 8 + 1      # 321 bases: starts 0 .. 150 and 171
    eng.reset_sample()
    eng.set_read_tiling(0, 0)
    with pytest.raises(MlstError, match="longer than 320"):
        eng.submit_fastq(long_rec + short_rec)
    eng.reset_sample()


def test_a_malformed_record_is_refused_as_before(eng):
    from metamlst_amd.engine import MlstError
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    with pytest.raises(MlstError, match="malformed FASTQ"):
        eng.submit_fastq(b"@a\n" + b"A" * 400 + b"\n+\n" + b"I" * 399 + b"\n")
    with pytest.raises(MlstError, match="malformed FASTQ"):
        eng.submit_fastq(b"a\n" + b"A" * 400 + b"\n+\n" + b"I" * 400 + b"\n")
    eng.reset_sample()


# ------------------------------------------------------------------ 6. the command
def write_sample(d, name, text, how):
    os.makedirs(d, exist_ok=True)
    path = d + "/" + name + {"plain": ".fastq", "gz": ".fastq.gz", "bgzf": ".fastq.gz"}[how]
    if how == "gz":
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(text)
    else:
        open(path, "wb").write(lr.bgzip(text) if how == "bgzf" else text)
    return path


@pytest.fixture(scope="module")
def isolates(ref):
    db, idx = ref
    out = []
    for k, row in enumerate((3, 15)):
        g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][row], size=100_000, seed=200 + k)
        text = lr.genome_reads(g, N_READS, seed=lr.SEED + k)
        out.append((row, text, lr.yardstick(text, (150, 25))))
    return out


def test_the_command_types_long_reads_like_the_tiled_text(ref, isolates, tmp_path, capsys):
    from metamlst_amd.cli import main
    db, idx = ref
    d = str(tmp_path)
    row, text, yard = isolates[0]
    tiled = write_sample(d + "/tiled", "long", yard, "plain")
    assert main(["type", tiled, "-d", db.path, "-o", d + "/out_tiled", "--quiet"]) == 0
    want = open(d + "/out_tiled/long.nfo", "rb").read()
    assert want
    for how in ("plain", "gz", "bgzf"):
        f = write_sample(d + "/" + how, "long", text, how)
        capsys.readouterr()
        assert main(["type", f, "--long-reads", "-d", db.path, "-o", d + "/out_" + how]) == 0
        assert "%s: %d records, %d longer than 150 cut into %d windows" % (f, N_READS, N_READS, yard.count(b"\n") // 4) in capsys.readouterr().out
        assert open(d + "/out_%s/long.nfo" % how, "rb").read() == want, how
    assert main(["merge", d + "/out_plain", "-d", db.path]) == 0
    rep = open(d + "/out_plain/merged/ecoli_report.txt").read().splitlines()
    assert {r.split("\t")[2]: r.split("\t")[0] for r in rep[1:]} == {"long": str(row + 1)}      # the planted ST
    # another tile
    assert main(["type", d + "/plain/long.fastq", "--long-reads", "--tile", "300,150", "-d", db.path, "-o", d + "/out_300", "--quiet"]) == 0
    tiled300 = write_sample(d + "/tiled300", "long", lr.yardstick(text, (300, 150)), "plain")
    assert main(["type", tiled300, "-d", db.path, "-o", d + "/out_tiled300", "--quiet"]) == 0
    assert open(d + "/out_300/long.nfo", "rb").read() == open(d + "/out_tiled300/long.nfo", "rb").read()


def test_a_folder_of_long_read_files_is_typed_like_one_run_per_file(ref, isolates, tmp_path):
    from metamlst_amd.cli import main
    db, idx = ref
    d = str(tmp_path)
    for k, (row, text, yard) in enumerate(isolates):
        write_sample(d + "/in", "iso%d" % k, text, ("plain", "bgzf")[k])
    assert main(["type", d + "/in", "--long-reads", "--quiet", "-d", db.path, "-o", d + "/out_folder"]) == 0
    for f in sorted(glob.glob(d + "/in/iso*")):
        assert main(["type", f, "--long-reads", "--quiet", "-d", db.path, "-o", d + "/out_single"]) == 0
    names = sorted(os.listdir(d + "/out_single"))
    assert names == ["iso0.nfo", "iso1.nfo"] and sorted(os.listdir(d + "/out_folder")) == names
    for n in names:
        assert open(d + "/out_folder/" + n, "rb").read() == open(d + "/out_single/" + n, "rb").read(), n
