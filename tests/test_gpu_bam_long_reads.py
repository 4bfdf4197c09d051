"""BAM reads longer than the tile cut into windows on the device (mlst_set_read_tiling on an unpaired reads stream, csrc/bam_tile.h)
against the yardstick of tests/bam_long_reads.py -- samin.bam_reads_fastq, then fastq.tile_fastq, then the FASTQ text path with
tiling off: the same packed rows byte for byte, and by every feed the same statistics, read indices, chosen alleles and consensus
letters; the refusals that stay; the command.  The builders' own figures: tests/test_bam_long_reads_host.py."""
import os

import numpy as np
import pytest

import bam_long_reads as bl
import bam_reads_zoo as bz
import fixtures as fx
import long_reads as lr
from metamlst_amd import synth

pytestmark = pytest.mark.gpu

N_READS = 1800      # the sample of tests/test_gpu_long_reads.py: reads of 400 .. 3,000 bases over 100,000


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
def test_rows_of_every_edge_length(eng, tmp_path, tile):
    lengths = [n for n in lr.edge_lengths(*tile) if n] + [321]      # 32,768 and 100,003 bases: lengths 16 bits with two flags cannot hold
    path = bl.write(tmp_path / "e.bam", bl.records(lengths))
    assert bl.assert_rows_equal(eng, path, tile) == sum(lr.fa_windows_of(n, *tile) for n in lengths)


def test_rows_at_every_nibble_parity(eng, tmp_path):
    """starts 0, 25, 50 ... are even and odd, lengths 1,000 and 1,001, both strands: every combination of start parity, length parity
    (the filler nibble) and strand"""
    path = bl.write(tmp_path / "p.bam", bl.records([1000, 1000, 1001, 1001], skip_every=0))
    flags, lseqs = bz.layout(path)[2:]
    assert [(int(f) & 16, int(n)) for f, n in zip(flags, lseqs)] == [(0, 1000), (16, 1000), (0, 1001), (16, 1001)]
    assert bl.assert_rows_equal(eng, path, (150, 25)) == 2 * 35 + 2 * 36


def test_rows_of_reads_without_qualities(eng, tmp_path):
    seqs = lr.random_records([900, 900, 100])
    path = bl.write(tmp_path / "q.bam", [bl.kept(0, seqs[0], False, qual="*"), bl.kept(1, seqs[1], True, qual="*"), bl.kept(2, seqs[2], True)])
    assert bl.assert_rows_equal(eng, path, (150, 25)) == 31 + 31 + 1
    qrows = eng.debug_last_packed()[1]
    assert (qrows[:62, :150] == 1).all() and not (qrows[62, :100] == 1).all()      # Phred 1 at every base of every window


def test_rows_with_non_acgt_nibbles_at_window_and_filler_edges(eng, tmp_path):
    rng = np.random.default_rng(lr.SEED + 3)
    recs = []
    for r, n in enumerate((1000, 1001, 1001, 1000)):
        s = bytearray(lr.bases(rng, n))
        for at, ch in ((0, "N"), (25, "R"), (149, "="), (150, "Y"), (174, "N"), (175, "K"), (n - 151, "="), (n - 150, "N"), (n - 2, "M"), (n - 1, "N")):
            s[at] = ord(ch)      # window starts and ends, the read's first base and its last (next to the filler nibble of an odd l_seq)
        q = lr.quals(n, r).decode("latin1")
        recs.append(bz.reverse_mapped("n%d" % r, bytes(s).decode(), q) if r >= 2 else bz.unmapped("n%d" % r, bytes(s).decode(), q))
    path = bl.write(tmp_path / "n.bam", recs)
    bl.assert_rows_equal(eng, path, (150, 25))
    lens = eng.debug_last_packed()[2]
    per = [35, 36, 36, 35]
    at = 0
    for w in per:      # starts 200 .. n - 325 hold none of them: bit 15 clear there, set in the windows over the edges
        flags = (lens[at:at + w] & 0x8000) != 0
        assert flags[:7].all() and flags[-7:].all() and not flags[8:w - 13].any(), flags
        at += w


@pytest.mark.parametrize("total", [63, 64, 65])      # k_bamr_pack's groups of 64 rows
def test_window_totals_at_the_pack_group_edges(eng, tmp_path, total):
    path = bl.write(tmp_path / "g.bam", bl.records([120] * 30 + [150 + 25 * (total - 60 - 1)] + [90] * 30))
    assert bl.assert_rows_equal(eng, path, (150, 25)) == total


@pytest.mark.parametrize("n_kept", [1023, 1024, 1025, 2049])      # k_bamt_count's workgroups of 1,024 kept reads
def test_kept_read_counts_at_the_workgroup_edges(eng, tmp_path, n_kept):
    cyc = (100, 150, 151, 176, 400, 37)      # 1, 1, 2, 3, 11 and 1 windows at 150,25
    path = bl.write(tmp_path / "k.bam", bl.records([cyc[k % len(cyc)] for k in range(n_kept)], lr.SEED + n_kept, skip_every=7))
    bl.assert_rows_equal(eng, path, (150, 25))


@pytest.mark.parametrize("where", ["first", "last", "only"])
def test_the_only_long_read_is_the_first_or_the_last(eng, tmp_path, where):
    short = [100, 150, 1, 149] * 300
    lengths = {"first": [777] + short, "last": short + [777], "only": [777]}[where]
    bl.assert_rows_equal(eng, bl.write(tmp_path / "o.bam", bl.records(lengths, skip_every=11)), (150, 25))


def test_rows_of_the_longest_read_a_record_holds(eng, tmp_path):
    seq = lr.random_records([bl.LONGEST])[0]
    path = bl.write(tmp_path / "big.bam", [bz.skipped("empty", 0), bz.reverse_mapped("r69", seq.decode(), lr.quals(bl.LONGEST, 0).decode("latin1"))])
    starts, end = bz.layout(path)[:2]
    assert end - int(starts[1]) == 1_047_044
    assert bl.assert_rows_equal(eng, path, (150, 150), how="call") == (bl.LONGEST - 150) // 150 + 1 + 1


@pytest.fixture(scope="module")
def spanning(tmp_path_factory):
    """a 100,003-base read on the reverse strand (150 KB: three BGZF blocks, five cells) behind a short read and a skipped record, and
    reads of both kinds behind it"""
    lengths = [120, 100_003, 200, 400, 150, 151]
    recs = bl.records(lengths, lr.SEED + 9, skip_every=2)
    path = bl.write(tmp_path_factory.mktemp("span") / "span.bam", recs)
    assert len(bz.bgzf_blocks(open(path, "rb").read())) == 4      # (three with data and the EOF block; the header shares the first)
    return path


@pytest.mark.parametrize("how", ["call", "blocks", "cut", "serial"])
def test_a_read_that_spans_blocks_and_cells_by_every_feed(eng, ref, spanning, how, monkeypatch):
    e = eng
    if how == "serial":      # (the switch is read once per handle)
        monkeypatch.setenv("MLST_BGZF_PIPE", "0")
        e = make_engine(ref)
    want = sum(lr.fa_windows_of(n, 150, 25) for n in [120, 100_003, 200, 400, 150, 151])
    assert bl.assert_rows_equal(e, spanning, (150, 25), how="blocks" if how == "serial" else how) == want


# ------------------------------------------------------------------ 2. no long read: the path of the switch off
def test_a_file_without_a_long_read_takes_the_path_of_the_switch_off(eng, tmp_path):
    path = bz.write(tmp_path / "z.bam", bz.zoo(500))      # reads of 1 .. 320 bases
    eng.reset_sample()
    eng.set_read_tiling(0, 0)
    assert eng.submit_bam_reads_file(path) == 500
    off, off_info, off_stats = eng.debug_last_packed(), eng.bam_reads_info(), eng.stats()
    assert eng.read_tiling_info() == {"records": 0, "cut": 0, "windows": 0, "longest": 0}
    eng.reset_sample()
    eng.set_read_tiling(320, 1)
    assert eng.submit_bam_reads_file(path) == 500
    on = eng.debug_last_packed()
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3])) and on[3:] == off[3:]
    assert eng.bam_reads_info() == off_info
    fx.assert_stats_equal(eng.stats(), off_stats)
    assert int(eng.stats().counters[2]) == int(off_stats.counters[2]) == 500
    assert eng.read_tiling_info() == {"records": 500, "cut": 0, "windows": 0, "longest": 320}
    eng.set_read_tiling(0, 0)


# ------------------------------------------------------------------ 3. typing: every feed gives the sample of the yardstick
@pytest.fixture(scope="module")
def sample(ref, tmp_path_factory):
    """the long-read sample with a planted ST as a BAM (every other read reverse-mapped); what the text path with tiling off makes of
    the yardstick text"""
    db, idx = ref
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][11], size=100_000)
    path = bl.write(tmp_path_factory.mktemp("sample") / "s.bam", bl.from_fastq(lr.genome_reads(g, N_READS)))
    back, yard = bl.yardstick(path, (150, 25))
    e = make_engine(ref)
    assert e.get_read_tiling() == (0, 0)
    n = e.submit_fastq(yard)
    want = typed(e)
    assert len(want[1]) == 7 and n == yard.count(b"\n") // 4 == 114_284
    return path, back, yard, n, want


@pytest.mark.parametrize("how", ["file", "blocks", "cut"])
def test_typing_equals_the_text_path_on_the_yardstick(eng, sample, how):
    path, back, yard, n, want = sample
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    n_reads, n_records = bl.feed(eng, path, how)
    assert n_reads == n and n_records in (None, N_READS)
    assert_typed_equal(typed(eng), want)
    info = eng.read_tiling_info()
    assert info["records"] == N_READS and info["cut"] == N_READS and info["windows"] == n and 400 <= info["longest"] <= 3000


def test_typing_equals_the_tiled_fastq_path(eng, sample):
    path, back, yard, n, want = sample
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    assert eng.submit_fastq(back) == n
    fq = typed(eng)
    assert_typed_equal(fq, want)
    eng.reset_sample()
    assert eng.submit_bam_reads_file(path) == n
    assert_typed_equal(typed(eng), fq)


# ------------------------------------------------------------------ 4. rounds
def test_rounds_of_64_windows(ref, sample, tmp_path, monkeypatch):
    recs = lr.parse(sample[1])
    body, total = [], 0
    for name, s, q in recs:      # long reads up to 960 windows at most, then 150-base reads IN FRONT of them up to 1,000: the last round is cut from long reads
        w = lr.fa_windows_of(len(s), 150, 25)
        if total + w > 960:
            break
        body.append((s, q))
        total += w
    pads = [(recs[k][1][:150], recs[k][2][:150]) for k in range(1000 - total)]
    case = b"".join(b"@c%d\n%s\n+\n%s\n" % (k, s, q) for k, (s, q) in enumerate(pads + body))
    path = bl.write(tmp_path / "rounds.bam", bl.from_fastq(case))
    yard = bl.yardstick(path, (150, 25))[1]
    names = [r[0] for r in lr.parse(yard)]
    assert len(names) == 1000 and total >= 900 and max(len(s) for s, _ in body) > 64 * 25 + 150      # a read of more than 64 windows
    one = make_engine(ref)
    one.set_read_tiling(150, 25)
    assert one.submit_bam_reads_file(path) == 1000
    lr.compare_rows(one.debug_last_packed(), lr.host_rows(yard), names)
    want = typed(one)
    monkeypatch.setenv("MLST_TILE_ROUND", "64")
    many = make_engine(ref)
    monkeypatch.delenv("MLST_TILE_ROUND")
    many.set_read_tiling(150, 25)
    assert many.submit_bam_reads_file(path) == 1000
    got = many.debug_last_packed()
    assert got[2].size == 1000 % 64
    lr.compare_rows(got, lr.host_rows(bl.tail_text(yard, 1000 % 64)), names, first=1000 - 1000 % 64)      # (every round's rows are as wide as the tile)
    assert_typed_equal(typed(many), want)
    assert many.read_tiling_info() == one.read_tiling_info()
    assert many.bam_reads_info()[:3] == one.bam_reads_info()[:3] == (1000, 0, 0)


# ------------------------------------------------------------------ 5. the refusals that stay
def test_unchanged_refusals(eng, tmp_path):
    from metamlst_amd.engine import MlstError
    from metamlst_amd import samin
    seqs = lr.random_records([100, 321, 80, 321])
    r321 = bl.write(tmp_path / "r321.bam", [bl.kept(0, seqs[0], False), bl.kept(1, seqs[1], True)])
    eng.reset_sample()
    eng.set_read_tiling(0, 0)
    with pytest.raises(MlstError, match=r"\(-5\).*a BAM read is longer than 320 bases"):      # the switch off
        eng.submit_bam_reads_file(r321)
    pair = bl.write(tmp_path / "pair.bam", [bz.unmapped("p0", seqs[2].decode(), "I" * 80, flag=77), bz.unmapped("p0", seqs[3].decode(), "I" * 321, flag=141)])
    eng.reset_sample()
    eng.set_read_tiling(150, 25)
    with pytest.raises(MlstError, match=r"\(-5\).*a BAM read is longer than 320 bases"):      # a paired stream, whatever the switch
        eng.submit_bam_reads_file(pair, paired=True)
    eng.reset_sample()
    assert eng.submit_bam_reads_file(r321) == 1 + 8      # (the handle is usable, and the same file is typed with the switch on)
    big = lr.random_records([700_000])[0]
    over = bl.write(tmp_path / "over.bam", [bz.unmapped("r700000", big.decode(), "I" * 700_000)])
    eng.reset_sample()
    with pytest.raises(MlstError, match=r"\(-5\).*a BAM record of more than \d+ bytes"):
        eng.submit_bam_reads_file(over)
    eng.reset_sample()
    names, lo, skip = samin.read_bam_header(r321)
    eng.bam_reads_open(len(names), skip)
    for tile in ((0, 0), (300, 150)):
        with pytest.raises(MlstError, match="a FASTQ stream is open"):
            eng.set_read_tiling(*tile)
    assert eng.get_read_tiling() == (150, 25)
    eng.reset_sample()
    eng.set_read_tiling(0, 0)


# ------------------------------------------------------------------ 6. the command
def test_the_command(ref, sample, tmp_path, capsys):
    import shutil
    from metamlst_amd.cli import main
    db, idx = ref
    path, back, yard, n, want = sample
    d = str(tmp_path)
    for k in ("d1", "d2", "two"):
        os.mkdir(d + "/" + k)
    shutil.copy(path, d + "/d1/s.bam")
    open(d + "/d2/s.fastq", "wb").write(back)
    assert main(["type", d + "/d1/s.bam", "--long-bam-reads", "-d", db.path, "-o", d + "/out1"]) == 0
    said = capsys.readouterr().out
    assert "s.bam: %d reads taken, 0 secondary / supplementary and 0 empty records skipped, %d longer than 150 cut into %d windows" % (n, N_READS, n) in said
    assert main(["type", d + "/d2/s.fastq", "--long-reads", "--quiet", "-d", db.path, "-o", d + "/out2"]) == 0
    nfo = open(d + "/out1/s.nfo", "rb").read()
    assert nfo and nfo == open(d + "/out2/s.nfo", "rb").read()
    # two BAMs in one command: one sample each, as one run each
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][15], size=100_000, seed=201)
    other = bl.write(d + "/two/t.bam", bl.from_fastq(lr.genome_reads(g, N_READS, seed=lr.SEED + 1)))
    assert main(["type", d + "/d1/s.bam", other, "--long-bam-reads", "--tile", "300,150", "-d", db.path, "-o", d + "/out_two"]) == 0
    said = capsys.readouterr().out
    assert "s.bam: " in said and "t.bam: " in said and said.count(" longer than 300 cut into ") == 2
    for f in (d + "/d1/s.bam", other):
        assert main(["type", f, "--long-bam-reads", "--tile", "300,150", "--quiet", "-d", db.path, "-o", d + "/out_single"]) == 0
    assert sorted(os.listdir(d + "/out_two")) == sorted(os.listdir(d + "/out_single")) == ["s.nfo", "t.nfo"]
    for name in ("s.nfo", "t.nfo"):
        assert open(d + "/out_two/" + name, "rb").read() == open(d + "/out_single/" + name, "rb").read(), name
