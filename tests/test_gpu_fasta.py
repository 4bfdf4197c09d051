"""Contigs tiled into reads on the device (mlst_submit_fasta, csrc/fasta_dev.h) against the text fastq.tile_fasta writes followed by
the FASTQ text path: the same packed rows, statistics, chosen alleles and consensus letters; the refusals, the host fallback of the
command and a folder of assemblies.  The crafted input is tests/fasta_zoo.py (its figures: tests/test_fasta_host.py).  The
10,000-base contig on one line alone gives 395 reads at 150,25: it is in the file of ~6,000 reads, not in those of 63 to 65."""
import glob
import gzip
import os

import numpy as np
import pytest

import fasta_zoo as fz
import fixtures as fx
from fasta_edges import assert_rows_equal
from metamlst_amd import synth
from metamlst_amd.fastq import fasta_chunks, tile_fasta

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


def typed(eng):
    st = eng.stats()
    eng.typing_enqueue()
    _, chosen, letters = eng.typing_fetch()
    return st, chosen, letters


# ------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("total", [63, 64, 65, 6000])
def test_packed_rows_equal_the_host_pack_of_the_yardstick_text(eng, tmp_path, total):
    path = str(tmp_path / "zoo.fna")
    fz.zoo(path, total, one_line_10k=total > 1000)
    assert_rows_equal(eng, path, (150, 25, 50), total)


@pytest.mark.parametrize("tile", [(320, 1, 50), (36, 100, 36), (150, 25, 151)])
def test_packed_rows_at_other_tiles(eng, tmp_path, tile):
    path = str(tmp_path / "zoo.fna")
    fz.zoo(path, 65)
    assert_rows_equal(eng, path, tile)


# ------------------------------------------------------------------ 2. statistics
@pytest.fixture(scope="module")
def genome(ref, tmp_path_factory):
    """a 200,000-base genome in three contigs (one reverse-complemented), 70-column lines; what the text path makes of it"""
    db, idx = ref
    d = tmp_path_factory.mktemp("asm")
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][11], size=200_000)
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    parts = [g[:70_000].tobytes(), comp[g[70_000:140_000]][::-1].tobytes(), g[140_000:].tobytes()]
    path = str(d / "asm12.fna")
    with open(path, "wb") as f:
        for k, s in enumerate(parts):
            f.write(b">contig%d\n" % k + b"".join(s[i:i + 70] + b"\n" for i in range(0, len(s), 70)))
    e = make_engine(ref)
    n = sum(e.submit_fastq(c) for c in tile_fasta(path, 150, 25, 50, chunk_reads=3000))
    want = typed(e)
    assert len(want[1]) == 7
    return path, n, want


@pytest.mark.parametrize("per_contig", [False, True])
def test_statistics_choice_and_consensus_equal_the_text_path(eng, genome, per_contig):
    path, n, want = genome
    eng.reset_sample()
    if per_contig:
        chunks = [bytes(c) for c in fasta_chunks(path, 1000)]
        assert len(chunks) == 3
        got = [eng.submit_fasta(c) for c in chunks]
        assert [c for c, _ in got] == [1, 1, 1] and sum(r for _, r in got) == n
    else:
        assert eng.submit_fasta_file(path) == (3, n)
    st, chosen, letters = typed(eng)
    fx.assert_stats_equal(st, want[0])
    assert int(st.counters[2]) == n
    assert chosen == want[1]
    assert letters.keys() == want[2].keys() and all(bytes(letters[a]) == bytes(want[2][a]) for a in letters)


# ------------------------------------------------------------------ 3. refusals and fallback
def test_parameter_refusals(eng, ref):
    from metamlst_amd.engine import Engine, MlstError
    text = b">c\n" + b"ACGT" * 100 + b"\n"
    eng.reset_sample()
    for tile, code in (((0, 25, 50), -1), ((150, 0, 50), -1), ((150, 25, 0), -1), ((321, 25, 50), -5)):
        with pytest.raises(MlstError, match=r"\(%d\)" % code):
            eng.submit_fasta(text, *tile)
    with pytest.raises(MlstError, match="no reference loaded"):
        Engine(0).submit_fasta(text)
    assert int(eng.stats().counters[2]) == 0
    assert eng.submit_fasta(b"no header\nACGT\n") == (0, 0) and eng.submit_fasta(b">c\nACGT\n") == (1, 0) and eng.submit_fasta(b"") == (0, 0)
    assert eng.submit_fasta(text, 320, 1, 1) == (1, 81)


def test_an_open_fastq_stream_refuses_the_entry(eng):
    from metamlst_amd.engine import MlstError
    eng.reset_sample()
    assert eng.submit_fastq_stream(b"@r\nACGT\n+\nIIII\n@s\nAC", final=False) == 1
    with pytest.raises(MlstError, match="a FASTQ stream is open"):
        eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n")
    eng.reset_sample()
    assert eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n") == (1, 11)


BAD = {"tab_at_line_end": (b"ACGTACGTAC\t\n", b"ACGTACGTAC\n"), "space_inside": (b"ACGTA CGTAC\n", b"ACGTACGTAC\n"), "lone_cr": (b"ACGTA\rCGTAC\n", b"ACGTACGTAC\n")}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_line_only_strip_treats_goes_to_the_host(eng, ref, genome, tmp_path, capfd, kind):
    from metamlst_amd.cli import main
    from metamlst_amd.engine import HostPathNeeded
    db, idx = ref
    raw = open(genome[0], "rb").read()
    lines = raw.split(b"\n")
    at = sum(len(l) + 1 for l in lines[:1500])      # a line of the second contig, far behind the first cell
    assert lines[1500][:1] != b">" and len(lines[1500]) == 70
    bad, clean = BAD[kind]
    d = str(tmp_path)
    for name, ins in (("bad", bad), ("clean", clean)):
        os.mkdir(d + "/" + name)
        with open(d + "/%s/asm.fna" % name, "wb") as f:
            f.write(raw[:at] + ins + raw[at:])
    if kind == "tab_at_line_end":      # (tile_fasta strips it: the two files hold the same windows; inside a line it would be a base)
        assert b"".join(tile_fasta(d + "/bad/asm.fna")) == b"".join(tile_fasta(d + "/clean/asm.fna"))
    eng.reset_sample()
    with pytest.raises(HostPathNeeded, match="at byte %d" % (at + bad.index(b"\r" if kind == "lone_cr" else b"\t" if kind == "tab_at_line_end" else b" "))):
        eng.submit_fasta(open(d + "/bad/asm.fna", "rb").read())
    st = eng.stats()
    assert int(st.counters[2]) == 0 and int(st.n_hits.sum()) == 0
    assert eng.submit_fasta(open(d + "/clean/asm.fna", "rb").read())[0] == 3      # the handle is usable afterwards
    capfd.readouterr()
    assert main(["type", d + "/bad/asm.fna", "--contigs", "-d", db.path, "-o", d + "/out_bad", "--quiet"]) == 0
    err = capfd.readouterr().err
    assert "host path needed" in err and "reading the file on the host instead" in err
    assert main(["type", d + "/clean/asm.fna", "--contigs", "-d", db.path, "-o", d + "/out_clean", "--quiet"]) == 0
    assert "host path" not in capfd.readouterr().err
    assert open(d + "/out_bad/asm.nfo").read() == open(d + "/out_clean/asm.nfo").read()


# ------------------------------------------------------------------ 4. a folder of assemblies
def test_a_folder_of_assemblies_is_typed_like_one_run_per_file(ref, tmp_path):
    from metamlst_amd.cli import main
    db, idx = ref
    d = str(tmp_path)
    os.mkdir(d + "/asm")
    sts = [3, 7, 11, 15, 19]
    for k, row in enumerate(sts):
        g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][row], size=120_000, seed=100 + k)
        s = g.tobytes()
        body = b">a\n" + b"".join(s[i:i + 80] + b"\n" for i in range(0, 60_000, 80)) + b">b\n" + s[60_000:] + b"\n"
        name = d + "/asm/iso%d.%s" % (k, ("fa", "fna", "fasta", "fas", "fna.gz")[k])
        with (gzip.open if name.endswith(".gz") else open)(name, "wb") as f:
            f.write(body)
    open(d + "/asm/reads.fastq", "wb").write(b"@r\nACGT\n+\nIIII\n")      # not an assembly: left alone
    assert main(["type", d + "/asm", "--contigs", "-d", db.path, "-o", d + "/out_folder", "--quiet"]) == 0
    for f in sorted(glob.glob(d + "/asm/iso*")):
        assert main(["type", f, "--contigs", "-d", db.path, "-o", d + "/out_single", "--quiet"]) == 0
    names = sorted(os.listdir(d + "/out_single"))
    assert names == ["iso%d.nfo" % k for k in range(5)] and sorted(os.listdir(d + "/out_folder")) == names
    for n in names:
        assert open(d + "/out_folder/" + n, "rb").read() == open(d + "/out_single/" + n, "rb").read(), n
    assert main(["merge", d + "/out_folder", "-d", db.path]) == 0
    rep = open(d + "/out_folder/merged/ecoli_report.txt").read().splitlines()
    called = {r.split("\t")[2]: r.split("\t")[0] for r in rep[1:]}
    assert called == {"iso%d" % k: str(row + 1) for k, row in enumerate(sts)}


def test_refusals_of_the_command(ref, tmp_path, capsys):
    from metamlst_amd.cli import main
    db, idx = ref
    f = str(tmp_path / "a.fna")
    open(f, "wb").write(b">c\nACGT\n")
    for extra, said in ((["-2", f], "neither -2 nor --alignments"), (["--alignments"], "neither -2 nor --alignments"), (["--tile", "150"], "--tile LEN,STEP"),
                        (["--tile", "a,b"], "--tile LEN,STEP"), (["--gpus", "2"], "--gpus applies to FASTQ input")):
        assert main(["type", f, "--contigs", "-d", db.path, "-o", str(tmp_path / "o")] + extra) == 1
        assert said in capsys.readouterr().out
