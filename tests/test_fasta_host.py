"""Host side of the contigs path (CPU): fastq.fasta_chunks cuts a FASTA into whole-contig chunks, cli.expand_samples collects
assemblies, and the crafted file of tests/fasta_zoo.py holds what tests/test_gpu_fasta.py says it holds."""
import gzip
import os

import numpy as np
import pytest

import fasta_zoo as fz
from metamlst_amd.cli import expand_samples
from metamlst_amd.fastq import fasta_chunks, tile_fasta


def windows(texts):
    """the (sequence, quality) lines of FASTQ texts, names left out (tile_fasta numbers contigs per file)"""
    out = []
    for t in texts:
        rec = t.split(b"\n")[:-1]
        out += [(rec[k + 1], rec[k + 3]) for k in range(0, len(rec), 4)]
    return out


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta")
    path = str(d / "zoo.fna")
    fz.zoo(path, 600, one_line_10k=True)
    raw = open(path, "rb").read()
    with gzip.open(path + ".gz", "wb") as f:
        f.write(raw)
    return path, raw


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("chunk_bytes", [1, 1000, 4096, 1 << 20])
def test_chunks_give_back_the_file_and_start_with_headers(fasta, gz, chunk_bytes):
    path, raw = fasta
    chunks = [bytes(c) for c in fasta_chunks(path + (".gz" if gz else ""), chunk_bytes)]
    assert b"".join(chunks) == raw
    assert all(c.startswith(b">") for c in chunks[1:])
    assert len(chunks) > 1 or chunk_bytes >= len(raw)


def test_a_cut_one_byte_over_and_one_byte_under_chunk_bytes(tmp_path):
    """three contigs of 1,000 bytes each, chunk_bytes one byte under, at and one byte over one and two contigs: every cut is in front
    of a header.  The last b"\n>" INSIDE the chunk counts (at 2,000 the '>' of the third contig is the byte behind the chunk, so the
    first chunk is one contig); what is left of the file is one chunk when it fits chunk_bytes; a chunk without a header inside it
    ends in front of the next one."""
    one = b">c\n" + b"A" * 996 + b"\n"
    assert len(one) == 1000
    path = str(tmp_path / "three.fa")
    open(path, "wb").write(one * 3)
    for cb, want in ((1999, [1000, 1000, 1000]), (2000, [1000, 2000]), (2001, [2000, 1000]), (999, [1000, 1000, 1000]), (1000, [1000, 1000, 1000]),
                     (1001, [1000, 1000, 1000])):
        got = [len(c) for c in fasta_chunks(path, cb)]
        assert got == want, (cb, got)
        assert all(bytes(c).startswith(b">") for c in fasta_chunks(path, cb))


def test_a_contig_longer_than_chunk_bytes_arrives_whole(tmp_path):
    path = str(tmp_path / "long.fa")
    body = b">short\nACGT\n>long\n" + b"ACGT" * 5000 + b"\n>after\nGG\n"
    open(path, "wb").write(body)
    chunks = [bytes(c) for c in fasta_chunks(path, 64)]
    assert b"".join(chunks) == body
    assert any(c.startswith(b">long\n") and c.endswith(b"ACGT\n") and len(c) == 20_007 for c in chunks)
    assert chunks[-1] == b">after\nGG\n"


@pytest.mark.parametrize("chunk_bytes", [1000, 5000, 1 << 20])
def test_windows_over_the_chunks_equal_windows_over_the_file(fasta, tmp_path, chunk_bytes):
    path, raw = fasta
    want = windows(tile_fasta(path, 150, 25, 50))
    got = []
    for k, c in enumerate(fasta_chunks(path, chunk_bytes)):
        p = str(tmp_path / ("c%d.fa" % k))
        open(p, "wb").write(bytes(c))
        got += windows(tile_fasta(p, 150, 25, 50))
    assert got == want and len(want) == 600


def test_the_crafted_file_holds_what_it_says(fasta, tmp_path):
    path, raw = fasta
    for n, reads in zip(fz.EDGE_LENS, fz.EDGE_READS):
        p = str(tmp_path / "one.fa")
        open(p, "wb").write(b">x\n" + b"A" * n + b"\n")
        assert fz.count_reads(p) == reads, n
    open(str(tmp_path / "k.fa"), "wb").write(b">x\n" + b"A" * 1000 + b"\n>y\n" + b"C" * 321)
    assert fz.count_reads(str(tmp_path / "k.fa"), 36, 100, 36) == 11 + 4 and fz.count_reads(str(tmp_path / "k.fa"), 320, 1, 50) == 681 + 2
    for total in (63, 64, 65):
        p = str(tmp_path / "z.fa")
        at = fz.zoo(p, total)
        assert fz.count_reads(p) == total
        body = open(p, "rb").read()[at["junk"]:]
        assert body[at["header_at_cell_start"]:][:1] == b">" and at["header_at_cell_start"] % fz.CELL == 0
        assert body[at["lf_at_cell_start"]:][:2] == b"\n>" and at["lf_at_cell_start"] % fz.CELL == 0
        assert body[at["crlf_over_edge"]:][:2] == b"\r\n" and at["crlf_over_edge"] % fz.CELL == fz.CELL - 1
        assert not body.endswith(b"\n") and b"\n>first_of_two\n>second_of_two\n" in body
    assert fz.count_reads(path) == 600 and (b"\n" + raw).count(b"\n>one_line\n") == 1
    assert max(len(l) for l in raw.split(b"\n")) == 10_000


def test_expand_samples_collects_assemblies_in_contigs_mode(tmp_path):
    d = str(tmp_path)
    names = ["b.fna", "a.fa", "c.fasta.gz", "d.fas", "e.fna.gz", "f.fasta", "r.fastq", "s.fq.gz", "notes.txt", "g.fa.bz2"]
    for n in names:
        open(os.path.join(d, n), "wb").close()
    got = expand_samples([d], contigs=True)
    assert got == [[os.path.join(d, n)] for n in ["a.fa", "b.fna", "c.fasta.gz", "d.fas", "e.fna.gz", "f.fasta"]]
    assert expand_samples([d + "/x.fna", d + "/y.fna"], contigs=True) == [[d + "/x.fna"], [d + "/y.fna"]]


def test_expand_samples_without_the_keyword_is_unchanged(tmp_path):
    d = str(tmp_path)
    for n in ["b.fna", "r.fastq", "s.fq.gz", "a.fq.bgz", "notes.txt"]:
        open(os.path.join(d, n), "wb").close()
    assert expand_samples([d]) == [[os.path.join(d, n)] for n in ["a.fq.bgz", "r.fastq", "s.fq.gz"]]
    assert expand_samples([d], contigs=False) == expand_samples([d])
    assert expand_samples(["r1.fq,r2.fq", d + "/b.fna"]) == [["r1.fq", "r2.fq"], [d + "/b.fna"]]
