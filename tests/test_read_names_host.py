"""The host side of `cli type --read-names` (no GPU): samout.read_qname -- the rule csrc/read_names.h applies on the device -- on crafted
header lines, the optional `names` argument of format_record / all_records_rule / write_sam, the way of a named file back through
samin's host reader, and the combinations the command refuses before it makes an engine."""
import os
import re
import struct
import zlib

import pytest

import fixtures as fx
import read_names_cases as rc
from metamlst_amd import cli, samin, samout
from metamlst_amd.typing import TypingArgs
from test_samout_host import hand_made

QNAME = re.compile(rb"[!-?A-~]{1,254}")


@pytest.fixture(scope="module")
def idx():
    return fx.ecoli_small(8)[1]


@pytest.mark.parametrize("header,want", rc.HEADERS, ids=[str(k) for k in range(len(rc.HEADERS))])
def test_read_qname_on_crafted_headers(header, want):
    for eol in (b"", b"\n", b"\r\n"):
        got = samout.read_qname(header + eol, 12345)
        assert got == (want if want is not None else b"r12345"), (header, eol)
        assert QNAME.fullmatch(got)                                          # the file stays valid whatever the input holds


def test_read_qname_edges():
    assert samout.read_qname(b"@" + b"x" * 254 + b" d", 0) == b"x" * 254 and samout.read_qname(b"@" + b"x" * 255 + b" d", 3) == b"r3"
    assert samout.read_qname(b"@name\r", 1) == b"name" and samout.read_qname(b"@name\tb c", 1) == b"name"
    assert samout.read_qname(b"@\r\n", 9) == b"r9" and samout.read_qname(b"@\tx", 9) == b"r9"
    assert samout.read_qname(b"@a b@c", 1) == b"a"                          # an `@` in the description is none in the name
    assert samout.read_qname(bytearray(b"@q/2 z"), 1) == b"q/2"
    # the names fastq.mates_share_names compares are these names
    assert samout.read_qname(b"@p7 1:N:0", 0) == samout.read_qname(b"@p7 2:N:0", 0) != samout.read_qname(b"@p7/2", 0)


def as_recs(idx, rows):
    """the tuples format_record takes from the rows of test_samout_host.hand_made"""
    return [(ri, strand, diag, int(idx.locus_id[a]), a, pos0, AS, XM, [(ln << 4) | op for ln, op in ops], seq, bytes(min(q, 93) for q in ph))
            for ri, a, pos0, strand, diag, AS, XM, ops, seq, ph in rows]


def test_names_none_gives_todays_bytes_and_a_dict_the_named_line(tmp_path, idx):
    chosen, aln, rows = hand_made(idx)
    recs = as_recs(idx, rows)
    names = {0: b"first", 5: b"M01:1:2:3", 7: b"mate/2", 9: b"x" * 254}          # reads 1-4, 6 and 8 have none: they keep r<k>
    for paired in (False, True):
        for r in recs:
            old = samout.format_record(idx, r, paired, False, None)
            assert samout.format_record(idx, r, paired, False, None, None) == samout.format_record(idx, r, paired, False, None, names=None) == old
            new = samout.format_record(idx, r, paired, True, 77, names)
            want_q = names.get(r[0], b"r%d" % (r[0] >> 1 if paired else r[0]))
            assert new.split(b"\t", 1)[0] == want_q
            assert new.split(b"\t", 1)[1] == samout.format_record(idx, r, paired, True, 77).split(b"\t", 1)[1]
        assert samout.all_records_rule(idx, recs, paired, None) == samout.all_records_rule(idx, recs, paired)
        named = samout.all_records_rule(idx, recs, paired, names)
        plain = samout.all_records_rule(idx, recs, paired)
        assert [l.split(b"\t", 1)[1] for l in named] == [l.split(b"\t", 1)[1] for l in plain] and named != plain
        p0, p1, p2 = (str(tmp_path / ("w%d_%d.sam" % (paired, k))) for k in range(3))
        assert samout.write_sam(p0, idx, chosen, aln, paired) == samout.write_sam(p1, idx, chosen, aln, paired, None) == len(aln)
        assert samout.write_sam(p2, idx, chosen, aln, paired, names=names) == len(aln)
        d0, d1, d2 = (open(p, "rb").read() for p in (p0, p1, p2))
        assert d0 == d1 != d2
        l0, l2 = d0.split(b"\n"), d2.split(b"\n")
        assert len(l0) == len(l2)
        order = samout.sam_order(chosen, aln)
        body0, body2 = [l for l in l0 if l and not l.startswith(b"@")], [l for l in l2 if l and not l.startswith(b"@")]
        assert [l for l in l0 if l.startswith(b"@")] == [l for l in l2 if l.startswith(b"@")]
        for k, a, b in zip(order.tolist(), body0, body2):
            ri = int(aln.read_index[k])
            assert a.split(b"\t", 1)[1] == b.split(b"\t", 1)[1]
            assert b.split(b"\t", 1)[0] == names.get(ri, b"r%d" % (ri >> 1 if paired else ri)) and a.split(b"\t", 1)[0] == b"r%d" % (ri >> 1 if paired else ri)


def test_a_named_file_accumulates_like_the_numbered_one(tmp_path, idx):
    chosen, aln, _ = hand_made(idx)
    # every read its own name (mates 6 / 7 and 8 / 9 share one, as the product submits pairs only then)
    names = {ri: b"HWI:%d:x" % (ri >> 1) for ri in set(int(r) for r in aln.read_index)}
    p0, p1 = str(tmp_path / "num.sam"), str(tmp_path / "named.sam")
    samout.write_sam(p0, idx, chosen, aln, True)
    samout.write_sam(p1, idx, chosen, aln, True, names=names)
    s0 = samin.AlignmentSample(idx, TypingArgs()).add_file(p0).stats()
    s1 = samin.AlignmentSample(idx, TypingArgs()).add_file(p1).stats()
    fx.assert_stats_equal(s1, s0)
    assert int(s0.n_hits.sum()) > 0


def tiny_bam(path):
    """a BGZF BAM without references or records"""
    data = b"BAM\x01" + struct.pack("<ii", 0, 0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    block = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(data), len(data))
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    open(path, "wb").write(block + eof)
    return str(path)


def test_cli_refuses_before_an_engine_is_made(tmp_path, monkeypatch, capsys):
    def no_engine(*a, **k):
        raise AssertionError("an engine was made")
    monkeypatch.setattr(cli, "Engine", no_engine)
    fq = tmp_path / "s.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    fq2 = tmp_path / "t.fastq"
    fq2.write_bytes(b"@a\nACGT\n+\nIIII\n")
    fa = tmp_path / "c.fa"
    fa.write_bytes(b">c\nACGT\n")
    sam = tmp_path / "in.sam"
    sam.write_bytes(b"@HD\tVN:1.6\n")
    folder = tmp_path / "many"
    os.mkdir(folder)
    (folder / "a.fastq").write_bytes(fq.read_bytes())
    (folder / "b.fastq").write_bytes(fq.read_bytes())
    bam = tiny_bam(tmp_path / "reads.bam")
    assert samin.is_bgzf_bam(bam)
    tail = ["-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "out"), "--read-names"]
    cases = [
        ([str(fq)], "--write-sam or --write-sam-all"),                                       # no export to name
        ([bam, "--write-sam"], "reads BAM"),
        ([str(fa), "--contigs", "--write-sam-all"], "--contigs"),
        ([str(fq), "--long-reads", "--write-sam"], "--long-reads"),
        ([bam, "--long-bam-reads", "--write-sam"], "--long-bam-reads"),
        ([str(sam), "--alignments", "--write-sam"], "--alignments"),
        ([str(sam), "--alignments"], "--alignments"),
        ([str(folder), "--write-sam-all"], "several samples or a folder"),
        ([str(fq), str(fq2), "--write-sam"], "several samples or a folder"),
        ([str(fq), "--gpus", "2", "--write-sam-all"], "--gpus N"),
    ]
    for args, reason in cases:
        assert cli.main(["type"] + args + tail) != 0, args
        out = capsys.readouterr().out
        assert out.startswith("--read-names: ") and reason in out, (args, out)
    assert not os.path.exists(tmp_path / "out")
    # without the flag, and with the flag on a command line it goes with, the command gets past these checks: to the database, which is not there
    for extra in ([], ["--read-names"]):
        assert cli.main(["type", str(fq), "--write-sam"] + tail[:-1] + extra) == 1
        assert capsys.readouterr().out.startswith("Failed to connect to the database")
