"""fastq.tile_fastq -- the host statement of the rule mlst_set_read_tiling applies on the device -- against a restatement of the
rule (tests/long_reads.py::window_starts), and the refusals of `cli type --long-reads`.  No GPU."""
import gzip

import numpy as np
import pytest

import long_reads as lr
from metamlst_amd.fastq import tile_fastq


@pytest.mark.parametrize("tile", lr.TILES)
def test_tile_fastq_equals_the_restated_rule(tile):
    read_len, stride = tile
    lengths = lr.edge_lengths(read_len, stride)
    seqs = lr.random_records(lengths)
    recs = lr.parse(lr.yardstick(lr.text_of(seqs), tile))
    at = 0
    for r, (n, s) in enumerate(zip(lengths, seqs)):
        starts = lr.window_starts(n, read_len, stride)
        assert len(starts) == lr.fa_windows_of(n, read_len, stride), (n, tile)
        q = lr.quals(n, r)
        cover = np.zeros(n, bool)
        for st in starts:
            name, ws, wq = recs[at]
            at += 1
            assert name == (b"@rec%d_%d" % (r, st) if n > read_len else b"@rec%d some comment" % r), (name, r, st)
            assert ws == s[st:st + read_len] and wq == q[st:st + read_len], (r, st)
            assert len(ws) == min(n, read_len)
            cover[st:st + len(ws)] = True
        assert starts[0] == 0 and starts[-1] + min(n, read_len) == n, (n, tile)      # the last window is flush with the end
        assert starts == sorted(set(starts))
        if stride <= read_len:      # (windows every `stride` bases leave gaps when they are shorter than that: 36,100)
            assert cover.all(), (n, tile)
        else:
            assert cover[:min(n, read_len)].all() and cover[max(0, n - read_len):].all()
    assert at == len(recs)


def test_chunks_hold_whole_records_in_order(tmp_path):
    seqs = lr.random_records([400, 10, 151, 150, 0, 700])
    p = str(tmp_path / "a.fastq")
    open(p, "wb").write(lr.text_of(seqs))
    whole = b"".join(tile_fastq(p, 150, 25))
    chunks = list(tile_fastq(p, 150, 25, chunk_reads=5))
    assert len(chunks) > 2 and b"".join(chunks) == whole and all(c.count(b"\n") % 4 == 0 for c in chunks)
    with gzip.open(p + ".gz", "wb") as f:
        f.write(lr.text_of(seqs))
    assert b"".join(tile_fastq(p + ".gz", 150, 25)) == whole
    with pytest.raises(ValueError):
        list(tile_fastq(p, 0, 25))
    with pytest.raises(ValueError):
        list(tile_fastq(p, 150, 0))


def test_crlf_a_quality_line_that_begins_with_at_and_no_final_newline(tmp_path):
    seqs = lr.random_records([7 * 41 + 150, 30, 200])
    lf = lr.yardstick(lr.text_of(seqs), (150, 25))
    assert lr.yardstick(lr.text_of(seqs, b"\r\n"), (150, 25)) == lf
    assert lr.yardstick(lr.text_of(seqs, final_eol=False), (150, 25)) == lf
    assert lr.yardstick(lr.text_of(seqs, b"\r\n", final_eol=False), (150, 25)) == lf
    # a record whose quality line begins with '@': Phred 31 at base 0 is (7 * 0 + r) % 41 = 31, record 31
    many = lr.random_records([200] * 32)
    text = lr.text_of(many)
    q31 = lr.quals(200, 31)
    assert q31[:1] == b"@" and (b"\n+\n" + q31 + b"\n") in text
    recs = lr.parse(lr.yardstick(text, (150, 25)))
    assert len(recs) == 32 * 3
    assert [r for r in recs if r[0].startswith(b"@rec31_")] == [(b"@rec31_%d" % st, many[31][st:st + 150], q31[st:st + 150]) for st in (0, 25, 50)]
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        lr.yardstick(b"@a\nACGT\n+\nIII\n", (150, 25))


def test_bases_are_not_touched(tmp_path):
    s = bytearray(lr.random_records([500])[0])
    s[10:20] = bytes(s[10:20]).lower()
    s[300] = ord("N")
    recs = lr.parse(lr.yardstick(lr.record(0, bytes(s)), (150, 25)))
    assert b"".join(w for _, w, _ in recs[::6])[:450] == bytes(s)[:450]
    assert sum(b"N" in w for _, w, _ in recs) == 6 and len(recs) == 15      # starts 175 .. 300 hold base 300


@pytest.mark.parametrize("extra, said", [(["-2", "MATES"], "it goes with none of -2, --alignments and --contigs"),
                                         (["--alignments"], "it goes with none of -2, --alignments and --contigs"),
                                         (["--contigs"], "it goes with none of -2, --alignments and --contigs"),
                                         (["--tile", "150"], "--tile LEN,STEP takes two positive numbers"),
                                         (["--tile", "0,25"], "--tile LEN,STEP takes two positive numbers"),
                                         (["--tile", "321,25"], "at most 320 bases")])
def test_refusals_of_the_command(tmp_path, capsys, extra, said):
    from metamlst_amd.cli import main
    f = str(tmp_path / "long.fastq")
    open(f, "wb").write(lr.record(0, b"ACGT" * 100))
    extra = [f if x == "MATES" else x for x in extra]
    assert main(["type", f, "--long-reads", "-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "o")] + extra) == 1
    assert said in capsys.readouterr().out


def test_a_bam_is_refused_before_any_engine_is_made(tmp_path, capsys):
    from bam_writer import _bgzf_block
    from metamlst_amd.cli import main
    f = str(tmp_path / "reads.bam")
    open(f, "wb").write(_bgzf_block(b"BAM\x01" + b"\x00" * 8) + _bgzf_block(b""))
    assert main(["type", f, "--long-reads", "-d", str(tmp_path / "no.db"), "-o", str(tmp_path / "o")]) == 1
    assert "--long-reads takes FASTQ" in capsys.readouterr().out
