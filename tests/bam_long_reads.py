"""Builders for BAM reads longer than a packed read -- TEST INFRASTRUCTURE (no GPU; used by tests/test_bam_long_reads_host.py and
tests/test_gpu_bam_long_reads.py).

The yardstick of every device test, stated once (yardstick): samin.bam_reads_fastq -- the reads `samtools fastq` would write --
followed by fastq.tile_fastq, the rule of mlst_set_read_tiling as include/mlst.h states it; the FASTQ text path with tiling off
takes it from there (long_reads.host_rows for rows, submit_fastq for typing).  Records come from bam_reads_zoo.unmapped /
reverse_mapped / skipped with long_reads.bases / quals: the Phred value of base i of read r is (7 i + r) % 41, so a window that
carries the wrong slice of QUAL -- or the right slice of the wrong strand -- cannot pass."""
import bam_reads_zoo as bz
import long_reads as lr
from metamlst_amd import samin

LONGEST = 698_000      # bases of the longest read tried: with a 7-letter name a record of 1,047,044 bytes, under BAM_REC_MAX (2^20 - 64)


def kept(r, seq, rev, qual=None, flag=None):
    """read r (bytes of bases) as a kept record: unmapped, or -- rev -- mapped to the reverse strand (SEQ holds its reverse
    complement, QUAL is reversed); qual: None = long_reads.quals(n, r), "*" = no qualities"""
    q = lr.quals(len(seq), r).decode("latin1") if qual is None else qual
    make = bz.reverse_mapped if rev else bz.unmapped
    return make("r%d" % r, seq.decode(), q) if flag is None else make("r%d" % r, seq.decode(), q, flag=flag)


def records(lengths, seed=lr.SEED, skip_every=3, first_rev=False):
    """kept reads of the given lengths, alternating unmapped / reverse-mapped, a skipped record (secondary, supplementary, empty in
    turn) in front of every skip_every-th of them and one at the very end"""
    out = []
    for r, seq in enumerate(lr.random_records(lengths, seed)):
        if skip_every and r % skip_every == 0:
            out.append(bz.skipped(("secondary", "supplementary", "empty")[(r // skip_every) % 3], r))
        out.append(kept(r, seq, bool(r % 2) != first_rev))
    if skip_every:
        out.append(bz.skipped("supplementary", 999999))
    return out


def from_fastq(text):
    """the records of FASTQ text (long_reads.text_of / genome_reads) as BAM records with the text's own quality lines, every other
    read reverse-mapped"""
    return [(bz.reverse_mapped if r % 2 else bz.unmapped)("r%d" % r, s.decode(), q.decode("latin1")) for r, (_, s, q) in enumerate(lr.parse(text))]


def write(path, recs):
    return bz.write(path, recs)


def reads_text(path, counts=None):
    """the reads of the BAM as FASTQ text, by the host statement of the rules"""
    return b"".join(samin.bam_reads_fastq(str(path), counts=counts))


def yardstick(path, tile, counts=None):
    """THE yardstick: (the reads `samtools fastq` would write, the text tile_fastq makes of them)"""
    text = reads_text(path, counts)
    return text, lr.yardstick(text, tile)


def tail_text(yard, k):
    """the last k records of yardstick text, as text"""
    recs = lr.parse(yard)
    return b"".join(b"\n".join((n, s, b"+", q)) + b"\n" for n, s, q in recs[len(recs) - k:])


def feed(eng, path, how="file"):
    """the records' blocks of a BAM into a reads stream (the stream's tiling is the engine's): "file" = submit_bam_reads_file; "call" =
    one call with all blocks; "blocks" = one BGZF block per call; "cut" = a buffer that ends inside a block, then the rest.
    -> (reads submitted, records counted by the calls: None for "file")"""
    if how == "file":
        return eng.submit_bam_reads_file(str(path)), None
    names, lo, skip = samin.read_bam_header(str(path))
    raw = open(str(path), "rb").read()[lo:]
    eng.bam_reads_open(len(names), skip, False)
    blocks, n = bz.bgzf_blocks(raw), 0
    if how == "call":
        n = eng.submit_bam_bgzf(raw, final=True)[0]
    elif how == "blocks":
        for k, (at, size) in enumerate(blocks):
            n += eng.submit_bam_bgzf(raw[at:at + size], final=k + 1 == len(blocks))[0]
    else:
        mid = blocks[len(blocks) // 2]
        n1, used = eng.submit_bam_bgzf(raw[:mid[0] + mid[1] // 2], final=False, partial=True)
        assert used == mid[0]
        n = n1 + eng.submit_bam_bgzf(raw[used:], final=True)[0]
    return eng.bam_reads_info()[0], n


def assert_rows_equal(eng, path, tile, how="file", n_want=None):
    """One tiled reads stream over the file against the yardstick: the read count, counters[2], bam_reads_info, read_tiling_info and
    the packed rows of the LAST submission word for word (a file of one piece: all its rows; else the yardstick's last rows).
    Returns the number of reads."""
    counts = {}
    text, yard = yardstick(path, tile, counts)
    recs = lr.parse(yard)
    src = [len(s) for _, s, _ in lr.parse(text)]
    eng.reset_sample()
    eng.set_read_tiling(*tile)
    n_reads, n_records = feed(eng, path, how)
    assert n_reads == len(recs) and (n_want is None or n_reads == n_want), (n_reads, len(recs), n_want)
    assert int(eng.stats().counters[2]) == n_reads
    assert eng.bam_reads_info()[:3] == (n_reads, counts["secondary"], counts["empty"])
    assert n_records is None or n_records == len(src) + counts["secondary"] + counts["empty"], (n_records, len(src), counts)
    cut = [n for n in src if n > tile[0]]
    assert eng.read_tiling_info() == {"records": len(src), "cut": len(cut), "windows": n_reads - (len(src) - len(cut)), "longest": max(src)}
    got = eng.debug_last_packed()
    k = int(got[2].size)
    assert 0 < k <= n_reads and (how in ("blocks", "cut") or k == n_reads), (k, n_reads)
    # (every submission of a piece with a cut read is as wide as the tile, and then its last rows hold a window of that width)
    lr.compare_rows(got, lr.host_rows(yard if k == n_reads else tail_text(yard, k)), [r[0] for r in recs], first=n_reads - k)
    return n_reads
