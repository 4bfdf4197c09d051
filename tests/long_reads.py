"""Builders for FASTQ records longer than a packed read -- TEST INFRASTRUCTURE (no GPU; used by tests/test_long_reads_host.py and
tests/test_gpu_long_reads.py).

The yardstick of every device test is fastq.tile_fastq -- the rule of mlst_set_read_tiling as include/mlst.h states it -- followed
by the host pack of its FASTQ text (assert_rows_equal).  The Phred value of base i of record r is 33 + (7 i + r) % 41: it changes
with the position, so a window that carries the wrong slice of the quality line cannot pass."""
import os
import tempfile

import numpy as np

from metamlst_amd.fastq import tile_fastq

TILES = ((150, 25), (320, 1), (36, 100), (150, 150))
SEED = 20_261_018


def edge_lengths(read_len, stride):
    """record lengths at every edge of the rule, and the two that do not fit 15 / 16 bits"""
    return [0, 1, read_len - 1, read_len, read_len + 1, read_len + stride, read_len + stride + 1, 32_767, 32_768, 100_003]


def bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def quals(n, r):
    return ((7 * np.arange(n, dtype=np.int64) + r) % 41 + 33).astype(np.uint8).tobytes()


def record(r, seq, eol=b"\n", name=None):
    return b"@" + (name if name is not None else b"rec%d some comment" % r) + eol + seq + eol + b"+" + eol + quals(len(seq), r) + eol


def text_of(seqs, eol=b"\n", final_eol=True):
    t = b"".join(record(r, s, eol) for r, s in enumerate(seqs))
    return t if final_eol else t[:len(t) - len(eol)]


def random_records(lengths, seed=SEED):
    rng = np.random.default_rng(seed)
    return [bases(rng, n) for n in lengths]


def window_starts(n, read_len, stride):
    """the rule restated on its own: starts of the windows of a record of n bases (one start, 0, for a record that is not cut)"""
    if n <= read_len:
        return [0]
    s = [k * stride for k in range((n - read_len) // stride + 1)]
    return s if (n - read_len) % stride == 0 else s + [n - read_len]


def fa_windows_of(n, read_len, stride, min_len=0):
    """csrc/fasta_dev.h's count, as arithmetic"""
    if n < min_len:
        return 0
    if n <= read_len:
        return 1
    span = n - read_len
    return span // stride + 1 + (1 if span % stride else 0)


def yardstick(text, tile, suffix=".fastq"):
    """the FASTQ text fastq.tile_fastq makes of a FASTQ given as bytes"""
    fd, path = tempfile.mkstemp(suffix=suffix)
    try:
        with os.fdopen(fd, "wb") as f:
            f.write(bytes(text))
        return b"".join(tile_fastq(path, *tile))
    finally:
        os.unlink(path)


def parse(text):
    """[(name line, sequence, quality)] of FASTQ text with LF line ends"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    assert all(l == b"+" for l in lines[2:-1:4])
    return list(zip(lines[0:-1:4], lines[1:-1:4], lines[3:-1:4]))


def host_rows(yard):
    """mlst_pack_fastq_host of yardstick text: (packed, qrows, lens, n, wpr, qstride) at the width of its longest read"""
    from metamlst_amd.engine import pack_fastq_host
    longest = max([len(s) for _, s, _ in parse(yard)] + [1])
    return pack_fastq_host(yard, read_len_max=longest)


def compare_rows(got, want, names, first=0):
    """debug_last_packed() against host_rows() (of the reads from `first` on: the caller packed only those); as
    tests/fasta_edges.py::assert_rows_equal compares"""
    packed, qrows, lens, wpr, qs = got
    h_packed, h_qrows, h_lens, n, h_wpr, h_qs = want
    assert (n, h_wpr, h_qs) == (lens.size, wpr, qs), ((n, h_wpr, h_qs), (lens.size, wpr, qs))
    bad = np.nonzero(lens != h_lens[:n])[0]
    assert bad.size == 0, "length of read %d (%r): %d, not %d" % (int(bad[0]), names[first + int(bad[0])], int(lens[bad[0]]), int(h_lens[bad[0]]))
    bad = np.nonzero((qrows != h_qrows[:n]).any(axis=1))[0]
    assert bad.size == 0, "quality row of read %d (%r)" % (int(bad[0]), names[first + int(bad[0])])
    assert packed.size == ((n + 63) // 64) * 64 * wpr
    bad = np.nonzero(packed != h_packed[:packed.size])[0]
    if bad.size:      # resident layout: groups of 64 reads, word c of read r at (r >> 6) * 64 * wpr + (((c >> 1) * 64 + (r & 63)) << 1) + (c & 1)
        r = np.unique((bad // (64 * wpr)) * 64 + ((bad % (64 * wpr)) >> 1 & 63))
        r = r[r < n]
        assert False, "packed row of " + ("read %d (%r)" % (int(r[0]), names[first + int(r[0])]) if r.size else "no read (padding word %d)" % int(bad[0]))


def assert_rows_equal(eng, text, tile, n_want=None):
    """One tiled submit_fastq of `text` against the yardstick: the read count, the packed rows word for word, counters[2] and the
    counts of read_tiling_info.  Returns the number of reads."""
    yard = yardstick(text, tile)
    recs = parse(yard)
    src = [len(s) for s in bytes(text).replace(b"\r\n", b"\n").split(b"\n")[1::4]]
    eng.reset_sample()
    eng.set_read_tiling(*tile)
    n_reads = eng.submit_fastq(text)
    assert n_reads == len(recs) and (n_want is None or n_reads == n_want), (n_reads, len(recs), n_want)
    assert int(eng.stats().counters[2]) == n_reads
    cut = [n for n in src if n > tile[0]]
    assert eng.read_tiling_info() == {"records": len(src), "cut": len(cut), "windows": n_reads - (len(src) - len(cut)), "longest": max(src)}
    compare_rows(eng.debug_last_packed(), host_rows(yard), [r[0] for r in recs])
    return n_reads


def genome_reads(genome, n_reads, lo=400, hi=3000, seed=SEED):
    """FASTQ text of n_reads reads of lo .. hi bases drawn from either strand of `genome` (uint8 ASCII)"""
    rng = np.random.default_rng(seed)
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    seqs = []
    for _ in range(n_reads):
        n = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, len(genome) - n))
        s = genome[at:at + n]
        seqs.append((comp[s][::-1] if rng.random() < 0.5 else s).tobytes())
    return text_of(seqs)


def bgzip(text, block=65280):
    """`text` as a BGZF file with the writer of tests/bam_writer.py (blocks of `block` bytes, the EOF block last)"""
    from bam_writer import _bgzf_block
    return b"".join(_bgzf_block(text[i:i + block]) for i in range(0, len(text), block)) + _bgzf_block(b"")
