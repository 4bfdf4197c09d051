"""A crafted FASTA for the device tiler (tests/test_gpu_fasta.py, figures checked in tests/test_fasta_host.py): every rule of
fastq.tile_fasta and every place where the 4 KB cells of csrc/fasta_dev.h could go wrong.  Offsets "in a cell" count from the first
header of the file: that is where the text of a call begins on the device."""
import numpy as np

from metamlst_amd.fastq import tile_fasta

CELL = 4096
EDGE_LENS = [0, 49, 50, 149, 150, 151, 175, 176, 1000]      # 0, 0, 1, 1, 1, 2, 2, 3, 35 reads at 150,25,50
EDGE_READS = [0, 0, 1, 1, 1, 2, 2, 3, 35]


def count_reads(path, read_len=150, stride=25, min_len=50):
    return b"".join(tile_fasta(path, read_len, stride, min_len)).count(b"\n") // 4


def zoo(path, total, one_line_10k=False, seed=7):
    """Writes the file; the number of reads at 150,25,50 is `total` (a filler contig makes up the difference).  Returns a dict of
    the byte offsets (from the first header) the edge cases were placed at.  one_line_10k: the 10,000-base contig on one line is
    in (it alone gives 395 reads, so the files of 63 to 65 reads cannot hold it)."""
    rng = np.random.default_rng(seed)
    body = bytearray()
    at = {}

    def bases(n):
        return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])

    def lines(s, width=70, eol=b"\n"):
        return b"".join(s[i:i + width] + eol for i in range(0, len(s), width))

    def pad_to(offset_mod):
        """a header line (an empty contig) that ends so that the next byte's offset is offset_mod modulo the cell size"""
        k = (offset_mod - (len(body) + 5)) % CELL      # b">pad" + k bytes + LF
        body.extend(b">pad" + b"x" * k + b"\n")
        assert len(body) % CELL == offset_mod

    for k, n in enumerate(EDGE_LENS):      # the edge lengths; the 1,000-base contig has lower-case stretches
        s = bases(n)
        if n == 1000:
            s = s[:100] + s[100:400].lower() + s[400:900] + s[900:].lower()
        body.extend(b">edge%d len=%d\n" % (k, n) + lines(s))
    body.extend(b">c321\n" + lines(bases(321), 60))
    body.extend(b">long " + b"h" * 5000 + b" > \t end\n" + lines(bases(120)))      # a header longer than a cell (with a tab and a '>' in it)
    pad_to(0)
    at["header_at_cell_start"] = len(body)
    s = bytearray(bases(60)); s[5:15] = b"N" * 10; s[20:26] = b"RYKMSW"; s[40:44] = b"nnnn"
    body.extend(b">cellstart\n" + lines(bytes(s)))
    pad_to(CELL - 80)
    body.extend(bases(80))      # the line's LF is the first byte of a cell, the next header follows it
    at["lf_at_cell_start"] = len(body)
    assert len(body) % CELL == 0
    body.extend(b"\n>after_lf\r\n" + lines(bases(80), 50, b"\r\n"))
    pad_to(CELL - 41)
    body.extend(bases(40))
    at["crlf_over_edge"] = len(body)
    assert len(body) % CELL == CELL - 1
    body.extend(b"\r\n" + bases(30) + b"\r\n")      # the CR is the last byte of a cell, its LF the first of the next
    s = bytearray(bases(70)); s[10] = ord(">"); s[30] = 0x80; s[31] = 0xFF; s[50] = 0; s[51] = ord("@")
    body.extend(b">odd_bytes\n" + bytes(s[:35]) + b"\n" + bytes(s[35:]) + b"\n")
    body.extend(b">empty_lines\n\n" + bases(30) + b"\n\n\r\n" + bases(30) + b"\r\n\n")
    body.extend(b">first_of_two\n>second_of_two\n" + lines(bases(90)))
    if one_line_10k:
        body.extend(b">one_line\n" + bases(10_000) + b"\n")
    tail = b">no_lf_at_end\n" + bases(55)
    junk = b"junk in front of the first header\n\tmore > junk\r\nACGTACGT\n"
    with open(path, "wb") as f:
        f.write(junk + bytes(body) + tail)
    need = total - count_reads(path)
    assert need >= 0, need
    while need > 0:      # fillers of at most 70 reads each: the groups of 64 reads span several contigs
        k = min(need, 70)
        body.extend(b">filler\n" + lines(bases(150 + (k - 1) * 25)))
        need -= k
    with open(path, "wb") as f:
        f.write(junk + bytes(body) + tail)
    at["junk"] = len(junk)
    return at
