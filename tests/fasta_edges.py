"""Crafted FASTA texts for the device tiler at its thread, wave, cell and turn edges -- TEST INFRASTRUCTURE (no GPU; figures checked
in tests/test_fasta_edges_host.py, submitted by tests/test_gpu_fasta_edges.py).  tests/fasta_zoo.py places a handful of bytes on
the 4 KB cell edge by hand; here ONE short text that holds every transition the walkers of csrc/fasta_dev.h distinguish (probe) is
slid over every edge of a given size (slide), and further texts reach what no small text can: the second turn of the one-workgroup
kernels (turn_texts, many_contigs), the repeat of a call whose contig tables were too small (tiny_contigs), runs of contigs without
reads in front of k_fa_reads' binary search (empty_runs), and every way a text can end (endings).

Every text begins with the '>' of its first header, so an offset in a returned dict is the offset the device sees.  Every
generator returns the bytes and a dict of where it put things; the random bases come from one fixed seed per text.

The yardstick is fastq.tile_fasta -- the rule as include/mlst.h states it -- followed by the host pack of its FASTQ text
(assert_rows_equal)."""
import os
import re
import tempfile

import numpy as np

from metamlst_amd.fastq import tile_fasta

CELL = 4096                 # FA_CELL: bytes per workgroup
THREAD, WAVE = 16, 1024     # bytes per thread, per wave
TURN = 1024                 # cells per turn of k_fa_state, values per turn of k_fa_scan
TILE = (150, 25, 50)
SEED = 20_261_018


def _bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def _lines(s, width=70, eol=b"\n"):
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width))


# ------------------------------------------------------------------ the yardstick
def yardstick(src, tile=TILE):
    """(FASTQ text of fastq.tile_fasta, contigs) of a FASTA given as bytes or as a path"""
    if isinstance(src, (bytes, bytearray, memoryview)):
        raw = bytes(src)
        fd, path = tempfile.mkstemp(suffix=".fna")
        try:
            with os.fdopen(fd, "wb") as f:
                f.write(raw)
            text = b"".join(tile_fasta(path, *tile))
        finally:
            os.unlink(path)
    else:
        raw = open(src, "rb").read()
        text = b"".join(tile_fasta(src, *tile))
    return text, (b"\n" + raw).count(b"\n>")


def count_reads(src, tile=TILE):
    return yardstick(src, tile)[0].count(b"\n") // 4


def _read_name(names, r):
    ci, st = names[r][1:].split(b"_")
    return "read %d: contig %d, start %d" % (r, int(ci), int(st))


def assert_rows_equal(eng, src, tile, n_want=None):
    """One submission of `src` (bytes or a path) through Engine.submit_fasta against the yardstick: counts, the packed rows word for
    word, counters[2].  A mismatch names the first differing read by the contig and start of its name in the yardstick text."""
    from metamlst_amd.engine import pack_fastq_host
    raw = bytes(src) if isinstance(src, (bytes, bytearray, memoryview)) else open(src, "rb").read()
    text, want_contigs = yardstick(src, tile)
    names = text.split(b"\n")[0::4]
    n_rec = text.count(b"\n") // 4
    eng.reset_sample()
    n_contigs, n_reads = eng.submit_fasta(raw, *tile)
    assert n_reads == n_rec and (n_want is None or n_reads == n_want), (n_reads, n_rec, n_want)
    assert n_contigs == want_contigs, (n_contigs, want_contigs)
    assert int(eng.stats().counters[2]) == n_reads
    if n_rec == 0:      # (nothing was packed: debug_last_packed still holds the submission before)
        return n_contigs, n_reads
    packed, qrows, lens, wpr, qs = eng.debug_last_packed()
    longest = max(len(l) for l in text.split(b"\n")[1::4])
    h_packed, h_qrows, h_lens, n, h_wpr, h_qs = pack_fastq_host(text, read_len_max=longest)
    assert (n, h_wpr, h_qs) == (n_reads, wpr, qs) and lens.size == n, ((n, h_wpr, h_qs), (n_reads, wpr, qs), lens.size)
    bad = np.nonzero(lens != h_lens[:n])[0]
    assert bad.size == 0, "length of " + _read_name(names, int(bad[0]))
    bad = np.nonzero((qrows != h_qrows[:n]).any(axis=1))[0]
    assert bad.size == 0, "quality row of " + _read_name(names, int(bad[0]))
    assert packed.size == ((n + 63) // 64) * 64 * wpr
    bad = np.nonzero(packed != h_packed[:packed.size])[0]
    if bad.size:      # resident layout: groups of 64 reads, word c of read r at (r >> 6) * 64 * wpr + (((c >> 1) * 64 + (r & 63)) << 1) + (c & 1)
        r = np.unique((bad // (64 * wpr)) * 64 + ((bad % (64 * wpr)) >> 1 & 63))
        r = r[r < n]
        assert False, "packed row of " + (_read_name(names, int(r[0])) if r.size else "no read (padding word %d)" % int(bad[0]))
    return n_contigs, n_reads


# ------------------------------------------------------------------ the probe
# name -> what stands at the offset probe() gives for it (a regular expression matched AT that offset)
PROBE_PATTERNS = {
    "bases LF >": rb"[ACGT]\n>",
    "header LF bases": rb"t\n[ACGT]",
    "header LF >": rb"y\n>",
    "bases CR LF bases": rb"[ACGT]\r\n[ACGT]",
    "bases LF LF bases": rb"[ACGT]\n\n[ACGT]",
    "LF CR LF": rb"\n\r\n",
    "> inside a sequence line": rb"[ACGT]>[ACGT]",
    "> inside a header": rb" > ",
    "tab inside a header": rb"\t",
    "lower-case stretch": rb"[acgt]{40}\n",
    "N": rb"NNN[ACGT]",
    "0x00 among the bases": rb"\x00[ACGT]",
    "0xFF among the bases": rb"\xff[ACGT]",
}


def probe():
    """A few hundred bytes with every transition the walkers distinguish; contigs of 100, 151, 0, 176, 60 and 50 bases: at 150,25,50
    they give 1, 2, 0, 3, 1 and 1 reads.  Returns (text, {name: offset}); the names are those of PROBE_PATTERNS."""
    rng = np.random.default_rng(SEED)
    t = bytearray()
    at = {}

    def put(x):
        t.extend(x)

    def mark(name, back=0):
        at[name] = len(t) - back

    put(b">p0 first"); mark("header LF bases", 1); put(b"\n" + _bases(rng, 60) + b"\n" + _bases(rng, 40))      # 100 bases
    mark("bases LF >", 1); put(b"\n")
    put(b">p1 with"); mark("> inside a header"); put(b" > and a"); mark("tab inside a header"); put(b"\ttab\n")
    put(_bases(rng, 50)); mark("bases CR LF bases", 1); put(b"\r\n" + _bases(rng, 50) + b"\r\n" + _bases(rng, 51) + b"\n")      # 151 bases
    put(b">empty"); mark("header LF >", 1); put(b"\n")
    put(b">p2\n" + _bases(rng, 40)); mark("bases LF LF bases", 1); put(b"\n\n" + _bases(rng, 40)); mark("LF CR LF"); put(b"\n\r\n")
    s = bytearray(_bases(rng, 30)); s[11] = ord(">"); put(s[:11]); mark("> inside a sequence line", 1); put(s[11:] + b"\n")
    mark("lower-case stretch"); put(_bases(rng, 40).lower() + b"\n")
    put(_bases(rng, 10)); mark("N"); put(b"NNN" + _bases(rng, 13) + b"\n")      # 40 + 40 + 30 + 40 + 26 = 176 bases
    s = bytearray(_bases(rng, 60)); s[20] = 0; s[41] = 0xFF
    put(b">p3\n"); mark("0x00 among the bases", -20); mark("0xFF among the bases", -41); put(bytes(s) + b"\n")
    put(b">p4 last\n" + _bases(rng, 50) + b"\n")
    assert set(at) == set(PROBE_PATTERNS)
    return bytes(t), at


PROBE_READS = 8      # at 150,25,50


def _pad_header(cur, want, edge, tag):
    """a header line (an empty contig) behind `cur` bytes of text that ends so that the next byte's offset is `want` modulo `edge`"""
    head = b">pad%d_" % tag
    k = (want - (cur + len(head) + 1)) % edge
    return head + b"x" * k + b"\n"


def slide(edge):
    """Copies of probe(), copy j behind a padding header whose length puts byte j of the probe at an offset that is 0 modulo
    `edge` (16: a thread's first byte, 1,024: a wave's, 4,096: a cell's) -- one copy per byte of the probe; at 16 one per
    residue.  Returns (text, {"copies": [(j, offset of the copy's byte 0)], "probe": probe's dict})."""
    assert edge in (THREAD, WAVE, CELL)
    p, at = probe()
    t = bytearray()
    copies = []
    for j in range(len(p) if edge > THREAD else THREAD):
        t.extend(_pad_header(len(t), -j, edge, j))
        assert (len(t) + j) % edge == 0
        copies.append((j, len(t)))
        t.extend(p)
    return bytes(t), {"copies": copies, "probe": at}


# ------------------------------------------------------------------ turns of the one-workgroup kernels
def _filler(rng, upto):
    """70-column contigs of 7,000 bases (47 reads at 150,150,50) up to at least `upto` bytes"""
    t = bytearray()
    k = 0
    while len(t) < upto:
        t.extend(b">fill%d\n" % k + _lines(_bases(rng, 7000)))
        k += 1
    return t


def turn_texts():
    """Texts of more than 1,024 cells: {name: (text, dict)}; dict["tile"] is the tile to use, dict["span"] = (first byte, byte
    behind the last one) of the line that lies over the turn edge(s), dict["min_cells"] what fasta_info()[0] must exceed.
      seq_over_turn                  a contig on ONE line from two cells (and more) in front of byte 1,024 x 4,096 to two behind it
      hdr_over_turn                  the same with a HEADER of 40,000 bytes over that byte, a 400-base contig behind it: the only
                                     shape that tells a carried kind from the FA_SEQ k_fa_state starts with
      turn_without_line_start        a header that begins in turn 1, covers cells 1,024 .. 2,047 and ends in turn 3
      turn_without_line_start_seq    the same line as a sequence line (tile 320,320,50: under 40,000 reads)"""
    out = {}
    edge = TURN * CELL
    for name in ("seq_over_turn", "hdr_over_turn"):
        rng = np.random.default_rng(SEED + 1)
        t = _filler(rng, 1019 * CELL)
        assert len(t) < edge - 3 * CELL
        if name == "seq_over_turn":
            t.extend(b">one_line\n")
            lo = len(t)
            t.extend(_bases(rng, edge + 2 * CELL + 777 - lo))
            hi = len(t)
            t.extend(b"\n")
        else:
            lo = len(t)
            t.extend(b">" + b"h" * 39_999)
            hi = len(t)
            t.extend(b"\n" + _lines(_bases(rng, 400)))
        t.extend(b">short\n" + _lines(_bases(rng, 230)))
        out[name] = (bytes(t), {"tile": (150, 150, 50), "span": (lo, hi), "min_cells": TURN})
    for name in ("turn_without_line_start", "turn_without_line_start_seq"):
        rng = np.random.default_rng(SEED + 2)
        t = bytearray(b">first\n" + _lines(_bases(rng, 400)))
        n = 2 * edge + CELL + 555 - len(t)
        if name == "turn_without_line_start":
            lo = len(t)
            t.extend(b">" + b"h" * (n - 1))
            hi = len(t)
            t.extend(b"\n" + _lines(_bases(rng, 400)))
        else:
            t.extend(b">one_line\n")
            lo = len(t)
            t.extend(_bases(rng, n))
            hi = len(t)
            t.extend(b"\n")
        t.extend(b">second\n" + _lines(_bases(rng, 230)))
        out[name] = (bytes(t), {"tile": (150, 150, 50) if name == "turn_without_line_start" else (320, 320, 50), "span": (lo, hi), "min_cells": 2 * TURN})
    return out


# ------------------------------------------------------------------ many contigs
MANY_LENS = (0, 49, 50, 150, 151, 176, 400)      # 0, 0, 1, 1, 2, 3, 11 reads at 150,25,50


def many_contigs(k=2500):
    """k contigs (60-column lines) whose lengths cycle through MANY_LENS: more than two turns of k_fa_scan over the contigs, fewer
    contigs than the entry's first guess of the tables.  Returns (text, {"contigs": k, "guess": len // 64 + 1024})."""
    rng = np.random.default_rng(SEED + 3)
    t = bytearray()
    for c in range(k):
        t.extend(b">c%d\n" % c + _lines(_bases(rng, MANY_LENS[c % len(MANY_LENS)]), 60))
    return bytes(t), {"contigs": k, "guess": len(t) // 64 + 1024}


def tiny_contigs(k=3000):
    """k contigs, contig c with c % 10 bases behind the header b">%d" % (c % 10): more contigs than the entry's guess of one per 64
    bytes and 1,024, so the call must grow its tables and repeat.  Returns (text, {"contigs": k, "guess": len // 64 + 1024})."""
    rng = np.random.default_rng(SEED + 4)
    t = bytearray()
    for c in range(k):
        t.extend(b">%d\n" % (c % 10) + _lines(_bases(rng, c % 10)))
    return bytes(t), {"contigs": k, "guess": len(t) // 64 + 1024}


# ------------------------------------------------------------------ runs of contigs without reads
START_RUNS = (1, 2, 65, 300)


def empty_runs(first=1):
    """Runs of contigs without reads at 150,25,50 and at 320,1,50 (no bases, or 1 .. 49 of them, in turn): `first` of them at the
    very start of the text, 300 in the middle, 300 at the very end, contigs with reads (400 and 170 bases) around the runs.
    Returns (text, {"runs": [(first contig, contigs)], "contigs": all of them})."""
    rng = np.random.default_rng(SEED + 5)
    t = bytearray()
    runs = []
    c = 0

    def run(n):
        nonlocal c
        runs.append((c, n))
        for k in range(n):
            t.extend(b">none%d\n" % c + _lines(_bases(rng, (0, 49, 1, 17, 0)[k % 5])))
            c += 1

    def full(n):
        nonlocal c
        t.extend(b">full%d\n" % c + _lines(_bases(rng, n)))
        c += 1

    run(first); full(400); full(170); run(300); full(170); full(400); run(300)
    return bytes(t), {"runs": runs, "contigs": c}


# ------------------------------------------------------------------ how a text ends
END_LENGTHS = (592, 593, 607, 4096, 4097)      # 0, 1 and 15 modulo 16; a whole cell; a cell and a byte
ENDINGS = ("bases", "bases_lf", "bases_crlf", "lf_gt", "lf_gt_name", "gt_alone", "gt_lf_alone", "bases_cr")


def endings():
    """{(name, length): text}: every ending at the lengths END_LENGTHS, the length set by the first header's; the header-only
    texts ("gt_alone": a header without its LF, "gt_lf_alone") also at their natural lengths 1 and 2 (b">" and b">\\n").
    "bases_cr" ends in a CR that is the last byte: the device refuses it (tile_fasta's strip() takes the CR off)."""
    rng = np.random.default_rng(SEED + 6)
    body = _lines(_bases(rng, 260)) + b">two\n" + _lines(_bases(rng, 130), 70, b"\r\n") + b">three\n" + _bases(rng, 55)
    tails = {"bases": b"", "bases_lf": b"\n", "bases_crlf": b"\r\n", "lf_gt": b"\n>", "lf_gt_name": b"\n>name", "bases_cr": b"\r"}
    out = {("gt_alone", 1): b">", ("gt_lf_alone", 2): b">\n"}
    for n in END_LENGTHS:
        for name, tail in tails.items():
            k = n - len(body) - len(tail) - 2
            assert k >= 0
            out[(name, n)] = b">" + b"e" * k + b"\n" + body + tail
        out[("gt_alone", n)] = b">" + b"e" * (n - 1)
        out[("gt_lf_alone", n)] = b">" + b"e" * (n - 2) + b"\n"
    assert all(len(v) == key[1] for key, v in out.items())
    return out


# ------------------------------------------------------------------ refusals
def three_cells():
    """A clean text of exactly three cells (one header, 70-column lines) and the offsets of sequence bytes the refusal tests
    overwrite: {"t3": the fourth byte of a thread in cell 0, "last": the last byte of a thread in cell 0 (its successor the first
    byte of the next thread), "cell2": a byte in mid-thread in cell 2, "hdr": a byte inside the header, "line_start": the first byte
    of a sequence line in cell 1, "cell0_end": the last byte of cell 0 -- a base, its successor the first of cell 1 too}."""
    rng = np.random.default_rng(SEED + 7)
    t = bytearray(b">three cells of text\n" + _lines(_bases(rng, 3 * CELL)))[:3 * CELL - 1] + b"\n"
    assert len(t) == 3 * CELL

    def base_at(p):
        while not (t[p] in b"ACGT" and t[p + 1] in b"ACGT" and t[p - 1] in b"ACGT"):
            p += THREAD
        return p
    at = {"t3": base_at(40 * THREAD + 3), "last": base_at(77 * THREAD + 15), "cell2": base_at(2 * CELL + 100 * THREAD + 7), "hdr": 7}
    ls = t.index(b"\n", CELL + 500) + 1
    assert t[ls] in b"ACGT" and t[ls + 1] in b"ACGT"
    at["line_start"] = ls
    assert all(t[p] in b"ACGT" for p in range(CELL - 2, CELL + 2))      # (an LF every 71 bytes: none of them on the cell edge)
    at["cell0_end"] = CELL - 1
    assert at["t3"] % THREAD == 3 and at["last"] % THREAD == 15 and at["t3"] < CELL and at["last"] < CELL and at["cell2"] >= 2 * CELL
    return bytes(t), at


def with_bytes(text, *puts):
    """text with (offset, byte string) pairs written over it"""
    t = bytearray(text)
    for p, x in puts:
        t[p:p + len(x)] = x
    return bytes(t)


def find(pattern, text, at):
    """True when the regular expression matches AT offset `at` of text"""
    return re.compile(pattern, re.S).match(text, at) is not None
