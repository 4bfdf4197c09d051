"""Shared by test_read_names_host.py and test_gpu_read_names.py: crafted FASTQ header lines with what samout.read_qname has to make
of them, a plain FASTQ reader (the yardstick of the device tests) and the sample builders."""
from __future__ import annotations

import functools

import numpy as np

import fixtures as fx
from metamlst_amd import samout

# (header line without its line end, the name kept -- None: no legal QNAME, the read keeps r<k>)
HEADERS = [
    (b"@read7", b"read7"),                                                  # name only
    (b"@M01:23:000-AB:1:1101:15589:1332 1:N:0:ATCACG", b"M01:23:000-AB:1:1101:15589:1332"),      # description behind a space
    (b"@SRR1.77\tlength=150", b"SRR1.77"),                                  # description behind a TAB
    (b"@", None),                                                           # `@` alone
    (b"@ only a description", None),                                        # an empty name in front of a space
    (b"@" + b"n" * 254, b"n" * 254),                                        # exactly 254 bytes
    (b"@" + b"N" * 255, None),                                              # 255 bytes
    (b"@" + b"L" * 300 + b" x", None),                                      # far longer
    (b"@left@right", None),                                                 # an inner `@`
    (b"@del\x7fete", None),                                                 # a byte 0x7F
    (b"@high\x80bit", None),                                                # a byte 0x80
    (b"@ctl\x01x", None),                                                   # a control byte
    (b"@!\"#$%&'()*+,-./0123456789:;<=>?", b"!\"#$%&'()*+,-./0123456789:;<=>?"),      # `!`..`?`: all legal
    (b"@A[\\]^_`az{|}~", b"A[\\]^_`az{|}~"),                                # `A`..`~`
    (b"@a/1", b"a/1"),
]


def fastq_records(text: bytes) -> list:
    """[(header line, sequence, quality)] of FASTQ text, line ends (LF or CRLF) stripped from sequence and quality, kept off the header"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [(lines[k], lines[k + 1].rstrip(b"\r"), lines[k + 3].rstrip(b"\r")) for k in range(0, len(lines), 4)]


def yardstick(texts, base: int = 0, interleave: bool = False) -> dict:
    """{read index: header line} of the reads of `texts` (FASTQ texts in submission order; interleave: two mate files, record j of
    the first is read 2 j, of the second read 2 j + 1)"""
    heads = [[h for h, _, _ in fastq_records(t)] for t in texts]
    if interleave:
        assert len(heads) == 2 and len(heads[0]) == len(heads[1])
        flat = [h for pair in zip(*heads) for h in pair]
    else:
        flat = [h for hs in heads for h in hs]
    return {base + k: h for k, h in enumerate(flat)}


def kept(heads: dict, retained) -> dict:
    """what Engine.read_names() has to return: the legal names of the retained reads"""
    out = {}
    for ri in retained:
        nm = samout.read_qname(heads[ri], -1)
        if nm != b"r-1":
            out[ri] = nm
    return out


def illumina(k: int) -> bytes:
    """an Illumina-style header of varying length, about 40 bytes of name"""
    return b"@M0%d:77:000000000-K%dXY:1:%d:%d:%d %d:N:0:ACGT" % (k % 7, k % 13, 1101 + k % 9, 1000 + 37 * k, 2000 + k, 1 + k % 2)


def header_of(k: int) -> bytes:
    """read k's header: one of HEADERS for every fifth read, an Illumina-style one otherwise"""
    return HEADERS[(k // 5) % len(HEADERS)][0] if k % 5 == 0 else illumina(k)


@functools.lru_cache(maxsize=None)
def sample(n_reads: int = 5000, read_len: int = 150):
    """(index, [(bases, quals)]): reads of an isolate of the small fixture database (one allele in five with a deletion) in a genome
    that is mostly off the loci, a 2-base deletion or insertion planted into every seventh / eleventh read (banded records)"""
    db, idx = fx.ecoli_small(40, 5)
    fb, fq, off, _, _ = fx.isolate_reads(db, "ecoli", 3, n_reads=n_reads, genome=40_000, read_len=read_len)
    rng = np.random.default_rng(read_len)
    reads = []
    for k in range(len(off) - 1):
        b, q = fb[int(off[k]):int(off[k + 1])].tobytes(), fq[int(off[k]):int(off[k + 1])].tobytes()
        mid = len(b) // 2
        if k % 7 == 0:
            b, q = b[:mid] + b[mid + 2:], q[:mid] + q[mid + 2:]
        elif k % 11 == 0:
            b = b[:mid] + bytes(rng.choice(list(b"ACGT"), size=2).astype(np.uint8)) + b[mid:-2]
        reads.append((b, q))
    return idx, reads


def fastq_text(reads, header=header_of, eol: bytes = b"\n", first: int = 0) -> bytes:
    return b"".join(header(first + k) + eol + b + eol + b"+" + eol + q + eol for k, (b, q) in enumerate(reads))
