"""The record "zoo" of the BAM reads tests (tests/test_bam_reads_host.py checks its figures on the CPU, tests/test_gpu_bam_reads.py
types it on the device): reads of an isolate, each written either as an unmapped record or as a reverse-strand "mapped" record that
holds its reverse complement, plus the edge records of the rules in include/mlst.h.  Test infrastructure only."""
import functools
import gzip
import struct

import numpy as np

import bam_writer
import fixtures as fx

REFS = [("chrHost", 5_000_000)]
EDGE_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 36, 150, 159, 160, 161, 319, 320)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
BLOCK = 60000      # bam_writer cuts a BGZF block every 60,000 inflated bytes


def revcomp(seq: str) -> str:
    return seq.encode().translate(_COMP)[::-1].decode()


def unmapped(name, seq, qual, flag=4, tags=()):
    return (name, flag, "*", 0, 0, "*", seq, qual, list(tags))


def reverse_mapped(name, seq, qual, flag=16, pos=1000, tags=()):
    """the read `seq` as a record on the reverse strand: SEQ is its reverse complement, QUAL reversed"""
    return (name, flag, "chrHost", pos, 30, "%dM" % len(seq), revcomp(seq), qual if qual == "*" else qual[::-1], list(tags))


def skipped(kind, k):
    if kind == "secondary":
        return ("sec%d" % k, 256 | 16, "chrHost", 50 + k, 3, "20M", "ACGTACGTACGTACGTACGT", "I" * 20, ["NM:i:1"])
    if kind == "supplementary":
        return ("sup%d" % k, 2048, "chrHost", 70 + k, 3, "10M10S", "ACGTACGTACGTACGTACGT", "*", [])
    return ("empty%d" % k, 4, "*", 0, 0, "*", "*", "*", [])


@functools.lru_cache(maxsize=None)
def isolate(n_reads=6000):
    db, idx = fx.ecoli_small()
    fb, fq, off, _, _ = fx.isolate_reads(db, "ecoli", 3, n_reads=n_reads)
    reads = []
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        reads.append((bytes(fb[lo:hi]).decode(), bytes(fq[lo:hi]).decode()))
    return reads


def edge_records():
    """kept and skipped edge records, in file order (the first record of the file is a skipped one)"""
    rng = np.random.default_rng(5)
    out = [skipped("secondary", 0), skipped("empty", 0)]
    for k, L in enumerate(EDGE_LENGTHS):
        seq = "".join(rng.choice(list("ACGT"), size=L)); qual = "".join(chr(33 + int(q)) for q in rng.integers(2, 42, size=L))
        out.append(unmapped("len%d" % L, seq, qual) if k % 2 else reverse_mapped("len%d" % L, seq, qual))
        if k % 4 == 1:
            out.append(skipped(("secondary", "supplementary", "empty")[k % 3], 10 + k))
    out.append(unmapped("allN", "N" * 37, "#" * 37))
    out.append(reverse_mapped("allNrev", "N" * 16, "5" * 16))
    out.append(unmapped("NbyFiller", "ACGTACGTN", "IIIIIIII!"))              # odd length: the N shares its byte with the filler nibble
    out.append(reverse_mapped("NbyFillerRev", "NACGTAC", "~IIIII!"))         # stored as GTACGTN: the same on the reverse strand
    out.append(unmapped("iupac", "ACGTRYKMSWBDHVN" + "ACGT" * 5, "I" * 35))
    out.append(reverse_mapped("iupacRev", "ACGTRYKMSWBDHVN" + "ACGT" * 5, "".join(chr(40 + k) for k in range(35))))
    out.append(unmapped("noQual", "ACGTTGCA" * 9, "*"))
    out.append(reverse_mapped("noQualRev", "ACGTTGCAA" * 7, "*"))
    out.append(unmapped("phred0and93", "ACGT" * 10, "!~" * 20))
    # raw quality bytes above 127 (the first one not 0xFF): clamped to 127, as the text path clamps chr(q + 33)
    out.append(unmapped("highQ", "ACGTACGTAC", "".join(chr(33 + q) for q in (128, 200, 254, 127, 126, 0, 255, 129, 93, 94))))
    out.append(reverse_mapped("highQrev", "ACGTTGCATGA", "".join(chr(33 + q) for q in (254, 5, 255, 128, 127, 200, 1, 0, 130, 222, 223))))
    out.append(skipped("supplementary", 40)); out.append(skipped("empty", 41)); out.append(skipped("secondary", 42))
    out.append(unmapped("q", "GATTACA" * 5, "F" * 35))                       # QNAME of 1 character
    out.append(reverse_mapped("Q" * 254, "GATTACA" * 6, "G" * 42))           # ... and of 254
    out.append(unmapped("bigTag", "ACGGT" * 12, "H" * 60, tags=["RG:Z:grp", "ZZ:Z:" + "x" * 20000, "NM:i:3"]))
    return out


def is_kept(rec) -> bool:
    return not rec[1] & 0x900 and rec[6] != "*"


def zoo(n_kept: int):
    """records whose kept reads number n_kept exactly: the edge records, isolate reads (every other one reverse-strand), skipped
    records sprinkled in between, and a skipped record at the very end"""
    recs = edge_records()
    have = sum(is_kept(r) for r in recs)
    assert n_kept >= have
    for k, (seq, qual) in enumerate(isolate()[:n_kept - have]):
        recs.append(reverse_mapped("iso%d" % k, seq, qual, pos=1 + 37 * k) if k % 2 else unmapped("iso%d" % k, seq, qual))
        if k % 97 == 13:
            recs.append(skipped(("secondary", "supplementary", "empty")[k % 3], 100 + k))
    recs.append(skipped("secondary", 999999))
    assert sum(is_kept(r) for r in recs) == n_kept
    return recs


def zoo_paired(n_pairs: int):
    """a name-collated paired file: mates adjacent (FLAG 0x1 with 0x40 / 0x80), the second mate often on the reverse strand, skipped
    records between some pairs and between the two mates of some pairs; an odd number of them in places so that the parity of the
    kept count at a block boundary varies"""
    reads = isolate()
    recs = [skipped("supplementary", 0)]
    for p in range(n_pairs):
        (s1, q1), (s2, q2) = reads[2 * p], reads[2 * p + 1]
        if p % 5 == 0:
            s1, q1 = s1[:40 + p % 90], q1[:40 + p % 90]
        if p % 3 == 0:      # a fragment as short as a read: the mates cover the same bases, so both land on the same locus where one does
            s2, q2 = revcomp(s1), q1[::-1]
        recs.append(unmapped("pair%d" % p, s1, q1, flag=1 | 4 | 8 | 64))
        if p % 23 == 7:
            recs.append(skipped(("secondary", "empty", "supplementary")[p % 3], 200 + p))      # between the mates of one pair
        recs.append(reverse_mapped("pair%d" % p, s2, q2, flag=1 | 16 | 128, pos=5 + p) if p % 2 else unmapped("pair%d" % p, s2, q2, flag=1 | 4 | 8 | 128))
        if p % 31 == 3:
            recs.append(skipped(("empty", "secondary")[p % 2], 300 + p))
    recs.append(skipped("empty", 999999))
    return recs


def write(path, recs, refs=REFS):
    bam_writer.write_bam(str(path), "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs), refs, recs)
    return str(path)


def layout(path):
    """(offset of every record in the inflated file, end of the last one, FLAG and l_seq per record) read from the file itself"""
    raw = gzip.open(path, "rb").read()
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]; at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    starts, flags, lseqs = [], [], []
    while at < len(raw):
        starts.append(at)
        flags.append(struct.unpack_from("<H", raw, at + 18)[0]); lseqs.append(struct.unpack_from("<i", raw, at + 20)[0])
        at += 4 + struct.unpack_from("<i", raw, at)[0]
    assert at == len(raw)
    return np.array(starts), at, np.array(flags), np.array(lseqs)


def kept_mask(flags, lseqs):
    return ((flags & 0x900) == 0) & (lseqs > 0)


def bgzf_blocks(raw: bytes):
    """[(offset, size)] of the BGZF blocks of a file"""
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append((at, size)); at += size
    return out


def reblock(text: bytes, path) -> str:
    """inflated BAM bytes written as BGZF blocks of BLOCK bytes and the EOF block (for files cut inside a record)"""
    with open(str(path), "wb") as f:
        for at in range(0, len(text), BLOCK):
            f.write(bam_writer._bgzf_block(text[at:at + BLOCK]))
        f.write(bam_writer._bgzf_block(b""))
    return str(path)


def split_fastq(text: bytes):
    """interleaved FASTQ text -> the two mate texts (records 0, 2, 4 ... and 1, 3, 5 ...)"""
    lines = text.split(b"\n")[:-1]
    recs = [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines), 4)]
    return b"".join(recs[0::2]), b"".join(recs[1::2])
