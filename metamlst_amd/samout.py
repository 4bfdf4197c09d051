"""The engine's alignments to the chosen alleles as SAM text (`cli type --write-sam`).

The reference leaves a BAM of each sample's reads on the MLST loci behind (the bowtie2 run in front of metamlst.py); here the
alignments are the engine's own, exported as records by Engine.export_alignments (mlst_alignments_export, include/mlst.h) and
formatted on the host by `write_sam(path, idx, chosen, aln, paired)`:

  * header: `@HD VN:1.6 SO:coordinate`, one `@SQ SN:<species>_<gene>_<allele> LN:<len>` per chosen allele in the order given
    (the names samin resolves: AlleleIndex.label), one `@PG` line;
  * records sorted by (position of the allele in `chosen`, pos0, read_index, strand, diag): the file's bytes do not depend on
    the order the device exported them in;
  * QNAME `r<k>`: the FASTQ path never carries read names to the device, so k is the read index, or read_index >> 1 when the
    sample was submitted as pairs -- the mates then share a name, as sequenceBank wants (metamlst.py:127).  No pairing flags, as
    with bowtie2 -U.  Under --long-reads / --long-bam-reads / --contigs the reads are windows and k is the window's index;
  * FLAG 16 * strand, plus 256 on every record of a read (a read index, not a QNAME) except its best one: the highest AS, ties
    to the first in the sort order above;
  * MAPQ 255, RNEXT *, PNEXT 0, TLEN 0; POS = pos0 + 1; SEQ as exported (reference strand); QUAL chr(min(q, 93) + 33);
  * optional fields in this order: AS:i XS:i XN:i:0 XM:i XO:i XG:i NM:i YT:Z:UU -- XM stands in the 15th column, which the
    reference reads by position (Q1).  AS and XM are the engine's true values.  XS carries the record's OWN AS: a documented
    placeholder (with -a over near-identical alleles every record has an equal-scoring sibling, and only records to the
    chosen alleles are exported).  XO (gap opens: I and D runs), XG (gap extensions: I and D bases) and NM (XG + the M
    columns whose SEQ letter is not the allele's, an N on either side included) are computed here from the CIGAR and the
    allele text.

Not written: BAM / BGZF, real read names, alignments to alleles that were not chosen, MD:Z."""
from __future__ import annotations

import numpy as np

from .index import AlleleIndex
from .samin import CIGAR_OPS

PG_LINE = "@PG\tID:metamlst_amd\tPN:metamlst_amd"


def gap_figures(ops, seq: bytes, allele: str, pos0: int) -> tuple[int, int, int]:
    """(XO, XG, NM) of one record: ops = its CIGAR (len << 4 | op), seq = its SEQ, allele = the allele's text, pos0 = its leftmost column"""
    xo = xg = mism = 0
    q, r = 0, pos0
    ref = allele.upper().encode()
    for o in ops:
        ln, op = int(o) >> 4, int(o) & 15
        if op == 0:
            a, b = seq[q:q + ln], ref[r:r + ln]
            mism += sum(1 for x, y in zip(a, b) if x != y or x == 78) + (ln - min(len(a), len(b)))
            q += ln; r += ln
        elif op == 1:
            xo += 1; xg += ln; q += ln
        elif op == 2:
            xo += 1; xg += ln; r += ln
        elif op == 4:
            q += ln
    return xo, xg, xg + mism


def sam_order(chosen, aln) -> np.ndarray:
    """the records' order in the file: by (position of the allele in `chosen`, pos0, read_index, strand, diag)"""
    slot = {int(a): k for k, a in enumerate(chosen)}
    ref = np.fromiter((slot[int(a)] for a in aln.allele), np.int64, len(aln))
    return np.lexsort((aln.diag, aln.flags & 1, aln.read_index, aln.pos0, ref))


def write_sam(path: str, idx: AlleleIndex, chosen, aln, paired: bool) -> int:
    """Write the records `aln` (engine.Alignments) of the chosen alleles (allele indices, in @SQ order) to `path`; paired: the
    sample was submitted as pairs.  Returns the number of records written.  The rules: the module's docstring."""
    chosen = [int(a) for a in chosen]
    order = sam_order(chosen, aln)
    n = len(aln)
    # the best record of every read: highest AS, ties to the first in file order
    rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    by_read = np.lexsort((rank, -aln.as_.astype(np.int64), aln.read_index))
    best = np.zeros(n, bool)
    if n:
        ri = aln.read_index[by_read]
        best[by_read[np.concatenate(([True], ri[1:] != ri[:-1]))]] = True
    qtab = bytes(min(q, 93) + 33 for q in range(256))
    seq_all, qual_all = aln.seq.tobytes(), aln.qual.tobytes().translate(qtab)
    with open(path, "w", newline="") as f:
        f.write("@HD\tVN:1.6\tSO:coordinate\n")
        for a in chosen:
            f.write("@SQ\tSN:%s\tLN:%d\n" % (idx.label(a), int(idx.off[a + 1] - idx.off[a])))
        f.write(PG_LINE + "\n")
        for k in order.tolist():
            a = int(aln.allele[k])
            ops = aln.cigar[int(aln.cigar_off[k]):int(aln.cigar_off[k + 1])]
            s0, s1 = int(aln.seq_off[k]), int(aln.seq_off[k + 1])
            seq = seq_all[s0:s1]
            ridx = int(aln.read_index[k])
            strand = int(aln.flags[k]) & 1
            xo, xg, nm = gap_figures(ops, seq, idx.sequence(a), int(aln.pos0[k]))
            f.write("r%d\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tAS:i:%d\tXS:i:%d\tXN:i:0\tXM:i:%d\tXO:i:%d\tXG:i:%d\tNM:i:%d\tYT:Z:UU\n" % (
                ridx >> 1 if paired else ridx, 16 * strand + (0 if best[k] else 256), idx.label(a), int(aln.pos0[k]) + 1,
                "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 15]) for o in ops), seq.decode("ascii"), qual_all[s0:s1].decode("ascii"),
                int(aln.as_[k]), int(aln.as_[k]), int(aln.xm[k]), xo, xg, nm))
    return n
