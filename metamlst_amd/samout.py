"""The engine's alignments as SAM text and its aligned reads as FASTQ (`cli type --write-sam` / `--write-sam-all` / `--write-reads`;
DESIGN.md section 6).

The reference leaves a BAM of each sample's reads on the MLST loci behind (the bowtie2 run in front of metamlst.py); here the
alignments are the engine's own, exported as records by Engine.export_alignments (mlst_alignments_export, include/mlst.h) and
formatted on the host by `write_sam(path, idx, chosen, aln, paired)`:

  * header: `@HD VN:1.6 SO:coordinate`, one `@SQ SN:<species>_<gene>_<allele> LN:<len>` per chosen allele in the order given
    (the names samin resolves: AlleleIndex.label), one `@PG` line;
  * records sorted by (position of the allele in `chosen`, pos0, read_index, strand, diag): the file's bytes do not depend on
    the order the device exported them in;
  * QNAME `r<k>`: k is the read index, or read_index >> 1 when the sample was submitted as pairs -- the mates then share a name,
    as sequenceBank wants (metamlst.py:127).  No pairing flags, as with bowtie2 -U.  Under --long-reads / --long-bam-reads /
    --contigs the reads are windows and k is the window's index.  With `--read-names` (Engine.set_read_names; FASTQ input only) the
    QNAME of both exports is the read's own name, `read_qname` below: the engine copies the names of the reads it retains out of the
    FASTQ text on the device (csrc/read_names.h) and hands `write_sam` the map {read index: name}; a name that is no legal QNAME
    keeps `r<k>`.  Every read carries its own name, mates included: the product submits mates as pairs only when their names are
    equal (fastq.mates_share_names), so "one entry per QNAME per locus" holds as it does with `r<k>`;
  * FLAG 16 * strand, plus 256 on every record of a read (a read index, not a QNAME) except its best one: the highest AS, ties
    to the first in the sort order above;
  * MAPQ 255, RNEXT *, PNEXT 0, TLEN 0; POS = pos0 + 1; SEQ as exported (reference strand); QUAL chr(min(q, 93) + 33);
  * optional fields in this order: AS:i XS:i XN:i:0 XM:i XO:i XG:i NM:i YT:Z:UU -- XM stands in the 15th column, which the
    reference reads by position (Q1).  AS and XM are the engine's true values.  XS carries the record's OWN AS: a documented
    placeholder (with -a over near-identical alleles every record has an equal-scoring sibling, and only records to the
    chosen alleles are exported).  XO (gap opens: I and D runs), XG (gap extensions: I and D bases) and NM (XG + the M
    columns whose SEQ letter is not the allele's, an N on either side included) are computed here from the CIGAR and the
    allele text.

EVERY alignment of the sample (`cli type --write-sam-all`, `write_sam_all(path, idx, eng, paired)`): what `bowtie2 -a` leaves in
front of metamlst.py, with the records formatted on the device (Engine.export_sam_text: mlst_alignments_text_open / _next / _close,
csrc/aln_text.h) and only the header written here.  The rule, which `format_record` and `all_records_rule` below state in plain
Python (they are the specification and the tests' yardstick; the command never calls them):

  * records: one for every (work item, allele of the item's locus) whose alignment, decided exactly as pass 1 decides that pair
    (the ungapped one, or the banded one where the gap trigger fires: align_pair of the oracle), has score >= the floor of the
    read's length and score > 0 -- the records pass 1 counts in MLST_CNT_TOTAL_RECORDS.  Records that fail the AS / XM tag filter
    are written too; mlst_set_depth_cap is ignored;
  * header: `@HD VN:1.6 SO:unsorted GO:query`, one `@SQ SN:<label> LN:<len>` for EVERY loaded allele in index order (what bowtie2
    writes and mlst_sam_open needs), the `@PG` line;
  * order: work items by (read index, locus index, strand, diag), inside an item the alleles ascending.  All records of a read are
    consecutive, two loci first seen in the same read keep locus order, and the bytes depend neither on the order of the item list
    nor on the size of the rounds the text leaves the device in;
  * columns 1-11 as above (QNAME r<k>, MAPQ 255, * 0 0, SEQ on the reference strand, QUAL chr(min(q, 93) + 33)); FLAG 16 * strand,
    plus 256 on every record of a read index except its best one: the highest AS, ties to the first in file order;
  * optional fields `AS:i [XS:i] XN:i:0 XM:i XO:i XG:i NM:i YT:Z:UU`.  XS:i is there iff the read index has two records or more in
    the file, and is the highest AS among the read's OTHER records.  A read with one record has no XS field, so XO stands in the
    15th column: Q1 by construction, as with bowtie2.  AS and XM are the true values; XO, XG and NM are `gap_figures` of the record.

MD:Z (`cli type --md`, `md=True` below; off by default): both exports then write bowtie2's `MD:Z:<text>` between `NM:i` and
`YT:Z:UU`, bowtie2's place -- columns 12 and 15 stay where they are, so Q1 and the positional parse of metamlst.py see what they
saw.  The text is `md_text` below: the match runs' lengths, the allele's letter under every M column that counts towards NM, `^` and
the allele's letters of every D run.  With SEQ and the CIGAR it gives the allele's bases under the record back, so a record stands
for itself (samtools calmd -e, pysam get_reference_sequence) without the allele FASTA.  `write_sam` formats it here; the full
export formats it on the device (Engine.set_export_md: mlst_set_export_md, csrc/aln_text.h).

THE READS THEMSELVES (`cli type --write-reads`, `write_reads(path, eng, paired)`): the reads that align to the loci as FASTQ, what
`bowtie2 --al FILE` writes and `samtools fastq` makes of the BAM in front of metamlst.py, formatted on the device
(Engine.export_reads_text: mlst_reads_text_open / _next / _close, csrc/reads_text.h).  The rule, which `reads_fastq_rule` below states
in plain Python (the device is held to it byte for byte; the command never calls it):

  * which reads: a read index is written iff it has at least one record in the full export above -- "aligned at least once".  Records
    that fail the AS / XM tag filter count, mlst_set_depth_cap is ignored, and a retained read without a record is not written;
  * order: ascending read index, each read once, however many records it has;
  * record: four lines with LF ends, `@<name>\n<SEQ>\n+\n<QUAL>\n`.  <name> is the QNAME of the SAM exports (r<k>, or under
    --read-names the kept name and r<k> for a fallback); when the sample was submitted as pairs `/1` follows for an even read index and
    `/2` for an odd one -- the mates share a QNAME there, and a FASTQ must tell them apart.  SEQ is the read as the engine holds it, in
    read orientation and never turned to the reference strand (the prepared, cut read where --trim* / --adapter ran): ACGT, and N for
    every other letter.  QUAL is chr(min(q, 93) + 33) of the stored Phred, `_QUAL_TAB`;
  * mates: each mate is written on its own, and only if it has a record itself.  The engine does not retain a mate that hit nothing, so
    the file is no `--al-conc`: the unaligned mate of an aligned read is not in it.

Not written: BAM / BGZF, the names of a reads BAM or of windows, pairing flags, the mate that hit nothing, reads without a record,
gzip'd FASTQ, the original letter case and IUPAC codes."""
from __future__ import annotations

import numpy as np

from .index import AlleleIndex
from .samin import CIGAR_OPS

PG_LINE = "@PG\tID:metamlst_amd\tPN:metamlst_amd"
_QUAL_TAB = bytes(min(q, 93) + 33 for q in range(256))      # raw Phred -> QUAL character


def read_qname(header_line: bytes, k: int) -> bytes:
    """The QNAME of a read under --read-names, from its FASTQ header line (with or without its line end): the bytes behind the `@`
    up to, not including, the first space, TAB, CR or LF (bowtie2's rule, and fastq.mates_share_names').  A name that is no legal SAM
    QNAME -- `[!-?A-~]{1,254}`: empty, longer than 254 bytes, an `@` or a byte outside `!`..`~` in it -- gives `r<k>`, as without the
    switch; k = the read index, or read index >> 1 when the sample was submitted as pairs.  The specification of csrc/read_names.h
    and the tests' yardstick; the command never calls it."""
    name = bytes(header_line)[1:]
    for i, c in enumerate(name):
        if c in b" \t\r\n":
            name = name[:i]
            break
    if 1 <= len(name) <= 254 and all(0x21 <= c <= 0x7E and c != 0x40 for c in name):
        return name
    return b"r%d" % int(k)


def _qname(ridx: int, paired: bool, names) -> str:
    """QNAME of read index ridx: its name in `names` (a mapping read index -> bytes, or None), else r<k>"""
    nm = names.get(int(ridx)) if names is not None else None
    return nm.decode("ascii") if nm else "r%d" % (int(ridx) >> 1 if paired else int(ridx))


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


def md_text(ops, seq: bytes, allele: str, pos0: int) -> str:
    """The MD:Z text of one record (arguments as gap_figures takes them): the specification of the device's text and the tests'
    yardstick.  The CIGAR is walked in reference orientation with q into SEQ, r = pos0 into the upper-cased allele and a match run u:
      * an M column matches iff SEQ[q] == REF[r] and SEQ[q] != 'N' -- the predicate of NM (gap_figures; csrc/aln_text.h:
        at_col_differs) and of samtools calmd, where an N on either side is a mismatch.  A match: u += 1.  Otherwise u in decimal, then
        the letter REF[r], and u = 0;
      * a D run: u (also when it is 0), then `^` and the run's allele letters, and u = 0;
      * I and S runs advance q only and do not break the match run;
      * at the end: u (also when it is 0).
    So the text always matches [0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*: the 0 between two neighbouring mismatches, and between a deletion and a
    mismatch behind it, is no special case.  An allele byte that is not A-Z after upper-casing is written as N.  That can happen:
    dbbuild.add_sequences stores a FASTA record's sequence lines as they are and AlleleIndex hands the bytes on unchanged (the engine
    packs every byte outside ACGT as an N column), so `-`, `*`, `.` or a digit in a database's FASTA reaches this function."""
    ref = allele.upper().encode()
    out, u = [], 0
    q, r = 0, int(pos0)
    for o in ops:
        ln, op = int(o) >> 4, int(o) & 15
        if op == 0:
            for k in range(ln):
                x, y = seq[q + k], ref[r + k]
                if x == y and x != 78:
                    u += 1
                else:
                    out.append("%d%s" % (u, chr(y) if 65 <= y <= 90 else "N"))
                    u = 0
            q += ln; r += ln
        elif op == 2:
            out.append("%d^%s" % (u, "".join(chr(y) if 65 <= y <= 90 else "N" for y in ref[r:r + ln])))
            u = 0; r += ln
        elif op in (1, 4):
            q += ln
    out.append("%d" % u)
    return "".join(out)


def sam_order(chosen, aln) -> np.ndarray:
    """the records' order in the file: by (position of the allele in `chosen`, pos0, read_index, strand, diag)"""
    slot = {int(a): k for k, a in enumerate(chosen)}
    ref = np.fromiter((slot[int(a)] for a in aln.allele), np.int64, len(aln))
    return np.lexsort((aln.diag, aln.flags & 1, aln.read_index, aln.pos0, ref))


def write_sam(path: str, idx: AlleleIndex, chosen, aln, paired: bool, names=None, md: bool = False) -> int:
    """Write the records `aln` (engine.Alignments) of the chosen alleles (allele indices, in @SQ order) to `path`; paired: the
    sample was submitted as pairs; names: {read index: name (bytes)} of Engine.read_names() -- a read in it gets its name as QNAME,
    None gives r<k> throughout; md: MD:Z:<md_text> between NM:i and YT:Z:UU.  Returns the number of records written.  The rules: the
    module's docstring."""
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
            mdz = "\tMD:Z:" + md_text(ops, seq, idx.sequence(a), int(aln.pos0[k])) if md else ""
            f.write("%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tAS:i:%d\tXS:i:%d\tXN:i:0\tXM:i:%d\tXO:i:%d\tXG:i:%d\tNM:i:%d%s\tYT:Z:UU\n" % (
                _qname(ridx, paired, names), 16 * strand + (0 if best[k] else 256), idx.label(a), int(aln.pos0[k]) + 1,
                "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 15]) for o in ops), seq.decode("ascii"), qual_all[s0:s1].decode("ascii"),
                int(aln.as_[k]), int(aln.as_[k]), int(aln.xm[k]), xo, xg, nm, mdz))
    return n


# ------------------------------------------------------------------ every alignment (--write-sam-all)
def sam_all_header(idx: AlleleIndex) -> str:
    """the header of the full export: every loaded allele, in index order"""
    sq = "".join("@SQ\tSN:%s\tLN:%d\n" % (idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles))
    return "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + sq + PG_LINE + "\n"


def format_record(idx: AlleleIndex, rec, paired: bool, secondary: bool, xs, names=None, md: bool = False) -> bytes:
    """One line of the full export.  rec = (read index, strand, diag, locus, allele, pos0, AS, XM, CIGAR ops (len << 4 | op), SEQ
    (ASCII, reference strand), QUAL (raw Phred)); secondary: not the best record of its read index; xs: the highest AS among the
    read's other records, None when it has no other record (no XS:i field then); names: {read index: name (bytes)} or None (r<k>);
    md: MD:Z:<md_text> between NM:i and YT:Z:UU."""
    ridx, strand, _diag, _locus, a, pos0, as_, xm, ops, seq, qual = rec
    xo, xg, nm = gap_figures(ops, bytes(seq), idx.sequence(int(a)), int(pos0))
    cols = [_qname(ridx, paired, names), "%d" % (16 * int(strand) + (256 if secondary else 0)), idx.label(int(a)), "%d" % (int(pos0) + 1), "255",
            "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 15]) for o in ops), "*", "0", "0", bytes(seq).decode("ascii"),
            bytes(qual).translate(_QUAL_TAB).decode("ascii"), "AS:i:%d" % int(as_)]
    if xs is not None:
        cols.append("XS:i:%d" % int(xs))
    cols += ["XN:i:0", "XM:i:%d" % int(xm), "XO:i:%d" % xo, "XG:i:%d" % xg, "NM:i:%d" % nm]
    if md:
        cols.append("MD:Z:" + md_text(ops, bytes(seq), idx.sequence(int(a)), int(pos0)))
    cols.append("YT:Z:UU")
    return ("\t".join(cols) + "\n").encode("ascii")


def all_records_rule(idx: AlleleIndex, recs, paired: bool, names=None, md: bool = False) -> list:
    """The lines of the full export for a sample's records (tuples as format_record takes them, in any order): sorted by (read
    index, locus, strand, diag, allele); per read index the best record (highest AS, ties to the first in that order) is the one
    without 256, and XS is the highest AS among the others.  names: {read index: name (bytes)} under --read-names, None: r<k>;
    md: the records carry MD:Z."""
    order = sorted(recs, key=lambda r: (int(r[0]), int(r[3]), int(r[1]), int(r[2]), int(r[4])))
    out, k = [], 0
    while k < len(order):
        e = k
        while e < len(order) and int(order[e][0]) == int(order[k][0]):
            e += 1
        scores = [int(r[6]) for r in order[k:e]]
        best = scores.index(max(scores))
        for t, r in enumerate(order[k:e]):
            others = scores[:t] + scores[t + 1:]
            out.append(format_record(idx, r, paired, t != best, max(others) if others else None, names, md))
        k = e
    return out


def write_sam_all(path: str, idx: AlleleIndex, eng, paired: bool, round_bytes: int = 0, md: bool = False) -> int:
    """Write every alignment of the sample on `eng` to `path`: the header here, the records as the device formats them, round by
    round (md: with MD:Z, formatted there too).  Returns the number of records written."""
    n = 0
    with open(path, "wb") as f:
        f.write(sam_all_header(idx).encode("ascii"))
        for chunk in eng.export_sam_text(idx, paired=paired, round_bytes=round_bytes, md=md):
            f.write(chunk)
            n += chunk.count(b"\n")
    return n


# ------------------------------------------------------------------ the reads that align to the loci (--write-reads)
_SEQ_TAB = bytes(c if c in b"ACGT" else (c - 32 if c in b"acgt" else 78) for c in range(256))      # the letters the engine holds: ACGT, else N


def reads_fastq_rule(reads, aligned, paired: bool, names=None) -> list:
    """The records of the reads export, one `bytes` of four lines per written read, in file order.  reads: read index -> (bases as
    ASCII, raw Phred bytes) of the read as the engine holds it (a mapping or a sequence; the prepared, cut read where the engine
    prepared it); aligned: the read indices that have a record in the full export, in any order and with repeats (one per record will
    do); paired: the sample was submitted as pairs; names: {read index: name (bytes)} under --read-names, None: r<k>.  The
    specification of csrc/reads_text.h and the tests' yardstick; the command never calls it."""
    out = []
    for ri in sorted(set(int(r) for r in aligned)):
        bases, quals = reads[ri]
        name = _qname(ri, paired, names).encode("ascii") + ((b"/2" if ri & 1 else b"/1") if paired else b"")
        out.append(b"@" + name + b"\n" + bytes(bases).translate(_SEQ_TAB) + b"\n+\n" + bytes(quals).translate(_QUAL_TAB) + b"\n")
    return out


def write_reads(path: str, eng, paired: bool, round_bytes: int = 0) -> int:
    """Write the reads of the sample on `eng` that have an alignment to `path` as FASTQ, as the device formats them, round by round
    (a sample without such a read gets an empty file).  Returns the number of reads written."""
    n = 0
    with open(path, "wb") as f:
        for chunk in eng.export_reads_text(paired=paired, round_bytes=round_bytes):
            f.write(chunk)
            n += chunk.count(b"\n") // 4
    return n
