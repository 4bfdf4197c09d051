"""Command-line entry points with the reference's flags.

    python -m metamlst_amd.cli type  SAMPLE.fastq[.gz] [-2 MATES.fastq] -d DB [-o out] [--penalty ...]   (metamlst.py:34-49)
    python -m metamlst_amd.cli type  READS.bam -d DB [-o out]            (the reads of a BAM, as `samtools fastq` takes them)
    python -m metamlst_amd.cli type  LONG.fastq --long-reads [--tile LEN,STEP] -d DB   (reads longer than 320 bases, cut into windows)
    python -m metamlst_amd.cli type  HIFI.bam --long-bam-reads [--tile LEN,STEP] -d DB  (the same for the reads of an unaligned BAM)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam -d DB      (also <out>/<sample>.sam: the alignments to the chosen alleles)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam-all -d DB  (also <out>/<sample>.all.sam: every alignment, as bowtie2 -a would leave it)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam-all --read-names -d DB  (QNAME = the reads' own names, kept on the GPU)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam --write-sam-all --md -d DB  (both exports with bowtie2's MD:Z field)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-reads -d DB    (also <out>/<sample>.loci.fastq: the reads that align to the loci, as bowtie2 --al)
    python -m metamlst_amd.cli merge FOLDER -d DB [-z 5] [--filter ...] [--meta ...] [--idField ...] [--aligner auto|gpu|muscle]   (metamlst-merge.py:35-49)
    python -m metamlst_amd.cli index -d DB [-s seqs.fasta,...] [-t typings.txt,...] [-q dump.fa] [--list]   (metamlst-index.py:24-33)

`type` takes reads instead of a bowtie2 BAM: the alignment happens on the GPU.  Everything it
writes (<out>/<sample>.nfo, optional --log file) has the reference's format; `merge` writes
merged/<species>_ST.txt and _report.txt.  --presorted / --debug / --version of the reference have
no meaning here and are accepted and ignored."""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import time

from . import db as mdb
from .engine import CorruptInput, Engine, crc_checked, default_params
from .fastq import is_bgzf, mates_share_names, pair_chunks, prefetch, text_chunks, tile_fasta
from .index import load_index
from .merge import EngineAligner, EngineMatcher, _muscle, merge_folder
from .typing import TypingArgs, log_table, sample_name, type_sample


def _type_parser(sub):
    p = sub.add_parser("type", help="reconstruct the MLST loci of one sample from its reads (counterpart of metamlst.py)")
    p.add_argument("READS", nargs="+",
                   help="FASTQ file (plain, .gz or bgzip; `a.fq,b.fq` = two files of one sample, as bowtie2 -U takes them), or a BAM "
                        "whose records are taken as reads the way `samtools fastq` takes them (unaligned BAMs, `samtools view -f 4`; "
                        "a name-collated paired BAM is typed as pairs); with "
                        "--alignments: a SAM (plain or .gz) or BAM file.  Several files, or a folder of FASTQ files: every one is a "
                        "sample of its own, typed one after the other (with --gpus N: whole samples dealt to the GPUs, rank 0 "
                        "gathers the .nfo lines) -- the many-samples-into-one-folder use that metamlst-merge.py reads")
    p.add_argument("--alignments", action="store_true",
                   help="READS is a SAM / BAM made by `bowtie2 --very-sensitive-local -a --no-unal` against the database's "
                        "alleles (the reference's own input): hit accumulation as metamlst.py:101-130, pileup on the GPU")
    p.add_argument("--contigs", action="store_true",
                   help="READS is a FASTA of contigs or an assembled genome (the input of the reference's mlst.py): it is cut into "
                        "overlapping windows (--tile LEN,STEP) that go through the same path as reads")
    p.add_argument("--long-reads", dest="long_reads", action="store_true",
                   help="READS holds reads longer than the 320 bases a packed read takes (merged pairs, amplicons, ONT / HiFi): a record "
                        "longer than LEN is cut into overlapping windows (--tile LEN,STEP; 300,150 suits merged pairs) that keep their "
                        "slice of the quality line and are typed as unpaired reads of their own; shorter records are typed as they are")
    p.add_argument("--long-bam-reads", dest="long_bam_reads", action="store_true",
                   help="--long-reads for the reads of BAM files (PacBio HiFi, ONT, merged pairs kept as unaligned BAM): the reads "
                        "`samtools fastq` would write are cut into windows (--tile LEN,STEP) on the GPU; every READS file is a BAM "
                        "of unpaired reads, one sample each")
    p.add_argument("--tile", default="150,25", metavar="LEN,STEP")
    p.add_argument("-2", dest="mates",
                   help="second FASTQ of a paired-end sample: record k of it is the mate of record k of READS.  Mates are aligned as "
                        "unpaired reads (the documented pipeline is bowtie2 -U r1,r2); when the two files give a pair ONE read name "
                        "(checked on the first record) the pair counts once per locus in the coverage figures, as in the "
                        "reference's sequenceBank (metamlst.py:127)")
    p.add_argument("-o", metavar="OUTPUT FOLDER", default="./out")
    p.add_argument("-d", "--database", metavar="DB PATH", required=True)
    p.add_argument("--filter", metavar="species1,species2...")
    p.add_argument("--penalty", default=100, type=int)
    p.add_argument("--minscore", default=80, type=int)
    p.add_argument("--max_xM", default=5, type=int)
    p.add_argument("--min_read_len", default=50, type=int)
    p.add_argument("--min_accuracy", default=0.90, type=float)
    p.add_argument("--nloci", default=100, type=int)
    p.add_argument("--log", action="store_true")
    p.add_argument("-a", action="store_true", help="Write known sequences")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--presorted", action="store_true")
    p.add_argument("--device", default=0, type=int)
    p.add_argument("--gpus", default=1, type=int,
                   help="type the sample on N GPUs of this node: one process per GPU, FASTQ chunks dealt to the ranks, the statistics "
                        "and pileup counts all-reduced over RCCL (plain or .gz FASTQ; the .nfo is byte-identical to --gpus 1)")
    p.add_argument("--no-verify-crc", dest="verify_crc", action="store_false",
                   help="bgzip'd input: do not check the CRC-32 of the BGZF blocks.  By default every block's text is checked against "
                        "the CRC in its trailer before its reads are typed (on the GPU; the boundary blocks of a --gpus N shard on the "
                        "host), as zlib, htslib and `bgzip -d` do; a mismatch ends the sample with an error and no .nfo")
    p.add_argument("--write-sam", dest="write_sam", action="store_true",
                   help="after the .nfo, write <out>/<sample>.sam: the engine's alignments of the sample's reads to the alleles the "
                        "typing tail chose, as SAM text (metamlst_amd/samout.py: QNAME r<read index>, secondary records flagged 256, the "
                        "optional fields of bowtie2 with XS a placeholder).  One sample of reads on one GPU: it goes with none of "
                        "--alignments (the file is the input there), several samples or a folder, and --gpus N")
    p.add_argument("--write-sam-all", dest="write_sam_all", action="store_true",
                   help="after the .nfo, write <out>/<sample>.all.sam: EVERY alignment the engine decides -- each work item against every "
                        "allele of its locus, what `bowtie2 -a` leaves in front of metamlst.py -- as SAM text formatted on the GPU "
                        "(metamlst_amd/samout.py: one @SQ per loaded allele, XS:i only where the read has a second record).  Accepted and "
                        "refused where --write-sam is; both may be given")
    p.add_argument("--write-reads", dest="write_reads", action="store_true",
                   help="after the .nfo (and the SAM files), write <out>/<sample>.loci.fastq: the reads that have at least one alignment to "
                        "a locus -- what `bowtie2 --al` writes --, as FASTQ formatted on the GPU in ascending read index "
                        "(metamlst_amd/samout.py: reads_fastq_rule).  Names are those of the SAM exports (r<read index>, or the reads' own "
                        "with --read-names), with /1 and /2 when the sample is typed as pairs; SEQ / QUAL are the reads as they were "
                        "aligned (prepared and cut where --trim* / --adapter ran).  A mate is written only if it aligns itself.  Accepted "
                        "and refused where --write-sam is; the .nfo and the --log file do not change")
    p.add_argument("--read-names", dest="read_names", action="store_true",
                   help="with --write-sam / --write-sam-all / --write-reads: QNAME is the read's own name (the FASTQ header behind the @ up to the first "
                        "white space, bowtie2's rule) instead of r<read index>; the names of the reads on the loci are copied out of the "
                        "FASTQ text on the GPU.  A name that is no legal SAM QNAME keeps r<k>, and such reads are counted.  FASTQ input of "
                        "one sample on one GPU (plain, .gz, bgzip, `a.fq,b.fq`, -2): it goes with none of a reads BAM, --contigs, "
                        "--long-reads, --long-bam-reads, --alignments, a folder or several samples, and --gpus N.  The .nfo and the --log "
                        "file do not change")
    p.add_argument("--md", dest="md", action="store_true",
                   help="with --write-sam / --write-sam-all: every record also carries bowtie2's MD:Z field, between NM:i and YT:Z (the "
                        "allele's letters under the mismatching and deleted columns: metamlst_amd/samout.py, md_text), so that the reference "
                        "bases can be rebuilt from the record alone (samtools calmd -e, pysam get_reference_sequence).  --write-sam-all "
                        "formats it on the GPU.  Accepted and refused where the export flags are; it combines with --read-names.  The "
                        ".nfo and the --log file do not change")
    p.add_argument("--trim5", default=0, type=int, metavar="N",
                   help="FASTQ input: remove N bases from the 5' end of every read before it is aligned (bowtie2 -5 / --trim5), on the GPU "
                        "(csrc/read_prep.h; the rule: metamlst_amd.fastq.prep_fastq).  The four read preparation flags (--trim5, --trim3, "
                        "--trim-qual, --phred64) apply to plain, .gz and bgzip'd FASTQ, `a.fq,b.fq`, -2, a folder or several samples and "
                        "--gpus N; they go with none of --alignments, --contigs, --long-reads, --long-bam-reads and a reads BAM.  A read "
                        "left without a base stays a read (indices, pairing and --read-names are those of the file); the exports carry "
                        "the prepared SEQ / QUAL, as bowtie2 prints trimmed reads")
    p.add_argument("--trim3", default=0, type=int, metavar="N",
                   help="FASTQ input: remove N bases from the 3' end of every read before it is aligned (bowtie2 -3 / --trim3); see --trim5")
    p.add_argument("--trim-qual", dest="trim_qual", default=0, type=int, metavar="Q",
                   help="FASTQ input: then trim the 3' end of every read by quality with threshold Q (the rule of cutadapt -q Q and "
                        "bwa aln -q Q, no minimum length), behind --trim5 / --trim3; 0 (default) = off; see --trim5")
    p.add_argument("--phred64", action="store_true",
                   help="FASTQ input: the qualities are Phred+64 (Illumina 1.3 - 1.7, bowtie2 --phred64), not Phred+33.  Nothing detects "
                        "the base: without the flag such a file is typed with every quality 31 too high; see --trim5")
    p.add_argument("--adapter", default="", metavar="SEQ[,SEQ...]",
                   help="FASTQ input: remove a 3' adapter from every read before it is aligned, on the GPU (csrc/read_adapt.h; the rule: "
                        "metamlst_amd.fastq.adapter_cut, modelled on `cutadapt -a SEQ --no-indels`; it is the project's own and claims none "
                        "of cutadapt's bytes).  1 to 8 adapters of 1 to 64 letters of ACGTN; illumina (AGATCGGAAGAGC), nextera (CTGTCTCTTATA) "
                        "and smallrna (TGGAATTCTCGG) are taken in place of a sequence.  The adapter may lie inside the read or hang over "
                        "its 3' end; the start with the most matching letters within the error rate is cut, one adapter per read, each "
                        "mate on its own, behind --trim5 / --trim3 / --trim-qual.  Accepted and refused where those flags are; a read left "
                        "without a base stays a read, and the exports carry the cut SEQ / QUAL.  At the default minimum overlap of 3 about "
                        "2 %% of random 150-base reads lose three or more bases by chance (cutadapt's default and its known price): raise "
                        "--adapter-min-overlap where that matters")
    p.add_argument("--adapter-min-overlap", dest="adapter_min_overlap", default=None, type=int, metavar="N",
                   help="--adapter: an adapter that hangs over the 3' end must lie on at least N bases of the read (1 to 64, default 3)")
    p.add_argument("--adapter-error-rate", dest="adapter_error_rate", default=None, type=float, metavar="X",
                   help="--adapter: at most floor(X * overlap) letters of the overlap may differ (0 to 0.5, default 0.1; kept as "
                        "round(1000 * X) permille)")
    p.add_argument("--read-stats", dest="read_stats", action="store_true",
                   help="FASTQ input: count per-cycle quality and base tables of the sample's reads on the GPU, next to the parser "
                        "(csrc/read_stats.h; the rule: metamlst_amd.fastq.read_stats), as they stand in the file (raw) and, where --trim* / "
                        "--adapter ran, as they are aligned (prepared); R1 and R2 apart.  After the .nfo, write <out>/<sample>.readstats.tsv "
                        "(the format: metamlst_amd.fastq.read_stats_text; the project's own) and, unless --quiet, print one line per stage "
                        "and side, and a hint when the qualities look like the other Phred base.  One sample on one GPU: plain, .gz and "
                        "bgzip'd FASTQ, `a.fq,b.fq`, -2; refused with --alignments, --contigs, --long-reads, --long-bam-reads, a reads BAM, "
                        "a folder or several samples, and --gpus N.  The .nfo, the --log file and every export do not change")
    p.add_argument("--dedup", dest="dedup", action="store_true",
                   help="FASTQ input: remove exact duplicate reads before they are aligned, on the GPU (csrc/read_dedup.h; the rule: "
                        "metamlst_amd.fastq.dedup_fastq).  A read whose letters (A, C, G, T in either case, everything else N) and length "
                        "repeat an earlier read of the sample is emptied; with -2 the unit is the pair, and both mates must repeat, in "
                        "order.  The first occurrence stays; a reverse complement is no duplicate; qualities and names play no part.  It "
                        "runs behind --trim* / --adapter, on what they left.  A duplicate stays a read without a base (indices, pairing "
                        "and --read-names are those of the file) and appears in no export.  The keys live in a table on the GPU (28 bytes "
                        "per slot, at least two slots per read: 48 M reads end at 3.75 GB).  One sample on one GPU: plain, .gz and bgzip'd "
                        "FASTQ, `a.fq,b.fq`, -2; refused with --alignments, --contigs, --long-reads, --long-bam-reads, a reads BAM, a "
                        "folder or several samples, and --gpus N.  Unless --quiet, one line reports units, duplicates, bases removed and "
                        "how often the distinct reads occur")
    p.add_argument("--pair-overlap", dest="pair_overlap", action="store_true",
                   help="-2 MATES: trim adapter read-through from both mates of every pair before they are aligned, on the GPU "
                        "(csrc/read_overlap.h; the rule: metamlst_amd.fastq.pair_overlap / trim_pair_overlap, modelled on fastp's overlap "
                        "analysis without indels; it is the project's own and claims none of fastp's bytes).  When the insert is shorter "
                        "than the reads, both mates run through it into the adapter; the mates overlap as reverse complements, and the "
                        "overlap says where the insert ends, so no adapter sequence is needed and a tail of one base is found.  It runs "
                        "behind --trim* / --adapter and in front of --dedup; with --read-stats the prepared stage shows the cut reads.  An "
                        "insert shorter than the minimum overlap is not seen (that is --adapter's job), and two mates of one "
                        "low-complexity repeat can overlap at a wrong offset.  One sample on one GPU with -2: plain, .gz and bgzip'd mates "
                        "whose records share their names; refused without -2, with --alignments, --contigs, --long-reads, "
                        "--long-bam-reads, a reads BAM, a folder or several samples, and --gpus N.  Unless --quiet, one line reports pairs, "
                        "overlapping pairs, pairs cut, bases removed and the median insert of the overlapping pairs")
    p.add_argument("--pair-overlap-min", dest="pair_overlap_min", default=None, type=int, metavar="N",
                   help="--pair-overlap: the mates must lie on each other over at least N bases (8 to 320, default 30)")
    p.add_argument("--pair-overlap-diff", dest="pair_overlap_diff", default=None, type=int, metavar="N",
                   help="--pair-overlap: at most N letters of the overlap may differ (0 to 64, default 5)")
    p.add_argument("--pair-overlap-rate", dest="pair_overlap_rate", default=None, type=float, metavar="X",
                   help="--pair-overlap: and at most floor(X * overlap) of them (0 to 0.5, default 0.2; kept as round(1000 * X) permille)")
    p.add_argument("--trim-poly-g", dest="trim_poly_g", action="store_true",
                   help="FASTQ input: trim a tail of G from the 3' end of every read before it is aligned, on the GPU (csrc/read_filter.h; "
                        "the rule: metamlst_amd.fastq.poly_tail, modelled on fastp --trim_poly_g; it is the project's own and claims none of "
                        "fastp's bytes).  Two-colour machines (NovaSeq, NextSeq) call G where a cluster gives no signal, at high quality, so "
                        "--trim-qual does not see such a tail.  A tail is at least --poly-min bases long, begins on a G and holds at most one "
                        "other base per eight, five at the most; the longest such tail is cut.  It runs behind --trim* / --adapter / "
                        "--pair-overlap and in front of --dedup, each mate on its own.  Accepted and refused where --adapter is, a folder, "
                        "several samples and --gpus N included; a read left without a base stays a read.  Unless --quiet, one line reports "
                        "what this and the four read filters (--min-length, --max-n, --low-complexity, --min-mean-qual) did")
    p.add_argument("--trim-poly-x", dest="trim_poly_x", action="store_true",
                   help="FASTQ input: as --trim-poly-g, for a tail of any one letter of A, C, G and T (fastp --trim_poly_x); give one of the two")
    p.add_argument("--poly-min", dest="poly_min", default=None, type=int, metavar="N",
                   help="--trim-poly-g / --trim-poly-x: the shortest tail that is cut (1 to 320, default 10; at 10 about 0.005 %% of random "
                        "150-base reads lose a G tail by chance, 0.015 %% a tail of any letter; at 5, 0.5 %%)")
    p.add_argument("--min-length", dest="min_length", default=None, type=int, metavar="N",
                   help="FASTQ input: remove every read that the trims left with fewer than N bases (1 to 320; fastp --length_required), on "
                        "the GPU behind the tail trim.  A removed read stays a read without a base (indices, pairing and --read-names are "
                        "those of the file; its mate stays) and appears in no export; see --trim-poly-g")
    p.add_argument("--max-n", dest="max_n", default=None, type=int, metavar="N",
                   help="FASTQ input: remove every read that holds more than N bases other than A, C, G and T (fastp --n_base_limit); see --min-length")
    p.add_argument("--low-complexity", dest="low_complexity", default=None, type=int, metavar="PCT",
                   help="FASTQ input: remove every read of which fewer than PCT percent of the bases differ from the next one (1 to 100; "
                        "fastp --low_complexity_filter with --complexity_threshold PCT, whose default is 30); see --min-length")
    p.add_argument("--min-mean-qual", dest="min_mean_qual", default=None, type=int, metavar="Q",
                   help="FASTQ input: remove every read whose mean quality is below Q (1 to 93; fastp --average_qual); see --min-length")
    p.add_argument("--max-retained", default=0, type=int, metavar="READS", help="capacity of the on-locus read store (default 4 M)")
    p.add_argument("--max-items", default=0, type=int, metavar="ITEMS", help="capacity of the (read, locus, strand) work-item list (default 8 M)")
    p.add_argument("--max-pair-results", default=0, type=int, metavar="PAIRS", help="capacity of the (item, allele) result arena (default 256 M)")
    p.add_argument("--depth-cap", default=0, type=int, metavar="N",
                   help="an ORDER-FREE approximation of pysam's pileup(max_depth) (metaMLST_functions.py:255-259 runs with 8000): a consensus column "
                        "sees the first N alignment records that span it, in read-index order.  NOT bit-identical to pysam on deep samples: htslib drops "
                        "whole reads at their start position in the coordinate-sorted BAM (DESIGN.md section 6); 0 (default) = all records")
    return p


def _merge_parser(sub):
    p = sub.add_parser("merge", help="detect the ST of every sample in a folder of .nfo files (counterpart of metamlst-merge.py)")
    p.add_argument("folder")
    p.add_argument("-d", "--database", metavar="DB PATH", required=True)
    p.add_argument("--filter", metavar="species1,species2...")
    p.add_argument("-z", metavar="ED", default=5, type=int)
    p.add_argument("--meta", metavar="METADATA_PATH")
    p.add_argument("--idField", default=0, type=int)
    p.add_argument("--outseqformat", choices=["A", "A+", "B", "B+", "C", "C+"])
    p.add_argument("-j", metavar="subjectID,diet,age...")
    p.add_argument("--jgroup", action="store_true")
    p.add_argument("--aligner", choices=["auto", "gpu", "muscle"], default="auto",
                   help="what aligns the sequences of a locus that differ in length (--outseqformat A / A+): muscle = the MUSCLE binary, as "
                        "the reference; gpu = the engine's centre-star alignment (no MUSCLE needed; not MUSCLE's gap placement); auto = "
                        "muscle where one is installed, gpu otherwise")
    p.add_argument("--device", default=0, type=int)
    return p


def _index_parser(sub):
    p = sub.add_parser("index", help="build / extend a MetaMLST SQLite database (ingest half of metamlst-index.py; no bowtie2 index is needed)")
    p.add_argument("-t", "--typings")
    p.add_argument("-s", "--sequences")
    p.add_argument("-q", "--dump_db")
    p.add_argument("-i", "--buildindex", help="accepted and ignored: the GPU index is built from the database when it is loaded")
    p.add_argument("-d", "--database", metavar="DB PATH", required=True)
    p.add_argument("--list", action="store_true")
    p.add_argument("--filter", default=None)
    return p


def run_index(a) -> int:
    from . import dbbuild
    conn = dbbuild.open_db(a.database)
    if a.list:      # metamlst-index.py:80-86
        for key, label in mdb.db_getOrganisms(conn).items():
            print(key.ljust(30) + " " * 5 + label.ljust(30))
        return 0
    if a.sequences:
        for f, r in dbbuild.add_sequences(conn, a.sequences.split(",")).items():
            print("ADDING SEQUENCES %s Added %d seqs (%d skipped)" % (f, r["added"], len(r["skipped"])))
    if a.typings:
        for f, r in dbbuild.add_typings(conn, a.typings.split(",")).items():
            print("%d/%d PROFILES LOADED from %s" % (r["loaded"], r["lines"], f))
    if a.dump_db:
        print("%d sequences written to %s" % (dbbuild.dump_db_to_fasta(conn, a.dump_db, a.filter), a.dump_db))
    conn.commit()
    conn.close()
    return 0


FASTQ_SUFFIXES = (".fastq", ".fq", ".fastq.gz", ".fq.gz", ".fastq.bgz", ".fq.bgz")
FASTA_SUFFIXES = (".fa", ".fna", ".fasta", ".fas", ".fa.gz", ".fna.gz", ".fasta.gz", ".fas.gz")


def expand_samples(reads: list[str], contigs: bool = False) -> list[list[str]]:
    """READS arguments -> one list of files per sample (a folder contributes its FASTQ files in name order; contigs: its FASTA
    files -- assemblies, one sample each -- instead)."""
    out = []
    for r in reads:
        if os.path.isdir(r):
            out += [[os.path.join(r, f)] for f in sorted(os.listdir(r)) if f.endswith(FASTA_SUFFIXES if contigs else FASTQ_SUFFIXES)]
        else:
            out.append(r.split(",") if "," in r and not os.path.exists(r) else [r])
    return out


def _parse_tile(text: str):
    """--tile LEN,STEP -> (read_len, stride), None (said) when it is not two positive numbers"""
    try:
        read_len, stride = (int(x) for x in text.split(","))
        if read_len < 1 or stride < 1:
            raise ValueError
    except ValueError:
        print("--tile LEN,STEP takes two positive numbers, not %r" % text)
        return None
    return read_len, stride


def run_type(a, argv=None) -> int:
    tile = long_reads = long_bam = None
    if a.long_reads:
        if a.mates or a.alignments or a.contigs:
            print("--long-reads takes unpaired FASTQ: it goes with none of -2, --alignments and --contigs")
            return 1
        long_reads = _parse_tile(a.tile)
        if long_reads is None:
            return 1
        if long_reads[0] > 320:
            print("--tile LEN,STEP: a window of --long-reads holds at most 320 bases, not %d" % long_reads[0])
            return 1
    if a.long_bam_reads:
        if a.mates or a.alignments or a.contigs or a.long_reads or a.gpus > 1:
            print("--long-bam-reads takes the unpaired reads of BAM files on one GPU: it goes with none of -2, --alignments, --contigs, --long-reads and --gpus N")
            return 1
        long_bam = _parse_tile(a.tile)
        if long_bam is None:
            return 1
        if long_bam[0] > 320:
            print("--tile LEN,STEP: a window of --long-bam-reads holds at most 320 bases, not %d" % long_bam[0])
            return 1
    if a.contigs:
        if a.mates or a.alignments:
            print("--contigs takes assemblies (FASTA): it goes with neither -2 nor --alignments")
            return 1
        t = _parse_tile(a.tile)
        if t is None:
            return 1
        tile = (t[0], t[1], a.min_read_len)
    samples = expand_samples(a.READS, contigs=bool(a.contigs))
    if not samples:
        print("no %s file found in " % ("FASTA" if a.contigs else "FASTQ") + ", ".join(a.READS))
        return 1
    many = len(samples) > 1
    if a.read_names:      # (refused before any GPU use, each with its reason)
        if _refused("--read-names: ", (
                (a.alignments, "with --alignments the file is the input, and its records carry their names already"),
                (many, "it names the reads of one sample's export: several samples or a folder are typed without exports"),
                (a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1, "the exports take one GPU, so do the names (not --gpus N)"),
                (a.contigs, "--contigs cuts assemblies into windows, and a window has no name"),
                (a.long_reads, "--long-reads cuts reads into windows, and a window has no name"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and a window has no name"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp), "the names of a reads BAM are not carried to the exports: FASTQ input only"),
                (not (a.write_sam or a.write_sam_all or a.write_reads), "it names the reads of an export: give --write-sam or --write-sam-all"))):
            return 1
    read_prep = _read_prep_of(a)
    if read_prep is not None:      # (refused before any GPU use, each with its reason)
        if read_prep is False:
            return 1
        if _refused("read preparation (--trim5, --trim3, --trim-qual, --phred64): ", (
                (a.alignments, "with --alignments the records are what they are: the file holds alignments, not reads to prepare"),
                (a.contigs, "--contigs cuts assemblies into windows, and a window is cut from the sequence as it stands"),
                (a.long_reads, "--long-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp),
                 "a reads BAM stores raw Phred and its own strand, and its reads are not prepared: FASTQ input only"))):
            return 1
    adapters = _adapters_of(a)
    if adapters is not None:      # (refused before any GPU use, each with its reason)
        if adapters is False:
            return 1
        if _refused("--adapter: ", (
                (a.alignments, "with --alignments the records are what they are: the file holds alignments, not reads to cut"),
                (a.contigs, "--contigs cuts assemblies into windows, and an assembly carries no adapter"),
                (a.long_reads, "--long-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp),
                 "the reads of a BAM are taken as they are stored: FASTQ input only"))):
            return 1
    read_filter = _read_filter_of(a)
    if read_filter is not None:      # (refused before any GPU use, each with its reason)
        if read_filter is False:
            return 1
        if _refused("read filter (--trim-poly-g, --trim-poly-x, --min-length, --max-n, --low-complexity, --min-mean-qual): ", (
                (a.alignments, "with --alignments the records are what they are: the file holds alignments, not reads to trim or remove"),
                (a.contigs, "--contigs cuts assemblies into windows, and an assembly has neither tails nor qualities"),
                (a.long_reads, "--long-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp),
                 "the reads of a BAM are taken as they are stored: FASTQ input only"))):
            return 1
    if getattr(a, "read_stats", False):      # (refused before any GPU use, each with its reason)
        if _refused("--read-stats: ", (
                (a.alignments, "with --alignments the file holds alignments, not the reads of a FASTQ file"),
                (a.contigs, "--contigs cuts assemblies into windows, and an assembly has neither cycles nor qualities"),
                (a.long_reads, "--long-reads cuts reads into windows, and the tables hold the 320 cycles of a short read"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and the tables hold the 320 cycles of a short read"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp), "the reads of a BAM are not counted: FASTQ input only"),
                (many, "it reports one sample: several samples or a folder are typed without it"),
                (a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1, "the tables are one GPU's: a rank of --gpus N counts its own share of the reads only"))):
            return 1
    if getattr(a, "dedup", False):      # (refused before any GPU use, each with its reason)
        if _refused("duplicate removal (--dedup): ", (
                (a.alignments, "with --alignments the file holds alignments, not reads to compare (duplicate alignments are samtools markdup's)"),
                (a.contigs, "--contigs cuts assemblies into windows, and the windows of an assembly are not copies of a molecule"),
                (a.long_reads, "--long-reads cuts reads into windows, and the windows of a read would be compared, not the read"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and the windows of a read would be compared, not the read"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp), "the reads of a BAM are not compared: FASTQ input only"),
                (many, "one table of keys per engine: several samples or a folder are typed without it (per-sample tables through the pipelined loop are the follow-up)"),
                (a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1, "a rank of --gpus N sees only its byte range, and duplicates across ranks would be missed"))):
            return 1
    pair_overlap = _pair_overlap_of(a)
    if pair_overlap is not None:      # (refused before any GPU use, each with its reason)
        if pair_overlap is False:
            return 1
        if _refused("--pair-overlap: ", (
                (a.alignments, "with --alignments the file holds alignments, not mates to lay on each other"),
                (a.contigs, "--contigs cuts assemblies into windows, and a window has no mate"),
                (a.long_reads, "--long-reads cuts unpaired reads into windows, and a window has no mate"),
                (a.long_bam_reads, "--long-bam-reads cuts unpaired reads into windows, and a window has no mate"),
                (not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp), "the mates of a BAM are taken as they are stored: FASTQ input with -2 only"),
                (many, "several samples or a folder are typed without it (the rule is per pair: summing the counters of the samples is the follow-up)"),
                (a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1, "one GPU: the counters of the ranks of --gpus N are not summed yet (the follow-up)"),
                (not a.mates, "it lays the mates of a pair on each other: give the second file with -2"),
                (bool(a.mates) and len(samples[0]) > 1, "it takes one file of first mates and one of second mates (-2), not `a.fq,b.fq`"))):
            return 1
        try:
            if not mates_share_names(samples[0][0], a.mates):
                print("--pair-overlap: the records of %s and %s do not share their names, so the files go in as two unpaired texts and no read has a mate" % (samples[0][0], a.mates))
                return 1
        except OSError as e:
            print("--pair-overlap: %s" % e)
            return 1
    if a.md and not (a.write_sam or a.write_sam_all):      # (with an export flag it is accepted and refused where that flag is: below)
        print("--md: it adds MD:Z to the records of an export: give --write-sam or --write-sam-all")
        return 1
    for flag in [f for f, on in (("--write-sam", a.write_sam), ("--write-sam-all", a.write_sam_all), ("--write-reads", a.write_reads)) if on]:      # (refused before any GPU use)
        if a.alignments:
            print(flag + " writes the engine's own alignments: with --alignments the file is the input")
            return 1
        if many:
            print(flag + " takes one sample: several samples or a folder are typed without it")
            return 1
        if a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            print(flag + " takes one GPU: a rank of --gpus N holds its own reads' alignments only")
            return 1
    if many and (a.alignments or a.mates):
        print("several samples at once: FASTQ input only (use `r1.fq,r2.fq` for a sample made of two files)")
        return 1
    a.READS, extra_files = samples[0][0], samples[0][1:]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    has_bam = not a.alignments and not a.contigs and any(_is_reads_bam(f) for smp in samples for f in smp)
    if has_bam and a.long_reads:
        print("--long-reads takes FASTQ: the long reads of a BAM are cut into windows by --long-bam-reads")
        return 1
    if a.long_bam_reads:      # every file a BAM of unpaired reads: windows are unpaired reads of their own
        from .samin import bam_first_read_flags
        for f in (f for smp in samples for f in smp):
            if not _is_reads_bam(f):
                print("--long-bam-reads takes BAM files: %s is none (FASTQ goes with --long-reads)" % f)
                return 1
            flags = bam_first_read_flags(f)
            if flags is not None and flags & 1:
                print("--long-bam-reads takes unpaired reads: the first read of %s carries FLAG 0x1 (a paired BAM is typed as pairs without the switch)" % f)
                return 1
    if has_bam and a.mates:
        print("-2 names the second FASTQ file of a pair: the mates of a BAM are records of the BAM itself (collate it by name)")
        return 1
    if a.gpus > 1 and world == 1:
        if a.alignments or (a.contigs and not many) or has_bam:      # (a folder of assemblies is dealt to the ranks, one assembly is not cut up)
            print("--gpus applies to FASTQ input")
            return 1
        from .multigpu import launch_ranks
        return launch_ranks(a.gpus, list(argv if argv is not None else sys.argv[1:]))      # before this process touches a GPU
    rank, device = 0, None
    if world > 1:
        from .multigpu import init_from_env
        rank, world, device = init_from_env()
        a.device = device.index
    try:
        database = mdb.metaMLST_db(a.database)
        idx = load_index(a.database, a.filter.split(",") if a.filter else None)
    except Exception as e:   # metamlst.py:73-75
        print("Failed to connect to the database: please check your database file! (%s)" % e)
        return 1
    prm = default_params()
    prm.minscore, prm.max_xm, prm.min_read_len = a.minscore, a.max_xM, a.min_read_len
    prm.max_retained_reads, prm.max_items, prm.max_pair_results = a.max_retained, a.max_items, a.max_pair_results
    if a.depth_cap and world > 1 and not many:
        print("--depth-cap orders the records of the whole sample by read index: one sample on several GPUs cannot apply it (use --gpus 1)")
        return 1
    eng = Engine(a.device, prm)
    eng.set_bgzf_verify(a.verify_crc)
    if long_reads or long_bam:
        eng.set_read_tiling(*(long_reads or long_bam))
    if a.read_names:      # (FASTQ input only: text, host-inflated .gz and BGZF all reach the device as text, where the names are kept)
        eng.set_read_names(True)
    _apply_read_chain(eng, a, read_prep, adapters, pair_overlap, read_filter)      # (the same entries; before a rank's first read index base)
    # the built host index is kept next to the database (as the reference keeps <idx>.1.bt2: metamlst-index.py:224-225) unless a
    # species filter made this index a one-off or MLST_INDEX_CACHE=0
    ref_cache = (a.database + ".mlstref") if (not a.filter and os.environ.get("MLST_INDEX_CACHE", "1") != "0") else ""
    eng.load_reference(idx, cache_path=ref_cache)
    from . import fastq as _fq
    from .engine import pinned_array
    _fq.set_buffer_allocator(pinned_array)      # file chunks are read into page-locked buffers
    if a.depth_cap:
        eng.set_depth_cap(a.depth_cap)
    engines = [eng]
    if many:      # the pipelined loop (metamlst_amd/pipeline.py): a few engines take turns on this rank's samples
        n_mine = (len(samples) + world - 1) // world
        # six engines: a sample of a few million reads is a chain of short device stages (copy, inflate, parse, pass 1, allele choice,
        # pile-up: 10-15 ms end to end, most of it latency) -- 16 bgzip'd samples of 2 M reads: 4 / 6 / 8 engines = 265 / 300 / 290 Mreads/s
        # (profiles/round5/inflate.md 6)
        for _ in range(max(0, min(int(os.environ.get("MLST_PIPELINE_DEPTH", "6")), n_mine) - 1)):
            e2 = Engine(a.device, prm)
            e2.load_reference(idx)      # (the host index is cached inside the library: an upload, not a build)
            e2.set_bgzf_verify(a.verify_crc)
            if long_reads or long_bam:
                e2.set_read_tiling(*(long_reads or long_bam))
            _apply_read_chain(e2, a, read_prep, adapters, pair_overlap, read_filter)      # (the switches refused for several samples are off)
            if a.depth_cap:
                e2.set_depth_cap(a.depth_cap)
            engines.append(e2)
    targs = TypingArgs(penalty=a.penalty, minscore=a.minscore, max_xM=a.max_xM, min_read_len=a.min_read_len,
                       min_accuracy=a.min_accuracy, nloci=a.nloci, a=a.a, quiet=a.quiet, filter=a.filter, log=a.log)
    chunk_bytes = int(os.environ.get("MLST_FASTQ_CHUNK", str(256 << 20)))
    if many:
        from .multigpu import type_many_samples
        prep_info = {"shortened": 0, "bases_removed": 0, "emptied": 0} if read_prep and not a.quiet else None
        adapt_info = {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0] * len(adapters["adapters"])} if adapters and not a.quiet else None
        filter_info = _sum_filter_infos([]) if read_filter and not a.quiet else None
        rc = type_many_samples(engines, idx, database, targs, samples, rank, world, a.o, a.log, chunk_bytes,
                               printer=None if a.quiet else (lambda results: _print_results(a, results)), tile=tile, long_reads=long_reads,
                               long_bam_reads=long_bam, read_prep_info=prep_info, read_adapters_info=adapt_info, read_filter_info=filter_info)
        if prep_info is not None:
            _say_read_prep(prep_info, world)
        if adapt_info is not None:
            _say_read_adapters(adapt_info, adapters["adapters"], world)
        if filter_info is not None:
            print(read_filter_line(filter_info, world), flush=True)
        database.closeConnection()
        return rc
    if a.alignments:
        from .engine import HostPathNeeded
        from .samin import AlignmentSample, BamSample, SamSample, is_bgzf_bam, is_sam_text, read_sam_header
        # a BGZF BAM: inflate, record split, accumulation and pile-up on the device; SAM text (plain or .gz): line table, parse,
        # accumulation and pile-up on the device (two passes over the file either way).  SAM text without @SQ lines gives the
        # device no names to look an RNAME up in: its first record would come back as "host path needed", so the host reader
        # takes such a file at once, as before
        Device = BamSample if is_bgzf_bam(a.READS) else SamSample if is_sam_text(a.READS) and read_sam_header(a.READS) else None
        if Device is not None:
            def said(e):      # which path typed the sample is the user's to know: the host reader is ~10^3 times slower
                print("%s: %s -- reading the file on the host instead" % (a.READS, str(e).split(": ", 1)[-1]), file=sys.stderr)

            def device_pileup(chosen):
                try:
                    return crc_checked([a.READS], lambda: bam.pileup(eng, chosen))
                except HostPathNeeded as e:      # (pass 2 only: a BAM's AS / XM tag by name that is no integer, a SAM line's QUAL.  The statistics stay
                    said(e)                      # the device's -- pass 1 treated every record; the host reader is built for the pile-up alone)
                    return AlignmentSample(idx, targs).add_file(a.READS).pileup(eng, chosen)
            try:
                bam = crc_checked([a.READS], lambda: Device(idx, targs, eng).add_file(a.READS))
                return _finish_type(a, idx, database, targs, bam.stats(), device_pileup)
            except HostPathNeeded as e:      # a record only the host reader treats: today's path, which raises or answers as the reference
                said(e)
                eng.reset_sample()
            except CorruptInput as e:   # nothing of the sample is typed: no .nfo
                print(e, file=sys.stderr)
                database.closeConnection()
                return 1
        smp = AlignmentSample(idx, targs).add_file(a.READS)
        return _finish_type(a, idx, database, targs, smp.stats(), lambda chosen: smp.pileup(eng, chosen))
    if a.contigs:      # the file's bytes go to the GPU and are cut into windows there (mlst_submit_fasta)
        submit_contigs(eng, a.READS, tile)
        return _finish_type_device(a, eng, idx, database, targs, paired=False)
    # Mates are unpaired reads for the aligner (bowtie2 -U r1,r2).  What a shared read name changes is sequenceBank
    # (metamlst.py:127: one entry per QNAME and locus): pairs whose files name both mates alike are submitted as pairs.
    paired = bool(a.mates) and mates_share_names(a.READS, a.mates)
    paths = [a.READS] + extra_files + ([a.mates] if a.mates else [])
    if world > 1:      # this rank's share of the files, then the two all-reduces; rank 0 writes (metamlst_amd/multigpu.py)
        from .multigpu import submit_fastq_shard, type_sharded
        try:
            submit_fastq_shard(eng, paths, rank, world, chunk_bytes, paired=paired, verify_crc=a.verify_crc)
        except CorruptInput as e:      # (this rank ends with an error: the command ends the others and returns its status)
            print("rank %d: %s" % (rank, e), file=sys.stderr, flush=True)
            os._exit(1)      # the other ranks wait in a collective: no orderly shutdown of the process group
        fileName = sample_name(a.READS)
        if rank == 0 and not os.path.isdir(a.o):
            os.mkdir(a.o)
        log_path = (a.o + "/" + fileName + "_" + str(int(time.time())) + ".out") if a.log else None
        results = type_sharded(eng, idx, database, targs, rank, world, device, fileName, a.o, log_path, a.READS)
        if rank == 0 and not a.quiet:
            _print_results(a, results)
        database.closeConnection()
        import torch.distributed as dist
        if read_prep:      # one line for the sample: the ranks' counters, summed
            box = [None] * world
            dist.all_gather_object(box, eng.read_prep_info())
            if rank == 0 and not a.quiet:
                _say_read_prep({key: sum(b[key] for b in box) for key in box[0]}, 1)
        if adapters:
            box = [None] * world
            dist.all_gather_object(box, eng.read_adapters_info())
            if rank == 0 and not a.quiet:
                _say_read_adapters(_sum_adapter_infos(box), adapters["adapters"], 1)
        if read_filter:
            box = [None] * world
            dist.all_gather_object(box, eng.read_filter_info())
            if rank == 0 and not a.quiet:
                print(read_filter_line(_sum_filter_infos(box)), flush=True)
        dist.destroy_process_group()
        return 0
    # FASTQ text goes to the GPU as is and is parsed there (mlst_submit_fastq); a reader thread stays two chunks ahead
    try:
        # --read-stats: mates whose names differ go in as unpaired text, the mate file counted into side 1 (R1 and R2 are reported apart)
        side1_from = len(paths) - 1 if (getattr(a, "read_stats", False) and a.mates and not paired) else None
        submit_sample_files(eng, paths, paired, chunk_bytes, report=None if a.quiet else print, long_reads=long_reads, long_bam_reads=long_bam, side1_from=side1_from)
    except CorruptInput as e:      # nothing of the sample is typed: no .nfo
        print(e, file=sys.stderr)
        database.closeConnection()
        return 1
    if (a.write_sam or a.write_sam_all or a.write_reads) and not paired and not (long_reads or long_bam) and all(_is_reads_bam(f) for f in paths):      # (as submit_bam_reads decides it)
        from .samin import bam_first_read_flags
        paired = any((bam_first_read_flags(f) or 0) & 1 for f in paths)
    return _finish_type_device(a, eng, idx, database, targs, paired=paired)


def _finish_type_device(a, eng, idx, database, targs, paired: bool = False) -> int:
    """Allele choice (metamlst.py:133-151, 244), pile-up and majority consensus on the device, queued behind pass 1
    (mlst_typing_enqueue): one host synchronisation per sample instead of three (statistics, host choice, pile-up).
    --write-sam: then the alignments to the alleles chosen there, as <out>/<sample>.sam (paired: the reads were submitted as pairs);
    --write-sam-all: then every alignment, as <out>/<sample>.all.sam;
    --write-reads: then the reads that have an alignment, as <out>/<sample>.loci.fastq."""
    eng.typing_enqueue(penalty=targs.penalty)
    st, chosen, letters = eng.typing_fetch()
    rc = _finish_type(a, idx, database, targs, st, None, typed=(chosen, letters))
    if rc == 0 and not a.quiet and _read_prep_of(a):
        _say_read_prep(eng.read_prep_info(), 1)
    if rc == 0 and not a.quiet and _adapters_of(a, say=False):
        _say_read_adapters(eng.read_adapters_info(), eng.get_read_adapters()["adapters"], 1)
    if rc == 0 and not a.quiet and _read_filter_of(a, say=False):
        print(read_filter_line(eng.read_filter_info()), flush=True)
    if rc == 0 and not a.quiet and _pair_overlap_of(a, say=False):
        print(read_pair_overlap_line(eng.read_pair_overlap_info()), flush=True)
    if rc == 0 and getattr(a, "read_stats", False):
        _write_read_stats(a, eng)
    if rc == 0 and not a.quiet and getattr(a, "dedup", False):
        print(read_dedup_line(eng.read_dedup_info(), paired), flush=True)
    names, md = None, bool(getattr(a, "md", False))      # --md: MD:Z in both exports (write_sam on the host, the full export on the device)
    if rc == 0 and getattr(a, "read_names", False):      # the engine knows its switch: the text export needs no more than that
        names = eng.read_names()
        info = eng.read_names_info()
        if not a.quiet:
            print("--read-names: %d reads on the loci keep their names, %d have a name that is no legal QNAME and keep r<k>" % (info["named"], info["fallbacks"]))
    if rc == 0 and a.write_sam:
        from .samout import write_sam
        alleles = [chosen[l] for l in sorted(chosen)]
        write_sam(a.o + "/" + sample_name(a.READS) + ".sam", idx, alleles, eng.export_alignments(alleles), paired, names=names, md=md)
    if rc == 0 and a.write_sam_all:
        from .samout import write_sam_all
        write_sam_all(a.o + "/" + sample_name(a.READS) + ".all.sam", idx, eng, paired, md=md)
    if rc == 0 and getattr(a, "write_reads", False):
        from .samout import write_reads
        n_written = write_reads(a.o + "/" + sample_name(a.READS) + ".loci.fastq", eng, paired)
        if not a.quiet:
            print("--write-reads: %d reads with an alignment written" % n_written)
    return rc


def _refused(prefix: str, rows) -> bool:
    """says the first reason of rows ((holds, sentence), ...) that holds, behind prefix"""
    for on, why in rows:
        if on:
            print(prefix + why)
            return True
    return False


def _apply_read_chain(eng, a, read_prep, adapters, pair_overlap, read_filter=None) -> None:
    """The switches of the read chain as the command was given them: the reads are prepared, cut, counted and compared
    where the FASTQ text is parsed"""
    if read_prep:
        eng.set_read_prep(**read_prep)
    if adapters:
        eng.set_read_adapters(**adapters)
    if getattr(a, "read_stats", False):
        eng.set_read_stats(True)
    if getattr(a, "dedup", False):
        eng.set_read_dedup(True)
    if pair_overlap:
        eng.set_read_pair_overlap(True, **pair_overlap)
    if read_filter:
        eng.set_read_filter(**read_filter)


def _read_prep_of(a):
    """The four read preparation flags -> the arguments of Engine.set_read_prep, None when none is given, False (said) when one is
    out of range"""
    t5, t3, tq, p64 = getattr(a, "trim5", 0), getattr(a, "trim3", 0), getattr(a, "trim_qual", 0), bool(getattr(a, "phred64", False))
    if not (t5 or t3 or tq or p64):
        return None
    for flag, v, top in (("--trim5", t5, 65535), ("--trim3", t3, 65535), ("--trim-qual", tq, 93)):
        if not 0 <= v <= top:
            print("%s takes a number from 0 to %d, not %d" % (flag, top, v))
            return False
    return {"trim5": t5, "trim3": t3, "trim_qual": tq, "phred64": p64}


def _say_read_prep(info: dict, world: int) -> None:
    """The line on what the read preparation did (info: Engine.read_prep_info(), summed over the samples of a folder; a rank of --gpus N
    speaks for its own reads)"""
    n, m, k = info["shortened"], info["bases_removed"], info["emptied"]
    rank = (" (the samples of rank %s of %d)" % (os.environ.get("RANK", "0"), world)) if world > 1 else ""
    print("read preparation: %d reads shortened, %d bases removed, %d reads left without a base%s" % (n, m, k, rank), flush=True)


def _adapters_of(a, say: bool = True):
    """--adapter, --adapter-min-overlap, --adapter-error-rate -> the arguments of Engine.set_read_adapters, None when --adapter is not
    given, False (said) when a flag is out of range or given without --adapter"""
    from .fastq import ADAPTER_NAMES, check_adapters
    spec, mo, er = getattr(a, "adapter", ""), getattr(a, "adapter_min_overlap", None), getattr(a, "adapter_error_rate", None)
    if not spec:
        for flag, v in (("--adapter-min-overlap", mo), ("--adapter-error-rate", er)):
            if v is not None:
                if say:
                    print(flag + " belongs to --adapter: give the adapter it applies to")
                return False
        return None
    try:
        if er is not None and not 0 <= er <= 0.5:
            raise ValueError("--adapter-error-rate takes a number from 0 to 0.5, not %r" % er)
        permille = 100 if er is None else int(round(1000 * er))
        ads = check_adapters([ADAPTER_NAMES.get(x.strip().lower(), x.strip()) for x in spec.split(",")], 3 if mo is None else mo, permille)
    except ValueError as e:
        if say:
            print("--adapter: %s" % e)
        return False
    return {"adapters": [x.decode() for x in ads], "min_overlap": 3 if mo is None else mo, "error_permille": permille}


def _pair_overlap_of(a, say: bool = True):
    """--pair-overlap, --pair-overlap-min, --pair-overlap-diff, --pair-overlap-rate -> the arguments of Engine.set_read_pair_overlap, None
    when --pair-overlap is not given, False (said) when a flag is out of range or given without --pair-overlap"""
    from .fastq import check_pair_overlap
    mo, mm, er = getattr(a, "pair_overlap_min", None), getattr(a, "pair_overlap_diff", None), getattr(a, "pair_overlap_rate", None)
    if not getattr(a, "pair_overlap", False):
        for flag, v in (("--pair-overlap-min", mo), ("--pair-overlap-diff", mm), ("--pair-overlap-rate", er)):
            if v is not None:
                if say:
                    print(flag + " belongs to --pair-overlap: give the switch it applies to")
                return False
        return None
    try:
        if er is not None and not 0 <= er <= 0.5:
            raise ValueError("--pair-overlap-rate takes a number from 0 to 0.5, not %r" % er)
        out = {"min_overlap": 30 if mo is None else mo, "max_mismatches": 5 if mm is None else mm, "error_permille": 200 if er is None else int(round(1000 * er))}
        check_pair_overlap(**out)
    except ValueError as e:
        if say:
            print("--pair-overlap: %s" % e)
        return False
    return out


def _read_filter_of(a, say: bool = True):
    """--trim-poly-g, --trim-poly-x, --poly-min, --min-length, --max-n, --low-complexity, --min-mean-qual -> the arguments of
    Engine.set_read_filter, None when none of them is given, False (said) when a flag is out of range, --poly-min stands alone or both
    tail switches are given"""
    from .fastq import check_read_filter
    g, x, pm = bool(getattr(a, "trim_poly_g", False)), bool(getattr(a, "trim_poly_x", False)), getattr(a, "poly_min", None)
    ml, mn, lc, mq = (getattr(a, k, None) for k in ("min_length", "max_n", "low_complexity", "min_mean_qual"))

    def no(text: str):
        if say:
            print(text)
        return False
    if g and x:
        return no("--trim-poly-x trims G tails too: give one of the two")
    if pm is not None and not (g or x):
        return no("--poly-min belongs to --trim-poly-g / --trim-poly-x: give the switch it applies to")
    if not (g or x) and ml is None and mn is None and lc is None and mq is None:
        return None
    for flag, v, lo, hi in (("--poly-min", pm, 1, 320), ("--min-length", ml, 1, 320), ("--max-n", mn, 0, 0xFFFFFFFE), ("--low-complexity", lc, 1, 100), ("--min-mean-qual", mq, 1, 93)):
        if v is not None and not lo <= v <= hi:
            return no("%s takes a number from %d to %d, not %d" % (flag, lo, hi, v))
    out = {"poly": "G" if g else "ACGT" if x else "", "poly_min": 10 if pm is None else pm, "min_length": ml or 0, "max_n": mn, "complexity": lc or 0, "mean_qual": mq or 0}
    check_read_filter(out["poly"], out["poly_min"], out["min_length"], out["max_n"], out["complexity"], out["mean_qual"])
    return out


def _sum_filter_infos(infos) -> dict:
    """Engine.read_filter_info() of several engines or ranks, added up (none: all zero)"""
    out = {"tail_trimmed": 0, "tail_bases": 0, "per_letter": [0, 0, 0, 0], "tail_emptied": 0, "failed_short": 0, "failed_n": 0, "failed_complexity": 0,
           "failed_quality": 0, "filtered_bases": 0}
    for b in infos:
        for key, v in b.items():
            out[key] = [p + q for p, q in zip(out[key], v)] if key == "per_letter" else out[key] + v
    return out


def read_filter_line(info: dict, world: int = 1) -> str:
    """The line on what the tail trim and the read filters did (info: Engine.read_filter_info() or fastq.filter_fastq's counters, summed
    over the samples of a folder; a rank of --gpus N then speaks for its own samples)"""
    failed = [int(info[k]) for k in ("failed_short", "failed_n", "failed_complexity", "failed_quality")]
    rank = (" (the samples of rank %s of %d)" % (os.environ.get("RANK", "0"), world)) if world > 1 else ""
    return ("read filter: %d poly tails trimmed (A %d, C %d, G %d, T %d), %d bases removed, %d reads left without a base; %d reads removed "
            "(%d too short, %d with too many N, %d of low complexity, %d of low quality), %d bases"
            % (int(info["tail_trimmed"]), *[int(v) for v in info["per_letter"]], int(info["tail_bases"]), int(info["tail_emptied"]), sum(failed), *failed,
               int(info["filtered_bases"]))) + rank


def read_pair_overlap_line(info: dict) -> str:
    """The line on what --pair-overlap did (info: Engine.read_pair_overlap_info() or fastq.trim_pair_overlap's counters): pairs,
    overlapping pairs and their share of the pairs to one decimal (in integers, rounded half up), pairs cut, bases removed, reads left
    without a base, and the median insert of the overlapping pairs (fastq.pair_overlap_median; left out when no pair overlaps)"""
    from .fastq import pair_overlap_median
    pairs, ov = int(info["pairs"]), int(info["overlapping"])
    tenths = (1000 * ov + pairs // 2) // pairs if pairs else 0
    line = ("mate overlap trimming: %d pairs, %d overlapping (%d.%d %%), %d pairs cut (%d reads), %d bases removed, %d reads left without a base"
            % (pairs, ov, tenths // 10, tenths % 10, int(info["trimmed_pairs"]), int(info["reads_trimmed"]), int(info["bases_removed"]), int(info["emptied"])))
    if ov:
        line += "; median insert of the overlapping pairs %d" % pair_overlap_median(info["insert_hist"])
    return line


def read_dedup_line(info: dict, paired: bool = False) -> str:
    """The line on what --dedup did (info: Engine.read_dedup_info() or fastq.dedup_fastq's counters): units seen, duplicates and their
    share of the units to one decimal (in integers, rounded half up), bases removed, the eight levels, and the clashes only when there
    are some"""
    units, dups = int(info["units"]), int(info["duplicates"])
    tenths = (1000 * dups + units // 2) // units if units else 0
    lv = info["levels"]
    line = ("duplicate removal: %d %s, %d duplicates (%d.%d %%), %d bases removed; distinct %d: x1 %d, x2 %d, x3 %d, x4 %d, x5-9 %d, x10-49 %d, x50-499 %d, x500+ %d"
            % (units, "pairs" if paired else "reads", dups, tenths // 10, tenths % 10, int(info["bases_removed"]), int(info["distinct"]), *[int(v) for v in lv]))
    if info.get("clashes"):
        line += "; %d kept on a 64-bit clash" % int(info["clashes"])
    return line


def read_stats_lines(stats: dict) -> list:
    """One line per counted stage and side of Engine.read_stats(): reads, bases, mean length, share of bases >= Q20 and >= Q30, GC %,
    share of non-ACGT bases"""
    out = []
    for stage in ["raw"] + (["prepared"] if stats.get("prepared_counted") else []):
        for side in (0, 1):
            t = stats[stage][side]
            reads, bases = int(t["reads"]), int(t["bases"])
            if side and not reads:
                continue
            q = t["qual"].sum(axis=0)
            b = t["base"].sum(axis=0)
            d = max(bases, 1)
            out.append("read statistics (%s, side %d): %d reads, %d bases, mean length %.1f, >= Q20 %.1f %%, >= Q30 %.1f %%, GC %.1f %%, non-ACGT %.2f %%"
                       % (stage, side, reads, bases, bases / max(reads, 1), 100.0 * int(q[20:].sum()) / d, 100.0 * int(q[30:].sum()) / d,
                          100.0 * int(b[1] + b[2]) / d, 100.0 * int(b[4]) / d))
    return out


def _write_read_stats(a, eng) -> None:
    """--read-stats: <out>/<sample>.readstats.tsv (fastq.read_stats_text) and, unless --quiet, the lines and the Phred hint"""
    from .fastq import phred_hint, read_stats_text
    stats = eng.read_stats()
    name = sample_name(a.READS)
    with open(a.o + "/" + name + ".readstats.tsv", "wb") as f:
        f.write(read_stats_text(stats, name))
    if not a.quiet:
        for line in read_stats_lines(stats):
            print(line, flush=True)
    hint = phred_hint(stats)
    if hint:
        print(hint, flush=True)


def _sum_adapter_infos(infos) -> dict:
    """Engine.read_adapters_info() of several engines or ranks, added up"""
    out = {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0] * len(infos[0]["per_adapter"])}
    for b in infos:
        for key in ("trimmed", "bases_removed", "emptied"):
            out[key] += b[key]
        out["per_adapter"] = [x + y for x, y in zip(out["per_adapter"], b["per_adapter"])]
    return out


def _say_read_adapters(info: dict, adapters: list, world: int) -> None:
    """The line on what --adapter did (info: Engine.read_adapters_info(), summed over the samples of a folder; a rank of --gpus N speaks
    for its own samples)"""
    rank = (" (the samples of rank %s of %d)" % (os.environ.get("RANK", "0"), world)) if world > 1 else ""
    per = ", ".join("%s %d" % (s, n) for s, n in zip(adapters, info["per_adapter"]))
    print("adapter removal: %d reads cut, %d bases removed, %d reads left without a base (%s)%s"
          % (info["trimmed"], info["bases_removed"], info["emptied"], per, rank), flush=True)


class _FileReader:
    """prefetch(text_chunks(path, reuse=True)) whose buffers go back to the pool when the consumer says it is done (close)."""

    def __init__(self, path: str, chunk_bytes: int, lo: int = 0, hi=None):
        self.ring: list = []
        self.it = prefetch(text_chunks(path, chunk_bytes, lo, hi, reuse=True, ring=self.ring))

    def __iter__(self):
        return self.it

    def close(self) -> None:
        from .fastq import release_buffers
        release_buffers(self.ring)


def open_sample_reader(paths, paired: bool, chunk_bytes: int):
    """The reader thread of a sample's FIRST file, started now (None when that file is not plain or gzip FASTQ text): a caller
    with many samples opens sample k + 1 before it feeds sample k, and k + 1's first chunks are read meanwhile."""
    if paired or not paths or is_bgzf(paths[0]):
        return None
    return _FileReader(paths[0], chunk_bytes)


def _is_reads_bam(path: str) -> bool:
    from .samin import is_bgzf_bam
    return os.path.isfile(path) and is_bgzf_bam(path)


def submit_bam_reads(eng, path: str, report=None, long_reads=None) -> int:
    """The reads of a BGZF BAM into one engine (Engine.submit_bam_reads_file): as pairs iff the first record kept carries FLAG 0x1
    (decided on the first record, as mates_share_names does for mate files).  report: called with one line on what was taken.
    long_reads = (read_len, stride): the reads are unpaired and those longer than read_len are cut into windows on the GPU
    (Engine.set_read_tiling); the line then says how many were cut into how many windows."""
    from .samin import bam_first_read_flags
    flags = bam_first_read_flags(path)
    paired = bool(flags is not None and flags & 1)
    if long_reads is not None:
        if paired:
            raise ValueError("long BAM reads are unpaired: the first read of %s carries FLAG 0x1" % path)
        if eng.get_read_tiling() != tuple(long_reads):
            eng.set_read_tiling(*long_reads)
        before = eng.read_tiling_info()
    n = crc_checked([path], lambda: eng.submit_bam_reads_file(path, paired=paired))
    if report is not None:
        _, n_sec, n_empty, _ = eng.bam_reads_info()
        line = "%s: %d reads taken%s, %d secondary / supplementary and %d empty records skipped" % (path, n, " as pairs" if paired else "", n_sec, n_empty)
        if long_reads is not None:
            info = eng.read_tiling_info()
            line += ", %d longer than %d cut into %d windows" % (info["cut"] - before["cut"], long_reads[0], info["windows"] - before["windows"])
        report(line)
    return n


def submit_contigs(eng, path: str, tile) -> int:
    """The contigs of one FASTA file into one engine as overlapping windows, tile = (read_len, stride, min_len): cut and packed on
    the GPU (Engine.submit_fasta_file).  A file with a sequence line only Python's strip() treats (HostPathNeeded) is said so on
    stderr and tiled on the host instead (tile_fasta, the statement of the rules).  Returns the reads submitted."""
    from .engine import HostPathNeeded
    read_len, stride, min_len = tile
    try:
        return eng.submit_fasta_file(path, read_len, stride, min_len)[1]
    except HostPathNeeded as e:      # which path typed the sample is the user's to know
        print("%s: %s -- reading the file on the host instead" % (path, str(e).split(": ", 1)[-1]), file=sys.stderr, flush=True)
        eng.reset_sample()
    n = 0
    for chunk in tile_fasta(path, read_len, stride, min_len):
        n += eng.submit_fastq(chunk, paired=False)
    return n


def submit_sample_files(eng, paths, paired: bool, chunk_bytes: int, first_reader=None, report=None, tile=None, long_reads=None,
                        long_bam_reads=None, side1_from=None) -> None:
    """All reads of one sample's file(s) into one engine: FASTQ (first_reader: open_sample_reader(paths, ...), if opened ahead), or
    BAMs whose records are taken as reads (report: see submit_bam_reads).  tile = (read_len, stride, min_len): the files are
    assemblies (FASTA), cut into windows on the GPU (submit_contigs).  long_reads = (read_len, stride): unpaired FASTQ whose records
    longer than read_len are cut into windows on the GPU (Engine.set_read_tiling: plain text and bgzip on the device path, single-
    stream .gz inflated on the host as always and cut on the device); report gets one line on what was cut.  long_bam_reads =
    (read_len, stride): the files are BAMs of unpaired reads, cut into windows the same way (submit_bam_reads).  side1_from = k: under
    Engine.set_read_stats the unpaired files from paths[k] on count into side 1 (a mate file whose names differ from its first file's)."""
    if long_bam_reads is not None:
        if paired or not all(_is_reads_bam(p) for p in paths):
            raise ValueError("long BAM reads are the unpaired reads of BAM files")
        for path in paths:
            submit_bam_reads(eng, path, report, long_reads=long_bam_reads)
        return
    if tile is not None:
        for path in paths:
            submit_contigs(eng, path, tile)
        return
    if long_reads is not None:
        if paired or any(_is_reads_bam(p) for p in paths):
            raise ValueError("long reads are unpaired FASTQ: neither mate files nor a BAM")
        if eng.get_read_tiling() != tuple(long_reads):
            eng.set_read_tiling(*long_reads)
        submit_sample_files(eng, paths, False, chunk_bytes, first_reader=first_reader)
        if report is not None:
            info = eng.read_tiling_info()
            report("%s: %d records, %d longer than %d cut into %d windows" % (",".join(paths), info["records"], info["cut"], long_reads[0], info["windows"]))
        return
    if paired and is_bgzf(paths[0]) and is_bgzf(paths[1]):      # bgzip'd mates: inflated and paired on the GPU
        crc_checked(paths, lambda: eng.submit_fastq_bgzf_pair_files(paths[0], paths[1]))
        return
    if paired:
        from .fastq import release_buffers
        ring: list = []
        for c1, c2 in prefetch(pair_chunks(paths[0], paths[1], chunk_bytes // 2, reuse=True, ring=ring)):
            eng.submit_fastq_pair(c1, c2)
        release_buffers(ring)
        return
    for k, path in enumerate(paths):
        if side1_from is not None and k == side1_from:
            eng.set_read_stats_side(1)
        if _is_reads_bam(path):      # a BAM that holds reads: inflated, chosen, strand-corrected and packed on the GPU
            submit_bam_reads(eng, path, report)
            continue
        if is_bgzf(path):      # bgzip'd FASTQ: the compressed blocks go to the GPU and are inflated there
            crc_checked([path], lambda: eng.submit_fastq_bgzf_file(path, paired=False))
            continue
        reader = first_reader if (k == 0 and first_reader is not None) else _FileReader(path, chunk_bytes)
        for chunk in reader:
            eng.submit_fastq(chunk, paired=False)      # (returns when the chunk has left the host buffer)
        reader.close()


def _finish_type(a, idx, database, targs, st, pileup_fn, typed=None) -> int:
    fileName = sample_name(a.READS)
    if not os.path.isdir(a.o):
        os.mkdir(a.o)
    if a.log:   # metamlst.py:159-172
        with open(a.o + "/" + fileName + "_" + str(int(time.time())) + ".out", "w", newline="") as f:
            f.write(log_table(idx, st, targs, a.READS))
    results = type_sample(idx, st, pileup_fn, database, fileName, targs, out_dir=a.o, typed=typed)
    if not a.quiet:
        _print_results(a, results)
    database.closeConnection()
    return 0


def _print_results(a, results) -> None:
    for r in results:
        print(" %-18s Detected Loci: %s" % (r.species, ", ".join(r.detected)))
        if r.missing:
            print(" " * 20 + "Missing Loci : " + ", ".join(r.missing))
        for g, (avg, hits, alleles, cov) in sorted(r.closest.items()):
            print("  %-7s%15s%7s%6s  %s" % (g, cov, avg, hits, ",".join(alleles[:5]) + ("... (%d more)" % len(alleles) if len(alleles) > 5 else "")))
        for l in r.loci_report:
            print("  %-7s%-7s%7s%7s%7s%15s%10s" % (l["locus"], l["ref"], l["length"], l["ns"], l["snps"], l["confidence"], l["notes"]))
        print("  -> " + ("Reconstruction Successful [WRITE]" if r.written else
                         ("Accuracy lower than %s%% [SKIP]" % round(a.min_accuracy * 100, 2) if r.passed_nloci else "not enough loci [SKIP]")))


def run_merge(a) -> int:
    database = mdb.metaMLST_db(a.database)
    idx = load_index(a.database)
    eng = Engine(a.device)
    eng.load_reference(idx)
    use_muscle = a.aligner == "muscle" or (a.aligner == "auto" and shutil.which("muscle") is not None)
    align, name = (_muscle, "MUSCLE") if use_muscle else (EngineAligner(eng), "the GPU engine (centre-star)")

    def aligner(seqs):
        sys.stderr.write("aligner: %s on %d sequences\n" % (name, len(seqs)))
        return align(seqs)

    tables = merge_folder(a.folder, database, EngineMatcher(eng, idx), z=a.z, filter=a.filter, meta=a.meta, idField=a.idField,
                          cache=mdb.DbCache(database.conn, idx), outseqformat=a.outseqformat, j=a.j, jgroup=a.jgroup, aligner=aligner)
    for sp, t in tables.items():
        print("%s: %d sample(s) typed, %d new profile(s)" % (sp, len(t["isolates"]), sum(1 for v in t["encounteredProfiles"].values() if v[2] in (1, 2))))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="metamlst_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    _type_parser(sub)
    _merge_parser(sub)
    _index_parser(sub)
    a = ap.parse_args(argv)
    if a.cmd == "type":
        return run_type(a, argv)
    return {"merge": run_merge, "index": run_index}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())
