"""Command-line entry points with the reference's flags.

    python -m metamlst_amd.cli type  SAMPLE.fastq[.gz] [-2 MATES.fastq] -d DB [-o out] [--penalty ...]   (metamlst.py:34-49)
    python -m metamlst_amd.cli type  READS.bam -d DB [-o out]            (the reads of a BAM, as `samtools fastq` takes them)
    python -m metamlst_amd.cli type  LONG.fastq --long-reads [--tile LEN,STEP] -d DB   (reads longer than 320 bases, cut into windows)
    python -m metamlst_amd.cli type  HIFI.bam --long-bam-reads [--tile LEN,STEP] -d DB  (the same for the reads of an unaligned BAM)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam -d DB      (also <out>/<sample>.sam: the alignments to the chosen alleles)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam-all -d DB  (also <out>/<sample>.all.sam: every alignment, as bowtie2 -a would leave it)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam-all --read-names -d DB  (QNAME = the reads' own names, kept on the GPU)
    python -m metamlst_amd.cli type  SAMPLE.fastq --write-sam --write-sam-all --md -d DB  (both exports with bowtie2's MD:Z field)
    python -m metamlst_amd.cli type  SAMPLE.fastq --cut-front 1,3 --cut-tail 1,3 --cut-right 4,15 --min-length 36 -d DB  (Trimmomatic's quality recipe, on the GPU)
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
from functools import reduce

from . import db as mdb, read_chain
from .read_chain import _read_filter_of, _sum_filter_infos, read_dedup_line, read_filter_line, read_pair_overlap_line, read_stats_lines, read_window_line  # noqa: F401
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
    read_chain.add_arguments(p)      # (the flags of the seven read chain stages: --trim5 ... --min-mean-qual)
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
    world = int(os.environ.get("WORLD_SIZE", "1"))
    gpus = a.gpus > 1 or world > 1
    reads_bam = not a.alignments and any(_is_reads_bam(f) for smp in samples for f in smp)      # (every file is opened once, here)
    if a.read_names:      # (refused before any GPU use, each with its reason)
        if _refused("--read-names: ", (
                (a.alignments, "with --alignments the file is the input, and its records carry their names already"),
                (many, "it names the reads of one sample's export: several samples or a folder are typed without exports"),
                (gpus, "the exports take one GPU, so do the names (not --gpus N)"),
                (a.contigs, "--contigs cuts assemblies into windows, and a window has no name"),
                (a.long_reads, "--long-reads cuts reads into windows, and a window has no name"),
                (a.long_bam_reads, "--long-bam-reads cuts reads into windows, and a window has no name"),
                (reads_bam, "the names of a reads BAM are not carried to the exports: FASTQ input only"),
                (not (a.write_sam or a.write_sam_all or a.write_reads), "it names the reads of an export: give --write-sam or --write-sam-all"))):
            return 1
    chain = read_chain.parse(a, samples, reads_bam, world)      # (the seven stages: refused before any GPU use, each with its reason)
    if chain is None:
        return 1
    if a.md and not (a.write_sam or a.write_sam_all):      # (with an export flag it is accepted and refused where that flag is: below)
        print("--md: it adds MD:Z to the records of an export: give --write-sam or --write-sam-all")
        return 1
    for flag in [f for f, on in (("--write-sam", a.write_sam), ("--write-sam-all", a.write_sam_all), ("--write-reads", a.write_reads)) if on]:      # (refused before any GPU use)
        if _refused(flag, ((a.alignments, " writes the engine's own alignments: with --alignments the file is the input"),
                           (many, " takes one sample: several samples or a folder are typed without it"),
                           (gpus, " takes one GPU: a rank of --gpus N holds its own reads' alignments only"))):
            return 1
    if many and (a.alignments or a.mates):
        print("several samples at once: FASTQ input only (use `r1.fq,r2.fq` for a sample made of two files)")
        return 1
    a.READS, extra_files = samples[0][0], samples[0][1:]
    has_bam = reads_bam and not a.contigs
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
    read_chain.apply(eng, chain)      # (the same entries; before a rank's first read index base)
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
            read_chain.apply(e2, chain)      # (the switches refused for several samples are off)
            if a.depth_cap:
                e2.set_depth_cap(a.depth_cap)
            engines.append(e2)
    targs = TypingArgs(penalty=a.penalty, minscore=a.minscore, max_xM=a.max_xM, min_read_len=a.min_read_len,
                       min_accuracy=a.min_accuracy, nloci=a.nloci, a=a.a, quiet=a.quiet, filter=a.filter, log=a.log)
    chunk_bytes = int(os.environ.get("MLST_FASTQ_CHUNK", str(256 << 20)))
    if many:
        from .multigpu import type_many_samples
        sums = {} if a.quiet else read_chain.zeros(chain)      # (the counters of the stages that sum over samples: filled by the feeders)
        rc = type_many_samples(engines, idx, database, targs, samples, rank, world, a.o, a.log, chunk_bytes,
                               printer=None if a.quiet else (lambda results: _print_results(a, results)), tile=tile, long_reads=long_reads,
                               long_bam_reads=long_bam, chain_infos=sums)
        read_chain.report_sums(sums, chain, world)
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
        return _finish_type_device(a, eng, idx, database, targs, chain, paired=False)
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
        mine = read_chain.infos(eng, read_chain.zeros(chain))
        if mine:      # one line per stage for the sample: the ranks' counters, summed
            box = [None] * world
            dist.all_gather_object(box, mine)
            if rank == 0 and not a.quiet:
                read_chain.report_sums(reduce(read_chain.add_infos, box), chain)
        dist.destroy_process_group()
        return 0
    # FASTQ text goes to the GPU as is and is parsed there (mlst_submit_fastq); a reader thread stays two chunks ahead
    try:
        side1_from = read_chain.stats_side1_from(chain, paths, a.mates, paired)
        submit_sample_files(eng, paths, paired, chunk_bytes, report=None if a.quiet else print, long_reads=long_reads, long_bam_reads=long_bam, side1_from=side1_from)
    except CorruptInput as e:      # nothing of the sample is typed: no .nfo
        print(e, file=sys.stderr)
        database.closeConnection()
        return 1
    if (a.write_sam or a.write_sam_all or a.write_reads) and not paired and not (long_reads or long_bam) and all(_is_reads_bam(f) for f in paths):      # (as submit_bam_reads decides it)
        from .samin import bam_first_read_flags
        paired = any((bam_first_read_flags(f) or 0) & 1 for f in paths)
    return _finish_type_device(a, eng, idx, database, targs, chain, paired=paired)


def _finish_type_device(a, eng, idx, database, targs, chain: dict, paired: bool = False) -> int:
    """Allele choice (metamlst.py:133-151, 244), pile-up and majority consensus on the device, queued behind pass 1
    (mlst_typing_enqueue): one host synchronisation per sample instead of three (statistics, host choice, pile-up).
    --write-sam: then the alignments to the alleles chosen there, as <out>/<sample>.sam (paired: the reads were submitted as pairs);
    --write-sam-all: then every alignment, as <out>/<sample>.all.sam;
    --write-reads: then the reads that have an alignment, as <out>/<sample>.loci.fastq."""
    eng.typing_enqueue(penalty=targs.penalty)
    st, chosen, letters = eng.typing_fetch()
    rc = _finish_type(a, idx, database, targs, st, None, typed=(chosen, letters))
    if rc == 0:
        read_chain.report(eng, chain, paired, a.quiet, a.o + "/" + sample_name(a.READS))
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
