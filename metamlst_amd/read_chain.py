"""The read chain as `cli type` drives it (the engine's half is csrc/read_chain.h): the seven stages that change or
describe the reads of FASTQ text, each stated ONCE -- its flags, how they become settings, where it is refused and in which words,
how it goes onto an Engine and comes back as counters, and the line it prints.  STAGES is the table: its order is that of the flags
in `type --help` and of the setters (apply); REFUSAL_ORDER and REPORT_ORDER are the two other orders a user sees.  Around it: what the
command calls (add_arguments, parse, apply, report) and what a folder and --gpus N sum over samples and ranks (zeros, infos,
add_infos, report_sums; SUMMING: the stages that do).  A chain is {stage key: settings} of the stages that are on.  Pure Python: no engine is imported here."""
from __future__ import annotations

import os
from functools import reduce

_WINDOW = {"long_reads": "--long-reads cuts reads into windows, and a window is cut from the record as it stands",
           "long_bam_reads": "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"}


def _rank(world: int) -> str:      # (a rank of --gpus N speaks for its own samples)
    return (" (the samples of rank %s of %d)" % (os.environ.get("RANK", "0"), world)) if world > 1 else ""


class Stage:
    """One stage.  key: its name in a chain; prefix + refusals[condition]: the sentence it is refused with where the condition holds (a
    condition that is absent: accepted there; the conditions: parse below), refuse_own(a, samples): a sentence for a condition only this
    stage knows, or None; Engine.<setter>(*switch, **settings) turns it on, Engine.<counters>() reads its counters back, zero(settings):
    those counters, all zero.  A stage states add_arguments(p) -- its flags --, parse(a) -- the command's namespace -> its settings, None
    when it is off, ValueError with the sentence to print for a bad value -- and lines(info, settings, paired, world), what it reports."""
    key = prefix = setter = counters = dest = ""
    switch, refusals = (), {}
    refuse_own = staticmethod(lambda a, samples: None)

    def parse(self, a):      # (a stage that is one switch, dest)
        return {} if getattr(a, self.dest, False) else None

    def report(self, info, cfg, quiet: bool, paired: bool = False, world: int = 1, stem=None) -> None:
        if not quiet:
            for line in self.lines(info, cfg, paired, world):
                print(line, flush=True)


class ReadPrep(Stage):
    key, setter, counters = "prep", "set_read_prep", "read_prep_info"
    prefix = "read preparation (--trim5, --trim3, --trim-qual, --phred64): "
    refusals = {"alignments": "with --alignments the records are what they are: the file holds alignments, not reads to prepare",
                "contigs": "--contigs cuts assemblies into windows, and a window is cut from the sequence as it stands", **_WINDOW,
                "reads_bam": "a reads BAM stores raw Phred and its own strand, and its reads are not prepared: FASTQ input only"}
    zero = staticmethod(lambda cfg: {"shortened": 0, "bases_removed": 0, "emptied": 0})

    def add_arguments(self, p):
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

    def parse(self, a):
        t5, t3, tq, p64 = getattr(a, "trim5", 0), getattr(a, "trim3", 0), getattr(a, "trim_qual", 0), bool(getattr(a, "phred64", False))
        if not (t5 or t3 or tq or p64):
            return None
        for flag, v, top in (("--trim5", t5, 65535), ("--trim3", t3, 65535), ("--trim-qual", tq, 93)):
            if not 0 <= v <= top:
                raise ValueError("%s takes a number from 0 to %d, not %d" % (flag, top, v))
        return {"trim5": t5, "trim3": t3, "trim_qual": tq, "phred64": p64}

    def lines(self, info, cfg, paired=False, world=1):
        return ["read preparation: %d reads shortened, %d bases removed, %d reads left without a base" % (info["shortened"], info["bases_removed"], info["emptied"]) + _rank(world)]


class ReadWindow(Stage):
    key, setter, counters = "window", "set_read_window", "read_window_info"
    prefix = "quality windows (--cut-front, --cut-right, --cut-tail): "
    refusals = {"alignments": "with --alignments the records are what they are: the file holds alignments, not reads to cut",
                "contigs": "--contigs cuts assemblies into windows, and an assembly has no qualities", **_WINDOW,
                "reads_bam": "a reads BAM stores raw Phred and its own strand, and its reads are not cut: FASTQ input only",
                "many": "several samples or a folder are typed without them (the rule is per read: summing the counters of the samples is the follow-up)",
                "gpus": "one GPU: the counters of the ranks of --gpus N are not summed yet (the follow-up)"}
    OPS = (("front", "--cut-front", "cut_front"), ("right", "--cut-right", "cut_right"), ("tail", "--cut-tail", "cut_tail"))

    def add_arguments(self, p):
        p.add_argument("--cut-front", dest="cut_front", default=None, metavar="W,Q",
                       help="FASTQ input: drop bases from the 5' end of every read up to the first window of W bases whose mean quality "
                            "reaches Q, on the GPU (csrc/read_window.h; the rule: metamlst_amd.fastq.window_cut / cut_windows, modelled on fastp "
                            "--cut_front; it is the project's own and claims neither fastp's nor Trimmomatic's bytes).  W is 1 to 320, Q 1 to "
                            "93; W = 1 is Trimmomatic's LEADING:Q.  A read without a passing window is left without a base.  The three "
                            "quality windows (--cut-front, --cut-right, --cut-tail) run in that order behind --trim5 / --trim3 / --trim-qual "
                            "and in front of --adapter, each mate on its own; with --min-length they are Trimmomatic's quality recipe "
                            "(LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15 MINLEN:36 = --cut-front 1,3 --cut-tail 1,3 --cut-right 4,15 --min-length "
                            "36).  One sample on one GPU: plain, .gz and bgzip'd FASTQ, `a.fq,b.fq`, -2; refused with --alignments, --contigs, "
                            "--long-reads, --long-bam-reads, a reads BAM, a folder or several samples, and --gpus N; --cut-front is refused "
                            "with --pair-overlap, which places the insert's end by --trim5 alone.  A read left without a base stays a read, "
                            "and the exports carry the cut SEQ / QUAL.  Unless --quiet, one line reports what the three did")
        p.add_argument("--cut-right", dest="cut_right", default=None, metavar="W,Q",
                       help="FASTQ input: cut every read at the first window of W bases, from the 5' end on, whose mean quality is below Q; "
                            "the bases at the front of that window that reach Q stay (fastp --cut_right, the model of Trimmomatic's "
                            "SLIDINGWINDOW:W:Q).  It catches a dip in the middle of a read, which --trim-qual's running sum tolerates; see --cut-front")
        p.add_argument("--cut-tail", dest="cut_tail", default=None, metavar="W,Q",
                       help="FASTQ input: drop bases from the 3' end of every read down to the last window of W bases whose mean quality "
                            "reaches Q (fastp --cut_tail; W = 1 is Trimmomatic's TRAILING:Q); see --cut-front")

    def parse(self, a):
        out = {}
        for name, flag, dest in self.OPS:
            text = getattr(a, dest, None)
            if text is None:
                out[name] = None
                continue
            try:
                w, q = (int(x) for x in text.split(","))
            except ValueError:
                raise ValueError("%s W,Q takes two numbers, not %r" % (flag, text)) from None
            if not 1 <= w <= 320:
                raise ValueError("%s W,Q: a window holds 1 to 320 bases, not %d" % (flag, w))
            if not 1 <= q <= 93:
                raise ValueError("%s W,Q: a quality is 1 to 93, not %d" % (flag, q))
            out[name] = (w, q)
        return out if any(v is not None for v in out.values()) else None

    def refuse_own(self, a, samples):
        if getattr(a, "cut_front", None) is not None and getattr(a, "pair_overlap", False):
            return ("--cut-front goes with no --pair-overlap, which places the insert's end by --trim5 alone (both mates lost the same number of "
                    "5' bases): a front cut per read would make it cut true insert bases (--cut-right and --cut-tail combine with it)")
        return None

    def lines(self, info, cfg, paired=False, world=1):
        return [read_window_line(info)]


class Adapters(Stage):
    key, setter, counters, prefix = "adapters", "set_read_adapters", "read_adapters_info", "--adapter: "
    refusals = {"alignments": "with --alignments the records are what they are: the file holds alignments, not reads to cut",
                "contigs": "--contigs cuts assemblies into windows, and an assembly carries no adapter", **_WINDOW,
                "reads_bam": "the reads of a BAM are taken as they are stored: FASTQ input only"}
    zero = staticmethod(lambda cfg: {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0] * len(cfg["adapters"])})

    def add_arguments(self, p):
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

    def parse(self, a):
        from .fastq import ADAPTER_NAMES, check_adapters
        spec, mo, er = getattr(a, "adapter", ""), getattr(a, "adapter_min_overlap", None), getattr(a, "adapter_error_rate", None)
        if not spec:
            for flag, v in (("--adapter-min-overlap", mo), ("--adapter-error-rate", er)):
                if v is not None:
                    raise ValueError(flag + " belongs to --adapter: give the adapter it applies to")
            return None
        try:
            if er is not None and not 0 <= er <= 0.5:
                raise ValueError("--adapter-error-rate takes a number from 0 to 0.5, not %r" % er)
            permille = 100 if er is None else int(round(1000 * er))
            ads = check_adapters([ADAPTER_NAMES.get(x.strip().lower(), x.strip()) for x in spec.split(",")], 3 if mo is None else mo, permille)
        except ValueError as e:
            raise ValueError("--adapter: %s" % e) from None
        return {"adapters": [x.decode() for x in ads], "min_overlap": 3 if mo is None else mo, "error_permille": permille}

    def lines(self, info, cfg, paired=False, world=1):
        per = ", ".join("%s %d" % (s, n) for s, n in zip(cfg["adapters"], info["per_adapter"]))
        return ["adapter removal: %d reads cut, %d bases removed, %d reads left without a base (%s)" % (info["trimmed"], info["bases_removed"], info["emptied"], per) + _rank(world)]


class ReadStats(Stage):
    key, dest, setter, switch, counters, prefix = "stats", "read_stats", "set_read_stats", (True,), "read_stats", "--read-stats: "
    refusals = {"alignments": "with --alignments the file holds alignments, not the reads of a FASTQ file",
                "contigs": "--contigs cuts assemblies into windows, and an assembly has neither cycles nor qualities",
                "long_reads": "--long-reads cuts reads into windows, and the tables hold the 320 cycles of a short read",
                "long_bam_reads": "--long-bam-reads cuts reads into windows, and the tables hold the 320 cycles of a short read",
                "reads_bam": "the reads of a BAM are not counted: FASTQ input only",
                "many": "it reports one sample: several samples or a folder are typed without it",
                "gpus": "the tables are one GPU's: a rank of --gpus N counts its own share of the reads only"}

    def add_arguments(self, p):
        p.add_argument("--read-stats", dest="read_stats", action="store_true",
                       help="FASTQ input: count per-cycle quality and base tables of the sample's reads on the GPU, next to the parser "
                            "(csrc/read_stats.h; the rule: metamlst_amd.fastq.read_stats), as they stand in the file (raw) and, where --trim* / "
                            "--adapter ran, as they are aligned (prepared); R1 and R2 apart.  After the .nfo, write <out>/<sample>.readstats.tsv "
                            "(the format: metamlst_amd.fastq.read_stats_text; the project's own) and, unless --quiet, print one line per stage "
                            "and side, and a hint when the qualities look like the other Phred base.  One sample on one GPU: plain, .gz and "
                            "bgzip'd FASTQ, `a.fq,b.fq`, -2; refused with --alignments, --contigs, --long-reads, --long-bam-reads, a reads BAM, "
                            "a folder or several samples, and --gpus N.  The .nfo, the --log file and every export do not change")

    def report(self, stats, cfg, quiet, paired=False, world=1, stem=None):      # (the file and the Phred hint under quiet too)
        from .fastq import phred_hint, read_stats_text
        with open(stem + ".readstats.tsv", "wb") as f:
            f.write(read_stats_text(stats, stem.split("/")[-1]))
        for line in ([] if quiet else read_stats_lines(stats)) + [phred_hint(stats)]:
            if line:
                print(line, flush=True)


class Dedup(Stage):
    key, dest, setter, switch, counters, prefix = "dedup", "dedup", "set_read_dedup", (True,), "read_dedup_info", "duplicate removal (--dedup): "
    refusals = {"alignments": "with --alignments the file holds alignments, not reads to compare (duplicate alignments are samtools markdup's)",
                "contigs": "--contigs cuts assemblies into windows, and the windows of an assembly are not copies of a molecule",
                "long_reads": "--long-reads cuts reads into windows, and the windows of a read would be compared, not the read",
                "long_bam_reads": "--long-bam-reads cuts reads into windows, and the windows of a read would be compared, not the read",
                "reads_bam": "the reads of a BAM are not compared: FASTQ input only",
                "many": "one table of keys per engine: several samples or a folder are typed without it (per-sample tables through the pipelined loop are the follow-up)",
                "gpus": "a rank of --gpus N sees only its byte range, and duplicates across ranks would be missed"}
    lines = staticmethod(lambda info, cfg, paired, world: [read_dedup_line(info, paired)])

    def add_arguments(self, p):
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


class PairOverlap(Stage):
    key, setter, switch, counters, prefix = "overlap", "set_read_pair_overlap", (True,), "read_pair_overlap_info", "--pair-overlap: "
    refusals = {"alignments": "with --alignments the file holds alignments, not mates to lay on each other",
                "contigs": "--contigs cuts assemblies into windows, and a window has no mate",
                "long_reads": "--long-reads cuts unpaired reads into windows, and a window has no mate",
                "long_bam_reads": "--long-bam-reads cuts unpaired reads into windows, and a window has no mate",
                "reads_bam": "the mates of a BAM are taken as they are stored: FASTQ input with -2 only",
                "many": "several samples or a folder are typed without it (the rule is per pair: summing the counters of the samples is the follow-up)",
                "gpus": "one GPU: the counters of the ranks of --gpus N are not summed yet (the follow-up)"}
    lines = staticmethod(lambda info, cfg, paired, world: [read_pair_overlap_line(info)])

    def add_arguments(self, p):
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

    def parse(self, a):
        from .fastq import check_pair_overlap
        mo, mm, er = getattr(a, "pair_overlap_min", None), getattr(a, "pair_overlap_diff", None), getattr(a, "pair_overlap_rate", None)
        if not getattr(a, "pair_overlap", False):
            for flag, v in (("--pair-overlap-min", mo), ("--pair-overlap-diff", mm), ("--pair-overlap-rate", er)):
                if v is not None:
                    raise ValueError(flag + " belongs to --pair-overlap: give the switch it applies to")
            return None
        try:
            if er is not None and not 0 <= er <= 0.5:
                raise ValueError("--pair-overlap-rate takes a number from 0 to 0.5, not %r" % er)
            out = {"min_overlap": 30 if mo is None else mo, "max_mismatches": 5 if mm is None else mm, "error_permille": 200 if er is None else int(round(1000 * er))}
            check_pair_overlap(**out)
        except ValueError as e:
            raise ValueError("--pair-overlap: %s" % e) from None
        return out

    def refuse_own(self, a, samples):
        from .fastq import mates_share_names
        if not a.mates:
            return "it lays the mates of a pair on each other: give the second file with -2"
        if len(samples[0]) > 1:
            return "it takes one file of first mates and one of second mates (-2), not `a.fq,b.fq`"
        try:
            return None if mates_share_names(samples[0][0], a.mates) else ("the records of %s and %s do not share their names, so the files go in as two unpaired "
                                                                         "texts and no read has a mate" % (samples[0][0], a.mates))
        except OSError as e:
            return str(e)


class ReadFilter(Stage):
    key, setter, counters = "filter", "set_read_filter", "read_filter_info"
    prefix = "read filter (--trim-poly-g, --trim-poly-x, --min-length, --max-n, --low-complexity, --min-mean-qual): "
    refusals = {"alignments": "with --alignments the records are what they are: the file holds alignments, not reads to trim or remove",
                "contigs": "--contigs cuts assemblies into windows, and an assembly has neither tails nor qualities", **_WINDOW,
                "reads_bam": "the reads of a BAM are taken as they are stored: FASTQ input only"}
    zero = staticmethod(lambda cfg: {"tail_trimmed": 0, "tail_bases": 0, "per_letter": [0, 0, 0, 0], "tail_emptied": 0, "failed_short": 0, "failed_n": 0,
                                     "failed_complexity": 0, "failed_quality": 0, "filtered_bases": 0})
    lines = staticmethod(lambda info, cfg, paired, world: [read_filter_line(info, world)])

    def add_arguments(self, p):
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

    def parse(self, a):
        from .fastq import check_read_filter
        g, x, pm = bool(getattr(a, "trim_poly_g", False)), bool(getattr(a, "trim_poly_x", False)), getattr(a, "poly_min", None)
        ml, mn, lc, mq = (getattr(a, k, None) for k in ("min_length", "max_n", "low_complexity", "min_mean_qual"))
        if g and x:
            raise ValueError("--trim-poly-x trims G tails too: give one of the two")
        if pm is not None and not (g or x):
            raise ValueError("--poly-min belongs to --trim-poly-g / --trim-poly-x: give the switch it applies to")
        if not (g or x) and ml is None and mn is None and lc is None and mq is None:
            return None
        for flag, v, lo, hi in (("--poly-min", pm, 1, 320), ("--min-length", ml, 1, 320), ("--max-n", mn, 0, 0xFFFFFFFE), ("--low-complexity", lc, 1, 100), ("--min-mean-qual", mq, 1, 93)):
            if v is not None and not lo <= v <= hi:
                raise ValueError("%s takes a number from %d to %d, not %d" % (flag, lo, hi, v))
        out = {"poly": "G" if g else "ACGT" if x else "", "poly_min": 10 if pm is None else pm, "min_length": ml or 0, "max_n": mn, "complexity": lc or 0, "mean_qual": mq or 0}
        check_read_filter(out["poly"], out["poly_min"], out["min_length"], out["max_n"], out["complexity"], out["mean_qual"])
        return out


PREP, WINDOW, ADAPTERS, STATS, DEDUP, OVERLAP, FILTER = STAGES = (ReadPrep(), ReadWindow(), Adapters(), ReadStats(), Dedup(), PairOverlap(), ReadFilter())      # the table
REFUSAL_ORDER = (PREP, WINDOW, ADAPTERS, FILTER, STATS, DEDUP, OVERLAP)      # which stage speaks first when several refuse
REPORT_ORDER = (PREP, WINDOW, ADAPTERS, FILTER, OVERLAP, STATS, DEDUP)      # the lines behind a sample
SUMMING = [s for s in STAGES if "many" not in s.refusals and "gpus" not in s.refusals]      # their counters add up over the samples of a folder and the ranks of --gpus N
_read_filter_of = FILTER.parse


def add_arguments(p) -> None:
    for s in STAGES:
        s.add_arguments(p)


def parse(a, samples, reads_bam: bool = False, world: int = 1):
    """The chain of the command a over samples (cli.expand_samples): {stage key: settings} of the stages that are on; None after the first bad value
    or refusal has been said.  reads_bam: a file is a BAM of reads; world: WORLD_SIZE.  The conditions are tried in this order, a stage's own last."""
    holds = {"alignments": a.alignments, "contigs": a.contigs, "long_reads": a.long_reads, "long_bam_reads": a.long_bam_reads, "reads_bam": reads_bam,
             "many": len(samples) > 1, "gpus": a.gpus > 1 or world > 1}
    chain = {}
    try:
        for s in REFUSAL_ORDER:
            cfg = s.parse(a)
            if cfg is not None:
                why = next((s.refusals[c] for c, on in holds.items() if on and c in s.refusals), None) or s.refuse_own(a, samples)
                if why:
                    raise ValueError(s.prefix + why)
                chain[s.key] = cfg
    except ValueError as e:
        print(e)
        return None
    return chain


def apply(eng, chain: dict) -> None:      # (the reads are prepared, cut, counted and compared where the FASTQ text is parsed)
    for s in STAGES:
        if s.key in chain:
            getattr(eng, s.setter)(*s.switch, **chain[s.key])


def report(eng, chain: dict, paired: bool, quiet: bool, stem: str) -> None:      # behind a sample; stem: <out>/<sample>, where the statistics file goes
    for s in REPORT_ORDER:
        if s.key in chain:
            s.report(getattr(eng, s.counters)(), chain[s.key], quiet, paired=paired, stem=stem)


def zeros(chain: dict) -> dict:      # {stage key: all-zero counters} of the summing stages that are on
    return {s.key: s.zero(chain[s.key]) for s in SUMMING if s.key in chain}


def infos(eng, keys) -> dict:      # {stage key: the engine's counters} of the stages in keys
    return {s.key: getattr(eng, s.counters)() for s in STAGES if s.key in keys}


def add_infos(a, b):      # counters added up: integers add, lists element by element, dicts ({stage key: counters} too) key by key
    if isinstance(b, dict):
        return {k: add_infos(a[k], v) for k, v in b.items()}
    return [x + y for x, y in zip(a, b)] if isinstance(b, list) else a + b


def report_sums(sums: dict, chain: dict, world: int = 1) -> None:      # sums: {stage key: counters}; world > 1: a rank speaks for its own samples
    for s in REPORT_ORDER:
        if s.key in sums:
            s.report(sums[s.key], chain[s.key], False, world=world)


def stats_side1_from(chain: dict, paths, mates, paired: bool):      # mates whose names differ go in as unpaired text, the mate file counted into side 1 -> its index
    return len(paths) - 1 if (STATS.key in chain and mates and not paired) else None


def _sum_filter_infos(infos_) -> dict:      # Engine.read_filter_info() of several engines or ranks, added up (none: all zero)
    return reduce(add_infos, infos_, FILTER.zero(None))


def read_filter_line(info: dict, world: int = 1) -> str:
    """The line on what the tail trim and the read filters did (info: Engine.read_filter_info() or fastq.filter_fastq's counters, summed
    over the samples of a folder; a rank of --gpus N then speaks for its own samples)"""
    failed = [int(info[k]) for k in ("failed_short", "failed_n", "failed_complexity", "failed_quality")]
    return ("read filter: %d poly tails trimmed (A %d, C %d, G %d, T %d), %d bases removed, %d reads left without a base; %d reads removed "
            "(%d too short, %d with too many N, %d of low complexity, %d of low quality), %d bases"
            % (int(info["tail_trimmed"]), *[int(v) for v in info["per_letter"]], int(info["tail_bases"]), int(info["tail_emptied"]), sum(failed), *failed,
               int(info["filtered_bases"]))) + _rank(world)


def read_window_line(info: dict) -> str:
    """The line on what --cut-front / --cut-right / --cut-tail did (info: Engine.read_window_info() or fastq.cut_windows' counters)"""
    return ("quality windows: %d reads cut (front %d reads / %d bases, right %d reads / %d bases, tail %d reads / %d bases), %d reads left without a base"
            % tuple(int(info[k]) for k in ("shortened", "front_reads", "front_bases", "right_reads", "right_bases", "tail_reads", "tail_bases", "emptied")))


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
