/*
 * mlst_policy.h -- named policy constants of the MLST-typing hot path.
 *
 * Constants only (no code): included by the HIP engine (metamlst_amd/csrc) and by the
 * CPU oracle (oracle/) so that both state the same specification.  Every value marked
 * [NOT IN TREE] restates the documented default of a dependency whose source is not under
 * /root/reference (bowtie2, cmseq, htslib); SURVEY.md section 8(c) lists them as
 * "parity unpinned".  Values marked with a reference file:line are pinned by the tree.
 */
#ifndef MLST_POLICY_H
#define MLST_POLICY_H

/* ---- MetaMLST filter defaults (metamlst.py:38-42, metaMLST_functions.py:258) ---- */
#define MLST_DEF_MINSCORE      80   /* --minscore      metamlst.py:39 */
#define MLST_DEF_MAX_XM         5   /* --max_xM        metamlst.py:40 */
#define MLST_DEF_MIN_READ_LEN  50   /* --min_read_len  metamlst.py:41 */
#define MLST_DEF_PENALTY      100   /* --penalty       metamlst.py:38 (host side only) */
#define MLST_DEF_MINQUAL       20   /* minqual=20      metaMLST_functions.py:258 */
#define MLST_DEF_MINCOV         1   /* mincov=1        metaMLST_functions.py:258 */

/* ---- bowtie2 --very-sensitive-local scoring [NOT IN TREE; wiki command via README.md:20] ---- */
#define MLST_DEF_MATCH_BONUS    2   /* --ma 2 (local mode) */
#define MLST_DEF_MM_MAX         6   /* --mp 6,2 : penalty = MN + floor((MX-MN)*min(Q,40)/40) */
#define MLST_DEF_MM_MIN         2
#define MLST_DEF_N_PENALTY      1   /* --np 1 ; an N column also counts in XM */
#define MLST_DEF_GAP_OPEN       5   /* --rdg 5,3 and --rfg 5,3 : a gap of length g costs 5+3g */
#define MLST_DEF_GAP_EXT        3
#define MLST_DEF_GBAR           4   /* --gbar 4 : no gap within 4 positions of either read end */
#define MLST_DEF_MINSCORE_CONST 20.0 /* --score-min G,20,8 : record exists iff AS >= (long)(20+8 ln L) */
#define MLST_DEF_MINSCORE_COEF   8.0

/* ---- engine seeding / extension policy (this engine's own; replaces bowtie2's heuristics) ---- */
#define MLST_SEED_LEN          20   /* exact seed length (bowtie2 -L 20 in --very-sensitive-local) */
#define MLST_SEED_STEP         16   /* seed every 16 read bases = one packed 32-bit word            */
#define MLST_MAX_POSTINGS      16   /* a seed with more distinct (locus,strand,pos) is repetitive: dropped */
#define MLST_MAX_CAND           8   /* distinct (locus,strand,diag) vote bins kept per read, first-seen order */
#define MLST_MIN_VOTES          1   /* seeds needed on the winning diagonal */
#define MLST_DEF_BAND_W         8   /* banded SW half-width around the voted diagonal */
#define MLST_DEF_GAP_TRIGGER_MM 12  /* banded SW runs iff the seed diagonal looks broken by an indel:
                                       ungapped full-overlap mismatches > this, the ungapped local score
                                       reaches the bowtie2 floor, and ... (next constant);
                                       a negative value means "always run banded SW" */
#define MLST_DEF_GAP_TRIGGER_CLIP 8 /* ... the ungapped local alignment leaves at least this many overlap
                                       columns unaligned (an indel clips the alignment; scattered SNPs do not),
                                       and at least half of those unaligned columns are mismatches (past an indel
                                       the diagonal looks random, ~75 % mismatches; a clipped SNP cluster does not) */
#define MLST_DEF_XM_FIELD_QUIRK 1   /* metamlst.py:110 reads SAM column 15 by position: it is XM only
                                       when XS:i is present (read has >= 2 records), else XO (Q1) */

/* ---- cmseq / pysam pileup policy [NOT IN TREE] ---- */
#define MLST_TIE_ORDER "ACGT"       /* majority-base ties resolve alphabetically (host side) */
#define MLST_DEPTH_CAP          0   /* default of mlst_set_depth_cap: pysam's max_depth=8000 depends on the order of the BAM
                                       file; 0 = not applied.  As a switch it is "the first n records that span a column,
                                       in (read index, strand) order" -- oracle: orc_pileup_capped */

/* ---- BAM input (mlst_submit_bam_bgzf) ---- */
#define MLST_BAM_QNAME_KEY    128   /* sequenceBank[locus][QNAME] (metamlst.py:127) on the device: a read name IS its 128-bit key (two
                                       independent 64-bit hashes of its bytes, and its length).  Two different names of one
                                       sample with the same key would count as one read for the locus' average length; at 10^9
                                       names the chance is ~10^-21.  The host path (samin.AlignmentSample) keeps the names. */
#define MLST_BAM_MAX_RECORD (1048576 - 64)   /* largest BAM record (block_size): the head room of a piece, MLST_E_LIMIT beyond */

/* ---- long reads (mlst_set_read_tiling) ---- */
#define MLST_LONG_READ_WINDOWS  1   /* a FASTQ record or a BAM read longer than the tile is typed as overlapping windows that are unpaired reads of
                                       their own, exactly as a contig's windows are: one long read that covers a locus adds several
                                       records and several sequenceBank lengths to it, where bowtie2 would report one local alignment
                                       per allele.  The reference states nothing for reads its aligner handles and the packed score
                                       fields (MLST_MAX_READ_LEN) cannot hold: the policy is this engine's own, like --contigs */

/* ---- duplicate reads (mlst_set_read_dedup) ---- */
#define MLST_DEDUP_KEY        128   /* on the device a read (a pair) IS its 128-bit key: two independent 64-bit hashes of its length(s) and
                                       its letters folded to A C G T N (both mates of a pair, in order).  The host rule
                                       (fastq.dedup_fastq) compares the letters themselves; the two agree unless two different units of
                                       one sample share all 128 bits (at 10^9 units the chance is ~10^-21), and then the later one is
                                       removed as a duplicate.  Two units that share only the first 64 bits are both kept (a "clash",
                                       counted).  The policy is this engine's own: the reference has no such step */

/* ---- centre-star alignment of a locus' alleles (mlst_msa_align; merge --outseqformat A) ----
 * The policy is this engine's own: the reference pipes the sequences through MUSCLE (metamlst-merge.py:402-405) [NOT IN TREE], whose
 * gap placement differs between its own versions.  The rule is stated in metamlst_amd/msa.py and in include/mlst.h. */
#define MLST_MSA_MATCH          5   /* same letter (case folded), one of A C G T */
#define MLST_MSA_MISMATCH     (-4)  /* everything else: N matches nothing, itself included */
#define MLST_MSA_GAP_OPEN      10   /* a gap of g bases costs GAP_OPEN + g * GAP_EXT, end gaps included */
#define MLST_MSA_GAP_EXT        1

/* ---- hard limits of the packed formats ---- */
#define MLST_MAX_READ_LEN     320   /* 20 packed words; xm field of the packed score is 8 bits */
#define MLST_MAX_ALLELE_LEN  4095   /* 12-bit position in a seed posting */
#define MLST_MAX_LOCI      262143   /* 18-bit locus id in a seed posting */

/* ---- packed DP value: (score << 16) | ((127 - xo) << 8) | (255 - xm) ----
 * One signed 32-bit max() orders by score, then fewer gap opens, then fewer mismatches. */
#define MLST_P_SHIFT   16
#define MLST_P0        0x7FFF              /* empty alignment: score 0, xo 0, xm 0 */
#define MLST_P_NEG     (-(1 << 29))

#endif
