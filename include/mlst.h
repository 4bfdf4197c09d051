/*
 * mlst.h -- C-ABI of the MI355X MLST-typing engine (libmlst_hip.so).
 *
 * The reference (SegataLab/metamlst) has no FFI for this path: the seams it offers are a
 * process pipe and Python functions.  Each entry point below names the
 * reference site it replaces.  Plain pointers and sizes only; the caller owns every
 * buffer; the library never returns owned memory.  Every function returns 0 on success
 * or a negative MLST_E_* code, with text available from mlst_last_error().  A handle is
 * bound to one GPU and is not thread-safe; distinct handles are independent.
 *
 * Binding from the reference's language (Python) is ctypes: see INTEGRATION.md.
 */
#ifndef MLST_H
#define MLST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLST_OK              0
#define MLST_E_INVALID      -1   /* bad argument / bad state */
#define MLST_E_NOGPU        -2   /* no usable HIP device: the product path has no CPU fallback */
#define MLST_E_HIP          -3   /* a HIP runtime call failed */
#define MLST_E_CAPACITY     -4   /* retained-read / item / worklist capacity exceeded */
#define MLST_E_LIMIT        -5   /* input exceeds a packed-format limit (mlst_policy.h) */

typedef struct mlst_handle mlst_handle;

/* Engine parameters.  Defaults (mlst_default_params) are the reference's:
 * minscore/max_xm/min_read_len = argparse defaults metamlst.py:39-41; minqual/mincov =
 * cmseq call metaMLST_functions.py:258; scoring = bowtie2 --very-sensitive-local [NOT IN TREE]. */
typedef struct mlst_params {
    int32_t minscore;          /* accept record iff AS >= minscore            metamlst.py:115 */
    int32_t max_xm;            /* ... and field15 <= max_xm                   metamlst.py:115 */
    int32_t min_read_len;      /* ... and len(SEQ) >= min_read_len            metamlst.py:115 */
    int32_t minqual;           /* pileup base quality floor                   metaMLST_functions.py:258 */
    int32_t mincov;            /* informational (applied host side)           metaMLST_functions.py:258 */
    int32_t match_bonus;       /* bowtie2 --ma */
    int32_t mm_max, mm_min;    /* bowtie2 --mp MX,MN */
    int32_t n_penalty;         /* bowtie2 --np */
    int32_t gap_open, gap_ext; /* bowtie2 --rdg/--rfg (symmetric) */
    int32_t gbar;              /* bowtie2 --gbar */
    int32_t band_w;            /* banded Smith-Waterman half width */
    int32_t gap_trigger_mm;    /* see mlst_policy.h; <0 = always banded SW */
    int32_t xm_field_quirk;    /* 1 = emulate metamlst.py:110 positional parse (Q1) */
    int32_t gap_trigger_clip;  /* see mlst_policy.h */
    double  minscore_const;    /* bowtie2 --score-min G,const,coef */
    double  minscore_coef;
    uint64_t max_retained_reads; /* capacity of the on-locus read store (0 = default) */
    uint64_t max_items;          /* capacity of the (read,locus,strand,diag) item list (0 = default) */
    uint64_t max_pair_results;   /* capacity of the per-(item,allele) result arena (0 = default) */
} mlst_params;

/* counters[] layout of mlst_get_allele_stats */
enum {
    MLST_CNT_TOTAL_RECORDS = 0,  /* totalReads   metamlst.py:130 (alignment records, Q13) */
    MLST_CNT_IGNORED       = 1,  /* ignoredReads metamlst.py:129 */
    MLST_CNT_READS_SEEN    = 2,  /* reads submitted */
    MLST_CNT_CANDIDATES    = 3,  /* reads that passed the seed sieve */
    MLST_CNT_RETAINED      = 4,  /* reads with at least one exact seed (kept for pass 2) */
    MLST_CNT_ITEMS         = 5,  /* (read,locus,strand,diag) work items */
    MLST_CNT_DP_PAIRS      = 6,  /* (item,allele) pairs sent to banded SW */
    MLST_CNT_SIEVE_PASS    = 7,  /* routed sieve: entries that passed the LDS filter and were examined exactly (a tuning figure) */
    MLST_CNT_N             = 8
};

void mlst_default_params(mlst_params* p);

/* Create / destroy an engine bound to HIP device `device`.  Fails with MLST_E_NOGPU when
 * no device is present (there is no CPU path in this library), and with MLST_E_LIMIT for scoring
 * parameters under which a read of MLST_MAX_READ_LEN bases could exceed a packed field (10-bit score,
 * 8-bit xm, 7-bit xo): match_bonus * 320 >= 1024, match_bonus > 4 * min(n_penalty, mm_min), or
 * 5 * match_bonus > 2 * (gap_open + gap_ext). */
int  mlst_create(int device, const mlst_params* p, mlst_handle** out);
void mlst_destroy(mlst_handle* h);
const char* mlst_last_error(const mlst_handle* h);   /* h may be NULL: last create error */

/* Load the allele reference.  Replaces dump_db_to_fasta + bowtie2-build
 * (metaMLST_functions.py:149-161, metamlst-index.py:222-247).
 *   ascii_concat : all allele sequences concatenated (bytes as stored in alleles.sequence)
 *   off[n+1]     : byte offsets into ascii_concat
 *   locus_id[n]  : dense locus index 0..L-1; alleles of one locus must be contiguous
 *   species_id[n], allele_no[n] : carried for the caller (alleles.bacterium / alleleVariant)
 */
int mlst_load_reference(mlst_handle* h, const uint8_t* ascii_concat, const uint64_t* off,
                        const uint32_t* locus_id, const uint32_t* species_id,
                        const int32_t* allele_no, uint32_t n_alleles);

/* The built host index on disk.  The reference keeps `<idx>.1.bt2` next to its FASTA dump and skips bowtie2-build when the
 * file is there (metamlst-index.py:224-225); here mlst_load_reference reads the index it would build (2-bit arena,
 * block-haplotype tables, seed table, sieves) from `path` when the file's header carries the key of the inputs (hashes of
 * the allele text, offsets, locus and species ids, the sieve switches), and writes the file after a build otherwise.
 * Process-wide; NULL or "" switches it off (the default).  A file that does not fit the inputs is ignored and replaced. */
int mlst_set_reference_cache(const char* path);

/* The host-side index built by the last mlst_load_reference of the process is kept (a second engine on the same
 * database only uploads it: 0.5 s instead of 13 s for the full database); this releases it (~0.6 GB for the full
 * database).  MLST_INDEX_CACHE=0 in the environment disables the cache. */
void mlst_release_index_cache(void);

/* Pass 1 over one batch of reads held in HOST memory (FASTQ fields as read from the file):
 * seed sieve -> exact seeds -> extension against every allele of the hit locus ->
 * per-allele {sum AS, hits}.  Replaces bowtie2 -a ... | samtools view + the hit
 * accumulator loop metamlst.py:96-130.  On-locus reads are retained on the GPU for pass 2.
 *   bases  : ASCII bases concatenated;  quals : ASCII Phred+33 concatenated (same offsets)
 *   off[n+1]; paired != 0 means reads 2k and 2k+1 are mates (share a QNAME, Q3). */
int mlst_submit_reads(mlst_handle* h, const uint8_t* bases, const uint8_t* quals,
                      const uint64_t* off, uint64_t n_reads, int paired);

/* Page-locked host memory for the caller's input buffers (FASTQ text read from files, packed arrays): host-to-device copies
 * from it are DMA transfers at the link's rate, without the runtime's staging copy.  Process-wide; no engine needed. */
int mlst_alloc_host(uint64_t n_bytes, void** out);
int mlst_free_host(void* p);

/* Pass 1 straight from FASTQ TEXT (uncompressed, 4 lines per record, LF or CRLF) held in host memory: the bytes
 * cross PCIe once and are parsed on the GPU (line starts by block newline counts + scan, then packed).  The chunk
 * must hold whole records (cut it after a multiple of four lines).  Replaces the FASTQ reader in front of
 * bowtie2 [NOT IN TREE].  n_reads_out (optional) receives the number of records found. */
int mlst_submit_fastq(mlst_handle* h, const uint8_t* text, uint64_t n_bytes, int paired, uint64_t* n_reads_out);

/* One chunk of an OPEN FASTQ stream: the text continues what the calls before left over (a partial record at the end of
 * a chunk is kept on the device and completed by the next call, whichever of mlst_submit_fastq_stream /
 * mlst_submit_fastq_bgzf it is: text and BGZF chunks of one stream may alternate); a chunk may be cut anywhere.  The last
 * chunk is passed with final_chunk != 0 and must end with a whole record (n_bytes may be 0 then).  Used for the head and
 * tail of a BGZF byte range, which the host inflates itself to find the record boundary (metamlst_amd/fastq.py). */
int mlst_submit_fastq_stream(mlst_handle* h, const uint8_t* text, uint64_t n_bytes, int final_chunk, int paired, uint64_t* n_reads_out);

/* Two chunks of FASTQ text from the two files of a paired-end sample, holding the SAME number of whole records each:
 * record k of text1 and record k of text2 are mates.  They are interleaved on the GPU (reads 2k, 2k+1) and submitted as
 * pairs, i.e. one QNAME per pair for sequenceBank (metamlst.py:127, Q3) -- bowtie2 itself sees them as unpaired reads
 * (-U r1,r2, README.md:20).  n_reads_out receives the number of reads (2 x records per file). */
int mlst_submit_fastq_pair(mlst_handle* h, const uint8_t* text1, uint64_t n1, const uint8_t* text2, uint64_t n2, uint64_t* n_reads_out);

/* The same from BGZF-compressed FASTQ (bgzip; a series of independent <= 64 KiB deflate blocks): the COMPRESSED bytes
 * cross PCIe, the blocks are inflated on the GPU (csrc/inflate_lane.h: one lane per block decodes the codes into tokens,
 * one workgroup per block turns tokens into bytes; csrc/inflate_wave.h for oversized blocks), the text is parsed as above.  A chunk is
 * a run of whole BGZF blocks cut anywhere between blocks; a record that straddles two chunks is completed by the next
 * call; the last chunk of a file is passed with final_chunk != 0 and must end with a whole record.  The inflated size of
 * every block is checked always; its CRC-32 is checked when mlst_set_bgzf_verify is on (below; off by default).  With n_consumed_out != NULL a non-final buffer may also end inside a block:
 * the call takes the whole blocks, reports their size, and the caller passes the rest again in front of the next
 * buffer (so a reader never has to walk the block headers itself).  Plain gzip has no block structure to parallelise:
 * inflate it on the host and use mlst_submit_fastq.
 * Three stages on three streams (round 5): a call queues the copy of ITS chunk and the inflate of it, then parses and submits
 * the chunk of the call BEFORE it while the GPU inflates -- so the reads of a non-final chunk enter the statistics with the
 * next call on this handle (whichever entry that is: every entry that looks at or adds to the sample's state finishes an open
 * chunk first), n_reads_out counts the records COMPLETED by the call (their sum over a file is the file's record count), and a
 * corrupt block is reported by the call that finishes its chunk.  `data` may be released when the call returns.
 * MLST_BGZF_PIPE=0 restores the serial behaviour (copy, inflate, parse and submit inside the call). */
int mlst_submit_fastq_bgzf(mlst_handle* h, const uint8_t* data, uint64_t n_bytes, int final_chunk, int paired, uint64_t* n_reads_out,
                           uint64_t* n_consumed_out);

/* The two bgzip'd files of a paired-end sample, inflated on the GPU and paired there (mlst_submit_fastq_pair for BGZF).  data1 /
 * data2 are runs of BGZF blocks of file 1 / file 2, cut as for mlst_submit_fastq_bgzf (with n_consumed1_out / n_consumed2_out
 * != NULL a non-final buffer may end inside a block: the call takes the whole blocks and reports how many bytes that was).  A
 * call may carry any number of records of either file, none of one of them included: record k of file 1 and record k of file 2
 * are mates, counted across calls, and become reads 2k, 2k + 1, submitted as pairs (one QNAME per pair for sequenceBank,
 * metamlst.py:127, Q3).  The records of the file that is ahead wait on the device for their mates, as does the partial record
 * at the end of each file's text; a carry that cannot be placed fails with MLST_E_LIMIT.  n_reads_out counts the reads
 * completed by the call (2 x pairs; over a sample: 2 x records per file).  The last call passes final_chunk != 0: both files
 * must end with a whole record and hold the same number of records ("mate files hold different numbers of records"); a corrupt
 * block is reported with the file (1 or 2) it belongs to.  Pipelined as mlst_submit_fastq_bgzf (the blocks of both files of
 * call k are inflated in one launch sequence while the pieces of call k - 1 are paired, parsed and submitted; every entry that
 * looks at or adds to the sample's state finishes an open piece first; MLST_BGZF_PIPE=0: serial).  While a paired stream is open
 * (its final call not made yet) the other mlst_submit_fastq* entries refuse to start, and this one refuses while a single
 * stream is open; mlst_reset_sample and any error drop both carries. */
int mlst_submit_fastq_bgzf_pair(mlst_handle* h, const uint8_t* data1, uint64_t n1, const uint8_t* data2, uint64_t n2, int final_chunk,
                                uint64_t* n_reads_out, uint64_t* n_consumed1_out, uint64_t* n_consumed2_out);

/* The CRC-32 in the trailer of every BGZF block (RFC 1952) against the text the block inflated to, computed on the GPU behind the
 * decoders (csrc/bgzf_crc.h) for mlst_submit_fastq_bgzf and mlst_submit_fastq_bgzf_pair: on != 0 switches the check on.  Off by
 * default (MLST_BGZF_CRC=1 in the environment: on for a new handle): nothing is queued for it then, and a block that inflates to
 * the right length with wrong bytes is typed as it is.  A mismatch fails the call that finishes the block's piece, before any of
 * the piece's reads are submitted, with MLST_E_INVALID and "CRC mismatch in BGZF block <n> of the chunk (stored 0x..., computed
 * 0x...)" (" of file <1|2> in the chunk" on the paired entry; n counts the chunk's blocks with data); the stream ends there as
 * after corrupt deflate data.  Blocks without data (the EOF marker) hold nothing to check.  The switch may change only while
 * no FASTQ stream of any kind (text, BGZF, paired) is open on the handle: MLST_E_INVALID "a FASTQ stream is open" otherwise. */
int mlst_set_bgzf_verify(mlst_handle* h, int on);
int mlst_get_bgzf_verify(mlst_handle* h, int* on);

/* ---- LONG READS: FASTQ records and BAM reads longer than a tile cut into windows on the GPU (csrc/fastq_tile.h, csrc/bam_tile.h) ----
 * A read longer than MLST_MAX_READ_LEN (320) bases cannot be packed (the packed score's fields), and without this
 * switch every FASTQ entry fails it with MLST_E_LIMIT "a FASTQ read is longer than 320 bases".  mlst_set_read_tiling(h, read_len,
 * stride) switches tiling on for the handle (0, 0: off, the default -- nothing changes then and nothing more is launched, copied or
 * waited for).  With it on, the UNPAIRED text entries -- mlst_submit_fastq, mlst_submit_fastq_stream and mlst_submit_fastq_bgzf with
 * paired == 0 -- apply the rule of metamlst_amd.fastq.tile_fastq on the device, behind the parser:
 *   - records keep their order.  A record of n <= read_len bases (n = 0 included) is one read, unchanged.
 *   - a record of n > read_len bases becomes windows of read_len bases at starts 0, stride, 2 * stride, ... <= n - read_len, plus one
 *     flush with the record's end when (n - read_len) % stride != 0 (mlst_submit_fasta's rule with min_len 0).
 *   - a window carries the same slice of the sequence line and of the quality line; bases are what the parser makes of them (N, lower
 *     case, CR as without the switch), and a window's non-ACGT bit (bit 15 of lens) is its own.
 *   - windows are unpaired reads of their own (MLST_LONG_READ_WINDOWS, mlst_policy.h): read indices continue the handle's count in
 *     record order, then start order, and n_reads_out counts reads, i.e. windows plus uncut records.
 * An UNPAIRED reads stream of a BAM (mlst_bam_reads_open with paired == 0) opened while the switch is on applies the same rule to the
 * reads `samtools fastq` would write (metamlst_amd.samin.bam_reads_fastq, then tile_fastq) -- windows are cut from the READ, not from the
 * stored SEQ (csrc/bam_tile.h):
 *   - kept records keep their order; secondary, supplementary and empty records are skipped and counted as without the switch.
 *   - a kept read of n <= read_len bases is one read, unchanged; one of n > read_len bases becomes the windows above.
 *   - FLAG 0x10: the read is the reverse complement of SEQ with QUAL reversed, so window st of the read is bases n - 1 - st ... n - st - len
 *     of SEQ, complemented; the window flush with the read's end lies at the front of the stored SEQ.
 *   - a window's Phred values are the same slice of the read's, clamped to 127; a first quality byte of 0xFF gives Phred 1 to every base
 *     of every window; non-ACGT nibbles pack as A with bit 7 in qrows, a window's bit 15 of lens is its own; the filler nibble of an
 *     odd l_seq is never a base.
 *   - read indices continue the handle's count in record order, then start order.  MLST_CNT_READS_SEEN and mlst_bam_reads_info[0] count
 *     reads (windows plus uncut reads); n_records_out of mlst_submit_bam_bgzf keeps counting BAM records.
 *   A piece (the blocks of one call) without a kept read longer than read_len goes exactly the way it goes without the switch; one with
 *   such a read costs what a FASTQ chunk costs, below.  Unchanged: with the switch off, and on a PAIRED reads stream whatever the switch,
 *   l_seq > 320 fails with MLST_E_LIMIT "a BAM read is longer than 320 bases"; a record larger than the 1 MiB head room
 *   (MLST_BAM_MAX_RECORD: about 698,900 bases with qualities) fails with MLST_E_LIMIT "a BAM record of more than ... bytes"; a piece
 *   that makes 2^32 windows or more fails with MLST_E_LIMIT.  A long read whose l_seq claims more bases and qualities than its
 *   block_size holds ends the stream with MLST_E_INVALID "malformed BAM record <n>: its bases and qualities do not fit its size".
 * A chunk without a record longer than read_len goes the way it goes without the switch (one flag test).  A chunk with one costs three
 * small kernels, one host synchronisation (the window count sizes the buffers) and a kernel that writes every window's offsets;
 * the windows are packed and submitted in rounds of at most MLST_TILE_ROUND windows (environment, read by mlst_create; default
 * 16,777,216: a bound on the pack buffers, ~3.4 GB at 150 bases).  A chunk that makes 2^32 windows or more fails with MLST_E_LIMIT.
 * NOT tiled, a long record there fails with MLST_E_LIMIT as before: paired submissions (paired != 0, mlst_submit_fastq_pair,
 * mlst_submit_fastq_bgzf_pair), paired reads streams of a BAM (mlst_bam_reads_open with paired != 0), mlst_submit_reads /
 * mlst_submit_reads_device and the
 * host-packed entries (mlst_pack_fastq_host, mlst_submit_packed_host, mlst_submit_packed_device).
 * Refused: read_len or stride of 0 when the other is not (MLST_E_INVALID); read_len > 320 (MLST_E_LIMIT); a change while a FASTQ or
 * BAM stream is open on the handle (MLST_E_INVALID "a FASTQ stream is open", as mlst_set_bgzf_verify): the switch governs the streams
 * opened after it.
 * mlst_get_read_tiling_info: since the last mlst_reset_sample, out[0] = records seen by tiled submissions (FASTQ records, and the kept
 * records of tiled reads streams), out[1] = records cut, out[2] = windows made of them, out[3] = bases of the longest record. */
int mlst_set_read_tiling(mlst_handle* h, uint32_t read_len, uint32_t stride);
int mlst_get_read_tiling(mlst_handle* h, uint32_t* read_len, uint32_t* stride);
int mlst_get_read_tiling_info(mlst_handle* h, uint64_t out[4]);

/* Host-packed input: what crosses the link is 2-bit bases + lengths (42 bytes per 150-base read instead of the 316 of its
 * FASTQ text); the Phred rows stay on the host and only those of the reads that pass the seed sieve (one in ~400 of a
 * metagenome) follow.  mlst_pack_fastq_host: FASTQ text (whole 4-line records) -> `packed` in the engine's resident layout
 * (ceil(n / 64) * 64 * words_per_read words: groups of 64 reads, transposed in 8-byte units), `qrows` (n x qual_stride raw
 * Phred, bit 7 = non-ACGT base), `lens` (bit 15 = the read holds such a base) -- byte for byte what mlst_submit_fastq's
 * device-side parser makes of the same text; all host threads (threads <= 0: as many as the machine has, at most 128).
 * No handle: pure host code.  mlst_submit_packed_host: pass 1 from such arrays in HOST memory; one host synchronisation in
 * the middle (the candidate list comes back before the quality rows go out), so this entry is not replayed as a graph.
 * Replaces, like mlst_submit_fastq, the user-run `bowtie2 ... -U <fastq>` of /root/reference/README.md:20. */
int mlst_pack_fastq_host(const uint8_t* text, uint64_t n_bytes, uint32_t words_per_read, uint32_t qual_stride, uint32_t* packed,
                         uint8_t* qrows, uint16_t* lens, uint64_t cap_reads, uint64_t* n_reads_out, int threads);
int mlst_submit_packed_host(mlst_handle* h, const uint32_t* packed, const uint8_t* qrows, const uint16_t* lens, uint64_t n_reads,
                            uint32_t words_per_read, uint32_t qual_stride, int paired);

/* Same, with the three arrays already in DEVICE memory (GPU-side FASTQ decode feeds this). */
int mlst_submit_reads_device(mlst_handle* h, const uint8_t* d_bases, const uint8_t* d_quals,
                             const uint64_t* d_off, uint64_t n_reads, uint32_t max_len, int paired);

/* Pack ASCII reads (device) into the resident format (device): 2-bit bases in rows of
 * words_per_read uint32 (even; base k at bits 2(k%16) of word k/16, A=0 C=1 G=2 T=3), quality rows
 * of qual_stride bytes holding raw Phred with bit 7 set for a non-ACGT base, and uint16 lengths
 * (bit 15 = the read holds a non-ACGT base).  This is the layout SURVEY.md 8(d) prices at 38+150 B
 * per 150 bp read.
 * The 2-bit rows are stored in groups of 64 reads, transposed in 8-byte units so that 64 lanes
 * owning the 64 reads of a group load every unit with one coalesced 512-byte access: words 2u and
 * 2u+1 of read r are the uint32 at
 *     (r / 64) * 64 * words_per_read  +  ((u * 64 + r % 64) * 2)   and the one after it.
 * qual_stride must be a multiple of 4 (rows are written as 32-bit words) and d_qual_rows 4-byte aligned.
 * d_packed must hold ceil(n_reads / 64) * 64 * words_per_read words (the rows that pad the last
 * group are written as zeros) and be 16-byte aligned; a batch that is packed in pieces must cut the
 * pieces at multiples of 64 reads. */
int mlst_pack_reads_device(mlst_handle* h, const uint8_t* d_bases, const uint8_t* d_quals,
                           const uint64_t* d_off, uint64_t n_reads,
                           uint32_t* d_packed, uint8_t* d_qual_rows, uint16_t* d_lens,
                           uint32_t words_per_read, uint32_t qual_stride);

/* Pass 1 over a batch already resident in the packed format (the benchmark's timed entry). */
int mlst_submit_packed_device(mlst_handle* h, const uint32_t* d_packed, const uint8_t* d_qual_rows,
                              const uint16_t* d_lens, uint64_t n_reads,
                              uint32_t words_per_read, uint32_t qual_stride, int paired);

/* Read back pass-1 statistics.  Replaces the `cel` / `sequenceBank` dictionaries of
 * metamlst.py:116-127.  Any pointer may be NULL.
 *   sum_score[n_alleles]  int64  : sum of AS over accepted records of the allele
 *   n_hits[n_alleles]     uint32 : number of accepted records
 *   locus_read_len_sum[L] uint64 : sum of len(SEQ) over reads with an accepted record on the locus
 *   locus_first_read[L]   uint64 : smallest read index with an accepted record (UINT64_MAX if none; Q6)
 *   counters[MLST_CNT_N]  uint64 */
int mlst_get_allele_stats(mlst_handle* h, int64_t* sum_score, uint32_t* n_hits,
                          uint64_t* locus_read_len_sum, uint64_t* locus_first_read,
                          uint64_t* counters);

/* Multi-GPU: copy the additive statistics to / from a caller-owned DEVICE buffer so the
 * host can all-reduce them with torch.distributed (RCCL).  Layout of d_sum (int64):
 * [sum_score(n_alleles) | n_hits(n_alleles) | locus_read_len_sum(L) | counters(MLST_CNT_N)];
 * d_min (int64, reduce with MIN): [locus_first_read(L)] (INT64_MAX if none). */
int mlst_stats_flat_sizes(mlst_handle* h, uint64_t* n_sum, uint64_t* n_min);
int mlst_export_stats_device(mlst_handle* h, int64_t* d_sum, int64_t* d_min);
int mlst_import_stats_device(mlst_handle* h, const int64_t* d_sum, const int64_t* d_min);

/* Pass 2: pileup of the retained reads against one chosen allele per locus.  Replaces
 * cmseq get_base_stats over pysam pileup (metaMLST_functions.py:255-259).
 *   chosen_allele_idx[n] : indices into the loaded allele list (at most one per locus)
 *   counts : uint32[sum(len(chosen))][4] A,C,G,T, alleles in the order given.
 * A base is counted iff its record has AS >= minscore and XM <= max_xm (true XM),
 * Phred >= minqual and base in ACGT. */
int mlst_pileup(mlst_handle* h, const uint32_t* chosen_allele_idx, uint32_t n, uint32_t* counts);
int mlst_pileup_device(mlst_handle* h, const uint32_t* chosen_allele_idx, uint32_t n,
                       uint32_t* d_counts /* device, n_cols*4, zeroed by the call */, uint64_t* n_cols);
/* pysam's pileup(max_depth = 8000) (metaMLST_functions.py:255-259; policy MLST_DEPTH_CAP of mlst_policy.h) as a switch.
 * cap = 0 (default): every record counts.  cap = n: a column of a chosen allele sees only the first n records that span it
 * (aligned columns first to last, deleted columns inside included), records ordered by (read index, strand); every record
 * of the aligner counts towards the depth, the AS / XM / Phred / ACGT filters apply to what a column saw.  Applies to every
 * pile-up that follows (mlst_pileup*, mlst_consensus, mlst_typing_*); ~40 extra passes over the work items, so a
 * literal-parity mode.  Single-engine samples only: a rank of a sharded sample knows its own reads' records only. */
int mlst_set_depth_cap(mlst_handle* h, uint32_t cap);

/* Pass 2 with the majority rule applied on the GPU: the string cmseq's
 * reference_free_consensus(mincov, noneCharacter, ...) returns for each chosen contig
 * (metaMLST_functions.py:258-259), concatenated in the order given.  A column with fewer than
 * mincov counted bases is none_char; ties resolve A < C < G < T (MLST_TIE_ORDER).
 *   out_seq : sum(len(chosen)) bytes;  counts (optional, may be NULL): as mlst_pileup. */
int mlst_consensus(mlst_handle* h, const uint32_t* chosen_allele_idx, uint32_t n, uint32_t mincov,
                   char none_char, uint8_t* out_seq, uint32_t* counts);

/* Multi-GPU variant: majority rule over pileup counts that already sit in DEVICE memory (the all-reduced
 * counts of every rank); out_seq is host memory, n_cols bytes. */
int mlst_consensus_from_counts_device(mlst_handle* h, const uint32_t* d_counts, uint64_t n_cols, uint32_t mincov,
                                      char none_char, uint8_t* out_seq);

/* Pass 2 for ready-made alignments (a SAM / BAM produced by the documented bowtie2 command):
 * counts as mlst_pileup, over the records given.  Replaces the cmseq / pysam pileup of the BAM
 * (metaMLST_functions.py:255-259 [cmseq NOT IN TREE]): a base counts when its record's AS >= minscore and
 * XM <= max_xm (true tags), its Phred >= minqual and it is A/C/G/T; secondary records count (stepper 'nofilter').
 *   rec_allele  : allele index of the record's contig      rec_pos0 : leftmost reference position, 0-based
 *   cigar       : len << 4 | op with the BAM operation codes (M I D N S H P = X), cigar_off[n_rec+1] delimits records
 *   seq / qual  : ASCII bases and raw Phred (not +33), seq_off[n_rec+1] delimits records (SEQ as stored in SAM,
 *                 i.e. already on the reference strand)
 *   counts      : host, sum(len(chosen)) * 4 uint32. */
int mlst_pileup_alignments(mlst_handle* h, const uint32_t* chosen_allele_idx, uint32_t n_chosen, uint64_t n_rec,
                           const uint32_t* rec_allele, const int32_t* rec_pos0, const int32_t* rec_as, const int32_t* rec_xm,
                           const uint64_t* cigar_off, const uint32_t* cigar, const uint64_t* seq_off,
                           const uint8_t* seq, const uint8_t* qual, int32_t minscore, int32_t max_xm, int32_t minqual,
                           uint32_t* counts);

/* ---- the engine's own alignments to the chosen alleles, as records (what the reference leaves behind as a BAM) --------------------
 * mlst_alignments_export walks every work item (mlst_get_items) whose locus has a chosen allele and decides it exactly as the
 * pile-up decides that (item, chosen allele): the ungapped alignment, or the banded one when the gap trigger fires (the policy of
 * pass 1: MLST_DEF_GAP_TRIGGER_MM / _CLIP).  A record exists iff score >= the floor of the read's length && score > 0.  Records
 * that fail the AS / XM tag filter are exported too: they sit in a bowtie2 BAM and count towards depth.  mlst_set_depth_cap is
 * ignored: every record is exported.  The totals (records, CIGAR operations, bases) size the arrays of mlst_alignments_fetch:
 *   read_index  : index of the read in submission order (mlst_item.read_index)
 *   rec_allele  : index of the chosen allele among the loaded alleles     rec_diag : the item's diagonal
 *   rec_flags   : bit 0 the item's strand (1 = the read is reverse-complemented), bit 1 the banded alignment was taken (used_dp)
 *   rec_as / rec_xm : the true AS and XM, the values the pile-up's tag filter sees
 *   rec_pos0    : the leftmost aligned allele column, 0-based
 *   cigar       : len << 4 | op, BAM operation codes, in reference orientation; cigar_off[n_rec + 1] delimits records.
 *                 Ungapped: [bs S] (be - bs) M [(n - be) S] with the aligned span [bs, be) in oriented read coordinates, so
 *                 rec_pos0 = bs + diag.  Banded: the traceback from its end back to its start, written forwards as M / I / D runs,
 *                 S for the oriented bases in front of and behind the walk.  No operation has length 0.
 *   seq / qual  : ASCII on the reference strand (reverse-complemented for strand 1; 'N' where the read has no A/C/G/T) and the raw
 *                 Phred (not +33) in the same orientation; seq_off[n_rec + 1] delimits records.
 * The arrays from rec_allele on, rec_diag and rec_flags left out, have the layout mlst_pileup_alignments takes: piled up with the
 * engine's minscore / max_xm / minqual they give mlst_pileup's counts.  The order of the records is unspecified (it follows the item
 * list).  The sample's state is read and none of it is changed: the statistics, a later mlst_pileup* / mlst_typing_* and
 * mlst_reset_sample behave as before; an open BGZF piece is finished first.  Two host synchronisations per export (the item count
 * sizes the tables, the totals size the arrays).  A sample without reads gives 0 records.  The records stay on the device until
 * the next export.
 *   Refused: a call while a BAM, SAM or paired stream is open on the handle, two chosen alleles of one locus, an allele out of
 *   range: MLST_E_INVALID.  mlst_alignments_fetch without a finished export (a refused one leaves none): MLST_E_INVALID. */
int mlst_alignments_export(mlst_handle* h, const uint32_t* chosen_allele_idx, uint32_t n,
                           uint64_t* n_rec_out, uint64_t* n_cigar_out, uint64_t* n_bases_out);
int mlst_alignments_fetch(mlst_handle* h, uint64_t* read_index, uint32_t* rec_allele, int32_t* rec_pos0, int32_t* rec_as,
                          int32_t* rec_xm, int32_t* rec_diag, uint8_t* rec_flags /* bit 0 strand, bit 1 used_dp */,
                          uint64_t* cigar_off /* n_rec+1 */, uint32_t* cigar, uint64_t* seq_off /* n_rec+1 */,
                          uint8_t* seq, uint8_t* qual);

/* ---- EVERY alignment of the sample as SAM text, formatted on the device (what `bowtie2 -a` leaves in front of metamlst.py) ---------
 * Records: one for every (work item, allele of the item's locus) whose alignment, decided exactly as pass 1 decides that pair
 *   (oracle/mlst_oracle.c: align_pair -- the ungapped alignment, or the banded one where the gap trigger fires), has
 *   score >= the floor of the read's length && score > 0: the records pass 1 counts in MLST_CNT_TOTAL_RECORDS.  Records that fail the
 *   AS / XM tag filter are written too; mlst_set_depth_cap is ignored.
 * Header: the caller's (metamlst_amd/samout.py: @HD VN:1.6 SO:unsorted GO:query, one @SQ per loaded allele in index order, @PG).
 * Order: work items by (read index, locus index, strand, diag), inside an item the alleles ascending: all records of a read are
 *   consecutive.  The bytes depend neither on the order of the item list nor on round_bytes.
 * Columns: QNAME r<k>, k = the read index (read index >> 1 with paired != 0), or the read's own name with mlst_set_read_names
 *   (below); FLAG 16 * strand, plus 256 on every record of a read
 *   index except its best one (the highest AS, ties to the first in file order); RNAME the allele's label; POS = the leftmost aligned
 *   column + 1; MAPQ 255; CIGAR as mlst_alignments_fetch describes it; * 0 0; SEQ on the reference strand; QUAL chr(min(q, 93) + 33);
 *   AS:i [XS:i] XN:i:0 XM:i XO:i XG:i NM:i YT:Z:UU.  XS:i is present iff the read index has two records or more, and is the
 *   highest AS among the read's other records (a read with one record has XO in the 15th column: quirk Q1 by construction).  AS and XM
 *   are the true values; XO = the I and D runs, XG = their columns, NM = XG + the M columns whose SEQ letter is not the allele's (an N
 *   on either side included).
 * mlst_alignments_text_open sorts the item list (on the host, per item), bounds every item's text from above -- (alleles of its locus)
 *   x (10 n + the longest label + 192 bytes for a read of n bases) -- and cuts the list into rounds of at most round_bytes (0: 256 MiB)
 *   of bounded text at read boundaries.  A read whose own bound exceeds round_bytes: MLST_E_LIMIT, the message names the bytes
 *   needed.  names / name_off[n_alleles + 1]: the RNAME labels, uploaded once per open.
 * mlst_alignments_text_next formats one round: whole lines only, n_bytes of them into text (host memory of cap bytes), n_records
 *   lines; done = 1 with the last round (and with n_bytes = 0 when there is none left).  text = NULL with cap = 0 asks for the size of
 *   the round that comes next (n_bytes, n_records; done = 1 iff none is left) and consumes nothing.
 * The sample's state is read and none of it is changed: the statistics, a later mlst_pileup* / mlst_typing_* / mlst_alignments_export
 *   and mlst_reset_sample behave as before (a reset closes the export); an open BGZF piece is finished first.
 *   Refused with MLST_E_INVALID: a call while a BAM, SAM or paired stream is open on the handle, mlst_alignments_text_next without an
 *   open export, cap smaller than the round. */
int mlst_alignments_text_open(mlst_handle* h, const uint8_t* names, const uint64_t* name_off /* n_alleles+1 */, int paired,
                              uint64_t round_bytes /* 0: 256 MiB */);
int mlst_alignments_text_next(mlst_handle* h, uint8_t* text, uint64_t cap, uint64_t* n_bytes, uint64_t* n_records, int* done);
int mlst_alignments_text_close(mlst_handle* h);

/* ---- the reads that align to the loci as FASTQ text, formatted on the device (what `bowtie2 --al FILE` writes; csrc/reads_text.h) -------
 * Which reads: a read index is written iff it has at least one record in the export above -- some (work item of the read, allele of
 *   the item's locus) whose alignment, decided exactly as pass 1 decides it, has score >= the floor of the read's length && score > 0:
 *   the records mlst_alignments_text_* writes and MLST_CNT_TOTAL_RECORDS counts.  Records that fail the AS / XM tag filter count;
 *   mlst_set_depth_cap is ignored.  A retained read without a record is not written.  The pairs are decided by the kernels of that
 *   export, so the set is its QNAMEs by construction.
 * Order: ascending read index; each read once, however many records it has.
 * Record: four lines with LF ends, `@<name>` / SEQ / `+` / QUAL.  <name> is the QNAME of the export above: r<k>, k = the read index
 *   (read index >> 1 with paired != 0), or with mlst_set_read_names the kept name (r<k> for a fallback).  With paired != 0 `/1` follows for
 *   an even read index and `/2` for an odd one (the mates share a QNAME; a FASTQ must tell them apart).  SEQ is the read as the engine
 *   holds it -- prepared and cut where mlst_set_read_prep / mlst_set_read_adapters ran --, in read orientation, never turned to the
 *   reference strand: ACGT, and N where the stored quality byte has bit 7 set.  QUAL is chr(min(q, 93) + 33) of the stored Phred.
 * Mates: each mate is written on its own, and only if it has a record itself -- the engine does not retain a mate that hit nothing.
 * mlst_reads_text_open plans the rounds with the planner of mlst_alignments_text_open (the same sort, rounds cut at read boundaries).
 *   What is summed against round_bytes (0: 256 MiB) per read of n bases with P (item, allele) pairs is
 *       max(2 n + max(21, the longest kept name) + 10,  36 P)
 *   -- a bound on its text (`@`, r + 20 digits or the name, `/1`, SEQ, `+`, QUAL, four LFs), or the bytes of the round's device tables
 *   for its pairs (AtPair 20, the entry of the banded list 8, the offsets entry 8), whichever is larger: for an isolate the tables
 *   dominate the text by orders of magnitude, and device memory for a round stays O(round_bytes).  A read whose own bound exceeds
 *   round_bytes: MLST_E_LIMIT, the message names the bytes needed.  The bytes depend neither on the order of the item list nor on
 *   round_bytes.
 * mlst_reads_text_next formats one round: whole records only, n_bytes of them into text (host memory of cap bytes), n_reads records;
 *   done = 1 with the last round that holds text, and at once (n_bytes = 0) when no read is left that has a record.  text = NULL with
 *   cap = 0 asks for the size of the round that comes next and consumes nothing.
 * The sample's state is read and none of it is changed; an open BGZF piece is finished first; mlst_reset_sample closes the export.
 * One text export exists at a time: opening either kind closes whichever was open, and _next of the kind that is not open is
 *   MLST_E_INVALID.  Also refused with MLST_E_INVALID: a call while a BAM, SAM or paired stream is open on the handle,
 *   mlst_reads_text_next without an open export, cap smaller than the round.  mlst_set_export_md has no bearing on this export. */
int mlst_reads_text_open(mlst_handle* h, int paired, uint64_t round_bytes /* 0: 256 MiB */);
int mlst_reads_text_next(mlst_handle* h, uint8_t* text, uint64_t cap, uint64_t* n_bytes, uint64_t* n_reads, int* done);
int mlst_reads_text_close(mlst_handle* h);

/* ---- the reads' own names as QNAME (off by default; csrc/read_names.h; `cli type --read-names`) ---------------------------------------
 * mlst_set_read_names(h, 1): the name of every read pass 1 retains is copied out of the FASTQ text on the device, before the text
 *   slot of its chunk is reused; mlst_alignments_text_* then writes that name as QNAME and mlst_read_names_fetch hands the names to the
 *   host (metamlst_amd.samout.write_sam).  With the switch off nothing is queued and nothing is allocated.
 * The rule (metamlst_amd.samout.read_qname states it in Python): the name is the header line's bytes behind the '@' up to, not
 *   including, the first space, TAB, CR or LF (bowtie2's rule).  A name that is no legal SAM QNAME ([!-?A-~]{1,254}: empty, longer than
 *   254 bytes, a '@' or a byte outside '!'..'~' in it) is not kept: the read's QNAME stays r<k> as without the switch, and the read is
 *   counted as a fallback.  Every read carries its own name, mates included (paired != 0 changes the k of a fallback only).
 * Entries that carry names: mlst_submit_fastq, mlst_submit_fastq_stream, mlst_submit_fastq_pair, mlst_submit_fastq_bgzf and
 *   mlst_submit_fastq_bgzf_pair.  With the switch on every other way of adding reads (mlst_submit_reads, mlst_submit_reads_device,
 *   mlst_submit_packed_device, mlst_submit_packed_host, mlst_submit_fasta, mlst_bam_reads_open) and mlst_set_read_tiling with a tile
 *   are refused with MLST_E_INVALID ("read names are on ..."), as is mlst_set_read_names(h, 1) behind mlst_set_read_tiling.
 * The switch may change only while the sample holds no reads (before the first submission or behind mlst_reset_sample; a non-zero
 *   mlst_set_read_index_base counts as reads: set the switch first) and no stream is open: MLST_E_INVALID otherwise.
 *   mlst_reset_sample empties the arena and keeps the switch.
 * Memory: the bytes of the kept names in an arena of MLST_NAMES_BYTES bytes (environment, read by mlst_create; default 256 MiB),
 *   offset and length per retained slot; allocated by the first submission under the switch.  An arena that is too small loses no
 *   statistics: the next entry that fetches statistics, names or the text export fails with MLST_E_LIMIT and names the bytes needed.
 * mlst_read_names_info: out[0] = retained reads with a kept name, out[1] = bytes of the kept names, out[2] = fallbacks (retained
 *   reads whose name was not kept), out[3] = the longest kept name in bytes.  All zero with the switch off.
 * mlst_read_names_fetch: read_index[n], off[n + 1], bytes[out[1]] with n = out[0] of mlst_read_names_info: the name of read
 *   read_index[i] is bytes[off[i] .. off[i + 1]).  The order is unspecified.  An open BGZF piece is finished first by both.
 * The text export bounds a line with the longest kept name in place of the 21 bytes of r<k> where that is longer. */
int mlst_set_read_names(mlst_handle* h, int on);
int mlst_get_read_names(mlst_handle* h, int* on);
int mlst_read_names_info(mlst_handle* h, uint64_t out[4]);
int mlst_read_names_fetch(mlst_handle* h, uint64_t* read_index /* n */, uint64_t* off /* n+1 */, uint8_t* bytes);

/* ---- reads prepared before they are aligned (off by default; csrc/read_prep.h; `cli type --trim5 / --trim3 / --trim-qual / --phred64`) --
 * mlst_set_read_prep(h, &p): every read of FASTQ text is changed on the device before it is packed, as bowtie2 -5 / -3 / --phred64 and a
 *   3' quality trimmer in front of it would have changed it; the engine then behaves as if it had been given the prepared text
 *   (metamlst_amd.fastq.prep_fastq states the rule in Python and writes that text).  NULL or {0, 0, 0, 33} is off: nothing is queued,
 *   nothing is allocated, and the kernels that run are those that ran before the switch existed.
 * The rule, per record, in this order (header and '+' line are not looked at):
 *   1. Phred: q[i] = clamp(character - phred_base, 0, 127), phred_base 33 or 64 (Illumina 1.3 - 1.7, bowtie2 --phred64).
 *   2. Fixed trims (bowtie2's): a = min(trim5, n), n1 = max(0, n - trim5 - trim3); bases and qualities [a, a + n1) remain.
 *   3. Quality trim of the 3' end (cutadapt -q T / bwa aln -q T, no minimum length) on what remains, T = trim_qual, 0 = off:
 *        s = 0, best = 0, cut = n1;  for i = n1 - 1 .. 0: s += T - q[a + i]; stop when s < 0; if s > best: best = s, cut = i
 *      and cut bases remain.
 *   4. A read left without a base stays a read of length 0: read indices, pairing and the names of mlst_set_read_names are those of
 *      the file.  It holds no seed and leaves no candidate.  Each mate of a pair is prepared on its own.
 *   A malformed record (sequence and quality lengths differ) and a read beyond MLST_MAX_READ_LEN are judged on the record as it stands
 *   in the file, before the trims.
 * Entries it applies to: mlst_submit_fastq, mlst_submit_fastq_stream, mlst_submit_fastq_pair, mlst_submit_fastq_bgzf and
 *   mlst_submit_fastq_bgzf_pair.  With the switch on every other way of adding reads (mlst_submit_reads, mlst_submit_reads_device,
 *   mlst_submit_packed_device, mlst_submit_packed_host, mlst_submit_fasta, mlst_bam_reads_open) and mlst_set_read_tiling with a tile
 *   are refused with MLST_E_INVALID ("<entry>: read preparation is on ..."), as is a setting other than off behind
 *   mlst_set_read_tiling: a read that silently kept its tail would be worse than a refusal.  It combines with mlst_set_read_names.
 * The setting may change only while the sample holds no reads (before the first submission or behind mlst_reset_sample; a non-zero
 *   mlst_set_read_index_base counts as reads) and no stream is open: MLST_E_INVALID otherwise.  phred_base other than 33 / 64,
 *   trim_qual > 93 or a trim > 65535: MLST_E_INVALID.  mlst_reset_sample zeroes the counters and keeps the setting.
 * mlst_read_prep_info: out[0] = reads whose length changed, out[1] = bases removed, out[2] = reads of length >= 1 left without a base,
 *   out[3] = 0.  All zero with the switch off.  An open BGZF piece is finished first.
 * The packed rows (width, quality stride, lens with bit 15 for a non-ACGT base among the remaining bases only) are those of the
 *   prepared text; no host synchronisation is added per chunk. */
typedef struct { uint32_t trim5, trim3, trim_qual, phred_base; } mlst_read_prep;   /* phred_base 33 or 64 */
int mlst_set_read_prep(mlst_handle* h, const mlst_read_prep* p);
int mlst_get_read_prep(mlst_handle* h, mlst_read_prep* out);
int mlst_read_prep_info(mlst_handle* h, uint64_t out[4]);

/* ---- 3' adapters removed before the reads are aligned (off by default; csrc/read_adapt.h; `cli type --adapter`) -------------------------
 * mlst_set_read_adapters(h, "SEQ[,SEQ...]", min_overlap, error_permille): a 3' adapter is removed from every read of FASTQ text on the
 *   device before it is packed; the engine then behaves as if it had been given the cut text (metamlst_amd.fastq.adapter_cut /
 *   trim_adapters state the rule in Python and write that text).  NULL or "" is off: nothing is queued, nothing is allocated, and the
 *   kernels that run are those that ran before the switch existed.
 * The rule is the project's own, modelled on `cutadapt -a ADAPTER --no-indels --times 1`; it does not claim cutadapt's bytes.  For a
 *   read of n bases and the adapters A_0 .. A_{K-1} (1 <= K <= 8; A_k: m_k letters of ACGTN, 1 <= m_k <= 64, at least one not N;
 *   either case, kept upper-cased):
 *   1. A candidate is an adapter k and a start p, 0 <= p <= n - min(min_overlap, m_k).  Its overlap is L = min(m_k, n - p): the
 *      adapter lies inside the read or hangs over its 3' end, never over the 5' end.
 *   2. Position i < L matches if A_k[i] is N, or if the read's byte at p + i, upper-cased, equals A_k[i] -- a non-ACGT byte of the
 *      read, N included, matches only an adapter N.  mism = L - matches.
 *   3. The candidate is valid if mism <= (L * error_permille) / 1000, in integers.
 *   4. The cut is the valid candidate with the most matches; among equals the smallest p, then the smallest k.  Bases and qualities
 *      [0, p) remain.  With no valid candidate the read is untouched.  One adapter is removed per read.
 *   5. It runs behind mlst_set_read_prep's steps (Phred base, fixed trims, quality trim -- cutadapt trims by quality first), on what
 *      they left.  A read left without a base stays a read of length 0; read indices, pairing and the names of mlst_set_read_names are
 *      those of the file.  Each mate of a pair is cut on its own, against the same adapters.
 *   At min_overlap 3 (cutadapt's default) about 2 % of random reads lose three or more bases by chance.
 * Entries it applies to, the entries refused while it is on ("<entry>: adapter removal is on (mlst_set_read_adapters) ...") and when
 *   the setting may change: exactly as for mlst_set_read_prep, with which it combines, as it does with mlst_set_read_names and the
 *   exports (they carry the cut SEQ / QUAL).  A letter outside ACGTN, an empty adapter or one of only Ns, more than 8 adapters, one
 *   longer than 64 letters, min_overlap outside 1..64, error_permille above 500: MLST_E_INVALID with the reason.  mlst_reset_sample
 *   zeroes the counters and keeps the setting.
 * mlst_get_read_adapters: the adapters as set, upper-cased and comma-separated, into adapters[cap] (NULL: not wanted; "" when off; at
 *   most 8 * 65 bytes with the final 0), and the two numbers (0, 0 when off).
 * mlst_get_read_adapters_info: out[0] = reads cut, out[1] = bases removed, out[2] = reads of length >= 1 cut at 0, out[3] = K,
 *   out[4 + k] = reads cut at adapter k.  The counters are separate from mlst_read_prep_info's.  An open BGZF piece is finished first. */
int mlst_set_read_adapters(mlst_handle* h, const char* adapters, uint32_t min_overlap, uint32_t error_permille);
int mlst_get_read_adapters(mlst_handle* h, char* adapters, uint64_t cap, uint32_t* min_overlap, uint32_t* error_permille);
int mlst_get_read_adapters_info(mlst_handle* h, uint64_t out[12]);

/* ---- per-cycle read statistics counted on the device (off by default; csrc/read_stats.h; `cli type --read-stats`) ----------------------
 * mlst_set_read_stats(h, 1): every read of FASTQ text is counted into per-cycle tables on the device, next to the parser, from bytes that
 *   are already there (metamlst_amd.fastq.read_stats states the rule in Python).  Typing is untouched: packed rows, statistics, counters
 *   and exports are the bytes they are without the switch.  Off: nothing is queued, nothing is allocated, and the kernels that run are
 *   those that ran before the switch existed.
 * The rule, per side (0 = unpaired reads and first mates, 1 = second mates) and stage, over the records counted:
 *   reads, bases (the sum of lengths);
 *   len_hist[0..320]: reads by length (a read of length 0 counts here and in reads only);
 *   base[c][0..4], c = 0..319: letters A, C, G, T (either case) and other at cycle c -- "other" is every byte the packed rows mark as a
 *     non-ACGT base (N, IUPAC codes, '.', anything else);
 *   qual[c][0..93]: Phred at cycle c = min(clamp(character - phred_base, 0, 127), 93), the character taken as 0..255 and phred_base
 *     that of mlst_set_read_prep (33, or 64); under 33 every character of 128 and above lands in bin 93;
 *   gc_hist[0..100]: reads of length n >= 1 by (100 * (#G + #C)) / n;  readqual_hist[0..93]: reads of length n >= 1 by (sum of Phred) / n,
 *     Phred as binned above, both in integers;
 *   clamped_low: quality characters below phred_base (stage raw only: a Phred+33 file read as Phred+64 shows here).
 * Sides: in a paired submission read 2k is side 0 and read 2k + 1 side 1; an unpaired submission counts into the current side,
 *   mlst_set_read_stats_side(h, 0 | 1), which may change whenever no stream is open and is 0 again behind mlst_reset_sample (mate files
 *   whose names differ go in as two unpaired texts and are still reported apart).
 * Stages: 0 = raw, the record as it stands in the file (offsets and lengths as the parser leaves them); 1 = prepared, the read as it is
 *   packed, behind mlst_set_read_prep's trims and mlst_set_read_adapters' cut, cycle 0 at the first remaining base.  With neither a trim
 *   nor an adapter set only raw is counted (one launch per chunk, not two) and stage 1 is reported as stage 0's block.
 * Entries it applies to: the five FASTQ entries (mlst_submit_fastq, _stream, _pair, _bgzf, _bgzf_pair).  While it is on every other way
 *   of adding reads and mlst_set_read_tiling with a tile are refused with MLST_E_INVALID ("<entry>: read statistics are on
 *   (mlst_set_read_stats) ..."): a report that silently covered part of a sample would be worse than a refusal.  It combines with
 *   mlst_set_read_names, mlst_set_read_prep, mlst_set_read_adapters and the exports.  The switch may change only while the sample holds
 *   no reads and no stream is open (mlst_set_read_prep's test).  mlst_reset_sample zeroes the tables and keeps the switch.
 * mlst_read_stats_fetch(h, stage, side, out, cap): one block of MLST_RS_WORDS 64-bit counters (cap >= MLST_RS_WORDS, else MLST_E_INVALID):
 *   out[MLST_RS_READS], out[MLST_RS_BASES], out[MLST_RS_CLAMPED_LOW], one word of padding, then len_hist at MLST_RS_LEN (321),
 *   base[320][5] at MLST_RS_BASE, qual[320][94] at MLST_RS_QUAL, gc_hist at MLST_RS_GC (101), readqual_hist at MLST_RS_READQUAL (94).
 *   All zero with the switch off.  An open BGZF piece is finished first.  A chunk refused as malformed is not counted.
 * mlst_read_stats_info: out[0] = launches of stage raw, out[1] = launches of stage prepared, out[2] = table bytes allocated, out[3] = 0.
 * No host synchronisation is added per chunk; mlst_get_kernel_time 20 is the counting kernel alone. */
#define MLST_RS_READS 0
#define MLST_RS_BASES 1
#define MLST_RS_CLAMPED_LOW 2
#define MLST_RS_LEN 4
#define MLST_RS_BASE 325
#define MLST_RS_QUAL 1925
#define MLST_RS_GC 32005
#define MLST_RS_READQUAL 32106
#define MLST_RS_WORDS 32200
int mlst_set_read_stats(mlst_handle* h, int on);
int mlst_get_read_stats(mlst_handle* h, int* on);
int mlst_set_read_stats_side(mlst_handle* h, int side);
int mlst_read_stats_fetch(mlst_handle* h, int stage, int side, uint64_t* out, uint64_t cap);
int mlst_read_stats_info(mlst_handle* h, uint64_t out[4]);

/* ---- exact duplicate reads removed before the reads are aligned (off by default; csrc/read_dedup.h; `cli type --dedup`) -----------------
 * mlst_set_read_dedup(h, 1): every read (every pair) of FASTQ text that repeats an earlier one of the sample is emptied on the device
 *   before it is packed; the engine then behaves as if it had been given the deduplicated text (metamlst_amd.fastq.dedup_fastq states
 *   the rule in Python and writes that text).  Off: nothing is queued, nothing is allocated, and the kernels that run are those that ran
 *   before the switch existed.
 * The rule:
 *   1. Letters.  A read's letters are its sequence as the engine aligns it: A C G T in either case stand for themselves, every other
 *      byte is N (the N bit of the packed rows).  The read's key is (length, folded letters); qualities and names play no part.
 *   2. Unpaired submissions: read r is a duplicate if a read with a lower read index in the sample has the same key.  The first
 *      occurrence is kept.
 *   3. Paired submissions: the unit is the pair.  Pair j is a duplicate if an earlier pair has the same key for mate 1 AND the same key
 *      for mate 2, in that order; swapped mates are not duplicates.  Both mates of a duplicate pair go, otherwise both stay.
 *   4. A read of length 0 is neither a duplicate nor a first occurrence, nor is a pair whose mates are both empty.  A pair with one empty
 *      mate takes part as it is.
 *   5. A duplicate stays a read of length 0 (mlst_set_read_prep's rule 4): read indices, pairing and the names of mlst_set_read_names
 *      are those of the file.  It holds no seed, leaves no candidate and appears in no export.
 *   6. Only the same orientation counts: a reverse complement is not a duplicate (fastp's and FastUniq's rule).
 *   7. It runs behind mlst_set_read_prep's steps and mlst_set_read_adapters' cut, on what they left: two reads that differ only in a
 *      tail the quality trim removes are duplicates.  The tables of mlst_set_read_stats are counted in front of it and are what they are
 *      without it.
 *   On the device a unit is its 128-bit key (MLST_DEDUP_KEY of mlst_policy.h): the rule above holds unless two different units share
 *   all 128 bits.  Two units that share the first 64 bits only are a clash: both are kept, the later one is counted in out[6].
 * The keys live in a hash table on the device that belongs to the handle: 28 bytes per slot, MLST_DEDUP_SLOTS slots at first (a power
 *   of two >= 64, default 2^22; read when the table is made), doubled and rehashed on the device whenever it would hold fewer than two
 *   slots per unit submitted; 48 M reads end at 2^27 slots, 3.75 GB.  An allocation that fails is MLST_E_LIMIT with the bytes needed.
 *   MLST_DEDUP_TAG_BITS (test switch, default 64, read when the table is made): only that many low bits of the first hash are used.
 * Entries it applies to, the entries refused while it is on ("<entry>: duplicate removal is on (mlst_set_read_dedup) ...") and when the
 *   switch may change: exactly as for mlst_set_read_prep, with which it combines, as it does with mlst_set_read_adapters,
 *   mlst_set_read_stats, mlst_set_read_names and the exports.  mlst_reset_sample empties the table, zeroes the counters and keeps the
 *   switch.  The result does not depend on how the text was cut into chunks; a paired chunk must hold whole pairs (every paired entry
 *   sees to that; a paired mlst_submit_fastq_stream chunk cut behind a first mate is refused with MLST_E_INVALID).
 * mlst_read_dedup_info: out[0] = reads seen, out[1] = units (reads or pairs) that took part, out[2] = duplicates (units removed),
 *   out[3] = reads removed, out[4] = bases removed, out[5] = distinct keys, out[6] = clashes, out[7] = slots of the table,
 *   out[8 + k], k = 0..7 = distinct keys that occur 1, 2, 3, 4, 5-9, 10-49, 50-499 and >= 500 times.  All zero with the switch off.  An
 *   open BGZF piece is finished first.
 * No host synchronisation is added per chunk; mlst_get_kernel_time 21 is the three launches of a chunk together. */
int mlst_set_read_dedup(mlst_handle* h, int on);
int mlst_get_read_dedup(mlst_handle* h, int* on);
int mlst_read_dedup_info(mlst_handle* h, uint64_t out[16]);

/* ---- adapter read-through trimmed from the overlap of the mates (off by default; csrc/read_overlap.h; `cli type -2 MATES --pair-overlap`) --
 * mlst_set_read_pair_overlap(h, 1, min_overlap, max_mismatches, error_permille): when the insert is shorter than the reads, both mates
 *   run through it into the adapter.  The mates overlap as reverse complements, so the overlap says where the insert ends: both mates
 *   of a paired FASTQ submission are cut there on the device before they are packed, and no adapter sequence is needed.  The engine then
 *   behaves as if it had been given the cut text (metamlst_amd.fastq.pair_overlap / trim_pair_overlap state the rule in Python and write
 *   that text).  Off: nothing is queued, nothing is allocated, and the kernels that run are those that ran before the switch existed.
 *   MLST_E_INVALID for min_overlap outside 8..320, max_mismatches outside 0..64, error_permille outside 0..500 (fastp's defaults:
 *   30, 5, 200), and while mlst_set_read_window holds a front cut (see there).  The rule is modelled on fastp's overlap analysis (no indels); it is the project's own and claims none of fastp's bytes.
 * The rule, per pair (mate 1 of n1 letters, mate 2 of n2):
 *   1. Letters are folded as mlst_set_read_dedup folds them: A C G T in either case stand for themselves, every other byte is N.  c2 is
 *      the reverse complement of mate 2; the complement of N is N.
 *   2. A candidate is an offset o: letter j of c2 lies on letter o + j of mate 1, -(n2 - min_overlap) <= o <= n1 - min_overlap.  Its
 *      overlap is positions max(0, o) .. min(n1, o + n2) - 1 of mate 1, L of them.  A candidate with L < min_overlap is none: a mate
 *      shorter than min_overlap has no candidate.
 *   3. A position matches if both letters are one of ACGT and equal; an N on either side is a mismatch.  mism = L - matches.
 *   4. A candidate is valid if mism <= max_mismatches and mism <= (L * error_permille) / 1000, in integers.
 *   5. The valid candidate with the most matches is chosen; among equals the smallest o.
 *   6. The insert then ends at I = o + n2 + trim5 in the coordinates of either prepared mate, trim5 being mlst_set_read_prep's (both
 *      mates lost that many bases in front).  Mate 1 keeps min(n1, I) bases and qualities, mate 2 min(n2, I).  A pair without a
 *      candidate stays as it is, and so does one whose I cuts neither mate: mates that overlap in their middles.
 *   7. A mate left without a base stays a read of length 0 (mlst_set_read_prep's rule 4).
 *   8. It runs behind mlst_set_read_prep's steps and mlst_set_read_adapters' cut and in front of mlst_set_read_dedup; the prepared tables
 *      of mlst_set_read_stats are counted behind it (also when it is the only step that ran).
 *   Limits: an insert shorter than min_overlap is not seen (that is mlst_set_read_adapters' job); two mates of one low-complexity repeat
 *   can overlap at a wrong offset.  Not done: correcting mismatching bases inside the overlap, merging the mates into one read.
 * Entries it applies to: the paired forms of the FASTQ entries -- mlst_submit_fastq and mlst_submit_fastq_stream with paired,
 *   mlst_submit_fastq_pair, mlst_submit_fastq_bgzf with paired, mlst_submit_fastq_bgzf_pair.  While it is on every other way of adding
 *   reads is MLST_E_INVALID with a reason: the entries mlst_set_read_dedup refuses ("<entry>: mate overlap trimming is on
 *   (mlst_set_read_pair_overlap) ..."), mlst_set_read_tiling, an unpaired FASTQ submission, and a paired chunk with an odd number of
 *   records (a paired mlst_submit_fastq_stream chunk cut behind a first mate; a BGZF piece that ends behind a first mate keeps
 *   that record for the next piece instead).  When the switch and its setting may change: exactly as
 *   for mlst_set_read_prep.  mlst_reset_sample zeroes the counters and keeps the switch and its setting.  The result does not depend on
 *   how the text was cut into chunks.
 * mlst_get_read_pair_overlap: the switch and the setting (the three pointers may be NULL).
 * mlst_read_pair_overlap_info: out[0] = pairs seen, out[1] = overlapping pairs (those with a chosen candidate), out[2] = pairs of which
 *   a mate was cut, out[3] = reads cut, out[4] = bases removed, out[5] = mates of length >= 1 left without a base, out[6..7] = 0.
 * mlst_read_pair_overlap_hist: MLST_PO_HIST words; word k = overlapping pairs with min(o + n2 + 2 * trim5, MLST_PO_HIST - 1) == k, the
 *   fragment length in the file's coordinates, each overlapping pair counted once.  cap < MLST_PO_HIST is MLST_E_INVALID.
 *   Both are all zero with the switch off; an open BGZF piece is finished first.
 * No host synchronisation is added per chunk; mlst_get_kernel_time 22 is k_po_cut alone. */
#define MLST_PO_HIST 1024
int mlst_set_read_pair_overlap(mlst_handle* h, int on, uint32_t min_overlap, uint32_t max_mismatches, uint32_t error_permille);
int mlst_get_read_pair_overlap(mlst_handle* h, int* on, uint32_t* min_overlap, uint32_t* max_mismatches, uint32_t* error_permille);
int mlst_read_pair_overlap_info(mlst_handle* h, uint64_t out[8]);
int mlst_read_pair_overlap_hist(mlst_handle* h, uint64_t* out, uint64_t cap);

/* ---- poly-G / poly-X tails trimmed and reads filtered (off by default; csrc/read_filter.h; `cli type --trim-poly-g / --trim-poly-x /
 * --min-length / --max-n / --low-complexity / --min-mean-qual`) ------------------------------------------------------------------------
 * mlst_set_read_filter(h, &f): two-colour machines (NovaSeq, NextSeq) call G where a cluster gives no signal, so reads of short inserts
 *   and of dying clusters end in a run of G of high quality that neither the quality trim nor the adapter cut sees; and a read that the
 *   trims left very short, that holds many Ns, that is one repeated letter pair or whose qualities are low is better not aligned at
 *   all.  Both are done on the device before the reads are packed, and the engine then behaves as if it had been given the filtered text
 *   (metamlst_amd.fastq.poly_tail / read_fails / filter_fastq state the rule in Python and write that text).  NULL or a struct with
 *   everything off (poly_mask 0, min_length 0, max_n MLST_RF_NO_LIMIT, complexity_pct 0, mean_qual 0) switches the stage off: nothing
 *   is queued, nothing is allocated, and the kernels that run are those that ran before the switch existed.  MLST_E_INVALID, with a
 *   sentence that names the field and its range, for poly_mask outside 0..15, poly_min outside 1..320 (looked at only with a poly_mask),
 *   min_length outside 0..320, complexity_pct outside 0..100, mean_qual outside 0..93 (every max_n is taken).
 *   The rule is modelled on fastp's --trim_poly_g / --trim_poly_x and its filters; it is the project's own and claims none of fastp's bytes.
 * The rule, per read of n bases (integers only):
 *   1. Letters are folded to upper case; a byte that is none of A C G T matches no letter.
 *   2. The tail (poly_mask: bit 0 = A, 1 = C, 2 = G, 3 = T; 0 = no tail trim).  For a letter X of the mask and a tail length L in 1..n,
 *      mism(L) is the number of the last L bases that are not X.  L is valid if L >= poly_min, the base at n - L is X (the tail begins
 *      on its letter) and mism(L) <= min(5, L / 8).  The largest valid L over all letters is cut: n - L bases and qualities remain.  Two
 *      letters cannot share a valid L.  A tail may step over a mismatch onto an earlier X: ten times ACGT and ten G are cut to 38.
 *   3. The filters judge what the tail trim left, n bases again; the first that holds empties the read.  A read of length 0 fails none.
 *        too short:       n < min_length
 *        too many N:      more than max_n bytes that are none of A C G T in either case (MLST_RF_NO_LIMIT: off)
 *        low complexity:  n >= 2 and 100 * d < complexity_pct * (n - 1), d = the positions i in [0, n - 1) whose folded letters at i and
 *                         i + 1 differ, every byte that is none of A C G T folded to N
 *        low quality:     sum(q) < mean_qual * n, q = clamp(character - phred base, 0, 127), the base mlst_set_read_prep's
 *   4. A read left without a base stays a read of length 0 (mlst_set_read_prep's rule 4).  Each mate of a pair is treated on its own: the
 *      partner of a failed mate stays.
 *   5. It runs behind mlst_set_read_prep's steps, mlst_set_read_adapters' cut and mlst_set_read_pair_overlap's cut (a tail outside the
 *      mates' overlap does not hinder that) and in front of mlst_set_read_dedup; the prepared tables of mlst_set_read_stats are counted
 *      behind it (also when it is the only step that ran): the filter judges the read as it is aligned.
 * Entries it applies to, what is refused while it is on ("<entry>: the read filter is on (mlst_set_read_filter) ..."), when the setting
 *   may change and what mlst_reset_sample does: exactly as for mlst_set_read_adapters.
 * mlst_get_read_filter: the setting (all off with the switch off).
 * mlst_read_filter_info: out[0] = reads whose tail was cut, out[1] = bases removed with the tails, out[2..5] = reads cut by the tail's
 *   letter (A, C, G, T), out[6] = reads of length >= 1 that were one tail, out[7] = reads emptied as too short, out[8] = with too many N,
 *   out[9] = of low complexity, out[10] = of low quality, out[11] = the bases those reads held behind the tail trim, out[12..15] = 0.
 *   All zero with the switch off; an open BGZF piece is finished first.
 * No host synchronisation is added per chunk; mlst_get_kernel_time 23 is k_rf_filter alone. */
#define MLST_RF_NO_LIMIT 0xFFFFFFFFu
typedef struct { uint32_t poly_mask, poly_min, min_length, max_n, complexity_pct, mean_qual; } mlst_read_filter;
int mlst_set_read_filter(mlst_handle* h, const mlst_read_filter* f);
int mlst_get_read_filter(mlst_handle* h, mlst_read_filter* out);
int mlst_read_filter_info(mlst_handle* h, uint64_t out[16]);

/* ---- sliding-window quality cuts (off by default; csrc/read_window.h; `cli type --cut-front W,Q / --cut-right W,Q / --cut-tail W,Q`) ----
 * mlst_set_read_window(h, &w): mlst_set_read_prep's trim_qual is a running sum from the 3' end: it tolerates a dip in the middle of a
 *   read that a window mean catches, and it never touches the 5' end.  The three operations here are the quality step of the usual
 *   preprocessing recipes (fastp --cut_front / --cut_right / --cut_tail; Trimmomatic LEADING:Q = front 1,Q, TRAILING:Q = tail 1,Q,
 *   SLIDINGWINDOW:W:Q = right W,Q; MINLEN is mlst_set_read_filter's min_length).  They are done on the device before the reads are
 *   packed, and the engine then behaves as if it had been given the cut text (metamlst_amd.fastq.window_cut / cut_windows state the rule
 *   in Python and write that text).  NULL or a struct with every w = 0 switches the stage off: nothing is queued, nothing is allocated,
 *   and the kernels that run are those that ran before the switch existed.  An operation with w = 0 is off (its q is not looked at and is
 *   kept as 0).  MLST_E_INVALID, with a sentence that names the field and its range, for a w outside 0..320 and for a q outside 1..93
 *   where w != 0.  The rule is modelled on fastp's three operations; it is the project's own and claims neither fastp's nor
 *   Trimmomatic's bytes.
 * The rule, per read (integers only).  q[0..n) are the Phred values as steps 1-3 of mlst_set_read_prep leave them:
 *   clamp(character - phred base, 0, 127).  Each operation X has its window W_X and its threshold Q_X; pass(a, w) is
 *   sum(q[a .. a + w)) >= Q * w.  In this order:
 *   1. front.  If n > 0: w = min(W, n); f = the smallest s in [0, n - w] with pass(s, w); none: f = n, the read is left without a base.
 *      Off: f = 0.
 *   2. right, on [f, n).  If n - f > 0: w = min(W, n - f); s* = the smallest s in [f, n - w] with !pass(s, w); none: e = n; otherwise
 *      e = s* + k, k = the number of leading values of that window that are >= Q (the good bases at the front of the first bad window
 *      stay; k < w always).  Off: e = n.
 *   3. tail, on [f, e).  If e - f > 0: w = min(W, e - f); t = the largest t in [f + w, e] with pass(t - w, w); none: t = f.  e = t.
 *   4. Bases and qualities [f, e) remain.  A read left without a base stays a read of length 0 (mlst_set_read_prep's rule 4); indices,
 *      pairing and names are the file's.  Each mate of a pair is cut on its own.
 *   5. It runs directly behind mlst_set_read_prep's steps and in front of mlst_set_read_adapters' cut (quality before adapters: cutadapt's
 *      and fastp's order); the prepared tables of mlst_set_read_stats are counted behind it (also when it is the only step that ran).
 *   Not done: Trimmomatic's per-base MAXINFO, fastp's skipping of N bases behind a front cut.
 * One combination is refused, in either order, with MLST_E_INVALID and its reason: front_w != 0 together with
 *   mlst_set_read_pair_overlap.  The overlap places the insert's end by trim5 alone (I = o + n2 + trim5: both mates lost the same
 *   number of 5' bases), and a front cut per read would make it cut true insert bases.  right and tail combine with it freely.
 * Entries it applies to, what is refused while it is on ("<entry>: the quality windows are on (mlst_set_read_window) ..."), when the
 *   setting may change and what mlst_reset_sample does: exactly as for mlst_set_read_filter.
 * mlst_get_read_window: the setting (every field 0 with the switch off).
 * mlst_read_window_info: out[0] = reads whose length changed, out[1] = reads cut by front, out[2] = the bases it removed (all n of a
 *   read it emptied), out[3] / out[4] = the same for right, out[5] / out[6] for tail, out[7] = reads of length >= 1 left without a base.
 *   All zero with the switch off; an open BGZF piece is finished first.
 * No host synchronisation is added per chunk; mlst_get_kernel_time 24 is k_rw_cut alone. */
typedef struct { uint32_t front_w, front_q, right_w, right_q, tail_w, tail_q; } mlst_read_window;   /* w = 0: that operation is off */
int mlst_set_read_window(mlst_handle* h, const mlst_read_window* w);   /* NULL or all-zero = off */
int mlst_get_read_window(mlst_handle* h, mlst_read_window* out);
int mlst_read_window_info(mlst_handle* h, uint64_t out[8]);

/* ---- bowtie2's MD:Z field in the text export (off by default; csrc/aln_text.h; `cli type --md`) --------------------------------------
 * mlst_set_export_md(h, 1): every record of mlst_alignments_text_* carries MD:Z:<text> between NM:i and YT:Z:UU, bowtie2's place;
 *   columns 1-11 and every other field are the bytes they are without it.  With the switch off the export writes what it wrote
 *   before the switch existed, with the kernels it ran then, and allocates nothing more.
 * The rule (metamlst_amd.samout.md_text states it in Python): the CIGAR is walked in reference orientation with a match run u = 0.
 *   An M column matches iff the SEQ letter is the upper-cased allele's and is not N -- the predicate of NM; a match: u += 1; otherwise
 *   u in decimal, the allele's letter, u = 0.  A D run: u (also 0), '^', the run's allele letters, u = 0.  I and S runs do not break
 *   the run.  At the end: u (also 0).  The text matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.  An allele byte outside A-Z after
 *   upper-casing is written as N.  SEQ + CIGAR + MD give the allele's bases under the record back.
 * The switch is read by mlst_alignments_text_open and holds for that export; changing it while an export is open: MLST_E_INVALID.  It
 *   is no part of the sample's state (statistics, pile-up, typing and mlst_reset_sample neither see nor change it) and may change at
 *   any other time.  Memory: two bytes per (item, allele) pair of the largest round while an export with it is open.
 * The line bound with the switch on: 3 n + 2 x 15 + 11 bytes more for a read of n bases -- 6 for TAB MD:Z:, 5 for the last run's
 *   digits, 2 per M column (a mismatch's letter and the digits of the run in front of it, which are no more than 1 + the run), 2 per D
 *   run and 1 per D column, with M + I <= n, fewer than 0.4 M gap runs (mlst_create admits 5 match_bonus <= 2 (gap_open + gap_ext)
 *   only, and a record's score is positive) and D <= I + 2 x 15 (the band: band_w <= 15): (alleles of the locus) x (13 n + the longest
 *   label + 233) per item.  MLST_E_LIMIT of mlst_alignments_text_open names the bytes needed under this bound. */
int mlst_set_export_md(mlst_handle* h, int on);
int mlst_get_export_md(mlst_handle* h, int* on);

/* ---- ready-made alignments straight from a BGZF BAM (the reference's one input, metamlst.py:34) ------------------------------
 * The file is streamed twice, as the reference reads it twice (samtools view, then pysam): pass 1 is the hit accumulation of
 * metamlst.py:101-130 (what mlst_submit_* do for reads), pass 2 the pile-up of the chosen contigs (mlst_pileup_alignments).  The
 * blocks are inflated on the GPU and the records are split, read and counted there, in place: device memory is the text of two
 * pieces plus the sequenceBank list, whatever the file's size.
 * mlst_bam_open: the BAM header is the caller's (metamlst_amd/samin.py reads it on the host, and checks the blocks it inflates
 *   itself -- they never reach mlst_set_bgzf_verify's kernel); it yields, per reference sequence,
 *   ref_allele (index into the loaded alleles or -1), ref_locus (locus index or -1), ref_flags (bit 0: the species passes
 *   --filter, bit 1: the name does not split in three at '_'), and skip_bytes: the inflated bytes of the first block submitted
 *   that still belong to the header.  pass = 1 accumulates into the sample's statistics (mlst_get_allele_stats, mlst_typing_*
 *   and mlst_reset_sample work as after reads); pass = 2 piles the records of the chosen alleles up (chosen_allele_idx,
 *   n_chosen; pass 1 ignores them).
 * mlst_submit_bam_bgzf: compressed bytes as for mlst_submit_fastq_bgzf (whole blocks, cut anywhere between them; with
 *   n_consumed_out a non-final buffer may end inside a block); records may straddle blocks and calls.  The 12th and the 15th
 *   column are the 1st and the 4th optional field BY POSITION (Q1); len(SEQ) of a record without SEQ is 1; sequenceBank holds one
 *   length per (locus, QNAME), the last record's -- a QNAME is identified by a 128-bit hash of its bytes (MLST_BAM_QNAME_KEY,
 *   mlst_policy.h).  The order of the records does not matter.  A call's piece is finished by the next call on the handle (as
 *   for mlst_submit_fastq_bgzf; MLST_BGZF_PIPE=0: by the call itself): n_records_out counts the records completed by the call, a
 *   corrupt block (or, with mlst_set_bgzf_verify, a CRC mismatch: same message, nothing of the piece is counted) is reported
 *   by the call that finishes its piece.  The last call passes final_chunk != 0; the file must end with a whole record.
 *   A record larger than the 1 MiB head room of a piece: MLST_E_LIMIT.  A record the device cannot treat the way the reference
 *   would -- no reference sequence, a contig name that does not split in three, fewer than four optional fields, a non-integer
 *   1st / 4th field (integer types c C s S i I), an unknown field type, a non-integer AS / XM (pass 2) -- ends the stream with
 *   MLST_E_INVALID "host path needed: <reason> at record <n>": the caller runs the host reader, which raises or answers as the
 *   reference would.  After any error the stream is closed and the sample's state is undefined (mlst_reset_sample).
 *   While a BAM stream is open the mlst_submit_* entries for reads refuse to start, and mlst_bam_open refuses while a FASTQ
 *   stream is open.
 * mlst_bam_set_capacity: most accepted records on known loci a pass-1 stream may list for sequenceBank (32 bytes each, allocated
 *   as the file needs them; 0 = default 2^26); MLST_E_CAPACITY beyond it.
 * mlst_bam_pileup_fetch: the counts of the finished pass-2 stream, BAM or SAM (mlst_sam_open below), layout of mlst_pileup (alleles in
 *   the order given). */
int mlst_bam_open(mlst_handle* h, int pass, const int32_t* ref_allele, const int32_t* ref_locus, const uint8_t* ref_flags, uint32_t n_ref,
                  uint32_t skip_bytes, const uint32_t* chosen_allele_idx, uint32_t n_chosen);
int mlst_submit_bam_bgzf(mlst_handle* h, const uint8_t* data, uint64_t n_bytes, int final_chunk, uint64_t* n_records_out, uint64_t* n_consumed_out);
int mlst_bam_set_capacity(mlst_handle* h, uint64_t max_entries);
int mlst_bam_pileup_fetch(mlst_handle* h, uint32_t* counts);

/* ---- ready-made alignments straight from SAM text (what the documented bowtie2 command writes with -S) -------------------------------
 * The text is streamed twice like a BAM (pass 1: metamlst.py:101-130, pass 2: the pile-up of the chosen contigs), and parsed on the
 * GPU (csrc/sam_dev.h): line starts from the newline table of the FASTQ parser, then one thread per line.  Device memory is the text
 * of one chunk plus the sequenceBank list, whatever the file's size.  The rules are samin.AlignmentSample's (its _iter_sam_lines, add
 * and pileup), and a line the device cannot treat exactly as that reader would is never guessed (below).
 * mlst_sam_open: names / name_off[n_ref + 1] are the SN: names of the file's @SQ lines, back to back (name i = bytes name_off[i] ..
 *   name_off[i + 1], name_off[0] = 0, under 4 GiB in all); ref_allele / ref_locus / ref_flags per name as for mlst_bam_open.  The
 *   library builds an open-addressing hash table of the names (a power of two of slots, at least 2 * n_ref) and uploads it with the
 *   names: the device hashes a line's RNAME, probes, and takes a hit only when length and bytes agree.  A name that comes twice
 *   keeps its first entry.  pass, chosen_allele_idx, n_chosen as for mlst_bam_open.  Refuses while any other stream is open; while a
 *   SAM stream is open the other submit entries, mlst_bam_open, mlst_bam_reads_open, mlst_bam_set_capacity, mlst_set_bgzf_verify
 *   and mlst_set_read_tiling refuse ("a SAM stream is open ...").
 * mlst_submit_sam_text: the file's bytes from its first byte on (header lines included), cut anywhere; the partial line at a chunk's
 *   end stays on the device and is completed by the next chunk.  The last call passes final_chunk != 0 (its text may be empty, and
 *   its last line need not end with LF).  A call is finished when it returns; n_records_out = record lines completed by it.
 *   - a line ends with LF; a CR directly in front of it is no part of the line.  A line whose first byte is '@' is no record,
 *     wherever it stands.  The record index (locus_first_read, error messages) is the number of record lines in front.
 *   - columns are cut at TAB.  The 12th and the 15th column are taken BY POSITION (Q1); their value is the text between the second
 *     colon and the third colon or the column's end (split(":")[2]).  len(SEQ) is the byte length of column 10: '*' counts 1.
 *     Species filter, accept test, counters, per-allele sums, locus_first and sequenceBank (QNAME key: MLST_BAM_QNAME_KEY) as for
 *     mlst_submit_bam_bgzf; mlst_bam_set_capacity bounds the list of either format.
 *   - pass 2, records on a chosen contig: AS and XM are taken BY NAME among columns 12 and later (a column counts when it holds
 *     two colons and its first part is the tag; the last occurrence wins; an absent tag fails the test); POS - 1 is the leftmost
 *     column; the CIGAR text is walked as mlst_pileup_alignments walks its operations (M = X count, I S advance the read, D N the
 *     reference, H P nothing, '*' no operation); the base is the SEQ byte & 0xDF, Phred the QUAL byte - 33, QUAL '*' Phred 0.
 *   - a line longer than MLST_BAM_MAX_RECORD bytes (its LF not counted): MLST_E_LIMIT "a SAM line of more than ... bytes".
 *   - NEVER GUESSED.  Each of these ends the stream with MLST_E_INVALID "host path needed: <reason> at record <n>", the smallest
 *     record index first; the caller runs the host reader, which raises or answers as the reference does:
 *       a CR that does not stand directly in front of an LF, in any line (Python ends a line there);
 *       a byte >= 0x80 or a NUL in a record line;  fewer than 15 columns (an empty line is such a line);
 *       FLAG, POS, the 12th or the 15th column's value not of the form -?[0-9]{1,9} (int() also takes "+5", " 5", "5_0");
 *       an RNAME that is not among the names (or '*'), or one that does not split in three at '_' (ref_flags bit 1);
 *       on a loaded contig (ref_allele >= 0), in either pass: an AS or XM column found by name whose value is no such integer, a
 *       CIGAR byte that is neither a digit nor one of MIDNSHP=X, an operation length >= 2^28 (the host reader parses all three
 *       for every record it keeps);
 *       pass 2, on a loaded contig: QUAL neither '*' nor as long as SEQ; on a chosen contig: a QUAL byte below 33.
 *   After any error the stream is closed and the sample's state is undefined (mlst_reset_sample). */
int mlst_sam_open(mlst_handle* h, int pass, const uint8_t* names, const uint64_t* name_off /* n_ref + 1 */,
                  const int32_t* ref_allele, const int32_t* ref_locus, const uint8_t* ref_flags, uint32_t n_ref,
                  const uint32_t* chosen_allele_idx, uint32_t n_chosen);
int mlst_submit_sam_text(mlst_handle* h, const uint8_t* text, uint64_t n_bytes, int final_chunk, uint64_t* n_records_out);

/* ---- the READS of a BGZF BAM (unaligned BAMs, the unmapped remainder of a host depletion, a BAM aligned to something else) -----
 * The records are taken as reads the way `samtools fastq` takes them with its defaults, chosen, strand-corrected and packed on the
 * GPU (csrc/bam_reads.h) and typed like the reads of a FASTQ file; their alignments are ignored.  Replaces the `samtools fastq`
 * run in front of the user-run bowtie2 [NOT IN TREE].  Records count in file order:
 *   - FLAG 0x100 (secondary) or 0x800 (supplementary): not a read; skipped and counted.
 *   - l_seq == 0: skipped and counted.  (A deviation: samtools writes an empty record; the FASTQ parser has no statement on
 *     empty reads.)  A record that is both counts as secondary / supplementary.
 *   - FLAG 0x10: the record is stored on the reference strand; the read is its reverse complement, its Phred values reversed.
 *   - base nibbles 1 2 4 8 are A C G T; every other nibble (N, IUPAC, =) is a non-ACGT base: packed as A, bit 7 in its qrows
 *     byte, bit 15 of lens -- what an N of FASTQ text gets.  The filler nibble of an odd l_seq is no base.  The complement swaps
 *     1 <-> 8 and 2 <-> 4; anything else stays non-ACGT.
 *   - Phred: the raw byte clamped to 0..127 (what the text path makes of chr(q + 33)).  A first quality byte of 0xFF means no
 *     qualities: every base gets Phred 1 (the default of samtools fastq -v).
 *   - l_seq > 320 (MLST_MAX_READ_LEN): MLST_E_LIMIT "a BAM read is longer than 320 bases"; the stream ends.  Not so on an unpaired
 *     stream opened behind mlst_set_read_tiling: there a read longer than the tile is cut into windows (LONG READS above), and
 *     mlst_bam_reads_info[0] counts windows plus uncut reads.  A paired stream is never tiled.
 *   - the read index is the number of reads kept before it: locus_first_read and mlst_set_read_index_base as after FASTQ.
 *   - ref_id, pos, CIGAR and the optional fields are stepped over.
 * mlst_bam_reads_open: n_ref = the header's reference count (0 for an unaligned BAM; it bounds the ref_id of a plausible record
 *   head, nothing else), skip_bytes as for mlst_bam_open.  Refuses while another stream is open; while it is open the other
 *   entries refuse as for mlst_bam_open.  The data follows through mlst_submit_bam_bgzf, unchanged in form (whole blocks,
 *   n_consumed_out, final_chunk, n_records_out = records completed by the call, CRC verification, MLST_BGZF_PIPE=0): a call copies
 *   and inflates its piece; the piece is split, its reads chosen, packed and submitted to pass 1 when it is finished -- by the next
 *   call on the handle or by any entry that looks at the sample's state (one host synchronisation per piece: the pack buffers are
 *   sized by its read count and longest read).
 *   paired != 0: the reads kept must come as neighbours -- kept reads 2k and 2k + 1 carry byte-identical QNAMEs and FLAG 0x1 both
 *   -- and are submitted as pairs (one QNAME per pair for sequenceBank, metamlst.py:127, Q3, as mlst_submit_fastq_pair); skipped
 *   records may stand between and behind them.  A kept read whose neighbour has another name, one without 0x1, or an odd number of
 *   kept reads at the end of the file: MLST_E_INVALID "record <n> has no mate next to it (a paired BAM must be collated by name)"
 *   (n counts all records of the file from 0).  Every submission holds whole pairs: a piece that ends on an odd number of kept
 *   reads hands its last kept record (and what follows it) on to the next piece; if that does not fit the 1 MiB head room:
 *   MLST_E_LIMIT, as for an oversized record.
 * mlst_bam_reads_info: of the reads stream just finished or still open (a piece in flight is finished first): [0] reads
 *   submitted, [1] records skipped as secondary / supplementary, [2] records skipped as empty, [3] cells the record split walked
 *   again (mlst_debug_bam_split). */
int mlst_bam_reads_open(mlst_handle* h, uint32_t n_ref, uint32_t skip_bytes, int paired);
int mlst_bam_reads_info(mlst_handle* h, uint64_t out[4]);

/* ---- CONTIGS (an assembled genome, the modality of the reference's mlst.py) tiled into reads on the GPU -----------------------------
 * `text` is uncompressed FASTA in host memory that holds whole contigs (a call's text is cut in front of a '>' that starts a line, as
 * mlst_submit_fastq wants whole records).  The bytes cross the link once; the contigs are cut into overlapping windows, packed on the
 * device (csrc/fasta_dev.h) and typed like unpaired reads of a FASTQ file.  Replaces the FASTQ text metamlst_amd.fastq.tile_fasta
 * writes on the host, whose rules these are:
 *   - a line whose first byte is '>' opens a contig; everything else on that line is ignored.  A '>' anywhere else is a base.
 *   - lines in front of the first header of a call are ignored.
 *   - a contig's sequence is the bytes of its lines with the line ends (LF or CRLF) removed; empty lines add nothing; the last line
 *     need not end with LF.
 *   - a contig of n bases: n < min_len: no read.  n <= read_len: one read of n bases.  Otherwise windows of read_len bases at starts
 *     0, stride, 2 * stride, ... <= n - read_len, plus one flush with the contig's end when (n - read_len) % stride != 0.
 *   - read order is contig order, then start order; read indices continue the handle's count across calls (locus_first_read and
 *     mlst_set_read_index_base as after FASTQ).
 *   - letters in either case are themselves; every other byte (N, IUPAC, '>', bytes >= 0x80, NUL) is a non-ACGT base: packed as A,
 *     bit 7 in its qrows byte, bit 15 of lens -- what an N of FASTQ text gets.
 *   - every base has Phred 40; qrows bytes past a read's end are 0.  words_per_read / qual_stride are those of the FASTQ path for
 *     the longest read of the call.
 * Refused: read_len, stride or min_len of 0 (MLST_E_INVALID); read_len > 320 (MLST_MAX_READ_LEN: MLST_E_LIMIT); a call while a FASTQ
 * or BAM stream is open on the handle.  A sequence line of a contig that holds 0x09, 0x0B, 0x0C, 0x20 or a CR that is not directly
 * in front of an LF -- where Python's strip() and a device rule could part ways -- submits nothing of the call and fails with
 * MLST_E_INVALID "host path needed: <reason> at byte <n>" (n counts the call's text from 0): the caller tiles the file on the host.
 * A call that yields no read returns 0 and submits nothing.  n_contigs_out / n_reads_out (optional): header lines / reads of the
 * call.  One host synchronisation per call (the counts size the pack buffers).  Compressed FASTA is inflated by the caller. */
int mlst_submit_fasta(mlst_handle* h, const uint8_t* text, uint64_t n_bytes, uint32_t read_len, uint32_t stride, uint32_t min_len,
                      uint64_t* n_contigs_out, uint64_t* n_reads_out);

/* ---- whole typing tail on the device, without a host round trip between the passes ----------------------
 * mlst_typing_enqueue queues, behind the pass-1 work already submitted on the engine's stream:
 *   the allele choice of metamlst.py:133-151 + :244 (per locus the allele with the highest
 *   round((sum AS - (maxHits - hits) * penalty) / hits, 1), ties to the lowest allele number, computed exactly
 *   as Python's round() does -- see mlst_round_tenths), pass 2 against the chosen alleles, the majority
 *   consensus of mlst_consensus, and the copies to the host.  It returns at once.
 * mlst_typing_fetch waits for it and returns the statistics of mlst_get_allele_stats, chosen[n_loci] (allele
 *   index, -1 = locus without an accepted record) and the consensus letters; the letters of locus l start at
 *   colbase[l] of mlst_typing_layout (one slot of the locus' longest allele per locus; only the first
 *   len(chosen allele) bytes of a slot are meaningful).
 * The choice is part of the host logic of the reference (float round + tie-break); the Python host keeps its
 * own statement of it (typing.pick_alleles_fast) and the tests compare the two. */
int mlst_typing_layout(mlst_handle* h, uint64_t* colbase /* n_loci + 1 */, uint64_t* total_cols);
int mlst_typing_enqueue(mlst_handle* h, int32_t penalty, uint32_t mincov, char none_char);
/* The two halves of mlst_typing_enqueue, for a multi-GPU caller that all-reduces the pileup counts in between:
 * choice + pileup into d_counts (device, total_cols * 4 uint32, zeroed by the call; NULL = internal buffer), then
 * consensus over d_counts + the copies to the host. */
int mlst_typing_choose_pileup(mlst_handle* h, int32_t penalty, uint32_t* d_counts);
int mlst_typing_finish(mlst_handle* h, uint32_t mincov, char none_char, const uint32_t* d_counts);
/* The same halves with the counts in a COMPACT layout, for the all-reduce in between: only the loci with a chosen
 * allele get a slot (of the locus' longest allele), in locus order -- every rank holds the same statistics after the
 * first exchange, chooses the same alleles and so derives the same layout.  d_counts: device, cap_cols * 4 uint32,
 * zeroed by the call.  The capacity is fixed by the caller before the need is known (the size of a collective is a
 * host decision): mlst_typing_compact_info, after mlst_typing_fetch, returns the columns needed and whether they
 * fitted.  If they did not, nothing was piled up, no letter of that fetch is valid, and the caller repeats both halves
 * with at least need_cols columns (mlst_typing_layout's total always suffices); statistics and choice are unaffected.
 * mlst_typing_fetch returns the letters in the fixed layout of mlst_typing_layout either way.  (No reference
 * counterpart: the reference is one process; what is exchanged are the counts behind cmseq's consensus,
 * metaMLST_functions.py:255-259.) */
int mlst_typing_choose_pileup_compact(mlst_handle* h, int32_t penalty, uint32_t* d_counts, uint64_t cap_cols);
int mlst_typing_finish_compact(mlst_handle* h, uint32_t mincov, char none_char, const uint32_t* d_counts);
int mlst_typing_compact_info(mlst_handle* h, uint64_t* need_cols, uint32_t* overflow);
int mlst_typing_fetch(mlst_handle* h, int64_t* sum_score, uint32_t* n_hits, uint64_t* locus_read_len_sum,
                      uint64_t* locus_first_read, uint64_t* counters, int32_t* chosen, uint8_t* letters);
/* mlst_typing_fetch in two halves: mlst_typing_wait waits for the queued typing step; its results stay in pinned memory (two
 * slots, written in turn) while the caller queues the engine's next step; mlst_typing_fetch_waited copies them out without
 * waiting.  (An engine on its own share of the CUs idles between the end of a step and the submission of the next.) */
int mlst_typing_wait(mlst_handle* h);
int mlst_typing_fetch_waited(mlst_handle* h, int64_t* sum_score, uint32_t* n_hits, uint64_t* locus_read_len_sum,
                             uint64_t* locus_first_read, uint64_t* counters, int32_t* chosen, uint8_t* letters);
/* round(float(p) / float(q), 1) of Python as an exact integer number of tenths (host function, the same code
 * the device uses); 0 when q == 0. */
long long mlst_round_tenths(long long p, uint32_t q);

/* Allele match: Hamming distance of `query` against every allele of `locus`, semantics of
 * stringDiff (metaMLST_functions.py:230-234: zip truncates, length difference not counted),
 * as used by metamlst-merge.py:177-181.  Outputs the first allele (load order) within z,
 * or -1, and the number of alleles within z. */
int mlst_hamming_le(mlst_handle* h, uint32_t locus, const uint8_t* query, uint32_t len,
                    uint32_t z, int32_t* first_allele_idx, uint32_t* n_within);
/* Full distance vector (dist[n_alleles_of_locus]) for tests and reports. */
int mlst_hamming_all(mlst_handle* h, uint32_t locus, const uint8_t* query, uint32_t len,
                     uint32_t* dist);

/* ---- centre-star alignment of the alleles of one locus (merge --outseqformat A / A+) ---------------------------------------------------
 * Replaces the MUSCLE run of metamlst-merge.py:402-405 [MUSCLE NOT IN TREE], which the reference needs when the sequences of a locus
 * differ in length.  The output is NOT MUSCLE's: the rule below is this engine's own (MLST_MSA_* of mlst_policy.h), stated in Python by
 * metamlst_amd/msa.py (center_star), and the device reproduces that statement byte for byte (csrc/msa_dev.h).
 * mlst_msa_align: seqs / off[n + 1] are the n sequences back to back (sequence r = bytes off[r] .. off[r + 1]).
 *   - the centre is the first sequence, in input order, of the most frequent length (the greatest such length on a tie).
 *   - every other sequence b (rows i = 1..len(b)) is aligned to the centre a (columns j = 1..m): global, affine, unbanded, int32.
 *     s(x, y) = MLST_MSA_MATCH when x & 0xDF == y & 0xDF and that letter is one of A C G T, MLST_MSA_MISMATCH otherwise (an N matches
 *     nothing, itself included; lower case matches its upper case).  A gap of g bases costs GO + g * GE (10 + g), end gaps included.
 *     States M (b_i on a_j), I (b_i opposite a gap), D (a_j opposite a gap):
 *       M[0][0] = 0, I[i][0] = -(GO + GE i), D[0][j] = -(GO + GE j), everything else on the border NEG
 *       M[i][j] = s + max(M, I, D)[i-1][j-1]
 *       I[i][j] = max(M[i-1][j] - GO - GE, I[i-1][j] - GE, D[i-1][j] - GO - GE)
 *       D[i][j] = max(M[i][j-1] - GO - GE, D[i][j-1] - GE, I[i][j-1] - GO - GE)
 *     in every max the first listed candidate wins ties; the end state is the first of M, I, D at the maximum of [len(b)][m]; the
 *     traceback follows the recorded choices.
 *   - slot k (k = 0..m) lies between centre columns k and k + 1 and is as wide as the longest insertion any row makes there.  A row
 *     is, for k = 0..m: its insertion in slot k, left-justified and padded with '-', then (k < m) its base on column k + 1, or '-'.
 *     The centre's slots are all '-'; letters keep their case; every row is width = m + sum of the slot widths bytes long; a row
 *     without its '-' is its sequence.  Insertions of different rows that share a slot are stacked, not aligned to each other.
 *   center_out / width_out (optional): index of the centre, bytes per row.  No reference needs to be loaded; nothing of the sample's
 *   state is read or changed, and mlst_reset_sample leaves a finished alignment alone.  The pairs are aligned in batches whose
 *   traceback store (about len x m bytes a pair) fits MLST_MSA_BATCH_BYTES (environment, read by mlst_create; default 1 GiB, floor
 *   one pair); one host synchronisation per call (the width sizes the rows).
 *   Refused: n = 0, an empty sequence, a byte that is not an ASCII letter ('-', white space and digits included): MLST_E_INVALID;
 *   a sequence longer than MLST_MAX_ALLELE_LEN (4095) bases, n x width >= 2^32: MLST_E_LIMIT; a call while a FASTQ, BAM or SAM
 *   stream is open on the handle: MLST_E_INVALID.  A refused call leaves no finished alignment; the handle stays usable.
 * mlst_msa_fetch: the n x width bytes of the alignment just finished, row after row (rows: host memory).  Without a finished
 *   mlst_msa_align: MLST_E_INVALID. */
int mlst_msa_align(mlst_handle* h, const uint8_t* seqs, const uint64_t* off /* n + 1 */, uint32_t n, uint32_t* center_out, uint32_t* width_out);
int mlst_msa_fetch(mlst_handle* h, uint8_t* rows /* n * width */);

/* Multi-GPU: index of this rank's first read in the whole sample, so that locus_first_read (the
 * first-seen order of metamlst.py's dicts, Q6) is global.  Call after mlst_reset_sample / before submitting. */
int mlst_set_read_index_base(mlst_handle* h, uint64_t base);

/* Forget reads and statistics, keep the reference (next sample). */
int mlst_reset_sample(mlst_handle* h);

/* ---- introspection (tests, bench) ---- */
typedef struct mlst_item {     /* one (read, locus, strand, diagonal) unit of extension work */
    uint64_t read_index;       /* index of the read in submission order */
    uint32_t locus;
    int32_t  diag;             /* allele position minus (oriented) read position */
    uint16_t strand;           /* 1 = read reverse-complemented */
    uint16_t votes;
    uint32_t reserved;
} mlst_item;
int mlst_get_items(mlst_handle* h, mlst_item* out, uint64_t cap, uint64_t* n);

/* Run the engine on the caller's HIP stream (hipStream_t; NULL = back on the engine's own stream).  Work queued so
 * far is waited for.  With the engine on the stream a torch.distributed collective is ordered against, a multi-GPU
 * step needs no host synchronisation between its kernels and its collectives (metamlst_amd/dist.py). */
int mlst_set_stream(mlst_handle* h, void* stream);
/* The engine's own stream restricted to share `part` of `n_parts` equal shares of the device's CUs (hipExtStreamCreateWithCUMask;
 * n_parts = 1: the whole device).  Engines of one process on disjoint shares run side by side instead of taking turns;
 * mlst_get_stream hands the stream out (e.g. for torch.cuda.ExternalStream), mlst_busy asks without waiting whether work
 * queued on the engine's current stream is still running (1) or not (0).  No reference counterpart (one process, one CPU). */
int mlst_set_cu_partition(mlst_handle* h, uint32_t part, uint32_t n_parts);
int mlst_get_stream(mlst_handle* h, void** stream);
int mlst_busy(mlst_handle* h);
/* mlst_export_stats_device / mlst_import_stats_device without the host synchronisation. */
int mlst_export_stats_device_async(mlst_handle* h, int64_t* d_sum, int64_t* d_min);
int mlst_import_stats_device_async(mlst_handle* h, const int64_t* d_sum, const int64_t* d_min);

int mlst_set_profiling(mlst_handle* h, int on);   /* 0 = off, 1 = events + sieve window, 2 = sieve window only (keeps the hipGraph replay of the launch sequences, which event profiling turns off) */
/* Per-kernel device time measured with HIP events on the engine's stream.
 * which: 0=sieve (all its kernels) 1=seed 2=extend (k_extend + k_extend_pairs) 3=banded-SW 4=accumulate 5=pileup 6=pack 12=k_ext_prep (the item records of k_extend);
 * 13 = k_fqt_count (a BAM piece: k_bamt_count) + k_fqt_scan + k_fqt_add and 14 = k_fqt_emit (k_bamt_emit) (long reads cut into windows,
 * csrc/fastq_tile.h, csrc/bam_tile.h; outside 6); 15 = the line table of a SAM chunk (k_fq_count, k_fq_scan, k_fq_lines, k_sam_flags), 16 =
 * k_sam_accumulate and 17 = k_sam_pileup (csrc/sam_dev.h; two entries of 15 per chunk); 18 = k_rp_qtrim (csrc/read_prep.h) and 19 = k_ra_cut
 * (csrc/read_adapt.h), each alone (inside 6); 20 = k_rs_count (csrc/read_stats.h; alone, inside 6); 21 = k_dd_insert + k_dd_sign + k_dd_mark
 * (csrc/read_dedup.h; the three launches of a chunk together, inside 6); 22 = k_po_cut (csrc/read_overlap.h; alone, inside 6); 23 = k_rf_filter
 * (csrc/read_filter.h; alone, inside 6); 24 = k_rw_cut (csrc/read_window.h; alone, inside 6); 9 = k_route, 10 =
 * k_route_probe and 11 = k_route_verify, the three kernels of the routed sieve (inside 0) (events bracket the launch on the engine's
 * stream, so with several engines on one GPU they include the time a kernel queues behind another stream's kernel);
 * 7 = the sieve's execution window measured inside the kernel (wall clock at the first workgroup's start and the last
 * one's end; one submission per sample), added up when the sample's statistics are fetched;
 * 8 = the longest residency of one workgroup of that launch (LDS sieve; one workgroup per CU, each doing an equal share):
 * what the launch takes once its workgroups run -- when it shares the GPU with another stream's kernel its workgroups
 * start one by one as CUs free up, which stretches the window (7) without the kernel being any slower. */
int mlst_get_kernel_time(mlst_handle* h, int which, double* total_ms, uint64_t* launches);
int mlst_reset_kernel_time(mlst_handle* h);
/* Bytes of the device-resident index structures: [0]=allele arena [1]=sieve [2]=seed table;
 * [3]=fill of the LDS first-level bitmap in parts per million (0 when the plain sieve kernel is in use) */
int mlst_get_index_bytes(mlst_handle* h, uint64_t out[4]);
/* The seed sieve chosen for the loaded database: [0] = kind (0 = half-seed bitmaps in LDS, 1 = hashed bitmap in global
 * memory, 3 = CU-routed filter slices in LDS; chosen by database size, MLST_SIEVE=lds / global / routed forces one), [1] = distinct canonical seeds, [2] = longest overflow walk of a key in the
 * fingerprint sieve (the kernels follow a chain for 64 buckets; the build keeps it <= 32), [3] = sieve buckets. */
int mlst_get_sieve_info(mlst_handle* h, uint64_t out[4]);
/* The block-haplotype tables k_extend scores against (SURVEY 8 f1 "locus backbone / variant-column table"; they replace
 * aligning a read against every allele one by one, which is what a bowtie2 -a run over the FASTA of
 * metaMLST_functions.py:149-161 does): [0] = distinct 32-base block haplotypes of all loci, [1] = bytes of the tables
 * (also counted in mlst_get_index_bytes [0]), [2] = loci that have them, [3] / [4] = most haplotypes in any run of 6 / 11
 * blocks (what a read of <= 160 / <= 320 bases covers), [5] / [6] = bytes of LDS a work item of k_extend_160 / _320 gets
 * for the summaries (MLST_EXT_LDS_KB bounds it; loci that need more are aligned pair by pair), [7] = threads per work item. */
int mlst_get_extend_info(mlst_handle* h, uint64_t out[8]);
/* Block until all work queued on the engine's stream is done. */
int mlst_synchronize(mlst_handle* h);

#ifdef __cplusplus
}
#endif
#endif
