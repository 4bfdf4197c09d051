/*
 * mlst_debug.h -- diagnostics and test hooks of libmlst_hip.so.
 *
 * NOT part of the drop-in boundary (include/mlst.h): nothing here has a counterpart in the reference, no data path calls
 * these, and a binding of the product needs none of them.  They are exported by the same library because the tests
 * (tests/test_inflate.py) and the profiling scripts (profiles/route_modes.py, profiles/inflate_rate.py) drive the device
 * code through them.
 */
#ifndef MLST_DEBUG_H
#define MLST_DEBUG_H

#include "mlst.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: the deflate decoder of the call above run on the HOST on one raw deflate stream (returns 0 or a negative
 * code of csrc/inflate_dev.h; *produced = bytes written).  Not a data path. */
int mlst_selftest_inflate(const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t cap, uint64_t* produced);

/* Test hook of the DEVICE decoder (csrc/inflate_wave.h): whole BGZF blocks in, their inflated text out (host buffers);
 * kernel_ms (optional) receives the duration of the inflate kernels alone (HIP events) -- with mlst_set_bgzf_verify on, which this
 * hook obeys too (a mismatch fails it with the block's number), of the inflate kernels and the CRC kernel behind them. */
int mlst_selftest_inflate_device(mlst_handle* h, const uint8_t* data, uint64_t n_bytes, uint8_t* out, uint64_t cap, uint64_t* produced, double* kernel_ms);

/* Which kernel inflated the blocks of the LAST mlst_selftest_inflate_device call (tests/test_inflate_streams.py; no data path reads
 * or writes what this returns).  *n_blocks: the BGZF blocks with data of that call; *left_to_wave: how many of them phase 1 of the
 * two-kernel inflate (k_inflate_tok / k_inflate_tok2) left to k_inflate -- the TOK_OVERFLOW entries of its token-count array;
 * 0 with MLST_INFLATE_MODE=1, where there is no phase 1.  MLST_E_INVALID before the first such call, after one that ended before
 * its kernels were launched (bad framing, no block with data, an allocation that failed), and after one of more than 16,384
 * blocks (more than one pass may have run: the array then holds the last pass only). */
int mlst_debug_inflate_paths(mlst_handle* h, uint64_t* n_blocks, uint64_t* left_to_wave);

/* Test hook of the CRC stage (csrc/bgzf_crc.h): whole BGZF blocks in; they are inflated as by the call above and the CRC-32 that
 * k_bgzf_crc computes of every block with data comes out, in file order, whatever the trailers say (nothing is compared).
 * cap: room in crc_out (values); *n_blocks: values written; kernel_ms (optional): the CRC kernel alone (HIP events). */
int mlst_selftest_bgzf_crc(mlst_handle* h, const uint8_t* data, uint64_t n_bytes, uint32_t* crc_out, uint64_t cap, uint64_t* n_blocks, double* kernel_ms);

/* The decoder of k_inflate_tok2 (csrc/inflate_canon.h: canonical limits, 800 bytes of state per stream) run on the HOST on one
 * raw deflate stream, its tokens replayed into bytes.  *left_to_other_kernel = 1: the literal / length code of a block holds
 * more symbols than the decoder's 192-entry table (the device leaves such a block to k_inflate); nothing is produced then. */
int mlst_selftest_inflate_canon(const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t cap, uint64_t* produced, int* left_to_other_kernel);

/* The BGZF blocks of a chunk as mlst_submit_fastq_bgzf lists them: the hook runs the product's lister (bgzf_list in
 * csrc/bgzf_host.h, with the four-thread walk; host code only, no device) and reports the blocks with data, the bytes they
 * inflate to, and -- a chunk of 32 MB or more is walked by four threads, three of them from a block start they find behind their
 * quarter mark -- how many of the four lists counted (a list counts only where the chain of the one before it lands on its first
 * block).  MLST_E_INVALID where the lister refuses the chunk: something that is not a whole block, or a block that claims more
 * than 65,536 bytes.  tests/test_inflate.py. */
int mlst_debug_bgzf_walk(const uint8_t* data, uint64_t n_bytes, uint64_t* n_blocks, uint64_t* text_bytes, int* lists_taken);

/* Diagnostics of the routed sieve (profiles/route_modes.py; no reference counterpart, not a data path).
 * mlst_get_route_trace: the first call switches the trace on; later calls wait for the stream and return, for the last
 * submission, out[0] = producer workgroups P, [1] = arena address, [2] = packed-row address, [3] = wall-clock kHz,
 * [4] = region capacity, [5] = filter address, [6] = flag address, [7] = arena capacity in entries, then four words per
 * workgroup (P producers, then the 256 consumers): XCC_ID | HW_ID << 32, wall clock at start, at end, 0.
 * *n_words = words needed (0 while nothing has been traced).
 * mlst_debug_route_realloc: free the routing arena (the next submission allocates it again), keeping pad_bytes of
 * device memory allocated in between so that the new arena lands elsewhere; pad_bytes = UINT64_MAX keeps the old arena itself
 * allocated (until mlst_destroy), so that the new one is different memory for certain. */
int mlst_get_route_trace(mlst_handle* h, uint64_t* out, uint64_t cap_words, uint64_t* n_words);
int mlst_debug_route_realloc(mlst_handle* h, uint64_t pad_bytes);

/* The consumer of the routed sieve (k_route_probe with examiner waves, MLST_PROBE_EXAM_WAVES; tests/test_gpu_probe_examiners.py).
 * Waits for the stream.  *ring_full: blocks of parked entries that found the workgroup's LDS ring full and went to the global
 * list instead, summed over the sample.  *n_cand: the sample's candidates; cand (optional, room for cap values): the candidate
 * list of the LAST submission, in no particular order -- the whole sample's only where the sample was one submission. */
int mlst_debug_route_probe(mlst_handle* h, uint64_t* ring_full, uint32_t* cand, uint64_t cap, uint64_t* n_cand);

/* The record split of BAM input (csrc/bam_dev.h): force_miss_every = n > 0 throws the guessed record start of every n-th cell
 * of the streams that follow away, so that the chain walk has to enter those cells from their true entry (the path a wrong guess
 * takes); 0 = off.  *cells_rewalked_out: cells walked again during the last stream.  Only while no BAM stream is open. */
int mlst_debug_bam_split(mlst_handle* h, uint32_t force_miss_every, uint64_t* cells_rewalked_out);

/* The pack buffers of the LAST submission made from FASTQ text (k_pack_text), from the reads of a BAM (k_bamr_pack,
 * csrc/bam_reads.h) or from contigs tiled on the device (mlst_submit_fasta: k_pack_text over csrc/fasta_dev.h's flat sequence), copied out: `packed` in the resident layout (ceil(n / 64) * 64 * wpr words), `qrows` (n x qstride), `lens`;
 * any of the three may be NULL.  out = { n_reads, words_per_read, qual_stride } (all 0 before the first such submission).  A
 * piece in flight is finished first; MLST_E_CAPACITY when a buffer is too small (out is filled in either way).
 * tests/test_gpu_bam_reads.py and tests/test_gpu_fasta.py compare the rows with mlst_pack_fastq_host's. */
int mlst_debug_last_packed(mlst_handle* h, uint32_t* packed, uint64_t cap_words, uint8_t* qrows, uint64_t cap_q, uint16_t* lens, uint64_t cap_reads,
                           uint64_t out[3] /* n_reads, wpr, qstride */);

/* Which paths the LAST mlst_submit_fasta call that reached the device took (csrc/fasta_dev.h; tests/test_gpu_fasta_edges.py):
 * out = { cells of 4,096 bytes of its text (k_fa_state scans 1,024 of them per turn), contigs it counted (k_fa_scan scans 1,024
 * per turn), entries of the contig tables when the call ended, passes over those tables (2: the tables were too small for the
 * contigs counted, were grown, and the steps behind the cell scan ran again) }.  Host fields the entry keeps anyway: nothing
 * is launched, copied or waited for.  MLST_E_INVALID before the first such call (an empty text or one without a header line
 * does not reach the device). */
int mlst_debug_fasta_info(mlst_handle* h, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
