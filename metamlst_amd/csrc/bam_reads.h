// bam_reads.h -- the READS of a BAM on the device (included by mlst_engine.hip behind bam_dev.h, whose record split it works on).
//
// A reads stream (mlst_bam_reads_open) takes the records of a BGZF BAM as reads, the way `samtools fastq` does with its defaults
// (the rules: include/mlst.h).  k_bam_link leaves, per cell of the piece's text, the starts of the records that begin in it
// (count, base, list).  From there:
//   k_bamr_count : kept records per cell (one thread per record, a workgroup per cell)
//   k_bamr_scan  : one workgroup: the cells' counts become read indices (prefix sum); a paired piece that holds an odd number of
//                  kept records hands its last kept record on to the next piece (BamMeta.carry_start moves back to it)
//   k_bamr_select: per kept record its read index (ballot / prefix inside the cell), the slot offset of the record, its length,
//                  strand and "no qualities" bits and its record index; the longest read, the skipped records by kind, and the
//                  first record that cannot be taken (atomicMin on record index << 4 | reason, as bam_flag does)
//   k_bamr_mates : paired streams: reads 2k and 2k + 1 carry the same QNAME, byte by byte
//   k_bamr_pack  : k_pack_text for nibble input: 4-bit bases -> the resident 2-bit rows, raw Phred -> qrows, lens; its windowed
//                  instantiation packs windows of reads (mlst_set_read_tiling on an unpaired stream: csrc/bam_tile.h)
// The offsets of SEQ and QUAL follow from the record's start and three bytes of its head (l_read_name, n_cigar_op); k_bamr_pack
// derives them once per read into LDS instead of k_bamr_select storing them per record of the piece.
// gfx950 build (hipcc -O3): no kernel of this file uses scratch; the register / LDS figures are in profiles/bam_reads.md
// and, with those of the windowed pack, in profiles/bam_long_reads.md.
// Bytes of the text are loaded one by one and assembled (records have no alignment); no unaligned wide loads.
#ifndef MLST_BAM_READS_H
#define MLST_BAM_READS_H

// reasons a reads stream ends at a record (low 4 bits of BamReadsMeta.err_key)
#define BAMR_ERR_LONG   1u                /* l_seq > MLST_MAX_READ_LEN (tiling off, or a paired stream) */
#define BAMR_ERR_MATE   2u                /* paired: no FLAG bit 0x1, another QNAME than its neighbour's, or no neighbour at the file's end */
#define BAMR_ERR_SPAN   3u                /* tiling on: l_seq > MLST_MAX_READ_LEN and SEQ + QUAL do not fit the record's block_size */
// rd_info of a kept read: l_seq (a record is at most BAM_REC_MAX = 2^20 - 64 bytes: l_seq < 2^20) and two flags
#define BAMR_LEN        0x3FFFFFFFu
#define BAMR_REV        (1u << 30)        /* FLAG 0x10: stored on the reference strand */
#define BAMR_NOQUAL     (1u << 31)        /* first quality byte 0xFF: no qualities */

struct BamReadsMeta {       // device-resident, next to BamMeta, lives as long as the stream
    u64 err_key;            // smallest (record index << 4 | BAMR_ERR_*) (~0: none)
    u64 n_secondary;        // records skipped for FLAG 0x100 / 0x800 (all pieces)
    u64 n_empty;            // records skipped for l_seq == 0 (all pieces)
    u32 n_reads;            // this piece: kept records (even on a paired stream)
    u32 max_len;            // this piece: l_seq of its longest kept read (32 bits hold every l_seq the record split lets through: < 2^20)
};

// 0: a read; 1: secondary / supplementary; 2: no bases
__device__ inline u32 bamr_class(const u8* __restrict__ t, u32 s) {
    if (bam_ld16(t + s + 18) & 0x900u) return 1u;
    return bam_ld32(t + s + 20) ? 0u : 2u;
}

__global__ __launch_bounds__(256) void k_bamr_count(const u8* __restrict__ text, u32 n_cells, const u32* __restrict__ count, const u32* __restrict__ list, u32* __restrict__ kept) {
    for (u32 k = blockIdx.x; k < n_cells; k += gridDim.x) {
        const u32 cnt = count[k]; u32 n = 0;
        for (u32 j0 = 0; j0 < cnt; j0 += 256u) {
            const u32 j = j0 + threadIdx.x;
            n += (u32)__syncthreads_count(j < cnt && bamr_class(text, list[(u64)k * BAM_CELL_CAP + j]) == 0u);
        }
        if (threadIdx.x == 0) kept[k] = n;
    }
}

// One workgroup of 1024 threads.  kbase[k]: read index (inside the piece) of the first kept record of cell k.
__global__ __launch_bounds__(1024) void k_bamr_scan(const u8* __restrict__ text, u32 text_end, u32 n_cells, BamMeta* __restrict__ meta, BamReadsMeta* __restrict__ rm,
                                                    const u32* __restrict__ count, const u32* __restrict__ base, const u32* __restrict__ list,
                                                    const u32* __restrict__ kept, u32* __restrict__ kbase, int paired, int final_piece) {
    __shared__ u32 s_wave[16]; __shared__ u32 s_run, s_last;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { s_run = 0; s_last = 0; }
    __syncthreads();
    u32 last = 0;      // the last cell that holds a kept record, plus one
    for (u32 k0 = 0; k0 < n_cells; k0 += 1024u) {
        const u32 k = k0 + tid; const u32 c = k < n_cells ? kept[k] : 0u;
        if (c) last = k + 1u;
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(incl, o); if (lane >= o) incl += y; }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        u32 before = s_run;
        for (int w = 0; w < wv; w++) before += s_wave[w];
        if (k < n_cells) kbase[k] = before + incl - c;
        __syncthreads();
        if (tid == 1023) s_run = before + incl;
        __syncthreads();
    }
    if (last) atomicMax(&s_last, last);
    __syncthreads();
    u32 total = s_run; const u32 kl = s_last - 1u;
    __syncthreads();
    if (paired && (total & 1u)) {      // (an odd total: some cell holds a kept record, s_last != 0)
        // the last kept record of the piece: the largest j of cell kl that is a read
        if (tid == 0) s_run = 0;
        __syncthreads();
        const u32 cnt = count[kl];
        for (u32 j = tid; j < cnt; j += 1024u) if (bamr_class(text, list[(u64)kl * BAM_CELL_CAP + j]) == 0u) atomicMax(&s_run, j);
        __syncthreads();
        const u32 j = s_run, s = list[(u64)kl * BAM_CELL_CAP + j];
        if (tid == 0) {
            if (final_piece) atomicMin((unsigned long long*)&rm->err_key, (unsigned long long)(((meta->rec_total + base[kl] + j) << 4) | BAMR_ERR_MATE));
            else if (text_end - s > BAM_HEAD) { if (!meta->err) { meta->err = BAM_ERR_LIMIT; meta->err_at = s; } }
            else { meta->carry_start = s; meta->carry_len = text_end - s; meta->n_rec = base[kl] + j; }      // that record and what follows it wait for the next piece
        }
        total -= 1u;
    }
    if (tid == 0) { rm->n_reads = meta->err ? 0u : total; rm->max_len = 0; }
}

__global__ __launch_bounds__(256) void k_bamr_select(const u8* __restrict__ text, u32 n_cells, const BamMeta* __restrict__ meta, BamReadsMeta* __restrict__ rm,
                                                     const u32* __restrict__ count, const u32* __restrict__ base, const u32* __restrict__ list, const u32* __restrict__ kbase,
                                                     u32* __restrict__ rd_rec, u32* __restrict__ rd_info, u32* __restrict__ rd_ridx, int paired, int tiled) {
    __shared__ u32 s_w[4];
    const u64 rec_base = meta->rec_total; const u32 n_rec = meta->n_rec, n_reads = rm->n_reads;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 c_sec = 0, c_empty = 0, c_max = 0;
    for (u32 k = blockIdx.x; k < n_cells; k += gridDim.x) {
        const u32 cnt = count[k], b = base[k]; u32 run = kbase[k];
        for (u32 j0 = 0; j0 < cnt; j0 += 256u) {
            const u32 j = j0 + threadIdx.x;
            bool keep = false; u32 s = 0, info = 0;
            if (j < cnt && b + j < n_rec) {      // (records from n_rec on belong to the next piece)
                s = list[(u64)k * BAM_CELL_CAP + j];
                const u32 cls = bamr_class(text, s);
                if (cls == 1u) c_sec++;
                else if (cls == 2u) c_empty++;
                else {
                    keep = true;
                    const u32 flag = bam_ld16(text + s + 18), lseq = bam_ld32(text + s + 20);
                    const u32 var = 36u + text[s + 12] + 4u * bam_ld16(text + s + 16);      // bytes in front of SEQ, block_size included
                    const u32 q0 = s + var + (lseq + 1u) / 2u;
                    // tiled (mlst_set_read_tiling on an unpaired stream): a long read is cut into windows later -- if its SEQ and QUAL lie inside
                    // the record (a short read reaches at most 480 bytes past its head, which the slack behind the text covers, as before)
                    u32 bad = 0;
                    if (lseq > (u32)MLST_MAX_READ_LEN)
                        bad = !tiled ? BAMR_ERR_LONG : ((u64)var + ((u64)lseq + 1u) / 2u + lseq > (u64)bam_ld32(text + s) + 4u ? BAMR_ERR_SPAN : 0u);
                    if (bad) atomicMin((unsigned long long*)&rm->err_key, (unsigned long long)(((rec_base + b + j) << 4) | bad));
                    else {
                        info = lseq | ((flag & 0x10u) ? BAMR_REV : 0u) | (text[q0] == 0xFFu ? BAMR_NOQUAL : 0u);
                        if (lseq > c_max) c_max = lseq;
                    }
                    if (paired && !(flag & 1u)) atomicMin((unsigned long long*)&rm->err_key, (unsigned long long)(((rec_base + b + j) << 4) | BAMR_ERR_MATE));
                }
            }
            const u64 m = __ballot(keep);
            if (lane == 0) s_w[wv] = (u32)__popcll(m);
            __syncthreads();
            u32 at = run + (u32)__popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; w++) at += s_w[w];
            run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
            if (keep && at < n_reads) { rd_rec[at] = s; rd_info[at] = info; rd_ridx[at] = b + j; }
            __syncthreads();
        }
    }
    c_sec = wave_sum_u32(c_sec); c_empty = wave_sum_u32(c_empty);
    for (int o = 32; o > 0; o >>= 1) { const u32 y = __shfl_xor(c_max, o); c_max = y > c_max ? y : c_max; }
    if (lane == 0) {
        if (c_sec) atomicAdd((unsigned long long*)&rm->n_secondary, (unsigned long long)c_sec);
        if (c_empty) atomicAdd((unsigned long long*)&rm->n_empty, (unsigned long long)c_empty);
        if (c_max) atomicMax(&rm->max_len, c_max);
    }
}

// One thread per pair: the QNAMEs of reads 2p and 2p + 1 (l_read_name counts the NUL), byte by byte.
__global__ __launch_bounds__(256) void k_bamr_mates(const u8* __restrict__ text, const BamMeta* __restrict__ meta, BamReadsMeta* __restrict__ rm,
                                                    const u32* __restrict__ rd_rec, const u32* __restrict__ rd_ridx) {
    const u32 n_pairs = rm->n_reads >> 1;
    for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += gridDim.x * blockDim.x) {
        const u32 a = rd_rec[2u * p], b = rd_rec[2u * p + 1u];
        const u32 ln = text[a + 12];
        bool same = ln == text[b + 12];
        for (u32 i = 0; same && i < ln; i++) same = text[a + 36u + i] == text[b + 36u + i];
        if (!same) atomicMin((unsigned long long*)&rm->err_key, (unsigned long long)(((meta->rec_total + rd_ridx[2u * p]) << 4) | BAMR_ERR_MATE));
    }
}

// One workgroup per group of 64 reads, pack_group's two phases (mlst_engine.hip) behind a phase that places the group's reads.
// Phase one: thread = one 16-base word of one read: 16 nibbles of SEQ (at most 9 bytes) and 16 bytes of QUAL, front to back, or,
// for a read stored on the reference strand, back to front with the complement.  Nibbles 1 2 4 8 are A C G T; every other one is a
// non-ACGT base (packed as A, bit 7 of its quality byte, bit 15 of the length).  Phase two: the words leave LDS in the resident
// (transposed) order; one thread per read stores its length.
// WIN: the rows are windows of reads (k_bamt_emit, csrc/bam_tile.h): win_a[r] = record start | rd_info << 32, win_b[r] = the window's
// start in the READ | its length << 32.  Base p of a window is base st + p of the read; where that lies in SEQ / QUAL follows from
// the read's l_seq, the word count and lens from the window's length.  !WIN: win_a = rd_rec, win_b = rd_info, a window is its read.
template <bool WIN>
__global__ __launch_bounds__(256) void k_bamr_pack(const u8* __restrict__ text, const void* __restrict__ win_a, const void* __restrict__ win_b, u64 n_reads,
                                                   u32* __restrict__ packed, u8* __restrict__ qrows, u16* __restrict__ lens, u32 wpr, u32 qstride) {
    __shared__ u32 s_words[64 * RW]; __shared__ u32 s_anyn[2]; __shared__ u32 s_seq[64], s_info[64]; __shared__ u32 s_st[WIN ? 64 : 1], s_wl[WIN ? 64 : 1];
    const int tid = threadIdx.x;
    const u64 n_groups = (n_reads + 63) >> 6; const u32 total = 64u * wpr;
    for (u64 grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        if (tid < 2) s_anyn[tid] = 0;
        if (tid < 64) {
            const u64 r = grp * 64 + tid; u32 seq = 0, info = 0;
            u32 s = 0, st = 0, wl = 0;
            if (r < n_reads) {
                if (WIN) { const u64 a = ((const u64*)win_a)[r], b = ((const u64*)win_b)[r]; s = (u32)a; info = (u32)(a >> 32); st = (u32)b; wl = (u32)(b >> 32); }
                else { s = ((const u32*)win_a)[r]; info = ((const u32*)win_b)[r]; }
                seq = s + 36u + text[s + 12] + 4u * bam_ld16(text + s + 16);
            }
            s_seq[tid] = seq; s_info[tid] = info;
            if (WIN) { s_st[tid] = st; s_wl[tid] = wl; }
        }
        __syncthreads();
        for (u32 idx = (u32)tid; idx < total; idx += 256u) {
            const u32 i = idx / wpr, w = idx - i * wpr; const u64 r = grp * 64 + i;
            const u32 info = s_info[i]; const int n = (int)(info & BAMR_LEN);      // bases of the read
            const int st = WIN ? (int)s_st[i] : 0, wl = WIN ? (int)s_wl[i] : n;      // the window: its first base in the read, its bases
            u32 word = 0;
            if (r < n_reads) {
                u32 qw[4] = {0, 0, 0, 0}, anyn = 0;
                if ((int)(w * 16u) < wl) {
                    const bool rev = (info & BAMR_REV) != 0, noq = (info & BAMR_NOQUAL) != 0;
                    const u8* __restrict__ sq = text + s_seq[i]; const u8* __restrict__ ql = sq + ((u32)n + 1u) / 2u;
                    // base p = w * 16 + k of the window is base lo + k of the read: base hi - k (reverse) or lo + k (forward) of SEQ
                    const int lo = st + (int)(w * 16u), hi = n - 1 - lo;
                    const int first = rev ? hi - 15 : lo;                       // (may be negative: those bases lie beyond the read)
                    const int b0 = first >> 1, n_bytes = (n + 1) >> 1;          // (arithmetic shift: floor)
                    u64 nibs = 0; u32 nib16 = 0;                                // nibbles 2 * b0 ... 2 * b0 + 15 (the first one on top), and the 17th
                    #pragma unroll
                    for (int y = 0; y < 8; y++) { const int at = b0 + y; const u32 v = (at >= 0 && at < n_bytes) ? (u32)sq[at] : 0u; nibs |= (u64)v << (56 - 8 * y); }
                    { const int at = b0 + 8; if (at >= 0 && at < n_bytes) nib16 = (u32)sq[at] >> 4; }
                    #pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const int sp = rev ? hi - k : lo + k;                   // position in SEQ / QUAL
                        if ((int)(w * 16u) + k < wl) {                          // (st + wl <= n: the filler nibble of an odd l_seq is never a base)
                            const int t = sp - 2 * b0;                          // 0 .. 16
                            const u32 nib = t < 16 ? (u32)(nibs >> (t < 16 ? 60 - 4 * t : 0)) & 15u : nib16;
                            u32 code = nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u;
                            const u32 isn = code >> 2;
                            code = isn ? 0u : (rev ? 3u - code : code);         // complement: 1 <-> 8, 2 <-> 4
                            u32 q = noq ? 1u : (u32)ql[sp];
                            q = q > 127u ? 127u : q;
                            word |= code << (2 * k);
                            qw[k >> 2] |= (q | (isn << 7)) << (8 * (k & 3));
                            anyn |= isn;
                        }
                    }
                }
                #pragma unroll
                for (int j = 0; j < 4; j++) if (w * 16 + 4 * j < qstride) reinterpret_cast<u32*>(qrows + r * qstride)[w * 4 + j] = qw[j];     // qstride is a multiple of 4
                if (anyn) atomicOr(&s_anyn[i >> 5], 1u << (i & 31));      // LDS
            }
            s_words[i * wpr + w] = word;
        }
        __syncthreads();
        u32* out = packed + grp * total;
        for (u32 o = (u32)tid; o < total; o += 256u) out[o] = s_words[((o >> 1) & 63u) * wpr + ((o >> 7) << 1) + (o & 1u)];
        if (tid < 64) { const u64 r = grp * 64 + tid; if (r < n_reads) lens[r] = (u16)((WIN ? s_wl[tid] : (s_info[tid] & BAMR_LEN)) | (((s_anyn[tid >> 5] >> (tid & 31)) & 1u) << 15)); }
        __syncthreads();
    }
}

#endif
