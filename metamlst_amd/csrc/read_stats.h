// read_stats.h -- per-cycle read statistics counted on the device (mlst_set_read_stats; the rule: include/mlst.h, stated on the host
// as metamlst_amd.fastq.read_stats; `cli type --read-stats`).  Included by mlst_engine.hip next to read_prep.h.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records; read_prep.h).  The tables
// are counted from those three and the text, which the parser has just touched, in front of the read-back of the parser's flags:
//   k_rs_count<QB>  lanes are CYCLES, not reads.  A wave takes one read at a time; lane l loads the four base bytes and the four quality
//                 bytes of cycles 4 l .. 4 l + 3 (one coalesced load of up to 256 bytes per line; lanes 0-15 load cycles 256 .. 319 of
//                 a read longer than 256 with a second one), and adds 1 to the LDS cells of those cycles.  Byte k of every lane goes
//                 out in one instruction, so its lanes stand on the cycles 4 l + k: 64 different rows, no two lanes of an instruction
//                 on one address, whatever the reads hold.  (The natural mapping, lane = read, sends all 64 lanes of cycle c to the
//                 handful of cells of that cycle.)  The row of cycle c is (c & 3) * 80 + (c >> 2): the lanes of an instruction stand on
//                 CONSECUTIVE rows, and with an odd row stride (95 words for the 94 quality bins, 5 for the letters) 32 consecutive
//                 rows fall on the 32 banks of a ds 32-bit operation's lane group when the lanes hold the same value; what is left
//                 are the chance meetings of different values.  Waves of the workgroup meet on a cell: the adds are LDS atomics.
//                 The offsets and lengths of 64 reads are loaded by the 64 lanes at once and handed round by lane index; the text of
//                 RS_DEPTH reads is loaded before the first of them is counted.
//                 Per read: the lanes' G/C counts and quality sums are packed into one word and reduced over the wave once; lane 0
//                 adds into the three small LDS histograms (length, GC %, mean quality).
//                 LDS: 320 x 95 + 320 x 5 + 321 + 101 + 94 words and three 64-bit totals = 130,120 bytes with alignment, one workgroup
//                 of 16 waves per CU.  A chunk holds fewer than 2^32 lines, so fewer than 2^30 reads: a 32-bit cell cannot overflow within a launch.
//                 Flush: once per workgroup, the non-zero cells go to the 64-bit tables with ordinary atomics, walked in the tables'
//                 order (consecutive lanes: consecutive bins of a cycle, consecutive banks, consecutive addresses).  The grid is at
//                 most one workgroup per CU and at most one per RS_WG_READS reads, so a small chunk pays a small flush.
//                 Paired chunks: a workgroup counts ONE side (blockIdx & 1) and takes only that side's reads, so the LDS holds one
//                 side's tables, nothing is zeroed or flushed twice and a paired chunk is one pass like an unpaired one; both sides'
//                 tables would need 254 KB.
// A chunk the parser flagged malformed is not walked (k_rp_qtrim's reason).  Plain vector stores and ordinary atomics only; no scratch,
// no per-thread array.
// The compiler's resource figures stand at the kernel.
#ifndef MLST_READ_STATS_H
#define MLST_READ_STATS_H

#define RS_CYCLES 320                 // MLST_MAX_READ_LEN
#define RS_NQ 94                      // Phred bins 0..93
#define RS_QSTRIDE 95                 // words per LDS row of the quality table (odd)
#define RS_LANE_ROWS 80               // RS_CYCLES / 4: the row of cycle c is (c & 3) * RS_LANE_ROWS + (c >> 2)
#define RS_WG_READS 4096u             // reads per workgroup below which the grid shrinks
#define RS_DEPTH 4u                   // reads a wave has in flight
// the table block of one stage and side, in 64-bit words (MLST_RS_* of include/mlst.h)
#define RS_O_READS 0
#define RS_O_BASES 1
#define RS_O_LOW 2
#define RS_O_LEN 4
#define RS_O_BASE (RS_O_LEN + RS_CYCLES + 1)
#define RS_O_QUAL (RS_O_BASE + RS_CYCLES * 5)
#define RS_O_GC (RS_O_QUAL + RS_CYCLES * RS_NQ)
#define RS_O_RQ (RS_O_GC + 101)
#define RS_WORDS (RS_O_RQ + RS_NQ)
static_assert(RS_CYCLES == MLST_MAX_READ_LEN, "the tables hold one row per cycle of the longest read");
static_assert(RS_WORDS == MLST_RS_WORDS && RS_O_LEN == MLST_RS_LEN && RS_O_BASE == MLST_RS_BASE && RS_O_QUAL == MLST_RS_QUAL && RS_O_GC == MLST_RS_GC && RS_O_RQ == MLST_RS_READQUAL,
              "include/mlst.h publishes the block's layout");

// four cycles c0 .. c0 + 3 of an n-base read: b4 / q4 are what rs_load4 loaded for them, row0 = c0 >> 2.  acc: quality sum in the
// low half, G + C count in the high half (at most 320 * 93 and 320 over a whole read); low: characters below the Phred base
template <u32 QB>
__device__ inline void rs_add4(u32 b4, u32 q4, u32 c0, u32 n, u32 row0, u32* s_qual, u32* s_base, u32& acc, u32& low) {
    const u32 sh = (c0 + 4 > n && n >= 4) ? 8 * (c0 + 4 - n) : 0u;      // the read's last, partial four bytes were loaded from n - 4 on (rs_load4)
    b4 >>= sh; q4 >>= sh;
    #pragma unroll
    for (u32 k = 0; k < 4; k++) {
        if (c0 + k < n) {
            const u32 b = ((b4 >> (8 * k)) & 0xFFu) & 0xDFu, ch = (q4 >> (8 * k)) & 0xFFu;
            const u32 col = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;      // (pack_group's N bit: every byte that is none of ACGT in either case)
            u32 v = ch > QB ? ch - QB : 0u; v = v > 93u ? 93u : v;      // min(clamp(ch - QB, 0, 127), 93)
            const u32 row = k * RS_LANE_ROWS + row0;
            atomicAdd(&s_qual[row * RS_QSTRIDE + v], 1u);
            atomicAdd(&s_base[row * 5 + col], 1u);
            acc += v + ((col == 1u || col == 2u) ? 0x10000u : 0u);
            low += ch < QB ? 1u : 0u;
        }
    }
}

// the bytes of cycles c0 .. c0 + 3 of the n-base line at p, as one unaligned 32-bit load whose value is not looked at here: several
// reads' loads are in flight before the first is counted.  Nothing outside the line is loaded: its last, partial four bytes come as
// the four bytes that END the line (rs_add4 shifts them down); only a line of fewer than four bytes is loaded byte by byte.
__device__ inline u32 rs_load4(const u8* __restrict__ p, u32 c0, u32 n) {
    u32 w = 0;
    if (c0 < n) {
        if (n >= 4) __builtin_memcpy(&w, p + (c0 + 4 <= n ? c0 : n - 4), 4);
        else {      // c0 is 0: one, two or three bytes
            w = p[0];
            if (n > 1) w |= (u32)p[1] << 8;
            if (n > 2) w |= (u32)p[2] << 16;
        }
    }
    return w;
}

// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, k_rs_count<33> and <64>: 80 VGPRs, 0 AGPRs, 81 / 80 SGPRs, no
// scratch, no spill of either kind, 130,120 bytes of LDS, 4 waves per SIMD -- the 16 waves of the one workgroup the LDS lets a CU hold
// (1024 threads take at most 128 VGPRs, so the registers cost no wave).
template <u32 QB>
__global__ __launch_bounds__(1024) void k_rs_count(const u8* __restrict__ text, const u64* __restrict__ seq_off, const u64* __restrict__ qual_off, const u16* __restrict__ lens,
                                                    u64 n_reads, u32 paired, u32 side /* unpaired: the current side */, u32 count_low /* the raw stage */,
                                                    const u32* __restrict__ flags /* the parser's: [1] = errors */, u64* __restrict__ tab /* the stage's two blocks: side 0, side 1 */) {
    if (flags[1]) return;      // (as in k_rp_qtrim: a malformed record's quality line may be shorter than its sequence; the host refuses the chunk)
    __shared__ u32 s_qual[RS_CYCLES * RS_QSTRIDE];
    __shared__ u32 s_base[RS_CYCLES * 5];
    __shared__ u32 s_len[RS_CYCLES + 1];
    __shared__ u32 s_gc[101];
    __shared__ u32 s_rq[RS_NQ];
    __shared__ unsigned long long s_tot[3];      // reads, bases, characters below the base
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;
    for (u32 i = tid; i < RS_CYCLES * RS_QSTRIDE; i += blockDim.x) s_qual[i] = 0;
    for (u32 i = tid; i < RS_CYCLES * 5; i += blockDim.x) s_base[i] = 0;
    for (u32 i = tid; i < RS_CYCLES + 1; i += blockDim.x) s_len[i] = 0;
    if (tid < 101) s_gc[tid] = 0;
    if (tid < RS_NQ) s_rq[tid] = 0;
    if (tid < 3) s_tot[tid] = 0;
    __syncthreads();
    // this workgroup's side and its place among the workgroups of that side
    const u32 my_side = paired ? (blockIdx.x & 1u) : side;
    const u64 wg = paired ? blockIdx.x >> 1 : blockIdx.x, n_wg = paired ? (gridDim.x + 1 - my_side) >> 1 : gridDim.x;
    const u64 n_mine = paired ? (n_reads + 1 - my_side) >> 1 : n_reads;      // reads of my side: 2 j + side, or j
    const u64 n_batches = (n_mine + 63) >> 6;
    u64 w_reads = 0, w_bases = 0; u32 low = 0;
    for (u64 bt = wg * n_waves + wave; bt < n_batches; bt += n_wg * n_waves) {
        const u64 j = bt * 64 + lane; const bool in = j < n_mine;
        const u64 r = paired ? 2 * j + my_side : j;
        const u64 so_l = in ? seq_off[r] : 0, qo_l = in ? qual_off[r] : 0;
        u32 n_l = in ? (u32)(lens[r] & 0x7FFFu) : 0u; n_l = n_l > RS_CYCLES ? RS_CYCLES : n_l;      // (a longer read has set flags[1]; the rows end at RS_CYCLES all the same)
        const u32 cnt = (u32)(n_mine - bt * 64 < 64 ? n_mine - bt * 64 : 64);
        // RS_DEPTH reads at a time: the loads of all of them, then their counting (a wave has one workgroup's share of the CU's 16
        // waves to hide the text's latency behind, so it keeps several reads in flight itself)
        for (u32 i0 = 0; i0 < cnt; i0 += RS_DEPTH) {
            u32 nn[RS_DEPTH], ba[RS_DEPTH], qa[RS_DEPTH], bb[RS_DEPTH], qb[RS_DEPTH];      // (constant indices only: registers)
            #pragma unroll
            for (u32 d = 0; d < RS_DEPTH; d++) {
                nn[d] = 0; ba[d] = qa[d] = bb[d] = qb[d] = 0;
                if (i0 + d < cnt) {
                    nn[d] = __shfl(n_l, (int)(i0 + d)); const u64 so = __shfl(so_l, (int)(i0 + d)), qo = __shfl(qo_l, (int)(i0 + d));
                    ba[d] = rs_load4(text + so, 4 * lane, nn[d]); qa[d] = rs_load4(text + qo, 4 * lane, nn[d]);
                    if (nn[d] > 256) { bb[d] = rs_load4(text + so, 256 + 4 * lane, nn[d]); qb[d] = rs_load4(text + qo, 256 + 4 * lane, nn[d]); }
                }
            }
            #pragma unroll
            for (u32 d = 0; d < RS_DEPTH; d++) {
                if (i0 + d < cnt) {
                    const u32 n = nn[d];
                    u32 acc = 0;
                    rs_add4<QB>(ba[d], qa[d], 4 * lane, n, lane, s_qual, s_base, acc, low);
                    if (n > 256) rs_add4<QB>(bb[d], qb[d], 256 + 4 * lane, n, 64 + lane, s_qual, s_base, acc, low);      // (lanes 16-63 stand beyond cycle 319: nothing)
                    acc = wave_sum_u32(acc);
                    if (lane == 0) {
                        atomicAdd(&s_len[n], 1u);
                        if (n) { atomicAdd(&s_gc[(100u * (acc >> 16)) / n], 1u); atomicAdd(&s_rq[(acc & 0xFFFFu) / n], 1u); }
                    }
                    w_reads++; w_bases += n;
                }
            }
        }
    }
    low = wave_sum_u32(low);
    if (lane == 0 && w_reads) {
        atomicAdd(&s_tot[0], (unsigned long long)w_reads); atomicAdd(&s_tot[1], (unsigned long long)w_bases);
        if (count_low && low) atomicAdd(&s_tot[2], (unsigned long long)low);
    }
    __syncthreads();
    // the flush, in the tables' order
    unsigned long long* const out = (unsigned long long*)(tab + (u64)my_side * RS_WORDS);
    for (u32 t = tid; t < RS_CYCLES * RS_NQ; t += blockDim.x) {
        const u32 c = t / RS_NQ, q = t - c * RS_NQ;
        const u32 v = s_qual[((c & 3u) * RS_LANE_ROWS + (c >> 2)) * RS_QSTRIDE + q];
        if (v) atomicAdd(out + RS_O_QUAL + t, (unsigned long long)v);
    }
    for (u32 t = tid; t < RS_CYCLES * 5; t += blockDim.x) {
        const u32 c = t / 5u, b = t - c * 5u;
        const u32 v = s_base[((c & 3u) * RS_LANE_ROWS + (c >> 2)) * 5 + b];
        if (v) atomicAdd(out + RS_O_BASE + t, (unsigned long long)v);
    }
    for (u32 t = tid; t < RS_CYCLES + 1; t += blockDim.x) if (s_len[t]) atomicAdd(out + RS_O_LEN + t, (unsigned long long)s_len[t]);
    if (tid < 101 && s_gc[tid]) atomicAdd(out + RS_O_GC + tid, (unsigned long long)s_gc[tid]);
    if (tid < RS_NQ && s_rq[tid]) atomicAdd(out + RS_O_RQ + tid, (unsigned long long)s_rq[tid]);
    if (tid < 3 && s_tot[tid]) atomicAdd(out + tid, s_tot[tid]);
}

#endif
