// reads_text.h -- the reads that align to the loci as FASTQ text, written on the device (mlst_reads_text_open / _next / _close; the rule:
// include/mlst.h and metamlst_amd/samout.py reads_fastq_rule, `cli type --write-reads`).  Included by mlst_engine.hip behind aln_text.h.
//
// A read is written iff one of its (work item, allele of the item's locus) pairs has a record in the full export (aln_text.h).  The host
// plans the rounds with the planner of that export (at_plan: the same sort, the same tables, rounds cut at read boundaries); a round
// first runs k_at_decide_160 / _320 and k_at_dp<false, false, false> as at_prepare launches them, so AT_REC of every pair is the full
// export's by construction.  Then, per round:
//   k_rt_mark   one wave per read: walks the AtPair of the read's consecutive pairs, 64 per turn, and leaves at the first turn whose
//               ballot finds AT_REC.  Lane 0 stores the exact byte length of the read's FASTQ record into the per-read table (AtDev::wex,
//               which holds one entry per READ of the round here, plus a closing entry of 0), 0 for a read that is not written.
//   k_at_local / k_fqt_scan / k_fqt_add (aln_text.h, fastq_tile.h) as they are, over the round's reads + 1: the lengths become the
//               records' offsets in the text, the closing entry the text's end.
//   k_rt_write  one wave per read whose record has a length: `@`, the name (r<k> through AtOut, or the kept name out of the arena through
//               at_qname) and `/1` `/2` under paired; SEQ and QUAL rendered once into LDS in read orientation (at_base with strand 0, the
//               clamp at 93) and copied by the wave with at_copy; `\n+\n` and the line ends.
// The read's retained slot is that of its first item in the sorted list (every item of a read index holds the same read).
// Plain vector stores and ordinary atomics only; no per-thread array, no scratch.
#ifndef MLST_READS_TEXT_H
#define MLST_READS_TEXT_H

// A bound from above on the bytes of one read's FASTQ record: `@`, the name (r + 20 digits, or the longest kept name where that is
// longer), `/1`, LF, SEQ, LF `+` LF, QUAL, LF = 2 n + name + 8 <= 2 n + max_qname + 10.
__host__ __device__ inline u64 rt_text_bound(u32 n, u64 max_qname) { return 2ull * n + (max_qname > 21 ? max_qname : 21ull) + 10ull; }
// The device tables of a round, per (item, allele) pair: AtPair, the entry of the list of the banded SW, and the 8 bytes the full export
// keeps per pair for its offsets (this export keeps them per read; the figure is the full export's, a bound from above here).
#define RT_PAIR_BYTES 36ull
// What the planner sums against round_bytes per read: its text or the tables of its pairs, whichever is larger.
__host__ __device__ inline u64 rt_read_bound(u32 n, u64 max_qname, u64 n_pairs) {
    const u64 t = rt_text_bound(n, max_qname), p = RT_PAIR_BYTES * n_pairs;
    return t > p ? t : p;
}

// the exact bytes of a read's record: @ name [/m] LF SEQ LF + LF QUAL LF
__device__ inline u64 rt_record_len(u32 n, u64 k, AtQn qn, int paired) {
    return 2ull * n + 6ull + (qn.len ? (u64)qn.len : 1ull + at_digits64(k)) + (paired ? 2ull : 0ull);
}

// k_rt_mark<NAMES>: one wave per read of the round; D.wex = the per-read table (R.r1 - R.r0 + 1 entries), D.n_rec = the written reads.
// gfx950, -O3 (kernel-resource-usage): <false> 36 VGPRs, 40 SGPRs, no LDS, no scratch, 8 waves per SIMD;
//                                      <true>  36 VGPRs, 42 SGPRs, no LDS, no scratch, 8 waves per SIMD.
template <bool NAMES>
__global__ __launch_bounds__(64) void k_rt_mark(const EngineDev* __restrict__ Ep, const AtDev* __restrict__ Dp, AtRound R) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    const int lane = threadIdx.x;
    u64 written = 0;
    for (u64 r = R.r0 + blockIdx.x; r < R.r1; r += gridDim.x) {      // block-uniform
        const u64 kf = D.read_first[r], kl = D.read_first[r + 1];
        const u64 q0 = D.pair_off[kf] - R.pb, q1 = D.pair_off[kl] - R.pb;
        bool any = false;
        for (u64 b = q0; b < q1 && !any; b += 64) {      // wave-uniform: the wave leaves at the first turn that finds a record
            const u64 q = b + (u64)lane;
            const bool rec = q < q1 && (D.meta[q].flags & AT_REC);
            any = __ballot(rec) != 0ull;
        }
        if (lane == 0) {
            u64 len = 0;
            if (any) {
                const ItemDev it = E.items[D.perm[kf]];
                const u64 ridx = E.ret_ridx[it.ret];
                len = rt_record_len((u32)(E.ret_len[it.ret] & 0x7FFFu), D.paired ? ridx >> 1 : ridx, at_qname<NAMES>(D, it.ret), D.paired);
                written++;
            }
            D.wex[r - R.r0] = len;
        }
    }
    if (lane == 0 && written) atomicAdd((u64*)D.n_rec, written);
}

// k_rt_write<NAMES>: one wave per read; D.wex = the records' offsets in the text (entry r + 1 - entry r = the record's bytes).
// gfx950, -O3 (kernel-resource-usage): <false> 96 VGPRs, 61 SGPRs, 640 bytes LDS, no scratch, 5 waves per SIMD;
//                                      <true>  96 VGPRs, 60 SGPRs, 640 bytes LDS, no scratch, 5 waves per SIMD
// (the two copies of at_copy are unrolled; the kernel waits on its stores, not on registers).
template <bool NAMES>
__global__ __launch_bounds__(64) void k_rt_write(const EngineDev* __restrict__ Ep, const AtDev* __restrict__ Dp, AtRound R, u8* __restrict__ text) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    __shared__ u8 s_seq[RQ]; __shared__ u8 s_qual[RQ];
    const int lane = threadIdx.x;
    for (u64 r = R.r0 + blockIdx.x; r < R.r1; r += gridDim.x) {      // block-uniform
        const u64 at = uniform_u64(D.wex[r - R.r0]), end = uniform_u64(D.wex[r - R.r0 + 1]);
        if (end == at) continue;      // (block-uniform) the read has no record: not written
        const ItemDev it = E.items[D.perm[D.read_first[r]]];
        const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
        const u64 ridx = E.ret_ridx[it.ret];
        const AtQn qn = at_qname<NAMES>(D, it.ret);
        __syncthreads();      // the rows of the read before are no longer read
        {
            auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
            for (int i = lane; i < n; i += 64) { u8 c, q; at_base(rb, rq, n, 0, i, c, q); s_seq[i] = c; s_qual[i] = (u8)((q > 93 ? 93 : q) + 33); }
        }
        __syncthreads();
        u8* p = text + at;
        u64 head;      // the bytes in front of SEQ: @ name [/m] LF
        if (qn.len) {
            for (u32 i = (u32)lane; i < qn.len; i += 64) p[1 + i] = qn.p[i];
            head = 1ull + qn.len;
        } else {
            const u64 k = D.paired ? ridx >> 1 : ridx;
            if (lane == 0) { AtOut<true> o; o.p = p; o.n = 1; o.ch('r'); o.dec64(k); }
            head = 2ull + at_digits64(k);
        }
        if (lane == 0) {
            p[0] = (u8)'@';
            if (D.paired) { p[head] = (u8)'/'; p[head + 1] = (u8)((ridx & 1ull) ? '2' : '1'); }
        }
        head += D.paired ? 2ull : 0ull;
        if (lane == 0) {
            p[head] = (u8)'\n';
            p[head + 1 + (u64)n] = (u8)'\n'; p[head + 2 + (u64)n] = (u8)'+'; p[head + 3 + (u64)n] = (u8)'\n';
            p[head + 4 + 2 * (u64)n] = (u8)'\n';
        }
        at_copy(p + head + 1, s_seq, n, lane);
        at_copy(p + head + 4 + (u64)n, s_qual, n, lane);
    }
}

#endif
