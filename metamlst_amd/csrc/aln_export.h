// aln_export.h -- the engine's alignments to the chosen alleles as records (mlst_alignments_export / mlst_alignments_fetch; the rule:
// include/mlst.h; the SAM text is written on the host by metamlst_amd/samout.py).  Included by mlst_engine.hip behind fastq_tile.h.
//
// Every work item whose locus has a chosen allele is decided exactly as the pile-up decides it (pileup_body / k_pileup_dp): the
// ungapped alignment, or the banded one when gap_trigger fires; a record exists iff score >= floor_tab[n] && score > 0.  Nothing of
// the sample's state is written.
//   k_ax_ungapped_160 / _320  one wave per item: the read's planes staged as k_extend_pairs stages them (stage_read_planes), then
//                 ungapped_planes<., true, .> against the chosen allele and gap_trigger.  Leaves the item's AxItem (record or not,
//                 AS, XM, span, CIGAR operations); an item whose trigger fired goes on a list.
//   k_ax_dp<false> one lane per listed item, 64 x 64 lanes on the traceback store of k_pileup_dp: banded<true>, then the walk of
//                 k_pileup_dp from the best cell back to the start, counting the M / I / D runs.  Fills the item's AxItem.
//   k_ax_local    a thread per item, a workgroup per FQT_GROUP items: records, CIGAR operations and bases in front of the item inside
//                 its workgroup, and the workgroup's sums (three tables; k_fqt_scan / k_fqt_add of fastq_tile.h turn each into the
//                 exclusive sums over the whole item list and leave the totals, which size the output).
//   k_ax_emit     one wave per item with a record: lane 0 writes the fixed fields and, for an ungapped record, the CIGAR
//                 [bs S] (be - bs) M [(n - be) S]; the wave writes SEQ (ASCII, reference strand) and QUAL (raw Phred), 64 bytes per store.
//   k_ax_dp<true> the banded alignment and the walk again, this time writing the runs: the walk goes from the end of the alignment
//                 to its start, so the operations are written from the record's last one down.
// Plain vector stores only.
#ifndef MLST_ALN_EXPORT_H
#define MLST_ALN_EXPORT_H

#define AX_REC  1u      /* the item has a record */
#define AX_DP   2u      /* the banded alignment was taken (used_dp) */
#define AX_PEND 4u      /* gap_trigger fired: the item waits for k_ax_dp */

struct AxItem { int as, pos0; u16 ncig, be, n; u8 xm, flags; };      // 16 bytes per work item
struct AxOut {          // the record arrays on the device (layout: mlst_alignments_fetch)
    u64* read_index; u32* allele; int* pos0; int* as; int* xm; int* diag; u8* flags;
    u64* cigar_off; u32* cigar; u64* seq_off; u8* seq; u8* qual;
};

template <int NB>
__device__ __forceinline__ void ax_ungapped_body(const EngineDev* __restrict__ Ep, const KParams& P, const int* __restrict__ locus_chosen,
                                                 u64 n_items, AxItem* __restrict__ meta, u64* __restrict__ dp_list, u64* __restrict__ dp_n) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    __shared__ u32 s_rl[RW / 2 + 2]; __shared__ u32 s_rh[RW / 2 + 2]; __shared__ u32 s_rn[RW / 2 + 2]; __shared__ u32 s_odd[RW / 2 + 2];
    __shared__ u8 s_pen[RQ]; __shared__ u8 s_pentab[128];
    const int tid = threadIdx.x;
    for (int i = tid; i < 128; i += 64) s_pentab[i] = E.pen_tab[i];
    for (u64 ii = blockIdx.x; ii < n_items; ii += gridDim.x) {      // block-uniform
        const ItemDev it = E.items[ii];
        const int ca = locus_chosen[it.locus];
        AxItem o; o.as = 0; o.pos0 = 0; o.ncig = 0; o.be = 0; o.n = 0; o.xm = 0; o.flags = 0;
        if (ca >= 0) {
            const LocusDev L = E.loci[it.locus];
            const u32 lw = E.ret_len[it.ret]; const int n = (int)(lw & 0x7FFFu); const bool read_has_n = (lw & 0x8000u) != 0;
            __syncthreads();      // the rows of the item before are no longer read
            const int pen_def = __builtin_amdgcn_readfirstlane(stage_read_planes(E, P, it, n, s_rl, s_rh, s_rn, s_odd, s_pen, s_pentab, tid, 64));
            __syncthreads();
            u32 rl[NB], rh[NB], od[NB], rn[NB];
            #pragma unroll
            for (int w = 0; w < NB; w++) {
                rl[w] = __builtin_amdgcn_readfirstlane(s_rl[w]); rh[w] = __builtin_amdgcn_readfirstlane(s_rh[w]);
                od[w] = __builtin_amdgcn_readfirstlane(s_odd[w]);
                rn[w] = read_has_n ? __builtin_amdgcn_readfirstlane(s_rn[w]) : 0u;
            }
            // every lane aligns the same pair (the function is written for lanes = alleles; here there is one allele)
            const u32 a = (u32)ca - L.a_begin;
            const int m = (int)E.allele_len[ca], floor_n = E.floor_tab[n];
            int mm, bs, be;
            const int best = L.has_n ? ungapped_planes<NB, true, true>(E, P, L, a, m, n, it.diag, rl, rh, od, rn, s_pen, pen_def, read_has_n, mm, bs, be)
                                     : ungapped_planes<NB, true, false>(E, P, L, a, m, n, it.diag, rl, rh, od, rn, s_pen, pen_def, read_has_n, mm, bs, be);
            const int score = best >> MLST_P_SHIFT, xm = 255 - (best & 0xFF);
            o.n = (u16)n;
            if (gap_trigger(P, mm, xm, score, floor_n, m, n, it.diag, bs, be)) {
                o.flags = (u8)AX_PEND;
                if (tid == 0) dp_list[atomicAdd(dp_n, 1ull)] = ii;      // (at most one entry per item: the list holds n_items)
            } else if (score >= floor_n && score > 0) {
                o.flags = (u8)AX_REC; o.as = score; o.xm = (u8)xm; o.pos0 = bs + it.diag; o.be = (u16)be;
                o.ncig = (u16)((bs > 0) + 1 + (n - be > 0));
            }
        }
        if (tid == 0) meta[ii] = o;
    }
}
// reads up to 160 bases / up to MLST_MAX_READ_LEN (as k_pileup_160 / _320)
__global__ __launch_bounds__(64) void k_ax_ungapped_160(const EngineDev* __restrict__ Ep, KParams P, const int* __restrict__ locus_chosen, u64 n_items,
                                                        AxItem* __restrict__ meta, u64* __restrict__ dp_list, u64* __restrict__ dp_n) {
    ax_ungapped_body<5>(Ep, P, locus_chosen, n_items, meta, dp_list, dp_n);
}
__global__ __launch_bounds__(64) void k_ax_ungapped_320(const EngineDev* __restrict__ Ep, KParams P, const int* __restrict__ locus_chosen, u64 n_items,
                                                        AxItem* __restrict__ meta, u64* __restrict__ dp_list, u64* __restrict__ dp_n) {
    ax_ungapped_body<RW / 2>(Ep, P, locus_chosen, n_items, meta, dp_list, dp_n);
}

// The walk of k_pileup_dp over the traceback bytes of banded<true>, from the best cell (bi, bb) back to the alignment's start, as
// CIGAR runs in reference orientation: M for a diagonal step, D for a step along the allele, I for a step along the read, S for the
// oriented bases behind row bi and in front of the first aligned row.  The walk meets the runs last to first: with cig != NULL run
// number k from the end is written to cig[ncig - 1 - k].  Returns the number of runs; pos0 = the leftmost allele column of the walk.
__device__ inline int ax_walk(const u8* __restrict__ TB, int bi, int bb, int diag, int W, int n, u32* __restrict__ cig, int ncig, int& pos0) {
    const int BWMAX = 2 * MAX_W + 1, BW = 2 * W + 1;
    int i = bi, b = bb, state = 0, ops = 0, run_op = -1, run_len = 0;
    auto flush = [&]() { if (run_len > 0) { if (cig && ops < ncig) cig[ncig - 1 - ops] = ((u32)run_len << 4) | (u32)run_op; ops++; } run_len = 0; };
    auto push = [&](int op, int len) { if (op != run_op) { flush(); run_op = op; } run_len += len; };
    pos0 = 0;
    if (n - 1 - bi > 0) push(4, n - 1 - bi);
    while (i >= 0 && b >= 0 && b < BW) {
        const u8 t = TB[i * BWMAX + b];
        if (state == 0) {
            const int src = t & 3;
            if (src == 0) break;
            if (src == 1) { pos0 = i + diag - W + b; push(0, 1); i--; }
            else if (src == 2) state = 1; else state = 2;
        } else if (state == 1) { const int ext = t & 4; pos0 = i + diag - W + b; push(2, 1); b--; state = ext ? 1 : 0; }
        else { const int ext = t & 8; push(1, 1); i--; b++; state = ext ? 2 : 0; }
    }
    if (i + 1 > 0) push(4, i + 1);
    flush();
    return ops;
}

// EMIT = false: the listed items' AxItem (banded score, XM, span, runs);  EMIT = true: the runs of those that have a record.
// 64 workgroups of 64 lanes at the most: lane k of workgroup g owns slice 64 g + k of the traceback store, as in k_pileup_dp.
template <bool EMIT>
__global__ __launch_bounds__(64) void k_ax_dp(const EngineDev* __restrict__ Ep, KParams P, const int* __restrict__ locus_chosen,
                                              const u64* __restrict__ dp_list, const u64* __restrict__ dp_n, u8* __restrict__ tb_scratch,
                                              AxItem* __restrict__ meta, const u64* __restrict__ off_cig, u32* __restrict__ cigar) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    __shared__ u8 s_pentab[128];
    for (int i = threadIdx.x; i < 128; i += 64) s_pentab[i] = E.pen_tab[i];
    __syncthreads();
    const u64 end = *dp_n;
    const int BWMAX = 2 * MAX_W + 1;
    u8* TB = tb_scratch + ((u64)blockIdx.x * 64 + threadIdx.x) * (u64)(MLST_MAX_READ_LEN * BWMAX);
    for (u64 k = (u64)blockIdx.x * 64 + threadIdx.x; k < end; k += (u64)gridDim.x * 64) {
        const u64 ii = dp_list[k];
        if (EMIT && !(meta[ii].flags & AX_REC)) continue;
        const ItemDev it = E.items[ii];
        const int ca = locus_chosen[it.locus];
        const LocusDev L = E.loci[it.locus];
        const u32 a = (u32)ca - L.a_begin;
        const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
        int bi, bb, pos0;
        const int best = banded<true>(E, P, it, L, a, n, s_pentab, TB, bi, bb);
        if (EMIT) { ax_walk(TB, bi, bb, it.diag, P.band_w, n, cigar + off_cig[ii], (int)meta[ii].ncig, pos0); continue; }
        const int score = best >> MLST_P_SHIFT, xm = 255 - (best & 0xFF);
        AxItem o; o.as = 0; o.pos0 = 0; o.ncig = 0; o.be = 0; o.n = (u16)n; o.xm = 0; o.flags = 0;
        if (score >= E.floor_tab[n] && score > 0) {
            o.ncig = (u16)ax_walk(TB, bi, bb, it.diag, P.band_w, n, nullptr, 0, pos0);
            o.flags = (u8)(AX_REC | AX_DP); o.as = score; o.xm = (u8)xm; o.pos0 = pos0;
        }
        meta[ii] = o;
    }
}

// Per item: records, CIGAR operations and bases of the items in front of it in its workgroup; per workgroup: its sums.
__global__ __launch_bounds__(1024) void k_ax_local(const AxItem* __restrict__ meta, u64 n_items, u64* __restrict__ wex_rec, u64* __restrict__ wex_cig,
                                                   u64* __restrict__ wex_seq, u64* __restrict__ gs_rec, u64* __restrict__ gs_cig, u64* __restrict__ gs_seq) {
    __shared__ u64 s_w[3][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 i = (u64)blockIdx.x * FQT_GROUP + threadIdx.x;
    u64 v[3] = {0, 0, 0};
    if (i < n_items) { const AxItem m = meta[i]; if (m.flags & AX_REC) { v[0] = 1; v[1] = m.ncig; v[2] = m.n; } }
    u64 inc[3];
    #pragma unroll
    for (int q = 0; q < 3; q++) { inc[q] = fqt_wave_incl(v[q]); if (lane == 63) s_w[q][wv] = inc[q]; }
    __syncthreads();
    u64* wex[3] = {wex_rec, wex_cig, wex_seq}; u64* gs[3] = {gs_rec, gs_cig, gs_seq};
    #pragma unroll
    for (int q = 0; q < 3; q++) {
        u64 before = 0, all = 0;
        for (int k = 0; k < 16; k++) { const u64 x = s_w[q][k]; if (k < wv) before += x; all += x; }
        if (i < n_items) wex[q][i] = before + inc[q] - v[q];
        if (threadIdx.x == 0) gs[q][blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(64) void k_ax_emit(const EngineDev* __restrict__ Ep, const int* __restrict__ locus_chosen, const AxItem* __restrict__ meta,
                                                u64 n_items, const u64* __restrict__ off_rec, const u64* __restrict__ off_cig, const u64* __restrict__ off_seq,
                                                AxOut O, u64 n_rec, u64 n_cig, u64 n_seq) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) { O.cigar_off[n_rec] = n_cig; O.seq_off[n_rec] = n_seq; }
    for (u64 ii = blockIdx.x; ii < n_items; ii += gridDim.x) {      // block-uniform
        const AxItem m = meta[ii];
        if (!(m.flags & AX_REC)) continue;
        const ItemDev it = E.items[ii];
        const u64 r = off_rec[ii], c0 = off_cig[ii], s0 = off_seq[ii];
        const int n = (int)m.n;
        if (lane == 0) {
            O.read_index[r] = E.ret_ridx[it.ret]; O.allele[r] = (u32)locus_chosen[it.locus]; O.pos0[r] = m.pos0; O.as[r] = m.as; O.xm[r] = (int)m.xm;
            O.diag[r] = it.diag; O.flags[r] = (u8)((it.strand ? 1u : 0u) | ((m.flags & AX_DP) ? 2u : 0u));
            O.cigar_off[r] = c0; O.seq_off[r] = s0;
            if (!(m.flags & AX_DP)) {
                const int bs = m.pos0 - it.diag, be = (int)m.be; u64 c = c0;
                if (bs > 0) O.cigar[c++] = ((u32)bs << 4) | 4u;
                O.cigar[c++] = (u32)(be - bs) << 4;
                if (n - be > 0) O.cigar[c++] = ((u32)(n - be) << 4) | 4u;
            }
        }
        auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
        for (int i = lane; i < n; i += 64) {
            const int s = it.strand ? n - 1 - i : i;
            const u8 qb = rq[s];
            u32 b = (rb[s >> 4] >> (2 * (s & 15))) & 3u; if (it.strand) b ^= 3u;
            O.seq[s0 + (u64)i] = (qb & 0x80u) ? (u8)'N' : (u8)(0x54474341u >> (8 * b));      // "ACGT"
            O.qual[s0 + (u64)i] = (u8)(qb & 0x7Fu);
        }
    }
}

#endif
