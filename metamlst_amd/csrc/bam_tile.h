// bam_tile.h -- BAM reads longer than the tile cut into windows on the device (included by mlst_engine.hip behind bam_reads.h and
// fastq_tile.h; switch: mlst_set_read_tiling on an unpaired reads stream; the rule: include/mlst.h, stated on the host as
// samin.bam_reads_fastq followed by fastq.tile_fastq).
//
// k_bamr_select has left the kept-read table of the piece (record start, l_seq | strand | no-qualities bits) and the piece's longest
// kept read.  Only a piece with a read longer than the tile comes here:
//   k_bamt_count : a thread per kept read, a workgroup per FQT_GROUP reads: the read's windows (fa_windows_of with min_len 0) from
//                  its l_seq, the windows of the workgroup's reads in front of it, and the workgroup's sum -- k_fqt_count with the
//                  kept-read table in place of the FASTQ line table
//   k_fqt_scan, k_fqt_add (csrc/fastq_tile.h) as they are, on the same FqtDev (wex, gsum, meta, n_recs, read_len, stride; the text
//                  and line-table fields stay unset)
//   k_bamt_emit  : a thread per window of a round [w0, w1): its read by binary search in the prefix table, then what k_bamr_pack<true>
//                  takes: the read's record start and info, the window's start IN THE READ and its length
// Windows are cut from the read, not from the stored SEQ: for a record on the reverse strand the packer turns the start round
// (window st of the read is bases n - 1 - st ... of SEQ, complemented; the window flush with the read's end lies at SEQ's front).
#ifndef MLST_BAM_TILE_H
#define MLST_BAM_TILE_H

__global__ __launch_bounds__(1024) void k_bamt_count(const FqtDev* __restrict__ Dp, const u32* __restrict__ rd_info) {
    __shared__ u64 s_w[16]; __shared__ u32 s_cut[16];
    const FqtDev& D = *Dp;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 r = (u64)blockIdx.x * FQT_GROUP + threadIdx.x;
    u64 n = 0, w = 0; u32 cut = 0;
    if (r < D.n_recs) {
        n = rd_info[r] & BAMR_LEN;
        w = fa_windows_of(n, D.read_len, D.stride, 0u);
        cut = n > (u64)D.read_len ? 1u : 0u;
    }
    const u64 inc = fqt_wave_incl(w);
    u64 mx = n;
    for (int o = 32; o > 0; o >>= 1) { const u64 y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
    cut = wave_sum_u32(cut);
    if (lane == 63) s_w[wv] = inc;
    if (lane == 0) { s_cut[wv] = cut; if (mx) atomicMax((unsigned long long*)&D.meta.p->max_rec, (unsigned long long)mx); }
    __syncthreads();
    u64 before = 0, all = 0; u32 c = 0;
    for (int k = 0; k < 16; k++) { const u64 x = s_w[k]; if (k < wv) before += x; all += x; c += s_cut[k]; }
    if (r < D.n_recs) D.wex[r] = before + inc - w;
    if (threadIdx.x == 0) { D.gsum[blockIdx.x] = all; if (c) atomicAdd((unsigned long long*)&D.meta.p->n_cut, (unsigned long long)c); }
}

// One thread per window of [w0, w1): entry w - w0 of win_a (record start | info << 32) and win_b (start in the read | length << 32):
// two coalesced 8-byte stores per thread.
__global__ __launch_bounds__(256) void k_bamt_emit(const FqtDev* __restrict__ Dp, const u32* __restrict__ rd_rec, const u32* __restrict__ rd_info, u64 w0, u64 w1,
                                                   u64* __restrict__ win_a, u64* __restrict__ win_b) {
    const FqtDev& D = *Dp;
    const u64 nr = D.n_recs; const u32 L = D.read_len, S = D.stride;
    for (u64 w = w0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; w < w1; w += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = nr;      // the last read with wex[r] <= w (every kept read has at least one window: the table rises strictly)
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (D.wex[mid] <= w) lo = mid + 1; else hi = mid; }
        const u64 r = lo - 1;     // (wex[0] = 0 <= w)
        const u32 info = rd_info[r]; const u64 n = info & BAMR_LEN;
        u64 st = 0; u32 len = (u32)n;
        if (n > (u64)L) { st = (w - D.wex[r]) * S; if (st > n - L) st = n - L; len = L; }
        const u64 o = w - w0;
        win_a[o] = (u64)rd_rec[r] | ((u64)info << 32); win_b[o] = st | ((u64)len << 32);
    }
}

#endif
