// fastq_tile.h -- FASTQ records longer than the tile cut into windows on the device (included by mlst_engine.hip behind
// fasta_dev.h; switch: mlst_set_read_tiling; the rule: include/mlst.h, stated on the host as metamlst_amd.fastq.tile_fastq).
//
// fastq_pipeline's parser has left the line table and, per record, where its sequence and quality lines start (k_fq_records in
// its tiling mode, which reports "a record longer than the tile is present" instead of failing it).  Only a chunk with such a
// record comes here:
//   k_fqt_count : a thread per record, a workgroup per FQT_GROUP records: the record's length from the line table in 64 bits
//                 (fq_record_span, the code k_fq_records runs), its windows (fa_windows_of with min_len 0), the windows of the
//                 workgroup's records in front of it, and the workgroup's sum
//   k_fqt_scan  : one workgroup: exclusive prefix sums of the workgroups' sums, the total
//   k_fqt_add   : the workgroup's base added: per record the global index of its first window
//   k_fqt_emit  : a thread per window of a round [w0, w1): its record by binary search in that table (every record has at least one
//                 window, so the table rises strictly), then seq_off / qual_off / lens as k_fq_records leaves them for k_pack_text
// A window is a sequence offset, a quality offset -- both moved by the window's start -- and a length: k_pack_text packs it
// from the chunk's text like any record and finds the window's own N bit.
// All offsets, lengths and window indices are 64-bit.  Descriptor fields are read through GP<> (address space 1).
#ifndef MLST_FASTQ_TILE_H
#define MLST_FASTQ_TILE_H

#define FQT_GROUP 1024u      /* records per workgroup of k_fqt_count / k_fqt_add: one per thread */

struct FqtMeta {            // device-resident results of a chunk (zeroed per chunk)
    u64 n_windows;          // windows plus uncut records: the reads of the chunk
    u64 n_cut;              // records longer than read_len
    u64 max_rec;            // bases of the longest record
    u32 max_len, pad_;      // the longest read
};
struct FqtDev {             // device-resident descriptor (uploaded per chunk)
    GP<const u8> text;      // the chunk's text
    GP<const u64> lines;    // line table (k_fq_lines)
    GP<const u64> rs, rq;   // per record: start of its sequence / quality line (k_fq_records)
    GP<u64> rlen;           // per record: bases
    GP<u64> wex;            // per record: windows in front of it (in its workgroup, then in the chunk)
    GP<u64> gsum;           // per workgroup: its windows, then (in place) the windows in front of it
    GP<FqtMeta> meta;
    u64 n_bytes, n_lines, n_recs;
    u32 read_len, stride;
};

// inclusive prefix sum over the wave (64-bit values have no DPP row operations: shuffles)
__device__ inline u64 fqt_wave_incl(u64 v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { const u64 y = __shfl_up(v, o); if (lane >= o) v += y; }
    return v;
}

__global__ __launch_bounds__(1024) void k_fqt_count(const FqtDev* __restrict__ Dp) {
    __shared__ u64 s_w[16]; __shared__ u32 s_cut[16];
    const FqtDev& D = *Dp;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 r = (u64)blockIdx.x * FQT_GROUP + threadIdx.x;
    u64 n = 0, w = 0; u32 cut = 0;
    if (r < D.n_recs) {
        u64 s0, q0, lq;
        fq_record_span(D.text.g(), D.n_bytes, D.lines.g(), D.n_lines, r, s0, q0, n, lq);
        w = fa_windows_of(n, D.read_len, D.stride, 0u);
        cut = n > (u64)D.read_len ? 1u : 0u;
        D.rlen[r] = n;
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

// One workgroup of 1024 threads, 1024 workgroup sums per turn (a chunk of 5 M records has 5 K of them).
__global__ __launch_bounds__(1024) void k_fqt_scan(const FqtDev* __restrict__ Dp, u64 n_groups) {
    __shared__ u64 s_w[16]; __shared__ u64 s_carry;
    const FqtDev& D = *Dp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u64 i0 = 0; i0 < n_groups; i0 += 1024u) {
        const u64 i = i0 + tid;
        const u64 v = i < n_groups ? D.gsum[i] : 0ull;
        const u64 inc = fqt_wave_incl(v);
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        u64 before = s_carry, all = 0;
        for (int k = 0; k < 16; k++) { const u64 x = s_w[k]; if (k < wv) before += x; all += x; }
        if (i < n_groups) D.gsum[i] = before + inc - v;
        __syncthreads();
        if (tid == 0) s_carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        D.meta->n_windows = s_carry;
        const u64 mr = D.meta->max_rec;      // (k_fqt_count has finished: same stream)
        D.meta->max_len = mr < (u64)D.read_len ? (u32)mr : D.read_len;
    }
}

__global__ __launch_bounds__(1024) void k_fqt_add(const FqtDev* __restrict__ Dp) {
    const FqtDev& D = *Dp;
    const u64 r = (u64)blockIdx.x * FQT_GROUP + threadIdx.x;
    if (r < D.n_recs) D.wex[r] += D.gsum[blockIdx.x];
}

// One thread per window of [w0, w1): entry w - w0 of seq_off / qual_off / lens (three coalesced stores per wave: 512 + 512 + 128 bytes).
__global__ __launch_bounds__(256) void k_fqt_emit(const FqtDev* __restrict__ Dp, u64 w0, u64 w1, u64* __restrict__ seq_off, u64* __restrict__ qual_off, u16* __restrict__ lens) {
    const FqtDev& D = *Dp;
    const u64 nr = D.n_recs; const u32 L = D.read_len, S = D.stride;
    for (u64 w = w0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; w < w1; w += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = nr;      // the last record with wex[r] <= w
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (D.wex[mid] <= w) lo = mid + 1; else hi = mid; }
        const u64 r = lo - 1;     // (wex[0] = 0 <= w)
        const u64 n = D.rlen[r];
        u64 st = 0; u32 len = (u32)n;
        if (n > (u64)L) { st = (w - D.wex[r]) * S; if (st > n - L) st = n - L; len = L; }
        const u64 o = w - w0;
        seq_off[o] = D.rs[r] + st; qual_off[o] = D.rq[r] + st; lens[o] = (u16)len;
    }
}

#endif
