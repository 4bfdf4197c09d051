// read_window.h -- sliding-window quality cuts on the device before the reads are packed (mlst_set_read_window; the rule: include/mlst.h,
// stated on the host as metamlst_amd.fastq.window_cut / cut_windows; `cli type --cut-front / --cut-right / --cut-tail`).  Included by
// mlst_engine.hip behind read_filter.h (rf_load16).  The rule is modelled on fastp's cut_front / cut_right / cut_tail (Trimmomatic's
// LEADING / SLIDINGWINDOW / TRAILING); it is the project's own and claims neither tool's bytes.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records; read_prep.h).  A front cut
// moves both offsets, every cut lowers the length:
//   k_rw_cut      a thread per read, directly behind k_rp_qtrim and in front of k_ra_cut.  Per operation the window sum is kept as
//                 sum += q[i + w] - q[i], sixteen steps per turn: the leading chunk and the chunk w bytes behind it are each one 16-byte
//                 load (rf_load16: whole where the 16 bytes lie inside the region, byte by byte at its edges, so no byte in front of the
//                 quality line or behind its end is touched), unrolled over their bytes with constant indices -- no ring of the last w
//                 values is kept.  front walks up from the 5' end and tail down from the 3' end, each leaving at its first passing
//                 window; right is the one full pass, up from front's cut to its first failing window, of which the leading values
//                 >= Q stay.  It adds front's cut to seq_off[r] and qual_off[r] (an emptied read's offsets are not observable and stay),
//                 writes lens[r], feeds the longest length it leaves into the parser's flags[0] (zeroed in front of it) and adds its
//                 eight counters, a wave together, into a block of its own.  The Phred base is a value (mlst_set_read_prep's), clamped
//                 as k_rp_qtrim clamps it.
// A chunk the parser flagged malformed is not walked.  Plain vector stores and ordinary atomics only.  No read-back, no host
// synchronisation.
#ifndef MLST_READ_WINDOW_H
#define MLST_READ_WINDOW_H

#define RW_MAX_W 320      // (MLST_MAX_READ_LEN: a wider window would be the whole read all the same)
#define RW_NONE 0xFFFFFFFFu

struct RwSet { u32 front_w, front_q, right_w, right_q, tail_w, tail_q; };      // mlst_read_window (w = 0: that operation is off)
struct RwCtr {          // device-resident counters (a block of their own), in the order of mlst_read_window_info
    u64 shortened;      // reads whose length changed
    u64 front_reads, front_bases;      // reads cut by front, and the bases it removed (all n of a read it emptied)
    u64 right_reads, right_bases;
    u64 tail_reads, tail_bases;
    u64 emptied;        // reads of length >= 1 left without a base
};

// byte k (constant) of a chunk rf_load16 filled, as a Phred value: clamp(character - base, 0, 127)
__device__ inline int rw_val(const u64 (&c8)[2], int k, int base) {
    const int v = (int)((u32)(c8[k >> 3] >> (8 * (k & 7))) & 0xFFu) - base;
    return v < 0 ? 0 : (v > 127 ? 127 : v);
}

// the sum of the values [a, b) of the m-byte region at p (0 <= a <= b <= m)
__device__ inline int rw_sum(const u8* __restrict__ p, int a, int b, int m, int base) {
    int s = 0;
    for (int lo = a; lo < b; lo += 16) {
        u64 c8[2];
        rf_load16(p, lo, m, c8);
        #pragma unroll
        for (int k = 0; k < 16; k++) if (lo + k < b) s += rw_val(c8, k, base);
    }
    return s;
}

// Windows of w values walked up the m-byte region at p (1 <= w <= m): the smallest s in [0, m - w] whose window [s, s + w) passes
// (PASS: sum >= thr) or fails (!PASS: sum < thr), RW_NONE if there is none
template <bool PASS> __device__ inline u32 rw_first_up(const u8* __restrict__ p, int m, int w, int thr, int base) {
    int sum = rw_sum(p, 0, w, m, base);
    if ((sum >= thr) == PASS) return 0u;
    u32 found = RW_NONE;
    for (int i = 0; i + w < m && found == RW_NONE; i += 16) {      // the windows i + 1 .. i + 16
        u64 lead[2], lag[2];
        rf_load16(p, i + w, m, lead);
        rf_load16(p, i, m, lag);
        #pragma unroll
        for (int k = 0; k < 16; k++) {
            if (i + k + w < m && found == RW_NONE) {
                sum += rw_val(lead, k, base) - rw_val(lag, k, base);
                if ((sum >= thr) == PASS) found = (u32)(i + k + 1);
            }
        }
    }
    return found;
}

// Windows of w values walked down the m-byte region at p (1 <= w <= m): the largest t in [w, m] whose window [t - w, t) passes, 0 if
// there is none
__device__ inline u32 rw_last_down(const u8* __restrict__ p, int m, int w, int thr, int base) {
    int sum = rw_sum(p, m - w, m, m, base);
    if (sum >= thr) return (u32)m;
    u32 found = RW_NONE;
    for (int hi = m; hi - w > 0 && found == RW_NONE; hi -= 16) {      // the windows that end at hi - 1 .. hi - 16
        u64 lead[2], lag[2];
        rf_load16(p, hi - 16, m, lead);          // the values that leave the window: byte idx
        rf_load16(p, hi - 16 - w, m, lag);       // ... and those that enter it: byte idx - w
        #pragma unroll
        for (int k = 15; k >= 0; k--) {
            const int idx = hi - 16 + k;
            if (idx - w >= 0 && found == RW_NONE) {
                sum += rw_val(lag, k, base) - rw_val(lead, k, base);
                if (sum >= thr) found = (u32)idx;
            }
        }
    }
    return found == RW_NONE ? 0u : found;
}

__global__ __launch_bounds__(256) void k_rw_cut(const u8* __restrict__ text, u64* __restrict__ seq_off, u64* __restrict__ qual_off, u16* __restrict__ lens, u64 n_reads, RwSet S,
                                                 u32 phred_base, u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */, RwCtr* __restrict__ C) {
    if (longest[1]) return;      // (as in k_rp_qtrim: the host refuses the chunk behind this kernel)
    const int base = (int)phred_base;
    u32 mx = 0, n_short = 0, n_empty = 0, n_fr = 0, n_fb = 0, n_rr = 0, n_rb = 0, n_tr = 0, n_tb = 0;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u32 n = (u32)(lens[r] & 0x7FFFu);      // plain lengths on entry (at most MLST_MAX_READ_LEN)
        const u64 qo = qual_off[r];
        const u8* const q = text + qo;
        u32 f = 0, e = n;
        if (S.front_w && n) {
            const u32 w = S.front_w < n ? S.front_w : n;
            const u32 s = rw_first_up<true>(q, (int)n, (int)w, (int)(S.front_q * w), base);
            f = s == RW_NONE ? n : s;
            if (f) { n_fr++; n_fb += f; }
        }
        if (S.right_w && n > f) {
            const u32 m = n - f, w = S.right_w < m ? S.right_w : m;
            const u32 s = rw_first_up<false>(q + f, (int)m, (int)w, (int)(S.right_q * w), base);
            if (s != RW_NONE) {
                u32 k = 0;      // the leading values of the failing window that are >= Q stay (one of the w is below it)
                #pragma unroll 1
                while (k + 1 < w) { int v = (int)q[f + s + k] - base; v = v < 0 ? 0 : (v > 127 ? 127 : v); if (v < (int)S.right_q) break; k++; }
                e = f + s + k;
                n_rr++; n_rb += n - e;
            }
        }
        if (S.tail_w && e > f) {
            const u32 m = e - f, w = S.tail_w < m ? S.tail_w : m;
            const u32 t = rw_last_down(q + f, (int)m, (int)w, (int)(S.tail_q * w), base);
            if (t != m) { n_tr++; n_tb += m - t; }
            e = f + t;
        }
        const u32 n2 = e - f;
        if (f && n2) { seq_off[r] += f; qual_off[r] = qo + f; }
        if (n2 != n) { lens[r] = (u16)n2; n_short++; if (!n2) n_empty++; }
        if (n2 > mx) mx = n2;
    }
    // one wave reduction, then one atomic per wave and counter
    n_short = wave_sum_u32(n_short); n_empty = wave_sum_u32(n_empty); n_fr = wave_sum_u32(n_fr); n_fb = wave_sum_u32(n_fb);
    n_rr = wave_sum_u32(n_rr); n_rb = wave_sum_u32(n_rb); n_tr = wave_sum_u32(n_tr); n_tb = wave_sum_u32(n_tb);
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(mx, o); mx = x > mx ? x : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(longest, mx);
        if (n_short) atomicAdd((unsigned long long*)&C->shortened, (unsigned long long)n_short);
        if (n_fr) atomicAdd((unsigned long long*)&C->front_reads, (unsigned long long)n_fr);
        if (n_fb) atomicAdd((unsigned long long*)&C->front_bases, (unsigned long long)n_fb);
        if (n_rr) atomicAdd((unsigned long long*)&C->right_reads, (unsigned long long)n_rr);
        if (n_rb) atomicAdd((unsigned long long*)&C->right_bases, (unsigned long long)n_rb);
        if (n_tr) atomicAdd((unsigned long long*)&C->tail_reads, (unsigned long long)n_tr);
        if (n_tb) atomicAdd((unsigned long long*)&C->tail_bases, (unsigned long long)n_tb);
        if (n_empty) atomicAdd((unsigned long long*)&C->emptied, (unsigned long long)n_empty);
    }
}

#endif
