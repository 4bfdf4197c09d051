// msa_dev.h -- centre-star alignment of a locus' alleles on the device (mlst_msa_align / mlst_msa_fetch; the rule: include/mlst.h,
// stated in Python by metamlst_amd/msa.py).  Included by mlst_engine.hip behind the DPP helpers.
//
// k_msa_dp     one wave per (sequence b, centre a) pair, up to MSA_WPB pairs per workgroup (as many as 48 KiB of row buffers allow).
//              The centre is cut into stripes of 64 columns: lane l owns column j = 64 k + l + 1 of stripe k and meets row i = t - l at step t, so the cells of one step lie on an
//              anti-diagonal and depend on nothing of the same step.  What a cell needs from its left neighbour comes as two packed
//              words by a DPP lane shift: H = max(M, I, D) of the neighbour's cell (the diagonal of the next step) and the D of this
//              cell, max(M - 11, D - 1, I - 11) taken over there.  A packed word is value * 4 + tag, tag 3 / 2 / 1 for the first /
//              second / third candidate of its max: one signed max over packed words picks the value and lets the first listed
//              candidate win ties.  Lane 0 takes the two words of the stripe's left border from an LDS row buffer (8 bytes per row and
//              wave) that lane 63 fills for the next stripe, in place: row i is read at step i and written at step i + 63.  The
//              letter of b moves along the lanes with the cells; lane 0 takes it from a register chunk of 64 letters.
//              Traceback: one byte per cell -- tag of M's max | tag of I's << 2 | tag of D's << 4 (I and D choose among three
//              sources each, which two bits apiece hold and one bit would not: an insertion directly followed by a deletion is
//              optimal once both are longer than five bases) -- packed per lane into words of four steps and stored by step, not by
//              row, so that a store is one coalesced 256 bytes per wave: cell (i, j) is byte (t & 3) of word
//              ((k * T4 + (t >> 2)) * 64 + l), t = i + l.  Plain vector stores only.
// k_msa_trace  one lane per pair walks the at most n + m steps from [n][m] and writes, per centre column, the 1-based index of the
//              base of b on it (0: none) and, per slot, start and length of the insertion; the slot widths take an atomicMax.
// k_msa_scan   one workgroup: where every slot starts in a row (exclusive sum of width + 1), and the row width.
// k_msa_rows   one thread per output byte.
#pragma once

#define MSA_WPB 4                      // most waves (pairs) per workgroup of k_msa_dp
#define MSA_NEG (-(1 << 28))
#define MSA_OPEN (MLST_MSA_GAP_OPEN + MLST_MSA_GAP_EXT)

struct MsaDev {
    const u8* seq; const u64* off;     // the sequences, back to back
    u32 n, center, m, nmax;            // sequences, index and length of the centre, longest sequence
    u16* col; u16* ins_start; u16* ins_len;      // [n][m + 1]: per centre column 1..m the base on it (1-based, 0 none); per slot 0..m the insertion
    u32* slot_w; u32* slot_at;         // [m + 1]: widest insertion of a slot, where the slot starts in a row
    u8* end_state;                     // [n]: the state the traceback starts in (0 M, 1 I, 2 D)
    u32* tb; u64 tb_words; u32 T4;     // traceback words of a batch: tb_words per pair, T4 words per stripe and lane
    u32* width;                        // the row width (one word)
};

__device__ __forceinline__ int msa_max3(int a, int b, int c) { const int x = a > b ? a : b; return x > c ? x : c; }
// A C G T in either case: 0..3; anything else `other` (4 on the centre's side, 5 on the sequence's: it matches nothing, itself included)
__device__ __forceinline__ int msa_code(u8 c, int other) {
    c &= 0xDF;
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : other;
}
__device__ __forceinline__ void msa_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

__global__ __launch_bounds__(64 * MSA_WPB) void k_msa_dp(MsaDev A, u32 r0, u32 r1) {
    extern __shared__ int2 msa_border[];
    const u32 lane = threadIdx.x & 63, wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 r = r0 + blockIdx.x * (blockDim.x >> 6) + wv;
    if (r >= r1 || r == A.center) return;      // (whole waves leave; the kernel has no workgroup barrier)
    int2* const bord = msa_border + (u64)wv * (A.nmax + 1);
    const u8* const a = A.seq + A.off[A.center]; const u32 m = A.m;
    const u8* const b = A.seq + A.off[r]; const u32 n = (u32)(A.off[r + 1] - A.off[r]);
    u32* const tb = A.tb + (u64)(r - r0) * A.tb_words;
    // column 0: M and D are NEG there, so H is I = -(10 + i) (second of M, I, D) and the D of column 1 opens from I (third of M, D, I)
    for (u32 i = 1 + lane; i <= n; i += 64) {
        const int v = -(MLST_MSA_GAP_OPEN + MLST_MSA_GAP_EXT * (int)i);
        bord[i] = make_int2(v * 4 + 2, (v - MSA_OPEN) * 4 + 1);
    }
    msa_wave_sync();
    const u32 steps = n + 63, stripes = (m + 63) / 64;
    for (u32 k = 0; k < stripes; k++) {
        const u32 j = k * 64 + lane + 1;
        const bool has_col = j <= m;
        const int ac = has_col ? msa_code(a[j - 1], 4) : 4;
        // row 0: M and I are NEG, D = -(10 + j); the diagonal of row 1 is H of (0, j - 1): M = 0 at the corner, else D (third)
        int Mp = MSA_NEG, Ip = MSA_NEG, Dp = -(MLST_MSA_GAP_OPEN + MLST_MSA_GAP_EXT * (int)j);
        int diag = j == 1 ? 3 : -(MLST_MSA_GAP_OPEN + MLST_MSA_GAP_EXT * (int)(j - 1)) * 4 + 1;
        int outH = 0, outD = 0, bc = 5, bchunk = 5;
        u32 word = 0;
        for (u32 t = 1; t <= steps; t++) {
            if (((t - 1) & 63) == 0) { const u32 x = t - 1 + lane; bchunk = x < n ? msa_code(b[x], 5) : 5; }
            const int b0 = __builtin_amdgcn_readlane(bchunk, (int)((t - 1) & 63));      // the letter of row t, for lane 0
            const int2 bd = bord[t <= n ? t : 0];
            const int inH = dpp_i32<DPP_WAVE_SHR1>(bd.x, outH);      // H of (i, j - 1): the diagonal of the next step
            const int inD = dpp_i32<DPP_WAVE_SHR1>(bd.y, outD);      // D of (i, j), packed
            bc = dpp_i32<DPP_WAVE_SHR1>(b0, bc);
            const int i = (int)t - (int)lane;
            u32 cell = 0;
            if (has_col && i >= 1 && i <= (int)n) {
                const int Mv = (bc == ac ? MLST_MSA_MATCH : MLST_MSA_MISMATCH) + (diag >> 2);
                const int I4 = msa_max3((Mp - MSA_OPEN) * 4 + 3, (Ip - MLST_MSA_GAP_EXT) * 4 + 2, (Dp - MSA_OPEN) * 4 + 1);
                const int Iv = I4 >> 2, Dv = inD >> 2;
                cell = (u32)(diag & 3) | (u32)(I4 & 3) << 2 | (u32)(inD & 3) << 4;
                outH = msa_max3(Mv * 4 + 3, Iv * 4 + 2, Dv * 4 + 1);
                outD = msa_max3((Mv - MSA_OPEN) * 4 + 3, (Dv - MLST_MSA_GAP_EXT) * 4 + 2, (Iv - MSA_OPEN) * 4 + 1);
                Mp = Mv; Ip = Iv; Dp = Dv; diag = inH;
                if (lane == 63) bord[i] = make_int2(outH, outD);      // the left border of the next stripe
                if (i == (int)n && j == m) A.end_state[r] = (u8)(3 - (outH & 3));
            }
            word |= cell << ((t & 3) * 8);
            if ((t & 3) == 3) { tb[((u64)k * A.T4 + (t >> 2)) * 64 + lane] = word; word = 0; }
        }
        if ((steps & 3) != 3) tb[((u64)k * A.T4 + (steps >> 2)) * 64 + lane] = word;
        msa_wave_sync();
    }
}

__global__ __launch_bounds__(64) void k_msa_trace(MsaDev A, u32 r0, u32 r1) {
    const u32 r = r0 + blockIdx.x * 64 + threadIdx.x;
    if (r >= r1) return;
    const u32 m = A.m;
    u16* const col = A.col + (u64)r * (m + 1); u16* const ins_start = A.ins_start + (u64)r * (m + 1); u16* const ins_len = A.ins_len + (u64)r * (m + 1);
    if (r == A.center) { for (u32 j = 1; j <= m; j++) col[j] = (u16)j; return; }
    const u8* const tb = (const u8*)(A.tb + (u64)(r - r0) * A.tb_words);
    u32 i = (u32)(A.off[r + 1] - A.off[r]), j = m, state = A.end_state[r], run = 0;
    while (i | j) {
        if (i == 0) state = 2; else if (j == 0) state = 1;      // on the border only one state is real
        u32 cell = 0;
        if (i && j) { const u32 l = (j - 1) & 63, t = i + l; cell = tb[(((u64)((j - 1) >> 6) * A.T4 + (t >> 2)) * 64 + l) * 4 + (t & 3)]; }
        if (state == 0) { col[j] = (u16)i; state = 3 - (cell & 3); i--; j--; }
        else if (state == 1) {
            run++; i--;
            state = j ? 3 - (cell >> 2 & 3) : 1;
            if (i == 0 || state != 1) { ins_start[j] = (u16)i; ins_len[j] = (u16)run; atomicMax(&A.slot_w[j], run); run = 0; }
        } else { const u32 tag = cell >> 4 & 3; col[j] = 0; state = i ? (tag == 3 ? 0 : tag) : 2; j--; }      // (M, D, I) -> tags 3, 2, 1
    }
}

__global__ __launch_bounds__(1024) void k_msa_scan(MsaDev A) {
    __shared__ u32 part[1024];
    const u32 t = threadIdx.x;
    u32 v[4], s = 0;
    for (u32 q = 0; q < 4; q++) { const u32 k = t * 4 + q; v[q] = k <= A.m ? A.slot_w[k] + 1 : 0; s += v[q]; }      // a slot and the column behind it
    part[t] = s;
    __syncthreads();
    for (u32 o = 1; o < 1024; o <<= 1) {
        const u32 y = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    u32 at = part[t] - s;
    for (u32 q = 0; q < 4; q++) { const u32 k = t * 4 + q; if (k <= A.m) { A.slot_at[k] = at; at += v[q]; } }
    if (t == 1023) *A.width = part[1023] - 1;      // (no column behind the last slot)
}

__global__ __launch_bounds__(256) void k_msa_rows(MsaDev A, u32 width, u8* __restrict__ rows) {
    const u64 total = (u64)A.n * width;
    for (u64 x = (u64)blockIdx.x * 256 + threadIdx.x; x < total; x += (u64)gridDim.x * 256) {
        const u32 r = (u32)(x / width), p = (u32)(x % width);
        u32 lo = 0, hi = A.m;      // the last slot that starts at or before p
        while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (A.slot_at[mid] <= p) lo = mid; else hi = mid - 1; }
        const u32 k = lo, at = p - A.slot_at[k];
        const u8* const b = A.seq + A.off[r];
        const u64 e = (u64)r * (A.m + 1);
        u8 c = '-';
        if (at < A.slot_w[k]) { if (at < A.ins_len[e + k]) c = b[A.ins_start[e + k] + at]; }
        else { const u32 i = A.col[e + k + 1]; if (i) c = b[i - 1]; }
        rows[x] = c;
    }
}
