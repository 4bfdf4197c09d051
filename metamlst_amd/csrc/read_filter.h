// read_filter.h -- poly-G / poly-X tails trimmed and reads filtered on the device before they are packed (mlst_set_read_filter; the rule:
// include/mlst.h, stated on the host as metamlst_amd.fastq.poly_tail / read_fails / filter_fastq; `cli type --trim-poly-g / --trim-poly-x /
// --min-length / --max-n / --low-complexity / --min-mean-qual`).  Included by mlst_engine.hip next to read_overlap.h.  The rule is modelled
// on fastp's --trim_poly_g / --trim_poly_x and its length, N, complexity and quality filters; it is the project's own and claims none of
// fastp's bytes.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records; read_prep.h).  Trimming a
// tail lowers the length, and a read that fails a filter gets the length 0:
//   k_rf_filter   a thread per read, behind k_po_cut (and whatever of the chain ran in front of it), in front of the prepared statistics,
//                 of duplicate removal and of the read-back of the parser's flags.  It reads seq_off[r], qual_off[r] and lens[r] and
//                 writes lens[r] only.
//                 1. The tail (poly_mask != 0).  The bases are walked from the 3' end down in 16-byte steps (loaded as rp_qtrim_len loads
//                    them), a mismatch counter per letter in registers.  A tail of length L of letter X is valid if L >= poly_min, the
//                    base it begins on is X and at most min(5, L / 8) of its bases are not X; the walk meets the lengths in ascending
//                    order, so the last valid one it sees is the cut, and it ends when every letter of the mask has met its sixth
//                    mismatch (a random read: about eight bases per letter, inside the first load).
//                 2. The filters on what the tail trim left.  min_length alone touches no text.  The N count, the adjacent-difference
//                    count and the quality sum take one pass over the read's sequence and quality bytes from the 5' end, 16 bytes per
//                    load and line; which of the two lines is loaded is the same for every thread (the setting).
//                 The kernel feeds the longest length it leaves into the parser's flags[0] (zeroed in front of it) and adds its twelve
//                 counters, a wave together, into a block of its own.  The Phred base is a value (mlst_set_read_prep's), clamped as
//                 k_rp_qtrim clamps it.
// A chunk the parser flagged malformed is not walked.  Plain vector stores and ordinary atomics only.  No read-back, no host
// synchronisation.
#ifndef MLST_READ_FILTER_H
#define MLST_READ_FILTER_H

#define RF_NO_LIMIT 0xFFFFFFFFu      // MLST_RF_NO_LIMIT
#define RF_MAX_LEN 320               // (MLST_MAX_READ_LEN: poly_min and min_length beyond it would say nothing)

struct RfSet { u32 poly_mask, poly_min, min_length, max_n, complexity_pct, mean_qual; };      // mlst_read_filter
struct RfCtr {          // device-resident counters (a block of their own), in the order of mlst_read_filter_info
    u64 tail_trimmed;   // reads whose tail was cut
    u64 tail_bases;     // bases removed with the tails
    u64 per_letter[4];  // reads cut, by the tail's letter (A, C, G, T)
    u64 tail_emptied;   // reads of length >= 1 that were one tail
    u64 failed[4];      // reads emptied by a filter: too short, too many N, low complexity, low quality
    u64 filtered_bases; // bases those reads held behind the tail trim
    u64 pad_[4];
};

// a byte as the engine aligns it: A 0, C 1, G 2, T 3 in either case, 4 = every other byte
__device__ inline u32 rf_code(u32 b) {
    const u32 f = b & 0xDFu;
    return f == 'A' ? 0u : f == 'C' ? 1u : f == 'G' ? 2u : f == 'T' ? 3u : 4u;
}

// sixteen bytes [lo, lo + 16) of the n-byte line at t into c8 (byte lo + k at bits 8 (k & 7) of c8[k >> 3]); bytes outside [0, n) are 0
// and are not loaded.  Constant indices only
__device__ inline void rf_load16(const u8* __restrict__ t, int lo, int n, u64 (&c8)[2]) {
    c8[0] = 0; c8[1] = 0;
    if (lo >= 0 && lo + 16 <= n) { __builtin_memcpy(c8, t + lo, 16); return; }      // (the compiler picks the widest loads the target allows unaligned)
    const int a = lo < 0 ? 0 : lo, b = lo + 16 < n ? lo + 16 : n;
    #pragma unroll 1
    for (int i = a; i < b; i++) { const u64 v = t[i]; const int k = i - lo; if (k < 8) c8[0] |= v << (8 * k); else c8[1] |= v << (8 * (k - 8)); }
}

// The tail of the n-base read at t: the new length, and the tail's letter in `letter` (untouched when nothing is cut).  mask: the letters
// looked for (bits 0..3 = A, C, G, T, not 0)
__device__ inline u32 rf_tail_len(const u8* __restrict__ t, u32 n, u32 mask, u32 poly_min, u32& letter) {
    u32 mm[4] = {0, 0, 0, 0};      // mismatches per letter so far (constant indices only: registers); 6 = the letter is out
    #pragma unroll
    for (int x = 0; x < 4; x++) if (!((mask >> x) & 1u)) mm[x] = 6;
    u32 best = 0;
    for (int end = (int)n; end > 0; end -= 16) {
        if (mm[0] > 5 && mm[1] > 5 && mm[2] > 5 && mm[3] > 5) break;
        const int lo = end - 16;
        u64 c8[2];
        rf_load16(t, lo, (int)n, c8);
        #pragma unroll
        for (int k = 15; k >= 0; k--) {
            const int i = lo + k;
            if (i >= 0) {
                const u32 c = rf_code((u32)(c8[k >> 3] >> (8 * (k & 7))) & 0xFFu);
                const u32 L = n - (u32)i, budget = (L >> 3) < 5u ? (L >> 3) : 5u;
                #pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (mm[x] <= 5) {
                        if (c != (u32)x) mm[x]++;
                        else if (L >= poly_min && mm[x] <= budget) { best = L; letter = (u32)x; }
                    }
                }
            }
        }
    }
    return n - best;
}

__global__ __launch_bounds__(256) void k_rf_filter(const u8* __restrict__ text, const u64* __restrict__ seq_off, const u64* __restrict__ qual_off, u16* __restrict__ lens,
                                                    u64 n_reads, RfSet S, u32 phred_base, u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */,
                                                    RfCtr* __restrict__ C) {
    if (longest[1]) return;      // (as in k_rp_qtrim: the host refuses the chunk behind this kernel)
    const bool need_seq = S.max_n != RF_NO_LIMIT || S.complexity_pct != 0, need_qual = S.mean_qual != 0;      // (the same for every thread)
    u32 mx = 0, n_tail = 0, n_tail_bases = 0, n_tail_empty = 0, n_fbases = 0;
    u32 pl[4] = {0, 0, 0, 0}, nf[4] = {0, 0, 0, 0};      // (constant indices only: registers)
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u32 n = (u32)(lens[r] & 0x7FFFu);      // plain lengths on entry (at most MLST_MAX_READ_LEN)
        const u8* const t = text + seq_off[r];
        u32 n2 = n;
        if (S.poly_mask && n >= S.poly_min) {
            u32 letter = 0;
            n2 = rf_tail_len(t, n, S.poly_mask, S.poly_min, letter);
            if (n2 != n) {
                n_tail++; n_tail_bases += n - n2; if (!n2) n_tail_empty++;
                #pragma unroll
                for (u32 x = 0; x < 4; x++) pl[x] += letter == x ? 1u : 0u;
            }
        }
        u32 why = 0;      // 1..4: the first filter the read fails
        if (n2) {
            if (n2 < S.min_length) why = 1;
            else if (need_seq || need_qual) {
                const u8* const q = text + qual_off[r];
                u32 n_n = 0, d = 0, qsum = 0, prev = 0;
                for (int lo = 0; lo < (int)n2; lo += 16) {
                    u64 c8[2];
                    if (need_seq) {
                        rf_load16(t, lo, (int)n2, c8);
                        #pragma unroll
                        for (int k = 0; k < 16; k++) {
                            if (lo + k < (int)n2) {
                                const u32 c = rf_code((u32)(c8[k >> 3] >> (8 * (k & 7))) & 0xFFu);
                                n_n += c == 4u ? 1u : 0u;
                                d += (lo + k > 0 && c != prev) ? 1u : 0u;
                                prev = c;
                            }
                        }
                    }
                    if (need_qual) {
                        rf_load16(q, lo, (int)n2, c8);
                        #pragma unroll
                        for (int k = 0; k < 16; k++) {
                            if (lo + k < (int)n2) {
                                int v = (int)((u32)(c8[k >> 3] >> (8 * (k & 7))) & 0xFFu) - (int)phred_base; v = v < 0 ? 0 : (v > 127 ? 127 : v);
                                qsum += (u32)v;
                            }
                        }
                    }
                }
                if (S.max_n != RF_NO_LIMIT && n_n > S.max_n) why = 2;
                else if (S.complexity_pct && n2 >= 2 && 100u * d < S.complexity_pct * (n2 - 1)) why = 3;
                else if (need_qual && qsum < S.mean_qual * n2) why = 4;
            }
        }
        if (why) { n_fbases += n2; n2 = 0; }
        #pragma unroll
        for (u32 x = 0; x < 4; x++) nf[x] += why == x + 1 ? 1u : 0u;
        if (n2 != n) lens[r] = (u16)n2;
        if (n2 > mx) mx = n2;
    }
    // one wave reduction, then one atomic per wave and counter
    n_tail = wave_sum_u32(n_tail); n_tail_bases = wave_sum_u32(n_tail_bases); n_tail_empty = wave_sum_u32(n_tail_empty); n_fbases = wave_sum_u32(n_fbases);
    #pragma unroll
    for (int x = 0; x < 4; x++) { pl[x] = wave_sum_u32(pl[x]); nf[x] = wave_sum_u32(nf[x]); }
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(mx, o); mx = x > mx ? x : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(longest, mx);
        if (n_tail) atomicAdd((unsigned long long*)&C->tail_trimmed, (unsigned long long)n_tail);
        if (n_tail_bases) atomicAdd((unsigned long long*)&C->tail_bases, (unsigned long long)n_tail_bases);
        if (n_tail_empty) atomicAdd((unsigned long long*)&C->tail_emptied, (unsigned long long)n_tail_empty);
        if (n_fbases) atomicAdd((unsigned long long*)&C->filtered_bases, (unsigned long long)n_fbases);
        #pragma unroll
        for (int x = 0; x < 4; x++) {
            if (pl[x]) atomicAdd((unsigned long long*)&C->per_letter[x], (unsigned long long)pl[x]);
            if (nf[x]) atomicAdd((unsigned long long*)&C->failed[x], (unsigned long long)nf[x]);
        }
    }
}

#endif
