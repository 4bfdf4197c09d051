// read_overlap.h -- adapter read-through trimmed from the overlap of the two mates, on the device before the reads are packed
// (mlst_set_read_pair_overlap; the rule: include/mlst.h, stated on the host as metamlst_amd.fastq.pair_overlap / trim_pair_overlap;
// `cli type -2 MATES --pair-overlap`).  Included by mlst_engine.hip next to read_dedup.h.  The rule is modelled on fastp's overlap
// analysis (no indels); it is the project's own and claims none of fastp's bytes.
//
// In a paired submission the mates of pair u are reads 2 u and 2 u + 1 of one text buffer: a sequence offset, a quality offset and a
// length each (k_fq_records, k_fq_pair_records; read_prep.h).  Cutting the read-through only lowers the two lengths:
//   k_po_cut      a WAVE per pair, its lanes the candidate offsets.  Chosen over a thread per pair because that shape keeps 4 x 10
//                 64-bit words of a pair in registers (indexed at run time, so in scratch, or unrolled over ten words for every length),
//                 and diverges on unequal lengths; here a pair's words sit in LDS once and 64 offsets are looked at per instruction,
//                 all of them of one pair, so the loop bounds are the wave's.
//                 1. Lanes 0-9 convert mate 1, thirty-two bases each (two ra_chunk), into 2-bit codes and an "is ACGT" mask of the same
//                    spacing (bit 2 i for base i); lanes 32-41 convert mate 2 likewise and store its reverse complement: the complement
//                    of a code is its bitwise NOT, the reverse is a reversal of the 2-bit groups of a word and of the word order.  The
//                    reversed string R starts with pad = 32 W2 - n2 positions that are no ACGT (W2 words hold mate 2), so letter j of
//                    the reverse complement is R[pad + j]; a zero word stands in front of R and zero words behind it.
//                 2. Lane l takes offset o = o0 + l (64 per round; 241 offsets of a 150 / 150 pair are four rounds) and walks the words of
//                    mate 1 that its overlap touches: the two neighbouring words of R funnel-shifted to the word of mate 1, XOR, fold of
//                    the two bits of a code, AND of both masks, popcount.  Bases outside the overlap meet a zero mask on one side, so
//                    the overlap's length is plain arithmetic.  The lanes of a round read at most three neighbouring words of either
//                    string per instruction: ds_read_b64 without a bank conflict.
//                 3. A wave max over (matches, -o) picks the valid candidate with the most matches, the smallest o among equals.  Lane 0
//                    writes lens[2 u] and lens[2 u + 1] -- nothing else of the reads changes -- and counts.
//                 The kernel feeds the longest length it leaves into the parser's flags[0] (zeroed in front of it), adds its counters a
//                 wave together into a block of its own, and adds the insert histogram through a copy in LDS that a workgroup flushes
//                 once: a library with a tight insert distribution would put every pair on a few global addresses.
// A chunk the parser flagged malformed is not walked.  Plain vector stores and ordinary atomics only.  No read-back, no host
// synchronisation.
//
// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, k_po_cut: 72 VGPRs, 0 AGPRs, 62 SGPRs, no scratch, no spill of
// either kind, 7,040 bytes of LDS per workgroup (the histogram and eight pairs), 7 waves per SIMD by registers.  A workgroup is eight
// waves, two per SIMD, so three of them fit a CU (with sixteen waves only one did: four waves per SIMD instead of six).
#ifndef MLST_READ_OVERLAP_H
#define MLST_READ_OVERLAP_H

#define PO_MAX_LEN 320      // (MLST_MAX_READ_LEN: ten 64-bit words of 2-bit codes)
#define PO_WORDS 10
#define PO_HIST 1024
#define PO_WAVES 8          // pairs a workgroup of 512 threads holds at a time (72 VGPRs: three such workgroups per CU, six waves per SIMD)

struct PoSet { u32 min_overlap, max_mism, permille, trim5; };
struct PoCtr {          // device-resident counters (a block of their own)
    u64 overlapping;    // pairs with a chosen candidate
    u64 trimmed_pairs;  // pairs of which a mate was cut
    u64 reads_trimmed;
    u64 bases_removed;
    u64 emptied;        // mates of length >= 1 cut at 0
    u64 pad_[3];
    u64 hist[PO_HIST];  // min(o + n2 + 2 trim5, 1023) of every overlapping pair
};
struct PoPair {         // one pair in LDS: mate 1 forward, mate 2 as the reversed complement R with a zero word in front (r*[1 + q] = word q of R)
    u64 m1c[PO_WORDS], m1v[PO_WORDS];
    u64 rc[PO_WORDS + 3], rv[PO_WORDS + 3];
};

// bases 32 k .. 32 k + 31 of the n-base read at t: 2-bit codes and the ACGT mask (ra_chunk twice)
__device__ inline void po_word(const u8* __restrict__ t, u32 k, u32 n, u64& codes, u64& valid) {
    u32 c0, v0, c1, v1;
    ra_chunk(t, 32 * k, n, c0, v0); ra_chunk(t, 32 * k + 16, n, c1, v1);
    codes = (u64)c0 | ((u64)c1 << 32); valid = (u64)v0 | ((u64)v1 << 32);
}
// the thirty-two 2-bit groups of x in reverse order
__device__ inline u64 po_rev2(u64 x) { x = __brevll(x); return ((x >> 1) & RA_EVEN) | ((x & RA_EVEN) << 1); }

__global__ __launch_bounds__(64 * PO_WAVES) void k_po_cut(const u8* __restrict__ text, const u64* __restrict__ seq_off, u16* __restrict__ lens, u64 n_pairs, PoSet S,
                                                  u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */, PoCtr* __restrict__ C) {
    __shared__ u32 s_hist[PO_HIST];
    __shared__ PoPair s_pair[PO_WAVES];
    if (longest[1]) return;      // (as in k_ra_cut: the host refuses the chunk behind this kernel; the same for every thread)
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (u32 k = threadIdx.x; k < PO_HIST; k += blockDim.x) s_hist[k] = 0;
    PoPair& P = s_pair[wv];
    u32 mx = 0, n_ov = 0, n_pairs_cut = 0, n_reads = 0, n_rem = 0, n_empty = 0;      // (the wave's: every lane holds the same)
    // the loop is the workgroup's: every wave meets both barriers of every turn
    for (u64 base = (u64)blockIdx.x * PO_WAVES; base < n_pairs; base += (u64)gridDim.x * PO_WAVES) {
        const u64 u = base + wv;
        const bool in = u < n_pairs;
        u32 n1 = in ? (u32)(lens[2 * u] & 0x7FFFu) : 0u, n2 = in ? (u32)(lens[2 * u + 1] & 0x7FFFu) : 0u;      // plain lengths on entry
        const u32 len1 = n1, len2 = n2;
        if (n1 > PO_MAX_LEN) n1 = PO_MAX_LEN;      // (the parser flags a longer read, and the host refuses the chunk: the arrays in LDS hold ten words)
        if (n2 > PO_MAX_LEN) n2 = PO_MAX_LEN;
        const u32 W2 = (n2 + 31) >> 5, pad = 32 * W2 - n2;
        if (lane < PO_WORDS) {
            u64 c = 0, v = 0;
            if (32 * lane < n1) po_word(text + seq_off[2 * u], lane, n1, c, v);
            P.m1c[lane] = c; P.m1v[lane] = v;
        } else if (lane >= 32 && lane < 32 + PO_WORDS) {
            const u32 k = lane - 32;
            if (k < W2) {
                u64 c, v;
                po_word(text + seq_off[2 * u + 1], k, n2, c, v);
                P.rc[W2 - k] = po_rev2(~c); P.rv[W2 - k] = __brevll(v) >> 1;      // word W2 - 1 - k of R, behind the zero word
            }
        } else if (lane >= 48 && lane < 48 + PO_WORDS + 3) {
            const u32 k = lane - 48;
            if (k == 0 || k > W2) { P.rc[k] = 0; P.rv[k] = 0; }
        }
        __syncthreads();
        u32 best = 0;      // (matches << 12) | (2048 - o): the most matches, then the smallest o; 0 = no valid candidate (a valid one has a match)
        if (n1 >= S.min_overlap && n2 >= S.min_overlap) {
            const int o_hi = (int)n1 - (int)S.min_overlap;
            for (int ob = -((int)n2 - (int)S.min_overlap); ob <= o_hi; ob += 64) {
                const int o = ob + (int)lane;
                if (o > o_hi) continue;
                const int a = o > 0 ? o : 0, b = (o + (int)n2 < (int)n1) ? o + (int)n2 : (int)n1;      // the overlap on mate 1: [a, b)
                const u32 L = (u32)(b - a);
                const int w0 = a >> 5, w1 = (b - 1) >> 5;
                const int d = 32 * w0 - o + (int)pad;      // the position of R that lies on base 32 w0 of mate 1 (>= -31)
                int q = d >> 5;
                const u32 sh = 2u * ((u32)d & 31u);
                u64 lo_c = P.rc[1 + q], lo_v = P.rv[1 + q];
                u32 matches = 0;
                for (int w = w0; w <= w1; w++) {
                    q++;
                    const u64 hi_c = P.rc[1 + q], hi_v = P.rv[1 + q];
                    const u64 xc = sh ? (lo_c >> sh) | (hi_c << (64 - sh)) : lo_c;
                    const u64 xv = sh ? (lo_v >> sh) | (hi_v << (64 - sh)) : lo_v;
                    const u64 x = P.m1c[w] ^ xc;
                    matches += (u32)__popcll(~(x | (x >> 1)) & P.m1v[w] & xv);
                    lo_c = hi_c; lo_v = hi_v;
                }
                const u32 mism = L - matches;
                if (mism <= S.max_mism && mism * 1000u <= L * S.permille) {
                    const u32 key = (matches << 12) | (u32)(2048 - o);
                    if (key > best) best = key;
                }
            }
        }
        for (int s = 32; s > 0; s >>= 1) { const u32 x = __shfl_xor(best, s); best = x > best ? x : best; }
        u32 k1 = len1, k2 = len2;
        if (best) {
            const int o = 2048 - (int)(best & 4095u);
            const u32 end = (u32)(o + (int)n2) + S.trim5;      // where the insert ends in either prepared mate (o + n2 >= min_overlap)
            u32 fl = end + S.trim5; if (fl > PO_HIST - 1) fl = PO_HIST - 1;
            n_ov++;
            u32 cut = 0;
            if (end < n1) { k1 = end; cut++; n_rem += n1 - end; if (!end) n_empty++; }
            if (end < n2) { k2 = end; cut++; n_rem += n2 - end; if (!end) n_empty++; }
            n_reads += cut; if (cut) n_pairs_cut++;
            if (lane == 0) {
                atomicAdd(&s_hist[fl], 1u);
                if (k1 != len1) lens[2 * u] = (u16)k1;
                if (k2 != len2) lens[2 * u + 1] = (u16)k2;
            }
        }
        const u32 m = k1 > k2 ? k1 : k2;
        if (m > mx) mx = m;
        __syncthreads();      // the pair's words are read: the next turn overwrites them
    }
    if (lane == 0) {      // one atomic per wave and counter
        if (mx) atomicMax(longest, mx);
        if (n_ov) atomicAdd((unsigned long long*)&C->overlapping, (unsigned long long)n_ov);
        if (n_pairs_cut) atomicAdd((unsigned long long*)&C->trimmed_pairs, (unsigned long long)n_pairs_cut);
        if (n_reads) atomicAdd((unsigned long long*)&C->reads_trimmed, (unsigned long long)n_reads);
        if (n_rem) atomicAdd((unsigned long long*)&C->bases_removed, (unsigned long long)n_rem);
        if (n_empty) atomicAdd((unsigned long long*)&C->emptied, (unsigned long long)n_empty);
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k < PO_HIST; k += blockDim.x) { const u32 v = s_hist[k]; if (v) atomicAdd((unsigned long long*)&C->hist[k], (unsigned long long)v); }
}

#endif
