// read_adapt.h -- 3' adapters removed on the device before the reads are packed (mlst_set_read_adapters; the rule: include/mlst.h, stated
// on the host as metamlst_amd.fastq.adapter_cut / trim_adapters; `cli type --adapter`).  Included by mlst_engine.hip next to read_prep.h.
// The rule is modelled on `cutadapt -a ADAPTER --no-indels --times 1`; it is the project's own and claims none of cutadapt's bytes.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records; read_prep.h), and removing
// a 3' adapter only lowers the length:
//   k_ra_cut      a thread per read, behind k_rp_qtrim when that runs and behind the parser alone otherwise, in front of the read-back
//                 of the parser's flags.  It reads seq_off[r] and lens[r] and writes lens[r] only.  The adapters (at most 8, at most 64
//                 letters) are kernel arguments: 2-bit codes, a mask of the letters that are not N, a mask of those that are, the
//                 length.  They are the same for every lane, so the loop over adapters is the outer one and an adapter stays in scalar
//                 registers while the lane slides a 64-base window of its read past it: 128 bits of 2-bit codes and an "is ACGT" mask
//                 of the same spacing (bit 2 i for base i), sixteen text bytes converted per sixteen starts (loaded as rp_qtrim_len
//                 loads them), the window shifted one base per start p.  A candidate (p, adapter) is then an XOR, a fold of the two
//                 bits of a code, two ANDs and a popcount per 64-bit word; the upper word is looked at only for an adapter longer
//                 than 32 letters, the adapter's N letters only where it has some.  No per-thread array is indexed at run time.
//                 The kernel feeds the longest length it leaves into the parser's flags[0] (zeroed in front of k_rp_qtrim and
//                 again in front of k_ra_cut, so the packed rows are as wide as those of the prepared, cut text) and adds its counters, a
//                 wave together, into a block of its own.
// A chunk the parser flagged malformed is not walked.  Plain vector stores and ordinary atomics only.
//
// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, k_ra_cut: 42 VGPRs, 0 AGPRs, 95 SGPRs, no scratch, no spill of
// either kind, no LDS, 8 waves per SIMD.  (With the read's last bytes loaded as sixteen predicated loads, as rp_qtrim_len loads them, their
// lane masks were hoisted out of the loop over adapters: 107 scalar registers spilled into vector lanes, 76 VGPRs, 6 waves -- hence the loop.)
#ifndef MLST_READ_ADAPT_H
#define MLST_READ_ADAPT_H

#define RA_MAX_ADAPTERS 8
#define RA_MAX_LEN 64
#define RA_EVEN 0x5555555555555555ull

struct RaAd {           // one adapter, letter i at bits 2 i / 2 i + 1 of code (A 0, C 1, G 2, T 3; [0]: letters 0-31, [1]: 32-63)
    u64 code[2];
    u64 care[2];        // bit 2 i: letter i is one of ACGT
    u64 anyn[2];        // bit 2 i: letter i is N (it matches every byte of the read)
    u32 m;              // letters
    u32 mo;             // min(min_overlap, m): the read must hold that many bases from the start on
};
struct RaSet { u32 K, permille, min_overlap, pad_; RaAd ad[RA_MAX_ADAPTERS]; };
struct RaCtr {          // device-resident counters (a block of their own)
    u64 trimmed;        // reads cut
    u64 removed;        // bases removed
    u64 emptied;        // reads of length >= 1 cut at 0
    u64 pad_;
    u64 per_adapter[RA_MAX_ADAPTERS];
};

// Bases q .. q + 15 of the n-base read at t: 2-bit codes (base q + j at bits 2 j) and the mask of those that are one of ACGT in either
// case (bit 2 j).  A base beyond the read is no ACGT.  The letter arithmetic is pack_group's.
__device__ inline void ra_chunk(const u8* __restrict__ t, u32 q, u32 n, u32& codes, u32& valid) {
    u64 c8[2] = {0, 0};      // (constant indices only)
    if (q + 16 <= n) __builtin_memcpy(c8, t + q, 16);      // (the compiler picks the widest loads the target allows unaligned)
    else {      // the read's last bytes, one by one: a loop, not sixteen predicated loads whose lane masks would crowd the scalar registers
        const u32 cnt = q < n ? n - q : 0u;
        #pragma unroll 1
        for (u32 k = 0; k < cnt; k++) { const u64 b = t[q + k]; if (k < 8) c8[0] |= b << (8 * k); else c8[1] |= b << (8 * (k - 8)); }
    }
    codes = 0; valid = 0;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32 b4 = (u32)(c8[j >> 1] >> (32 * (j & 1)));
        const u32 y = (b4 >> 1) & 0x03030303u, y0 = y & 0x01010101u, y1 = (y >> 1) & 0x01010101u;      // bits 1-2 of a letter: A 0, C 1, T 2, G 3 (either case)
        const u32 code = y ^ y1;                                                                        // A 0, C 1, G 2, T 3
        const u32 expect = 0x41414141u + y0 * 2u + y1 * 0x13u - (y0 & y1) * 0x0Fu;                       // the upper-case letter those bits stand for
        const u32 diff = (b4 & 0xDFDFDFDFu) ^ expect;                                                   // non-zero byte: not one of ACGT
        const u32 ok = (~((diff | ((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7)) & 0x01010101u;
        codes |= ((code * 0x01041040u) >> 24) << (8 * j);                                               // four 2-bit codes -> one byte
        valid |= ((ok * 0x01041040u) >> 24) << (8 * j);                                                 // four flags -> bits 0, 2, 4, 6 of one byte
    }
}

// Every start p of adapter A (index k) on the n-base read at t; (best, bp, bk) = the matches, start and adapter of the valid candidate
// with the most matches so far (best 0: none yet -- a valid candidate has at least one match, its budget being at most half its overlap).
// Among equals the smallest p wins, then the smallest k: the adapters come in ascending k and the starts in ascending p.
__device__ inline void ra_scan(const u8* __restrict__ t, u32 n, const RaAd& A, u32 permille, u32 k, u32& best, u32& bp, u32& bk) {
    if (n < A.mo) return;
    const u32 last = n - A.mo;
    const bool wide = A.m > 32, has_n = (A.anyn[0] | A.anyn[1]) != 0;      // (the same for every lane)
    u32 c0, v0, c1, v1;
    ra_chunk(t, 0, n, c0, v0); ra_chunk(t, 16, n, c1, v1);
    u64 lo = (u64)c0 | ((u64)c1 << 32), vlo = (u64)v0 | ((u64)v1 << 32);
    ra_chunk(t, 32, n, c0, v0); ra_chunk(t, 48, n, c1, v1);
    u64 hi = (u64)c0 | ((u64)c1 << 32), vhi = (u64)v0 | ((u64)v1 << 32);
    u32 nx = 0, nv = 0;      // bases p + 64 .. of the sixteen starts under way
    for (u32 p = 0; p <= last; p++) {
        if ((p & 15u) == 0) { nx = 0; nv = 0; if (p + 64 < n) ra_chunk(t, p + 64, n, nx, nv); }
        const u32 rem = n - p;
        const u64 xlo = lo ^ A.code[0];
        u64 mlo = ~(xlo | (xlo >> 1)) & A.care[0] & vlo;      // bit 2 i: letter i of the adapter equals base p + i (an ACGT one, inside the read)
        u64 mhi = 0;
        if (wide) { const u64 xhi = hi ^ A.code[1]; mhi = ~(xhi | (xhi >> 1)) & A.care[1] & vhi; }
        if (has_n) {      // the adapter's N letters match whatever byte of the read they meet
            mlo |= A.anyn[0] & (rem >= 32 ? RA_EVEN : ((1ull << (2 * rem)) - 1));
            if (wide && rem > 32) mhi |= A.anyn[1] & (rem >= 64 ? RA_EVEN : ((1ull << (2 * (rem - 32))) - 1));
        }
        const u32 matches = (u32)__popcll(mlo) + (u32)__popcll(mhi);
        const u32 L = A.m < rem ? A.m : rem;
        if ((L - matches) * 1000u <= L * permille && (matches > best || (matches == best && p < bp))) { best = matches; bp = p; bk = k; }
        lo = (lo >> 2) | (hi << 62); hi = (hi >> 2) | ((u64)(nx & 3u) << 62); nx >>= 2;
        vlo = (vlo >> 2) | (vhi << 62); vhi = (vhi >> 2) | ((u64)(nv & 3u) << 62); nv >>= 2;
    }
}

__global__ __launch_bounds__(256) void k_ra_cut(const u8* __restrict__ text, const u64* __restrict__ seq_off, u16* __restrict__ lens, u64 n_reads, RaSet S,
                                                 u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */, RaCtr* __restrict__ C) {
    if (longest[1]) return;      // (as in k_rp_qtrim: the host refuses the chunk behind this kernel)
    u32 mx = 0, n_trim = 0, n_rem = 0, n_empty = 0;
    u32 pa[RA_MAX_ADAPTERS] = {0, 0, 0, 0, 0, 0, 0, 0};      // reads cut per adapter, the wave's (constant indices only: registers)
    // the loop is the wave's, not the lane's: the ballots below count every lane
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n_reads; base += (u64)gridDim.x * blockDim.x) {
        const u64 r = base + threadIdx.x;
        const bool in = r < n_reads;
        const u32 n = in ? (u32)(lens[r] & 0x7FFFu) : 0u;      // plain lengths on entry (at most MLST_MAX_READ_LEN)
        const u8* t = text + (in ? seq_off[r] : 0);
        u32 best = 0, bp = 0, bk = 0;
        #pragma unroll 1
        for (u32 k = 0; k < S.K; k++) ra_scan(t, n, S.ad[k], S.permille, k, best, bp, bk);
        u32 n2 = n;
        if (best) { n2 = bp; lens[r] = (u16)bp; n_trim++; n_rem += n - bp; if (!bp) n_empty++; }
        if (n2 > mx) mx = n2;
        #pragma unroll
        for (u32 k = 0; k < RA_MAX_ADAPTERS; k++) pa[k] += (u32)__popcll(__ballot(best != 0 && bk == k));
    }
    // one wave reduction, then one atomic per wave and counter
    n_trim = wave_sum_u32(n_trim); n_rem = wave_sum_u32(n_rem); n_empty = wave_sum_u32(n_empty);
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(mx, o); mx = x > mx ? x : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(longest, mx);
        if (n_trim) atomicAdd((unsigned long long*)&C->trimmed, (unsigned long long)n_trim);
        if (n_rem) atomicAdd((unsigned long long*)&C->removed, (unsigned long long)n_rem);
        if (n_empty) atomicAdd((unsigned long long*)&C->emptied, (unsigned long long)n_empty);
        #pragma unroll
        for (u32 k = 0; k < RA_MAX_ADAPTERS; k++) if (pa[k]) atomicAdd((unsigned long long*)&C->per_adapter[k], (unsigned long long)pa[k]);
    }
}

#endif
