// read_prep.h -- reads prepared on the device before they are packed (mlst_set_read_prep; the rule: include/mlst.h, stated on the
// host as metamlst_amd.fastq.prep_fastq; `cli type --trim5 / --trim3 / --trim-qual / --phred64`).  Included by mlst_engine.hip next to
// read_names.h.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records), so preparing it is
// arithmetic on those three, done behind the parser and in front of the length read-back and of k_pack_text:
//   k_rp_qtrim    a thread per read.  The fixed trims (bowtie2's -5 / -3) move both offsets by a = min(trim5, n) and leave
//                 n1 = max(0, n - trim5 - trim3) bases.  The quality trim of the 3' end (cutadapt -q / bwa aln -q; trim_qual 0: off)
//                 then walks the n1 quality bytes from the last one down in 16-byte steps, the running sum of T - q in registers, and
//                 leaves at the first negative sum; the length becomes the index at which the sum was largest (among equals, the one met first).
//                 It writes the offsets and the length, feeds the longest prepared length (the parser's flags[0], zeroed in front of
//                 it: the packed rows are as wide as those of the prepared text) and adds the three counters, a wave together.
// The Phred base (33 / 64) is k_pack_text's template parameter (pack_group in mlst_engine.hip); the walk here takes it as a value.
// Errors (sequence and quality lengths differ, a read beyond MLST_MAX_READ_LEN) are the parser's and are judged on the record as it
// stands in the file.  Plain vector stores only.
#ifndef MLST_READ_PREP_H
#define MLST_READ_PREP_H

struct RpCtr {          // device-resident counters (a block of their own: EngineDev::ctr keeps its layout)
    u64 shortened;      // reads whose length changed
    u64 removed;        // bases removed
    u64 emptied;        // reads of length >= 1 left without a base
    u64 pad_;
};
struct RpSet { u32 trim5, trim3, trim_qual, phred_base; };      // mlst_read_prep

// The quality trim on the n1 quality bytes at q: the new length.  s = sum of T - q[i] from the 3' end down; the walk ends at the
// first negative s; the cut is the i at which s first reached its largest value (an equal sum further down does not move it).
__device__ inline u32 rp_qtrim_len(const u8* __restrict__ q, u32 n1, int T, int base) {
    int s = 0, best = 0; u32 cut = n1; bool done = false;
    for (int end = (int)n1; end > 0 && !done; end -= 16) {
        const int lo = end - 16;      // cq[k] is byte lo + k of the read; bytes in front of the read are not loaded
        u8 cq[16];
        if (lo >= 0) __builtin_memcpy(cq, q + lo, 16);      // (the compiler picks the widest loads the target allows unaligned)
        else {
            #pragma unroll
            for (int k = 0; k < 16; k++) cq[k] = lo + k >= 0 ? q[lo + k] : (u8)0;
        }
        #pragma unroll
        for (int k = 15; k >= 0; k--) {
            const int i = lo + k;
            if (i >= 0 && !done) {
                int v = (int)cq[k] - base; v = v < 0 ? 0 : (v > 127 ? 127 : v);
                s += T - v;
                if (s < 0) done = true;
                else if (s > best) { best = s; cut = (u32)i; }
            }
        }
    }
    return cut;
}

__global__ __launch_bounds__(256) void k_rp_qtrim(const u8* __restrict__ text, u64* __restrict__ seq_off, u64* __restrict__ qual_off, u16* __restrict__ lens,
                                                   u64 n_reads, RpSet P, u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */, RpCtr* __restrict__ C) {
    // longest[1]: the parser's error bits.  A chunk with a malformed record is refused by the host behind this kernel; its quality line may
    // be shorter than its sequence, so it is not walked (and not counted)
    if (longest[1]) return;
    u32 mx = 0, n_short = 0, n_rem = 0, n_empty = 0;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u32 n = lens[r];      // plain lengths on entry, as the parser leaves them (at most MLST_MAX_READ_LEN)
        const u32 a = P.trim5 < n ? P.trim5 : n;
        const u32 n1 = n > P.trim5 + P.trim3 ? n - P.trim5 - P.trim3 : 0u;      // (both trims are at most 65535)
        const u64 qo = qual_off[r] + a;
        u32 n2 = n1;
        if (P.trim_qual && n1) n2 = rp_qtrim_len(text + qo, n1, (int)P.trim_qual, (int)P.phred_base);
        if (a) { seq_off[r] += a; qual_off[r] = qo; }
        if (n2 != n) { lens[r] = (u16)n2; n_short++; n_rem += n - n2; if (!n2) n_empty++; }
        if (n2 > mx) mx = n2;
    }
    // one wave reduction, then one atomic per wave and counter
    n_short = wave_sum_u32(n_short); n_rem = wave_sum_u32(n_rem); n_empty = wave_sum_u32(n_empty);
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(mx, o); mx = x > mx ? x : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(longest, mx);
        if (n_short) atomicAdd((unsigned long long*)&C->shortened, (unsigned long long)n_short);
        if (n_rem) atomicAdd((unsigned long long*)&C->removed, (unsigned long long)n_rem);
        if (n_empty) atomicAdd((unsigned long long*)&C->emptied, (unsigned long long)n_empty);
    }
}

#endif
