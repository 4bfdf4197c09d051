// read_names.h -- the names of the retained reads, copied out of the FASTQ text on the device (mlst_set_read_names; the rule:
// include/mlst.h, stated on the host as metamlst_amd.samout.read_qname; `cli type --read-names`).  Included by mlst_engine.hip in
// front of aln_text.h, whose kernels write a kept name as QNAME.
//
// The text of a chunk sits in its text slot while the chunk is parsed; with the switch on the slot is released (ev_packed) behind
// k_rn_gather instead of behind k_pack_text, so the header lines are still there when pass 1 has decided which reads it retains.
//   k_rn_gather   queued by fq_pack_submit behind the submission (outside its captured graph).  Walks the retained slots from the
//                 names cursor to min(n_ret, cap_ret) -- both read on the device --, a lane per slot: the slot's read of the chunk
//                 (ret_ridx - read_base), its header line from the parser's line table, the rule.  A wave reserves the bytes of its
//                 64 names with one returning atomic and copies them, the wave together, name after name.
//   k_rn_advance  one thread: the names cursor moves up to min(n_ret, cap_ret).
// Plain vector stores only.
#ifndef MLST_READ_NAMES_H
#define MLST_READ_NAMES_H

#define RN_MAX_NAME 254u      /* the longest legal SAM QNAME */

struct RnCtr {          // device-resident counters of the name arena (a block of their own: EngineDev::ctr keeps its layout)
    u64 bytes;          // bump cursor: bytes reserved so far (beyond cap_bytes: the bytes that would have been needed)
    u64 done;           // the retained slots [0, done) have their ret_name_off / ret_name_len
    u64 fallbacks;      // retained reads whose name is no legal QNAME (ret_name_len = 0: the export writes r<k>)
    u64 longest;        // longest kept name, bytes
    u64 err;            // bit0: the arena is full
    u64 pad_[3];
};
// where the header lines of the chunk's reads start: read r of the chunk is record rec of a line table
//   pair_k == 0, lines2 == NULL   one file: rec = r of lines1 (k_fq_records)
//   pair_k != 0                   two files back to back in one table: r = 2 j + f is record j + f * pair_k of lines1 (k_fq_records)
//   lines2 != NULL                two tables: r = 2 j + f is record j of lines1 (f = 0) or lines2 (f = 1) (k_fq_pair_records)
struct RnSrc { const u64* lines1; const u64* lines2; u64 pair_k; };

// The rule on one header line (text[at] is its '@'): the bytes behind the '@' up to the first space, TAB, CR or LF.  Returns the
// name's length, or 0 when it is no legal QNAME (empty, longer than RN_MAX_NAME, a '@' or a byte outside '!'..'~' in it).  A header
// line ends with a LF in front of its record's sequence line, so the walk stays inside the text.
__device__ inline u32 rn_name_len(const u8* __restrict__ text, u64 at) {
    const u8* p = text + at + 1;
    u32 n = 0; bool ok = true;
    for (; n <= RN_MAX_NAME; n++) {
        const u8 c = p[n];
        if (c == (u8)' ' || c == (u8)'\t' || c == (u8)'\r' || c == (u8)'\n') break;
        if (c < (u8)'!' || c > (u8)'~' || c == (u8)'@') ok = false;
    }
    return (ok && n >= 1 && n <= RN_MAX_NAME) ? n : 0u;
}

__global__ __launch_bounds__(256) void k_rn_gather(const EngineDev* __restrict__ Ep, const u8* __restrict__ text, RnSrc S, u64 read_base, u64 n_reads,
                                                    RnCtr* __restrict__ C, u8* __restrict__ arena, u64 cap_bytes, u64* __restrict__ name_off, u16* __restrict__ name_len) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const u64 begin = C->done, end = E.ctr->n_ret < E.cap_ret ? E.ctr->n_ret : E.cap_ret;
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * (blockDim.x >> 6);
    u32 n_fall = 0, longest = 0;
    for (u64 s0 = begin + wave * 64; s0 < end; s0 += n_waves * 64) {      // wave-uniform
        const u64 slot = s0 + (u64)lane;
        u64 at = 0; u32 len = 0;
        if (slot < end) {
            const u64 r = E.ret_ridx[slot] - read_base;
            if (r < n_reads) {      // (a slot of this chunk: the cursor stood at the chunk's first slot)
                const u64 j = r >> 1, f = r & 1;
                if (S.lines2) at = (f ? S.lines2 : S.lines1)[4 * j];
                else at = S.lines1[4 * (S.pair_k ? j + f * S.pair_k : r)];
                len = rn_name_len(text, at);
                if (!len) n_fall++;
                if (len > longest) longest = len;
            }
        }
        // the wave's bytes: one returning atomic, every lane's name behind the names of the lanes in front of it
        u32 inc = len;
        for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        const u32 total = __shfl(inc, 63);
        u64 base = 0;
        if (lane == 0 && total) base = atomicAdd((unsigned long long*)&C->bytes, (unsigned long long)total);
        base = __shfl(base, 0);
        const bool fits = base + (u64)total <= cap_bytes;
        if (!fits && lane == 0) atomicOr((unsigned long long*)&C->err, 1ull);
        const u64 off = base + (u64)(inc - len);
        if (slot < end) { name_off[slot] = fits ? off : 0ull; name_len[slot] = fits ? (u16)len : (u16)0; }
        u64 m = __ballot(fits && len > 0);
        while (m) {      // name after name, the wave together: a byte per lane and store
            const int t = __ffsll((long long)m) - 1; m &= m - 1;
            const u64 src = uniform_u64(__shfl(at, t)) + 1, dst = uniform_u64(__shfl(off, t));
            const u32 n = (u32)__shfl((int)len, t);
            for (u32 i = (u32)lane; i < n; i += 64) arena[dst + i] = text[src + i];
        }
    }
    n_fall = wave_sum_u32(n_fall);
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(longest, o); longest = x > longest ? x : longest; }
    if (lane == 0) {
        if (n_fall) atomicAdd((unsigned long long*)&C->fallbacks, (unsigned long long)n_fall);
        if (longest) atomicMax((unsigned long long*)&C->longest, (unsigned long long)longest);
    }
}
__global__ void k_rn_advance(const EngineDev* __restrict__ Ep, RnCtr* __restrict__ C) {
    const EngineDev& E = *Ep;
    const u64 end = E.ctr->n_ret < E.cap_ret ? E.ctr->n_ret : E.cap_ret;
    if (end > C->done) C->done = end;
}

#endif
