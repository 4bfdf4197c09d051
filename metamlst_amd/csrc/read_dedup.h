// read_dedup.h -- exact duplicate reads removed on the device before the reads are packed (mlst_set_read_dedup; the rule: include/mlst.h,
// stated on the host as metamlst_amd.fastq.dedup_fastq; `cli type --dedup`).  Included by mlst_engine.hip next to read_adapt.h.
//
// A read of FASTQ text is a sequence offset, a quality offset and a length (k_fq_records, k_fq_pair_records; read_prep.h), and removing a
// duplicate only sets its length to 0.  A unit (a read; a pair in a paired submission) is its 128-bit key (MLST_DEDUP_KEY): two 64-bit
// hashes of its length(s) and its letters folded to A C G T N.  The keys of a sample live in a table in device memory, parallel arrays
// over a power-of-two number of slots: tag (the first hash, never 0; 0 = empty), chk (the second hash), first (the lowest unit index of
// the key, ~0 at first) and cnt (its later copies).  Per chunk, behind k_ra_cut and in front of the read-back of the parser's flags:
//   k_dd_insert   a thread per unit.  Both hashes of the unit (the text sixteen bytes at a time: ra_chunk), then a linear probe from the
//                 first hash with a 64-bit atomicCAS on tag; on a free or an equal tag atomicMin(first[s], unit index).  The slot and
//                 the second hash are kept per unit of the chunk for the two launches behind it (slot_of, key2).
//   k_dd_sign     the unit whose index IS first[s] writes chk[s]: a key new in this chunk has exactly one such unit.
//   k_dd_mark     a unit that owns its slot is kept; one whose second hash equals chk[s] is a duplicate (length(s) 0, cnt[s] + 1); one
//                 whose second hash differs shares only the first 64 bits with the slot's key (a clash): kept and counted.  The kernel
//                 feeds the longest remaining length into the parser's flags[0] (zeroed in front of it) and adds its counters, a wave
//                 together.
// Three launches, so that no thread waits for another: there is no spin loop, and every probe is bounded by the slot count (a probe that
// runs out sets DdCtr::err, which the host reports as MLST_E_HIP).  The owner of a slot is the lowest unit index whatever order the
// threads ran in, and chunks are queued on one stream in read-index order, so the outcome is a function of the text alone.
//   k_dd_rehash   a thread per slot of the old table: every occupied slot is inserted into a larger one (tags are distinct, so the CAS
//                 claims a free slot) and its chk, first and cnt are copied.
//   k_dd_levels   a thread per slot: the histogram of cnt + 1 over occupied slots in eight bins (mlst_read_dedup_info).
// A chunk the parser flagged malformed is not walked.  Plain vector stores and ordinary atomics only.
//
// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage: k_dd_insert 28 VGPRs, 78 SGPRs; k_dd_sign 18 / 30; k_dd_mark
// 28 / 40; k_dd_rehash 18 / 52; k_dd_levels 12 / 29 and 32 bytes of LDS; no scratch, no spill, 8 waves per SIMD each.
#ifndef MLST_READ_DEDUP_H
#define MLST_READ_DEDUP_H

#define DD_NONE 0xFFFFFFFFu

struct DdCtr {          // device-resident counters (a block of their own)
    u64 units;          // reads or pairs that took part
    u64 dups;           // units removed
    u64 reads_removed;
    u64 bases_removed;
    u64 distinct;       // occupied slots
    u64 clashes;
    u64 err;            // a probe ran through the whole table
    u64 pad_;
    u64 levels[8];      // k_dd_levels
};
struct DdTab { u64* tag; u64* chk; u64* first; u32* cnt; u64 slots; u64 tag_mask; };

__device__ inline u64 dd_fmix(u64 x) { x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33; return x; }
// one 64-bit word into both hashes: two multiplicative mixes with constants, rotations and an operation of their own
__device__ inline void dd_absorb(u64& h1, u64& h2, u64 x) {
    h1 = (h1 ^ x) * 0x9E3779B97F4A7C15ull; h1 ^= h1 >> 29;
    h2 = (h2 + x) * 0xD6E8FEB86659FD93ull; h2 = (h2 << 27) | (h2 >> 37);
}
// the n-base read at t: its length, then per sixteen bases the 2-bit codes (0 where the byte is not one of ACGT) and the ACGT mask --
// words that determine (length, folded letters) and are determined by them
__device__ inline void dd_hash_read(const u8* __restrict__ t, u32 n, u64& h1, u64& h2) {
    dd_absorb(h1, h2, 0x8000000000000000ull | n);
    for (u32 q = 0; q < n; q += 16) {
        u32 codes, valid;
        ra_chunk(t, q, n, codes, valid);
        codes &= valid | (valid << 1);
        dd_absorb(h1, h2, (u64)codes | ((u64)valid << 32));
    }
}

__global__ __launch_bounds__(256) void k_dd_insert(const u8* __restrict__ text, const u64* __restrict__ seq_off, const u16* __restrict__ lens, u64 n_units, u32 paired,
                                                    u64 unit_base, DdTab T, u32* __restrict__ slot_of, u64* __restrict__ key2,
                                                    const u32* __restrict__ flags /* the parser's: [1] = errors */, DdCtr* __restrict__ C) {
    if (flags[1]) return;
    for (u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (u64)gridDim.x * blockDim.x) {
        const u64 r = paired ? 2 * u : u;
        const u32 n0 = lens[r] & 0x7FFFu, n1 = paired ? (u32)(lens[r + 1] & 0x7FFFu) : 0u;
        u32 s_found = DD_NONE; u64 h2 = 0;
        if (n0 | n1) {
            u64 h1 = 0x243F6A8885A308D3ull; h2 = 0x13198A2E03707344ull;
            dd_hash_read(text + seq_off[r], n0, h1, h2);
            if (paired) dd_hash_read(text + seq_off[r + 1], n1, h1, h2);
            h1 = dd_fmix(h1); h2 = dd_fmix(h2);
            const u64 low = h1 & T.tag_mask, tag = low ? low : 1ull;      // (0 is the empty slot)
            const u64 mask = T.slots - 1;
            u64 s = tag & mask;      // (from the tag, not the hash: k_dd_rehash starts where a later look-up will)
            for (u64 i = 0; i < T.slots; i++, s = (s + 1) & mask) {
                const u64 old = atomicCAS((unsigned long long*)&T.tag[s], 0ull, (unsigned long long)tag);
                if (old == 0 || old == tag) { atomicMin((unsigned long long*)&T.first[s], (unsigned long long)(unit_base + u)); s_found = (u32)s; break; }
            }
            if (s_found == DD_NONE) atomicOr((unsigned long long*)&C->err, 1ull);
        }
        slot_of[u] = s_found; key2[u] = h2;
    }
}

__global__ __launch_bounds__(256) void k_dd_sign(u64 n_units, u64 unit_base, DdTab T, const u32* __restrict__ slot_of, const u64* __restrict__ key2,
                                                  const u32* __restrict__ flags, DdCtr* __restrict__ C) {
    if (flags[1]) return;
    u32 n_new = 0;
    // the loop is the wave's, not the lane's (the reduction below counts every lane)
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n_units; base += (u64)gridDim.x * blockDim.x) {
        const u64 u = base + threadIdx.x;
        const u32 s = u < n_units ? slot_of[u] : DD_NONE;
        if (s != DD_NONE && T.first[s] == unit_base + u) { T.chk[s] = key2[u]; n_new++; }
    }
    n_new = wave_sum_u32(n_new);
    if ((threadIdx.x & 63) == 0 && n_new) atomicAdd((unsigned long long*)&C->distinct, (unsigned long long)n_new);
}

__global__ __launch_bounds__(256) void k_dd_mark(u16* __restrict__ lens, u64 n_units, u32 paired, u64 unit_base, DdTab T, const u32* __restrict__ slot_of,
                                                  const u64* __restrict__ key2, u32* __restrict__ longest /* the parser's flags: [0] = longest length, [1] = errors */,
                                                  DdCtr* __restrict__ C) {
    if (longest[1] & ~8u) return;      // (bit 3 is this kernel's own, below)
    if (blockIdx.x == 0 && threadIdx.x == 0 && C->err) atomicOr(&longest[1], 8u);      // a probe ran out (k_dd_insert, k_dd_rehash): the host refuses the chunk
    u32 mx = 0, n_unit = 0, n_dup = 0, n_reads = 0, n_bases = 0, n_clash = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n_units; base += (u64)gridDim.x * blockDim.x) {
        const u64 u = base + threadIdx.x;
        if (u < n_units) {
            const u64 r = paired ? 2 * u : u;
            u32 n0 = lens[r] & 0x7FFFu, n1 = paired ? (u32)(lens[r + 1] & 0x7FFFu) : 0u;
            const u32 s = slot_of[u];
            if (s != DD_NONE) {
                n_unit++;
                if (T.first[s] != unit_base + u) {
                    if (T.chk[s] == key2[u]) {
                        atomicAdd(&T.cnt[s], 1u);
                        n_dup++; n_reads += paired ? 2u : 1u; n_bases += n0 + n1;
                        lens[r] = 0; if (paired) lens[r + 1] = 0;
                        n0 = n1 = 0;
                    } else n_clash++;
                }
            }
            const u32 m = n0 > n1 ? n0 : n1;
            if (m > mx) mx = m;
        }
    }
    // one wave reduction, then one atomic per wave and counter
    n_unit = wave_sum_u32(n_unit); n_dup = wave_sum_u32(n_dup); n_reads = wave_sum_u32(n_reads); n_bases = wave_sum_u32(n_bases); n_clash = wave_sum_u32(n_clash);
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(mx, o); mx = x > mx ? x : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(longest, mx);
        if (n_unit) atomicAdd((unsigned long long*)&C->units, (unsigned long long)n_unit);
        if (n_dup) atomicAdd((unsigned long long*)&C->dups, (unsigned long long)n_dup);
        if (n_reads) atomicAdd((unsigned long long*)&C->reads_removed, (unsigned long long)n_reads);
        if (n_bases) atomicAdd((unsigned long long*)&C->bases_removed, (unsigned long long)n_bases);
        if (n_clash) atomicAdd((unsigned long long*)&C->clashes, (unsigned long long)n_clash);
    }
}

// every occupied slot of `from` into the empty, larger `to` (the same tag mask): the set of (tag, chk, first, cnt) is preserved exactly
__global__ __launch_bounds__(256) void k_dd_rehash(DdTab from, DdTab to, DdCtr* __restrict__ C) {
    const u64 mask = to.slots - 1;
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < from.slots; k += (u64)gridDim.x * blockDim.x) {
        const u64 tag = from.tag[k];
        if (!tag) continue;
        u64 s = tag & mask;      // (k_dd_insert's start)
        bool put = false;
        for (u64 i = 0; i < to.slots; i++, s = (s + 1) & mask) {
            if (atomicCAS((unsigned long long*)&to.tag[s], 0ull, (unsigned long long)tag) == 0) { to.chk[s] = from.chk[k]; to.first[s] = from.first[k]; to.cnt[s] = from.cnt[k]; put = true; break; }
        }
        if (!put) atomicOr((unsigned long long*)&C->err, 1ull);
    }
}

// distinct keys by how often they occur (cnt + 1): 1, 2, 3, 4, 5-9, 10-49, 50-499, >= 500 -- per workgroup in LDS, then eight atomics
__global__ __launch_bounds__(256) void k_dd_levels(DdTab T, DdCtr* __restrict__ C) {
    __shared__ u32 s_lv[8];
    if (threadIdx.x < 8) s_lv[threadIdx.x] = 0;
    __syncthreads();
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < T.slots; k += (u64)gridDim.x * blockDim.x) {
        if (!T.tag[k]) continue;
        const u64 c = (u64)T.cnt[k] + 1;
        const u32 lv = c < 5 ? (u32)c - 1 : (c < 10 ? 4u : (c < 50 ? 5u : (c < 500 ? 6u : 7u)));
        atomicAdd(&s_lv[lv], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 8 && s_lv[threadIdx.x]) atomicAdd((unsigned long long*)&C->levels[threadIdx.x], (unsigned long long)s_lv[threadIdx.x]);
}

#endif
