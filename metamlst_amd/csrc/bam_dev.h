// bam_dev.h -- BAM records on the device (included by mlst_engine.hip behind the engine's device-side views).
//
// The inflated bytes of a piece of a BGZF BAM lie in a text slot behind BAM_HEAD bytes of head room; the partial record the piece
// before left over is copied in front of them (k_bam_carry_in).  BAM records are a chain (block_size prefix) that ignores BGZF
// block boundaries, so the starts are found the way bgzf_walk_parallel finds block headers: the text is cut into cells of BAM_CELL
// bytes; one workgroup per cell GUESSES the first record start of its cell (lanes test consecutive offsets for a plausible record
// head with plausible records chained behind it) and walks the chain inside the cell from there (k_bam_cells); k_bam_link then goes
// over the cells in order: a cell's list counts only where the chain of the cells before it lands on the cell's guess, and a cell
// whose guess is wrong (or missing) is walked again from its true entry -- never trusted.  By induction from the known entry of
// the piece every start is exact.  k_bam_link also turns the cells' counts into record indices (prefix sum) and finds where the
// carry for the next piece begins.
//   k_bam_accumulate : pass 1, metamlst.py:101-130 on the records in place (one thread per record)
//   k_bam_bank_*     : sequenceBank (metamlst.py:127): distinct QNAME per locus, last record wins, lengths summed
//   k_bam_pileup     : pass 2, what k_pileup_aln does, from the records in place
// gfx950 build (hipcc -O3): no kernel of this file uses scratch; the register / LDS figures are in profiles/bam_gpu.md.
// Bytes of the text are loaded one by one and assembled (records have no alignment); no unaligned 32-bit loads.
#ifndef MLST_BAM_DEV_H
#define MLST_BAM_DEV_H

#define BAM_CELL      32768u
#define BAM_CELL_CAP  896u                /* a record is at least 37 bytes: at most 885 starts per cell */
#define BAM_HEAD      (1u << 20)          /* head room of a text slot (the carry of the piece before) */
#define BAM_REC_MAX   (BAM_HEAD - 64u)    /* largest block_size taken: a record has to fit the head room (MLST_E_LIMIT beyond) */
#define BAM_NONE      0xFFFFFFFFu
#define BAM_BAD       0xFFFFFFFEu
// BamMeta.err
#define BAM_ERR_RECORD   1u               /* a record head that cannot be one (at a true record start) */
#define BAM_ERR_LIMIT    2u               /* a record larger than the head room */
#define BAM_ERR_LIST     3u               /* sequenceBank list full */
#define BAM_ERR_TRUNC    4u               /* the file ends inside a record */
#define BAM_ERR_INFLATE  9u               /* the piece's blocks did not inflate / failed their CRC: nothing of it is counted */
// reasons a record is left to the host path (low 4 bits of BamMeta.flag_key)
#define BAM_FLAG_UNMAPPED 1u
#define BAM_FLAG_NAME     2u
#define BAM_FLAG_FEWTAGS  3u
#define BAM_FLAG_NONINT   4u
#define BAM_FLAG_AUX      5u
#define BAM_FLAG_TAGTYPE  6u

struct BamMeta {            // device-resident, lives as long as the stream
    u64 rec_total;          // records of the pieces before this one
    u64 n_entries;          // fill of the sequenceBank list
    u64 flag_key;           // smallest (record index << 4 | reason) of a record the device does not treat (~0: none)
    u64 err_at;             // text offset the error was met at
    u32 carry_len;          // bytes in the carry buffer
    u32 entry;              // this piece: offset of its first record start in the slot
    u32 n_rec;              // this piece: whole records
    u32 carry_start;        // this piece: where the partial record at its end begins
    u32 err;                // BAM_ERR_* (sticky)
    u32 rewalked;           // cells walked again by k_bam_link (all pieces)
    u32 pad_[2];
};
struct BamEntry { u64 k0, k1, rec; u32 locus, seqlen; };      // one accepted record on a known locus: QNAME key, record index, len(SEQ)

__device__ inline u32 bam_ld16(const u8* __restrict__ p) { return (u32)p[0] | ((u32)p[1] << 8); }
__device__ inline u32 bam_ld32(const u8* __restrict__ p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

// A record head at s that can be one: its size in the text (block_size + 4), or 0.  Needs s + 36 <= text_end.
__device__ inline u32 bam_head(const u8* __restrict__ t, u32 s, u32 text_end, int n_ref) {
    const u32 bs = bam_ld32(t + s);
    if (bs < 33u || bs > BAM_REC_MAX) return 0;
    const int ref = (int)bam_ld32(t + s + 4), pos = (int)bam_ld32(t + s + 8);
    if (ref < -1 || ref >= n_ref || pos < -1) return 0;
    const u32 lrn = t[s + 12], ncig = bam_ld16(t + s + 16); const int lseq = (int)bam_ld32(t + s + 20);
    if (lrn < 1u || lseq < 0) return 0;
    const u64 need = 32ull + lrn + 4ull * ncig + ((u64)lseq + 1) / 2 + (u64)lseq;
    if (need > bs) return 0;
    const u32 nul = s + 36u + lrn - 1u;
    if (nul < text_end && t[nul] != 0) return 0;
    return bs + 4u;
}
// The chain from s inside [.., cell_end): starts go to lst (when lane_writes), returns their number; ex: the first start at or
// behind cell_end, or (below cell_end) the start of a record that the text does not hold whole, or BAM_BAD.
__device__ inline u32 bam_walk(const u8* __restrict__ t, u32 s, u32 cell_end, u32 text_end, int n_ref, u32* __restrict__ lst, bool writes, u32& ex) {
    u32 n = 0;
    for (;;) {
        if (s >= cell_end) { ex = s; break; }
        if (s + 36u > text_end) { ex = s; break; }
        const u32 tot = bam_head(t, s, text_end, n_ref);
        if (!tot) { ex = BAM_BAD; break; }
        if (s + tot > text_end) { ex = s; break; }
        if (writes && n < BAM_CELL_CAP) lst[n] = s;
        n++; s += tot;
    }
    return n < BAM_CELL_CAP ? n : BAM_CELL_CAP;
}

// the carry of the piece before goes in front of the piece's text; the piece's entry is where it begins (skip: bytes of the BAM
// header in the first block of a stream)
__global__ __launch_bounds__(256) void k_bam_carry_in(u8* __restrict__ text, const u8* __restrict__ carry, BamMeta* __restrict__ meta, u32 skip) {
    const u32 len = meta->carry_len;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) text[BAM_HEAD - len + i] = carry[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) meta->entry = BAM_HEAD - len + skip;
}

__global__ __launch_bounds__(256) void k_bam_cells(const u8* __restrict__ text, u32 text_end, u32 n_cells, int n_ref, const BamMeta* __restrict__ meta,
                                                   u32* __restrict__ first, u32* __restrict__ exit_, u32* __restrict__ count, u32* __restrict__ list, u32 force_miss) {
    __shared__ u32 s_min;
    const u32 entry = meta->entry;
    for (u32 k = blockIdx.x; k < n_cells; k += gridDim.x) {
        const u32 c0 = k * BAM_CELL, c1 = c0 + BAM_CELL;
        u32 guess = BAM_NONE;
        if (c1 > entry && c0 < text_end) {
            if (c0 <= entry) guess = entry;
            else {
                if (threadIdx.x == 0) s_min = BAM_NONE;
                __syncthreads();
                const u32 lim = c1 < text_end ? c1 : text_end;
                for (u32 r = c0; r < lim; r += 256u) {
                    const u32 s = r + threadIdx.x;
                    if (s < lim && s + 36u <= text_end) {
                        u32 tot = bam_head(text, s, text_end, n_ref);
                        u32 q = s;
                        for (int d = 0; tot && d < 2; d++) {         // two plausible records chained behind it (as far as the text goes)
                            q += tot;
                            if (q > text_end || q + 36u > text_end) break;
                            tot = bam_head(text, q, text_end, n_ref);
                        }
                        if (tot) atomicMin(&s_min, s);
                    }
                    __syncthreads();
                    const u32 m = s_min;
                    __syncthreads();
                    if (m != BAM_NONE) { guess = m; break; }
                }
            }
            if (force_miss && k % force_miss == force_miss - 1u) guess = BAM_NONE;      // test hook (mlst_debug_bam_split): k_bam_link has to walk the cell itself
        }
        if (threadIdx.x == 0) {
            u32 ex = BAM_NONE, n = 0;
            if (guess != BAM_NONE) n = bam_walk(text, guess, c1, text_end, n_ref, list + (u64)k * BAM_CELL_CAP, true, ex);
            first[k] = guess; exit_[k] = ex; count[k] = n;
        }
        __syncthreads();
    }
}

// One wave.  Lanes load the figures of 64 cells at a time; the decisions are taken by all lanes alike (uniform), lane 0 stores.
__global__ __launch_bounds__(64) void k_bam_link(const u8* __restrict__ text, u32 text_end, u32 n_cells, int n_ref, BamMeta* __restrict__ meta, const u32* __restrict__ infl_err,
                                                 const u32* __restrict__ first, const u32* __restrict__ exit_, u32* __restrict__ count, u32* __restrict__ base,
                                                 u32* __restrict__ list, int final_piece) {
    const int lane = threadIdx.x;
    u32 in = meta->entry, err = meta->err, total = 0, rewalked = 0, carry_start = in; u64 err_at = 0;
    if (!err && infl_err[0]) err = BAM_ERR_INFLATE;
    bool stop = err != 0;
    for (u32 k0 = 0; k0 < n_cells; k0 += 64u) {
        const u32 k = k0 + lane;
        const u32 f = k < n_cells ? first[k] : BAM_NONE, e = k < n_cells ? exit_[k] : BAM_NONE;
        u32 c = k < n_cells ? count[k] : 0u;
        const int lim = n_cells - k0 < 64u ? (int)(n_cells - k0) : 64;
        for (int i = 0; i < lim; i++) {
            const u32 c1 = (k0 + i + 1u) * BAM_CELL;
            const u32 fi = __shfl(f, i); u32 ei = __shfl(e, i);
            bool zero = stop || in >= c1;
            if (!zero) {
                if (fi != in) {
                    const u32 n = bam_walk(text, in, c1, text_end, n_ref, list + (u64)(k0 + i) * BAM_CELL_CAP, lane == 0, ei);
                    if (lane == i) c = n;
                    rewalked++;
                }
                if (ei == BAM_BAD) {      // (at a true start: the chain before it is exact)
                    u32 s = in;             // where: the chain once more, up to the record that fails
                    for (;;) { if (s + 36u > text_end) break; const u32 tot = bam_head(text, s, text_end, n_ref); if (!tot) break; s += tot; if (s >= c1) break; }
                    const u32 bs = s + 4u <= text_end ? bam_ld32(text + s) : 0u;
                    err = (bs > BAM_REC_MAX && bs < 0x80000000u) ? BAM_ERR_LIMIT : BAM_ERR_RECORD; err_at = s; stop = true; carry_start = text_end;
                } else if (ei < c1) { carry_start = ei; stop = true; in = ei; }
                else { in = ei; carry_start = ei < text_end ? ei : text_end; }
            }
            if (zero && lane == i) c = 0;
        }
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(incl, o); if (lane >= o) incl += y; }
        if (k < n_cells) { base[k] = total + incl - c; count[k] = c; }
        total += __shfl(incl, 63);
    }
    if (err) { total = 0; carry_start = text_end; for (u32 k = lane; k < n_cells; k += 64u) count[k] = 0; }
    if (carry_start > text_end) carry_start = text_end;
    if (!err && final_piece && carry_start != text_end) { err = BAM_ERR_TRUNC; err_at = carry_start; }
    if (lane == 0) {
        meta->n_rec = total; meta->carry_start = carry_start; meta->carry_len = text_end - carry_start;
        if (err && !meta->err) { meta->err = err; meta->err_at = err_at; }
        meta->rewalked += rewalked;
    }
}

// the partial record at the piece's end goes to the carry buffer; the record count moves on
__global__ __launch_bounds__(256) void k_bam_carry_out(const u8* __restrict__ text, u8* __restrict__ carry, BamMeta* __restrict__ meta) {
    const u32 len = meta->carry_len, s0 = meta->carry_start;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) carry[i] = text[s0 + i];
    if (blockIdx.x == 0 && threadIdx.x == 0) meta->rec_total += meta->n_rec;
}

// One optional field at p (p + 3 <= end checked by the caller): p moves behind it; integer types give their value.
// false: a type the reference's reader does not know, or a field that leaves the record.
__device__ inline bool bam_aux_next(const u8* __restrict__ t, u32& p, u32 end, bool& is_int, long long& val) {
    const u8 ty = t[p + 2]; p += 3; is_int = false; val = 0;
    u32 sz = 0;
    switch (ty) {
        case 'A': sz = 1; break;
        case 'c': sz = 1; if (p + 1 <= end) { val = (long long)(signed char)t[p]; is_int = true; } break;
        case 'C': sz = 1; if (p + 1 <= end) { val = (long long)t[p]; is_int = true; } break;
        case 's': sz = 2; if (p + 2 <= end) { val = (long long)(short)bam_ld16(t + p); is_int = true; } break;
        case 'S': sz = 2; if (p + 2 <= end) { val = (long long)bam_ld16(t + p); is_int = true; } break;
        case 'i': sz = 4; if (p + 4 <= end) { val = (long long)(int)bam_ld32(t + p); is_int = true; } break;
        case 'I': sz = 4; if (p + 4 <= end) { val = (long long)bam_ld32(t + p); is_int = true; } break;
        case 'f': sz = 4; break;
        case 'Z': case 'H': { u32 q = p; while (q < end && t[q]) q++; if (q >= end) return false; sz = q + 1 - p; break; }
        case 'B': {
            if (p + 5 > end) return false;
            const u8 sub = t[p]; const u32 cnt = bam_ld32(t + p + 1);
            const u32 w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            if (!w || cnt > (end - p) / w) return false;
            sz = 5u + cnt * w; break;
        }
        default: return false;
    }
    if (p + sz > end || p + sz < p) return false;
    p += sz;
    return true;
}

__device__ inline void bam_flag(BamMeta* __restrict__ meta, u64 ridx, u32 reason) { atomicMin((unsigned long long*)&meta->flag_key, (unsigned long long)((ridx << 4) | reason)); }

// ------------------------------------------------------------------ pass 1 (metamlst.py:101-130 as samin.AlignmentSample.add states it)
__global__ __launch_bounds__(256) void k_bam_accumulate(const EngineDev* __restrict__ Ep, KParams P, const u8* __restrict__ text, u32 n_cells, BamMeta* __restrict__ meta,
                                                        const u32* __restrict__ count, const u32* __restrict__ base, const u32* __restrict__ list,
                                                        const int* __restrict__ ref_allele, const int* __restrict__ ref_locus, const u8* __restrict__ ref_flags,
                                                        BamEntry* __restrict__ entries, u64 cap_entries) {
    const EngineDev& E = *Ep;
    const u64 rec_base = meta->rec_total;
    const int lane = threadIdx.x & 63;
    u32 c_tot = 0, c_ign = 0;
    for (u32 k = blockIdx.x; k < n_cells; k += gridDim.x) {
        const u32 cnt = count[k]; const u32 b = base[k];
        for (u32 j0 = 0; j0 < cnt; j0 += 256u) {
            const u32 j = j0 + threadIdx.x;
            bool want = false; BamEntry en; en.k0 = en.k1 = en.rec = 0; en.locus = en.seqlen = 0;
            if (j < cnt) {
                const u32 s = list[(u64)k * BAM_CELL_CAP + j]; const u64 ridx = rec_base + b + j;
                const u32 end = s + 4u + bam_ld32(text + s);
                const int ref = (int)bam_ld32(text + s + 4);
                const u32 lrn = text[s + 12], ncig = bam_ld16(text + s + 16), lseq = bam_ld32(text + s + 20);
                u32 p = s + 36u + lrn + 4u * ncig + (lseq + 1u) / 2u + lseq;
                u32 reason = 0; u8 fl = 0;
                if (ref < 0) reason = BAM_FLAG_UNMAPPED;
                else { fl = ref_flags[ref]; if (fl & 2u) reason = BAM_FLAG_NAME; }
                long long score = 0, xm = 0; u32 nf = 0;
                while (!reason && p < end) {
                    bool is_int; long long v;
                    if (p + 3u > end || !bam_aux_next(text, p, end, is_int, v)) { reason = BAM_FLAG_AUX; break; }
                    if (nf == 0) { if (is_int) score = v; else reason = BAM_FLAG_NONINT; }        // 12th column (metamlst.py:109)
                    else if (nf == 3) { if (is_int) xm = v; else reason = BAM_FLAG_NONINT; }      // 15th column BY POSITION (Q1, metamlst.py:110)
                    nf++;
                }
                if (!reason && nf < 4u) reason = BAM_FLAG_FEWTAGS;
                if (reason) bam_flag(meta, ridx, reason);
                else if (fl & 1u) {                                                                // species filter (metamlst.py:114)
                    const u32 seqlen = lseq ? lseq : 1u;                                           // SEQ '*' has length 1
                    c_tot++;
                    if (score >= (long long)P.minscore && (long long)seqlen >= (long long)P.min_read_len && xm <= (long long)P.max_xm) {
                        const int a = ref_allele[ref], l = ref_locus[ref];
                        if (a >= 0) { atomicAdd((u64*)&E.sum_score[a], (u64)score); atomicAdd(&E.n_hits[a], 1u); }
                        if (l >= 0) {
                            atomicMin(&E.locus_first[l], ridx);
                            u64 h0 = 0xcbf29ce484222325ull, h1 = 0x9E3779B97F4A7C15ull;
                            for (u32 i = 0; i + 1u < lrn; i++) {
                                const u64 ch = text[s + 36u + i];
                                h0 = (h0 ^ ch) * 0x100000001b3ull;
                                h1 = (h1 + ch + 1u) * 0xff51afd7ed558ccdull; h1 ^= h1 >> 29;
                            }
                            en.k0 = h0; en.k1 = h1 ^ ((u64)lrn << 56); en.rec = ridx; en.locus = (u32)l; en.seqlen = seqlen; want = true;
                        }
                    } else c_ign++;
                }
            }
            const u64 m = __ballot(want);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                u64 at = 0;
                if (lane == leader) at = atomicAdd((unsigned long long*)&meta->n_entries, (unsigned long long)__popcll(m));
                at = ((u64)(u32)__shfl((int)(at >> 32), leader) << 32) | (u64)(u32)__shfl((int)at, leader);
                if (want) {
                    at += (u64)__popcll(m & ((1ull << lane) - 1ull));
                    if (at < cap_entries) entries[at] = en; else atomicCAS(&meta->err, 0u, BAM_ERR_LIST);
                }
            }
        }
    }
    c_tot = wave_sum_u32(c_tot); c_ign = wave_sum_u32(c_ign);
    if (lane == 0) {
        if (c_tot) atomicAdd(&E.ctr->cnt[MLST_CNT_TOTAL_RECORDS], (u64)c_tot);
        if (c_ign) atomicAdd(&E.ctr->cnt[MLST_CNT_IGNORED], (u64)c_ign);
    }
}

// ------------------------------------------------------------------ sequenceBank (metamlst.py:127)
// The list is sorted by record index, then (stable) by a 64-bit mix of (locus, QNAME key): inside a run of equal mixes the records
// of one (locus, QNAME) stand in file order, so an entry is the dictionary's final value iff no entry of the same full key follows it.
__device__ inline u64 bam_mix(const BamEntry& e) {
    u64 x = e.k0 ^ (e.k1 * 0x9E3779B97F4A7C15ull) ^ ((u64)e.locus * 0xD6E8FEB86659FD93ull);
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}
__global__ __launch_bounds__(256) void k_bam_bank_keys(const BamEntry* __restrict__ entries, u64 n, u64* __restrict__ keys, u32* __restrict__ idx) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) { keys[i] = entries[i].rec; idx[i] = (u32)i; }
}
__global__ __launch_bounds__(256) void k_bam_bank_mix(const BamEntry* __restrict__ entries, u64 n, const u32* __restrict__ idx, u64* __restrict__ keys) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) keys[i] = bam_mix(entries[idx[i]]);
}
__global__ __launch_bounds__(256) void k_bam_bank_sum(const EngineDev* __restrict__ Ep, const BamEntry* __restrict__ entries, u64 n, const u32* __restrict__ idx, const u64* __restrict__ keys) {
    const EngineDev& E = *Ep;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const BamEntry e = entries[idx[i]]; const u64 key = keys[i];
        bool last = true;
        for (u64 m = i + 1; m < n && keys[m] == key; m++) {
            const BamEntry f = entries[idx[m]];
            if (f.locus == e.locus && f.k0 == e.k0 && f.k1 == e.k1) { last = false; break; }
        }
        if (last) atomicAdd(&E.locus_len[e.locus], (u64)e.seqlen);
    }
}

// ------------------------------------------------------------------ pass 2 (k_pileup_aln from the records in place)
// AS / XM by NAME among the optional fields (cmseq's BAM_tagFilter; the last occurrence wins, an absent one fails the test).
__global__ __launch_bounds__(256) void k_bam_pileup(const u8* __restrict__ text, u32 n_cells, BamMeta* __restrict__ meta, const u32* __restrict__ count, const u32* __restrict__ base,
                                                    const u32* __restrict__ list, const int* __restrict__ ref_allele, const int* __restrict__ allele_slot,
                                                    const u64* __restrict__ aoff, int minscore, int max_xm, int minqual, u32* __restrict__ counts) {
    const u64 rec_base = meta->rec_total;
    for (u32 k = blockIdx.x; k < n_cells; k += gridDim.x) {
        const u32 cnt = count[k]; const u32 b = base[k];
        for (u32 j = threadIdx.x; j < cnt; j += 256u) {
            const u32 s = list[(u64)k * BAM_CELL_CAP + j];
            const int ref = (int)bam_ld32(text + s + 4);
            if (ref < 0) continue;
            const int a = ref_allele[ref];
            if (a < 0) continue;
            const int cb = allele_slot[a];
            if (cb < 0) continue;
            const u32 end = s + 4u + bam_ld32(text + s);
            const u32 lrn = text[s + 12], ncig = bam_ld16(text + s + 16), lseq = bam_ld32(text + s + 20);
            const u32 cig0 = s + 36u + lrn, seq0 = cig0 + 4u * ncig, q0 = seq0 + (lseq + 1u) / 2u;
            u32 p = q0 + lseq;
            long long as_ = -(1ll << 40), xm = (1ll << 40); bool bad = false;
            while (p < end) {
                if (p + 3u > end) { bad = true; break; }
                const u32 t0 = text[p], t1 = text[p + 1]; bool is_int; long long v;
                if (!bam_aux_next(text, p, end, is_int, v)) { bad = true; break; }
                if (t0 == 'A' && t1 == 'S') { if (is_int) as_ = v; else { bad = true; break; } }
                else if (t0 == 'X' && t1 == 'M') { if (is_int) xm = v; else { bad = true; break; } }
            }
            if (bad) { bam_flag(meta, rec_base + b + j, BAM_FLAG_TAGTYPE); continue; }
            if (as_ < (long long)minscore || xm > (long long)max_xm) continue;
            const long long alen = (long long)(aoff[a + 1] - aoff[a]);
            const bool noq = lseq && text[q0] == 0xFF;
            long long r = (long long)(int)bam_ld32(text + s + 8); u32 q = 0;
            for (u32 c = 0; c < ncig; c++) {
                const u32 w = bam_ld32(text + cig0 + 4u * c), ln = w >> 4, op = w & 15u;
                if (op == 0 || op == 7 || op == 8) {
                    for (u32 t = 0; t < ln && q + t < lseq; t++) {
                        const u32 at = q + t; const u32 nib = (text[seq0 + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 15u;
                        const int bc = nib == 1 ? 0 : nib == 2 ? 1 : nib == 4 ? 2 : nib == 8 ? 3 : -1;
                        const int ph = noq ? 0 : (int)text[q0 + at];
                        const long long col = r + t;
                        if (bc >= 0 && ph >= minqual && col >= 0 && col < alen) atomicAdd(&counts[((u64)cb + (u64)col) * 4 + bc], 1u);
                    }
                    r += ln; q += ln;
                } else if (op == 1 || op == 4) q += ln;
                else if (op == 2 || op == 3) r += ln;
            }
        }
    }
}

#endif
