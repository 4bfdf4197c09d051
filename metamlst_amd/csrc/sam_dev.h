// sam_dev.h -- SAM text on the device (included by mlst_engine.hip behind bam_dev.h, whose stream state, list and reasons' key it shares).
//
// A chunk of SAM text lies in a text slot behind BAM_HEAD bytes of head room; the partial line the chunk before left over is copied
// in front of it.  Line starts come from the newline table of the FASTQ parser (k_fq_count / k_fq_scan / k_fq_lines), from the
// 4,096-byte block the first line begins in.  One thread per line does the rest:
//   k_sam_flags      : per 256 lines the number of record lines (first byte not '@'); scanned by k_fq_scan: the record index of a
//                      line is the number of record lines in front of it, counted across chunks (AlignmentSample.n_records there)
//   k_sam_accumulate : pass 1, metamlst.py:101-130 as samin.AlignmentSample.add states it, from the line in place
//   k_sam_pileup     : pass 2, what k_pileup_aln does, from the line in place
// The list of pass 1 is bam_dev.h's (BamEntry, same QNAME key): k_bam_bank_* run unchanged at the end of the stream.
// A line the device cannot treat exactly as the host reader would is never guessed: the smallest record index with its reason
// goes to BamMeta.flag_key (bam_flag), and the caller runs the host reader.
// gfx950 build (hipcc -O3): no kernel of this file uses scratch; the register / LDS figures are in profiles/sam_gpu.md.
// Bytes of a line are loaded one by one (lines have no alignment).
#ifndef MLST_SAM_DEV_H
#define MLST_SAM_DEV_H

// reasons a line is left to the host path (low 4 bits of BamMeta.flag_key)
#define SAM_FLAG_CR        1u      /* a CR that does not stand directly in front of an LF (Python ends a line there) */
#define SAM_FLAG_BYTE      2u      /* a byte >= 0x80 or a NUL in a record line */
#define SAM_FLAG_COLUMNS   3u      /* fewer than 15 columns */
#define SAM_FLAG_INT       4u      /* FLAG, POS, the 12th or the 15th column's value not -?[0-9]{1,9} */
#define SAM_FLAG_RNAME     5u      /* RNAME not among the header's @SQ names (or *) */
#define SAM_FLAG_NAME      6u      /* a contig name that does not split in three at '_' */
#define SAM_FLAG_TAG       7u      /* AS / XM found by name on a loaded contig, value not such an integer */
#define SAM_FLAG_CIGAR     8u      /* a CIGAR byte that is neither a digit nor one of MIDNSHP=X (loaded contig) */
#define SAM_FLAG_CIGLEN    9u      /* a CIGAR operation of 2^28 bases or more (loaded contig) */
#define SAM_FLAG_QUALLEN   10u     /* pass 2, loaded contig: QUAL neither * nor as long as SEQ */
#define SAM_FLAG_QUALBYTE  11u     /* pass 2, chosen contig: a QUAL byte below 33 */

// the header's names: an open-addressing table built on the host (capacity a power of two, at least 2 * n_ref; slot = index + 1,
// 0 = empty), the names themselves behind it: a hit is confirmed by length and bytes
struct SamNames { const u32* htab; const u32* off; const u8* arena; u32 mask; };
__host__ __device__ inline u32 sam_name_hash(const u8* p, u32 n) {
    u32 x = 0x811C9DC5u;
    for (u32 i = 0; i < n; i++) x = (x ^ p[i]) * 0x01000193u;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12;
    return x;
}
__device__ inline int sam_ref_lookup(const u8* __restrict__ t, u32 a, u32 b, const SamNames& N) {
    const u32 n = b - a;
    u32 slot = sam_name_hash(t + a, n) & N.mask;
    for (u32 probe = 0; probe <= N.mask; probe++) {
        const u32 v = N.htab[slot];
        if (!v) return -1;
        const u32 o = N.off[v - 1];
        if (N.off[v] - o == n) {
            u32 i = 0;
            while (i < n && N.arena[o + i] == t[a + i]) i++;
            if (i == n) return (int)(v - 1);
        }
        slot = (slot + 1u) & N.mask;
    }
    return -1;
}

// line i of the table: [s, e) without its LF; lf: the line ends with one (the last line of the final chunk need not)
__device__ inline void sam_line(const u64* __restrict__ lines, u32 n_nl, u32 nb, u32 i, u32& s, u32& e, bool& lf) {
    s = (u32)lines[i]; lf = i < n_nl; e = lf ? (u32)lines[i + 1] - 1u : nb;
}
__device__ inline bool sam_is_record(const u8* __restrict__ t, u32 s, u32 e) { return !(e > s && t[s] == (u8)'@'); }

// positions of the tabs that end columns 1-6, 9-12, 14, 15 (t15: the line's end when it has exactly 15 columns)
struct SamCols { u32 t1, t2, t3, t4, t5, t6, t9, t10, t11, t12, t14, t15, ntab; };
// The bytes of a line once: the CR of a CRLF leaves e; returns a SAM_FLAG_* or 0.  record: columns are cut and bytes are checked.
__device__ inline u32 sam_scan(const u8* __restrict__ t, u32 s, u32& e, bool lf, bool record, SamCols& L) {
    if (lf && e > s && t[e - 1] == (u8)'\r') e--;
    u32 ntab = 0; bool cr = false, odd = false;
    L.t1 = L.t2 = L.t3 = L.t4 = L.t5 = L.t6 = L.t9 = L.t10 = L.t11 = L.t12 = L.t14 = L.t15 = e;
    for (u32 p = s; p < e; p++) {
        const u8 c = t[p];
        if (c == (u8)'\r') cr = true;
        else if (record) {
            if (c == (u8)'\t') {
                ntab++;
                switch (ntab) {
                    case 1: L.t1 = p; break;   case 2: L.t2 = p; break;   case 3: L.t3 = p; break;   case 4: L.t4 = p; break;
                    case 5: L.t5 = p; break;   case 6: L.t6 = p; break;   case 9: L.t9 = p; break;   case 10: L.t10 = p; break;
                    case 11: L.t11 = p; break; case 12: L.t12 = p; break; case 14: L.t14 = p; break; case 15: L.t15 = p; break;
                    default: break;
                }
            } else if (c == 0 || c >= 0x80u) odd = true;
        }
    }
    L.ntab = ntab;
    if (cr) return SAM_FLAG_CR;
    if (odd) return SAM_FLAG_BYTE;
    if (record && ntab < 14u) return SAM_FLAG_COLUMNS;
    return 0;
}
// -?[0-9]{1,9} in [a, b): what Python's int() and the device agree on
__device__ inline bool sam_int(const u8* __restrict__ t, u32 a, u32 b, int& v) {
    bool neg = false;
    if (a < b && t[a] == (u8)'-') { neg = true; a++; }
    if (b <= a || b - a > 9u) return false;
    int x = 0;
    for (; a < b; a++) { const u32 d = (u32)t[a] - 48u; if (d > 9u) return false; x = x * 10 + (int)d; }
    v = neg ? -x : x;
    return true;
}
// split(":")[2] of the column [a, b): the text between the second colon and the third colon or the column's end; false: fewer than two colons
__device__ inline bool sam_tag_value(const u8* __restrict__ t, u32 a, u32 b, u32& va, u32& vb) {
    u32 p = a;
    while (p < b && t[p] != (u8)':') p++;
    if (p >= b) return false;
    p++;
    while (p < b && t[p] != (u8)':') p++;
    if (p >= b) return false;
    p++; va = p;
    while (p < b && t[p] != (u8)':') p++;
    vb = p;
    return true;
}
// AS / XM by NAME among the columns from the 12th on (samin.AlignmentSample.add: a column counts when it holds two colons and its
// first part is the tag; the last occurrence wins, and int() is taken of that one alone).  false: a value that is no such integer.
__device__ inline bool sam_tags(const u8* __restrict__ t, u32 from, u32 e, int& as_, int& xm) {
    u32 as0 = 0, as1 = 0, xm0 = 0, xm1 = 0; bool has_as = false, has_xm = false;
    u32 cs = from;
    while (cs <= e) {
        u32 ce = cs;
        while (ce < e && t[ce] != (u8)'\t') ce++;
        if (ce - cs >= 4u && t[cs + 2] == (u8)':') {
            const u8 c0 = t[cs], c1 = t[cs + 1]; u32 va, vb;
            if (c0 == (u8)'A' && c1 == (u8)'S') { if (sam_tag_value(t, cs, ce, va, vb)) { as0 = va; as1 = vb; has_as = true; } }
            else if (c0 == (u8)'X' && c1 == (u8)'M') { if (sam_tag_value(t, cs, ce, va, vb)) { xm0 = va; xm1 = vb; has_xm = true; } }
        }
        cs = ce + 1u;
    }
    as_ = -(1 << 30); xm = 1 << 30;
    if (has_as && !sam_int(t, as0, as1, as_)) return false;
    if (has_xm && !sam_int(t, xm0, xm1, xm)) return false;
    return true;
}
// the CIGAR text [a, b) as samin.parse_cigar reads it: 0, or the reason the host reader is needed
__device__ inline u32 sam_cigar_check(const u8* __restrict__ t, u32 a, u32 b) {
    if (b - a == 1u && t[a] == (u8)'*') return 0;
    u64 n = 0;
    for (u32 p = a; p < b; p++) {
        const u8 c = t[p]; const u32 d = (u32)c - 48u;
        if (d <= 9u) { n = n * 10u + d; if (n > (1ull << 40)) n = 1ull << 40; continue; }
        if (!(c == 'M' || c == 'I' || c == 'D' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == '=' || c == 'X')) return SAM_FLAG_CIGAR;
        if (n >= (1ull << 28)) return SAM_FLAG_CIGLEN;
        n = 0;
    }
    return 0;
}
// what both passes ask of a record line before they use it: columns, integers, the contig.  Returns a SAM_FLAG_* or 0.
__device__ inline u32 sam_record(const u8* __restrict__ t, u32 s, u32& e, bool lf, SamCols& L, const SamNames& N, const u8* __restrict__ ref_flags,
                                 int& ref, int& pos, int& score, int& xm15) {
    u32 reason = sam_scan(t, s, e, lf, true, L);
    if (reason) return reason;
    int flag; u32 va, vb;
    if (!sam_int(t, L.t1 + 1u, L.t2, flag) || !sam_int(t, L.t3 + 1u, L.t4, pos)) return SAM_FLAG_INT;
    if (!sam_tag_value(t, L.t11 + 1u, L.t12, va, vb) || !sam_int(t, va, vb, score)) return SAM_FLAG_INT;      // 12th column (metamlst.py:109)
    if (!sam_tag_value(t, L.t14 + 1u, L.t15, va, vb) || !sam_int(t, va, vb, xm15)) return SAM_FLAG_INT;       // 15th column BY POSITION (Q1, metamlst.py:110)
    ref = sam_ref_lookup(t, L.t2 + 1u, L.t3, N);
    if (ref < 0) return SAM_FLAG_RNAME;
    if (ref_flags[ref] & 2u) return SAM_FLAG_NAME;
    return 0;
}

// ------------------------------------------------------------------ the record index
__global__ __launch_bounds__(256) void k_sam_flags(const u8* __restrict__ t, u32 nb, const u64* __restrict__ lines, u32 n_lines, u32 n_nl, u32* __restrict__ wg_count) {
    __shared__ u32 s_c[4];
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    bool rec = false;
    if (i < n_lines) { u32 s, e; bool lf; sam_line(lines, n_nl, nb, i, s, e, lf); rec = sam_is_record(t, s, e); }
    const u32 c = (u32)__popcll(__ballot(rec));
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) wg_count[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}
// record lines in front of this thread's line inside its 256 lines (every thread of the workgroup calls it)
__device__ inline u32 sam_rank(bool rec, u32* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 m = __ballot(rec);
    __syncthreads();                                   // (the turn before has read s_w)
    if (lane == 0) s_w[wv] = (u32)__popcll(m);
    __syncthreads();
    u32 before = (u32)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; w++) before += s_w[w];
    return before;
}

// ------------------------------------------------------------------ pass 1 (metamlst.py:101-130 as samin.AlignmentSample.add states it)
__global__ __launch_bounds__(256) void k_sam_accumulate(const EngineDev* __restrict__ Ep, KParams P, const u8* __restrict__ t, u32 nb, const u64* __restrict__ lines, u32 n_lines,
                                                        u32 n_nl, const u32* __restrict__ wg_excl, u64 rec_base, BamMeta* __restrict__ meta, SamNames N,
                                                        const int* __restrict__ ref_allele, const int* __restrict__ ref_locus, const u8* __restrict__ ref_flags,
                                                        BamEntry* __restrict__ entries, u64 cap_entries) {
    __shared__ u32 s_w[4];
    const EngineDev& E = *Ep;
    const int lane = threadIdx.x & 63;
    const u32 n_wg = (n_lines + 255u) / 256u;
    u32 c_tot = 0, c_ign = 0;
    for (u32 k = blockIdx.x; k < n_wg; k += gridDim.x) {
        const u32 i = k * 256u + threadIdx.x;
        u32 s = 0, e = 0; bool lf = false, rec = false;
        if (i < n_lines) { sam_line(lines, n_nl, nb, i, s, e, lf); rec = sam_is_record(t, s, e); }
        const u64 ridx = rec_base + wg_excl[k] + sam_rank(rec, s_w);
        bool want = false; BamEntry en; en.k0 = en.k1 = en.rec = 0; en.locus = en.seqlen = 0;
        if (i < n_lines) {
            SamCols L; u32 reason = 0;
            if (e - s > BAM_REC_MAX) atomicCAS(&meta->err, 0u, BAM_ERR_LIMIT);
            else if (!rec) reason = sam_scan(t, s, e, lf, false, L);
            else {
                int ref = -1, pos = 0, score = 0, xm = 0;
                reason = sam_record(t, s, e, lf, L, N, ref_flags, ref, pos, score, xm);
                if (!reason) {
                    const int a = ref_allele[ref], l = ref_locus[ref];
                    if (a >= 0) {      // (a loaded contig: the host reader keeps the record for the pile-up and reads its true tags and its CIGAR)
                        int as_, xm_;
                        if (!sam_tags(t, L.t11 + 1u, e, as_, xm_)) reason = SAM_FLAG_TAG;
                        else reason = sam_cigar_check(t, L.t5 + 1u, L.t6);
                    }
                    if (!reason && (ref_flags[ref] & 1u)) {                                        // species filter (metamlst.py:114)
                        const u32 seqlen = L.t10 - (L.t9 + 1u);                                    // len(SEQ) in bytes: '*' counts 1
                        c_tot++;
                        if (score >= P.minscore && (long long)seqlen >= (long long)P.min_read_len && xm <= P.max_xm) {
                            if (a >= 0) { atomicAdd((u64*)&E.sum_score[a], (u64)(long long)score); atomicAdd(&E.n_hits[a], 1u); }
                            if (l >= 0) {
                                atomicMin(&E.locus_first[l], ridx);
                                u64 h0 = 0xcbf29ce484222325ull, h1 = 0x9E3779B97F4A7C15ull;
                                for (u32 p = s; p < L.t1; p++) {
                                    const u64 ch = t[p];
                                    h0 = (h0 ^ ch) * 0x100000001b3ull;
                                    h1 = (h1 + ch + 1u) * 0xff51afd7ed558ccdull; h1 ^= h1 >> 29;
                                }
                                en.k0 = h0; en.k1 = h1 ^ ((u64)(L.t1 - s + 1u) << 56); en.rec = ridx; en.locus = (u32)l; en.seqlen = seqlen; want = true;
                            }
                        } else c_ign++;
                    }
                }
            }
            if (reason) bam_flag(meta, ridx, reason);
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
    c_tot = wave_sum_u32(c_tot); c_ign = wave_sum_u32(c_ign);
    if (lane == 0) {
        if (c_tot) atomicAdd(&E.ctr->cnt[MLST_CNT_TOTAL_RECORDS], (u64)c_tot);
        if (c_ign) atomicAdd(&E.ctr->cnt[MLST_CNT_IGNORED], (u64)c_ign);
    }
}

// ------------------------------------------------------------------ pass 2 (k_pileup_aln from the lines in place)
__global__ __launch_bounds__(256) void k_sam_pileup(const u8* __restrict__ t, u32 nb, const u64* __restrict__ lines, u32 n_lines, u32 n_nl, const u32* __restrict__ wg_excl,
                                                    u64 rec_base, BamMeta* __restrict__ meta, SamNames N, const int* __restrict__ ref_allele, const u8* __restrict__ ref_flags,
                                                    const int* __restrict__ allele_slot, const u64* __restrict__ aoff, int minscore, int max_xm, int minqual,
                                                    u32* __restrict__ counts) {
    __shared__ u32 s_w[4];
    const u32 n_wg = (n_lines + 255u) / 256u;
    for (u32 k = blockIdx.x; k < n_wg; k += gridDim.x) {
        const u32 i = k * 256u + threadIdx.x;
        u32 s = 0, e = 0; bool lf = false, rec = false;
        if (i < n_lines) { sam_line(lines, n_nl, nb, i, s, e, lf); rec = sam_is_record(t, s, e); }
        const u64 ridx = rec_base + wg_excl[k] + sam_rank(rec, s_w);
        if (i >= n_lines) continue;
        SamCols L;
        if (e - s > BAM_REC_MAX) { atomicCAS(&meta->err, 0u, BAM_ERR_LIMIT); continue; }
        if (!rec) { const u32 reason = sam_scan(t, s, e, lf, false, L); if (reason) bam_flag(meta, ridx, reason); continue; }
        int ref = -1, pos = 0, score = 0, xm15 = 0;
        u32 reason = sam_record(t, s, e, lf, L, N, ref_flags, ref, pos, score, xm15);
        if (reason) { bam_flag(meta, ridx, reason); continue; }
        const int a = ref_allele[ref];
        if (a < 0) continue;
        int as_, xm;
        const u32 cig0 = L.t5 + 1u, cig1 = L.t6, seq0 = L.t9 + 1u, q0 = L.t10 + 1u;
        const u32 nseq = L.t10 - seq0, nq = L.t11 - q0;
        const bool noq = nq == 1u && t[q0] == (u8)'*';
        if (!sam_tags(t, L.t11 + 1u, e, as_, xm)) reason = SAM_FLAG_TAG;
        else if ((reason = sam_cigar_check(t, cig0, cig1)) != 0) {}
        else if (!noq && nq != nseq) reason = SAM_FLAG_QUALLEN;
        if (reason) { bam_flag(meta, ridx, reason); continue; }
        const int cb = allele_slot[a];
        if (cb < 0) continue;
        if (!noq) {
            bool low = false;
            for (u32 p = q0; p < L.t11; p++) low |= t[p] < 33u;
            if (low) { bam_flag(meta, ridx, SAM_FLAG_QUALBYTE); continue; }
        }
        if (as_ < minscore || xm > max_xm) continue;
        const u32 lseq = (nseq == 1u && t[seq0] == (u8)'*') ? 0u : nseq;
        if (cig1 - cig0 == 1u && t[cig0] == (u8)'*') continue;      // no operation
        const long long alen = (long long)(aoff[a + 1] - aoff[a]);
        long long r = (long long)pos - 1; u64 q = 0; u32 n = 0;
        for (u32 p = cig0; p < cig1; p++) {
            const u8 c = t[p]; const u32 d = (u32)c - 48u;
            if (d <= 9u) { n = n * 10u + d; continue; }      // (below 2^28 at every operation: sam_cigar_check)
            const u32 ln = n; n = 0;
            if (c == 'M' || c == '=' || c == 'X') {
                for (u32 j = 0; j < ln && q + j < lseq; j++) {
                    const u32 at = (u32)q + j; const u8 ch = t[seq0 + at] & 0xDF;      // upper case
                    const int bc = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
                    const int ph = noq ? 0 : (int)t[q0 + at] - 33;
                    const long long col = r + j;
                    if (bc >= 0 && ph >= minqual && col >= 0 && col < alen) atomicAdd(&counts[((u64)cb + (u64)col) * 4 + bc], 1u);
                }
                r += ln; q += ln;
            } else if (c == 'I' || c == 'S') q += ln;
            else if (c == 'D' || c == 'N') r += ln;
        }
    }
}

#endif
