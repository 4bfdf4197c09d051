// aln_text.h -- every alignment of the sample as SAM text, written on the device (mlst_alignments_text_open / _next / _close; the rule:
// include/mlst.h and metamlst_amd/samout.py, `cli type --write-sam-all`).  Included by mlst_engine.hip behind aln_export.h.
//
// One record per (work item, allele of the item's locus) that pass 1 counts: the pair is decided as pass 1 decides it (the ungapped
// alignment, or the banded one when gap_trigger fires; a record iff score >= floor_tab[n] && score > 0).  The host sorts the item
// list by (read index, locus, strand, diag) and cuts it into rounds at read boundaries against the caller's byte budget (a bound
// from above on every line: at_line_bound); a round is one pass of these kernels over its items.  Nothing of the sample's state is
// written.
//   k_at_decide_160 / _320  one wave per item, lanes = alleles in passes of 64: the read's planes staged once (stage_read_planes), its
//                 letters rendered once into LDS, ungapped_planes<., true, .> and gap_trigger per lane.  Leaves every pair's AtPair
//                 (record or not, AS, XM, span, the width of its CIGAR text, NM); the wave counts the M columns of a record whose SEQ
//                 letter is not the allele's, 64 columns per turn.  Pairs whose trigger fired go on an (item, allele) list.
//   k_at_dp<false> one lane per listed pair, 64 x 64 lanes on the traceback store of k_pileup_dp: banded<true>, then the walk of
//                 k_ax_dp from the best cell back to the start.  Fills the pair's AtPair (and XO, XG, NM from the walk).
//   k_at_reads    one wave per read over the pairs of its consecutive items: the records, the best AS and the first pair that holds it,
//                 the best AS among the others; then the exact byte length of every record's line (at_line<false>) into the table
//                 that k_at_local / k_fqt_scan / k_fqt_add turn into the lines' offsets in the text.
//   k_at_write    one wave per item: SEQ and QUAL rendered once into LDS; per pass of 64 alleles every lane formats the other columns
//                 of its record (at_line<true>), then the wave copies SEQ and QUAL into each record, four bytes per lane and store.
// QNAME: r<k>, or with mlst_set_read_names the read's own name out of the name arena (at_qname; csrc/read_names.h).
//   k_at_dp<true> the banded alignment and the walk again for the listed pairs that have a record: the CIGAR text, written from its
//                 last character down (the walk meets the runs last to first).
// MD:Z (mlst_set_export_md; the rule: samout.md_text): a template parameter of every kernel above, as NAMES is -- without it the kernels
//   are the ones they were.  With it k_at_decide / k_at_dp<false> also leave the width of every pair's MD text (AtDev::mdw, a table that
//   exists only then), at_line places the field between NM:i and YT:Z, k_at_md writes an ungapped record's text on the walk that counted
//   it and k_at_dp<true> a banded record's from its last character down.
// Plain vector stores only.
#ifndef MLST_ALN_TEXT_H
#define MLST_ALN_TEXT_H

#define AT_REC  1u      /* the pair has a record */
#define AT_DP   2u      /* the banded alignment was taken */
#define AT_PEND 4u      /* gap_trigger fired: the pair waits for k_at_dp */

struct AtPair { int as, pos0; u16 be, cigw, nm, xg; u8 xm, xo, flags, pad_; };      // 20 bytes per (item, allele) of a round
struct AtRead { u64 best_pair; u32 nrec; int best_as, other_as; };                  // per read of a round (best_pair: index in the round)
struct AtDev {          // device-resident descriptor of an export (uploaded by mlst_alignments_text_open)
    GP<const u32> perm;         // sorted position -> work item
    GP<const u64> pair_off;     // sorted position -> pairs in front of it (n_items + 1 entries)
    GP<const u32> item_read;    // sorted position -> its read's number in the sorted list
    GP<const u64> read_first;   // read number -> sorted position of its first item (n_reads + 1 entries)
    GP<const u8> names; GP<const u64> name_off;      // RNAME labels of the loaded alleles
    GP<const u8> ascii; GP<const u64> aoff;          // the alleles' text
    GP<AtPair> meta; GP<AtRead> reads; GP<u64> wex; GP<u64> gsum; GP<u64> dp_list; GP<u64> dp_n; GP<u64> n_rec;
    int paired;
    GP<const u8> rn_bytes; GP<const u64> rn_off; GP<const u16> rn_len;      // the retained reads' names (csrc/read_names.h); NULL: mlst_set_read_names is off
    GP<u16> mdw;                // per pair of a round: the bytes of its MD:Z text; NULL: mlst_set_export_md is off (the table exists only with it)
};
struct AtRound { u64 k0, k1, r0, r1, pb, n_pairs; };      // sorted positions, reads and first pair of a round

__host__ __device__ inline u32 at_digits32(u32 v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__host__ __device__ inline u32 at_digits64(u64 v) {
    if (v < (1ull << 32)) return at_digits32((u32)v);
    u32 d = 10; v /= 10000000000ull;
    while (v) { d++; v /= 10; }
    return d;
}
// A bound from above on the bytes of one record's line for a read of n bases and RNAMEs of at most max_name bytes (the round planner).
// Columns 1-5 and 7-9: QNAME max_qname (r + 20 digits, or the longest kept name where that is longer), FLAG 3, RNAME, POS 10, 255, *, 0, 0 and their TABs; CIGAR: a run holds a column at the least
// and its text (digits + letter) is no longer than twice its columns, S / M / I runs hold n read bases together (2 n), and at most
// n + 1 D runs of at most five digits stand between them (6 (n + 1)); SEQ and QUAL with their TABs 2 n + 2; six integer tags of at
// most 17 bytes with their TABs, XN:i:0, YT:Z:UU and the LF.
// With mlst_set_export_md the field TAB MD:Z: (6 bytes) and its text.  The text holds, per break (a mismatching M column or a D run), the
// digits of the match run in front of it -- no more than 1 + the run's columns -- and one byte (the letter, or ^), one byte per D
// column, and the digits of the last run (5 at the most: a run is shorter than 2^15): at most 2 M + 2 R + D + 5 bytes for M M columns,
// R D runs and D D columns.  What the scoring leaves a record (score > 0, local): every M, I and S column holds a read base, so
// M + I <= n; a gap run costs gap_open + gap_ext, which mlst_create admits only with 5 match_bonus <= 2 (gap_open + gap_ext), and a
// column earns match_bonus at the most, so 2.5 R match_bonus < M match_bonus: R < 0.4 M; gap_ext may be 0, so the scores do not bound
// D, the band does: a D column moves the walk one band cell down and an I column one up inside 2 band_w + 1 cells, so
// D <= I + 2 band_w <= I + 2 MAX_W.  Together: 2 M + 0.8 M + I + 2 MAX_W + 5 <= 3 n + 2 MAX_W + 5 (an ungapped record: 2 n + 5).
__host__ __device__ inline u64 at_md_bound(u32 n) { return 3ull * n + 2ull * MAX_W + 5ull + 6ull; }
__host__ __device__ inline u64 at_line_bound(u32 n, u64 max_name, u64 max_qname = 21, bool md = false) {
    return 10ull * n + max_name + 171ull + (max_qname > 21 ? max_qname : 21ull) + (md ? at_md_bound(n) : 0ull);
}

// The columns of a line, either counted (WRITE = false) or written.  SEQ, QUAL and a banded record's CIGAR are left out: their bytes are
// counted and, when writing, skipped -- the wave and k_at_dp<true> write them.
template <bool WRITE> struct AtOut {
    u8* p; u64 n;
    __device__ inline void ch(char c) { if (WRITE) p[n] = (u8)c; n++; }
    __device__ inline void dec32(u32 v) {
        const u32 d = at_digits32(v);
        if (WRITE) { for (int i = (int)d - 1; i >= 0; i--) { p[n + i] = (u8)('0' + v % 10u); v /= 10u; } }
        n += d;
    }
    __device__ inline void dec64(u64 v) {
        if (v < (1ull << 32)) { dec32((u32)v); return; }
        const u32 d = at_digits64(v);
        if (WRITE) { for (int i = (int)d - 1; i >= 0; i--) { p[n + i] = (u8)('0' + (u32)(v % 10ull)); v /= 10ull; } }
        n += d;
    }
    __device__ inline void tag(char a, char b, u32 v) { ch('\t'); ch(a); ch(b); ch(':'); ch('i'); ch(':'); dec32(v); }
    __device__ inline void skip(u64 k) { n += k; }
};
// the QNAME of a retained read: its kept name (len bytes at p), or len = 0: r<k> (the switch is off, or the name is no legal QNAME)
// NAMES = false is the export without the switch: no load, and at_head's branch folds away -- the kernels are the ones they were
struct AtQn { GP<const u8>::G* p; u32 len; };
template <bool NAMES>
__device__ inline AtQn at_qname(const AtDev& D, u32 ret) {
    AtQn q; q.p = nullptr; q.len = 0;
    if (NAMES) { q.len = D.rn_len[ret]; q.p = D.rn_bytes.g() + D.rn_off[ret]; }
    return q;
}
// bytes in front of the CIGAR column: QNAME, FLAG, RNAME, POS, MAPQ and their TABs
template <bool WRITE>
__device__ inline void at_head(AtOut<WRITE>& o, u64 qname, AtQn qn, u32 flag, GP<const u8>::G* name, u32 name_len, int pos0) {
    if (qn.len) {
        if (WRITE) for (u32 i = 0; i < qn.len; i++) o.p[o.n + i] = qn.p[i];
        o.n += qn.len;
    } else { o.ch('r'); o.dec64(qname); }
    o.ch('\t'); o.dec32(flag); o.ch('\t');
    if (WRITE) for (u32 i = 0; i < name_len; i++) o.p[o.n + i] = name[i];
    o.n += name_len;
    o.ch('\t'); o.dec32((u32)(pos0 + 1)); o.ch('\t'); o.ch('2'); o.ch('5'); o.ch('5'); o.ch('\t');
}
// the whole line; returns its bytes.  seq_at = where SEQ starts (QUAL starts n + 1 bytes behind it)
// MD (mlst_set_export_md): TAB MD:Z: and mdw bytes behind NM:i -- the text itself is left out as SEQ is (the wave of k_at_write writes
// an ungapped record's, k_at_dp<true> a banded one's); md_at = where it starts.  MD = false is the line as it was.
template <bool WRITE, bool MD = false>
__device__ inline u64 at_line(u8* p, const AtPair& m, u64 qname, AtQn qn, u32 flag, GP<const u8>::G* name, u32 name_len, int n, int bs,
                              bool has_xs, int xs, u64& seq_at, u32 mdw = 0, u64* md_at = nullptr) {
    AtOut<WRITE> o; o.p = p; o.n = 0;
    at_head<WRITE>(o, qname, qn, flag, name, name_len, m.pos0);
    if (m.flags & AT_DP) o.skip(m.cigw);
    else {
        const int be = (int)m.be;
        if (bs > 0) { o.dec32((u32)bs); o.ch('S'); }
        o.dec32((u32)(be - bs)); o.ch('M');
        if (n - be > 0) { o.dec32((u32)(n - be)); o.ch('S'); }
    }
    o.ch('\t'); o.ch('*'); o.ch('\t'); o.ch('0'); o.ch('\t'); o.ch('0'); o.ch('\t');
    seq_at = o.n; o.skip((u64)n);
    o.ch('\t'); o.skip((u64)n);
    o.tag('A', 'S', (u32)m.as);
    if (has_xs) o.tag('X', 'S', (u32)xs);
    o.ch('\t'); o.ch('X'); o.ch('N'); o.ch(':'); o.ch('i'); o.ch(':'); o.ch('0');
    o.tag('X', 'M', (u32)m.xm); o.tag('X', 'O', (u32)m.xo); o.tag('X', 'G', (u32)m.xg); o.tag('N', 'M', (u32)m.nm);
    if (MD) { o.ch('\t'); o.ch('M'); o.ch('D'); o.ch(':'); o.ch('Z'); o.ch(':'); if (md_at) *md_at = o.n; o.skip((u64)mdw); }
    o.ch('\t'); o.ch('Y'); o.ch('T'); o.ch(':'); o.ch('Z'); o.ch(':'); o.ch('U'); o.ch('U'); o.ch('\n');
    return o.n;
}

// the letter and the Phred of oriented position i of a retained read
__device__ inline void at_base(GP<u32>::G* rb, GP<u8>::G* rq, int n, int strand, int i, u8& letter, u8& phred) {
    const int s = strand ? n - 1 - i : i;
    const u8 qb = rq[s];
    u32 b = (rb[s >> 4] >> (2 * (s & 15))) & 3u; if (strand) b ^= 3u;
    letter = (qb & 0x80u) ? (u8)'N' : (u8)(0x54474341u >> (8 * b));      // "ACGT"
    phred = (u8)(qb & 0x7Fu);
}
__device__ inline u8 at_upper(u8 c) { return (c >= (u8)'a' && c <= (u8)'z') ? (u8)(c - 32) : c; }
// an M column counts towards NM when the SEQ letter is not the allele's, an N on either side included (samout.gap_figures)
__device__ inline u32 at_col_differs(u8 x, u8 y) { return (x != at_upper(y) || x == (u8)'N') ? 1u : 0u; }
// MD:Z (samout.md_text): the allele's letter as the text shows it -- upper case, a byte outside A-Z as N
__device__ inline u8 at_md_letter(u8 y) { const u8 c = at_upper(y); return (c >= (u8)'A' && c <= (u8)'Z') ? c : (u8)'N'; }
// One turn of 64 M columns of an ungapped record, a column per lane: mk = the ballot of the mismatching columns, run = the matching
// columns in front of the turn since the last mismatch (wave-uniform).  at_md_run: the match run in front of a mismatching lane;
// at_md_carry: run for the next turn, cols = this turn's columns.
__device__ inline u32 at_md_run(u64 mk, int lane, u32 run) {
    const u64 below = mk & ((1ull << lane) - 1ull);
    return below ? (u32)(lane - (64 - __clzll((long long)below))) : run + (u32)lane;
}
__device__ inline u32 at_md_carry(u64 mk, int cols, u32 run) { return mk ? (u32)(cols - (64 - __clzll((long long)mk))) : run + (u32)cols; }

// MD (mlst_set_export_md): the turns that count NM also leave the bytes of the record's MD:Z text in D.mdw
template <int NB, bool MD>
__device__ __forceinline__ void at_decide_body(const EngineDev* __restrict__ Ep, const KParams& P, const AtDev* __restrict__ Dp, AtRound R) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    __shared__ u32 s_rl[RW / 2 + 2]; __shared__ u32 s_rh[RW / 2 + 2]; __shared__ u32 s_rn[RW / 2 + 2]; __shared__ u32 s_odd[RW / 2 + 2];
    __shared__ u8 s_pen[RQ]; __shared__ u8 s_pentab[128]; __shared__ u8 s_seq[RQ];
    const int tid = threadIdx.x;
    for (int i = tid; i < 128; i += 64) s_pentab[i] = E.pen_tab[i];
    for (u64 k = R.k0 + blockIdx.x; k < R.k1; k += gridDim.x) {      // block-uniform
        const ItemDev it = E.items[D.perm[k]];
        const LocusDev L = E.loci[it.locus];
        const u32 lw = E.ret_len[it.ret]; const int n = (int)(lw & 0x7FFFu); const bool read_has_n = (lw & 0x8000u) != 0;
        __syncthreads();      // the rows of the item before are no longer read
        const int pen_def = __builtin_amdgcn_readfirstlane(stage_read_planes(E, P, it, n, s_rl, s_rh, s_rn, s_odd, s_pen, s_pentab, tid, 64));
        {
            auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
            for (int i = tid; i < n; i += 64) { u8 c, q; at_base(rb, rq, n, it.strand, i, c, q); s_seq[i] = c; }
        }
        __syncthreads();
        u32 rl[NB], rh[NB], od[NB], rn[NB];
        #pragma unroll
        for (int w = 0; w < NB; w++) {
            rl[w] = __builtin_amdgcn_readfirstlane(s_rl[w]); rh[w] = __builtin_amdgcn_readfirstlane(s_rh[w]);
            od[w] = __builtin_amdgcn_readfirstlane(s_odd[w]);
            rn[w] = read_has_n ? __builtin_amdgcn_readfirstlane(s_rn[w]) : 0u;
        }
        const int floor_n = E.floor_tab[n];
        const u64 p0 = D.pair_off[k] - R.pb;      // the item's first pair in the round
        for (u32 a0 = 0; a0 < L.n_alleles; a0 += 64) {      // block-uniform; a0 + lane < n_pad: the rows of the arena hold n_pad alleles
            const u32 a = a0 + (u32)tid;
            const bool valid = a < L.n_alleles;
            const int m = valid ? (int)E.allele_len[L.a_begin + a] : 0;      // (a lane behind the locus' last allele: no overlap, P0)
            int mm, bs, be;
            const int best = L.has_n ? ungapped_planes<NB, true, true>(E, P, L, a, m, n, it.diag, rl, rh, od, rn, s_pen, pen_def, read_has_n, mm, bs, be)
                                     : ungapped_planes<NB, true, false>(E, P, L, a, m, n, it.diag, rl, rh, od, rn, s_pen, pen_def, read_has_n, mm, bs, be);
            const int score = best >> MLST_P_SHIFT, xm = 255 - (best & 0xFF);
            AtPair o; o.as = 0; o.pos0 = 0; o.be = 0; o.cigw = 0; o.nm = 0; o.xg = 0; o.xm = 0; o.xo = 0; o.flags = 0; o.pad_ = 0;
            u32 mdw = 0;
            const bool pend = valid && gap_trigger(P, mm, xm, score, floor_n, m, n, it.diag, bs, be);
            const bool rec = valid && !pend && score >= floor_n && score > 0;
            if (pend) o.flags = (u8)AT_PEND;
            if (rec) {
                o.flags = (u8)AT_REC; o.as = score; o.xm = (u8)xm; o.pos0 = bs + it.diag; o.be = (u16)be;
                o.cigw = (u16)((bs > 0 ? at_digits32((u32)bs) + 1u : 0u) + at_digits32((u32)(be - bs)) + 1u + (n - be > 0 ? at_digits32((u32)(n - be)) + 1u : 0u));
            }
            const u64 wm = __ballot(pend);
            if (wm) {      // the list of the banded SW: one returning atomic per wave (the list holds every pair of the round)
                const int leader = __ffsll((long long)wm) - 1; u64 base = 0;
                if (tid == leader) base = atomicAdd((u64*)D.dp_n, (u64)__popcll(wm));
                base = __shfl(base, leader);
                if (pend) D.dp_list[base + __popcll(wm & ((1ull << tid) - 1))] = ((k - R.k0) << 20) | (u64)a;
            }
            // NM of the ungapped records: the wave walks each record's M columns [bs, be), 64 columns per turn
            u64 rm = __ballot(rec);
            while (rm) {
                const int t = __ffsll((long long)rm) - 1; rm &= rm - 1;
                const int tbs = __shfl(bs, t), tbe = __shfl(be, t);
                auto ref = D.ascii.g() + D.aoff[L.a_begin + a0 + (u32)t] + it.diag;      // (bs + diag >= 0 and be + diag <= m)
                u32 c = 0;
                if (MD) {      // per mismatch the digits of the match run in front of it and its letter, then the digits of the last run
                    constexpr int NT = (32 * NB + 63) / 64;      // turns of the longest M span; the allele's letters of all of them are fetched first: one wait
                    u8 y[NT];
                    #pragma unroll
                    for (int q = 0; q < NT; q++) { const int i = tbs + 64 * q + tid; y[q] = i < tbe ? ref[i] : (u8)0; }
                    u32 w = 0, run = 0;
                    #pragma unroll
                    for (int q = 0; q < NT; q++) {
                        const int i0 = tbs + 64 * q, i = i0 + tid;
                        if (i0 < tbe) {      // wave-uniform
                            const bool d = i < tbe && at_col_differs(s_seq[i], y[q]);
                            const u64 mk = __ballot(d);
                            if (d) { c++; w += at_digits32(at_md_run(mk, tid, run)) + 1u; }
                            run = at_md_carry(mk, tbe - i0 < 64 ? tbe - i0 : 64, run);
                        }
                    }
                    w = wave_sum_u32(w) + at_digits32(run);
                    if (tid == t) mdw = w;
                } else
                for (int i = tbs + tid; i < tbe; i += 64) c += at_col_differs(s_seq[i], ref[i]);
                c = wave_sum_u32(c);
                if (tid == t) o.nm = (u16)c;
            }
            if (valid) D.meta[p0 + a] = o;
            if (MD) { if (valid) D.mdw[p0 + a] = (u16)mdw; }
        }
    }
}
// reads up to 160 bases / up to MLST_MAX_READ_LEN (as k_pileup_160 / _320)
__global__ __launch_bounds__(64) void k_at_decide_160(const EngineDev* __restrict__ Ep, KParams P, const AtDev* __restrict__ Dp, AtRound R) { at_decide_body<5, false>(Ep, P, Dp, R); }
__global__ __launch_bounds__(64) void k_at_decide_320(const EngineDev* __restrict__ Ep, KParams P, const AtDev* __restrict__ Dp, AtRound R) { at_decide_body<RW / 2, false>(Ep, P, Dp, R); }
__global__ __launch_bounds__(64) void k_at_decide_160_md(const EngineDev* __restrict__ Ep, KParams P, const AtDev* __restrict__ Dp, AtRound R) { at_decide_body<5, true>(Ep, P, Dp, R); }
__global__ __launch_bounds__(64) void k_at_decide_320_md(const EngineDev* __restrict__ Ep, KParams P, const AtDev* __restrict__ Dp, AtRound R) { at_decide_body<RW / 2, true>(Ep, P, Dp, R); }

// XS and FLAG of a record from its read's figures
__device__ inline void at_xs_flag(const AtRead& rd, u64 pi, int strand, bool& has_xs, int& xs, u32& flag) {
    has_xs = rd.nrec >= 2u;
    xs = pi == rd.best_pair ? rd.other_as : rd.best_as;
    flag = (strand ? 16u : 0u) + (pi == rd.best_pair ? 0u : 256u);
}

// The walk of ax_walk (aln_export.h) with what the text needs.  text == NULL: the runs are counted -- cigw = the bytes of the CIGAR
// text, xo / xg = the I and D runs and their columns, nm = xg + the M columns whose SEQ letter is not the allele's.  text != NULL: the
// CIGAR text is written so that it ends at text[cigw - 1]; the walk meets the runs last to first, every run is written from its
// letter down to its first digit.
// MD (mlst_set_export_md): the same for the MD:Z text (samout.md_text), met last character first -- text == NULL: mdw = its bytes;
// text != NULL: written so that it ends at md[mdw - 1].  Backwards a match run's digits come before the break in front of it: a
// mismatching M column writes the run met so far, then its letter; the first D column met of a run writes the run met so far (also 0),
// every D column its letter, and the next column that is no D (or the walk's end) the ^ in front of them; the end writes the last run.
template <bool MD>
__device__ inline void at_walk(const u8* __restrict__ TB, int bi, int bb, int diag, int W, int n, GP<u32>::G* rb, GP<u8>::G* rq, int strand,
                               GP<const u8>::G* ref, u8* __restrict__ text, u32& cigw, u32& xo, u32& xg, u32& nm, int& pos0,
                               u8* __restrict__ md, u32& mdw) {
    const int BWMAX = 2 * MAX_W + 1, BW = 2 * W + 1;
    int i = bi, b = bb, state = 0, run_op = -1; u32 run_len = 0, at = cigw, w = 0, mism = 0;
    u32 mrun = 0, mat = mdw, mw = 0; bool indel = false;
    auto md_chr = [&](u8 c) { if (text) md[--mat] = c; mw++; };
    auto md_num = [&](u32 v) { const u32 d = at_digits32(v); if (text) for (u32 q = 0; q < d; q++) { md[--mat] = (u8)('0' + v % 10u); v /= 10u; } mw += d; };
    auto md_close = [&]() { if (indel) { md_chr((u8)'^'); indel = false; } };
    xo = 0; xg = 0;
    auto flush = [&]() {
        if (run_len > 0) {
            const u32 d = at_digits32(run_len);
            if (text) { text[--at] = (u8)(0x530044494Dull >> (8 * run_op) & 0xFF); u32 v = run_len; for (u32 q = 0; q < d; q++) { text[--at] = (u8)('0' + v % 10u); v /= 10u; } }
            w += d + 1;
            if (run_op == 1 || run_op == 2) { xo++; xg += run_len; }
        }
        run_len = 0;
    };
    auto push = [&](int op, u32 len) { if (op != run_op) { flush(); run_op = op; } run_len += len; };
    pos0 = 0;
    if (n - 1 - bi > 0) push(4, (u32)(n - 1 - bi));
    while (i >= 0 && b >= 0 && b < BW) {
        const u8 t = TB[i * BWMAX + b];
        if (state == 0) {
            const int src = t & 3;
            if (src == 0) break;
            if (src == 1) {
                const int j = i + diag - W + b; pos0 = j; push(0, 1);
                if (!text || MD) {
                    u8 c, q; at_base(rb, rq, n, strand, i, c, q);
                    const u32 df = at_col_differs(c, ref[j]);
                    if (!text) mism += df;
                    if (MD) { md_close(); if (df) { md_num(mrun); md_chr(at_md_letter(ref[j])); mrun = 0; } else mrun++; }
                }
                i--;
            }
            else if (src == 2) state = 1; else state = 2;
        } else if (state == 1) {
            const int ext = t & 4; pos0 = i + diag - W + b; push(2, 1);
            if (MD) { if (!indel) { md_num(mrun); mrun = 0; indel = true; } md_chr(at_md_letter(ref[pos0])); }
            b--; state = ext ? 1 : 0;
        }
        else { const int ext = t & 8; push(1, 1); if (MD) md_close(); i--; b++; state = ext ? 2 : 0; }
    }
    if (i + 1 > 0) push(4, (u32)(i + 1));
    flush();
    if (MD) { md_close(); md_num(mrun); if (!text) mdw = mw; }
    if (!text) { cigw = w; nm = xg + mism; }
}

// NAMES: the reads carry their own names (at_qname); only the EMIT pass looks at them.
// EMIT = false: the listed pairs' AtPair;  EMIT = true: the CIGAR text of those that have a record (text = the round's text, the
// lines' offsets in D.wex).  64 workgroups of 64 lanes at the most: lane k of workgroup g owns slice 64 g + k of the traceback store.
// MD: mlst_set_export_md -- EMIT = false also leaves the bytes of the MD:Z text in D.mdw, EMIT = true also writes that text.
template <bool EMIT, bool NAMES, bool MD>
__global__ __launch_bounds__(64) void k_at_dp(const EngineDev* __restrict__ Ep, KParams P, const AtDev* __restrict__ Dp, AtRound R,
                                              u8* __restrict__ tb_scratch, u8* __restrict__ text) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    __shared__ u8 s_pentab[128];
    for (int i = threadIdx.x; i < 128; i += 64) s_pentab[i] = E.pen_tab[i];
    __syncthreads();
    const u64 end = D.dp_n[0];
    const int BWMAX = 2 * MAX_W + 1;
    u8* TB = tb_scratch + ((u64)blockIdx.x * 64 + threadIdx.x) * (u64)(MLST_MAX_READ_LEN * BWMAX);
    for (u64 e = (u64)blockIdx.x * 64 + threadIdx.x; e < end; e += (u64)gridDim.x * 64) {
        const u64 ent = D.dp_list[e];
        const u64 k = R.k0 + (ent >> 20); const u32 a = (u32)(ent & 0xFFFFFu);
        const u64 pi = D.pair_off[k] - R.pb + a;
        AtPair o = D.meta[pi];
        if (EMIT && !(o.flags & AT_REC)) continue;
        const ItemDev it = E.items[D.perm[k]];
        const LocusDev L = E.loci[it.locus];
        const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
        auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
        auto ref = D.ascii.g() + D.aoff[L.a_begin + a];
        int bi, bb, pos0;
        const int best = banded<true>(E, P, it, L, a, n, s_pentab, TB, bi, bb);
        u32 cigw = o.cigw, xo, xg, nm, mdw = 0;
        if (EMIT) {
            const u32 r = D.item_read[k];
            const AtRead rd = D.reads[r - R.r0];
            const u64 ridx = E.ret_ridx[it.ret];
            const u32 flag = (it.strand ? 16u : 0u) + (rd.best_pair == pi ? 0u : 256u);
            const u64 g = L.a_begin + a;
            AtOut<false> h; h.p = nullptr; h.n = 0;
            at_head<false>(h, D.paired ? ridx >> 1 : ridx, at_qname<NAMES>(D, it.ret), flag, nullptr, (u32)(D.name_off[g + 1] - D.name_off[g]), o.pos0);
            u64 md_at = 0;
            if (MD) {      // where the MD text stands: the widths in front of it (the line as k_at_reads counted it)
                bool has_xs; int xs; u32 fl; u64 seq_at;
                at_xs_flag(rd, pi, it.strand, has_xs, xs, fl);
                mdw = D.mdw[pi];
                at_line<false, true>(nullptr, o, D.paired ? ridx >> 1 : ridx, at_qname<NAMES>(D, it.ret), fl, nullptr, (u32)(D.name_off[g + 1] - D.name_off[g]), n, 0, has_xs, xs, seq_at, mdw, &md_at);
            }
            at_walk<MD>(TB, bi, bb, it.diag, P.band_w, n, rb, rq, it.strand, ref, text + D.wex[pi] + h.n, cigw, xo, xg, nm, pos0, text + D.wex[pi] + md_at, mdw);
            continue;
        }
        const int score = best >> MLST_P_SHIFT, xm = 255 - (best & 0xFF);
        o.as = 0; o.pos0 = 0; o.be = 0; o.cigw = 0; o.nm = 0; o.xg = 0; o.xm = 0; o.xo = 0; o.flags = 0;
        if (score >= E.floor_tab[n] && score > 0) {
            at_walk<MD>(TB, bi, bb, it.diag, P.band_w, n, rb, rq, it.strand, ref, nullptr, cigw, xo, xg, nm, pos0, nullptr, mdw);
            o.flags = (u8)(AT_REC | AT_DP); o.as = score; o.xm = (u8)xm; o.pos0 = pos0;
            o.cigw = (u16)cigw; o.xo = (u8)xo; o.xg = (u16)xg; o.nm = (u16)nm;
        }
        D.meta[pi] = o;
        if (MD) D.mdw[pi] = (u16)mdw;
    }
}

// One wave per read of the round: its pairs are consecutive (the items are sorted by read first).
template <bool NAMES, bool MD>
__global__ __launch_bounds__(64) void k_at_reads(const EngineDev* __restrict__ Ep, const AtDev* __restrict__ Dp, AtRound R) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    const int lane = threadIdx.x;
    u64 recs = 0;
    for (u64 r = R.r0 + blockIdx.x; r < R.r1; r += gridDim.x) {      // block-uniform
        const u64 kf = D.read_first[r], kl = D.read_first[r + 1];
        const u64 q0 = D.pair_off[kf] - R.pb, q1 = D.pair_off[kl] - R.pb;
        // the best AS and the first pair in file order that holds it (the pairs' order is the file's order)
        int bas = 0; u64 bpi = ~0ull; u32 cnt = 0;
        for (u64 q = q0 + lane; q < q1; q += 64) {
            const AtPair m = D.meta[q];
            if (m.flags & AT_REC) { cnt++; if (m.as > bas) { bas = m.as; bpi = q; } }      // (q ascends: the first of equal ones stays)
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int oas = __shfl_xor(bas, o); const u64 opi = __shfl_xor(bpi, o);
            if (oas > bas || (oas == bas && opi < bpi)) { bas = oas; bpi = opi; }
        }
        cnt = wave_sum_u32(cnt);
        int oth = 0;
        for (u64 q = q0 + lane; q < q1; q += 64) {
            const AtPair m = D.meta[q];
            if ((m.flags & AT_REC) && q != bpi && m.as > oth) oth = m.as;
        }
        for (int o = 32; o > 0; o >>= 1) { const int x = __shfl_xor(oth, o); oth = x > oth ? x : oth; }
        AtRead rd; rd.best_pair = bpi; rd.nrec = cnt; rd.best_as = bas; rd.other_as = oth;
        if (lane == 0) { D.reads[r - R.r0] = rd; recs += cnt; }
        // the bytes of every line
        for (u64 k = kf; k < kl; k++) {
            const ItemDev it = E.items[D.perm[k]];
            const LocusDev L = E.loci[it.locus];
            const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
            const u64 ridx = E.ret_ridx[it.ret];
            const AtQn qn = at_qname<NAMES>(D, it.ret);
            const u64 p0 = D.pair_off[k] - R.pb;
            for (u32 a = (u32)lane; a < L.n_alleles; a += 64) {
                const AtPair m = D.meta[p0 + a];
                u64 len = 0;
                if (m.flags & AT_REC) {
                    bool has_xs; int xs; u32 flag; u64 seq_at;
                    at_xs_flag(rd, p0 + a, it.strand, has_xs, xs, flag);
                    const u64 g = L.a_begin + a;
                    len = at_line<false, MD>(nullptr, m, D.paired ? ridx >> 1 : ridx, qn, flag, nullptr, (u32)(D.name_off[g + 1] - D.name_off[g]), n, m.pos0 - it.diag, has_xs, xs, seq_at, MD ? (u32)D.mdw[p0 + a] : 0u);
                }
                D.wex[p0 + a] = len;
            }
        }
    }
    if (lane == 0 && recs) atomicAdd((u64*)D.n_rec, recs);
}

// Per pair: the bytes of the lines in front of it inside its workgroup (in place); per workgroup: its bytes.
__global__ __launch_bounds__(1024) void k_at_local(u64* __restrict__ wex, u64 n_pairs, u64* __restrict__ gsum) {
    __shared__ u64 s_w[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 i = (u64)blockIdx.x * FQT_GROUP + threadIdx.x;
    const u64 v = i < n_pairs ? wex[i] : 0ull;
    const u64 inc = fqt_wave_incl(v);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int k = 0; k < 16; k++) { const u64 x = s_w[k]; if (k < wv) before += x; all += x; }
    if (i < n_pairs) wex[i] = before + inc - v;
    if (threadIdx.x == 0) gsum[blockIdx.x] = all;
}

// n bytes from LDS to dst, the wave together: the bytes up to dst's next 4-byte boundary one per lane, then four per lane and store
__device__ __forceinline__ void at_copy(u8* __restrict__ dst, const u8* s_src, int n, int lane) {
    int head = (int)((4u - (u32)((u64)dst & 3u)) & 3u); if (head > n) head = n;
    if (lane < head) dst[lane] = s_src[lane];
    const int nw = (n - head) >> 2;
    u32* dw = (u32*)(dst + head);
    for (int w = lane; w < nw; w += 64) {
        const u8* s = s_src + head + 4 * w;
        dw[w] = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
    }
    const int t0 = head + 4 * nw;
    if (lane < n - t0) dst[t0 + lane] = s_src[t0 + lane];
}

// MD (mlst_set_export_md): the line leaves room for the MD:Z text (at_line<true, true>); k_at_md and k_at_dp<true> write it.
template <bool NAMES, bool MD>
__global__ __launch_bounds__(64) void k_at_write(const EngineDev* __restrict__ Ep, const AtDev* __restrict__ Dp, AtRound R, u8* __restrict__ text) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    __shared__ u8 s_seq[RQ]; __shared__ u8 s_qual[RQ];
    const int lane = threadIdx.x;
    for (u64 k = R.k0 + blockIdx.x; k < R.k1; k += gridDim.x) {      // block-uniform
        const ItemDev it = E.items[D.perm[k]];
        const LocusDev L = E.loci[it.locus];
        const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
        const u64 ridx = E.ret_ridx[it.ret];
        const AtQn qn = at_qname<NAMES>(D, it.ret);
        const AtRead rd = D.reads[D.item_read[k] - R.r0];
        const u64 p0 = D.pair_off[k] - R.pb;
        __syncthreads();      // the rows of the item before are no longer read
        {
            auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
            for (int i = lane; i < n; i += 64) { u8 c, q; at_base(rb, rq, n, it.strand, i, c, q); s_seq[i] = c; s_qual[i] = (u8)((q > 93 ? 93 : q) + 33); }
        }
        __syncthreads();
        for (u32 a0 = 0; a0 < L.n_alleles; a0 += 64) {      // block-uniform
            const u32 a = a0 + (u32)lane;
            bool rec = false; u64 at = 0, seq_at = 0;
            if (a < L.n_alleles) {
                const AtPair m = D.meta[p0 + a];
                if (m.flags & AT_REC) {
                    rec = true; at = D.wex[p0 + a];
                    bool has_xs; int xs; u32 flag;
                    at_xs_flag(rd, p0 + a, it.strand, has_xs, xs, flag);
                    const u64 g = L.a_begin + a; const u64 n0 = D.name_off[g];
                    at_line<true, MD>(text + at, m, D.paired ? ridx >> 1 : ridx, qn, flag, D.names.g() + n0, (u32)(D.name_off[g + 1] - n0), n, m.pos0 - it.diag, has_xs, xs, seq_at, MD ? (u32)D.mdw[p0 + a] : 0u);
                }
            }
            u64 rm = __ballot(rec);
            while (rm) {      // SEQ and QUAL of every record of the pass: the same bytes, copied by the wave
                const int t = __ffsll((long long)rm) - 1; rm &= rm - 1;
                const u64 s0 = uniform_u64(__shfl(at + seq_at, t));
                at_copy(text + s0, s_seq, n, lane);
                at_copy(text + s0 + (u64)n + 1, s_qual, n, lane);
            }
        }
    }
}

// mlst_set_export_md: the MD:Z text of the ungapped records of a round, on the walk k_at_decide counted it on.  One workgroup of
// AT_MD_WAVES waves per item (a round of an isolate holds a hundred items of a thousand records each: one wave per item, as k_at_write
// has it, would walk them one behind the other, a round trip to the allele text each); the read's letters are rendered once into LDS,
// wave w takes the passes of 64 alleles w, w + AT_MD_WAVES, ...  Per pass every lane finds where its record's text starts (at_line<false,
// true>: the widths in front of the field); then the wave takes record after record: the allele's letters under all of its M columns
// are fetched first (64 columns per turn, MLST_MAX_READ_LEN / 64 turns at the most: one wait per record), then turn by turn a
// mismatching lane writes the digits of the match run in front of it and the allele's letter at the turn's offset + the widths of the
// lanes below it (an inclusive scan; a turn without a mismatch costs its ballot only); one lane writes the last run.
#define AT_MD_WAVES 16
template <bool NAMES>
__global__ __launch_bounds__(64 * AT_MD_WAVES) void k_at_md(const EngineDev* __restrict__ Ep, const AtDev* __restrict__ Dp, AtRound R, u8* __restrict__ text) {
    const EngineDev& E = *Ep;     // device-resident descriptor: fields are scalar-loaded on demand
    const AtDev& D = *Dp;
    constexpr int NT = (MLST_MAX_READ_LEN + 63) / 64;      // turns of the longest M span
    __shared__ u8 s_seq[RQ];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (u64 k = R.k0 + blockIdx.x; k < R.k1; k += gridDim.x) {      // block-uniform
        const ItemDev it = E.items[D.perm[k]];
        const LocusDev L = E.loci[it.locus];
        const int n = (int)(E.ret_len[it.ret] & 0x7FFFu);
        const u64 ridx = E.ret_ridx[it.ret];
        const AtQn qn = at_qname<NAMES>(D, it.ret);
        const AtRead rd = D.reads[D.item_read[k] - R.r0];
        const u64 p0 = D.pair_off[k] - R.pb;
        __syncthreads();      // the letters of the item before are no longer read
        {
            auto rb = E.ret_bases.g() + (u64)it.ret * RW; auto rq = E.ret_quals.g() + (u64)it.ret * RQ;
            for (int i = threadIdx.x; i < n; i += 64 * AT_MD_WAVES) { u8 c, q; at_base(rb, rq, n, it.strand, i, c, q); s_seq[i] = c; }
        }
        __syncthreads();
        for (u32 a0 = 64u * (u32)wv; a0 < L.n_alleles; a0 += 64u * AT_MD_WAVES) {      // wave-uniform
            const u32 a = a0 + (u32)lane;
            u64 md_pos = 0; int mbs = 0, mbe = 0;      // (mbe stays 0 where the lane has no ungapped record: k_at_dp<true> writes a banded one's text)
            if (a < L.n_alleles) {
                const AtPair m = D.meta[p0 + a];
                if ((m.flags & AT_REC) && !(m.flags & AT_DP)) {
                    bool has_xs; int xs; u32 flag; u64 seq_at, md_at = 0;
                    at_xs_flag(rd, p0 + a, it.strand, has_xs, xs, flag);
                    const u64 g = L.a_begin + a;
                    mbs = m.pos0 - it.diag; mbe = (int)m.be;
                    at_line<false, true>(nullptr, m, D.paired ? ridx >> 1 : ridx, qn, flag, nullptr, (u32)(D.name_off[g + 1] - D.name_off[g]), n, mbs, has_xs, xs, seq_at, (u32)D.mdw[p0 + a], &md_at);
                    md_pos = D.wex[p0 + a] + md_at;
                }
            }
            u64 rm = __ballot(mbe > mbs);
            while (rm) {
                const int t = __ffsll((long long)rm) - 1; rm &= rm - 1;
                const int tbs = __shfl(mbs, t), tbe = __shfl(mbe, t);
                u64 pos = uniform_u64(__shfl(md_pos, t));
                auto ref = D.ascii.g() + D.aoff[L.a_begin + a0 + (u32)t] + it.diag;      // (as k_at_decide reads it)
                u8 y[NT];
                #pragma unroll
                for (int q = 0; q < NT; q++) { const int i = tbs + 64 * q + lane; y[q] = i < tbe ? ref[i] : (u8)0; }
                u32 run = 0;
                #pragma unroll
                for (int q = 0; q < NT; q++) {
                    const int i0 = tbs + 64 * q, i = i0 + lane;
                    if (i0 < tbe) {      // wave-uniform
                        const bool d = i < tbe && at_col_differs(s_seq[i], y[q]);
                        const u64 mk = __ballot(d);
                        if (mk) {
                            const u32 r = at_md_run(mk, lane, run), w = d ? at_digits32(r) + 1u : 0u;
                            u32 inc = w;
                            for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(inc, o); if (lane >= o) inc += x; }
                            if (d) { AtOut<true> out; out.p = text; out.n = pos + inc - w; out.dec32(r); out.ch((char)at_md_letter(y[q])); }
                            pos += (u64)(u32)__builtin_amdgcn_readlane((int)inc, 63);
                        }
                        run = at_md_carry(mk, tbe - i0 < 64 ? tbe - i0 : 64, run);
                    }
                }
                if (lane == 0) { AtOut<true> out; out.p = text; out.n = pos; out.dec32(run); }
            }
        }
    }
}

#endif
