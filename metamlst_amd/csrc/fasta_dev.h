// fasta_dev.h -- contigs tiled into reads on the device (included by mlst_engine.hip behind bam_reads.h; entry: mlst_submit_fasta).
//
// The text of a call (uncompressed FASTA, its first byte the '>' of the first header: the host steps over what stands in front)
// is cut into cells of FA_CELL bytes, a workgroup each, a thread per 16 bytes.  Whether a byte belongs to a header or to a
// sequence is a property of the LINE it is in, and that line may have begun any number of cells earlier (a contig on one line, a
// header longer than a cell).  So the kind of a line is a state carried over the cells:
//   k_fa_kind    : per cell the kind of the last line start in it (header / sequence) or "none"
//   k_fa_state   : one workgroup: "the last one that is not none" scanned over the cells -> the kind of the line a cell opens in
//   k_fa_count   : per cell the sequence bytes and the header lines; the first byte only the host reader treats (white space inside
//                  a sequence line, a CR without its LF: atomicMin on byte << 3 | reason)
//   k_fa_scan    : one workgroup: exclusive prefix sums (64-bit) of both -> where a cell's bases go in the flat sequence, which
//                  contig its first header opens; again behind k_fa_windows for the reads in front of every contig
//   k_fa_compact : the sequence bytes, line ends removed, into one flat array; per contig where it starts there
//   k_fa_windows : per contig how many reads tile_fasta cuts from it (the rules: include/mlst.h), and the longest read
//   k_fa_reads   : a thread per read: its contig by binary search in the prefix sums, then offset and length in the flat array
// A line start is a byte whose predecessor is LF (or byte 0); the predecessor of a thread's first byte and the successor of its
// last one (a CR LF over a thread or cell edge) are loaded from the text, so cell edges need no state of their own.
// The reads are then packed by k_pack_text itself: the flat array begins with FA_QUAL 'I's, the one quality string of every read
// (Phred 40), so a read is a sequence offset, the quality offset 0 and a length -- what k_fq_records leaves for FASTQ text.
// All offsets into the text and the flat array are 64-bit.  Descriptor fields are read through GP<> (address space 1).
#ifndef MLST_FASTA_DEV_H
#define MLST_FASTA_DEV_H

#define FA_CELL     4096u      /* bytes of text per workgroup: 256 threads x 16 */
#define FA_QUAL     336u       /* 'I's in front of the flat sequence (MLST_MAX_READ_LEN rounded up to whole 16-byte loads) */
#define FA_HDR      1u
#define FA_SEQ      2u
#define FA_BAD_WS   1u         /* 0x09 0x0B 0x0C 0x20 in a sequence line (Python's strip() takes them off a line's ends only) */
#define FA_BAD_CR   2u         /* a CR that is not directly in front of an LF */

struct FaMeta {             // device-resident results of a call (zeroed per call, err_key = ~0)
    u64 err_key;            // smallest (byte << 3 | FA_BAD_*)
    u64 n_seq;              // bases in the flat array
    u64 n_contigs;          // header lines
    u64 n_reads;
    u32 max_len, pad_;      // the longest read
};
struct FaDev {              // device-resident descriptor (uploaded per call)
    GP<const u8> text;      // the call's text
    GP<u8> flat;            // FA_QUAL 'I's, then the sequence
    GP<u32> kind;           // per cell: k_fa_kind's last line kind, then (in place) k_fa_state's entry kind
    GP<u64> cseq, chdr;     // per cell: sequence bytes / header lines, then (in place) their exclusive prefix sums
    GP<u64> cstart;         // per contig: its first base in the sequence
    GP<u64> wcnt;           // per contig: its reads, then (in place) the reads in front of it
    GP<FaMeta> meta;
    u64 cap_contigs;        // entries of cstart / wcnt (contigs beyond are counted, not stored: the host grows the tables and repeats)
};

// a thread's 16 bytes in b[1..16], the byte in front of them in b[0] (LF in front of byte 0), the byte behind them in b[17]
__device__ inline void fa_load(const FaDev& D, u64 n_bytes, u64 p0, u8 (&b)[18]) {
    if (p0 + 16 <= n_bytes) { const uint4 v = *(const GLOBAL_AS uint4*)(D.text.g() + p0); __builtin_memcpy(b + 1, &v, 16); }      // (cells and threads start at multiples of 16)
    else {
        #pragma unroll
        for (int k = 0; k < 16; k++) b[1 + k] = p0 + k < n_bytes ? D.text[p0 + k] : (u8)0;
    }
    b[0] = (p0 && p0 <= n_bytes) ? D.text[p0 - 1] : (u8)'\n';
    b[17] = p0 + 16 < n_bytes ? D.text[p0 + 16] : (u8)0;
}
// kind of the last line that starts in the thread's bytes (0: none does)
__device__ inline u32 fa_last_kind(const u8 (&b)[18], u64 p0, u64 n_bytes) {
    u32 t = 0;
    #pragma unroll
    for (int k = 0; k < 16; k++) if (p0 + k < n_bytes && b[k] == (u8)'\n') t = b[k + 1] == (u8)'>' ? FA_HDR : FA_SEQ;
    return t;
}
// The thread's bytes in order, `kind` being the kind of the line its first byte is in: on_hdr() at a header's '>', on_seq(c) for a
// base, on_bad(p, reason) for a byte of a sequence line that only the host reader treats.
template <typename FS, typename FH, typename FB>
__device__ inline void fa_walk(const u8 (&b)[18], u64 p0, u64 n_bytes, u32 kind, FS on_seq, FH on_hdr, FB on_bad) {
    #pragma unroll
    for (int k = 0; k < 16; k++) {
        const u64 p = p0 + k;
        if (p < n_bytes) {
            const u32 c = b[k + 1];
            if (b[k] == (u8)'\n') { kind = c == (u32)'>' ? FA_HDR : FA_SEQ; if (kind == FA_HDR) on_hdr(); }
            if (kind == FA_SEQ && c != (u32)'\n') {
                if (c == (u32)'\r') { if (!(p + 1 < n_bytes && b[k + 2] == (u8)'\n')) on_bad(p, FA_BAD_CR); }
                else if (c == 0x09u || c == 0x0Bu || c == 0x0Cu || c == 0x20u) on_bad(p, FA_BAD_WS);
                else on_seq((u8)c);
            }
        }
    }
}
// Exclusive scan over the workgroup's threads (NW waves) with the operator "the later one unless it is 0": what the last thread in
// front of this one with v != 0 holds, `carry` when there is none.  *all: the last v != 0 of the whole workgroup (0: none).
// Ends with a barrier (s_w may be used again).
template <int NW>
__device__ inline u32 fa_last_excl(u32 v, u32* s_w, u32 carry, u32* all) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 inc = v;
    for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(inc, o); if (lane >= o && !inc) inc = y; }
    u32 ex = __shfl_up(inc, 1); if (lane == 0) ex = 0;
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    u32 before = 0, last = 0;
    for (int w = 0; w < NW; w++) { const u32 x = s_w[w]; if (x) { last = x; if (w < wv) before = x; } }
    *all = last;
    __syncthreads();
    return ex ? ex : (before ? before : carry);
}

__global__ __launch_bounds__(256) void k_fa_kind(const FaDev* __restrict__ Dp, u64 n_bytes) {
    __shared__ u32 s_w[4];
    const FaDev& D = *Dp;
    const u64 p0 = (u64)blockIdx.x * FA_CELL + (u64)threadIdx.x * 16;
    u8 b[18]; fa_load(D, n_bytes, p0, b);
    u32 all; (void)fa_last_excl<4>(fa_last_kind(b, p0, n_bytes), s_w, 0u, &all);
    if (threadIdx.x == 0) D.kind[blockIdx.x] = all;
}

// One workgroup of 1024 threads, 1024 cells per turn.  (Cell 0 opens at byte 0, a line start: its entry kind is never used.)
__global__ __launch_bounds__(1024) void k_fa_state(const FaDev* __restrict__ Dp, u32 n_cells) {
    __shared__ u32 s_w[16]; __shared__ u32 s_carry;
    const FaDev& D = *Dp;
    if (threadIdx.x == 0) s_carry = FA_SEQ;
    __syncthreads();
    for (u32 k0 = 0; k0 < n_cells; k0 += 1024u) {
        const u32 k = k0 + threadIdx.x; const u32 v = k < n_cells ? D.kind[k] : 0u;
        u32 all; const u32 ex = fa_last_excl<16>(v, s_w, s_carry, &all);      // (its barriers stand between this read of s_carry and the write below)
        if (k < n_cells) D.kind[k] = ex;
        if (threadIdx.x == 0 && all) s_carry = all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_fa_count(const FaDev* __restrict__ Dp, u64 n_bytes) {
    __shared__ u32 s_w[4]; __shared__ u32 s_n[2][4];
    const FaDev& D = *Dp;
    const u64 p0 = (u64)blockIdx.x * FA_CELL + (u64)threadIdx.x * 16;
    u8 b[18]; fa_load(D, n_bytes, p0, b);
    u32 all; const u32 kind = fa_last_excl<4>(fa_last_kind(b, p0, n_bytes), s_w, D.kind[blockIdx.x], &all);
    u32 ns = 0, nh = 0; u64 bad = ~0ull;
    fa_walk(b, p0, n_bytes, kind, [&](u8) { ns++; }, [&]() { nh++; }, [&](u64 p, u32 why) { const u64 key = (p << 3) | why; if (key < bad) bad = key; });
    if (bad != ~0ull) atomicMin((unsigned long long*)&D.meta.p->err_key, (unsigned long long)bad);      // (rare: the call is refused)
    ns = wave_sum_u32(ns); nh = wave_sum_u32(nh);
    if ((threadIdx.x & 63) == 0) { s_n[0][threadIdx.x >> 6] = ns; s_n[1][threadIdx.x >> 6] = nh; }
    __syncthreads();
    if (threadIdx.x == 0) { D.cseq[blockIdx.x] = (u64)(s_n[0][0] + s_n[0][1] + s_n[0][2] + s_n[0][3]); D.chdr[blockIdx.x] = (u64)(s_n[1][0] + s_n[1][1] + s_n[1][2] + s_n[1][3]); }
}

// One workgroup of 1024 threads: exclusive prefix sums in place, 1024 values per turn (a wave scan, the waves' totals through LDS).
// which = 0: cseq and chdr over the n_cells cells, totals -> meta.n_seq / n_contigs; which = 1: wcnt over the contigs (those that
// are stored), total -> meta.n_reads.
__global__ __launch_bounds__(1024) void k_fa_scan(const FaDev* __restrict__ Dp, int which, u64 n_cells) {
    __shared__ u64 s_w[2][16]; __shared__ u64 s_carry[2];
    const FaDev& D = *Dp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 nc = D.meta->n_contigs;
    const u64 n = which ? (nc < D.cap_contigs ? nc : D.cap_contigs) : n_cells;
    if (tid < 2) s_carry[tid] = 0;
    __syncthreads();
    for (u64 i0 = 0; i0 < n; i0 += 1024u) {
        const u64 i = i0 + tid;
        const u64 va = i < n ? (which ? D.wcnt[i] : D.cseq[i]) : 0ull, vb = (i < n && !which) ? D.chdr[i] : 0ull;
        u64 ia = va, ib = vb;
        for (int o = 1; o < 64; o <<= 1) { const u64 ya = __shfl_up(ia, o), yb = __shfl_up(ib, o); if (lane >= o) { ia += ya; ib += yb; } }
        if (lane == 63) { s_w[0][wv] = ia; s_w[1][wv] = ib; }
        __syncthreads();
        u64 ba = s_carry[0], bb = s_carry[1], ta = 0, tb = 0;
        for (int w = 0; w < 16; w++) { const u64 xa = s_w[0][w], xb = s_w[1][w]; if (w < wv) { ba += xa; bb += xb; } ta += xa; tb += xb; }
        if (i < n) { if (which) D.wcnt[i] = ba + ia - va; else { D.cseq[i] = ba + ia - va; D.chdr[i] = bb + ib - vb; } }
        __syncthreads();
        if (tid == 0) { s_carry[0] += ta; s_carry[1] += tb; }
        __syncthreads();
    }
    if (tid == 0) { if (which) D.meta->n_reads = s_carry[0]; else { D.meta->n_seq = s_carry[0]; D.meta->n_contigs = s_carry[1]; } }
}

__global__ __launch_bounds__(256) void k_fa_compact(const FaDev* __restrict__ Dp, u64 n_bytes) {
    __shared__ u32 s_w[4]; __shared__ u32 s_n[2][4];
    const FaDev& D = *Dp;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 p0 = (u64)blockIdx.x * FA_CELL + (u64)threadIdx.x * 16;
    u8 b[18]; fa_load(D, n_bytes, p0, b);
    u32 all; const u32 kind = fa_last_excl<4>(fa_last_kind(b, p0, n_bytes), s_w, D.kind[blockIdx.x], &all);
    u32 ns = 0, nh = 0;
    fa_walk(b, p0, n_bytes, kind, [&](u8) { ns++; }, [&]() { nh++; }, [&](u64, u32) {});
    const u32 is = wave_incl_scan_dpp(ns), ih = wave_incl_scan_dpp(nh);
    if (lane == 63) { s_n[0][wv] = is; s_n[1][wv] = ih; }
    __syncthreads();
    u64 at = D.cseq[blockIdx.x] + (is - ns), ci = D.chdr[blockIdx.x] + (ih - nh);      // the thread's first base in the sequence, the first contig it opens
    for (int w = 0; w < wv; w++) { at += s_n[0][w]; ci += s_n[1][w]; }
    const u64 cap = D.cap_contigs;
    fa_walk(b, p0, n_bytes, kind, [&](u8 c) { D.flat[(u64)FA_QUAL + at] = c; at++; }, [&]() { if (ci < cap) D.cstart[ci] = at; ci++; }, [&](u64, u32) {});
}

// reads of a contig of n bases (tile_fasta): none below min_len, one of n bases up to read_len, else a window every `stride`
// bases up to start n - read_len, and one more flush with the end when that start is not a multiple of the stride
__device__ inline u64 fa_windows_of(u64 n, u32 read_len, u32 stride, u32 min_len) {
    if (n < (u64)min_len) return 0;
    if (n <= (u64)read_len) return 1;
    const u64 span = n - read_len;
    return span / stride + 1 + (span % stride ? 1 : 0);
}
__global__ __launch_bounds__(256) void k_fa_windows(const FaDev* __restrict__ Dp, u32 read_len, u32 stride, u32 min_len) {
    const FaDev& D = *Dp;
    const u64 nc_all = D.meta->n_contigs, nc = nc_all < D.cap_contigs ? nc_all : D.cap_contigs, n_seq = D.meta->n_seq;
    u32 mx = 0;
    for (u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += (u64)gridDim.x * blockDim.x) {
        const u64 n = (c + 1 < nc_all && c + 1 < D.cap_contigs ? D.cstart[c + 1] : n_seq) - D.cstart[c];
        const u64 w = fa_windows_of(n, read_len, stride, min_len);
        D.wcnt[c] = w;
        if (w) { const u32 l = n < (u64)read_len ? (u32)n : read_len; if (l > mx) mx = l; }
    }
    for (int o = 32; o > 0; o >>= 1) { const u32 y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&D.meta.p->max_len, mx);
}

// One thread per read: seq_off / qual_off / lens as k_fq_records leaves them for k_pack_text (offsets into D.flat).
__global__ __launch_bounds__(256) void k_fa_reads(const FaDev* __restrict__ Dp, u64 n_reads, u32 read_len, u32 stride,
                                                  u64* __restrict__ seq_off, u64* __restrict__ qual_off, u16* __restrict__ lens) {
    const FaDev& D = *Dp;
    const u64 nc = D.meta->n_contigs, n_seq = D.meta->n_seq;      // (nc <= cap_contigs: the host has seen to it)
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = nc;      // the last contig with wcnt[c] <= r (contigs without reads share their successor's value and lie in front of it)
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (D.wcnt[mid] <= r) lo = mid + 1; else hi = mid; }
        const u64 c = lo - 1;     // (wcnt[0] = 0 <= r)
        const u64 cs = D.cstart[c], n = (c + 1 < nc ? D.cstart[c + 1] : n_seq) - cs;
        u64 st = 0; u32 len = (u32)n;
        if (n > (u64)read_len) { st = (r - D.wcnt[c]) * stride; if (st > n - read_len) st = n - read_len; len = read_len; }
        seq_off[r] = (u64)FA_QUAL + cs + st; qual_off[r] = 0; lens[r] = (u16)len;
    }
}

#endif
