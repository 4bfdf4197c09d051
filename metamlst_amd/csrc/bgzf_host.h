// bgzf_host.h -- BGZF framing on the host: one block's header, the four-thread walk over a chunk's headers, and the ONE lister that
// turns a caller's buffer into the block records the inflate kernels read.  Plain C++17 (no HIP call, no engine handle, no formatting):
// every input path of the engine lists its blocks here and adds its own bases, limits and messages; tests/host/bgzf_list_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <thread>
#include <vector>

typedef unsigned long long u64; typedef unsigned int u32; typedef unsigned char u8;

// one BGZF block: its deflate stream in the compressed buffer, its text in the output (the record of the kernels of inflate_lane.h, which keeps its name)
namespace inflate_lane { struct Blk { u64 in_off, out_off; u32 in_len, out_len; }; }
typedef inflate_lane::Blk BgzfBlk;

struct BzHdr { u64 off; u32 total, coff, clen, isize; };      // one BGZF block of a chunk: where it starts, its size, where its deflate data lies, the bytes it inflates to
// BGZF framing (SAM spec 4.1): gzip member with an extra subfield 'B','C' holding the block size - 1; deflate data; CRC32, ISIZE
static bool bgzf_block(const u8* p, u64 left, u64& total, u64& cdata_off, u64& cdata_len, u32& isize) {
    if (left < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
    const u32 xlen = (u32)p[10] | ((u32)p[11] << 8);
    if (left < 12ull + xlen) return false;
    u32 bsize = 0; bool found = false;
    for (u32 o = 0; o + 4 <= xlen; ) {
        const u8* sf = p + 12 + o; const u32 slen = (u32)sf[2] | ((u32)sf[3] << 8);
        if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && o + 6 <= xlen) { bsize = (u32)sf[4] | ((u32)sf[5] << 8); found = true; }
        o += 4 + slen;
    }
    if (!found) return false;
    total = (u64)bsize + 1;
    if (total > left || total < 12ull + xlen + 8) return false;
    cdata_off = 12ull + xlen; cdata_len = total - cdata_off - 8;
    isize = (u32)p[total - 4] | ((u32)p[total - 3] << 8) | ((u32)p[total - 2] << 16) | ((u32)p[total - 1] << 24);
    return true;
}

// The walk over a chunk's block headers is a chain of cache (and TLB) misses, ~190 ns per block (the next header's place is in this
// one): a chunk of 32 MB or more is walked by four threads, each from a block start it FINDS behind its quarter mark (the header's
// fixed bytes, parsed, and the block behind it parsed too); a list is taken only where the chain of the list before it lands exactly
// on its first block -- so a false start (header bytes inside deflate data) costs the time, never the result -- and the caller's
// serial loop goes on from `walked`, where the accepted lists end (all errors are its).  lists_taken: how many of the four counted.
static void bgzf_walk_parallel(const u8* data, u64 n_bytes, std::vector<BzHdr>& hdr, u64& walked, int* lists_taken) {
    hdr.clear(); walked = 0; if (lists_taken) *lists_taken = 0;
    static const bool one = [] { const char* e = getenv("MLST_BGZF_WALK"); return e && e[0] == '1'; }();      // MLST_BGZF_WALK=1: the serial walk (A/B)
    if (n_bytes < (32ull << 20) || one) return;
    enum { WT = 4 };
    std::vector<BzHdr> part[WT]; u64 stop[WT] = {0}, cand[WT] = {0}; bool have[WT] = {false};
    auto work = [&](int k) {
        u64 from = 0;
        if (k) {
            const u64 s0 = n_bytes * (u64)k / WT, s1 = std::min<u64>(s0 + 131072, n_bytes - 18);
            bool ok = false;
            for (u64 q = s0; q < s1 && !ok; q++) {
                if (data[q] != 0x1f || data[q + 1] != 0x8b || data[q + 2] != 8 || !(data[q + 3] & 4)) continue;
                u64 t, co, cl; u32 is;
                if (!bgzf_block(data + q, n_bytes - q, t, co, cl, is)) continue;
                u64 t2, co2, cl2; u32 is2;
                if (q + t != n_bytes && !bgzf_block(data + q + t, n_bytes - q - t, t2, co2, cl2, is2)) continue;
                from = q; ok = true;
            }
            if (!ok) return;
            cand[k] = from; have[k] = true;
        }
        const u64 limit = k + 1 < WT ? std::min<u64>(n_bytes * (u64)(k + 1) / WT + 262144, n_bytes) : n_bytes;
        part[k].reserve((size_t)((limit - from) / 8192 + 64));
        u64 off = from;
        while (off < limit) {
            u64 t, co, cl; u32 is;
            if (!bgzf_block(data + off, n_bytes - off, t, co, cl, is)) break;
            part[k].push_back(BzHdr{off, (u32)t, (u32)co, (u32)cl, is});
            off += t;
        }
        stop[k] = off;
    };
    std::thread th[WT - 1];
    for (int k = 1; k < WT; k++) th[k - 1] = std::thread(work, k);
    work(0);
    for (auto& t : th) t.join();
    hdr.swap(part[0]); walked = stop[0];
    int taken = 1;
    for (int k = 1; k < WT; k++) {
        if (!have[k]) break;
        size_t i = hdr.size();
        while (i > 0 && hdr[i - 1].off > cand[k]) i--;
        if (i == 0 || hdr[i - 1].off != cand[k]) break;      // the chain does not pass through the start this thread found: its list is dropped, and those behind it
        hdr.resize(i - 1);
        hdr.insert(hdr.end(), part[k].begin(), part[k].end());
        walked = stop[k]; taken++;
    }
    if (lists_taken) *lists_taken = taken;
}

// The blocks of a buffer, listed.  Blocks with data are APPENDED to `blks` (in_off relative to `data`, out_off counted from 0 for
// this call; the caller adds its bases), empty blocks (the EOF marker) are skipped; start (optional): the offset in `data` where
// every listed block begins.  parallel: bgzf_walk_parallel first (headers of its lists, then block by block from where they end).
// may_cut: a block cut off by the end of the buffer is left to the caller -- the buffer ends inside its header, or the header's
// fixed bytes are there and the block does not parse -- and `taken` is where it starts; anything else that is no block is an
// error even then.  The first failing block in file order decides the result: `bad_off` is where it starts, `bad_isize` what it claims.
enum BgzfListRc { BGZF_LIST_OK = 0, BGZF_LIST_NOT_WHOLE, BGZF_LIST_CLAIMS };      // a list / not a whole block at bad_off / the block at bad_off claims bad_isize (> 65536) bytes
struct BgzfList { u64 text = 0, taken = 0, bad_off = 0; u32 bad_isize = 0; };      // text: the sum of isize; taken: bytes of `data` consumed (n_bytes, or the start of the cut block)
static BgzfListRc bgzf_list(const u8* data, u64 n_bytes, bool may_cut, bool parallel, std::vector<BgzfBlk>& blks, BgzfList& L,
                            std::vector<u64>* start = nullptr, int* lists_taken = nullptr) {
    L = BgzfList(); if (lists_taken) *lists_taken = 0;
    std::vector<BzHdr> hdr; u64 walked = 0;
    if (parallel) bgzf_walk_parallel(data, n_bytes, hdr, walked, lists_taken);
    size_t hi_ = 0; u64 off = 0;      // (headers of `hdr` first, then block by block from `walked`)
    while (off < n_bytes) {
        u64 total, coff, clen; u32 isize;
        if (hi_ < hdr.size()) { const BzHdr& q = hdr[hi_++]; off = q.off; total = q.total; coff = q.coff; clen = q.clen; isize = q.isize; }
        else if (off < walked) { off = walked; continue; }
        else if (!bgzf_block(data + off, n_bytes - off, total, coff, clen, isize)) {
            const bool cut = n_bytes - off < 18 || (data[off] == 0x1f && data[off + 1] == 0x8b && data[off + 2] == 8 && (data[off + 3] & 4));
            if (may_cut && cut) break;
            L.bad_off = off; return BGZF_LIST_NOT_WHOLE;
        }
        if (isize > 65536) { L.bad_off = off; L.bad_isize = isize; return BGZF_LIST_CLAIMS; }
        if (isize) { BgzfBlk b; b.in_off = off + coff; b.in_len = (u32)clen; b.out_off = L.text; b.out_len = isize; blks.push_back(b); if (start) start->push_back(off); L.text += isize; }
        off += total;
    }
    L.taken = off;
    return BGZF_LIST_OK;
}
