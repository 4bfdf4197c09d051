// bgzf_list_check.cpp -- csrc/bgzf_host.h on its own: bgzf_list against a serial walk written out here (bgzf_block alone), on the
// smallest buffers that can go wrong and on one of just over 32 MB (the four-thread walk).  Stored deflate blocks, written here: no
// zlib.  Exit status 0 = every check held; a failed check prints its line and the program goes on.   c++ -O1 -std=c++17 -pthread
#include "bgzf_host.h"
#include <cstdio>
#include <cstring>
#include <string>

typedef std::vector<u8> Buf;
static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); g_bad++; } } while (0)

static void put16(Buf& b, u32 v) { b.push_back((u8)v); b.push_back((u8)(v >> 8)); }
static void put32(Buf& b, u32 v) { put16(b, v & 0xFFFF); put16(b, v >> 16); }
// one BGZF block holding `n` bytes of `text` as a stored deflate block; extra: subfields in front of 'BC'; bc: with the 'BC' subfield
static Buf block(const u8* text, u32 n, const Buf& extra = Buf(), bool bc = true) {
    Buf b = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
    const u32 xlen = (u32)extra.size() + 6, total = 12 + xlen + 5 + n + 8;
    put16(b, xlen);
    b.insert(b.end(), extra.begin(), extra.end());
    b.push_back(bc ? 'B' : 'X'); b.push_back(bc ? 'C' : 'Y'); put16(b, 2); put16(b, total - 1);
    b.push_back(1); put16(b, n); put16(b, ~n & 0xFFFF);
    b.insert(b.end(), text, text + n);
    put32(b, 0); put32(b, n);      // (CRC32: the lister does not look at it)
    return b;
}
static void add(Buf& to, const Buf& b) { to.insert(to.end(), b.begin(), b.end()); }
static void set_isize(Buf& b, u32 v) { for (int k = 0; k < 4; k++) b[b.size() - 4 + k] = (u8)(v >> (8 * k)); }

struct Out { int rc = 0; std::vector<BgzfBlk> blks; std::vector<u64> start; BgzfList L; int lists = -1; };
// the serial walk, block by block with bgzf_block alone
static Out serial(const u8* d, u64 n, bool may_cut) {
    Out o; u64 off = 0;
    while (off < n) {
        u64 total, coff, clen; u32 isize;
        if (!bgzf_block(d + off, n - off, total, coff, clen, isize)) {
            const bool magic = n - off >= 4 && d[off] == 0x1f && d[off + 1] == 0x8b && d[off + 2] == 8 && (d[off + 3] & 4);
            if (may_cut && (n - off < 18 || magic)) break;
            o.rc = BGZF_LIST_NOT_WHOLE; o.L.bad_off = off; return o;
        }
        if (isize > 65536) { o.rc = BGZF_LIST_CLAIMS; o.L.bad_off = off; o.L.bad_isize = isize; return o; }
        if (isize) { o.blks.push_back(BgzfBlk{off + coff, o.L.text, (u32)clen, isize}); o.start.push_back(off); o.L.text += isize; }
        off += total;
    }
    o.L.taken = off;
    return o;
}
// the lister, compared with the serial walk field by field
static Out list(const Buf& b, bool may_cut, bool parallel, int line) {
    Out o; o.rc = bgzf_list(b.data(), b.size(), may_cut, parallel, o.blks, o.L, &o.start, &o.lists);
    const Out w = serial(b.data(), b.size(), may_cut);
    bool same = o.rc == w.rc && o.L.bad_off == w.L.bad_off && o.L.bad_isize == w.L.bad_isize;
    if (same && o.rc == BGZF_LIST_OK) {
        same = o.L.text == w.L.text && o.L.taken == w.L.taken && o.blks.size() == w.blks.size() && o.start == w.start;
        for (size_t i = 0; same && i < o.blks.size(); i++)
            same = o.blks[i].in_off == w.blks[i].in_off && o.blks[i].out_off == w.blks[i].out_off && o.blks[i].in_len == w.blks[i].in_len && o.blks[i].out_len == w.blks[i].out_len;
    }
    if (!same) { fprintf(stderr, "line %d: the lister and the serial walk differ (rc %d / %d, %zu / %zu blocks)\n", line, o.rc, w.rc, o.blks.size(), w.blks.size()); g_bad++; }
    // without the optional outputs: the same list
    std::vector<BgzfBlk> b2; BgzfList L2;
    if (bgzf_list(b.data(), b.size(), may_cut, parallel, b2, L2) != o.rc || b2.size() != o.blks.size() || L2.taken != o.L.taken) { fprintf(stderr, "line %d: differs without start / lists_taken\n", line); g_bad++; }
    return o;
}
#define LIST(b, cut, par) list(b, cut, par, __LINE__)

int main() {
    setenv("MLST_BGZF_WALK", "0", 1);      // (the four-thread walk is what is tested)
    std::string t(70000, ' ');
    { u32 s = 12345; for (auto& c : t) { s = s * 1664525u + 1013904223u; c = (char)(32 + (s >> 16) % 95); } }      // printable: no header bytes in it
    const u8* txt = (const u8*)t.data();
    const Buf A = block(txt, 300), B = block(txt + 300, 200), C = block(txt + 500, 250), E = block(txt, 0);

    {   // an empty buffer (and no buffer)
        Out o = LIST(Buf(), false, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.empty() && o.L.taken == 0 && o.L.text == 0 && o.lists == 0);
        std::vector<BgzfBlk> b; BgzfList L; CHECK(bgzf_list(nullptr, 0, true, true, b, L) == BGZF_LIST_OK && b.empty() && L.taken == 0);
    }
    {   // one block
        Out o = LIST(A, false, true);
        CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == 1 && o.L.taken == A.size() && o.L.text == 300 && o.lists == 0);
        CHECK(o.blks[0].in_off == 18 && o.blks[0].in_len == 305 && o.blks[0].out_off == 0 && o.blks[0].out_len == 300 && o.start[0] == 0);
    }
    {   // three blocks and an empty (EOF) block between them: not listed, consumed, the text offsets run on; appended behind what the list holds
        Buf b; add(b, A); add(b, E); add(b, B); add(b, C);
        Out o = LIST(b, false, false);
        CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == 3 && o.L.taken == b.size() && o.L.text == 750 && o.lists == 0);
        CHECK(o.blks[1].out_off == 300 && o.blks[2].out_off == 500 && o.start[1] == A.size() + E.size() && o.blks[1].in_off == o.start[1] + 18);
        std::vector<BgzfBlk> keep(2); BgzfList L;
        CHECK(bgzf_list(b.data(), b.size(), false, false, keep, L) == BGZF_LIST_OK && keep.size() == 5 && keep[2].out_off == 0 && keep[4].out_off == 500);
    }
    {   // the buffer ends 1, 17, 18 bytes into the next header, and inside the block's body
        Buf ab; add(ab, A); add(ab, B);
        for (size_t cutlen : {(size_t)1, (size_t)17, (size_t)18, (size_t)100, C.size() - 1}) {
            Buf b = ab; b.insert(b.end(), C.begin(), C.begin() + cutlen);
            Out o = LIST(b, true, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == 2 && o.L.taken == ab.size() && o.L.text == 500);
            o = LIST(b, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == ab.size());
        }
    }
    {   // bytes at a block boundary that are no header: an error even with may_cut when 18 or more are left (fewer: they may be a header's start)
        Buf b = A; b.insert(b.end(), 18, (u8)'x');
        Out o = LIST(b, true, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
        o = LIST(b, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
        b.pop_back();
        o = LIST(b, true, true); CHECK(o.rc == BGZF_LIST_OK && o.L.taken == A.size());
        o = LIST(b, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
    }
    {   // a trailer that claims 65,537 bytes is refused with its offset and the value; 65,536 is accepted; the first bad block in file order decides
        Buf big = B; set_isize(big, 65537);
        Buf b; add(b, A); add(b, big); b.insert(b.end(), 40, (u8)'x');
        Out o = LIST(b, true, false); CHECK(o.rc == BGZF_LIST_CLAIMS && o.L.bad_off == A.size() && o.L.bad_isize == 65537);
        Buf b2; add(b2, A); b2.insert(b2.end(), 40, (u8)'x'); add(b2, big);
        o = LIST(b2, false, false); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
        Buf ok = B; set_isize(ok, 65536);
        Buf b3; add(b3, A); add(b3, ok); add(b3, C);
        o = LIST(b3, false, false); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == 3 && o.blks[1].out_len == 65536 && o.blks[2].out_off == 300 + 65536);
    }
    {   // an extra subfield in front of 'BC'; no 'BC' subfield; an xlen that runs past the buffer
        const Buf extra = {'Z', 'Z', 3, 0, 1, 2, 3};
        Buf b; add(b, A); add(b, block(txt, 100, extra)); add(b, C);
        Out o = LIST(b, false, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == 3 && o.blks[1].in_off == A.size() + 18 + extra.size() && o.blks[1].in_len == 105);
        Buf n; add(n, A); add(n, block(txt, 100, Buf(), false)); add(n, C);
        o = LIST(n, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
        o = LIST(n, true, true); CHECK(o.rc == BGZF_LIST_OK && o.L.taken == A.size() && o.blks.size() == 1);      // (header bytes: as a cut block)
        Buf x = A; const size_t at = x.size(); add(x, B); x[at + 10] = 0x60; x[at + 11] = 0xEA;      // xlen 60,000
        o = LIST(x, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == A.size());
    }
    {   // just over 32 MB of stored blocks: the four-thread walk
        Buf big; std::vector<u64> at;
        for (int k = 0; big.size() <= (32ull << 20) + 100000; k++) { at.push_back(big.size()); add(big, block(txt + k % 7, 59000 + (k * 37) % 900)); }
        at.push_back(big.size()); add(big, E);
        const size_t n = at.size() - 1;
        Out o = LIST(big, false, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == n && o.L.taken == big.size() && o.lists == 4);
        o = LIST(big, false, false); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == n && o.lists == 0);
        {   Buf cut(big.begin(), big.end() - E.size() - 30000);      // cut inside the last block with data: the serial tail of the walk says so
            o = LIST(cut, true, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == n - 1 && o.L.taken == at[n - 1] && o.lists == 4);
            o = LIST(cut, false, true); CHECK(o.rc == BGZF_LIST_NOT_WHOLE && o.L.bad_off == at[n - 1]); }
        {   Buf bad = big; for (int k = 0; k < 4; k++) bad[at[n / 2 + 1] - 4 + k] = (u8)(65537u >> (8 * k));      // a block in a later thread's list claims too much
            o = LIST(bad, false, true); CHECK(o.rc == BGZF_LIST_CLAIMS && o.L.bad_off == at[n / 2] && o.L.bad_isize == 65537); }
        // two chained false headers in the stored data right behind every quarter mark: the three threads that start there find them,
        // their lists are dropped, the list is the serial walk's
        Buf fake = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x27, 0};
        Buf trap = fake; trap.insert(trap.end(), 22, (u8)'x'); add(trap, fake); trap.insert(trap.end(), 22, (u8)'y');
        for (u64 q = 1; q <= 3; q++) {
            const u64 mark = big.size() * q / 4;
            size_t k = 0; while (at[k + 1] <= mark) k++;      // the block that holds the mark
            const u64 pos = std::max<u64>(mark, at[k] + 23) + 40;
            CHECK(pos + trap.size() + 108 < at[k + 1]);
            memcpy(big.data() + pos, trap.data(), trap.size());
        }
        o = LIST(big, false, true); CHECK(o.rc == BGZF_LIST_OK && o.blks.size() == n && o.L.taken == big.size() && o.lists == 1);
    }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("bgzf_list: all checks held\n");
    return 0;
}
