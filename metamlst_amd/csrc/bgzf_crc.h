// CRC-32 (RFC 1952: reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF) of an inflated BGZF block, one
// wave per block (k_bgzf_crc in mlst_engine.hip).  The same code compiles for the host, lane by lane (tests drive the device).
//
// The wave reads the block 1 KiB at a time, lane l the 16 bytes at 16 l of it: one fully coalesced 16-byte load per lane and
// step.  A lane's bytes therefore lie STRIDE bytes apart, and its register is carried over the GAP between them by the table
// itself: far[j][b] is the raw CRC register (initial value 0, no final XOR) of byte b followed by 15 - j + GAP zero bytes, so
//     acc' = XOR_j far[j][byte j of (chunk ^ acc in its first four bytes)]
// is one step of slicing-by-16 AND the 1008 zero bytes behind the chunk -- 16 LDS look-ups per 16 bytes, no more than a plain
// slicing-by-16 over a contiguous run, with no multiplication per step.  The raw CRC is linear and blind to leading zero bytes:
// the steps are aligned to the END of the block, the bytes in front of it count as zeros, and the initial value is XORed into the
// block's first four bytes as they are loaded (head_chunk).  At the end lane l holds its bytes' share of the CRC multiplied by
// x^(8 GAP) and misplaced by 16 (63 - l) bytes; as 16 * 63 = GAP both are mended by ONE multiplication by x^(-128 l) mod P per lane
// (mul: 32 shift-and-XOR steps in plain VALU code -- gfx950 has no carry-less multiply -- once per lane and block against
// 16 look-ups per 16 bytes), and the 64 products are XORed together.
#pragma once
#include <stdint.h>

#if !defined(MLST_HD)
#if defined(__HIPCC__)
#define MLST_HD __host__ __device__
#else
#define MLST_HD
#endif
#endif

namespace bgzf_crc {

constexpr uint32_t POLY = 0xEDB88320u;
enum { LANES = 64, CHUNK = 16, STRIDE = LANES * CHUNK, GAP = STRIDE - CHUNK };

struct Tables {
    uint32_t far[CHUNK * 256];      // [j][b]
    uint32_t lane_mul[LANES];       // x^(-128 l) mod P (reflected: x^0 = 0x80000000)
};

constexpr uint32_t byte_tab(uint32_t b) { for (int k = 0; k < 8; k++) b = (b & 1u) ? (b >> 1) ^ POLY : b >> 1; return b; }
constexpr uint32_t div_x(uint32_t v) { return (v & 0x80000000u) ? ((v ^ POLY) << 1) | 1u : v << 1; }      // v / x mod P (P's x^0 term is bit 31)

constexpr Tables make_tables() {
    Tables t{};
    uint32_t tab0[256] = {};
    for (uint32_t b = 0; b < 256; b++) tab0[b] = byte_tab(b);
    // far[15]: a byte and GAP zero bytes -- worked out for the eight one-bit bytes, the rest by linearity
    uint32_t bit[8] = {};
    for (int k = 0; k < 8; k++) {
        uint32_t r = tab0[1u << k];
        for (int z = 0; z < GAP; z++) r = tab0[r & 0xffu] ^ (r >> 8);
        bit[k] = r;
    }
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t r = 0;
        for (int k = 0; k < 8; k++) if (b >> k & 1u) r ^= bit[k];
        t.far[15 * 256 + b] = r;
    }
    for (int j = 14; j >= 0; j--)      // one more zero byte behind it
        for (uint32_t b = 0; b < 256; b++) { const uint32_t r = t.far[(j + 1) * 256 + b]; t.far[j * 256 + b] = tab0[r & 0xffu] ^ (r >> 8); }
    uint32_t c = 0x80000000u;
    for (int l = 0; l < LANES; l++) { t.lane_mul[l] = c; for (int k = 0; k < 8 * CHUNK; k++) c = div_x(c); }
    return t;
}

// a * b mod P, both reflected
MLST_HD inline uint32_t mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
    }
    return p;
}

struct Chunk { uint32_t w[4]; };

// one step: far: the 16 tables (LDS on the device)
template <typename TabPtr>
MLST_HD inline uint32_t step(TabPtr far, uint32_t acc, const Chunk& c) {
    uint32_t r = 0;
    const uint32_t w0 = c.w[0] ^ acc;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t w = q ? c.w[q] : w0;
        r ^= far[(4 * q + 0) * 256 + (w & 0xffu)] ^ far[(4 * q + 1) * 256 + ((w >> 8) & 0xffu)]
           ^ far[(4 * q + 2) * 256 + ((w >> 16) & 0xffu)] ^ far[(4 * q + 3) * 256 + (w >> 24)];
    }
    return r;
}

// the chunk at p in [-15, 3] from the block's start (text = the block's first byte, n its length; p + 16 <= n): the bytes in front
// of the block count as zeros, its first four bytes carry the initial value.  Read byte by byte: nothing in front of the block is touched.
MLST_HD inline Chunk head_chunk(const uint8_t* text, int p) {
    Chunk c = {{0, 0, 0, 0}};
    for (int j = 0; j < CHUNK; j++) {
        const int at = p + j;
        if (at < 0) continue;
        const uint32_t b = (uint32_t)text[at] ^ (at < 4 ? 0xffu : 0u);
        c.w[j >> 2] |= b << (8 * (j & 3));
    }
    return c;
}

// what is left to do on the XOR of the lanes' products: an initial value of which 4 - n bytes were never met by data, the final XOR
MLST_HD inline uint32_t finish(uint32_t v, uint32_t n) { return v ^ 0xFFFFFFFFu ^ (n < 4u ? 0xFFFFFFFFu >> (8u * n) : 0u); }

#if !defined(__HIP_DEVICE_COMPILE__)
// the device's algorithm on the host, lane after lane (a check of the tables and of the head / tail handling)
inline uint32_t crc_host(const Tables& t, const uint8_t* text, uint32_t n) {
    const uint32_t K = (n + STRIDE - 1) / STRIDE;
    uint32_t v = 0;
    for (int lane = 0; lane < LANES; lane++) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < K; k++) {
            const int p = (int)n - (int)((K - k) * STRIDE) + CHUNK * lane;
            if (p <= -CHUNK) continue;
            Chunk c;
            if (p < 4) c = head_chunk(text, p);
            else for (int q = 0; q < 4; q++) c.w[q] = (uint32_t)text[p + 4 * q] | (uint32_t)text[p + 4 * q + 1] << 8 | (uint32_t)text[p + 4 * q + 2] << 16 | (uint32_t)text[p + 4 * q + 3] << 24;
            acc = step(t.far, acc, c);
        }
        v ^= mul(acc, t.lane_mul[lane]);
    }
    return finish(v, n);
}
#endif

}      // namespace bgzf_crc
