"""The inflate decoders on deflate streams that zlib never writes (tests/deflate_writer.py builds them; zlib's inflate is the
reference of every one).  On the host through the two test hooks -- csrc/inflate_dev.h and csrc/inflate_canon.h -- and on the
GPU through the three device paths, with the kernel that has to take each block predicted from the rules in the headers and
compared with what ran (mlst_debug_inflate_paths).  profiles/round6/inflate_streams.md has the corpus' composition."""
import os
import struct
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from deflate_writer import Header, dynamic, fixed, stored
from test_inflate import _bgzf_raw, deflate, inflate, inflate_canon, payloads

TOK_CAP, LIT_BASE, NSYM_L, SYM_ESC = 24576, 65280, 192, 224      # mlst_engine.hip INFL_TOK_CAP, inflate_lane.h, inflate_canon.h
MODES = ("2", "2c", "1")
SEEDS = list(range(400, 400 + max(6, int(os.environ.get("MLST_STREAM_FUZZ_N", "6")))))      # (the variable lengthens the list, never shortens it)


class Case:
    def __init__(self, group, name, s, friendly=None, doc=""):
        self.group, self.name, self.s, self.doc = group, name, s, doc
        self.friendly = friendly            # True: encoded for csrc/inflate_canon.h (it has to decode it itself)
        assert len(s.raw) + 26 <= 65536, name


# ------------------------------------------------------------------------------------------------------------- payloads
def fastq_like(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while sum(map(len, out)) < n:
        L = int(rng.integers(50, 151))
        out.append(b"@r%d.%d\n%s\n+\n%s\n" % (seed, k, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)),
                                              bytes(rng.choice(np.frombuffer(b"#,5:<AFHIJ", np.uint8), L, p=[.02, .03, .05, .05, .05, .1, .2, .2, .2, .1]))))
        k += 1
    return b"".join(out)[:n]


def bam_like(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    while sum(map(len, out)) < n:
        L = int(rng.integers(30, 120))
        out.append(struct.pack("<iiiBBHHHIiii", 300 + L, int(rng.integers(0, 40)), int(rng.integers(0, 5000)), 8, 255, 4680, 1, 16 * int(rng.integers(0, 2)), L, -1, -1, 0)
                   + b"read%d\0" % int(rng.integers(0, 999)) + struct.pack("<I", L << 4) + bytes(rng.integers(0, 256, (L + 1) // 2, dtype=np.uint8))
                   + bytes(rng.integers(2, 41, L, dtype=np.uint8)) + b"ASC" + bytes([int(rng.integers(0, 255))]) + b"XSC" + bytes([int(rng.integers(0, 255))]))
    return b"".join(out)[:n]


def payload(kind: str, n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed + 77)
    if kind == "fastq":
        return fastq_like(n, seed)
    if kind == "bam":
        return bam_like(n, seed)
    if kind == "low":
        return bytes(rng.choice(np.frombuffer(b"AAAAAAAC\n", np.uint8), n))
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def friendly_spare():
    """symbols csrc/inflate_canon.h keeps as bytes: literals below SYM_ESC and the length symbols"""
    return list(range(32, SYM_ESC)) + list(range(257, 286)) + list(range(0, 32))


def both(group, name, make, doc):
    """a named case in its two encodings: fixed code (or unrestricted dynamic) for the look-up-table kernels, and dynamic with at
    most NSYM_L symbols in use and no literal of SYM_ESC or more for k_inflate_tok2"""
    out = []
    for friendly in (False, True):
        s = make(friendly)
        c = Case(group, name + ("/canon" if friendly else "/lut"), s, friendly, doc)
        if friendly:
            assert not s.left_by_canon, c.name
        out.append(c)
    return out


def huff(toks, friendly, **kw):
    """the look-up-table encoding is the fixed code; the other a dynamic block built from the counts"""
    return dynamic(toks, **kw) if friendly else fixed(toks)


# ---------------------------------------------------------------------------------------------- group 1: long codes
def _insert(toks, extra, seed):
    rng = np.random.default_rng(seed)
    toks = list(toks)
    for t in extra:
        toks.insert(int(rng.integers(len(toks) // 2, len(toks))), t)
    return toks


def long_literal_codes(friendly, end_with_all_ones=False):
    """inflate_lane.h:62-75 and :89-92 (long_code<Huff::LB + 1>): rare literals and lengths with codes of 10 .. 15 bits on a block
    of fewer than 24,576 tokens; end_with_all_ones: the 15-bit all-ones code is the last symbol before end-of-block"""
    base = dw.random_parse(fastq_like(30000, 1), 1, 0.5)
    ll = dw.lengths_from_counts(dw.token_counts(base)[0])
    s0 = max((s for s in range(286) if 0 < ll[s] <= 9), key=lambda s: (ll[s], s))      # (the chain hangs under a code of at most 9 bits: 10 .. 15 all occur)
    rare = [ord("N"), ord("n"), 257 + dw.lsym(100), 200, ord("%"), 257 + dw.lsym(227), ord("~"), 1, 2, 3, 257 + dw.lsym(258), 4, 5, 6]
    if not friendly:
        rare[3], rare[7] = 230, 255
    fill = [s for s in rare if not ll[s]][:15 - ll[s0]]
    assert len(fill) == 15 - ll[s0]
    ll = dw.push_deep(ll, s0, fill)
    extra = []
    for s in fill * 6:
        extra.append(s if s < 256 else (dw.LBASE[s - 257], 7))
    toks = _insert(base, extra, 2)
    if end_with_all_ones:
        top = [s for s, (c, l) in dw.canon(ll).items() if l == 15 and c == 0x7FFF][0]
        toks.append(top if top < 256 else (dw.LBASE[top - 257], 9))
    dl = dw.lengths_from_counts(dw.token_counts(toks)[1])
    s = dw.stream([dynamic(toks, ll, dl)])
    assert s.tokens < TOK_CAP and s.blocks[0].max_llen_used == 15 and len(set(ll[f] for f in fill)) >= 15 - 10
    return s


def long_distance_codes(friendly):
    """inflate_lane.h:106-109 (long_code<HuffD::LB + 1>): distance codes of 9 .. 15 bits, longer than HuffD::LB = 8"""
    base = dw.random_parse(fastq_like(40000, 3), 3, 0.6)
    base = [t if not isinstance(t, tuple) or t[1] <= 512 else t[1] & 63 | 64 for t in base]      # (far matches out: their symbols stay free)
    base += [(258, 4)] * 40                                   # (room for the farthest distance symbols)
    text_len = len(dw.replay(base))
    assert text_len > 24577 + 64
    dl = dw.lengths_from_counts(dw.token_counts(base)[1])
    s0 = max((s for s in range(30) if 0 < dl[s] <= 8), key=lambda s: (dl[s], s))
    free = [s for s in range(29, -1, -1) if not dl[s]][:15 - dl[s0]]
    assert len(free) == 15 - dl[s0], (dl, free)
    dl = dw.push_deep(dl, s0, free)
    toks = list(base)
    for k, s in enumerate(free * 4):
        toks.append((3 + k % 40, min(dw.DBASE[s] + k, text_len)))
    assert all(dw.dsym(t[1]) in free for t in toks[len(base):])
    blk = dynamic(toks, dl=dl)
    if not friendly:
        blk.ll = dw.use_exactly(dw.lengths_from_counts(dw.token_counts(toks)[0]), 200, range(286))
    s = dw.stream([blk])
    assert s.tokens < TOK_CAP and s.blocks[0].max_dlen_used == 15 and s.blocks[0].max_dlen == 15
    return s


# ---------------------------------------------------------------------------------------------- group 2: chain depth
def chain_depth(s) -> int:
    """The deepest pointer chain k_inflate_ptr meets (inflate_lane.h:213-243): a literal or stored byte is final; byte j of a match
    with dist >= len points `dist` back; of a periodic one (dist < len) into the period in front of the match."""
    depth = np.zeros(len(s.data) + 1, np.int64)
    at = 0
    for b in s.toks:
        if not isinstance(b, tuple):
            at += 1
            continue
        n, d = b
        j = np.arange(n)
        depth[at:at + n] = depth[at - d + (j % d if d < n else j)] + 1
        at += n
    return int(depth.max())


def chain(n, d, total=LIT_BASE, lens=None):
    def make(friendly):
        head = list(b"ACGTTGCAAT" * 30)[:d]
        toks, at, k = list(head), d, 0
        while True:
            m = n if lens is None else lens[k % len(lens)]
            if at + m > total:
                break
            toks.append((m, d if lens is None else (lens[(k - 1) % len(lens)] if k else d)))
            at += m
            k += 1
        toks += [65] * (total - at)
        s = dw.stream([huff(toks, friendly)])
        assert len(s.data) == total
        return s
    return make


# ------------------------------------------------------------------------------------------ group 3: periodic matches
def periodic_table(friendly):
    """inflate_lane.h:236-242 (the float reciprocal): every dist in 1 .. 64 with len in {dist + 1, 2 dist, 2 dist + 1, 257, 258}"""
    toks = list(b"@r\nACGTTGCA\n+\nIIHHGG\n" * 4)
    for d in range(1, 65):
        for n in (d + 1, 2 * d, 2 * d + 1, 257, 258):
            if 3 <= n <= 258:
                toks += [(n, d), 65 + (d & 15)]
    return dw.stream([huff(toks, friendly)])


def periodic_wide(friendly):
    """inflate_lane.h:236-242 for the distances in between: dist 65 .. 257 with len = dist + 1 and 258, dist = 2^k +- 1"""
    toks = list(fastq_like(600, 5))
    for d in list(range(65, 258, 7)) + [127, 128, 129, 255, 256, 257]:
        toks += [(d + 1, d), 66, (258, d), 67]
    return dw.stream([huff(toks, friendly)])


def lane_to_wave(friendly):
    """inflate_lane.h:216-222 and :243: dist >= len with len in {16, 17, 64, 258} -- the lane fills 16 bytes, the wave the rest"""
    toks = list(fastq_like(1200, 6))
    for n in (15, 16, 17, 18, 64, 258):
        for d in (n, n + 1, 300, 1000):
            toks += [(n, d), 68]
    return dw.stream([huff(toks, friendly)])


def far_match(friendly):
    """inflate_lane.h:215 (dist = (t & 0x7FFF) + 1): distance 32,768 exactly, the top of the 15-bit field"""
    toks = dw.random_parse(fastq_like(32768, 7), 7, 0.8)
    toks = [t if not isinstance(t, tuple) or t[1] < 16385 else 78 for t in toks]      # (keeps the text's length: checked below)
    n = len(dw.replay(toks))
    toks = toks + [66] * (32768 - n) + [(258, 32768), 10, (3, 32768), (40, 32767)]
    s = dw.stream([huff(toks, friendly)])
    assert len(s.data) == 32768 + 258 + 1 + 3 + 40
    return s


def match_into_stored(friendly):
    """inflate_lane.h:244-247 then :222 / :241: matches, periodic ones too, whose source is a stored run of an earlier deflate block"""
    run = fastq_like(700, 8)
    toks = [(20, 14), 10, (258, 700), (30, 3), (5, 760), 65, (100, 1), (16, 16), (17, 300)]
    return dw.stream([stored(run), huff(toks, friendly), stored(b"tail"), huff([(4, 4), (9, 2)], friendly)])


# ------------------------------------------------------------------------------------- group 4: stored after Huffman
def stored_at_phase(phase):
    def make(friendly):
        for nlit in range(1, 40):
            first = huff([200 if not friendly else 71] * nlit, friendly)
            run = b"stored-run-%d\n" % phase * 50
            s = dw.stream([first, stored(run), stored(b""), huff([(20, 14), 10], friendly), stored(b"xyz")])
            if s.blocks[1].bit_phase == phase:
                return s
        raise AssertionError("no phase %d" % phase)
    make.__doc__ = "inflate_dev.h:225 / inflate_canon.h:171 (b.pos -= b.cnt >> 3): a stored block whose header starts at bit %d of a byte, behind a Huffman block" % phase
    return make


def empty_stored_everywhere(friendly):
    """inflate_dev.h:225-233 with len = 0 (what a sync flush leaves), before, between and after the other blocks; OutTok::raw :46"""
    t = fastq_like(300, 9)
    return dw.stream([stored(b""), stored(b""), huff(list(t[:100]), friendly), stored(b""), stored(t[100:200]), stored(b""), huff(list(t[200:]) + [(50, 250)], friendly),
                      stored(b""), stored(b"")])


def big_stored_after_empty(friendly):
    """inflate_lane.h:244-247: a stored run of 65,280 bytes (every pointer of the block) behind an empty Huffman block"""
    return dw.stream([huff([], friendly), stored(payload("random", LIT_BASE, 10))])


def sixty_blocks(friendly):
    """inflate_dev.h:221-279: 60 deflate blocks of alternating type in one BGZF block"""
    t = fastq_like(12000, 11)
    blocks = []
    for k in range(60):
        part = t[200 * k:200 * k + 200]
        toks = list(part) + ([(30 + k, 150 + k)] if k else [])
        blocks.append([stored(part), huff(toks, friendly), dynamic(toks, hdr=Header(repeats=bool(k & 2)))][k % 3] if not friendly else [stored(part), dynamic(toks)][k % 2])
    return dw.stream(blocks)


# ------------------------------------------------------------------------------------------------ group 5: thresholds
def n_tokens(n):
    """mlst_engine.hip INFL_TOK_CAP / OutTok::emit inflate_lane.h:42: a block of exactly n tokens"""
    t = fastq_like(n + 14000, 12)
    toks = dw.random_parse(t, 12, 0.1)[:n]
    s = dw.stream([dynamic(toks[:n // 2]), dynamic(toks[n // 2:])])
    assert s.tokens == n and not s.left_by_canon
    return s


def n_symbols(n):
    """inflate_canon.h:83 (offs > cap, NSYM_L = 192): exactly n literal / length symbols in use, none of them a literal >= 224"""
    toks = dw.random_parse(fastq_like(20000, 13), 13, 0.6)
    ll = dw.use_exactly(dw.lengths_from_counts(dw.token_counts(toks)[0]), n, friendly_spare())
    s = dw.stream([dynamic(toks, ll)])
    assert s.blocks[0].lsyms == n and s.blocks[0].max_lit < SYM_ESC
    return s


def highest_literal(v):
    """inflate_canon.h:88 (SYM_ESC = 224): the highest literal with a code is v, few symbols in use"""
    toks = dw.random_parse(fastq_like(20000, 14), 14, 0.6) + [v, v, (3, 1)]
    s = dw.stream([dynamic(toks)])
    assert s.blocks[0].max_lit == v and s.blocks[0].lsyms < NSYM_L
    return s


def text_bytes(n):
    """inflate_lane.h:137 (want > LIT_BASE) and :267 (ptr[total], ptr[total + 1]): a block of exactly n bytes of text"""
    s = dw.stream([dynamic(dw.random_parse(fastq_like(n, 15), 15, 0.8))])
    assert len(s.data) == n and s.tokens < TOK_CAP and not s.left_by_canon
    return s


def residue(k):
    """inflate_lane.h:317 (the 16-byte write-out only where the text starts on a 16-byte boundary): 4,097 + k bytes, so that the
    blocks behind it start at every residue mod 16"""
    return dw.stream([dynamic(dw.random_parse(fastq_like(4097 + k, 16 + k), 16 + k, 0.7))])


# --------------------------------------------------------------------------------------------------- group 6: headers
def _hdr_case(hdr, toks_fn=None, dl_fn=None, check=None):
    def make(friendly):
        toks = toks_fn() if toks_fn else dw.random_parse(fastq_like(6000, 17), 17, 0.6)
        lc, dc = dw.token_counts(toks)
        ll = dw.lengths_from_counts(lc)
        if not friendly:
            ll = dw.use_exactly(ll, 230, list(range(255, -1, -1)))
        s = dw.stream([dynamic(toks, ll, dl_fn(dc) if dl_fn else None, hdr)])
        if check:
            assert check(s.blocks[0]), s.blocks[0]
        return s
    return make


def _lits_only():
    return list(fastq_like(3000, 18))


def _far_only():
    toks = list(fastq_like(3000, 19))
    return toks + [(10, 600 + 37 * k) for k in range(60)]


def named_cases():
    C = []
    g = "1 long codes"
    C += both(g, "long_literal_codes", long_literal_codes, long_literal_codes.__doc__)
    C += both(g, "all_ones_15_before_eob", lambda f: long_literal_codes(f, True), long_literal_codes.__doc__)
    C += both(g, "long_distance_codes", long_distance_codes, long_distance_codes.__doc__)
    g = "2 chain depth"
    doc = "inflate_lane.h:274 (18 rounds of pointer jumping): matches (len %s, dist %s) to 65,280 bytes, every one a link deeper"
    for n, d in ((3, 1), (3, 3), (4, 4), (258, 258)):
        C += both(g, "chain_%d_%d" % (n, d), chain(n, d), doc % (n, d))
    C += both(g, "chain_each_copies_the_last", chain(0, 5, lens=[3, 5, 4, 9, 3, 17, 6]), doc % ("3 .. 17", "the match before"))
    g = "3 periodic"
    for f in (periodic_table, periodic_wide, lane_to_wave, far_match, match_into_stored):
        C += both(g, f.__name__, f, f.__doc__)
    g = "4 stored after huffman"
    for ph in range(8):
        f = stored_at_phase(ph)
        C += both(g, "stored_at_phase_%d" % ph, f, f.__doc__)
    for f in (empty_stored_everywhere, big_stored_after_empty, sixty_blocks):
        C += both(g, f.__name__, f, f.__doc__)
    g = "5 thresholds"
    C += [Case(g, "tokens_%d" % n, n_tokens(n), None, n_tokens.__doc__) for n in (TOK_CAP - 1, TOK_CAP, TOK_CAP + 1)]
    C += [Case(g, "symbols_%d" % n, n_symbols(n), None, n_symbols.__doc__) for n in (NSYM_L - 1, NSYM_L, NSYM_L + 1)]
    C += [Case(g, "highest_literal_%d" % v, highest_literal(v), None, highest_literal.__doc__) for v in (SYM_ESC - 1, SYM_ESC)]
    C += [Case(g, "text_%d" % n, text_bytes(n), None, text_bytes.__doc__) for n in (LIT_BASE - 1, LIT_BASE, LIT_BASE + 1, 65536)]
    C += [Case(g, "residue_%d" % k, residue(k), None, residue.__doc__) for k in range(16)]
    g = "6 headers"
    H = [("hlit_286_unused_tail", Header(hlit=286), None, None, lambda b: b.hlit == 286, "inflate_dev.h:248-249: HLIT = 286, the tail sent as zeros"),
         ("hdist_30", Header(hdist=30), None, None, lambda b: b.hdist == 30, "inflate_dev.h:248-249: HDIST = 30"),
         ("hlit_286_hdist_30_no_repeats", Header(hlit=286, hdist=30, repeats=False), None, None, lambda b: b.hlit == 286 and b.hdist == 30,
          "inflate_dev.h:254-257: 316 code lengths sent one by one"),
         ("no_distance_code", Header(), _lits_only, lambda dc: [0], lambda b: b.dsyms == 0, "inflate_dev.h:114 / :272-273: a literal-only block with HDIST = 1 and that length 0"),
         ("one_distance_code", Header(), lambda: _lits_only() + [(9, 9)] * 30, None, lambda b: b.dsyms == 1 and b.max_dlen == 1,
          "inflate_dev.h:273: the one legal incomplete code, a single distance code of one bit"),
         ("all_30_distance_codes", Header(), _far_only, lambda dc: dw.use_exactly(dw.lengths_from_counts(dc), 30, range(30)), lambda b: b.dsyms == 30,
          "inflate_dev.h:272: a distance code with all 30 symbols in use"),
         ("repeat_18_across_the_boundary", Header(hlit=286, cross=True), _far_only, None, lambda b: b.crossed,
          "inflate_dev.h:258-268: a repeat code that runs from the literal / length lengths into the distance lengths"),
         ("repeats_kept_apart", Header(hlit=286, cross=False), _far_only, None, lambda b: not b.crossed, "inflate_dev.h:258-268: the same lengths with no run across the boundary"),
         ("hclen_19_seven_bit_code_length_codes", Header(hclen=19, cl_deep=True, repeats=False), None, None, lambda b: b.hclen == 19 and b.max_cllen == 7,
          "inflate_dev.h:251-252: HCLEN = 19 and a code-length code with 7-bit codes (HuffD's tables, LB = 8)")]
    for name, hdr, tf, df, chk, doc in H:
        C += both(g, name, _hdr_case(hdr, tf, df, chk), doc)
    return C


def random_cases():
    C = []
    for seed in SEEDS:
        for kind in ("fastq", "bam", "low", "random"):
            n = int(np.random.default_rng(seed).integers(1, 24000))
            data = payload(kind, n, seed)
            for friendly in (False, True, True):
                seed += 1000
                C.append(Case("random", "%s_%d%s" % (kind, seed, "/canon" if friendly else ""), dw.random_stream(data, seed, friendly, 0.8 if kind != "random" else 0.2), None,
                              "seeded: random parse x random block split x random code shaping"))
    return C


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = named_cases() + random_cases()
        assert len(set(c.name for c in _CORPUS)) == len(_CORPUS)
    return _CORPUS


def predicted(cases, mode):
    """blocks phase 1 has to leave to k_inflate in this mode (blocks without text are never launched)"""
    return sum(1 for c in cases if c.s.left_to_wave(mode, TOK_CAP, LIT_BASE))


# ------------------------------------------------------------------------------------------------------------ rejected
def rejected_cases():
    """(name, raw stream, room for the text): streams no decoder may accept; zlib rejects every one"""
    F, sb, fl = dw._fields, dw._symbol_bits, dw.canon(dw.FIXED_LL)
    pk = lambda *bits: np.packbits(np.concatenate(bits), bitorder="little").tobytes()      # noqa: E731
    code = lambda c, l: F([int(format(c, "0%db" % l)[::-1], 2)], [l])      # noqa: E731
    lits = list(b"ACGT" * 8)
    R = [("fixed_distance_beyond_start", pk(F([1, 1], [1, 2]), sb([97, (3, 5)], dw.FIXED_LL, dw.FIXED_DL)), 100),
         ("fixed_length_symbol_286", pk(F([1, 1], [1, 2]), sb(lits, dw.FIXED_LL, dw.FIXED_DL)[:-7], code(*fl[286]), F([0, 0], [5, 7])), 100),
         ("fixed_length_symbol_287", pk(F([1, 1], [1, 2]), sb(lits, dw.FIXED_LL, dw.FIXED_DL)[:-7], code(*fl[287]), F([0, 0], [5, 7])), 100),
         ("fixed_distance_symbol_30", pk(F([1, 1], [1, 2]), sb(lits, dw.FIXED_LL, dw.FIXED_DL)[:-7], code(*fl[257]), code(30, 5), F([0], [7])), 100),
         ("fixed_distance_symbol_31", pk(F([1, 1], [1, 2]), sb(lits, dw.FIXED_LL, dw.FIXED_DL)[:-7], code(*fl[257]), code(31, 5), F([0], [7])), 100)]

    def dyn(ll, dl, toks, hdr=None, tail=True):
        ll, dl = list(ll) + [0] * (286 - len(ll)), list(dl) + [0] * (30 - len(dl))
        head = dw._dynamic_header(ll, dl, hdr or Header(), dw.BlockReport("dynamic", 0, 0))
        return pk(F([1, 2], [1, 2]), head, *([sb(toks, ll, dl)] if tail else []), F([0], [16]))

    ll = [0] * 286
    for s in (65, 67, 71, 84):
        ll[s] = 3
    ll[97], ll[256], ll[257] = 2, 3, 3
    assert dw.kraft(ll) == 1 << 15
    R.append(("dynamic_distance_beyond_start", dyn(ll, [1, 1], [97, (3, 2)] + lits), 100))
    over = list(ll); over[66] = 2
    R.append(("oversubscribed_literal_code", dyn(over, [1, 1], lits, tail=False), 100))
    inc = list(ll); inc[97] = 0
    R.append(("incomplete_literal_code", dyn(inc, [1, 1], lits, tail=False), 100))
    R.append(("oversubscribed_distance_code", dyn(ll, [1, 1, 1], lits, tail=False), 100))
    R.append(("incomplete_distance_code", dyn(ll, [2, 2], lits, tail=False), 100))
    noeob = list(ll); noeob[256], noeob[258] = 0, 3
    R.append(("no_end_of_block_code", dyn(noeob, [1, 1], lits, tail=False), 100))
    good = dw.stream([dynamic(dw.random_parse(fastq_like(5000, 30), 30, 0.6))])
    R.append(("ends_inside_a_symbol", good.raw[:len(good.raw) * 2 // 3], len(good.data)))
    R.append(("ends_before_end_of_block", good.raw[:-1], len(good.data)))
    R.append(("text_longer_than_isize", good.raw, len(good.data) - 5))
    # a repeat code with nothing to repeat: the code-length code has symbols 16 and 0 (one bit each), and 16 comes first
    R.append(("repeat_with_nothing_to_repeat", pk(F([1, 2, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0], [1, 2, 5, 5, 4, 3, 3, 3, 3, 1, 2, 16])), 100))
    R.append(("hlit_287", pk(F([1, 2, 30, 0, 0, 1, 0, 0, 1, 0, 0], [1, 2, 5, 5, 4, 3, 3, 3, 3, 16, 16])), 100))
    R.append(("hdist_31", pk(F([1, 2, 0, 30, 0, 1, 0, 0, 1, 0, 0], [1, 2, 5, 5, 4, 3, 3, 3, 3, 16, 16])), 100))
    R.append(("stored_length_check", pk(F([1, 0, 0], [1, 2, 5])) + b"\x04\x00\xfb\xfe" + b"abcd", 100))
    return R


def zlib_rejects(raw, cap):
    d = zlib.decompressobj(wbits=-15)
    try:
        got = d.decompress(raw)
    except zlib.error:
        return True
    return not d.eof or len(got) > cap


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_corpus_composition():
    """The conditions on the corpus: every named group has cases, a case sits on each side of every threshold, the deepest chain
    is the deepest the format allows, and the shares of the device paths; prints the composition (-s)."""
    cases = corpus()
    groups = {}
    for c in cases:
        groups.setdefault(c.group, []).append(c)
    by = {c.name: c for c in cases}
    print()
    for g in sorted(groups):
        print("group %-24s %3d cases, %8d bytes of text, %7d compressed" % (g, len(groups[g]), sum(len(c.s.data) for c in groups[g]), sum(len(c.s.raw) for c in groups[g])))
    with_text = [c for c in cases if c.s.data]
    for mode in MODES:
        left = predicted(cases, mode)
        print("mode %-2s: %d blocks with text, %d predicted for phase 1 (%s), %d left to k_inflate" % (
            mode, len(with_text), len(with_text) - left if mode != "1" else 0, {"2": "k_inflate_tok", "2c": "k_inflate_tok2", "1": "none"}[mode], left if mode != "1" else len(with_text)))
    assert all(len(groups.get(g, [])) > 0 for g in ("1 long codes", "2 chain depth", "3 periodic", "4 stored after huffman", "5 thresholds", "6 headers", "random"))
    for c in cases:
        assert c.doc and ("inflate_" in c.doc or "mlst_engine" in c.doc or c.group == "random"), c.name
    # thresholds: one case exactly on each side
    assert [by["tokens_%d" % n].s.tokens for n in (TOK_CAP - 1, TOK_CAP, TOK_CAP + 1)] == [TOK_CAP - 1, TOK_CAP, TOK_CAP + 1]
    assert [by["tokens_%d" % n].s.left_to_wave("2") for n in (TOK_CAP - 1, TOK_CAP, TOK_CAP + 1)] == [False, False, True]
    assert [by["symbols_%d" % n].s.left_by_canon for n in (NSYM_L - 1, NSYM_L, NSYM_L + 1)] == [False, False, True]
    assert [by["highest_literal_%d" % v].s.left_by_canon for v in (SYM_ESC - 1, SYM_ESC)] == [False, True]
    assert [by["text_%d" % n].s.left_to_wave("2") for n in (LIT_BASE - 1, LIT_BASE, LIT_BASE + 1, 65536)] == [False, False, True, True]
    assert sorted(len(by["residue_%d" % k].s.data) % 16 for k in range(16)) == list(range(16))
    # the deepest chain: a block of N bytes starts with a literal and every match is at least 3 bytes and at most one link deeper
    # than what it copies, so no chain has more than (N - 1) // 3 links
    depths = {c.name: chain_depth(c.s) for c in groups["2 chain depth"]}
    print("chain depths:", depths)
    assert max(depths.values()) == depths["chain_3_1/lut"] == depths["chain_3_1/canon"] == (LIT_BASE - 1) // 3 and (LIT_BASE - 1) // 3 < 1 << 18
    assert depths["chain_258_258/lut"] == (LIT_BASE - 258) // 258 and min(depths.values()) > 200
    # shares of the device paths
    n = len(with_text)
    assert (n - predicted(cases, "2")) * 3 >= 2 * n, "mode 2: fewer than two thirds of the cases take the lane path"
    assert (n - predicted(cases, "2c")) * 2 >= n, "mode 2c: fewer than half of the cases take the canonical decoder"
    assert predicted(cases, "2") >= 3 and predicted(cases, "2c") > predicted(cases, "2")


def test_every_valid_case_through_the_lookup_table_decoder():
    """mlst_selftest_inflate (csrc/inflate_dev.h on the host): rc 0 and the bytes, for every case"""
    bad = []
    for c in corpus():
        rc, got = inflate(c.s.raw, len(c.s.data))
        if not (rc == 0 and got == c.s.data):
            bad.append((c.name, rc, len(got), len(c.s.data)))
    assert not bad, "%d cases fail: %s" % (len(bad), bad)


def test_every_valid_case_through_the_canonical_decoder():
    """mlst_selftest_inflate_canon (csrc/inflate_canon.h on the host): rc 0, left_to_other_kernel EQUAL to what the writer's report
    predicts from inflate_canon.h:12-13 and :31-35, and the bytes wherever the decoder kept the stream"""
    kept, bad = 0, []
    for c in corpus():
        rc, got, over = inflate_canon(c.s.raw, len(c.s.data))
        if rc != 0:
            bad.append((c.name, "rc", rc))
        elif over != c.s.left_by_canon or (c.friendly and over):
            bad.append((c.name, "left_to_other_kernel", over, [(b.kind, b.lsyms, b.max_lit) for b in c.s.blocks]))
        elif not over:
            kept += 1
            if got != c.s.data:
                bad.append((c.name, "bytes", len(got), len(c.s.data)))
    assert not bad, "%d cases fail: %s" % (len(bad), bad)
    assert kept * 2 >= len(corpus())


def _lib_payloads():
    return [p[:65280] for p in payloads()] + [fastq_like(65280, 40), fastq_like(777, 41), bam_like(50000, 42)]


@pytest.mark.parametrize("level", [0, 1, 6, 9, 12])
def test_libdeflate_streams_on_the_host(level):
    """the second producer: libdeflate's streams (accepted by zlib first) through both host decoders"""
    if dw.libdeflate() is None:
        pytest.skip("libdeflate.so.0 is not installed")
    for k, data in enumerate(_lib_payloads()):
        raw = dw.libdeflate_stream(data, level)
        rc, got = inflate(raw, len(data))
        assert rc == 0 and got == data, (k, level)
        rc, got, over = inflate_canon(raw, len(data))
        # (no report exists for a stream libdeflate wrote, so which way `over` has to come out cannot be said here; the corpus test
        # above asserts it both ways)
        assert rc == 0 and (over or got == data), (k, level)


# The five rejected streams that are fixed-code blocks.  csrc/inflate_canon.h does not decode the fixed code at all (:230: 288 symbols
# in use): it hands such a stream over without an error, and on the device k_inflate -- inflate_wave.h, table-driven like inflate_dev.h,
# whose host twin mlst_selftest_inflate has to reject every one -- decodes it.  Only the fixed code gives the symbols 286 / 287 / 30 / 31
# a code, so these are the streams that reach the selects at inflate_lane.h:98 and inflate_wave.h:315 / :332.
HANDED_OVER_BY_CANON = ("fixed_distance_beyond_start", "fixed_length_symbol_286", "fixed_length_symbol_287", "fixed_distance_symbol_30", "fixed_distance_symbol_31")
REJECTED_NAMES = HANDED_OVER_BY_CANON + (
    "dynamic_distance_beyond_start", "oversubscribed_literal_code", "incomplete_literal_code", "oversubscribed_distance_code", "incomplete_distance_code",
    "no_end_of_block_code", "ends_inside_a_symbol", "ends_before_end_of_block", "text_longer_than_isize", "repeat_with_nothing_to_repeat", "hlit_287", "hdist_31",
    "stored_length_check")


def host_verdicts():
    """-> {name: (rc of mlst_selftest_inflate, rc of mlst_selftest_inflate_canon, handed over by it)} of the 18 rejected streams"""
    out = {}
    for name, raw, cap in rejected_cases():
        rc, got = inflate(raw, cap)
        rc2, got2, over = inflate_canon(raw, cap)
        assert len(got) <= cap and len(got2) <= cap, name
        out[name] = (rc, rc2, over)
    return out


def test_rejected_streams_on_the_host():
    """Every one of the 18 rejected streams: zlib refuses it, mlst_selftest_inflate returns an error, and so does
    mlst_selftest_inflate_canon -- for the 13 streams it decodes.  The five of HANDED_OVER_BY_CANON it must hand over (rc 0,
    left_to_other_kernel): it never enters a fixed-code block, so it can have no verdict on what is wrong inside one."""
    cases = rejected_cases()
    assert tuple(name for name, _, _ in cases) == REJECTED_NAMES and len(cases) == 18
    for name, raw, cap in cases:
        assert zlib_rejects(raw, cap), name
    for name, (rc, rc2, over) in host_verdicts().items():
        assert rc < 0, (name, rc)
        if name in HANDED_OVER_BY_CANON:
            assert (rc2, over) == (0, True), (name, rc2, over)
        else:
            assert rc2 < 0 and not over, (name, rc2, over)


# ----------------------------------------------------------------------------------------------------------------- GPU
def set_decoder(monkeypatch, mode):
    monkeypatch.setenv("MLST_INFLATE_MODE", mode[0])      # (read when an engine inflates for the first time)
    monkeypatch.setenv("MLST_INFLATE_TOK", "2" if mode == "2c" else "1")


def ordinary(k):
    data = fastq_like(1500 + 37 * (k % 50), 900 + k % 50)
    return data, deflate(data, (1, 6, 9)[k % 3])


def check_buffer(eng, items, mode, what, crc=True):
    """items: [(name, raw, data, left to k_inflate?)] as ONE buffer of BGZF blocks: the bytes, which kernel ran, and the CRC-32s"""
    buf = b"".join(dw.bgzf(raw, data) for _, raw, data, _ in items)
    got = eng.inflate_bgzf(buf)
    want = b"".join(data for _, _, data, _ in items)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(len(a), len(b))
        diff = np.nonzero(a[:n] != b[:n])[0]
        at = int(diff[0]) if len(diff) else n
        off = 0
        for name, _, data, _ in items:
            if at < off + len(data):
                raise AssertionError("%s, mode %s: %d bytes for %d; first difference in case %s at its byte %d of %d (got %r, want %r; %d bytes differ in all)" % (
                    what, mode, len(got), len(want), name, at - off, len(data), got[at:at + 8], want[at:at + 8], len(diff)))
            off += len(data)
        raise AssertionError("%s, mode %s: %d bytes for %d" % (what, mode, len(got), len(want)))
    n_blk, left = eng.inflate_paths()
    with_text = [it for it in items if it[2]]
    want_left = 0 if mode == "1" else sum(1 for it in with_text if it[3])
    assert (n_blk, left) == (len(with_text), want_left), "%s, mode %s: %d of %d blocks were left to k_inflate, the headers' rules say %d" % (what, mode, left, n_blk, want_left)
    if not crc:
        return left
    crcs = eng.bgzf_block_crcs(buf)
    want_crc = np.array([zlib.crc32(it[2]) & 0xFFFFFFFF for it in with_text], np.uint32)
    bad = np.nonzero(crcs != want_crc)[0] if len(crcs) == len(want_crc) else [0]
    assert len(bad) == 0, "%s, mode %s: CRC-32 of case %s" % (what, mode, with_text[int(bad[0])][0])
    return left


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_device_decoders_on_the_whole_corpus(mode, monkeypatch):
    """Every valid case as ONE buffer of BGZF blocks through Engine.inflate_bgzf, in two orders -- as listed (the corpus' last case is
    the last block of the buffer: the clamp at inflate_dev.h:62), and reversed with an ordinary block between every two cases, so
    that the blocks of all kinds share waves and their text starts at every residue mod 16 (inflate_lane.h:317).  The bytes equal
    the data, the CRC-32s equal zlib's, and the number of blocks phase 1 left to k_inflate EQUALS the prediction."""
    from metamlst_amd.engine import Engine
    set_decoder(monkeypatch, mode)
    cases = corpus()
    eng = Engine(0)
    items = [(c.name, c.s.raw, c.s.data, c.s.left_to_wave(mode, TOK_CAP, LIT_BASE)) for c in cases]
    left = check_buffer(eng, items, mode, "as listed")
    print("\nmode %s: %d blocks with text, %d left to k_inflate (predicted %d)" % (mode, sum(1 for it in items if it[2]), left, predicted(cases, mode) if mode != "1" else 0))
    mixed, off, starts = [], 0, set()
    for k, it in enumerate(reversed(items)):
        if not it[3] and it[2]:
            starts.add(off % 16)
        mixed.append(it)
        data, raw = ordinary(k)
        mixed.append(("ordinary_%d" % k, raw, data, False))
        off += len(it[2]) + len(data)
    assert starts == set(range(16))
    check_buffer(eng, mixed, mode, "reversed and interleaved")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_named_case_at_the_ends_of_a_wave_and_of_the_buffer(mode, monkeypatch):
    """Position in the launch: every named case once as lane 63 of a wave of ordinary blocks and the LAST block of the buffer (the
    16 bytes of padding behind it are all the refill may read: inflate_dev.h:62), and once as lane 0 with 63 ordinary blocks behind."""
    from metamlst_amd.engine import Engine
    set_decoder(monkeypatch, mode)
    eng = Engine(0)
    ords = [("ordinary_%d" % k,) + ordinary(k)[::-1] + (False,) for k in range(63)]
    for c in named_cases_cached():
        it = (c.name, c.s.raw, c.s.data, c.s.left_to_wave(mode, TOK_CAP, LIT_BASE))
        check_buffer(eng, ords + [it], mode, c.name + " as lane 63, last of the buffer", crc=False)
        check_buffer(eng, [it] + ords, mode, c.name + " as lane 0", crc=False)
    eng.close()


def named_cases_cached():
    return [c for c in corpus() if c.group != "random"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_libdeflate_streams_on_the_device(mode, monkeypatch):
    """libdeflate's streams (levels 0, 1, 6, 9, 12) of the payloads of test_inflate.py and of FASTQ and BAM-like text in one buffer"""
    if dw.libdeflate() is None:
        pytest.skip("libdeflate.so.0 is not installed")
    from metamlst_amd.engine import Engine
    set_decoder(monkeypatch, mode)
    blocks, want = [], []
    for level in (0, 1, 6, 9, 12):
        for data in _lib_payloads():
            raw = dw.libdeflate_stream(data, level)
            if len(raw) + 26 <= 65536:
                blocks.append(_bgzf_raw(raw, data))
                want.append(data)
    assert len(want) >= 40
    eng = Engine(0)
    got = eng.inflate_bgzf(b"".join(blocks))
    assert len(got) == sum(map(len, want))
    off = 0
    for k, data in enumerate(want):
        assert got[off:off + len(data)] == data, "libdeflate stream %d (mode %s)" % (k, mode)
        off += len(data)
    assert eng.bgzf_block_crcs(b"".join(blocks)).tolist() == [zlib.crc32(d) & 0xFFFFFFFF for d in want if d]
    eng.close()


def reencode(data: bytes, seed: int) -> bytes:
    """a BGZF block of data by the random parser (another seed where the stream does not fit the format's 64 KiB)"""
    for k in range(8):
        s = dw.random_stream(data, seed + 7919 * k, bool((seed + k) & 1), 0.85)
        if len(s.raw) + 26 <= 65536:
            return _bgzf_raw(s.raw, s.data)
    raise AssertionError("no encoding of %d bytes fits a BGZF block" % len(data))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fastq_reencoded_by_the_random_parser_types_like_the_plain_text(mode, monkeypatch):
    """3,000 reads re-encoded block by block by the random parser, in blocks whose sizes are no multiples of 16, through
    submit_fastq_bgzf in three pieces of which the first two end inside a record: record count and statistics equal those of
    submit_fastq of the plain text (the newline cells counted during write-out, inflate_lane.h:326-337, feed the parser)."""
    import fixtures as fx
    from metamlst_amd import synth
    from metamlst_amd.engine import Engine
    set_decoder(monkeypatch, mode)
    db, idx = fx.ecoli_small(80)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][2], size=100_000)
    b, q = synth.sample_reads(g, 3000)
    text = b"".join(b"@r%d\n" % k + b[k].tobytes() + b"\n+\n" + q[k].tobytes() + b"\n" for k in range(len(b)))
    blocks, sizes, at, k = [], [], 0, 0
    while at < len(text):
        n = (39989, 64999, 12345, 50001, 7)[k % 5]
        blocks.append(reencode(text[at:at + n], 50 + k))
        sizes.append(len(text[at:at + n]))
        at += n
        k += 1
    assert len(blocks) >= 12
    eng = Engine(0)
    eng.load_reference(idx)
    eng.set_bgzf_verify(True)
    eng.submit_fastq(text)
    want = eng.stats()
    eng.reset_sample()
    cut1, cut2 = len(blocks) // 3, 2 * len(blocks) // 3
    heads = set(np.cumsum([0] + [len(b"@r%d\n" % k) + 2 * len(b[k]) + 4 for k in range(len(b))]).tolist())      # where the records start
    assert len(text) in heads
    for end in (sum(sizes[:cut1]), sum(sizes[:cut2])):
        assert 0 < end < len(text) and end not in heads, "a piece ends between two records, not inside one"
    n = eng.submit_fastq_bgzf(b"".join(blocks[:cut1]), final=False)
    n += eng.submit_fastq_bgzf(b"".join(blocks[cut1:cut2]), final=False)
    n += eng.submit_fastq_bgzf(b"".join(blocks[cut2:]) + _bgzf_raw(deflate(b"", 6), b""), final=True)
    assert n == 3000
    fx.assert_stats_equal(eng.stats(), want)
    eng.close()


@pytest.mark.gpu
def test_bam_reencoded_by_the_random_parser_and_by_libdeflate(tmp_path):
    """The record zoo of test_bam_gpu.py with every BGZF block re-encoded by the random parser and, where the library is
    installed, by libdeflate: the device path's statistics equal the host path's."""
    import golden_util as gu
    import test_bam_gpu as tb
    from metamlst_amd.index import load_index
    idx = load_index(gu.golden_db())
    refs, recs = tb.zoo(idx, 6000)
    path = tb.write(tmp_path / "zoo.bam", refs, recs)
    raw = open(path, "rb").read()
    texts, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        texts.append(zlib.decompress(raw[at + 18:at + size - 8], -15))
        at += size
    assert len(texts) > 10
    _, want = tb.host_stats(idx, None, path)
    variants = {"random": b"".join(reencode(t, 300 + k) if t else _bgzf_raw(deflate(b"", 6), b"") for k, t in enumerate(texts))}
    if dw.libdeflate() is not None:
        variants["libdeflate"] = b"".join(_bgzf_raw(dw.libdeflate_stream(t, (1, 6, 9, 12)[k % 4]), t) for k, t in enumerate(texts))
    eng = tb.make_engine(idx, verify=True)
    for name, data in variants.items():
        p = str(tmp_path / (name + ".bam"))
        open(p, "wb").write(data)
        n, got = tb.device_stats(eng, p)
        assert n == 6000, name
        tb.assert_stats_equal(got, want)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_rejected_streams_on_the_device(mode, monkeypatch):
    """All 18 rejected streams, each in a launch of its own, once: an MlstError comes back.  A stream goes to the device only
    after every host decoder that decodes it has returned an error: both for 13 of them; for the five fixed-code streams
    mlst_selftest_inflate alone, because inflate_canon.h hands them over undecoded (mode 2c: to k_inflate, like modes 2 and 1 table
    driven).  They are the only streams that reach the symbol selects at inflate_lane.h:98 and inflate_wave.h:315 / :332;
    inflate_lane.h:111 (ds >= 30) stays unreached: the fixed distance code is built from 30 lengths, so the codes of 30 and 31 end
    in long_code's E_SYMBOL before it."""
    from metamlst_amd.engine import Engine, MlstError
    set_decoder(monkeypatch, mode)
    verdicts = host_verdicts()
    eng = Engine(0)
    sent = []
    for name, raw, cap in rejected_cases():
        rc, rc2, over = verdicts[name]
        if not (rc < 0 and (rc2 < 0 or (over and name in HANDED_OVER_BY_CANON))):
            continue
        blk = (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", 0, cap))
        with pytest.raises(MlstError):
            eng.inflate_bgzf(blk)
        sent.append(name)
    assert tuple(sent) == REJECTED_NAMES
    eng.close()
