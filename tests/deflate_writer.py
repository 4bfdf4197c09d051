"""A deflate WRITER for tests: an explicit description (tokens, their split into deflate blocks, each block's kind, code lengths
and header encoding) -> a raw RFC 1951 stream, plus a report of what was written.  Test infrastructure like bam_writer.py;
the product package never imports it.

zlib only ever writes a narrow subset of what the format allows (greedy / lazy longest matches, one block kind per
~16 K symbols, minimal headers).  The device decoders (csrc/inflate_lane.h, inflate_canon.h, inflate_wave.h) have paths
that such streams never reach; tests/test_inflate_streams.py drives them with streams built here.

The reference is zlib's inflate: stream() runs every stream it returns through zlib.decompressobj(wbits=-15) and raises
unless the data comes back exactly, at the end of the stream, with no unused input.

A token is an int (a literal byte) or a tuple (length 3..258, distance 1..32768).
"""
from __future__ import annotations

import bisect
import ctypes as C
import heapq
import zlib
from dataclasses import dataclass, field

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 30

_LBASE = np.array(LBASE, np.int64)
_LEXT = np.array(LEXT, np.int64)
_DBASE = np.array(DBASE, np.int64)
_DEXT = np.array(DEXT, np.int64)
_LSYM = np.zeros(259, np.int64)                       # length -> length symbol (0..28); 258 has a symbol of its own
for _s in range(28):
    _LSYM[LBASE[_s]:LBASE[_s] + (1 << LEXT[_s])] = _s
_LSYM[258] = 28


def lsym(n: int) -> int:
    return int(_LSYM[n])


def dsym(d: int) -> int:
    return int(np.searchsorted(_DBASE, d, side="right")) - 1


# ---------------------------------------------------------------------------------------------------------------- codes
def kraft(lengths, maxbits: int = 15) -> int:
    """sum of 2^(maxbits - l) over the lengths in use; a complete code has 2^maxbits"""
    return sum(1 << (maxbits - l) for l in lengths if l)


def canon(lengths):
    """code lengths -> {symbol: (code sent most significant bit first, length)} (RFC 1951, 3.2.2)"""
    cnt = [0] * 17
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + cnt[l - 1]) << 1
        nxt[l] = c
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def lengths_from_counts(counts, limit: int = 15):
    """Huffman code lengths of the symbols with a count, at most `limit` bits: complete, or one code of 1 bit where a single
    symbol has a count.  (Too deep a tree: the counts are flattened until it fits -- not optimal, always legal.)"""
    counts = [int(c) for c in counts]
    used = [s for s, c in enumerate(counts) if c > 0]
    out = [0] * len(counts)
    if not used:
        return out
    if len(used) == 1:
        out[used[0]] = 1
        return out
    w = {s: counts[s] for s in used}
    while True:
        heap = [(c, s, (s,)) for s, c in w.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        tie = len(counts)
        while len(heap) > 1:
            c1, _, m1 = heapq.heappop(heap)
            c2, _, m2 = heapq.heappop(heap)
            for s in m1 + m2:
                depth[s] += 1
            heapq.heappush(heap, (c1 + c2, tie, m1 + m2))
            tie += 1
        if max(depth.values()) <= limit:
            break
        w = {s: max(1, c >> 1) for s, c in w.items()}
    for s in used:
        out[s] = depth[s]
    return out


def push_deep(lengths, sym: int, fillers, depth: int = 15):
    """Shape a complete code: the leaf of `sym` (a bits) becomes a chain that ends `depth` bits down -- `sym` gets `depth` bits,
    and the (depth - a) symbols of `fillers`, none of which has a code yet, take the chain's siblings: a+1, a+2, ..., depth-1,
    depth bits.  The code stays complete; the fillers need not occur in the block."""
    a = lengths[sym]
    assert 0 < a < depth and len(fillers) == depth - a and all(lengths[f] == 0 for f in fillers) and len(set(fillers)) == len(fillers)
    out = list(lengths)
    out[sym] = depth
    for k, f in enumerate(fillers):
        out[f] = min(a + 1 + k, depth) if k < depth - a - 1 else depth
    return out


def use_exactly(lengths, n: int, spare, maxbits: int = 15):
    """Shape a complete code until exactly `n` symbols have a code: a leaf is split in two (its symbol and the next of `spare`,
    both one bit longer) until the count is reached; the longest leaf that still can be split goes first, so the short codes
    of the frequent symbols stay."""
    out = list(lengths)
    spare = [s for s in spare if out[s] == 0]
    have = sum(1 for l in out if l)
    assert have <= n <= have + len(spare), (have, n, len(spare))
    for f in spare[:n - have]:
        s = max((k for k, l in enumerate(out) if 0 < l < maxbits), key=lambda k: (out[k], k))
        out[s] += 1
        out[f] = out[s]
    return out


# ------------------------------------------------------------------------------------------------------------ bit pieces
def _fields(vals, nbits):
    """fields (value, number of bits), each written least significant bit first -> an array of bits"""
    vals = np.asarray(vals, np.int64)
    nbits = np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    if total == 0:
        return np.zeros(0, np.uint8)
    starts = np.cumsum(nbits) - nbits
    k = np.arange(total, dtype=np.int64) - np.repeat(starts, nbits)
    return ((np.repeat(vals, nbits) >> k) & 1).astype(np.uint8)


def _code_tables(lengths):
    """-> (code as the stream wants it: bit-reversed, so that it goes out least significant bit first; length), per symbol"""
    rev = np.zeros(len(lengths), np.int64)
    ln = np.array(lengths, np.int64)
    for s, (c, l) in canon(lengths).items():
        rev[s] = int(format(c, "0%db" % l)[::-1], 2)
    return rev, ln


def _token_arrays(toks):
    n = len(toks)
    lit = np.full(n, -1, np.int64)
    mlen = np.zeros(n, np.int64)
    dist = np.zeros(n, np.int64)
    for i, t in enumerate(toks):
        if isinstance(t, tuple):
            mlen[i], dist[i] = t
        else:
            lit[i] = t
    return lit, mlen, dist


def token_counts(toks):
    """-> (286 literal / length counts with the end-of-block symbol counted once, 30 distance counts)"""
    lit, mlen, dist = _token_arrays(toks)
    m = lit < 0
    assert np.all((lit[~m] >= 0) & (lit[~m] < 256)) and np.all((mlen[m] >= 3) & (mlen[m] <= 258)) and np.all((dist[m] >= 1) & (dist[m] <= 32768))
    lc = np.bincount(np.concatenate([lit[~m], 257 + _LSYM[mlen[m]], [256]]), minlength=286)
    dc = np.bincount(np.searchsorted(_DBASE, dist[m], side="right") - 1, minlength=30)
    return [int(x) for x in lc], [int(x) for x in dc]


def _symbol_bits(toks, ll, dl):
    lit, mlen, dist = _token_arrays(toks)
    m = lit < 0
    ls = np.where(m, 257 + _LSYM[np.where(m, mlen, 3)], lit)
    ds = np.where(m, np.searchsorted(_DBASE, np.where(m, dist, 1), side="right") - 1, 0)
    lrev, lln = _code_tables(ll)
    drev, dln = _code_tables(dl) if any(dl) else (np.zeros(30, np.int64), np.zeros(30, np.int64))
    if np.any(lln[ls] == 0) or lln[256] == 0 or np.any(dln[ds[m]] == 0):
        raise ValueError("a token's symbol has no code")
    n = len(toks)
    vals = np.zeros((n + 1, 4), np.int64)
    nb = np.zeros((n + 1, 4), np.int64)
    vals[:n, 0], nb[:n, 0] = lrev[ls], lln[ls]
    li = np.where(m, ls - 257, 0)
    vals[:n, 1], nb[:n, 1] = np.where(m, mlen - _LBASE[li], 0), np.where(m, _LEXT[li], 0)
    vals[:n, 2], nb[:n, 2] = np.where(m, drev[ds], 0), np.where(m, dln[ds], 0)
    vals[:n, 3], nb[:n, 3] = np.where(m, dist - _DBASE[ds], 0), np.where(m, _DEXT[ds], 0)
    vals[n, 0], nb[n, 0] = lrev[256], lln[256]                                     # end of block
    return _fields(vals.ravel(), nb.ravel())


# --------------------------------------------------------------------------------------------------------- descriptions
@dataclass
class Header:
    """How a dynamic block's code lengths are sent.  hlit / hdist: symbols sent (None: up to the last one with a code; more: the
    tail is sent as zeros); hclen: code-length code lengths sent (None: as few as the format allows); repeats: use the repeat
    codes 16 / 17 / 18; cross: a run may go on from the literal / length lengths into the distance lengths; cl_lengths: the 19
    lengths of the code-length code (None: built from the counts, at most 7 bits); cl_deep: that built code shaped so that its longest
    code has 7 bits (push_deep with code-length symbols the header does not use)."""
    hlit: int | None = None
    hdist: int | None = None
    hclen: int | None = None
    repeats: bool = True
    cross: bool = True
    cl_lengths: list | None = None
    cl_deep: bool = False


@dataclass
class Block:
    kind: str                                    # "stored" | "fixed" | "dynamic"
    toks: list = field(default_factory=list)     # stored: literals only (its bytes)
    ll: list | None = None                       # dynamic: literal / length code lengths (up to 286) ...
    dl: list | None = None                       # ... and distance code lengths (up to 30); None: built from the block's counts
    hdr: Header = field(default_factory=Header)


def stored(data: bytes) -> Block:
    assert len(data) <= 65535
    return Block("stored", list(data))


def fixed(toks) -> Block:
    return Block("fixed", list(toks))


def dynamic(toks, ll=None, dl=None, hdr: Header | None = None) -> Block:
    return Block("dynamic", list(toks), None if ll is None else list(ll), None if dl is None else list(dl), hdr or Header())


@dataclass
class BlockReport:
    kind: str
    tokens: int          # as the device counts them (csrc/inflate_lane.h): a literal 1, a match 1, a stored run that is not empty 2
    out_bytes: int
    lsyms: int = 0       # literal / length symbols with a code (the fixed code: 288)
    dsyms: int = 0
    max_lit: int = -1    # highest literal with a code
    max_llen: int = 0    # longest literal / length code; the longest one a token of the block uses: max_llen_used
    max_dlen: int = 0
    max_llen_used: int = 0
    max_dlen_used: int = 0
    hlit: int = 0
    hdist: int = 0
    hclen: int = 0
    max_cllen: int = 0
    crossed: bool = False      # a repeat code ran from the literal / length lengths into the distance lengths
    bit_phase: int = 0         # position (mod 8) of the block's first header bit in the stream


@dataclass
class Stream:
    raw: bytes
    data: bytes
    blocks: list
    toks: list = field(default_factory=list)      # the tokens of all blocks in order (a stored block's bytes as literals)

    @property
    def tokens(self) -> int:
        return sum(b.tokens for b in self.blocks)

    @property
    def left_by_canon(self) -> bool:
        """csrc/inflate_canon.h leaves the stream to the other kernel: a Huffman block whose literal / length code has more than
        NSYM_L = 192 symbols in use, or a code for a literal of SYM_ESC = 224 or more (the fixed code has both)"""
        return any(b.kind != "stored" and (b.lsyms > 192 or b.max_lit >= 224) for b in self.blocks)

    def left_to_wave(self, mode: str, tok_cap: int = 24576, lit_base: int = 65280) -> bool:
        """Does phase 1 of the two-kernel inflate leave this BGZF block to k_inflate?  mode "2": k_inflate_tok, "2c": k_inflate_tok2,
        "1": there is no phase 1.  (Blocks without text are not launched at all.)"""
        if mode == "1" or not self.data:
            return False
        return len(self.data) > lit_base or self.tokens > tok_cap or (mode == "2c" and self.left_by_canon)


def replay(toks, history: bytes = b"") -> bytes:
    o = bytearray(history)
    for t in toks:
        if isinstance(t, tuple):
            n, d = t
            if d > len(o):
                raise ValueError("distance beyond the start of the stream")
            if d >= n:
                o += o[len(o) - d:len(o) - d + n]
            else:
                for _ in range(n):
                    o.append(o[-d])
        else:
            o.append(t)
    return bytes(o[len(history):])


# --------------------------------------------------------------------------------------------------- the header's lengths
def _rle(seq, repeats: bool):
    """code lengths -> code-length symbols [(symbol, extra value, extra bits)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if not repeats:
            out += [(v, 0, 0)] * run
        elif v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11, 7)); run -= k
            if run >= 3:
                out.append((17, run - 3, 3)); run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3, 2)); run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


def _dynamic_header(ll, dl, hdr: Header, rep: BlockReport):
    hlit = hdr.hlit if hdr.hlit is not None else max(257, max(s for s, l in enumerate(ll) if l) + 1)
    hdist = hdr.hdist if hdr.hdist is not None else max(1, max([s for s, l in enumerate(dl) if l], default=0) + 1)
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(ll[hlit:]) and not any(dl[hdist:])
    a, b = list(ll[:hlit]) + [0] * (hlit - len(ll)), list(dl[:hdist]) + [0] * (hdist - len(dl))
    if hdr.cross:
        syms = _rle(a + b, hdr.repeats)
        at = 0
        for s, x, _ in syms:
            n = 1 if s < 16 else (3 + x if s < 18 else 11 + x)
            rep.crossed = rep.crossed or (at < hlit < at + n)
            at += n
    else:
        syms = _rle(a, hdr.repeats) + _rle(b, hdr.repeats)
    cl = hdr.cl_lengths
    if cl is None:
        cl = lengths_from_counts(np.bincount([s for s, _, _ in syms], minlength=19), 7)
        if sum(1 for l in cl if l) == 1:                      # (the code-length code has to be complete: a second symbol)
            cl[[s for s in range(19) if not cl[s]][0]] = 1
        if hdr.cl_deep and max(cl) < 7:
            s0 = max((s for s in range(19) if cl[s]), key=lambda s: (cl[s], s))
            cl = push_deep(cl, s0, [s for s in range(19) if not cl[s]][:7 - cl[s0]], 7)
    assert len(cl) == 19 and max(cl) <= 7 and kraft(cl, 7) == 1 << 7 and all(cl[s] for s, _, _ in syms), "code-length code"
    hclen = hdr.hclen if hdr.hclen is not None else max(4, max(k for k, s in enumerate(CL_ORDER) if cl[s]) + 1)
    assert 4 <= hclen <= 19 and not any(cl[s] for s in CL_ORDER[hclen:])
    rep.hlit, rep.hdist, rep.hclen, rep.max_cllen = hlit, hdist, hclen, max(cl)
    crev, cln = _code_tables(cl)
    vals = [hlit - 257, hdist - 1, hclen - 4] + [cl[s] for s in CL_ORDER[:hclen]]
    nb = [5, 5, 4] + [3] * hclen
    for s, x, xb in syms:
        vals += [int(crev[s]), x]
        nb += [int(cln[s]), xb]
    return _fields(vals, nb)


def _check_code(lengths, what: str, n_max: int):
    assert len(lengths) <= n_max and all(0 <= l <= 15 for l in lengths), what
    k, used = kraft(lengths), sum(1 for l in lengths if l)
    if not (k == 1 << 15 or (used == 1 and max(lengths) == 1) or (used == 0 and what == "distance")):
        raise ValueError("%s code is neither complete nor a single code of one bit" % what)


def stream(blocks, check: bool = True) -> Stream:
    """The deflate stream of `blocks` (the last one is marked final), the bytes it stands for, and the report.
    check=False (streams that are meant to be rejected) skips zlib."""
    pieces, reports, nbits = [], [], 0
    data = bytearray()
    for bi, blk in enumerate(blocks):
        last = 1 if bi == len(blocks) - 1 else 0
        text = replay(blk.toks, bytes(data))
        rep = BlockReport(blk.kind, 0, len(text), bit_phase=nbits & 7)
        if blk.kind == "stored":
            assert all(isinstance(t, int) for t in blk.toks)
            head = _fields([last, 0], [1, 2])
            pad = np.zeros(-(nbits + 3) & 7, np.uint8)
            body = np.frombuffer(len(text).to_bytes(2, "little") + (len(text) ^ 0xFFFF).to_bytes(2, "little") + text, np.uint8)
            piece = np.concatenate([head, pad, np.unpackbits(body, bitorder="little")])
            rep.tokens = 2 if text else 0
        else:
            if blk.kind == "fixed":
                ll, dl, head = FIXED_LL, FIXED_DL, _fields([last, 1], [1, 2])
                rep.lsyms, rep.dsyms, rep.max_lit, rep.max_llen, rep.max_dlen = 288, 30, 255, 9, 5
            else:
                ll, dl = blk.ll, blk.dl
                if ll is None or dl is None:
                    lc, dc = token_counts(blk.toks)
                    ll = lengths_from_counts(lc) if ll is None else ll
                    dl = lengths_from_counts(dc) if dl is None else dl
                ll, dl = list(ll) + [0] * (286 - len(ll)), list(dl) + [0] * (30 - len(dl))
                _check_code(ll, "literal / length", 286)
                _check_code(dl, "distance", 30)
                head = np.concatenate([_fields([last, 2], [1, 2]), _dynamic_header(ll, dl, blk.hdr, rep)])
                rep.lsyms, rep.dsyms = sum(1 for l in ll if l), sum(1 for l in dl if l)
                rep.max_lit = max((s for s in range(256) if ll[s]), default=-1)
                rep.max_llen, rep.max_dlen = max(ll), max(dl)
            lc, dc = token_counts(blk.toks)
            rep.max_llen_used = max(ll[s] for s in range(len(lc)) if lc[s])
            rep.max_dlen_used = max((dl[s] for s in range(30) if dc[s]), default=0)
            piece = np.concatenate([head, _symbol_bits(blk.toks, ll, dl)])
            rep.tokens = len(blk.toks)
        pieces.append(piece)
        nbits += len(piece)
        data += text
        reports.append(rep)
    raw = np.packbits(np.concatenate(pieces), bitorder="little").tobytes()
    s = Stream(raw, bytes(data), reports, [t for blk in blocks for t in blk.toks])
    if check:
        zlib_accepts(s.raw, s.data)
    return s


def zlib_accepts(raw: bytes, data: bytes) -> None:
    d = zlib.decompressobj(wbits=-15)
    got = d.decompress(raw)
    if got != data or not d.eof or d.unused_data:
        raise ValueError("zlib does not return the data from this stream (%d of %d bytes, eof %s, %d unused)" % (len(got), len(data), d.eof, len(d.unused_data)))


def bgzf(raw: bytes, data: bytes) -> bytes:
    from test_inflate import _bgzf_raw
    assert len(raw) + 26 <= 65536 and len(data) <= 65536, "a BGZF block holds at most 64 KiB, compressed and not"
    return _bgzf_raw(raw, data)


# ------------------------------------------------------------------------------------------------------- the random parser
def random_parse(data: bytes, seed: int, p_match: float = 0.7, p_longest: float = 0.3):
    """data -> tokens.  At every position, with probability p_match, ONE of all the earlier occurrences (within 32,768 bytes) of
    the next three bytes is chosen at random -- not the nearest, not the one with the longest match; matches that overlap
    themselves included -- and a random part of what matches there is taken (all of it with probability p_longest)."""
    rng = np.random.default_rng(seed)
    n = len(data)
    grams: dict = {}
    for j in range(n - 2):
        grams.setdefault(data[j:j + 3], []).append(j)
    toks, i = [], 0
    coin = rng.random(n + 1)
    pick = rng.random(n + 1)
    cut = rng.random(n + 1)
    while i < n:
        took = False
        if i + 3 <= n and coin[i] < p_match:
            pos = grams[data[i:i + 3]]
            lo, hi = bisect.bisect_left(pos, i - 32768), bisect.bisect_left(pos, i)
            if hi > lo:
                j = pos[lo + int(pick[i] * (hi - lo))]
                top, m = min(258, n - i), 3
                while m < top and data[j + m] == data[i + m]:
                    m += 1
                if cut[i] >= p_longest:
                    m = 3 + int((cut[i] - p_longest) / (1.0 - p_longest) * (m - 2))
                toks.append((m, i - j))
                i += m
                took = True
        if not took:
            toks.append(data[i])
            i += 1
    return toks


def random_split(toks, seed: int, max_blocks: int = 6):
    """tokens -> runs of tokens (deflate blocks) at random cuts"""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, max_blocks + 1))
    cuts = sorted(set(int(c) for c in rng.integers(0, len(toks) + 1, k - 1))) if toks else []
    edges = [0] + cuts + [len(toks)]
    return [toks[a:b] for a, b in zip(edges[:-1], edges[1:])]


def random_block(toks, seed: int, canon_friendly: bool = False) -> Block:
    """A run of tokens as a stored (literals only), fixed or dynamic block with a randomly shaped code and header.
    canon_friendly: a dynamic block with at most 192 literal / length symbols in use and none for a literal of 224 or more
    where the tokens allow it (what csrc/inflate_canon.h decodes itself)."""
    rng = np.random.default_rng(seed)
    only_lits = all(isinstance(t, int) for t in toks)
    kind = int(rng.integers(0, 8))
    if only_lits and len(toks) <= 65535 and kind == 0 and not canon_friendly:
        return stored(bytes(toks))
    if kind == 1 and not canon_friendly:
        return fixed(toks)
    lc, dc = token_counts(toks)
    ll, dl = lengths_from_counts(lc), lengths_from_counts(dc)
    free_l = [s for s in range(286) if not ll[s] and (not canon_friendly or s < 224 or s > 256)]
    rng.shuffle(free_l)
    shape = int(rng.integers(0, 4))
    used = [s for s in range(286) if ll[s]]
    if len(used) >= 2:
        if shape == 1:                                   # a long chain under one of the block's own symbols
            s = used[int(rng.integers(len(used)))]
            need = 15 - ll[s]
            if 0 < need <= len(free_l):
                ll = push_deep(ll, s, free_l[:need])
        elif shape == 2:                                 # more symbols in use than the block needs
            room = (192 if canon_friendly else 286) - len(used)
            if room > 0:
                ll = use_exactly(ll, len(used) + int(rng.integers(0, min(room, len(free_l)) + 1)), free_l)
    used_d = [s for s in range(30) if dl[s]]
    if len(used_d) >= 2 and shape == 3:
        s = used_d[int(rng.integers(len(used_d)))]
        free_d = [k for k in range(30) if not dl[k]]
        need = 15 - dl[s]
        if 0 < need <= len(free_d):
            dl = push_deep(dl, s, free_d[:need])
    hdr = Header(repeats=bool(rng.integers(0, 4)), cross=bool(rng.integers(0, 2)))
    if rng.integers(0, 3) == 0:
        hdr.hlit = 286
    if rng.integers(0, 3) == 0:
        hdr.hdist = 30
    if rng.integers(0, 3) == 0:
        hdr.hclen = 19
    return dynamic(toks, ll, dl, hdr)


def random_stream(data: bytes, seed: int, canon_friendly: bool = False, p_match: float = 0.7) -> Stream:
    toks = random_parse(data, seed, p_match)
    return stream([random_block(run, seed * 131 + k, canon_friendly) for k, run in enumerate(random_split(toks, seed + 1))])


# ------------------------------------------------------------------------------------------- a second producer: libdeflate
_LIBDEFLATE = None


def libdeflate():
    """libdeflate through ctypes, or None where the library is not installed"""
    global _LIBDEFLATE
    if _LIBDEFLATE is None:
        try:
            lib = C.CDLL("libdeflate.so.0")
            lib.libdeflate_alloc_compressor.restype = C.c_void_p
            lib.libdeflate_alloc_compressor.argtypes = [C.c_int]
            lib.libdeflate_deflate_compress.restype = C.c_size_t
            lib.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
            lib.libdeflate_free_compressor.argtypes = [C.c_void_p]
            _LIBDEFLATE = lib
        except (OSError, AttributeError):
            _LIBDEFLATE = False
    return _LIBDEFLATE or None


def libdeflate_stream(data: bytes, level: int) -> bytes:
    """raw deflate of data by libdeflate, accepted by zlib"""
    lib = libdeflate()
    comp = lib.libdeflate_alloc_compressor(level)
    assert comp
    out = C.create_string_buffer(len(data) + len(data) // 8 + 512)
    n = lib.libdeflate_deflate_compress(comp, data, len(data), out, len(out))
    lib.libdeflate_free_compressor(comp)
    assert n > 0
    raw = out.raw[:n]
    zlib_accepts(raw, data)
    return raw
