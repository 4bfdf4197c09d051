"""Centre-star alignment of the alleles of one locus: the written rule behind `merge --outseqformat A --aligner gpu`.

metamlst-merge.py:402-405 pipes the sequences of a locus through MUSCLE [NOT IN TREE] when they differ in length.  The engine
aligns them itself (csrc/msa_dev.h, mlst_msa_align); this module is the statement of what it computes, in numpy, clear before fast:
the yardstick of the device path and its documentation, not a product path.  The policy is this engine's own (MLST_MSA_* of
include/mlst_policy.h); MUSCLE's bytes are not reproduced.

Centre.   The most frequent length; on a tie the greatest such length; among the sequences of that length the first in input order.
Pairs.    Every other sequence b (rows i = 1..n) is aligned to the centre a (columns j = 1..m): global, affine, unbanded, int32.
          s(x, y) = +5 when x & 0xDF == y & 0xDF and that letter is one of A C G T, -4 otherwise (N matches nothing).
          A gap of g bases costs 10 + g, end gaps included.  States M (b_i on a_j), I (b_i opposite a gap), D (a_j opposite a gap):
            M[0][0] = 0, I[i][0] = -(10 + i), D[0][j] = -(10 + j), everything else on the border NEG
            M[i][j] = s + max(M, I, D)[i-1][j-1]
            I[i][j] = max(M[i-1][j] - 11, I[i-1][j] - 1, D[i-1][j] - 11)
            D[i][j] = max(M[i][j-1] - 11, D[i][j-1] - 1, I[i][j-1] - 11)
          In every max the first listed candidate wins ties; the end state is the first of M, I, D that reaches the maximum at
          [n][m]; the traceback follows the recorded choices.
Merge.    Slot k (k = 0..m) lies between centre columns k and k + 1 and is as wide as the longest insertion any row makes there.
          A row is, for k = 0..m: its insertion in slot k, left-justified and padded with '-', then (k < m) its base on column k + 1
          or '-'.  Letters keep their case.  Insertions of different rows that share a slot are stacked, not aligned to each other.
"""
from __future__ import annotations

import numpy as np

MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 5, -4, 10, 1       # MLST_MSA_MATCH / _MISMATCH / _GAP_OPEN / _GAP_EXT (include/mlst_policy.h)
MAX_LEN = 4095                                          # MLST_MAX_ALLELE_LEN
NEG = -(1 << 28)
_M, _I, _D = 0, 1, 2


def check_input(seqs) -> list[bytes]:
    seqs = [bytes(s) for s in seqs]
    if not seqs:
        raise ValueError("no sequence to align")
    for r, s in enumerate(seqs):
        if not s:
            raise ValueError("sequence %d is empty" % r)
        if len(s) > MAX_LEN:
            raise ValueError("sequence %d is longer than %d bases" % (r, MAX_LEN))
        if not all(65 <= c <= 90 or 97 <= c <= 122 for c in s):
            raise ValueError("sequence %d holds a byte that is not an ASCII letter" % r)
    return seqs


def pick_center(seqs: list[bytes]) -> int:
    count: dict = {}
    for s in seqs:
        count[len(s)] = count.get(len(s), 0) + 1
    best = max(count.items(), key=lambda kv: (kv[1], kv[0]))[0]      # most frequent, then greatest
    return next(r for r, s in enumerate(seqs) if len(s) == best)


def _codes(s: bytes) -> np.ndarray:
    u = np.frombuffer(s, np.uint8) & 0xDF
    c = np.full(len(s), -1, np.int32)                     # -1: not A C G T, matches nothing
    for k, letter in enumerate(b"ACGT"):
        c[u == letter] = k
    return c


def _first_max(c0, c1, c2):
    """max of three candidates and the index of the FIRST that reaches it: the tie rule."""
    best = np.maximum(np.maximum(c0, c1), c2)
    return best, np.where(c0 == best, 0, np.where(c1 == best, 1, 2)).astype(np.uint8)


def align_pairs(a: bytes, bs: list[bytes]) -> list:
    """Every b of bs against the centre a.  Returns one (col, ins) per b: col[j - 1] = index into b of the base on centre column j,
    or -1; ins[k] = (start, length) of the run of b inserted in slot k (length 0: none).
    The cells of one anti-diagonal d = i + j do not depend on each other, so a diagonal is one numpy step, taken for all pairs at
    once (axis 0).  The three value arrays are indexed by the row i and hold the diagonals d - 1 and d - 2.  Shorter sequences are padded to the longest with a code that matches nothing: a cell
    depends on cells above and left of it only, so the rows past a sequence's end are computed and never read."""
    out = []
    m = len(a)
    n = max(map(len, bs))
    per = max(1, (1 << 28) // ((n + 1) * (n + m + 1)))      # pairs per sweep: bounds the choice table
    for at in range(0, len(bs), per):
        out += _sweep(a, bs[at:at + per])
    return out


def _sweep(a: bytes, bs: list[bytes]) -> list:
    m, n, R = len(a), max(map(len, bs)), len(bs)
    ca = _codes(a)
    cb = np.full((R, n), -2, np.int32)
    for r, b in enumerate(bs):
        cb[r, :len(b)] = np.where(_codes(b) < 0, -2, _codes(b))      # -2 on this side, -1 on the centre's: N never equals N
    open_ = GAP_OPEN + GAP_EXT
    # choice of M | choice of I << 2 | choice of D << 4 of cell (i, j) at [i + j][pair][i], each 0..2 = index in its max
    tb = np.zeros((n + m + 1, R, n + 1), np.uint8)
    new = lambda: [np.full((R, n + 1), NEG, np.int32) for _ in range(3)]
    p2, p1 = new(), new()                                 # diagonals d - 2 and d - 1: [M, I, D]
    p1[_M][:, 0] = 0                                      # d = 0: cell (0, 0)
    last = np.zeros((R, 3), np.int32)                     # M, I, D at [len(b)][m]
    for d in range(1, n + m + 1):
        cur = new()
        if d <= m:
            cur[_D][:, 0] = -(GAP_OPEN + GAP_EXT * d)     # cell (0, d)
        if d <= n:
            cur[_I][:, d] = -(GAP_OPEN + GAP_EXT * d)     # cell (d, 0)
        lo, hi = max(1, d - m), min(n, d - 1)             # interior rows of the diagonal
        if lo <= hi:
            # rows i = lo..hi meet columns j = d - i: b_i is cb[i - 1], a_j is ca[d - i - 1] 
            s = np.where(cb[:, lo - 1:hi] == ca[d - hi - 1:d - lo][::-1], np.int32(MATCH), np.int32(MISMATCH))
            M2, I2, D2 = (x[:, lo - 1:hi] for x in p2)    # cells (i - 1, j - 1)
            Mu, Iu, Du = (x[:, lo - 1:hi] for x in p1)    # cells (i - 1, j)
            Ml, Il, Dl = (x[:, lo:hi + 1] for x in p1)    # cells (i, j - 1)
            best, km = _first_max(M2, I2, D2)
            cur[_M][:, lo:hi + 1] = s + best
            cur[_I][:, lo:hi + 1], ki = _first_max(Mu - open_, Iu - GAP_EXT, Du - open_)
            cur[_D][:, lo:hi + 1], kd = _first_max(Ml - open_, Dl - GAP_EXT, Il - open_)
            tb[d][:, lo:hi + 1] = km | ki << 2 | kd << 4
        for r, b in enumerate(bs):
            if d == len(b) + m:
                last[r] = [cur[_M][r, len(b)], cur[_I][r, len(b)], cur[_D][r, len(b)]]
        p2, p1 = p1, cur
    return [_traceback(tb[:, r], len(b), m, int(last[r].argmax())) for r, b in enumerate(bs)]      # end state: first of M, I, D at the maximum


def _traceback(tb, n: int, m: int, state: int):
    from_m, from_i, from_d = (_M, _I, _D), (_M, _I, _D), (_M, _D, _I)      # candidate order of each max
    col = [-1] * m
    ins = [(0, 0)] * (m + 1)
    i, j = n, m
    while i > 0 or j > 0:
        if i == 0:
            state = _D
        elif j == 0:
            state = _I
        t = int(tb[i + j, i])
        if state == _M:
            col[j - 1] = i - 1
            state = from_m[t & 3]
            i, j = i - 1, j - 1
        elif state == _I:
            ins[j] = (i - 1, ins[j][1] + 1)               # the run is walked backwards: its start is the last base seen
            state = from_i[t >> 2 & 3]
            i -= 1
        else:
            state = from_d[t >> 4 & 3]
            j -= 1
    return col, ins


def center_star(seqs) -> tuple[int, list[bytes]]:
    seqs = check_input(seqs)
    if len(seqs) == 1:
        return 0, [seqs[0]]
    c = pick_center(seqs)
    a = seqs[c]
    m = len(a)
    distinct = sorted(set(seqs[:c] + seqs[c + 1:]))       # identical sequences align identically
    done = dict(zip(distinct, align_pairs(a, distinct)))
    pairs = [done.get(b) for b in seqs]
    pairs[c] = (list(range(m)), [(0, 0)] * (m + 1))       # the centre is itself, without a look at the scores
    width = [max(p[1][k][1] for p in pairs) for k in range(m + 1)]
    rows = []
    for b, (col, ins) in zip(seqs, pairs):
        out = bytearray()
        for k in range(m + 1):
            st, ln = ins[k]
            out += b[st:st + ln] + b"-" * (width[k] - ln)
            if k < m:
                out += b[col[k]:col[k] + 1] if col[k] >= 0 else b"-"
        rows.append(bytes(out))
    return c, rows
