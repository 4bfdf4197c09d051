"""Crafted inputs for the device typing tail -- TEST INFRASTRUCTURE (no GPU).

The kernels that turn statistics into the answer (k_choose, k_layout_compact, k_consensus, k_consensus_expand, k_hamming, k_export /
k_import) take everything through entries that need no reads: statistics are injected (mlst_import_stats_device), pile-up counts are
written into a buffer the caller owns.  This module builds ONE database whose loci sit on the edges of those kernels' thread layouts
(k_choose: block = locus, 256 threads, thread t takes alleles t, t + 256, ...; k_layout_compact: 1,024 loci per turn;
k_consensus_expand: 256 columns per turn of a slot; k_hamming: 256 alleles per block), the crafted statistics, counts and queries,
and the plain models the GPU module compares with.  A statistics case records where it put its winner and tie partners (`expect`);
tests/test_tail_cases.py checks those properties in the loaded index, tests/test_gpu_tail_cases.py runs the cases on the engine."""
from __future__ import annotations

import atexit
import functools
import os
import shutil
import sqlite3
import tempfile
from dataclasses import dataclass, field

import numpy as np

from metamlst_amd import synth
from metamlst_amd.index import load_index
from metamlst_amd.typing import NO_READ, SampleStats, compile_cel, consensus_from_counts, pick_alleles, pick_alleles_fast

SPA, SPZ = "spA", "spZ"                 # spZ holds the locus with a repeated alleleVariant, and sorts last
N_LOCI = 1030                           # k_layout_compact: one turn of 1,024 loci and one of 6
RAGGED_LEN = {1: 40, 2: 41, 3: 255, 4: 256, 5: 257, 6: 300, 7: 599, 8: 600}      # allele number -> columns kept
# locus position -> (tag, alleles, bases): the named loci.  Gene names carry the position, so that the sorted order of the index is
# this order; the tests read positions back from the loaded index.
NAMED = {0: ("n257", 257, 40), 100: ("n1", 1, 40), 200: ("n63", 63, 40), 300: ("n64", 64, 255), 400: ("n65", 65, 256),
         500: ("n255", 255, 257), 600: ("n256", 256, 40), 700: ("w600", 3, 600), 800: ("ragged", len(RAGGED_LEN), 600),
         1023: ("n513", 513, 40), 1024: ("n1025", 1025, 40)}
DUP_POS, DUP_ROWS, DUP_NO = 1029, 513, 256      # numbers 1..255 once, 256 twice, 257..512 once: the pair sits at rows 255 and 256
WIDE_FILLERS = range(900, 940)          # fillers of 257 bases: columns 255 and 256 of a slot, once per counts pattern
PENALTIES = (100, 3, 0)
MINCOVS = (0, 1, 2, 8000)
NONE_CHARS = ("N", "-")
M32 = (1 << 32) - 1
SENTINEL = np.iinfo(np.int64).max       # "no read" in the flat int64 form of export / import (0xFFFF... in the engine)
HAMMING_LIMIT = 60000                   # bytes of a query (the kernel keeps it in dynamic LDS)
MLST_E_LIMIT = -5


def gene_name(pos: int) -> str:
    return "g%04d_%s" % (pos, NAMED[pos][0] if pos in NAMED else "dup" if pos == DUP_POS else "wide" if pos in WIDE_FILLERS else "f")


def _plan():
    """species -> [(gene, bases)], {(species, gene): alleles} in position order."""
    loci, counts = {SPA: [], SPZ: []}, {}
    for pos in range(N_LOCI):
        sp = SPZ if pos == DUP_POS else SPA
        _, n, length = NAMED.get(pos, ("dup", DUP_ROWS, 40) if pos == DUP_POS else ("wide", 2, 257) if pos in WIDE_FILLERS else ("f", 2, 40))
        loci[sp].append((gene_name(pos), length))
        counts[(sp, gene_name(pos))] = n
    return loci, counts


def _rewrite(db_path: str) -> None:
    """Ragged allele lengths, and one alleleVariant twice in the spZ locus: rewrite rows of the database make_db wrote."""
    conn = sqlite3.connect(db_path)
    gene = gene_name(800)
    for rid, no, s in conn.execute("SELECT recID, alleleVariant, sequence FROM alleles WHERE bacterium=? AND gene=?", (SPA, gene)).fetchall():
        conn.execute("UPDATE alleles SET sequence=?, alignedSequence=? WHERE recID=?", (s[:RAGGED_LEN[int(no)]], s[:RAGGED_LEN[int(no)]], rid))
    conn.execute("UPDATE alleles SET alleleVariant = alleleVariant - 1 WHERE bacterium=? AND alleleVariant > ?", (SPZ, DUP_NO))
    conn.commit()
    conn.close()


@dataclass
class StatsCase:
    name: str
    sum_score: np.ndarray               # int64[n_alleles]
    n_hits: np.ndarray                  # int64[n_alleles], every value < 2^32
    locus_first: np.ndarray             # int64[n_loci], SENTINEL exactly where the locus has no allele with hits
    expect: dict = field(default_factory=dict)      # locus -> {winner, partners, mx, wave, turn, ...}: allele indices INSIDE the locus
    dup: bool = False                   # ties two rows of one alleleVariant: the literal restatement cannot tell them apart

    def stats(self) -> SampleStats:
        first = self.locus_first.astype(np.uint64)
        first[self.locus_first == SENTINEL] = NO_READ
        return SampleStats(self.sum_score.copy(), self.n_hits.astype(np.uint32), np.zeros(len(first), np.uint64), first, np.zeros(8, np.uint64))

    def flat(self, n_sum: int) -> np.ndarray:
        """The int64 vector mlst_import_stats_device takes beside locus_first: sums, hits, per-locus lengths, counters."""
        nA = len(self.sum_score)
        return np.concatenate([self.sum_score, self.n_hits, np.zeros(n_sum - 2 * nA, np.int64)])

    def chosen_loci(self) -> list:
        return np.nonzero(self.locus_first != SENTINEL)[0].tolist()


class _Stats:
    """Statistics of one case under construction, addressed by (locus, allele index inside the locus)."""

    def __init__(self, ix, name, dup=False):
        self.ix, self.name, self.dup = ix, name, dup
        self.ss, self.nh = np.zeros(ix.n_alleles, np.int64), np.zeros(ix.n_alleles, np.int64)
        self.expect = {}

    def span(self, l):
        return int(self.ix.locus_begin[l]), int(self.ix.locus_count[l])

    def background(self, l, keep=lambda j: True):
        """100 hits each, averages 200.0 .. 249.0 (no penalty applies between equal depths)."""
        b, n = self.span(l)
        for j in range(n):
            if keep(j):
                self.nh[b + j], self.ss[b + j] = 100, 100 * (200 + (7 * j + l) % 50)

    def put(self, l, k, nh, ss):
        b, n = self.span(l)
        assert 0 <= k < n and 0 <= nh <= M32
        self.nh[b + k], self.ss[b + k] = nh, ss

    def done(self) -> StatsCase:
        ix = self.ix
        hit = np.add.reduceat(self.nh, ix.locus_begin.astype(np.intp)) > 0
        first = np.where(hit, (np.arange(ix.n_loci, dtype=np.int64) * 7919) % 100003, SENTINEL)
        return StatsCase(self.name, self.ss, self.nh, first, self.expect, self.dup)


def numbers(ix, l) -> list:
    b, n = int(ix.locus_begin[l]), int(ix.locus_count[l])
    return [int(x) for x in ix.allele_no[b:b + n]]


def where(k: int) -> tuple:
    """(wave, turn) of k_choose's thread that takes allele index k of a locus."""
    return k % 256 // 64, k // 256


# ---- placements of a two-way tie: candidate (i, j), i < j, in a fixed order -------------------------------------------------------
def _same_thread(n):
    return ((i, i + 256) for i in range(n - 256))


def _same_wave(n):
    return ((i, j) for i in range(n) for j in range(min(n, (i // 64 + 1) * 64) - 1, i, -1))


def _wave0_vs_wave3(n):
    t = 256 if n >= 512 else 0                      # the second turn where the locus has a full one
    return ((i, j) for i in range(t, t + 64) for j in range(t + 192, min(n, t + 256)))


def _turn1_vs_turn5(n):
    return ((i, 1024) for i in range(256) if n > 1024)


PLACEMENTS = {"same_thread_two_turns": _same_thread, "two_lanes_of_one_wave": _same_wave, "wave0_vs_wave3": _wave0_vs_wave3,
              "turn1_vs_turn5": _turn1_vs_turn5}
WINNER_AT = (0, 63, 64, 127, 128, 191, 192, 255, 256, 511, 512, "last")
PRESENCE = ("none_missing", "all_missing", "missing_0", "missing_1023", "missing_1024", "missing_1029", "missing_even", "missing_odd",
            "missing_first_turn", "missing_second_turn")


def missing_loci(pattern: str, n_loci: int) -> set:
    kind = pattern[len("missing_"):] if pattern.startswith("missing_") else pattern
    if kind == "none_missing":
        return set()
    if kind == "all_missing":
        return set(range(n_loci))
    if kind.isdigit():
        return {int(kind)}
    return {"even": set(range(0, n_loci, 2)), "odd": set(range(1, n_loci, 2)), "first_turn": set(range(min(1024, n_loci))),
            "second_turn": set(range(1024, n_loci))}[kind]


def duplicate_pair(ix, l) -> tuple:
    """(k1, k2), k1 < k2: the two rows of locus l that carry the same alleleVariant."""
    no = numbers(ix, l)
    k = [j for j, x in enumerate(no) if no.count(x) > 1]
    assert len(k) == 2, k
    return k[0], k[1]


def has_duplicates(ix, l) -> bool:
    no = numbers(ix, l)
    return len(set(no)) != len(no)


def dup_case(ix, l) -> StatsCase:
    """The two rows of one number tie at the top of locus l; every other locus has an ordinary winner."""
    s = _Stats(ix, "duplicate_number_tie", dup=True)
    for m in range(ix.n_loci):
        s.background(m)
    k1, k2 = duplicate_pair(ix, l)
    s.put(l, k1, 100, 30000); s.put(l, k2, 100, 30000)
    s.expect[l] = dict(winner=k1, partners=(k1, k2))
    return s.done()


def stats_cases(ix, dup_locus=None) -> list:
    """Every statistics case for the index, generated from it: a case says "winner at allele index k of locus L"."""
    nL = ix.n_loci
    sizes = [int(x) for x in ix.locus_count]
    plain = {l for l in range(nL) if not has_duplicates(ix, l)}
    out = []

    for at in WINNER_AT:                                          # a unique winner at a fixed index, in every locus that has it
        s = _Stats(ix, "winner_at_%s" % at)
        for l in range(nL):
            s.background(l)
            k = sizes[l] - 1 if at == "last" else at
            if k < sizes[l]:
                s.put(l, k, 100, 30000)
                s.expect[l] = dict(winner=k)
        out.append(s.done())

    for place, gen in PLACEMENTS.items():                         # two-way ties on the ROUNDED average (300.10 and 300.14)
        for order in ("lower_number_first", "lower_number_second"):
            s = _Stats(ix, "tie/%s/%s" % (place, order))
            for l in range(nL):
                s.background(l)
                if l not in plain:
                    continue
                no = numbers(ix, l)
                pair = next(((i, j) for i, j in gen(sizes[l]) if (no[i] < no[j]) == (order == "lower_number_first")), None)
                if pair:
                    i, j = pair
                    s.put(l, i, 100, 30010 if (l + i) & 1 else 30014); s.put(l, j, 100, 30014 if (l + i) & 1 else 30010)
                    s.expect[l] = dict(winner=i if no[i] < no[j] else j, partners=pair, place=place, order=order)
            assert s.expect, s.name
            out.append(s.done())

    for lowest in (0, 1, 2):                                      # three-way tie across three waves, the lowest number in each of them
        s = _Stats(ix, "tie/three_waves/lowest_in_%d" % lowest)
        for l in range(nL):
            s.background(l)
            n = sizes[l]
            if l not in plain or n < 129:
                continue
            no = numbers(ix, l)
            third = 192 if n > 192 else 128
            tri = next(((i, j, m) for i in range(0, 8) for j in range(64, 72) for m in range(third, min(n, third + 8))
                        if min((no[i], 0), (no[j], 1), (no[m], 2))[1] == lowest), None)
            if tri:
                for k, sc in zip(tri, (30011, 30012, 30013)):
                    s.put(l, k, 100, sc)
                s.expect[l] = dict(winner=tri[lowest], partners=tri)
        assert s.expect, s.name
        out.append(s.done())

    # The allele with the most hits (mx) far from thread 0 and NOT the winner.  W (wave 0) has 990 hits at 250; C (wave 1) has 500 at
    # 300 and loses to W only because it pays (mx - 500) * 100; the alleles of 3 hits go negative under the penalty (round_tenths'
    # floor division).  With penalty 3 or 0 the model's winner is C.
    for name in ("mx_in_wave3", "mx_in_last_turn"):
        s = _Stats(ix, name)
        for l in range(nL):
            n = sizes[l]
            if l not in plain or n < 256 or (name == "mx_in_last_turn" and n < 257):
                s.background(l)
                continue
            mx = 200 + l % 50 if name == "mx_in_wave3" else n - 1
            for j in range(0, n, 3):
                s.put(l, j, 3, 600)
            s.put(l, 5, 990, 990 * 250); s.put(l, 70, 500, 500 * 300); s.put(l, mx, 1000, 1000 * 100)
            s.expect[l] = dict(winner_at_100=5, mx=mx)
        out.append(s.done())

    s = _Stats(ix, "hits_only_from_256_on")
    for l in range(nL):
        n = sizes[l]
        if n < 257:
            s.background(l)
            continue
        s.background(l, keep=lambda j: j >= 256)
        k = 256 + (n - 257) // 2
        s.put(l, k, 100, 30000)
        s.expect[l] = dict(winner=k)
    out.append(s.done())

    s = _Stats(ix, "single_hit_allele")
    for l in range(nL):
        k = (37 * l) % sizes[l]
        s.put(l, k, 7, 7 * 123 + 3)
        s.expect[l] = dict(winner=k)
    out.append(s.done())

    for par in (0, 1):                                            # hit alleles alternate with n_hits = 0 (whose sums must be ignored)
        s = _Stats(ix, "alternating/%s" % ("even", "odd")[par])
        for l in range(nL):
            b, n = s.span(l)
            s.background(l, keep=lambda j: j % 2 == par)
            for j in range(1 - par, n, 2):
                s.ss[b + j] = 10 ** 9 + j
            if n > par:
                k = ((n - 1 - par) // 2) * 2 + par                # the last index of that parity
                s.put(l, k, 100, 30000)
                s.expect[l] = dict(winner=k)
        out.append(s.done())

    # n_hits = 2^32 - 1 and sums up to +-2^44 (the range tests/test_round_tenths.py covers), spread over the locus
    for sign in (1, -1):
        s = _Stats(ix, "extremes/%s" % ("positive" if sign > 0 else "negative"))
        for l in range(nL):
            n = sizes[l]
            at = sorted({0, n // 3, 2 * n // 3, n - 1})
            vals = ([(M32, 1 << 44), (M32, (1 << 44) - 1), (M32, -(1 << 44)), (1, 1 << 43)] if sign > 0 else
                    [(M32, -(1 << 44)), (M32, -(1 << 44) + 1), (M32 - 1, -(1 << 44)), (1, -(1 << 43))])
            for k, (nh, ss) in zip(at, vals):
                s.put(l, k, nh, ss)
        out.append(s.done())

    for pattern in PRESENCE:                                      # loci without any record
        s = _Stats(ix, "presence/%s" % pattern)
        gone = missing_loci(pattern, nL)
        for l in range(nL):
            if l in gone:
                continue
            s.background(l)
            k = (13 * l) % sizes[l]
            s.put(l, k, 100, 30000)
            s.expect[l] = dict(winner=k)
        s.expect["missing"] = gone
        out.append(s.done())

    if dup_locus is not None:
        out.append(dup_case(ix, dup_locus))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- models: the reference's own lines ---------------------------------------------------------------------------------------------
def choice_literal(ix, case: StatsCase, penalty: int) -> dict:
    """{locus: label} by compile_cel + pick_alleles (metamlst.py:133-151, 244)."""
    cel = compile_cel(ix, case.stats(), penalty)
    return {ix.locus_index(sp, g): sp + "_" + g + "_" + k for sp, genes in cel.items() for g, k in pick_alleles(genes, sp)}


def choice_fast(ix, case: StatsCase, penalty: int) -> dict:
    """{locus: allele index} by pick_alleles_fast."""
    return pick_alleles_fast(ix, case.stats(), penalty)


def string_diff(s1: bytes, s2: bytes) -> int:
    """stringDiff, metaMLST_functions.py:230-234."""
    return sum(a != b for a, b in zip(s1, s2))


def hamming_model(ix, l: int, query: bytes) -> np.ndarray:
    b, n = int(ix.locus_begin[l]), int(ix.locus_count[l])
    return np.array([string_diff(ix.sequence(a).encode(), query) for a in range(b, b + n)], np.uint32)


def fixed_colbase(ix) -> np.ndarray:
    """Column bases of the fixed layout (mlst_typing_layout): one slot of the locus' longest allele per locus, in locus order."""
    return np.concatenate(([0], np.cumsum(ix.locus_maxlen))).astype(np.uint64)


def compact_layout(colbase, chosen_loci) -> tuple:
    """({locus: column base}, columns needed): the loci with a chosen allele in locus order, each with its fixed slot width."""
    base, at = {}, 0
    for l in sorted(chosen_loci):
        base[l] = at
        at += int(colbase[l + 1]) - int(colbase[l])
    return base, at


def compact_counts(counts_fixed: np.ndarray, colbase, chosen_loci) -> np.ndarray:
    """The slots of the chosen loci, taken from a fixed-layout counts array and laid out by compact_layout."""
    base, need = compact_layout(colbase, chosen_loci)
    out = np.zeros((need, 4), np.uint32)
    for l, at in base.items():
        lo, hi = int(colbase[l]), int(colbase[l + 1])
        out[at:at + hi - lo] = counts_fixed[lo:hi]
    return out


# ---- counts ------------------------------------------------------------------------------------------------------------------------
# The kernels add the four counts of a column in 32 bits: a column whose counts sum to 2^32 or more is out of range (a depth no
# sample reaches: the pile-up adds one per aligned base) and is not tested.
def count_patterns() -> list:
    one = [tuple(int(i == b) for i in range(4)) for b in range(4)]
    pats = [("zero", (0, 0, 0, 0))] + [("single_" + "ACGT"[b], one[b]) for b in range(4)]
    for k in (2, 3, 4):                                          # every tie of k bases (the first of ACGT wins); a smaller count elsewhere
        for mask in range(16):
            if bin(mask).count("1") == k:
                pats.append(("tie_" + "".join("ACGT"[b] for b in range(4) if mask >> b & 1), tuple(5 if mask >> b & 1 else 4 for b in range(4))))
    for mc in (2, 8000):                                         # totals of exactly mincov - 1 and mincov (mincov 1: "zero", "single_*")
        q = mc // 4
        pats.append(("total_%d" % (mc - 1), (q, mc - 1 - 3 * q, q, q) if mc > 2 else (0, 0, 1, 0)))
        pats.append(("total_%d" % mc, (q - 1, q, mc - 3 * q + 1, q) if mc > 2 else (0, 1, 0, 1)))
    pats += [("max_" + "ACGT"[b], tuple(M32 if i == b else 0 for i in range(4))) for b in range(4)]
    pats += [("sum_max_G", (1 << 30, (1 << 30) - 1, 1 << 31, 0)), ("sum_max_T", (1 << 29, (1 << 29) - 1, 1 << 30, 1 << 31))]
    assert all(sum(p) <= M32 for _, p in pats) and len({n for n, _ in pats}) == len(pats)
    return pats


def pattern_of_column(l: int, c: int, n_patterns: int) -> int:
    """Which pattern column c of locus l's slot holds: shifted by the locus, so that neighbouring slots differ at equal columns."""
    return (c + l) % n_patterns


def crafted_counts(colbase) -> np.ndarray:
    """uint32[total_cols][4]: every slot of the fixed layout filled with the patterns."""
    pats = np.array([p for _, p in count_patterns()], np.uint32)
    out = np.zeros((int(colbase[-1]), 4), np.uint32)
    for l in range(len(colbase) - 1):
        lo, hi = int(colbase[l]), int(colbase[l + 1])
        out[lo:hi] = pats[(np.arange(hi - lo) + l) % len(pats)]
    return out


def letters_model(counts_fixed: np.ndarray, colbase, chosen_loci, mincov: int, none_char: str) -> np.ndarray:
    """The whole fixed-layout letter array: typing.consensus_from_counts per slot; a locus without a chosen allele has zero counts."""
    chosen = set(chosen_loci)
    out = np.zeros(int(colbase[-1]), np.uint8)
    for l in range(len(colbase) - 1):
        lo, hi = int(colbase[l]), int(colbase[l + 1])
        slot = counts_fixed[lo:hi] if l in chosen else np.zeros((hi - lo, 4), np.uint32)
        out[lo:hi] = np.frombuffer("".join(consensus_from_counts(slot, mincov, none_char)).encode(), np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _letters_all_or_none(mincov: int, none_char: str) -> tuple:
    ix = corpus().idx
    cb = fixed_colbase(ix)
    return (letters_model(counts_fixed(), cb, range(ix.n_loci), mincov, none_char), letters_model(counts_fixed(), cb, (), mincov, none_char))


def letters_of_corpus(chosen_loci, mincov: int, none_char: str) -> np.ndarray:
    """letters_model over the corpus' crafted counts, from its two extremes (every slot's model depends on that slot alone)."""
    ix = corpus().idx
    full, zero = _letters_all_or_none(mincov, none_char)
    mask = np.zeros(ix.n_loci, bool)
    mask[list(chosen_loci)] = True
    return np.where(np.repeat(mask, ix.locus_maxlen), full, zero)


# ---- Hamming queries ---------------------------------------------------------------------------------------------------------------
def _other(c: int) -> int:
    return b"CGTA"[b"ACGT".index(bytes([c]))]


@functools.lru_cache(maxsize=None)
def _query_tail() -> bytes:
    return bytes(np.random.default_rng(4000).choice(list(b"ACGT"), size=HAMMING_LIMIT).astype(np.uint8))


def hamming_queries(ix, l: int) -> list:
    """[(name, query)] for locus l: lengths around the shortest and the longest allele, edits of an allele, case."""
    b, n = int(ix.locus_begin[l]), int(ix.locus_count[l])
    seqs = [ix.sequence(a).encode() for a in range(b, b + n)]
    short, long_ = min(seqs, key=len), max(seqs, key=len)
    grow = long_ + _query_tail()
    out = [("len_%s" % name, grow[:k]) for name, k in (("0", 0), ("1", 1), ("shortest-1", len(short) - 1), ("shortest", len(short)),
                                                        ("shortest+1", len(short) + 1), ("longest+1", len(long_) + 1), ("limit", HAMMING_LIMIT))]
    for name, a in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        s = seqs[a]
        one = bytearray(s); one[len(s) // 2] = _other(one[len(s) // 2])
        two = bytearray(s); two[0] = _other(two[0]); two[-1] = _other(two[-1])
        out += [("%s/exact" % name, s), ("%s/one_changed" % name, bytes(one)), ("%s/two_changed" % name, bytes(two)),
                ("%s/all_changed" % name, bytes(_other(c) for c in s)), ("%s/lower_case" % name, s.lower())]
    return out


def hamming_loci(ix) -> list:
    """Every named locus, the locus of the repeated number, and a filler at each end and of each width: the loci whose queries
    also go through mlst_hamming_le (mlst_hamming_all sees the queries of every locus)."""
    return sorted(set(NAMED) | {DUP_POS, 1, WIDE_FILLERS[0], 1022, 1025})


def hamming_le_model(dist: np.ndarray, begin: int, z: int) -> tuple:
    """(first allele index in index order with distance <= z or -1, how many)."""
    hit = np.nonzero(dist <= z)[0]
    return (begin + int(hit[0]) if hit.size else -1), int(hit.size)


# ---- export / import ---------------------------------------------------------------------------------------------------------------
def export_vectors(n_alleles: int, n_loci: int, n_sum: int) -> list:
    """[(name, flat int64[n_sum], first int64[n_loci])]: sums, hits, per-locus lengths, counters; first reads."""
    rng = np.random.default_rng(4100)
    out = []
    firsts = np.array([0, 1, 1 << 40, 1 << 62, SENTINEL], np.int64)
    for name in ("negative_sums", "max_hits", "mixed"):
        ss = rng.integers(-(1 << 44), 1 << 44, size=n_alleles) if name != "negative_sums" else -rng.integers(1, 1 << 44, size=n_alleles)
        nh = np.full(n_alleles, M32, np.int64) if name == "max_hits" else rng.integers(0, 1 << 32, size=n_alleles)
        ln = rng.integers(0, 1 << 50, size=n_loci)
        ctr = rng.integers(1, 1 << 40, size=n_sum - 2 * n_alleles - n_loci)
        first = firsts[(np.arange(n_loci) + len(out)) % len(firsts)]
        out.append((name, np.concatenate([ss, nh, ln, ctr]).astype(np.int64), first.copy()))
    return out


# ---- the corpus --------------------------------------------------------------------------------------------------------------------
@dataclass
class Corpus:
    db: synth.SynthDB
    idx: object                          # every locus, alleles of a locus in similarity order (the order the engine is given)
    idx_dup: object                      # species spZ alone, alleles in (number, row) order: the repeated number at rows 255 and 256
    cases: list

    def position(self, tag: str) -> int:
        pos = next(p for p, v in NAMED.items() if v[0] == tag) if tag != "dup" else DUP_POS
        sp = SPZ if tag == "dup" else SPA
        return self.idx.locus_index(sp, gene_name(pos))

    def case(self, name: str) -> StatsCase:
        return next(c for c in self.cases if c.name == name)


_TMP = tempfile.mkdtemp(prefix="mlst_tail_cases_")
atexit.register(shutil.rmtree, _TMP, True)


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    path = os.path.join(_TMP, "tail.db")
    for p in (path, path + ".mlstidx"):
        if os.path.exists(p):
            os.remove(p)
    loci, counts = _plan()
    db = synth.make_db(path, loci, counts, n_profiles=1, seed=911, max_div=0.25)
    _rewrite(path)
    idx = load_index(path, cache=False)
    idx_dup = load_index(path, species_filter=[SPZ], cluster=False, cache=False)
    return Corpus(db, idx, idx_dup, stats_cases(idx, dup_locus=idx.locus_index(SPZ, gene_name(DUP_POS))))


@functools.lru_cache(maxsize=None)
def counts_fixed() -> np.ndarray:
    a = crafted_counts(fixed_colbase(corpus().idx))
    a.setflags(write=False)
    return a
