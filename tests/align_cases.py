"""Crafted reads for the alignment core -- TEST INFRASTRUCTURE (no GPU).

A small database and named groups of reads that sit on the geometric edges of the extension kernels: block origins
outside the allele, short last blocks, mismatch counts above eight bits, each inequality of the gap trigger, the vote
bins and the postings limit of the seeding policy.  Everything is deterministic (one seeded generator per purpose).

A case is ONE read with a name and a *predicted path*: what DESIGN section 2 says must happen to it, written down from
its construction (number of work items, votes, records, and for named (allele, strand, diagonal) pairs mm_total, used_dp,
score).  tests/test_align_cases.py asks the oracle to confirm every prediction; tests/test_gpu_align_cases.py submits the
groups to the engine.  A prediction key that is absent is not predicted (the overhanging bases of a read are random, say);
a key that is present must hold."""
from __future__ import annotations

import atexit
import functools
import math
import os
import shutil
import sqlite3
import tempfile
from dataclasses import dataclass, field

import numpy as np

from metamlst_amd import synth
from metamlst_amd.index import load_index

K, STEP = 20, 16                      # MLST_SEED_LEN, MLST_SEED_STEP
SPA, SPB = "spA", "spB"
LOCI_A = [("plain", 530), ("ragged", 520), ("n1", 260), ("n2", 260), ("n63", 300), ("n64", 300), ("n65", 300), ("n129", 300),
          ("n257", 320), ("amb", 400), ("dupA", 400), ("dupB", 400), ("rep16", 640), ("rep17", 640), ("s1", 260), ("s1b", 260),
          ("n127", 300), ("n128", 300), ("n256", 320)]
LOCI_B = [("other", 450)]
N_ALLELES = {"plain": 20, "ragged": 16, "n1": 1, "n2": 2, "n63": 63, "n64": 64, "n65": 65, "n129": 129, "n257": 257, "amb": 12,
             "dupA": 6, "dupB": 6, "rep16": 2, "rep17": 2, "other": 10, "s1": 1, "s1b": 3, "n127": 127, "n128": 128, "n256": 256}
RAGGED_LEN = {1: 33, 2: 63, 3: 64, 4: 65, 5: 95, 6: 96, 7: 97, 8: 129, 9: 519, 10: 500, 11: 481}      # allele number -> columns kept
REP_GAP = 24                           # distance of the planted 20-mers of the rep loci
REP_PLANTS = {"rep16": (("X16", 16), ("Z7", 7)), "rep17": (("Y17", 17), ("Z8", 8))}
LANES = (0, 31, 32, 63)
GROUPS = ("overhang_start", "overhang_end", "block_phase", "short_alleles", "lengths", "score_limits", "mm_over_255", "gap_trigger",
          "q1_records", "votes", "allele_counts")
# Groups of reads that equal an allele of their locus but for scattered single mismatches or N: the other alleles differ by
# scattered SNPs, and DESIGN section 2 step 4 says that scattered mismatches never start the banded Smith-Waterman.
NO_DP_GROUPS = ("overhang_start", "overhang_end", "block_phase", "lengths", "score_limits", "allele_counts")


def rc(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))


def other_base(c: int, k: int = 1) -> int:
    """A base that differs from c (k = 1..3 picks which)."""
    return b"ACGT"[(b"ACGT".index(bytes([c]).upper()) + k) % 4] if bytes([c]).upper() in (b"A", b"C", b"G", b"T") else b"ACGT"[k]


def floor_score(n: int) -> int:
    return int(20.0 + 8.0 * math.log(n))


@dataclass
class Case:
    name: str
    group: str
    bases: bytes
    quals: bytes
    expect: dict = field(default_factory=dict)      # items, votes, records, q1, dp_pairs, pairs=[{allele,strand,diag,...}]


@dataclass
class Corpus:
    db: synth.SynthDB
    idx: object
    cases: list
    plants: dict                                    # name -> (20-mer, locus gene, [positions])

    def groups(self) -> list[str]:
        out = []
        for c in self.cases:
            if c.group not in out:
                out.append(c.group)
        return out

    def of(self, group: str) -> list:
        return [c for c in self.cases if c.group == group]

    def allele(self, gene: str, no: int, species: str = SPA) -> int:
        l = self.idx.locus_index(species, gene)
        b, n = int(self.idx.locus_begin[l]), int(self.idx.locus_count[l])
        for a in range(b, b + n):
            if int(self.idx.allele_no[a]) == no:
                return a
        raise KeyError((gene, no))

    def seq(self, a: int) -> bytes:
        return self.idx.sequence(a).encode()

    def layout(self, cases, lanes: bool | None = None):
        """(bases, quals, off, case_of_read): the reads of `cases` as one submission.  lanes: crafted reads at lanes 0, 31,
        32 and 63 of groups of 64 with off-locus reads between (default: for groups of up to 160 cases)."""
        if lanes is None:
            lanes = len(cases) <= 160
        reads, quals, owner = [], [], []
        if not lanes:
            for k, c in enumerate(cases):
                reads.append(c.bases); quals.append(c.quals); owner.append(k)
        else:
            rng = np.random.default_rng(77)
            k = 0
            while k < len(cases):
                for lane in range(64):
                    if lane in LANES and k < len(cases):
                        reads.append(cases[k].bases); quals.append(cases[k].quals); owner.append(k); k += 1
                    else:
                        reads.append(bytes(rng.choice(list(b"ACGT"), size=150).astype(np.uint8))); quals.append(b"I" * 150); owner.append(-1)
        fb, fq, off = synth.ragged_reads(reads, quals)
        return fb, fq, off, owner


def _rewrite(db_path: str, rng) -> dict:
    """Alleles of different lengths, ambiguity codes, planted 20-mers: rewrite rows of the database make_db wrote."""
    conn = sqlite3.connect(db_path)
    rows = {(g, int(v)): (rid, s) for rid, g, v, s in conn.execute("SELECT recID, gene, alleleVariant, sequence FROM alleles WHERE bacterium=?", (SPA,))}
    upd = {}
    for no, keep in RAGGED_LEN.items():
        upd[("ragged", no)] = rows[("ragged", no)][1][:keep]
    for no in range(1, N_ALLELES["amb"] + 1):                  # allele 1 stays plain; the others get two or three codes each
        s = list(rows[("amb", no)][1])
        if no > 1:
            for p, ch in zip((17 * no + 40, 23 * no + 5, 391 - 9 * no), "NRW"):
                s[p] = ch
        upd[("amb", no)] = "".join(s)
    plants = {}
    for gene, spec in REP_PLANTS.items():
        L = dict(LOCI_A)[gene]
        bg = bytearray(rng.choice(list(b"ACGT"), size=L).astype(np.uint8))
        at = 12
        for name, count in spec:
            mer = bytes(rng.choice(list(b"ACGT"), size=K).astype(np.uint8))
            pos = []
            for _ in range(count):
                bg[at:at + K] = mer
                pos.append(at)
                at += REP_GAP
            plants[name] = (mer, gene, pos)
        assert at <= L - 10
        second = bytearray(bg)
        second[L - 5] = other_base(second[L - 5])
        upd[(gene, 1)], upd[(gene, 2)] = bytes(bg).decode(), bytes(second).decode()
    for key, s in upd.items():
        conn.execute("UPDATE alleles SET sequence=?, alignedSequence=? WHERE recID=?", (s, s, rows[key][0]))
    conn.commit()
    conn.close()
    return plants


def seed_votes(n: int, strand: int, clean) -> int:
    """Seeds of a read of n bases that lie wholly on clean[i] columns (i in the orientation of the allele)."""
    v = 0
    for o in range(0, n - K + 1, STEP):
        lo = n - K - o if strand else o
        v += all(clean[lo:lo + K])
    return v


class _Builder:
    def __init__(self, cp: Corpus):
        self.cp, self.cases, self.rng = cp, cp.cases, np.random.default_rng(20240)

    def rand(self, n: int) -> bytes:
        return bytes(self.rng.choice(list(b"ACGT"), size=n).astype(np.uint8))

    def add(self, group, name, fwd: bytes, strand=0, quals: bytes | None = None, **expect):
        """fwd / quals are given in the orientation of the allele; a strand-1 case submits the reverse complement."""
        quals = quals if quals is not None else b"I" * len(fwd)
        assert len(quals) == len(fwd) and not any(c.name == name for c in self.cases), name
        b, q = (rc(fwd), quals[::-1]) if strand else (fwd, quals)
        for p in expect.get("pairs", ()):
            p.setdefault("strand", strand)
        if group in NO_DP_GROUPS:
            expect.setdefault("dp_pairs", 0)
        self.cases.append(Case(name, group, b, q, expect))

    # ---- groups ----------------------------------------------------------------------------------------------------
    def overhang(self):
        cp = self.cp
        a = cp.allele("plain", 3); s = cp.seq(a); nloc = N_ALLELES["plain"]
        for n in (150, 300):
            for end in ("start", "end"):
                for strand in (0, 1):
                    for d in range(0, n + 1):               # every d until the read has no seed inside (that d included)
                        over = self.rand(d)
                        if end == "start":
                            fwd, diag, clean = over + s[:n - d], -d, [i >= d for i in range(n)]
                        else:
                            fwd, diag, clean = s[len(s) - (n - d):] + over, len(s) - (n - d), [i < n - d for i in range(n)]
                        votes = seed_votes(n, strand, clean)
                        exp = dict(items=1 if votes else 0, pairs=[])
                        if votes:
                            sc = 2 * (n - d)
                            exp.update(votes=votes)
                            exp["pairs"] = [dict(allele=a, diag=diag, mm_total=0, used_dp=0, score=sc, record=sc >= floor_score(n))]
                            if sc >= floor_score(n) + 60:
                                exp["records"] = nloc
                        else:
                            exp.update(records=0)
                        self.add("overhang_" + end, "overhang_%s/L%d/s%d/d%d" % (end, n, strand, d), fwd, strand, **exp)
                        if not votes:
                            break

    def block_phase(self):
        cp = self.cp
        a = cp.allele("plain", 5); s = cp.seq(a); n = 150
        for ph in range(32):
            for strand in (0, 1) if ph in (0, 1, 31) else (ph & 1,):
                at = 64 + ph
                self.add("block_phase", "block_phase/perfect/ph%d/s%d" % (ph, strand), s[at:at + n], strand, items=1, votes=9, records=20,
                         pairs=[dict(allele=a, diag=at, mm_total=0, used_dp=0, score=300)])
                r = bytearray(s[at:at + n]); r[70] = other_base(r[70])
                self.add("block_phase", "block_phase/one_mm/ph%d/s%d" % (ph, strand), bytes(r), strand, items=1, records=20,
                         pairs=[dict(allele=a, diag=at, mm_total=1, used_dp=0, score=292)])
        for at in (64, 69, 95, 101):                        # a mismatch on the first and the last column of every covered block
            for col in sorted({c for b in range(at // 32, (at + n - 1) // 32 + 1) for c in (32 * b, 32 * b + 31) if at <= c < at + n}):
                r = bytearray(s[at:at + n]); r[col - at] = other_base(r[col - at], 2)
                self.add("block_phase", "block_phase/edge_mm/d%d/col%d" % (at, col), bytes(r), (col >> 5) & 1, items=1, records=20,
                         pairs=[dict(allele=a, diag=at, mm_total=1, used_dp=0)])

    def short_alleles(self):
        cp = self.cp
        full = cp.allele("ragged", 14); s = cp.seq(full)
        shorts = {no: cp.allele("ragged", no) for no in RAGGED_LEN}
        for n in (150, 300):
            for at in (0, 1, 20, 31, 32, 33, 40, 60, 64, 65, 90, 97, 120, 129, 200, len(s) - n - 40, len(s) - n - 19, len(s) - n - 1, len(s) - n):
                for strand in (0, 1):
                    pairs = [dict(allele=full, diag=at, mm_total=0, used_dp=0, score=2 * n)]
                    for no, al in shorts.items():          # the overlap with a short allele ends at its last column
                        ov = max(0, min(RAGGED_LEN[no], at + n) - at)
                        if ov == 0:
                            pairs.append(dict(allele=al, diag=at, mm_total=0, used_dp=0, score=0, record=False))
                    self.add("short_alleles", "short_alleles/L%d/at%d/s%d" % (n, at, strand), s[at:at + n], strand, items=1, pairs=pairs)
        for no, al in shorts.items():                       # a read of the short allele itself that hangs over its end
            sa = cp.seq(al); keep = min(len(sa), 90)
            for strand in (0, 1):
                fwd = sa[len(sa) - keep:] + self.rand(150 - keep)
                clean = [i < keep for i in range(150)]
                v = seed_votes(150, strand, clean)
                self.add("short_alleles", "short_alleles/own_end/a%d/s%d" % (no, strand), fwd, strand, items=1 if v else 0,
                         pairs=[dict(allele=al, diag=len(sa) - keep, mm_total=0, used_dp=0, score=2 * keep)] if v else [])

    def lengths(self):
        cp = self.cp
        a = cp.allele("plain", 7); s = cp.seq(a)
        for n in list(range(19, 61)) + list(range(155, 166)) + list(range(315, 321)):
            at = 100 + n % 32
            strand = n & 1
            nv = len(range(0, n - K + 1, STEP))
            self.add("lengths", "lengths/perfect/L%d" % n, s[at:at + n], strand, items=1 if nv else 0, votes=nv,
                     pairs=[dict(allele=a, diag=at, mm_total=0, used_dp=0, score=2 * n, record=2 * n >= floor_score(n))] if nv else [])
        for n in (36, 52, 148, 164, 308):                   # L = 4 (mod 16): the last seed ends on the last base
            offs = list(range(0, n - K + 1, STEP))
            assert offs[-1] + K == n
            for which, keep in (("last", offs[-1]), ("first", offs[0]), ("middle", offs[len(offs) // 2])):
                for strand in (0, 1):
                    r = bytearray(s[90:90 + n])
                    for o in offs:
                        if o != keep:
                            lo = (n - K - o if strand else o) + 8          # column 8 of a seed belongs to that seed alone
                            r[lo] = other_base(r[lo])
                    self.add("lengths", "lengths/one_seed_%s/L%d/s%d" % (which, n, strand), bytes(r), strand, items=1, votes=1,
                             pairs=[dict(allele=a, diag=90, mm_total=len(offs) - 1)])

    def score_limits(self):
        cp = self.cp
        a = cp.allele("plain", 9); s = cp.seq(a)
        for strand in (0, 1):
            self.add("score_limits", "score_limits/perfect320/s%d" % strand, s[100:420], strand, items=1, records=20,
                     pairs=[dict(allele=a, diag=100, mm_total=0, used_dp=0, score=640)])
            w = 140 if strand else 144                      # the one clean seed: read offset 160 on strand 1, 144 on strand 0
            for every in (2, 3):
                r = bytearray(s[100:420]); k = 0
                for i in range(1, 319):
                    if not (w <= i < w + K) and i % every == every - 1:
                        r[i] = ord("N"); k += 1
                self.add("score_limits", "score_limits/N_every_%d/s%d" % (every, strand), bytes(r), strand, items=1, votes=1,
                         pairs=[dict(allele=a, diag=100, mm_total=k, used_dp=0, score=2 * (320 - k) - k, xm=k)])
        for ph, pen in ((0, 2), (2, 2), (19, 3), (20, 4), (40, 6), (41, 6), (93, 6)):
            r = bytearray(s[100:250]); r[75] = other_base(r[75]); q = bytearray(b"I" * 150); q[75] = 33 + ph
            self.add("score_limits", "score_limits/phred%d" % ph, bytes(r), ph & 1, bytes(q), items=1, records=20,
                     pairs=[dict(allele=a, diag=100, mm_total=1, used_dp=0, score=298 - pen, xm=1)])
        for ph in (19, 20, 21):                             # minqual edge of the pile-up: whole reads at Phred 19, 20, 21
            self.add("score_limits", "score_limits/minqual%d" % ph, s[130:280], 0, bytes([33 + ph]) * 150, items=1, records=20,
                     pairs=[dict(allele=a, diag=130, mm_total=0, used_dp=0, score=300)])

        ab = cp.allele("amb", 4); sb = cp.seq(ab)            # ambiguity codes in the allele: N columns
        for at in (0, 60, 120, 250):
            fwd = bytes(c if c in b"ACGT" else ord("A") for c in sb[at:at + 150])
            nn = sum(c not in b"ACGT" for c in sb[at:at + 150])
            self.add("score_limits", "score_limits/ambiguity/at%d" % at, fwd, (at // 60) & 1, items=1, pairs=[dict(allele=ab, diag=at, mm_total=nn, used_dp=0)])

    def _core_read(self, s, at, n, core_lo, core_len, extra_matches=0):
        """n bases aligned to s[at:at+n] that mismatch on every column except a matching core and `extra_matches` isolated
        matching columns (each between mismatches, far from the core)."""
        r = bytearray(other_base(s[at + i], 1 + i % 3) for i in range(n))
        r[core_lo:core_lo + core_len] = s[at + core_lo:at + core_lo + core_len]
        spots = [i for i in range(2, n - 2, 3) if i < core_lo - 3 or i > core_lo + core_len + 3]
        assert extra_matches <= len(spots)
        for i in spots[:extra_matches]:
            r[i] = s[at + i]
        return bytes(r)

    def mm_over_255(self):
        cp = self.cp
        a = cp.allele("plain", 11); s = cp.seq(a); n, at, fl = 320, 100, floor_score(320)
        for mm, core in ((250, 48), (255, 48), (256, 48), (257, 48), (272, 48), (260, 60), (280, 40)):
            for strand in (0, 1):
                fwd = self._core_read(s, at, n, 128, core, n - core - mm)
                self.add("mm_over_255", "mm_over_255/mm%d/core%d/s%d" % (mm, core, strand), fwd, strand, items=1,
                         pairs=[dict(allele=a, diag=at, mm_total=mm, used_dp=1, ungapped_score=2 * core, record=True)])
        for core, name in ((fl // 2 - 1, "below_floor"), ((fl + 1) // 2, "at_floor")):
            rec = 2 * core >= fl
            self.add("mm_over_255", "mm_over_255/%s" % name, self._core_read(s, at, n, 128, core), 0, items=1,
                     pairs=[dict(allele=a, diag=at, mm_total=n - core, used_dp=int(rec), ungapped_score=2 * core, record=rec)])

    def gap_trigger(self):
        cp = self.cp
        a = cp.allele("plain", 13); s = cp.seq(a); n, at = 150, 120

        def cluster(lead: str, interior: int, end: str):
            """lead: 'X' mismatch / '=' match per column from the read's end inwards; interior: isolated Phred-40 mismatches."""
            r = bytearray(s[at:at + n])
            for i, ch in enumerate(lead):
                p = i if end == "left" else n - 1 - i
                if ch == "X":
                    r[p] = other_base(r[p])
            for k in range(interior):
                p = 30 + 11 * k
                r[p] = other_base(r[p], 2)
            return bytes(r)
        for end in ("left", "right"):
            strand = int(end == "right")
            for c, k, fire in ((8, 4, 0), (8, 5, 1), (7, 6, 0), (7, 5, 0), (9, 4, 1)):          # mm = c + k against 12; clipped = c against 8
                self.add("gap_trigger", "gap_trigger/cluster_%s/clip%d/mm%d" % (end, c, c + k), cluster("X" * c, k, end), strand, items=1,
                         records=20, pairs=[dict(allele=a, diag=at, mm_total=c + k, used_dp=fire, ungapped_score=2 * (n - c - k) - 6 * k)])
            for lead, c in (("X=X=X=X=X", 9), ("X=X=X=X=X=", 10), ("X=X=X=X=X==", 11)):          # 2 * (mm - xm) = 10 against clipped 9, 10, 11
                fire = int(10 >= c)
                self.add("gap_trigger", "gap_trigger/half_%s/clip%d" % (end, c), cluster(lead[::-1], 8, end), strand, items=1, records=20,
                         pairs=[dict(allele=a, diag=at, mm_total=13, used_dp=fire, ungapped_score=2 * (n - c - 8) - 48)])
        fl = floor_score(n)                                  # the score floor: a 31-base core with one cheap mismatch inside
        for ph, pen in ((15, 3), (2, 2)):
            r = bytearray(self._core_read(s, at, n, 32, 32)); r[52] = other_base(s[at + 52]); q = bytearray(b"I" * n); q[52] = 33 + ph
            sc = 62 - pen
            assert (sc == fl - 1) if pen == 3 else (sc == fl)
            self.add("gap_trigger", "gap_trigger/floor/score%d" % sc, bytes(r), 0, bytes(q), items=1,
                     pairs=[dict(allele=a, diag=at, mm_total=n - 31, used_dp=int(sc >= fl), ungapped_score=sc, record=sc >= fl)])
        for dl in (1, 2, 3, 7, 8, 9):                        # real indels in the middle of the read: votes tie, the smaller diagonal wins
            for strand in (0, 1):
                fwd = s[at:at + 75] + s[at + 75 + dl:at + n + dl]
                self.add("gap_trigger", "gap_trigger/deletion%d/s%d" % (dl, strand), fwd, strand, items=1, votes=4,
                         pairs=[dict(allele=a, diag=at, used_dp=1, record=True)] + ([dict(allele=a, diag=at, score=300 - 5 - 3 * dl, xo=1, xm=0)] if dl <= 8 else []))
                fwd = s[at:at + 75] + self.rand(dl) + s[at + 75:at + n - dl]
                behind = seed_votes(n, strand, [i >= 75 + dl for i in range(n)])      # a long insertion breaks one more seed behind it
                self.add("gap_trigger", "gap_trigger/insertion%d/s%d" % (dl, strand), fwd, strand, items=1, votes=4,
                         pairs=[dict(allele=a, diag=at - dl if behind == 4 else at, record=True)])
        for pos in (3, 4, 5):                                # gbar: indels 3, 4, 5 bases from either end
            for dl in (1, 2, 3):
                for end in ("left", "right"):
                    p = pos if end == "left" else n - pos
                    fwd = s[at:at + p] + s[at + p + dl:at + n + dl]
                    self.add("gap_trigger", "gap_trigger/gbar_%s/pos%d/del%d" % (end, pos, dl), fwd, dl & 1, items=1, records=20,
                             pairs=[dict(allele=a, diag=at + dl if end == "left" else at, used_dp=0)])
        for tail in (6, 7, 8, 9, 10):                        # a real indel 6..10 columns from the end: the clipped span around 8
            for dl in (1, 2, 3):
                fwd = s[at:at + n - tail] + s[at + n - tail + dl:at + n + dl]
                self.add("gap_trigger", "gap_trigger/tail%d/del%d" % (tail, dl), fwd, tail & 1, items=1, records=20,
                         pairs=[dict(allele=a, diag=at)])
        a1 = cp.allele("n1", 1); s1 = cp.seq(a1)             # the same clusters on the one-allele locus: DP_PAIRS of the read is that pair's
        for c, k, fire in ((8, 4, 0), (8, 5, 1), (7, 6, 0), (9, 4, 1)):
            r = bytearray(s1[50:50 + n])
            for i in list(range(c)) + [30 + 11 * j for j in range(k)]:
                r[i] = other_base(r[i])
            self.add("gap_trigger", "gap_trigger/one_allele/clip%d/mm%d" % (c, c + k), bytes(r), k & 1, items=1, records=1, dp_pairs=fire,
                     pairs=[dict(allele=a1, diag=50, mm_total=c + k, used_dp=fire, ungapped_score=2 * (n - c - k) - 6 * k)])
        ab = cp.allele("amb", 4); sb = cp.seq(ab)            # the span walk over N columns of the allele (codes at columns 97 and 108)
        for c, k in ((7, 6), (8, 5)):
            r = bytearray(ch if ch in b"ACGT" else ord("A") for ch in sb[60:60 + n])
            assert sum(ch not in b"ACGT" for ch in sb[60:60 + n]) == 2
            for i in list(range(c)) + [30 + 11 * j for j in range(k)]:
                assert sb[60 + i] in b"ACGT"
                r[i] = other_base(r[i])
            self.add("gap_trigger", "gap_trigger/amb_walk/clip%d" % c, bytes(r), c & 1, items=1,
                     pairs=[dict(allele=ab, diag=60, mm_total=c + k + 2, used_dp=int(c >= 8), ungapped_score=2 * (n - c - k - 2) - 6 * k - 2)])

    def q1_records(self):
        cp = self.cp
        a1 = cp.allele("n1", 1); s1 = cp.seq(a1)
        a2 = cp.allele("n2", 1); s2 = cp.seq(a2)
        ap = cp.allele("plain", 2); sp = cp.seq(ap)

        def with_mm(s, at, n, k):
            r = bytearray(s[at:at + n])
            for j in range(k):
                r[12 + 21 * j] = other_base(r[12 + 21 * j])
            return bytes(r)
        for k in (0, 5, 6):
            for strand in (0, 1):
                self.add("q1_records", "q1_records/one_record/xm%d/s%d" % (k, strand), with_mm(s1, 40, 150, k), strand, items=1, records=1, q1=True, dp_pairs=0,
                         pairs=[dict(allele=a1, diag=40, mm_total=k, used_dp=0, score=300 - 8 * k, xm=k)])
                self.add("q1_records", "q1_records/two_records/xm%d/s%d" % (k, strand), with_mm(s2, 40, 150, k), strand, items=1, records=2, q1=False, dp_pairs=0,
                         pairs=[dict(allele=a2, diag=40, mm_total=k, used_dp=0, score=300 - 8 * k, xm=k)])
        for dl in (1, 2):                                    # one record with a gap: field 15 is XO = 1 under the quirk, XM = 0 without
            fwd = s1[40:115] + s1[115 + dl:190 + dl]
            self.add("q1_records", "q1_records/one_record/gap%d" % dl, fwd, 0, items=1, records=1, q1=True, dp_pairs=1,
                     pairs=[dict(allele=a1, diag=40, used_dp=1, score=300 - 5 - 3 * dl, xo=1, xm=0)])
        self.add("q1_records", "q1_records/no_record", self._core_read(s1, 40, 150, 32, 29), 0, items=1, records=0, dp_pairs=0,
                 pairs=[dict(allele=a1, diag=40, ungapped_score=58, record=False)])
        # two items, one of them with exactly one record
        fwd = s1[40:120] + sp[200:270]
        self.add("q1_records", "q1_records/two_items/one_plus_twenty", fwd, 0, items=2, records=21, q1=False,
                 pairs=[dict(allele=a1, diag=40, record=True), dict(allele=ap, diag=120, record=True)])
        tail = bytearray(self._core_read(sp, 200, 70, 16, 22))
        fwd = s1[40:120] + bytes(tail)                       # the second item (one seed) stays below the floor: the read has ONE record
        self.add("q1_records", "q1_records/two_items/one_plus_none", fwd, 0, items=2, records=1, q1=True,
                 pairs=[dict(allele=a1, diag=40, record=True), dict(allele=ap, diag=120, record=False)])
        # The same two shapes with NO tracked pair, so that the fast pass itself meets an item of exactly one record in a read of
        # several items.  1 + 0: 128 bases of the one-allele locus, then one 20-mer of the plain locus (a single seed, 40 points: below
        # the floor) chosen to mismatch the one-allele locus on at most 12 of its 20 columns, so that mm_total stays at the trigger.
        n_at, mer_at, ham = next((x, y, h) for x in range(0, 100) for y in range(0, len(sp) - K)
                                 for h in [sum(u != v for u, v in zip(s1[x + 128:x + 148], sp[y:y + K]))] if h <= 12)
        fwd = s1[n_at:n_at + 128] + sp[mer_at:mer_at + K]
        self.add("q1_records", "q1_records/two_items/untracked_one_plus_none", fwd, 0, items=2, records=1, q1=True, dp_pairs=0,
                 pairs=[dict(allele=a1, diag=n_at, mm_total=ham, used_dp=0, record=True), dict(allele=ap, diag=mer_at - 128, used_dp=0, record=False)])
        # 1 + 3: a one-allele locus and its near-duplicate of three alleles share their seeds
        as1 = cp.allele("s1", 1); ss1 = cp.seq(as1)
        for strand in (0, 1):
            self.add("q1_records", "q1_records/two_items/untracked_one_plus_three/s%d" % strand, ss1[40:190], strand, items=2, records=4, q1=False,
                     dp_pairs=0, pairs=[dict(allele=as1, diag=40, mm_total=0, used_dp=0, score=300)])
        fwd = sp[100:175] + rc(sp[300:375])                  # both strands of one locus
        self.add("q1_records", "q1_records/both_strands", fwd, 0, items=2, records=40, q1=False,
                 pairs=[dict(allele=ap, diag=100, strand=0, record=True), dict(allele=ap, diag=300, strand=1, record=True)])
        ad = cp.allele("dupA", 1); sd = cp.seq(ad)           # near-duplicate loci: one read, several work items
        for strand in (0, 1):
            self.add("q1_records", "q1_records/dup_loci/s%d" % strand, sd[100:250], strand, items=2, records=12, q1=False,
                     pairs=[dict(allele=ad, diag=100, mm_total=0, used_dp=0, score=300)])

    def votes(self):
        cp = self.cp
        ap = cp.allele("plain", 4); sp = cp.seq(ap)
        pl = cp.plants
        for name, count, items in (("Z7", 7, 2), ("Z8", 8, 1)):              # 7 + 1 = 8 bins: the plain locus is kept; 8 + 1 = 9: dropped
            mer, gene, pos = pl[name]
            self.add("votes", "votes/%d_bins" % (count + 1), mer + sp[220:350], 0, items=items)
        mer, gene, pos = pl["X16"]
        a16 = cp.allele(gene, 1)
        self.add("votes", "votes/postings16", mer + self.rand(130), 0, items=1, votes=1,
                 pairs=[dict(allele=a16, diag=pos[0])])              # 16 postings: kept; 8 bins of one vote each, the smallest diagonal wins
        mer, gene, pos = pl["Y17"]
        self.add("votes", "votes/postings17", mer + self.rand(130), 0, items=0, records=0)
        self.add("votes", "votes/postings17_second_seed", self.rand(16) + mer + self.rand(114), 0, items=0, records=0)
        for dl, name in ((5, "tie_first_seen_wins"), (-3, "tie_second_seen_wins")):      # two seeds on each of two diagonals
            fwd = sp[200:240] + sp[240 + dl:284 + dl]
            self.add("votes", "votes/%s" % name, fwd, 0, items=1, votes=2, pairs=[dict(allele=ap, diag=200 + min(0, dl))])
            self.add("votes", "votes/%s/rev" % name, fwd, 1, items=1, votes=2, pairs=[dict(allele=ap, diag=200 + min(0, dl))])
        fwd = sp[200:240] + sp[245:305]                      # 2 votes against 3: the majority, although the larger diagonal
        self.add("votes", "votes/majority", fwd, 0, items=1, votes=3, pairs=[dict(allele=ap, diag=205)])

    def allele_counts(self):
        cp = self.cp
        for gene in ("n1", "n2", "n63", "n64", "n65", "n127", "n128", "n129", "n256", "n257"):
            cnt = N_ALLELES[gene]
            for no in sorted({1, cnt}):
                a = cp.allele(gene, no); s = cp.seq(a)
                for strand in (0, 1):
                    self.add("allele_counts", "allele_counts/%s/a%d/s%d" % (gene, no, strand), s[37:187], strand, items=1, records=cnt,
                             pairs=[dict(allele=a, diag=37, mm_total=0, used_dp=0, score=300)])
        a = cp.allele("other", 3, SPB); s = cp.seq(a)
        self.add("allele_counts", "allele_counts/second_species", s[10:160], 1, items=1, records=N_ALLELES["other"],
                 pairs=[dict(allele=a, diag=10, mm_total=0, used_dp=0, score=300)])


_TMP = tempfile.mkdtemp(prefix="mlst_align_cases_")
atexit.register(shutil.rmtree, _TMP, True)


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    path = os.path.join(_TMP, "cases.db")
    for p in (path, path + ".mlstidx"):
        if os.path.exists(p):
            os.remove(p)
    counts = {(SPA, g): N_ALLELES[g] for g, _ in LOCI_A}
    counts.update({(SPB, g): N_ALLELES[g] for g, _ in LOCI_B})
    db = synth.make_db(path, {SPA: list(LOCI_A), SPB: list(LOCI_B)}, counts, n_profiles=4, seed=811, max_div=0.04,
                       roots={(SPA, "dupB"): (SPA, "dupA"), (SPA, "s1b"): (SPA, "s1")})
    plants = _rewrite(path, np.random.default_rng(812))
    cp = Corpus(db, load_index(path, cache=False), [], plants)
    b = _Builder(cp)
    for g in (b.overhang, b.block_phase, b.short_alleles, b.lengths, b.score_limits, b.mm_over_255, b.gap_trigger, b.q1_records, b.votes,
              b.allele_counts):
        g()
    return cp


WIDE_B0, WIDE_B1 = 129, 128                       # block haplotypes of the two 32-column blocks: 16,512 alleles


@functools.lru_cache(maxsize=None)
def wide_locus():
    """(index, reads): ONE locus of 16,512 alleles of 64 columns, every combination of 129 variants of the first block and 128
    of the second -- more alleles than the 16,384 pending additions the haplotype kernel keeps per item -- and a few reads."""
    rng = np.random.default_rng(813)
    root = bytearray(rng.choice(list(b"ACGT"), size=64).astype(np.uint8))

    def variants(lo, count):
        out = [bytes(root[lo:lo + 32])]
        for i in range(32):
            for k in (1, 2, 3):
                v = bytearray(root[lo:lo + 32]); v[i] = other_base(v[i], k); out.append(bytes(v))
        for i in range(32):
            v = bytearray(root[lo:lo + 32]); v[i] = other_base(v[i]); v[(i + 7) % 32] = other_base(v[(i + 7) % 32], 2); out.append(bytes(v))
        assert len(set(out[:count])) == count
        return out[:count]
    b0, b1 = variants(0, WIDE_B0), variants(32, WIDE_B1)
    path = os.path.join(_TMP, "wide.db")
    if os.path.exists(path):
        os.remove(path)
    conn = sqlite3.connect(path)
    synth.create_schema(conn)
    conn.execute("INSERT INTO organisms (organismkey,label) VALUES (?,?)", (SPA, "Synthetic " + SPA))
    conn.execute("INSERT INTO genes (geneName,bacterium) VALUES (?,?)", ("wide", SPA))
    seqs = [(x + y).decode() for x in b0 for y in b1]
    conn.executemany("INSERT INTO alleles (bacterium,gene,sequence,alignedSequence,alleleVariant) VALUES (?,?,?,?,?)",
                     [(SPA, "wide", q, q, k + 1) for k, q in enumerate(seqs)])
    conn.commit()
    conn.close()
    idx = load_index(path, cluster=False, cache=False)
    reads = []
    for no in (0, 5 * WIDE_B1 + 77, len(seqs) - 1):      # a read of the first, of a middle and of the last allele, both strands
        q = seqs[no].encode()
        reads += [q[2:62], rc(q), q[:31] + bytes([other_base(q[31])]) + q[32:]]
    return idx, reads
