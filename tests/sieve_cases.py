"""One planted seed per read, for every words-per-read instantiation of the sieves -- TEST INFRASTRUCTURE (no GPU).

A 150-base on-locus read carries nine seeds and any one of them makes it a sieve candidate, so a kernel that loses one slot
changes no statistic.  The reads here carry exactly ONE database seed, at a chosen slot, and the submissions are built so
that the longest read picks every row width W = 2, 4, .. 20 (lengths 16 (W - 2) + 1 .. 16 W).  Everything is seeded.

The database: three species x a few loci x 60 alleles (small enough for the LDS bitmaps), the rep16 / rep17 loci of
tests/align_cases.py (a 20-mer with 16 postings: kept; one with 17: repetitive, dropped) and one extra allele of locus g0 that
holds a 20-mer equal to its own reverse complement (the tie of the strand comparison in k_route, canon40, sieve_half_flip).

A submission (`submission(W, kind)`) holds 3,400 reads:
  planted     for every length, every slot t < nseeds and both strands: a background without any seed of K (checked with the
              model at every slot), one key of K written at offset 16 t, forward or reverse-complemented
  shift1/15   the same key at offsets 16 t + 1 and 16 t + 15: not required
  n_inside    the key at the slot with one N inside its window (on a base that is no A): not required, not even allowed for
  n_inside_a  the N on an A of the key: the packed row holds the key itself -- allowed for, not required
  post17      the 17-posting 20-mer at the slot: not required
  n_outside   the key at the slot, N everywhere else: required
  on_locus    64 error-free reads of random alleles per main length, both strands: records for pass 1 under every width
  background  reads without any seed of K
shuffled by a fixed permutation; chosen planted reads then take lanes 0 / 31 / 32 / 63 of the first and the last 64-read group
of a 1,024-read tile (and of a 512- and a 256-read tile), reads 1,023 and 1,024, and the partly empty last tile.
kind "mixed": every length of the width and 19 .. 37 below them where they fit (the masked path of k_sieve_q); "full": every
read has nseeds >= NT = W - 1 (the all_full path); "paired": the mixed reads of W = 8 submitted as mates (reads 2k, 2k + 1)."""
from __future__ import annotations

import atexit
import functools
import os
import shutil
import sqlite3
import tempfile
from dataclasses import dataclass

import numpy as np

import sieve_model as sm
from metamlst_amd import synth
from metamlst_amd.index import load_index

WIDTHS = tuple(range(2, 21, 2))
N_READS = 3400                                 # three tiles of 1,024 and 328 reads of a fourth
SMALL = (19, 20, 21, 35, 36, 37)
REP_GAP = 24
PINS = (0, 31, 32, 63, 192, 255, 256, 448, 511, 512, 960, 991, 992, 1023, 1024, 1055, 3072, N_READS - 1)
_TMP = tempfile.mkdtemp(prefix="mlst_sieve_cases_")
atexit.register(shutil.rmtree, _TMP, True)


def wpr_of(max_len: int) -> int:
    """The row width a submission whose longest read has max_len bases must get: 16 bases per word, at least 2, even."""
    w = max(2, (max_len + 15) // 16)
    return w + (w & 1)


def main_lengths(W: int) -> list[int]:
    return sorted({16 * (W - 2) + 1, 16 * W - 13, 16 * W - 12, 16 * W})


def lengths(W: int, kind: str) -> list[int]:
    if kind == "full":                         # nseeds >= NT for every read: n >= 16 (W - 2) + 20
        return [16 * W - 12, 16 * W - 5, 16 * W]
    return sorted(set(main_lengths(W)) | {n for n in SMALL if n <= 16 * W})


@dataclass
class Database:
    path: str
    idx: object
    model: sm.Model
    keys: list                                 # K sorted: what the planted reads draw from
    palindrome: bytes
    x16: bytes
    y17: bytes


@functools.lru_cache(maxsize=None)
def database() -> Database:
    path = os.path.join(_TMP, "sieve.db")
    for p in (path, path + ".mlstidx"):
        if os.path.exists(p):
            os.remove(p)
    rng = np.random.default_rng(9102)
    loci = {"spA": [("g%d" % k, 420 + 17 * k) for k in range(6)] + [("rep16", 640), ("rep17", 640)],
            "spB": [("h%d" % k, 450 + 11 * k) for k in range(4)], "spC": [("k%d" % k, 500 + 7 * k) for k in range(3)]}
    counts = {(sp, g): 60 for sp, ls in loci.items() for g, _ in ls}
    counts[("spA", "rep16")] = counts[("spA", "rep17")] = 2
    synth.make_db(path, loci, counts, n_profiles=4, seed=9101)
    conn = sqlite3.connect(path)
    rows = {(g, int(v)): (rid, s) for rid, g, v, s in conn.execute("SELECT recID, gene, alleleVariant, sequence FROM alleles WHERE bacterium='spA'")}
    mers = {}
    for gene, count in (("rep16", 16), ("rep17", 17)):      # one 20-mer `count` times, 24 columns apart (tests/align_cases.py)
        bg = bytearray(rng.choice(list(b"ACGT"), size=640).astype(np.uint8))
        mers[gene] = bytes(rng.choice(list(b"ACGT"), size=sm.K_LEN).astype(np.uint8))
        for k in range(count):
            bg[12 + REP_GAP * k:12 + REP_GAP * k + sm.K_LEN] = mers[gene]
        second = bytearray(bg)
        second[635] = ord("A") if second[635] != ord("A") else ord("C")
        for no, s in ((1, bg), (2, second)):
            conn.execute("UPDATE alleles SET sequence=?, alignedSequence=? WHERE recID=?", (bytes(s).decode(), bytes(s).decode(), rows[(gene, no)][0]))
    half = bytes(rng.choice(list(b"ACGT"), size=sm.K_LEN // 2).astype(np.uint8))
    pal = half + sm.revcomp(half)
    assert pal == sm.revcomp(pal)
    s = bytearray(rows[("g0", 1)][1].encode())
    s[100:100 + sm.K_LEN] = pal
    conn.execute("INSERT INTO alleles (bacterium,gene,sequence,alignedSequence,alleleVariant) VALUES ('spA','g0',?,?,61)", (bytes(s).decode(),) * 2)
    conn.commit()
    conn.close()
    idx = load_index(path, cache=False)
    model = sm.Model(idx)
    post = sm.postings(idx)
    assert len(post[mers["rep16"]]) == 16 and mers["rep16"] in model.K              # sixteen postings: kept
    assert len(post[mers["rep17"]]) == 17 and mers["rep17"] not in model.K          # seventeen: repetitive
    assert len(post[pal]) == 2 and pal in model.K                                   # the palindrome: both strands of one position
    return Database(path, idx, model, sorted(model.K), pal, mers["rep16"], mers["rep17"])


@dataclass
class Read:
    bases: bytes
    what: str                                   # planted, shift1, shift15, n_inside, n_inside_a, post17, n_outside, on_locus, background
    slot: int = -1
    strand: int = 0
    key: str = ""                               # "", "palindrome" or "postings16": the named keys


@dataclass
class Submission:
    W: int
    kind: str
    reads: list                                 # of Read, in submission order
    fb: np.ndarray
    fq: np.ndarray
    off: np.ndarray
    paired: bool
    must: np.ndarray                            # bool per read: has to be a candidate (mates included when paired)
    may: np.ndarray                             # bool per read: may be a candidate without being a false positive
    foreign: int                                # S: (read, slot) seeds that are not in K

    def where(self, i: int) -> tuple:
        i = int(i)
        r = self.reads[i]
        return (self.W, len(r.bases), r.slot, r.strand, i & 63, i >> 6, i >> 10)      # (W, length, slot, strand, lane, group, tile)

    def text(self) -> bytes:
        return b"".join(b"@s%d\n%s\n+\n%s\n" % (i, r.bases, b"I" * len(r.bases)) for i, r in enumerate(self.reads))


class _Maker:
    def __init__(self, W: int, kind: str):
        self.db, self.W, self.kind = database(), W, kind
        self.rng = np.random.default_rng(9200 + 10 * W + (kind == "full"))
        self.m = self.db.model

    def rand(self, n: int) -> bytes:
        return bytes(self.rng.choice(list(b"ACGT"), size=n).astype(np.uint8))

    def background(self, n: int) -> bytes:
        while True:
            b = self.rand(n)
            if not self.m.may(b):
                return b

    def key(self, strand: int, named: bytes | None = None) -> bytes:
        k = named if named is not None else self.db.keys[int(self.rng.integers(len(self.db.keys)))]
        return sm.revcomp(k) if strand else k

    def put(self, n: int, at: int, mer: bytes, want_hits: list, want_may: list | None = None):
        """A background of n bases with `mer` at offset `at` whose slots in K are exactly want_hits (and want_may in the packed
        view): drawn again until the model says so (a neighbouring slot shares four bases with the key); None when no background does."""
        for _ in range(40):
            b = bytearray(self.background(n))
            b[at:at + len(mer)] = mer
            b = bytes(b)
            if self.m.hits(b) == want_hits and self.m.hits(b, packed_view=True) == (want_hits if want_may is None else want_may):
                return b
        return None

    def group(self, n: int, ns: int, t: int, strand: int, named: str, thin: bool):
        """The planted read of (length, slot, strand) and its controls around one key; None when a control cannot be built."""
        db = self.db
        k = self.key(strand, {"palindrome": db.palindrome, "postings16": db.x16}.get(named))
        out = [Read(self.put(n, 16 * t, k, [t]), "planted", t, strand, named)]
        if not thin:
            for sh in (1, 15):
                if 16 * t + sh + sm.K_LEN <= n:
                    out.append(Read(self.put(n, 16 * t + sh, k, []), "shift%d" % sh, t, strand))
            pos = [i for i in range(4, 16) if k[i] != ord("A")]      # (columns 4 .. 15 belong to this slot's window alone)
            i = pos[int(self.rng.integers(len(pos)))]
            out.append(Read(self.put(n, 16 * t, k[:i] + b"N" + k[i + 1:], []), "n_inside", t, strand))
            out.append(Read(self.put(n, 16 * t, self.key(strand, db.y17), []), "post17", t, strand))
            if t in (0, ns // 2, ns - 1) and (t + strand) % 2 == 0:
                pos = [i for i in range(4, 16) if k[i] == ord("A")]
                if pos:
                    out.append(Read(self.put(n, 16 * t, k[:pos[0]] + b"N" + k[pos[0] + 1:], [], [t]), "n_inside_a", t, strand))
                b = bytearray(b"N" * n)
                b[16 * t:16 * t + sm.K_LEN] = k
                if self.m.hits(bytes(b), packed_view=True) == [t]:      # (a key that ends in A would pair with the A the Ns are stored as)
                    out.append(Read(bytes(b), "n_outside", t, strand))
        if named:                                          # the named keys are what they are: a control they defeat is left out
            out = out[:1] + [r for r in out[1:] if r.bases is not None]      # (all four bases precede the 16 copies of postings16)
        return None if any(r.bases is None for r in out) else out

    def specials(self) -> list:
        out, db = [], self.db
        H, NT = self.W // 2, self.W - 1                    # H = (NT + 1) / 2: the first seed of k_route's second counting batch
        for n in lengths(self.W, self.kind):
            ns = len(sm.slots(n))
            for t in range(ns):
                for strand in (0, 1):
                    named = ""
                    if n == 16 * self.W and t == H and strand == 0 and H < ns:
                        named = "palindrome"
                    elif n == 16 * self.W and t == ns - 1 and strand == 1:
                        named = "postings16"
                    thin = self.kind == "full" and (t + strand) % 3 != 0      # (the controls of a full submission: every third)
                    for _ in range(100):                   # a key whose neighbourhood in the alleles defeats a control is drawn again
                        group = self.group(n, ns, t, strand, named, thin)
                        if group is not None:
                            break
                    assert group is not None, (self.W, n, t, strand, named)
                    out += group
        k = 0
        while sum(r.what == "planted" for r in out) < 3 * len(PINS):      # narrow rows have few slots: more keys at the same slots
            n = lengths(self.W, self.kind)[::-1][k % len(lengths(self.W, self.kind))]
            ns, k = len(sm.slots(n)), k + 1
            for t in range(ns):
                for strand in (0, 1):
                    out.append(Read(self.put(n, 16 * t, self.key(strand), [t]), "planted", t, strand))
            out = [r for r in out if r.bases is not None]
        assert any(r.what == "n_outside" for r in out)
        idx = db.idx
        for n in main_lengths(self.W) if self.kind != "full" else lengths(self.W, self.kind):
            for k in range(64):
                a = int(self.rng.integers(idx.n_alleles))
                s = idx.sequence(a).encode()
                at = int(self.rng.integers(0, len(s) - n + 1))
                out.append(Read(sm.revcomp(s[at:at + n]) if k & 1 else s[at:at + n], "on_locus", -1, k & 1))
        return out

    def make(self) -> list:
        sp = self.specials()
        assert len(sp) <= 0.7 * N_READS, (self.W, self.kind, len(sp))
        ls = lengths(self.W, self.kind)
        reads = sp + [Read(self.background(ls[int(self.rng.integers(len(ls)))]), "background") for _ in range(N_READS - len(sp))]
        reads = [reads[i] for i in self.rng.permutation(N_READS)]
        # chosen planted reads onto the pinned places: the longest reads' slots H, NT - 1, H - 1, 0 first, both strands
        H, NT = self.W // 2, self.W - 1
        order = {t: k for k, t in enumerate((H, NT - 1, H - 1, 0))}
        planted = sorted((i for i, r in enumerate(reads) if r.what == "planted" and i not in PINS),
                         key=lambda i: (-len(reads[i].bases), order.get(reads[i].slot, 9), reads[i].slot, reads[i].strand, i))
        for pin, i in zip(PINS, planted):
            reads[pin], reads[i] = reads[i], reads[pin]
        assert max(len(r.bases) for r in reads) == 16 * self.W and all(reads[p].what == "planted" for p in PINS)
        return reads


@functools.lru_cache(maxsize=None)
def submission(W: int, kind: str) -> Submission:
    db = database()
    paired = kind == "paired"
    assert not paired or W == 8
    reads = submission(W, "mixed").reads if paired else _Maker(W, kind).make()
    must = np.array([db.model.must(r.bases) for r in reads])
    may = np.array([db.model.may(r.bases) for r in reads])
    for r, mu, ma in zip(reads, must, may):            # the construction and the model agree on every read
        assert mu == (r.what in ("planted", "n_outside")) or r.what == "on_locus", (W, kind, r)
        assert ma == (mu or r.what == "n_inside_a") or r.what == "on_locus", (W, kind, r)
    if paired:                                          # mates (reads 2k, 2k + 1) are candidates together
        must = must | must.reshape(-1, 2)[:, ::-1].reshape(-1)
        may = may | may.reshape(-1, 2)[:, ::-1].reshape(-1)
    fb, fq, off = synth.ragged_reads([r.bases for r in reads], [b"I" * len(r.bases) for r in reads])
    assert wpr_of(int(np.diff(off.astype(np.int64)).max())) == W
    return Submission(W, kind, reads, fb, fq, off, paired, must, may, sum(db.model.foreign_seeds(r.bases) for r in reads))


def all_submissions() -> list:
    return [(W, kind) for W in WIDTHS for kind in ("mixed", "full")] + [(8, "paired")]
