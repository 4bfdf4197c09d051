"""A plain model of the sieve's contract -- TEST INFRASTRUCTURE (NumPy and plain Python, no GPU, no engine code).

DESIGN section 2 step 1 and the index builder ("group, drop repetitive seeds"), stated on strings:

  K        every 20-mer, in both orientations, of every allele window that holds only ACGT, kept when it has at most
           MLST_MAX_POSTINGS distinct (locus, strand, position) postings.  Both orientations are kept so that nothing here
           restates the engine's choice of a canonical form.
  slots    a read of n bases carries seeds at offsets 0, 16, ...: (n - 20) // 16 + 1 of them for n >= 20, none below.
  must     some slot's window has no N and lies in K: the read HAS to be a sieve candidate (k_seed will find a posting).
  may      the same with every non-ACGT base read as A: the packed row stores code 0 there and the sieve kernels do not
           look at the N bit (k_seed drops such seeds later).  A candidate outside `may` is a false positive of the 16-bit
           fingerprints, or a mate.

tests/test_sieve_model.py ties `must` to the oracle ("the read has a work item"); tests/test_gpu_sieve_words.py holds the
candidate lists of the three sieves against `must` and `may`."""
from __future__ import annotations

import numpy as np

K_LEN, STEP, MAX_POSTINGS = 20, 16, 16              # MLST_SEED_LEN, MLST_SEED_STEP, MLST_MAX_POSTINGS (include/mlst_policy.h)
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = frozenset(b"ACGT")


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(_RC)


def slots(n: int) -> list[int]:
    """The seed offsets of a read of n bases."""
    return [STEP * t for t in range((n - K_LEN) // STEP + 1)] if n >= K_LEN else []


def as_packed(read: bytes, nmask=None) -> bytes:
    """The read as the packed row holds it: every non-ACGT base (and every base flagged in nmask) is an A."""
    return bytes(c if c in _ACGT and not (nmask is not None and nmask[i]) else 65 for i, c in enumerate(read))


def postings(idx) -> dict:
    """{20-mer: set of (locus, strand, position)} over both orientations of every all-ACGT allele window."""
    post: dict = {}
    for a in range(idx.n_alleles):
        s = bytes(idx.ascii_concat[int(idx.off[a]):int(idx.off[a + 1])]).upper()
        l = int(idx.locus_id[a])
        for p in range(len(s) - K_LEN + 1):
            w = s[p:p + K_LEN]
            if not _ACGT.issuperset(w):
                continue
            post.setdefault(w, set()).add((l, 0, p))
            post.setdefault(revcomp(w), set()).add((l, 1, p))
    return post


def keys(idx) -> frozenset:
    """K: the 20-mers a read's seed is looked up against and found."""
    return frozenset(w for w, ps in postings(idx).items() if len(ps) <= MAX_POSTINGS)


def n_canonical(K) -> int:
    """Distinct keys when a 20-mer and its reverse complement count once (what an index of canonical keys holds)."""
    return len({min(w, revcomp(w)) for w in K})


class Model:
    def __init__(self, idx):
        self.K = keys(idx)

    def hits(self, read: bytes, nmask=None, packed_view: bool = False) -> list[int]:
        """The slot numbers whose window lies in K: windows with an N count for the packed view only (as the A they are stored as)."""
        read = read.upper()                                # (the packer takes either case)
        seen = as_packed(read, nmask)
        clean = [c in _ACGT and not (nmask is not None and nmask[i]) for i, c in enumerate(read)]
        return [t for t, o in enumerate(slots(len(read))) if seen[o:o + K_LEN] in self.K and (packed_view or all(clean[o:o + K_LEN]))]

    def must(self, read: bytes, nmask=None) -> bool:
        return bool(self.hits(read, nmask))

    def may(self, read: bytes, nmask=None) -> bool:
        return bool(self.hits(read, nmask, packed_view=True))

    def foreign_seeds(self, read: bytes) -> int:
        """Seeds of the read, as the sieve sees them, that are not in K: each one is a chance of a fingerprint false positive."""
        seen = as_packed(read.upper())
        return sum(seen[o:o + K_LEN] not in self.K for o in slots(len(read)))


def split(fb: np.ndarray, off: np.ndarray) -> list[bytes]:
    """The reads of a flat submission."""
    raw = bytes(np.ascontiguousarray(fb, np.uint8))
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
