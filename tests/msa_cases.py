"""Inputs shared by tests/test_msa_host.py and tests/test_gpu_msa.py: seeded sequences, the family of near-identical alleles, and a tiny
database (built with dbbuild) whose species has one locus with alleles of different lengths, plus a folder of .nfo lines for it."""
from __future__ import annotations

import os
import random

from metamlst_amd import db as mdb
from metamlst_amd import dbbuild
from metamlst_amd.merge import merge_folder


def rand_seq(n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def family(n_rows: int = 300, length: int = 450, seed: int = 20260) -> list[bytes]:
    """Rows from one ancestor with 0-8 SNPs and 0-3 indels of 1-12 bases each."""
    rng = random.Random(seed)
    anc = bytes(rng.choice(b"ACGT") for _ in range(length))
    rows = []
    for _ in range(n_rows):
        b = bytearray(anc)
        for _ in range(rng.randint(0, 8)):
            b[rng.randrange(len(b))] = rng.choice(b"ACGT")
        for _ in range(rng.randint(0, 3)):
            at, g = rng.randrange(len(b)), rng.randint(1, 12)
            if rng.random() < 0.5:
                del b[at:at + g]
            else:
                b[at:at] = bytes(rng.choice(b"ACGT") for _ in range(g))
        rows.append(bytes(b))
    return rows


SPECIES = "tinysp"
_G1 = rand_seq(60, 1).decode()
_G2 = rand_seq(72, 2).decode()
_G3 = rand_seq(66, 3).decode()


def _snp(s: str, at: int) -> str:
    return s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]


# gene -> allele number -> sequence; g2 is the locus with length variants (a 3-base deletion, a 5-base insertion)
ALLELES = {
    "g1": {1: _G1, 2: _snp(_G1, 10), 3: _snp(_G1, 40)},
    "g2": {1: _G2, 2: _snp(_G2, 20), 3: _G2[:30] + _G2[33:], 4: _G2[:50] + "GATTC" + _G2[50:]},
    "g3": {1: _G3, 2: _snp(_G3, 5)},
}
PROFILES = {1: (1, 1, 1), 2: (2, 2, 1), 3: (1, 3, 2), 4: (3, 4, 1)}
NEW_G2 = _G2[:66]                     # a sample's new allele: six bases short at the end, another length again (and, for the command's
                                      # matcher, within z of allele 1 by the truncating stringDiff)


def tiny_database(folder: str) -> str:
    """The database file and, next to it, `nfo/` with three samples: ST 3 (the deletion allele), ST 4 (the insertion allele) and
    one with NEW_G2."""
    os.makedirs(folder, exist_ok=True)
    fa, ty, path = os.path.join(folder, "alleles.fa"), os.path.join(folder, "typings.txt"), os.path.join(folder, "tiny.db")
    with open(fa, "w") as f:
        for gene, alleles in ALLELES.items():
            for no, seq in alleles.items():
                f.write(">%s_%s_%d\n%s\n" % (SPECIES, gene, no, seq))
    with open(ty, "w") as f:
        f.write("#%s|Tiny species\nST\tg1\tg2\tg3\n" % SPECIES)
        for st, row in PROFILES.items():
            f.write("%d\t%s\n" % (st, "\t".join(map(str, row))))
    if os.path.exists(path):
        os.remove(path)
    conn = dbbuild.open_db(path)
    dbbuild.add_sequences(conn, [fa])
    dbbuild.add_typings(conn, [ty], logfile=None)
    conn.close()
    nfo = os.path.join(folder, "nfo")
    os.makedirs(nfo, exist_ok=True)

    def line(sample, g1, g2, g3, g2_seq=None):
        seqs = (ALLELES["g1"][g1], g2_seq or ALLELES["g2"][g2], ALLELES["g3"][g3])
        return SPECIES + "\t" + sample + "\t" + "\t".join("%s_%s_%d::%s::100.0::0.0" % (SPECIES, g, a, s)
                                                           for g, a, s in zip(("g1", "g2", "g3"), (g1, g2, g3), seqs)) + "\n"

    with open(os.path.join(nfo, "s1.nfo"), "w") as f:
        f.write(line("s1", 1, 3, 2))
    with open(os.path.join(nfo, "s2.nfo"), "w") as f:
        f.write(line("s2", 3, 4, 1))
    with open(os.path.join(nfo, "s3.nfo"), "w") as f:
        f.write(line("s3", 2, 2, 1, NEW_G2))
    return path


def merge_tiny(folder: str, aligner, outseqformat: str = "A"):
    """merge_folder over the tiny database's .nfo folder (every new allele accepted); returns (tables, records of _sequences.fna)."""
    path = tiny_database(folder)
    database = mdb.metaMLST_db(path)
    tables = merge_folder(os.path.join(folder, "nfo"), database, lambda *a: True, z=5, outseqformat=outseqformat, aligner=aligner)
    database.closeConnection()
    return tables[SPECIES], list(dbbuild.read_fasta(os.path.join(folder, "nfo", "merged", SPECIES + "_sequences.fna")))


def expected_concatenations(tables: dict) -> dict:
    """ST -> the concatenation of its profile's allele sequences, genes in sorted order (metamlst-merge.py:431, :469), straight
    from the tables and ALLELES, without write_sequences."""
    label = dict(("%s_%s_%d" % (SPECIES, g, no), s) for g, al in ALLELES.items() for no, s in al.items())
    for news in tables["newSequences"].values():
        label.update(news)
    out = {}
    for code, (hits, profile) in tables["oldProfiles"].items():
        out[code] = "".join(label["%s_%s_%s" % (SPECIES, g, a)] for g, a in sorted(profile.items()))
    for code, (profile, hits, kind) in tables["encounteredProfiles"].items():
        out[code] = "".join(label["%s_%s_%s" % (SPECIES, g, a[0])] for g, a in sorted(profile.items()))
    return out
