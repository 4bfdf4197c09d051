"""mlst_msa_align / mlst_msa_fetch (csrc/msa_dev.h) against the written rule, metamlst_amd.msa.center_star: centre, width and every byte
of every row, at the lane and stripe edges of the wavefront, at indels on the first and last column and across a stripe boundary, for
stacked insertions, N and lower case, a family of 300 near-identical rows (in one batch and in three), the refusals, and the
`merge --outseqformat A --aligner gpu` command on a tiny database."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import msa_cases as mc
from metamlst_amd import engine as eng_mod
from metamlst_amd.engine import Engine, MlstError
from metamlst_amd.msa import center_star

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWAP = bytes.maketrans(b"ACGT", b"CATG")          # a base that matches nothing it stood for


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def family_rows():
    seqs = mc.family()
    return seqs, center_star(seqs)


def same(e, seqs):
    want = center_star(seqs)
    got = e.align_center_star(seqs)
    assert got[0] == want[0], "centre"
    assert len(got[1][0]) == len(want[1][0]), "width"
    assert got[1] == want[1]
    return want


def around(length, seed):
    """A centre of `length` bases (twice, so it is the centre), a row with a base cut, one with a base filled in, one with a SNP."""
    a = mc.rand_seq(length, seed)
    cut = a[:length // 2] + a[length // 2 + 1:]
    return [a, a] + ([cut] if cut else []) + [a[:length // 3] + b"G" + a[length // 3:], a[:-1] + a[-1:].translate(SWAP)]


def test_one_and_two_sequences(eng):
    a = mc.rand_seq(100, 11)
    same(eng, [a])
    same(eng, [a, a[:40] + a[44:]])
    same(eng, [b"A"])
    same(eng, [b"A", b"C"])


@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193])
def test_lane_and_stripe_edges(eng, length):
    same(eng, around(length, 100 + length))


def test_rows_of_every_edge_length_against_one_centre(eng):
    a = mc.rand_seq(193, 12)
    same(eng, [a] + [a[:n] for n in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)] + [a[193 - n:] for n in (1, 63, 64, 65, 128, 129)])


def test_longest_pair_runs_64_stripes(eng):
    a = mc.rand_seq(4095, 13)
    b = a[:1000] + a[1007:2500] + b"GTCA" + a[2500:3900] + a[3902:]
    assert len(b) == 4090
    want = same(eng, [a, b])
    assert want[0] == 0 and len(want[1][0]) == 4099


def test_indels_at_the_ends_and_across_a_stripe_boundary(eng):
    a = mc.rand_seq(200, 14)
    fill = mc.rand_seq(70, 15)
    seqs = [a, a,
            a[3:], a[:-3], b"TTGCA" + a, a + b"CCATG",          # first and last column
            a[:59] + a[70:],                                    # columns 60..70 cut: the run crosses lane 63 / lane 0
            a[:100] + fill + a[100:],                           # 70 bases in one slot
            a[:64] + fill[:5] + a[64:], a[:63] + a[65:],        # at the boundary itself
            a[:80] + a[80:88].translate(SWAP) + a[92:]]         # 8 bases that match nothing for 12: an insertion directly followed by a deletion
    want = same(eng, seqs)
    row = want[1][-1]
    assert b"-" in row and b"-" in want[1][0] and len(want[1][0]) >= 200 + 70


def test_rows_that_share_a_slot(eng):
    a = mc.rand_seq(150, 16)
    x = bytes(c for c in b"ACGT" if c not in (a[69], a[70]))[:1]      # a run of it between columns 70 and 71 can stand nowhere else
    two = [a, a, a[:70] + x + a[70:], a[:70] + x * 5 + a[70:]]
    want = same(eng, two)
    assert len(want[1][0]) == 155 and want[1][2][70:75] == x + b"----" and want[1][3][70:75] == x * 5
    same(eng, two + [a[:70] + x * 3 + a[70:], a[:64] + b"AC" + a[64:70] + x * 9 + a[70:]])


def test_mismatches_n_and_lower_case(eng):
    a = mc.rand_seq(100, 17)
    same(eng, [a, a, a.translate(SWAP)])                        # a row that matches nowhere
    c = mc.rand_seq(500, 18)
    same(eng, [c, c, b"G"])                                     # one base against 500 columns
    n = a[:20] + b"NNN" + a[23:50].lower() + a[50:]
    same(eng, [n, n, a, a.lower(), a[:10] + b"N" * 15 + a[25:], n[:30] + n[33:], b"n" * 40 + a[40:], a[:60] + b"RYK" + a[60:]])
    q = b"AAAAA" + b"N" * 14 + b"CCCCC"
    same(eng, [q, q])                                           # N on N is a mismatch: 14 of them cost more than two gaps


def test_family_of_300(eng, family_rows):
    seqs, want = family_rows
    got = eng.align_center_star(seqs)
    assert got[0] == want[0] and got[1] == want[1]
    assert [r.replace(b"-", b"") for r in got[1]] == seqs


CHILD = r"""
import pickle, sys
from metamlst_amd.engine import Engine
seqs = pickle.load(open(sys.argv[1], "rb"))
pickle.dump(Engine(0).align_center_star(seqs), open(sys.argv[2], "wb"))
"""


def test_family_in_three_batches(family_rows, tmp_path):
    """MLST_MSA_BATCH_BYTES is read when the engine is made: a fresh process.  The traceback store of a pair is
    ceil(m / 64) * ((longest + 63) // 4 + 1) * 256 bytes (csrc/msa_dev.h); the budget below holds fewer than half of the family's."""
    seqs, want = family_rows
    m, longest = len(seqs[want[0]]), max(map(len, seqs))
    per_pair = (m + 63) // 64 * ((longest + 63) // 4 + 1) * 256
    budget = per_pair * 107
    assert 3 <= -(-len(seqs) // (budget // per_pair)) < len(seqs)
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    pickle.dump(seqs, open(src, "wb"))
    env = dict(os.environ, MLST_MSA_BATCH_BYTES=str(budget),
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, "-c", CHILD, src, dst], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = pickle.load(open(dst, "rb"))
    assert got[0] == want[0] and got[1] == want[1]


def _align(e, seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
    flat = np.frombuffer(b"".join(seqs) or b"\0", np.uint8)
    width = C.c_uint32()
    return e.lib.mlst_msa_align(e._h, eng_mod._ptr(flat), eng_mod._ptr(off), len(seqs), None, C.byref(width)), width.value


def test_refusals_leave_the_handle_usable():
    e = Engine(0)
    buf = np.zeros(64, np.uint8)
    assert e.lib.mlst_msa_fetch(e._h, eng_mod._ptr(buf)) == -1                 # nothing aligned yet
    a = mc.rand_seq(50, 19)
    for seqs, rc in [([], -1), ([a, b""], -1), ([a, b"AC-T"], -1), ([b"AC T"], -1), ([a, b"AC1T"], -1), ([b"ACG\n"], -1), ([a, b"A" * 4096], -5)]:
        assert _align(e, seqs)[0] == rc, seqs
        assert e.lib.mlst_msa_fetch(e._h, eng_mod._ptr(buf)) == -1             # a refused call leaves no finished alignment
        same(e, [a, a[:20] + a[22:]])
    with pytest.raises(MlstError):
        e.align_center_star([a, b"AC-T"])
    # n x width >= 2^32: 1,050,000 sequences of one base and one of 4,095 that fills a slot of the one-column centre
    rc, _ = _align(e, [b"A"] * 1_050_000 + [b"C" * 4095])
    assert rc == -5 and b"2^32" in e.lib.mlst_last_error(e._h)
    assert e.lib.mlst_msa_fetch(e._h, eng_mod._ptr(buf)) == -1
    same(e, [a, a[:20] + a[22:]])
    e.close()


def test_refused_while_a_stream_is_open_and_typing_is_untouched():
    db, idx = fixtures.ecoli_small()
    fb, fq, off, _, _ = fixtures.isolate_reads(db, "ecoli", 3, n_reads=4000)
    a = mc.rand_seq(300, 20)
    seqs = [a, a, a[:100] + a[104:], a[:200] + b"GGA" + a[200:]]
    plain = Engine(0)
    plain.load_reference(idx)
    plain.submit_reads(fb, fq, off)
    want = plain.stats()
    e = Engine(0)
    e.load_reference(idx)
    e.submit_reads(fb, fq, off)
    rows = same(e, seqs)
    fixtures.assert_stats_equal(e.stats(), want)
    e.reset_sample()                                                            # leaves the finished alignment alone
    out = np.zeros((len(seqs), len(rows[1][0])), np.uint8)
    assert e.lib.mlst_msa_fetch(e._h, eng_mod._ptr(out)) == 0 and [r.tobytes() for r in out] == rows[1]
    e.submit_fastq_stream(b"@r\nACGTACGTAC", final=False)                       # a record cut in its sequence line: the stream stays open
    assert _align(e, seqs)[0] == -1 and b"FASTQ stream is open" in e.lib.mlst_last_error(e._h)
    assert e.lib.mlst_msa_fetch(e._h, eng_mod._ptr(out)) == -1
    e.reset_sample()
    same(e, seqs)
    e.submit_reads(fb, fq, off)
    fixtures.assert_stats_equal(e.stats(), want)
    same(e, seqs)
    e.close(); plain.close()


@pytest.fixture(scope="module")
def host_merged(tmp_path_factory):
    """merged/ of the tiny database as write_sequences leaves it with the host statement as aligner."""
    def statement(seqs):
        _, rows = center_star([q.encode() for _, q in seqs])
        return dict((i, r.decode()) for (i, _), r in zip(seqs, rows))

    folder = str(tmp_path_factory.mktemp("msa_host"))
    mc.merge_tiny(folder, statement)
    return os.path.join(folder, "nfo", "merged")


def _cli_merge(tmp_path, *more):
    path = mc.tiny_database(str(tmp_path / "cli"))
    empty = tmp_path / "nobin"
    empty.mkdir()
    env = dict(os.environ, PATH=str(empty),                                     # no MUSCLE to be found, wherever the test runs
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    return subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "merge", str(tmp_path / "cli" / "nfo"), "-d", path, "--outseqformat", "A"] + list(more),
                          env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("more", [("--aligner", "gpu"), ()], ids=["gpu", "auto_without_muscle"])
def test_cli_merge_with_the_gpu_aligner(tmp_path, host_merged, more):
    r = _cli_merge(tmp_path, *more)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr.count("aligner: the GPU engine (centre-star) on 5 sequences") == 1      # g2: four alleles of the database and the new one
    for name in ("_sequences.fna", "_ST.txt", "_report.txt"):
        host = open(os.path.join(host_merged, mc.SPECIES + name), "rb").read()
        assert open(str(tmp_path / "cli" / "nfo" / "merged" / (mc.SPECIES + name)), "rb").read() == host, name


def test_cli_merge_aligner_muscle_still_needs_muscle(tmp_path):
    r = _cli_merge(tmp_path, "--aligner", "muscle")
    assert r.returncode != 0 and "MUSCLE is needed" in r.stderr and "aligner: MUSCLE on 5 sequences" in r.stderr
