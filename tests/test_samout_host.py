"""metamlst_amd.samout.write_sam on hand-made records (no GPU): every column against the rules of the module's docstring, the
file's bytes under a permutation of the records, XO / XG / NM against a plain recount, the way back through samin's host SAM
reader, and the three combinations `cli type --write-sam` refuses."""
import numpy as np
import pytest

import fixtures as fx
from metamlst_amd import cli, samin, samout
from metamlst_amd.engine import Alignments
from metamlst_amd.typing import TypingArgs

M, I, D, S = 0, 1, 2, 4
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def hand_made(idx):
    """(chosen, Alignments, rows): records written down by hand on the first allele of loci 0..2.  A row is (read_index, allele,
    pos0, strand, diag, AS, XM, [(len, op)], SEQ, Phred list): SEQ follows the allele on M except where a mismatch or an N is
    planted, is foreign on I and S."""
    chosen = [int(idx.locus_begin[l]) for l in (2, 0, 1)]                  # @SQ order is the order given, not allele order
    a0, a1, a2 = (int(idx.locus_begin[l]) for l in (0, 1, 2))
    rng = np.random.default_rng(5)

    def seq_for(a, pos0, ops, mism=(), n_at=()):
        ref, out, r = idx.sequence(a).encode(), bytearray(), pos0
        for ln, op in ops:
            if op == M:
                out += ref[r:r + ln]; r += ln
            elif op == D:
                r += ln
            else:
                out += bytes(rng.choice(list(b"ACGT"), size=ln).astype(np.uint8))
        for p in mism:
            out[p] = out[p:p + 1].translate(COMP)[0]
        for p in n_at:
            out[p] = ord("N")
        return bytes(out)

    def row(ri, a, pos0, strand, diag, AS, XM, ops, q=None, **kw):
        seq = seq_for(a, pos0, ops, **kw)
        return (ri, a, pos0, strand, diag, AS, XM, ops, seq, q if q is not None else [40] * len(seq))
    rows = [
        row(0, a0, 10, 0, 10, 100, 0, [(50, M)]),
        row(1, a0, 10, 1, 5, 84, 1, [(5, S), (40, M), (7, S)], mism=(20,)),                                   # clips at either end, reverse strand
        row(2, a0, 30, 0, 30, 120, 0, [(30, M), (3, I), (40, M)]),                                             # an I run
        row(3, a1, 0, 1, 0, 111, 2, [(4, S), (25, M), (2, D), (30, M)], mism=(10, 40)),                        # a D run, leading clip
        row(4, a1, 7, 0, 7, 90, 2, [(45, M)], q=[0, 93, 127] + [30] * 42, mism=(20,), n_at=(9,)),              # an N, Phred 0 / 93 / 127
        row(5, a2, 3, 0, 3, 96, 0, [(48, M)]), row(5, a2, 200, 1, 200, 96, 0, [(48, M)]),                      # two records of one read, equal AS
        row(5, a0, 100, 0, 100, 60, 6, [(30, M), (1, D), (1, I), (20, M)]),                                    # a third, worse one (I next to D)
        row(6, a2, 50, 0, 50, 100, 0, [(50, M)]), row(7, a2, 120, 1, 120, 98, 1, [(50, M)], mism=(3,)),        # mates: read 6 and read 7
        row(9, a2, 50, 1, 50, 100, 0, [(50, M)]), row(8, a2, 50, 0, 50, 100, 0, [(50, M)]),                    # equal (allele, pos0): read_index decides
    ]
    return chosen, to_alignments(rows), rows


def to_alignments(rows) -> Alignments:
    n = len(rows)
    co, so = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    co[1:] = np.cumsum([len(r[7]) for r in rows]); so[1:] = np.cumsum([len(r[8]) for r in rows])
    return Alignments(np.array([r[0] for r in rows], np.uint64), np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], np.int32),
                      np.array([r[5] for r in rows], np.int32), np.array([r[6] for r in rows], np.int32), np.array([r[4] for r in rows], np.int32),
                      np.array([r[3] for r in rows], np.uint8), co, np.array([(ln << 4) | op for r in rows for ln, op in r[7]], np.uint32), so,
                      np.frombuffer(b"".join(r[8] for r in rows), np.uint8), np.array([q for r in rows for q in r[9]], np.uint8))


def recount(ops, seq, allele, pos0):
    """XO, XG, NM column by column"""
    xo = xg = nm = 0
    q, r = 0, pos0
    for ln, op in ops:
        for k in range(ln):
            if op == M:
                nm += seq[q] != allele[r] or seq[q] == "N"; q += 1; r += 1
            elif op == I:
                xg += 1; nm += 1; q += 1
            elif op == D:
                xg += 1; nm += 1; r += 1
            else:
                q += 1
        xo += op in (I, D)
    return xo, xg, nm


@pytest.fixture(scope="module")
def idx():
    return fx.ecoli_small(8)[1]


def written(tmp_path, idx, chosen, aln, paired, name="s.sam"):
    p = str(tmp_path / name)
    assert samout.write_sam(p, idx, chosen, aln, paired) == len(aln)
    return p, open(p, "rb").read()


def test_every_column_follows_the_rules(tmp_path, idx):
    chosen, aln, rows = hand_made(idx)
    for paired in (False, True):
        _, data = written(tmp_path, idx, chosen, aln, paired, "p%d.sam" % paired)
        lines = data.decode().split("\n")
        assert lines[-1] == "" and lines[0] == "@HD\tVN:1.6\tSO:coordinate"
        assert lines[1:4] == ["@SQ\tSN:%s\tLN:%d" % (idx.label(a), len(idx.sequence(a))) for a in chosen]
        assert lines[4].startswith("@PG\t") and not lines[5].startswith("@")
        body = [l.split("\t") for l in lines[5:-1]]
        want = sorted(rows, key=lambda r: (chosen.index(r[1]), r[2], r[0], r[3], r[4]))
        assert len(body) == len(want)
        # the best record of a read: highest AS, ties to the first in file order
        best = {}
        for k, r in enumerate(want):
            if r[0] not in best or r[5] > want[best[r[0]]][5]:
                best[r[0]] = k
        for k, (f, r) in enumerate(zip(body, want)):
            ri, a, pos0, strand, diag, AS, XM, ops, seq, q = r
            xo, xg, nm = recount(ops, seq.decode(), idx.sequence(a), pos0)
            assert f[0] == "r%d" % (ri >> 1 if paired else ri)
            assert int(f[1]) == 16 * strand + (0 if best[ri] == k else 256)
            assert f[2:9] == [idx.label(a), str(pos0 + 1), "255", "".join("%d%s" % (ln, "MIDNS"[op]) for ln, op in ops), "*", "0", "0"]
            assert f[9] == seq.decode() and f[10] == "".join(chr(min(x, 93) + 33) for x in q)
            assert f[11:] == ["AS:i:%d" % AS, "XS:i:%d" % AS, "XN:i:0", "XM:i:%d" % XM, "XO:i:%d" % xo, "XG:i:%d" % xg, "NM:i:%d" % nm, "YT:Z:UU"]
        flags = {}
        for f in body:
            flags.setdefault(f[0], []).append(int(f[1]) & 256)
        if not paired:
            assert flags["r5"].count(0) == 1 and len(flags["r5"]) == 3 and flags["r6"] == [0] and flags["r7"] == [0]
            assert [f[0] for f in body if f[2] == idx.label(chosen[0]) and f[3] == "51"] == ["r6", "r8", "r9"]
        else:
            assert flags["r3"] == [0, 0]                                   # the mates share a name; each keeps its own primary record
    text = written(tmp_path, idx, chosen, aln, False)[1].decode()
    assert "\t~!~" not in text and "!~~" in text                           # Phred 0, 93 and 127 (capped) of read 4


def test_gap_figures_equal_a_plain_recount(idx):
    chosen, aln, rows = hand_made(idx)
    seen = set()
    for k, r in enumerate(rows):
        ops = aln.cigar[int(aln.cigar_off[k]):int(aln.cigar_off[k + 1])]
        got = samout.gap_figures(ops, r[8], idx.sequence(r[1]), r[2])
        assert got == recount(r[7], r[8].decode(), idx.sequence(r[1]), r[2]), k
        seen.add(got)
    assert (1, 3, 3) in seen and (1, 2, 4) in seen and (2, 2, 2) in seen and any(g[0] == 0 and g[2] == 2 for g in seen)      # I, D + 2 mismatches, D next to I, mismatch + N


def test_the_bytes_do_not_depend_on_the_order_of_the_records(tmp_path, idx):
    chosen, aln, rows = hand_made(idx)
    _, want = written(tmp_path, idx, chosen, aln, True, "a.sam")
    rng = np.random.default_rng(11)
    for t in range(3):
        perm = rng.permutation(len(rows)).tolist()
        _, got = written(tmp_path, idx, chosen, to_alignments([rows[k] for k in perm]), True, "b%d.sam" % t)
        assert got == want
    _, none = written(tmp_path, idx, chosen, to_alignments([]), False, "empty.sam")
    assert none.decode().count("\n") == 2 + len(chosen) and b"\nr" not in none      # a header-only file


def test_samins_host_reader_parses_the_file_back(tmp_path, idx):
    chosen, aln, rows = hand_made(idx)
    p, _ = written(tmp_path, idx, chosen, aln, False)
    smp = samin.AlignmentSample(idx, TypingArgs()).add_file(p)
    want = sorted(rows, key=lambda r: (chosen.index(r[1]), r[2], r[0], r[3], r[4]))
    assert len(smp._rec) == len(want) == smp.n_records
    for got, r in zip(smp._rec, want):
        ri, a, pos0, strand, diag, AS, XM, ops, seq, q = r
        assert got == (a, pos0, AS, XM, [(ln << 4) | op for ln, op in ops], seq.decode(), "".join(chr(min(x, 93) + 33) for x in q))
    assert samin.read_sam_header(p) == [idx.label(a) for a in chosen]
    # ... and the 12th / 15th columns the reference reads by position are AS and XM (metamlst.py:109-110)
    st = smp.stats()
    ok = [r for r in rows if r[5] >= 80 and r[6] <= 5 and len(r[8]) >= 50]
    for a in chosen:
        assert int(st.sum_score[a]) == sum(r[5] for r in ok if r[1] == a) and int(st.n_hits[a]) == sum(1 for r in ok if r[1] == a)


REFUSED = {
    "alignments": (["x.sam", "--alignments"], "with --alignments the file is the input"),
    "several_samples": (["a.fastq", "b.fastq"], "--write-sam takes one sample"),
    "gpus": (["a.fastq", "--gpus", "2"], "--write-sam takes one GPU"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_the_cli_refuses_before_any_engine_is_made(name, tmp_path, capsys, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an Engine was created")
    monkeypatch.setattr(cli, "Engine", no_engine)
    monkeypatch.setattr("metamlst_amd.multigpu.launch_ranks", no_engine, raising=False)
    argv, words = REFUSED[name]
    assert cli.main(["type"] + argv + ["--write-sam", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]) == 1
    out = capsys.readouterr().out
    assert words in out and out.count("\n") == 1
    assert not (tmp_path / "out").exists()
