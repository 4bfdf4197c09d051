"""metamlst_amd.samout.format_record / all_records_rule on hand-made tuples (no GPU): the plain-Python statement of the full export
(`cli type --write-sam-all`): XS present / absent, FLAG ties, the order of the file, XO / XG / NM against gap_figures and a plain
recount, the header, and the way back through samin's host SAM reader."""
import io

import pytest

import fixtures as fx
from metamlst_amd import cli, samin, samout

M, I, D, S = 0, 1, 2, 4


@pytest.fixture(scope="module")
def idx():
    return fx.ecoli_small(8)[1]


def ops_of(*runs):
    return [(ln << 4) | op for ln, op in runs]


def rec(idx, ri, strand, diag, a, pos0, AS, XM, runs, mism=(), phred=40):
    """a tuple as format_record takes it: SEQ follows the allele on M (except at `mism`), is 'T...' on I and S"""
    ref, out, r = idx.sequence(a).upper().encode(), bytearray(), pos0
    for ln, op in runs:
        if op == M:
            out += ref[r:r + ln]; r += ln
        elif op == D:
            r += ln
        else:
            out += b"T" * ln
    for p in mism:
        out[p] = ord("A") if out[p] != ord("A") else ord("C")
    return (ri, strand, diag, int(idx.locus_id[a]), a, pos0, AS, XM, ops_of(*runs), bytes(out), bytes([phred]) * len(out))


def sample(idx):
    a0, a1 = int(idx.locus_begin[0]), int(idx.locus_begin[1])
    return [
        rec(idx, 7, 0, 10, a0, 10, 100, 0, [(50, M)]),                                        # read 7: one record -> no XS
        rec(idx, 3, 1, 5, a0 + 1, 10, 84, 1, [(5, S), (40, M), (7, S)], mism=(20,)),          # read 3: three records, two share the best AS
        rec(idx, 3, 1, 5, a0, 10, 90, 1, [(5, S), (40, M), (7, S)], mism=(21,)),
        rec(idx, 3, 0, 40, a1, 40, 90, 0, [(30, M), (3, I), (12, M)]),
        rec(idx, 5, 0, 0, a1 + 2, 0, 70, 2, [(4, S), (25, M), (2, D), (30, M)], mism=(10, 40)),      # read 5: two records, the later one is better
        rec(idx, 5, 0, 0, a1 + 3, 0, 96, 0, [(59, M)], phred=120),
        rec(idx, 2 ** 32 + 1, 1, -3, a0, 0, 60, 0, [(3, S), (30, M)]),                        # a read index past 32 bits, overhang at the start
    ]


def fields(line: bytes):
    assert line.endswith(b"\n") and b"\n" not in line[:-1] and b"\t\t" not in line
    return line[:-1].decode().split("\t")


def test_xs_flag_and_order(idx):
    recs = sample(idx)
    lines = samout.all_records_rule(idx, recs, False)
    f = [fields(l) for l in lines]
    assert [x[0] for x in f] == ["r3", "r3", "r3", "r5", "r5", "r7", "r%d" % (2 ** 32 + 1)]
    # read 3: locus 0 before locus 1; inside the item the alleles ascend; the first of the two records with AS 90 is the best
    a0, a1 = int(idx.locus_begin[0]), int(idx.locus_begin[1])
    assert [x[2] for x in f[:3]] == [idx.label(a0), idx.label(a0 + 1), idx.label(a1)]
    assert [int(x[1]) for x in f[:3]] == [16, 16 + 256, 256]
    assert [x[11:13] for x in f[:3]] == [["AS:i:90", "XS:i:90"], ["AS:i:84", "XS:i:90"], ["AS:i:90", "XS:i:90"]]
    # read 5: the second record in file order is the best one; XS is the other's AS
    assert [int(x[1]) for x in f[3:5]] == [256, 0] and [x[11:13] for x in f[3:5]] == [["AS:i:70", "XS:i:96"], ["AS:i:96", "XS:i:70"]]
    # one record: no XS, so XO stands in the 15th column (Q1)
    for x in (f[5], f[6]):
        assert len(x) == 18 and x[12] == "XN:i:0" and x[13].startswith("XM:i:") and x[14].startswith("XO:i:")
    assert all(len(x) == 19 and x[14].startswith("XM:i:") for x in f[:5])
    assert int(f[6][1]) == 16 and f[6][3] == "1" and f[6][5] == "3S30M"
    assert f[4][10] == chr(93 + 33) * 59 and f[0][10] == "I" * 52                     # QUAL is capped at Phred 93
    # the lines do not depend on the order the tuples come in
    assert samout.all_records_rule(idx, recs[::-1], False) == lines
    # paired: mates share a name, the rest stays
    assert [fields(l)[0] for l in samout.all_records_rule(idx, recs, True)] == ["r1", "r1", "r1", "r2", "r2", "r3", "r%d" % (2 ** 31)]
    assert [fields(l)[1:] for l in samout.all_records_rule(idx, recs, True)] == [x[1:] for x in f]


def test_gap_figures_agree_with_a_recount(idx):
    for r, line in zip(sorted(sample(idx), key=lambda r: (r[0], r[3], r[1], r[2], r[4])), samout.all_records_rule(idx, sample(idx), False)):
        tags = dict((t[:2], int(t[5:])) for t in fields(line)[11:] if t[3] == "i")
        ref, seq = idx.sequence(r[4]).upper(), r[9].decode()
        xo = xg = nm = 0
        q, p = 0, r[5]
        for o in r[8]:
            ln, op = o >> 4, o & 15
            if op == M:
                nm += sum(1 for k in range(ln) if seq[q + k] != ref[p + k] or seq[q + k] == "N"); q += ln; p += ln
            elif op == I:
                xo += 1; xg += ln; nm += ln; q += ln
            elif op == D:
                xo += 1; xg += ln; nm += ln; p += ln
            else:
                q += ln
        assert (tags["XO"], tags["XG"], tags["NM"]) == (xo, xg, nm) == samout.gap_figures(r[8], r[9], idx.sequence(r[4]), r[5])
        assert (tags["AS"], tags["XM"]) == (r[6], r[7])
    assert any(fields(l)[15] != "XG:i:0" for l in samout.all_records_rule(idx, sample(idx), False))


def test_header_and_the_way_back_through_the_host_reader(idx):
    head = samout.sam_all_header(idx)
    hl = head.split("\n")
    assert hl[0] == "@HD\tVN:1.6\tSO:unsorted\tGO:query" and hl[-2] == samout.PG_LINE and hl[-1] == ""
    assert hl[1:-2] == ["@SQ\tSN:%s\tLN:%d" % (idx.label(a), len(idx.sequence(a))) for a in range(idx.n_alleles)]
    recs = sample(idx)
    lines = samout.all_records_rule(idx, recs, False)
    back = list(samin._iter_sam_lines(io.StringIO(head + b"".join(lines).decode())))
    order = sorted(recs, key=lambda r: (r[0], r[3], r[1], r[2], r[4]))
    assert len(back) == len(order)
    for al, r in zip(back, order):
        assert (al.qname, al.flag & 16, al.rname, al.pos, al.seq) == ("r%d" % r[0], 16 * r[1], idx.label(r[4]), r[5] + 1, r[9].decode())
        assert samin.parse_cigar(al.cigar) == r[8] and al.tags[-1] == "YT:Z:UU"
    # every record again through format_record, with the FLAG and XS the file states: the same bytes
    again = []
    for al, r in zip(back, order):
        xs = [int(t[5:]) for t in al.tags if t.startswith("XS:i:")]
        again.append(samout.format_record(idx, r, False, bool(al.flag & 256), xs[0] if xs else None))
    assert again == lines


@pytest.mark.parametrize("argv, words", [(["a.sam", "--alignments"], "--write-sam-all writes the engine's own alignments"),
                                         (["a.fastq", "b.fastq"], "--write-sam-all takes one sample"),
                                         (["a.fastq", "--gpus", "2"], "--write-sam-all takes one GPU")])
def test_cli_refuses_what_write_sam_refuses(tmp_path, capsys, monkeypatch, argv, words):
    def no_engine(*a, **k):
        raise AssertionError("an Engine was created")
    monkeypatch.setattr(cli, "Engine", no_engine)
    monkeypatch.setattr("metamlst_amd.multigpu.launch_ranks", no_engine, raising=False)
    for f in ("a.sam", "a.fastq", "b.fastq"):
        (tmp_path / f).write_text("")
    argv = [str(tmp_path / x) if x.endswith((".sam", ".fastq")) else x for x in argv]
    assert cli.main(["type"] + argv + ["--write-sam-all", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]) == 1
    assert words in capsys.readouterr().out
