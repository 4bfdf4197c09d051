"""metamlst_amd.samout.md_text and the `md=True` of write_sam / format_record / all_records_rule (no GPU): bowtie2's MD:Z field as the
plain-Python rule states it.  Hand-written known answers, then an independent inverse -- the allele's bases under a record rebuilt
from SEQ + CIGAR + MD alone (`ref_from_md`, which shares no code with md_text) -- over every record the oracle decides for the
align_cases corpus, then the bytes without the switch and the refusals of `cli type --md`."""
import functools
import re

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
from metamlst_amd import cli, samin, samout, synth

M, I, D, S = 0, 1, 2, 4
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
CAP = 1 << 16
AZ_ELSE_N = bytes(c if 65 <= c <= 90 else 78 for c in range(256))      # the allele's letter as MD shows it
MINUS_33 = bytes((c - 33) & 255 for c in range(256))


def ops_of(*runs):
    return [(ln << 4) | op for ln, op in runs]


# ------------------------------------------------------------------ the inverse (shared with tests/test_gpu_export_md.py)
def ref_from_md(ops, seq: bytes, md: str) -> tuple[bytes, int, int]:
    """(the reference letters under the record's M and D columns, mismatch letters, deleted letters) from SEQ + CIGAR + MD alone, the
    way samtools / pysam rebuild them: the MD text is cut into numbers, letters and ^runs; an M column takes SEQ's letter while a
    number lasts and MD's letter where one stands; a D run takes its ^run.  Every token has to be used up exactly."""
    assert MD_RE.fullmatch(md), md
    toks = re.findall(r"[0-9]+|\^[A-Z]+|[A-Z]", md)
    assert "".join(toks) == md
    toks = [int(t) if t[0].isdigit() else t for t in toks]
    out, k, left, q, mism, dele = bytearray(), 0, toks[0], 0, 0, 0      # left: match columns still promised by the number at toks[k]
    for o in ops:
        ln, op = int(o) >> 4, int(o) & 15
        if op == M:
            end = q + ln
            while q < end:
                if left > 0:
                    take = min(left, end - q)
                    out += seq[q:q + take]; left -= take; q += take
                else:
                    t = toks[k + 1]
                    assert isinstance(t, str) and len(t) == 1, (md, k)
                    out.append(ord(t)); mism += 1
                    k += 2; left = toks[k]; q += 1
        elif op == D:
            assert left == 0, (md, k)                                    # a deletion stands behind a number that is used up
            t = toks[k + 1]
            assert isinstance(t, str) and t[0] == "^" and len(t) == ln + 1, (md, k, ln)
            out += t[1:].encode(); dele += ln
            k += 2; left = toks[k]
        elif op in (I, S):
            q += ln
        else:
            raise AssertionError("operation %d" % op)
    assert left == 0 and k == len(toks) - 1 and q == len(seq), (md, k, left)
    return bytes(out), mism, dele


def assert_inverse(idx, a, pos0, ops, seq: bytes, md: str, nm: int):
    """MD rebuilds allele[pos0 : pos0 + M + D] (upper case; a byte outside A-Z as N), and NM = mismatch letters + deleted letters +
    inserted bases"""
    ref, mism, dele = ref_from_md(ops, seq, md)
    span = sum(int(o) >> 4 for o in ops if int(o) & 15 in (M, D))
    want = idx.sequence(a).upper().encode()[pos0:pos0 + span].translate(AZ_ELSE_N)
    assert len(want) == span and ref == want, (a, pos0, md)
    ins = sum(int(o) >> 4 for o in ops if int(o) & 15 == I)
    assert nm == mism + dele + ins == samout.gap_figures(ops, seq, idx.sequence(a), pos0)[2], (a, pos0, md)


def assert_line_inverse(idx, label2a, line: bytes):
    """one line of an export with MD:Z: the field stands between NM:i and YT:Z:UU and passes the inverse; returns the MD text"""
    f = line.decode().rstrip("\n").split("\t")
    assert f[-1] == "YT:Z:UU" and f[-2].startswith("MD:Z:") and f[-3].startswith("NM:i:"), f[11:]
    assert sum(1 for t in f[11:] if t.startswith("MD:")) == 1
    assert_inverse(idx, label2a[f[2]], int(f[3]) - 1, samin.parse_cigar(f[5]), f[9].encode(), f[-2][5:], int(f[-3][5:]))
    return f[-2][5:]


# ------------------------------------------------------------------ known answers
class OneAllele:
    """as much of an AlleleIndex as format_record asks for: one allele"""
    n_alleles = 1
    off = [0, 0]

    def __init__(self, s):
        self.s, self.off = s, [0, len(s)]

    def sequence(self, a):
        return self.s

    def label(self, a):
        return "sp_gene_1"


REF = "ACGTTGCAAC" * 40      # 400 columns; REF[k] for the planted mismatches below


def seq_on(pos0, n, mism=()):
    """REF[pos0 : pos0 + n] with the read positions `mism` changed to another base"""
    s = bytearray(REF[pos0:pos0 + n].encode())
    for p in mism:
        s[p] = ac.other_base(s[p])
    return bytes(s)


def test_known_answers():
    md = samout.md_text
    assert md(ops_of((36, M)), seq_on(5, 36), REF, 5) == "36"
    assert md(ops_of((36, M)), seq_on(5, 36), REF.lower(), 5) == "36"                       # the allele is upper-cased first
    assert md(ops_of((35, M)), seq_on(0, 35, [0]), REF, 0) == "0A34"
    assert md(ops_of((35, M)), seq_on(10, 35, [34]), REF, 10) == "34%s0" % REF[44] == "34T0"
    assert md(ops_of((17, M)), seq_on(0, 17, [10, 11]), REF, 0) == "10A0C5"
    # a deletion, then a deletion directly followed by a mismatch: reference ...GGGGG AC T GGG
    ref = "GGGGGACTGGG"
    assert md(ops_of((5, M), (2, D), (4, M)), b"GGGGGTGGG", ref, 0) == "5^AC4"
    assert md(ops_of((5, M), (2, D), (4, M)), b"GGGGGAGGG", ref, 0) == "5^AC0T3"
    assert md(ops_of((4, M), (1, D), (2, M)), b"CGTTCA", "acgttgcaac", 1) == "4^G2"         # one base, lower-case allele, pos0 = 1
    # an insertion does not break a run; soft clips on both ends
    assert md(ops_of((20, M), (3, I), (30, M)), seq_on(7, 20) + b"TTT" + seq_on(27, 30), REF, 7) == "50"
    assert md(ops_of((4, S), (30, M), (6, S)), b"TTTT" + seq_on(100, 30) + b"GGGGGG", REF, 100) == "30"
    assert md(ops_of((4, S), (30, M), (6, S)), b"TTTT" + seq_on(100, 30, [0, 29]) + b"GGGGGG", REF, 100) == "0A28C0"
    assert md(ops_of((2, S), (10, M), (2, I), (10, M), (1, D), (10, M)), b"NN" + seq_on(0, 10) + b"AA" + seq_on(10, 10) + seq_on(21, 10, [0]), REF, 0) == "20^A0C9"
    # N on either side is a mismatch; the allele's N is written as N, a byte outside A-Z too
    assert md(ops_of((5, M)), b"ACNTT", "ACGTT", 0) == "2G2"
    assert md(ops_of((5, M)), b"ACGTT", "ACNTT", 0) == "2N2"
    assert md(ops_of((5, M)), b"ACNTT", "ACNTT", 0) == "2N2"
    assert md(ops_of((5, M)), b"ACGTT", "AC-TT", 0) == "2N2" and md(ops_of((2, M), (2, D), (1, M)), b"ACT", "ac*rt", 0) == "2^NR1"
    # runs of 9, 10, 99, 100 and 319 columns
    for run in (9, 10, 99, 100, 319):
        assert md(ops_of((run, M)), seq_on(3, run), REF, 3) == "%d" % run
        assert md(ops_of((run + 1, M)), seq_on(3, run + 1, [run]), REF, 3) == "%d%s0" % (run, REF[3 + run])
        assert md(ops_of((run + 1, M)), seq_on(3, run + 1, [0]), REF, 3) == "0%s%d" % (REF[3], run)


def test_the_inverse_on_the_known_answers():
    idx = OneAllele(REF)
    for ops, seq, pos0 in ((ops_of((36, M)), seq_on(5, 36), 5), (ops_of((17, M)), seq_on(0, 17, [10, 11]), 0),
                           (ops_of((4, S), (30, M), (6, S)), b"TTTT" + seq_on(100, 30, [0, 29]) + b"GGGGGG", 100),
                           (ops_of((2, S), (10, M), (2, I), (10, M), (1, D), (10, M)), b"NN" + seq_on(0, 10) + b"AA" + seq_on(10, 10) + seq_on(21, 10, [0]), 0),
                           (ops_of((320, M)), seq_on(40, 320, [63, 64, 319]), 40)):
        text = samout.md_text(ops, seq, REF, pos0)
        assert_inverse(idx, 0, pos0, ops, seq, text, samout.gap_figures(ops, seq, REF, pos0)[2])
    with pytest.raises(AssertionError):                                                      # the inverse does tell a wrong text
        assert_inverse(idx, 0, 5, ops_of((36, M)), seq_on(5, 36, [7]), "36", 1)
    with pytest.raises(AssertionError):
        assert_inverse(idx, 0, 0, ops_of((17, M)), seq_on(0, 17, [10, 11]), "10A0G5", 2)


# ------------------------------------------------------------------ the oracle's records of the crafted corpus
def ops_from_cols(cols, n):
    """the CIGAR of an alignment from its M columns (oriented read position, allele column): read bases between two columns are an
    insertion, allele columns a deletion (an insertion first where both stand), the ends are soft clips"""
    c = np.asarray(cols, np.int64)
    di, dj = np.diff(c[:, 0]) - 1, np.diff(c[:, 1]) - 1
    assert np.all(di >= 0) and np.all(dj >= 0)
    cuts = np.flatnonzero((di > 0) | (dj > 0))                           # a gap stands behind M column cuts[k]
    runs, start = [(int(c[0, 0]), S)], 0
    for k in cuts.tolist():
        runs += [(k + 1 - start, M), (int(di[k]), I), (int(dj[k]), D)]
        start = k + 1
    runs += [(len(c) - start, M), (n - 1 - int(c[-1, 0]), S)]
    return ops_of(*[(ln, op) for ln, op in runs if ln > 0])


@functools.lru_cache(maxsize=None)
def corpus_records():
    """the tuples format_record takes for every record the oracle decides over its own item list of the corpus (the reads of
    test_gpu_align_export.corpus_reads: the cases, then a planted 3-base insertion and deletion)"""
    cp = ac.corpus()
    a13 = cp.allele("plain", 13); s = cp.seq(a13)
    extra = [s[200:275] + b"GAT" + s[275:347], s[200:275] + s[278:353]]
    reads = [c.bases for c in cp.cases] + extra
    quals = [c.quals for c in cp.cases] + [b"I" * len(r) for r in extra]
    orc = oracle_lib.Oracle(cp.idx)
    orc.submit_reads(*synth.ragged_reads(reads, quals))
    _, items = orc.stats(want_items=CAP)
    assert 0 < len(items) < CAP
    out = []
    for ri, loc, strand, diag, _ in items.tolist():
        b, q = reads[ri], quals[ri]
        a0 = int(cp.idx.locus_begin[loc])
        for a in range(a0, a0 + int(cp.idx.locus_count[loc])):
            r = orc.align_one(b, q, a, strand, diag)
            if r["score"] >= ac.floor_score(len(b)) and r["score"] > 0:
                seq = ac.rc(b) if strand else b
                raw = (q[::-1] if strand else q).translate(MINUS_33)
                out.append((ri, strand, diag, loc, a, r["cols"][0][1], r["score"], r["xm"], ops_from_cols(r["cols"], len(b)), seq, raw))
    return out


def test_every_corpus_record_passes_the_inverse():
    idx = ac.corpus().idx
    recs = corpus_records()
    label2a = {idx.label(a): a for a in range(idx.n_alleles)}
    lines = samout.all_records_rule(idx, recs, False, md=True)
    assert len(lines) == len(recs) > 1000
    kinds = set()
    for line in lines:
        text = assert_line_inverse(idx, label2a, line)
        kinds |= {"plain"} if text.isdigit() else set()
        kinds |= {"del"} if "^" in text else set()
        kinds |= {"zero between"} if re.search(r"[A-Z]0[A-Z]", text) else set()
        kinds |= {"three digits"} if re.search(r"[0-9]{3}", text) else set()
        kinds |= {"N"} if "N" in text else set()
    # (a local alignment neither starts nor ends on a mismatch: those two stand among the known answers and in the crafted GPU set)
    assert kinds >= {"plain", "del", "zero between", "three digits", "N"}, kinds
    # the field is the only difference to the line without it (every 16th record, FLAG and XS as given)
    for r in recs[::16]:
        with_md, plain = samout.format_record(idx, r, False, True, 50, md=True), samout.format_record(idx, r, False, True, 50)
        assert re.sub(rb"\tMD:Z:[0-9A-Z^]+", b"", with_md) == plain != with_md and b"MD:Z" not in plain


# ------------------------------------------------------------------ switch off; the refusals
def test_md_false_gives_the_bytes_of_today(tmp_path):
    db, idx = fx.ecoli_small(8)
    a0 = int(idx.locus_begin[0])
    ref = idx.sequence(a0).upper().encode()
    sq = bytearray(ref[10:40] + ref[42:70]); sq[5] = ac.other_base(sq[5]); sq = bytes(sq)
    rec = (3, 0, 10, 0, a0, 10, 90, 1, ops_of((30, M), (2, D), (28, M)), sq, bytes([40]) * len(sq))
    base = samout.format_record(idx, rec, False, False, None)
    assert samout.format_record(idx, rec, False, False, None, None, False) == base and b"MD:Z" not in base
    with_md = samout.format_record(idx, rec, False, False, 77, md=True)
    text = "5%s24^%s28" % (chr(ref[15]), ref[40:42].decode())
    assert with_md.decode().rstrip("\n").split("\t")[11:] == ["AS:i:90", "XS:i:77", "XN:i:0", "XM:i:1", "XO:i:1", "XG:i:2", "NM:i:3", "MD:Z:" + text, "YT:Z:UU"]
    assert samout.all_records_rule(idx, [rec], False) == samout.all_records_rule(idx, [rec], False, None, False) == [base]

    class Aln:      # engine.Alignments, as far as write_sam reads it
        read_index = np.array([3], np.uint64); allele = np.array([a0], np.uint32); pos0 = np.array([10], np.int32)
        as_ = np.array([90], np.int32); xm = np.array([1], np.int32); diag = np.array([10], np.int32); flags = np.array([0], np.uint8)
        cigar_off = np.array([0, 3], np.uint64); cigar = np.array(ops_of((30, M), (2, D), (28, M)), np.uint32)
        seq_off = np.array([0, len(sq)], np.uint64); seq = np.frombuffer(sq, np.uint8); qual = np.full(len(sq), 40, np.uint8)

        def __len__(self):
            return 1
    assert samout.write_sam(str(tmp_path / "a.sam"), idx, [a0], Aln(), False) == 1
    assert samout.write_sam(str(tmp_path / "b.sam"), idx, [a0], Aln(), False, None, False) == 1
    assert samout.write_sam(str(tmp_path / "c.sam"), idx, [a0], Aln(), False, md=True) == 1
    a, b, c = (open(tmp_path / f, "rb").read() for f in ("a.sam", "b.sam", "c.sam"))
    assert a == b and b"MD:Z" not in a
    assert c == a.replace(b"\tNM:i:3\tYT:Z:UU", b"\tNM:i:3\tMD:Z:" + text.encode() + b"\tYT:Z:UU") != a
    # columns 12 and 15 are where they were (Q1, the positional parse)
    la, lc = a.splitlines()[-1].split(b"\t"), c.splitlines()[-1].split(b"\t")
    assert la[:18] == lc[:18] and lc[11].startswith(b"AS:i:") and lc[14].startswith(b"XM:i:")


@pytest.mark.parametrize("argv, words", [(["a.fastq"], "--md: it adds MD:Z to the records of an export: give --write-sam or --write-sam-all"),
                                         (["a.sam", "--alignments", "--write-sam"], "--write-sam writes the engine's own alignments"),
                                         (["a.fastq", "b.fastq", "--write-sam-all"], "--write-sam-all takes one sample"),
                                         (["a.fastq", "--gpus", "2", "--write-sam", "--write-sam-all"], "--write-sam takes one GPU"),
                                         (["a.fastq", "--read-names"], "--read-names: it names the reads of an export")])
def test_cli_refuses_md_where_the_exports_are_refused(tmp_path, capsys, monkeypatch, argv, words):
    def no_engine(*a, **k):
        raise AssertionError("an Engine was created")
    monkeypatch.setattr(cli, "Engine", no_engine)
    monkeypatch.setattr("metamlst_amd.multigpu.launch_ranks", no_engine, raising=False)
    for f in ("a.sam", "a.fastq", "b.fastq"):
        (tmp_path / f).write_text("")
    argv = [str(tmp_path / x) if x.endswith((".sam", ".fastq")) else x for x in argv]
    assert cli.main(["type"] + argv + ["--md", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]) == 1
    assert words in capsys.readouterr().out
