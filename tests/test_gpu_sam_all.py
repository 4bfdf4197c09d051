"""mlst_alignments_text_open / _next / _close (csrc/aln_text.h), Engine.export_sam_text, samout.write_sam_all and
`cli type --write-sam-all`: every alignment of a sample as SAM text formatted on the device, against the oracle's align_one over the
item list, the plain-Python rule (samout.format_record), pass 1's statistics, the export to the chosen alleles and both SAM readers.

The file carries no diagonal, so "the set of (read, strand, diag, allele)" is checked through the order: the oracle's records are
laid out in the stated order (items by read, locus, strand, diag; alleles ascending) and the k-th record of the file has to be the
k-th of them, with the columns (pairs_of its CIGAR) the oracle aligned on that diagonal.

orc_accumulate_records knows no mates (it credits a locus once per read index), so under paired=True the oracle is given the read
indices and checks sum_score, n_hits and the counters; locus_len_sum under paired=True is checked by the reference-pinned host reader
(samin.AlignmentSample), which sees the shared names."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
from metamlst_amd import cli, samin, samout
from metamlst_amd.engine import MlstError, _ptr
from metamlst_amd.typing import TypingArgs, pick_alleles_fast
from test_gpu_align_export import CAP, corpus_oracle, corpus_reads, make_engine, pairs_of, synth_sample

pytestmark = pytest.mark.gpu

ORDER = "the records are not in (read index, locus, strand, diag, allele) order"


class Rec:
    """one parsed record of the full export"""
    __slots__ = ("ri", "flag", "a", "pos0", "ops", "seq", "qual", "tags", "xs")

    def __init__(self, al, label2a):
        assert re.fullmatch(r"r(0|[1-9][0-9]*)", al.qname), al.qname
        self.ri, self.flag, self.a, self.pos0 = int(al.qname[1:]), al.flag, label2a[al.rname], al.pos - 1
        self.ops, self.seq, self.qual = samin.parse_cigar(al.cigar), al.seq.encode(), al.qual.encode()
        names = [t[:5] for t in al.tags]
        self.xs = int(al.tags[1][5:]) if names[1] == "XS:i:" else None
        assert names == ["AS:i:"] + (["XS:i:"] if self.xs is not None else []) + ["XN:i:", "XM:i:", "XO:i:", "XG:i:", "NM:i:", "YT:Z:"], al.tags
        assert al.tags[-1] == "YT:Z:UU" and "XN:i:0" in al.tags
        self.tags = {t[:2]: int(t[5:]) for t in al.tags[:-1]}

    def as_tuple(self, idx):
        """the tuple samout.format_record takes (the diagonal is no column of the file: 0)"""
        return (self.ri, (self.flag >> 4) & 1, 0, int(idx.locus_id[self.a]), self.a, self.pos0, self.tags["AS"], self.tags["XM"], self.ops, self.seq,
                bytes(c - 33 for c in self.qual))


def export(eng, idx, path, paired=False, round_bytes=0):
    """(records, record bytes): the file written by samout.write_sam_all, its header checked against the stated one"""
    n = samout.write_sam_all(str(path), idx, eng, paired, round_bytes)
    data = open(path, "rb").read()
    head = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (idx.label(a), len(idx.sequence(a))) for a in range(idx.n_alleles)) + "@PG\tID:metamlst_amd\tPN:metamlst_amd\n"
    assert data.startswith(head.encode())
    body = data[len(head):]
    assert body.count(b"\n") == n and (not body or body.endswith(b"\n")) and b"@" not in body[:1]
    label2a = {idx.label(a): a for a in range(idx.n_alleles)}
    recs = [Rec(al, label2a) for al in samin.read_alignments(str(path))]
    assert len(recs) == n
    return recs, body


def assert_flag_and_xs(recs):
    """FLAG 256 on every record of a read but its best (highest AS, the first of equal ones); XS iff the read has two records or more,
    the highest AS among the others"""
    k = 0
    while k < len(recs):
        e = k
        while e < len(recs) and recs[e].ri == recs[k].ri:
            e += 1
        scores = [r.tags["AS"] for r in recs[k:e]]
        best = scores.index(max(scores))
        for t, r in enumerate(recs[k:e]):
            others = scores[:t] + scores[t + 1:]
            assert r.flag & ~(16 | 256) == 0 and bool(r.flag & 256) == (t != best), (r.ri, t)
            assert r.xs == (max(others) if others else None), (r.ri, t)
        k = e
    assert len(set(r.ri for r in recs)) == sum(1 for k, r in enumerate(recs) if k == 0 or recs[k - 1].ri != r.ri), "the records of a read are not consecutive"


def assert_rule_bytes(idx, recs, body):
    """format_record over the parsed records gives the file's bytes: no leading zeros, single TABs, LF"""
    assert b"".join(samout.format_record(idx, r.as_tuple(idx), False, bool(r.flag & 256), r.xs) for r in recs) == body


# ------------------------------------------------------------------ the crafted corpus
@pytest.fixture(scope="module")
def corpus_engine():
    eng = make_engine(ac.corpus().idx)
    eng.submit_reads(*corpus_reads())
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def corpus_export(corpus_engine, tmp_path_factory):
    idx = ac.corpus().idx
    path = tmp_path_factory.mktemp("all") / "corpus.all.sam"
    recs, body = export(corpus_engine, idx, path)
    return str(path), recs, body


@functools.lru_cache(maxsize=None)
def _expected(items_key):
    """the oracle's records over the item list, in file order: (read, strand, diag, allele, align_one's result)"""
    cp = ac.corpus()
    fb, fq, off = corpus_reads()
    orc, _ = corpus_oracle()
    out = []
    for ri, loc, strand, diag in sorted(items_key, key=lambda t: (t[0], t[1], t[2], t[3])):
        b, q = fb[int(off[ri]):int(off[ri + 1])].tobytes(), fq[int(off[ri]):int(off[ri + 1])].tobytes()
        a0 = int(cp.idx.locus_begin[loc])
        for a in range(a0, a0 + int(cp.idx.locus_count[loc])):
            r = orc.align_one(b, q, a, strand, diag)
            if r["score"] >= ac.floor_score(len(b)) and r["score"] > 0:
                out.append((ri, strand, diag, a, r))
    return out


def expected(eng):
    return _expected(tuple((int(ri), int(loc), int(strand), int(diag)) for ri, loc, strand, diag, _ in eng.items(CAP).tolist()))


def test_corpus_records_equal_the_oracle_exhaustively(corpus_engine, corpus_export):
    cp, eng = ac.corpus(), corpus_engine
    idx = cp.idx
    fb, fq, off = corpus_reads()
    _, so = corpus_oracle()
    fx.assert_stats_equal(eng.stats(), so)
    _, recs, _ = corpus_export
    want = expected(eng)
    assert int(eng.stats().counters[0]) == len(want) > 1000                                  # MLST_CNT_TOTAL_RECORDS
    got_keys, want_keys = [(r.ri, (r.flag >> 4) & 1, r.a) for r in recs], [(ri, s, a) for ri, s, _, a, _ in want]
    assert got_keys == want_keys, "first difference at record %d" % next((k for k, (x, y) in enumerate(zip(got_keys, want_keys)) if x != y), min(len(got_keys), len(want_keys)))
    kinds = set()
    n_per_read = {}
    for r in recs:
        n_per_read[r.ri] = n_per_read.get(r.ri, 0) + 1
    for r, (ri, strand, diag, a, o) in zip(recs, want):
        key = (ri, strand, diag, a)
        b, q = fb[int(off[ri]):int(off[ri + 1])].tobytes(), fq[int(off[ri]):int(off[ri + 1])].tobytes()
        n, m = len(b), len(idx.sequence(a))
        ops = [(x >> 4, x & 15) for x in r.ops]
        assert (r.tags["AS"], r.tags["XM"], r.tags["XO"]) == (o["score"], o["xm"], o["xo"]), key
        assert pairs_of(ops, r.pos0) == o["cols"] and r.pos0 == min(j for _, j in o["cols"]), (key, ops)
        assert all(ln > 0 for ln, _ in ops) and all(op != ops[t + 1][1] for t, (_, op) in enumerate(ops[:-1])), (key, ops)
        assert r.seq == (ac.rc(b) if strand else b), key
        assert r.qual == bytes(min(x - 33, 93) + 33 for x in (q[::-1] if strand else q)), key
        assert (r.tags["XO"], r.tags["XG"], r.tags["NM"]) == samout.gap_figures(r.ops, r.seq, idx.sequence(a), r.pos0), key
        assert (r.xs is None) == (n_per_read[ri] == 1), key
        kinds |= {"I" if op == 1 else "D" for _, op in ops if op in (1, 2)}
        kinds |= {"lead%d" % strand} if ops[0][1] == 4 else set()
        kinds |= {"trail%d" % strand} if ops[-1][1] == 4 else set()
        kinds |= ({"over_start"} if diag < 0 else set()) | ({"over_end"} if diag + n > m else set())
        kinds |= {"tag_filter"} if (o["score"] < 80 or o["xm"] > 5) else set()
        kinds |= ({"N"} if b"N" in b else set()) | ({"n36"} if n == 36 else set()) | ({"n320"} if n == 320 else set())
        kinds |= {"I3"} if (3, 1) in ops else set()
        kinds |= {"D3"} if (3, 2) in ops else set()
        kinds |= {"XS absent"} if r.xs is None else {"XS present"}
        kinds |= {"XS absent with a gap"} if r.xs is None and r.tags["XO"] > 0 else set()
        cnt, a_local = int(idx.locus_count[idx.locus_id[a]]), a - int(idx.locus_begin[idx.locus_id[a]])
        kinds |= {"partly empty wave"} if cnt % 64 and a_local >= cnt - cnt % 64 else set()      # a record in a pass whose lanes are not all alleles
        kinds |= {"second pass"} if a_local >= 64 else set()
        kinds |= {"dp"} if o["used_dp"] else set()
    assert kinds >= {"I", "D", "lead0", "lead1", "trail0", "trail1", "over_start", "over_end", "tag_filter", "N", "n36", "n320", "I3", "D3",
                     "XS absent", "XS present", "XS absent with a gap", "partly empty wave", "second pass", "dp"}, kinds
    assert_flag_and_xs(recs)


def test_corpus_bytes_are_the_rule(corpus_engine, corpus_export):
    idx = ac.corpus().idx
    _, recs, body = corpus_export
    keys = [(r.ri, int(idx.locus_id[r.a])) for r in recs]
    assert keys == sorted(keys), ORDER
    assert_rule_bytes(idx, recs, body)
    assert b"\t\t" not in body and b"\r" not in body and b" " not in body


@pytest.mark.parametrize("base", [2 ** 32 - 3, 10 ** 10 - 3])
def test_read_indices_past_32_bits_and_ten_digits(corpus_export, tmp_path, base):
    cp = ac.corpus()
    _, recs0, _ = corpus_export
    eng = make_engine(cp.idx)
    try:
        eng.set_read_index_base(base)
        eng.submit_reads(*corpus_reads())
        recs, body = export(eng, cp.idx, tmp_path / "base.all.sam")
        names = set(r.ri for r in recs)
        assert min(names) < 2 ** 32 <= max(names) if base < 2 ** 32 else min(names) < 10 ** 10 <= max(names)
        assert [(r.ri - base, r.flag, r.a, r.pos0, r.ops, r.xs, r.tags) for r in recs] == [(r.ri, r.flag, r.a, r.pos0, r.ops, r.xs, r.tags) for r in recs0]
        assert_rule_bytes(cp.idx, recs, body)
    finally:
        eng.close()


def test_rounds_are_cut_at_reads_and_give_the_same_bytes(corpus_engine, corpus_export):
    cp, eng = ac.corpus(), corpus_engine
    _, recs, body = corpus_export
    s0 = eng.stats()
    with pytest.raises(MlstError, match=r"too small: the records of one read may need \d+ bytes") as e:
        list(eng.export_sam_text(cp.idx, round_bytes=1))
    bound = int(re.search(r"may need (\d+) bytes", str(e.value)).group(1))
    chunks = list(eng.export_sam_text(cp.idx, round_bytes=bound))
    assert len(chunks) > 20 and b"".join(chunks) == body
    seen = set()
    for c in chunks:
        assert c.endswith(b"\n")
        names = set(l.split(b"\t", 1)[0] for l in c.splitlines())
        assert not names & seen, "a read's records sit in two rounds"
        seen |= names
    assert b"".join(eng.export_sam_text(cp.idx, round_bytes=4 * bound + 17)) == body
    with pytest.raises(MlstError, match="too small") as e2:
        list(eng.export_sam_text(cp.idx, round_bytes=bound - 1))
    assert "-5" in str(e2.value) or "may need %d bytes" % bound in str(e2.value)            # MLST_E_LIMIT
    s1 = eng.stats()
    fx.assert_stats_equal(s1, s0)
    assert np.array_equal(s1.counters, s0.counters)
    assert b"".join(eng.export_sam_text(cp.idx)) == body                                     # and an export still gives the file


# ------------------------------------------------------------------ pass 1 with the default parameters
def sample_reads(which, paired=False):
    """the corpus (every case of it; a paired submission holds whole pairs, so a copy of its last read closes the last pair) or a synth_sample"""
    if which != "corpus":
        return synth_sample(int(which))
    fb, fq, off = corpus_reads()
    if paired and (len(off) - 1) % 2:
        lo, hi = int(off[-2]), int(off[-1])
        fb, fq, off = np.concatenate((fb, fb[lo:hi])), np.concatenate((fq, fq[lo:hi])), np.concatenate((off, off[-1:] + np.uint64(hi - lo)))
    return ac.corpus().idx, (fb, fq, off)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("which", ["corpus", "150", "250"])
def test_the_file_accumulates_to_pass_one(tmp_path, which, paired):
    idx, (fb, fq, off) = sample_reads(which, paired)
    eng = make_engine(idx)                                                                   # default parameters: Q1 and min_read_len as they are
    try:
        eng.submit_reads(fb, fq, off, paired=paired)
        st = eng.stats()
        path = tmp_path / "s.all.sam"
        recs, body = export(eng, idx, path, paired=paired)
        assert len(recs) == int(st.counters[0]) > 100
        by_index, body_u = (recs, body) if not paired else export(eng, idx, tmp_path / "u.all.sam")      # read-index names: they say which mate a record belongs to
        assert_flag_and_xs(by_index)
        assert_rule_bytes(idx, by_index, body_u)
        ri = [r.ri for r in by_index]
        if paired:
            assert [l.split(b"\t", 1)[1] for l in body.splitlines()] == [l.split(b"\t", 1)[1] for l in body_u.splitlines()]
            assert [r.ri for r in recs] == [x >> 1 for x in ri]
            assert set(x >> 1 for x in ri if x % 2 == 0) & set(x >> 1 for x in ri if x % 2 == 1), "no pair with records of both mates"
        assert any(r.xs is not None for r in recs)
        if which == "corpus":
            assert any(r.xs is None for r in recs)                                           # (Q1: XO stands in the 15th column there)
        else:
            assert any(o & 15 == 1 for r in recs for o in r.ops) and any(o & 15 == 2 for r in recs for o in r.ops)
        orc = oracle_lib.Oracle(idx)
        so = orc.accumulate_records(ri, [r.a for r in recs], [r.tags["AS"] for r in recs], [r.tags["XM"] for r in recs], [r.tags["XO"] for r in recs],
                                    [len(r.seq) for r in recs])
        host = samin.AlignmentSample(idx, TypingArgs()).add_file(str(path)).stats()
        for name, s in (("oracle", so), ("host reader", host)):
            assert np.array_equal(s.sum_score, st.sum_score) and np.array_equal(s.n_hits, st.n_hits), name
            assert [int(x) for x in s.counters[:2]] == [int(x) for x in st.counters[:2]], name
            if not (paired and name == "oracle"):
                assert np.array_equal(s.locus_len_sum, st.locus_len_sum), name
        assert int(st.n_hits.sum()) > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ the export to the chosen alleles is a subset
@pytest.mark.parametrize("which", ["corpus", "150", "250"])
def test_the_records_of_the_chosen_alleles_are_the_chosen_export(tmp_path, which):
    idx, (fb, fq, off) = sample_reads(which)
    eng = make_engine(idx)
    try:
        eng.submit_reads(fb, fq, off)
        chosen = sorted(pick_alleles_fast(idx, eng.stats(), 100).values())
        recs, _ = export(eng, idx, tmp_path / "s.all.sam")
        aln = eng.export_alignments(chosen)
        want = {}
        for k in range(len(aln)):
            s0, s1 = int(aln.seq_off[k]), int(aln.seq_off[k + 1])
            key = (int(aln.read_index[k]), int(aln.flags[k]) & 1, int(aln.allele[k]), int(aln.pos0[k]))
            val = (int(aln.as_[k]), int(aln.xm[k]), [int(o) for o in aln.cigar[int(aln.cigar_off[k]):int(aln.cigar_off[k + 1])]], aln.seq[s0:s1].tobytes(),
                   bytes(min(int(q), 93) + 33 for q in aln.qual[s0:s1]))
            want.setdefault(key, []).append(val)
        got = {}
        for r in recs:
            if r.a in chosen:
                got.setdefault((r.ri, (r.flag >> 4) & 1, r.a, r.pos0), []).append((r.tags["AS"], r.tags["XM"], r.ops, r.seq, r.qual))
        assert len(aln) > 0 and sorted(got) == sorted(want)
        for key in want:
            assert sorted(got[key]) == sorted(want[key]), key
    finally:
        eng.close()


# ------------------------------------------------------------------ the sample's state, the refusals
def test_an_export_changes_nothing_of_the_sample(tmp_path):
    idx, (fb, fq, off) = synth_sample(150)
    eng = make_engine(idx)
    nb, nr, done = (C.c_uint64(), C.c_uint64(), C.c_int())

    def nxt():
        return eng.lib.mlst_alignments_text_next(eng._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done))
    try:
        assert list(eng.export_sam_text(idx)) == []                                          # before any submission
        with pytest.raises(MlstError, match="no export is open"):
            eng._check(nxt(), "mlst_alignments_text_next")
        eng.submit_reads(fb, fq, off)
        s0 = eng.stats()
        chosen = sorted(pick_alleles_fast(idx, s0, 100).values())
        p0 = eng.pileup(chosen)
        a0 = eng.export_alignments(chosen)
        eng.typing_enqueue(penalty=100)
        body = b"".join(eng.export_sam_text(idx))                                            # between enqueue and fetch
        st, dev_chosen, letters = eng.typing_fetch()
        assert sorted(dev_chosen.values()) == chosen and body.count(b"\n") == int(s0.counters[0]) > 0
        fx.assert_stats_equal(st, s0)
        p1 = eng.pileup(chosen)
        assert all(np.array_equal(p0[a], p1[a]) for a in chosen)
        s1 = eng.stats()
        fx.assert_stats_equal(s1, s0)
        assert np.array_equal(s1.counters, s0.counters)
        a1 = eng.export_alignments(chosen)
        assert len(a1) == len(a0) and np.array_equal(np.sort(a1.as_), np.sort(a0.as_))
        assert b"".join(eng.export_sam_text(idx)) == body                                    # and the export itself repeats
        eng.typing_enqueue(penalty=100)
        assert eng.typing_fetch()[1] == dev_chosen
        # cap smaller than the round; the export stays open and can go on
        names = [idx.label(a).encode() for a in range(idx.n_alleles)]
        noff = np.zeros(len(names) + 1, np.uint64); noff[1:] = np.cumsum([len(x) for x in names])
        flat = np.frombuffer(b"".join(names), np.uint8)
        eng._check(eng.lib.mlst_alignments_text_open(eng._h, _ptr(flat), _ptr(noff), 0, 0), "mlst_alignments_text_open")
        eng._check(nxt(), "mlst_alignments_text_next")
        assert nb.value == len(body) and nr.value == body.count(b"\n") and done.value == 0
        small = np.zeros(16, np.uint8)
        with pytest.raises(MlstError, match="smaller than the round"):
            eng._check(eng.lib.mlst_alignments_text_next(eng._h, _ptr(small), 16, C.byref(nb), C.byref(nr), C.byref(done)), "mlst_alignments_text_next")
        big = np.zeros(len(body), np.uint8)
        eng._check(eng.lib.mlst_alignments_text_next(eng._h, _ptr(big), len(big), C.byref(nb), C.byref(nr), C.byref(done)), "mlst_alignments_text_next")
        assert big.tobytes() == body and done.value == 1
        eng._check(eng.lib.mlst_alignments_text_close(eng._h), "mlst_alignments_text_close")
        with pytest.raises(MlstError, match="no export is open"):
            eng._check(nxt(), "mlst_alignments_text_next")
        # a stream of ready-made alignments is open: refused
        eng.reset_sample()
        eng.bam_open(1, *samin.bam_ref_table(idx, [idx.label(a) for a in range(idx.n_alleles)], None), skip_bytes=0)
        with pytest.raises(MlstError, match="BAM stream is open"):
            list(eng.export_sam_text(idx))
        eng.reset_sample()
        # no read on a locus: a header-only file
        from metamlst_amd import synth
        rnd = np.random.default_rng(3).choice(list(b"ACGT"), size=(200, 150)).astype(np.uint8)
        eng.submit_reads(*synth.flatten_reads(rnd, np.full_like(rnd, ord("I"))))
        p = tmp_path / "none.all.sam"
        assert samout.write_sam_all(str(p), idx, eng, False) == 0
        lines = open(p).read().splitlines()
        assert all(l.startswith("@") for l in lines) and len(lines) == 2 + idx.n_alleles
    finally:
        eng.close()


# ------------------------------------------------------------------ end to end
def test_cli_write_sam_all_types_to_the_same_nfo_through_both_readers(tmp_path):
    db, idx = fx.ecoli_small(40, 5)
    _, (fb, fq, off) = synth_sample(150)
    fastq = tmp_path / "small.fastq"
    with open(fastq, "wb") as f:
        for k in range(len(off) - 1):
            f.write(b"@x%d\n%s\n+\n%s\n" % (k, fb[int(off[k]):int(off[k + 1])].tobytes(), fq[int(off[k]):int(off[k + 1])].tobytes()))
    tail = ["-d", db.path, "--quiet", "--min_accuracy", "0", "--nloci", "0"]                 # (the .nfo is written whatever the coverage)
    assert cli.main(["type", str(fastq)] + tail + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(["type", str(fastq)] + tail + ["-o", str(tmp_path / "all"), "--write-sam-all"]) == 0
    assert cli.main(["type", str(fastq)] + tail + ["-o", str(tmp_path / "both"), "--write-sam-all", "--write-sam"]) == 0
    assert os.listdir(tmp_path / "plain") == ["small.nfo"] and sorted(os.listdir(tmp_path / "all")) == ["small.all.sam", "small.nfo"]
    assert sorted(os.listdir(tmp_path / "both")) == ["small.all.sam", "small.nfo", "small.sam"]
    nfo = open(tmp_path / "plain" / "small.nfo", "rb").read()
    assert nfo == open(tmp_path / "all" / "small.nfo", "rb").read() == open(tmp_path / "both" / "small.nfo", "rb").read() and len(nfo) > 0
    assert open(tmp_path / "all" / "small.all.sam", "rb").read() == open(tmp_path / "both" / "small.all.sam", "rb").read()
    sam = tmp_path / "in" / "small.all.sam"
    os.makedirs(sam.parent)
    os.replace(tmp_path / "all" / "small.all.sam", sam)
    assert cli.main(["type", str(sam), "--alignments"] + tail + ["-o", str(tmp_path / "dev")]) == 0      # the device SAM path
    assert open(tmp_path / "dev" / "small.nfo", "rb").read() == nfo
    # the host reader forced: SAM text without @SQ lines gives the device no names, so the command reads it on the host
    bare = tmp_path / "bare" / "small.all.sam"
    os.makedirs(bare.parent)
    with open(sam, "rb") as f, open(bare, "wb") as g:
        g.writelines(l for l in f if not l.startswith(b"@SQ"))
    assert not samin.read_sam_header(str(bare))
    assert cli.main(["type", str(bare), "--alignments"] + tail + ["-o", str(tmp_path / "host")]) == 0
    assert open(tmp_path / "host" / "small.nfo", "rb").read() == nfo
