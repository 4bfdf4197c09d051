"""mlst_alignments_export / mlst_alignments_fetch (csrc/aln_export.h) and `cli type --write-sam`: the exported records against the
pile-up they restate, the oracle's align_one, the item list, pass 1 and the two SAM readers.

Check (d) -- the sum of AS and the count of the records that pass minscore / max_xM equal pass 1's sum_score / n_hits of the chosen
alleles -- is the pile-up's tag filter against pass 1's accept test (metamlst.py:115).  The two are the same test only where pass 1
reads XM from the 15th column and asks for no read length: quirk Q1 puts XO there for a read with one record, and a read under
min_read_len is never accepted.  So (d) runs on an engine with xm_field_quirk = 0 and min_read_len = 1 (PLAIN); everything else
runs with the default parameters as well."""
import functools
import os

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
import samin_ref
from metamlst_amd import cli, samin, samout, synth
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.typing import TypingArgs, pick_alleles_fast

pytestmark = pytest.mark.gpu

CAP = 1 << 16
PLAIN = {"xm_field_quirk": 0, "min_read_len": 1}


def params_of(over):
    p = default_params()
    for k, v in over.items():
        setattr(p, k, v)
    return p


def make_engine(idx, over=None):
    eng = Engine(0, params_of(over or {}))
    eng.load_reference(idx)
    return eng


@functools.lru_cache(maxsize=None)
def corpus_reads():
    """(bases, quals, off): every group of align_cases in one submission, then two reads of locus `plain` with a planted 3-base
    insertion / deletion (the corpus' own indel reads are 1, 2, 3, 7, 8 and 9 bases; the oracle says which kinds it yields: (e))."""
    cp = ac.corpus()
    a = cp.allele("plain", 13); s = cp.seq(a)
    extra = [s[200:275] + b"GAT" + s[275:347], s[200:275] + s[278:353]]
    reads = [c.bases for c in cp.cases] + extra
    quals = [c.quals for c in cp.cases] + [b"I" * len(r) for r in extra]
    return synth.ragged_reads(reads, quals)


def cigar_of(aln, k):
    return [(int(o) >> 4, int(o) & 15) for o in aln.cigar[int(aln.cigar_off[k]):int(aln.cigar_off[k + 1])]]


def pairs_of(ops, pos0):
    """(oriented read position, allele column) of every M column of a CIGAR"""
    out, i, j = [], 0, pos0
    for ln, op in ops:
        if op == 0:
            out += [(i + t, j + t) for t in range(ln)]; i += ln; j += ln
        elif op in (1, 4):
            i += ln
        elif op == 2:
            j += ln
        else:
            raise AssertionError("operation %d in an exported CIGAR" % op)
    return out


def assert_well_formed(aln, idx):
    n = len(aln)
    assert len(aln.cigar_off) == n + 1 == len(aln.seq_off) and int(aln.cigar_off[0]) == 0 == int(aln.seq_off[0])
    assert int(aln.cigar_off[-1]) == len(aln.cigar) and int(aln.seq_off[-1]) == len(aln.seq) == len(aln.qual)
    assert np.all(np.diff(aln.cigar_off.astype(np.int64)) >= 1) and np.all((aln.cigar >> 4) > 0) and np.all(np.isin(aln.cigar & 15, (0, 1, 2, 4)))
    assert np.all(np.isin(aln.seq, np.frombuffer(b"ACGTN", np.uint8))) and np.all(aln.qual < 128) and np.all(aln.flags < 4)
    for k in range(n):                                                     # the bases of a CIGAR are the read's
        ops = cigar_of(aln, k)
        assert sum(ln for ln, op in ops if op in (0, 1, 4)) == int(aln.seq_off[k + 1] - aln.seq_off[k]), k
        assert all(op != ops[t + 1][1] for t, (_, op) in enumerate(ops[:-1])), (k, ops)      # runs are maximal


def assert_pileup_round_trip(eng, chosen, aln):
    want, got = eng.pileup(chosen), eng.pileup_alignments(chosen, *aln.pileup_arrays())
    for a in chosen:
        assert np.array_equal(got[a], want[a]), "the exported records pile up differently on allele %d" % a
    return want


def assert_pass1_sums(eng, idx, chosen, aln, minscore=80, max_xm=5):
    st = eng.stats()
    ok = (aln.as_ >= minscore) & (aln.xm <= max_xm)
    for a in chosen:
        m = ok & (aln.allele == a)
        assert (int(aln.as_[m].sum()), int(m.sum())) == (int(st.sum_score[a]), int(st.n_hits[a])), "allele %d" % a


def same_arrays(a, b):
    """two exports as the same SET of records (the order is unspecified): keyed by (read, allele, strand, diag)"""
    def keyed(x):
        return {(int(x.read_index[k]), int(x.allele[k]), int(x.flags[k]), int(x.diag[k])):
                (int(x.pos0[k]), int(x.as_[k]), int(x.xm[k]), tuple(cigar_of(x, k)), x.seq[int(x.seq_off[k]):int(x.seq_off[k + 1])].tobytes(),
                 x.qual[int(x.seq_off[k]):int(x.seq_off[k + 1])].tobytes()) for k in range(len(x))}
    ka, kb = keyed(a), keyed(b)
    return len(ka) == len(a) and ka == kb


# ------------------------------------------------------------------ 1. the crafted corpus
@pytest.fixture(scope="module")
def corpus_engine():
    eng = make_engine(ac.corpus().idx)
    fb, fq, off = corpus_reads()
    eng.submit_reads(fb, fq, off)
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def corpus_oracle():
    cp = ac.corpus()
    orc = oracle_lib.Oracle(cp.idx)
    orc.submit_reads(*corpus_reads())
    return orc, orc.stats()


def corpus_choices(eng):
    cp = ac.corpus()
    tail = sorted(pick_alleles_fast(cp.idx, eng.stats(), 100).values())
    first = [int(cp.idx.locus_begin[l]) for l in range(cp.idx.n_loci)]
    assert tail != first
    return {"tail": tail, "first": first}


@pytest.mark.parametrize("choice", ["tail", "first"])
def test_corpus_records_equal_the_pileup_the_oracle_and_the_items(corpus_engine, choice):
    cp, eng = ac.corpus(), corpus_engine
    fb, fq, off = corpus_reads()
    orc, so = corpus_oracle()
    fx.assert_stats_equal(eng.stats(), so)
    chosen = corpus_choices(eng)[choice]
    aln = eng.export_alignments(chosen)
    assert_well_formed(aln, cp.idx)
    assert_pileup_round_trip(eng, chosen, aln)                                                  # (a)
    by_locus = {int(cp.idx.locus_id[a]): a for a in chosen}
    got = {}
    for k in range(len(aln)):
        key = (int(aln.read_index[k]), int(aln.flags[k]) & 1, int(aln.diag[k]), int(aln.allele[k]))
        assert key not in got, "record exported twice: %s" % (key,)
        got[key] = k
    want, kinds = set(), set()
    for ri, loc, strand, diag, votes in eng.items(CAP).tolist():
        if loc not in by_locus:
            continue
        a = by_locus[loc]
        b, q = fb[int(off[ri]):int(off[ri + 1])].tobytes(), fq[int(off[ri]):int(off[ri + 1])].tobytes()
        n, m = len(b), int(cp.idx.off[a + 1] - cp.idx.off[a])
        r = orc.align_one(b, q, a, strand, diag)
        if not (r["score"] >= ac.floor_score(n) and r["score"] > 0):
            continue
        want.add((ri, strand, diag, a))
        k = got.get((ri, strand, diag, a))
        if k is None:
            continue                                                                            # (reported by (c) below)
        ops = cigar_of(aln, k)
        assert (int(aln.as_[k]), int(aln.xm[k]), int(aln.flags[k]) >> 1) == (r["score"], r["xm"], r["used_dp"]), (ri, strand, diag, a)      # (b)
        assert pairs_of(ops, int(aln.pos0[k])) == r["cols"] and int(aln.pos0[k]) == min(j for _, j in r["cols"]), (ri, strand, diag, a, ops)
        if r["used_dp"] == 0:
            assert int(aln.pos0[k]) == r["cols"][0][0] + diag
        # SEQ / QUAL are the oriented read
        sq = aln.seq[int(aln.seq_off[k]):int(aln.seq_off[k + 1])].tobytes(); ql = aln.qual[int(aln.seq_off[k]):int(aln.seq_off[k + 1])].tobytes()
        assert sq == (ac.rc(b) if strand else b) and ql == bytes(x - 33 for x in (q[::-1] if strand else q)), (ri, strand)
        kinds |= {"I" if op == 1 else "D" for _, op in ops if op in (1, 2)}
        kinds |= {"lead%d" % strand} if ops[0][1] == 4 else set()
        kinds |= {"trail%d" % strand} if ops[-1][1] == 4 else set()
        kinds |= ({"over_start"} if diag < 0 else set()) | ({"over_end"} if diag + n > m else set())
        kinds |= {"tag_filter"} if (r["score"] < 80 or r["xm"] > 5) else set()
        kinds |= ({"N"} if b"N" in b else set()) | ({"n36"} if n == 36 else set()) | ({"n320"} if n == 320 else set())
        kinds |= {"I3"} if (3, 1) in ops else set()
        kinds |= {"D3"} if (3, 2) in ops else set()
    assert set(got) == want, "missing %s, extra %s" % (sorted(want - set(got))[:5], sorted(set(got) - want)[:5])      # (c)
    assert kinds >= {"I", "D", "lead0", "lead1", "trail0", "trail1", "over_start", "over_end", "tag_filter", "N", "n36", "n320", "I3", "D3"}, kinds      # (e)


@pytest.mark.parametrize("choice", ["tail", "first"])
def test_corpus_records_that_pass_the_tag_filter_sum_to_pass_one(choice):
    cp = ac.corpus()
    eng = make_engine(cp.idx, PLAIN)
    try:
        eng.submit_reads(*corpus_reads())
        chosen = corpus_choices(eng)[choice]
        aln = eng.export_alignments(chosen)
        assert_pileup_round_trip(eng, chosen, aln)                                              # (a)
        assert_pass1_sums(eng, cp.idx, chosen, aln)                                             # (d)
        assert int(((aln.as_ < 80) | (aln.xm > 5)).sum()) > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. both row widths
@functools.lru_cache(maxsize=None)
def synth_sample(read_len):
    """a few thousand reads of an isolate of the small fixture database (one allele in five with a deletion), a 2-base deletion or
    insertion planted into every seventh / eleventh read"""
    db, idx = fx.ecoli_small(40, 5)
    fb, fq, off, _, _ = fx.isolate_reads(db, "ecoli", 3, n_reads=3000, genome=40_000, read_len=read_len)
    rng = np.random.default_rng(read_len)
    reads, quals = [], []
    for k in range(len(off) - 1):
        b, q = fb[int(off[k]):int(off[k + 1])].tobytes(), fq[int(off[k]):int(off[k + 1])].tobytes()
        mid = len(b) // 2
        if k % 7 == 0:
            b, q = b[:mid] + b[mid + 2:], q[:mid] + q[mid + 2:]
        elif k % 11 == 0:
            b, q = b[:mid] + bytes(rng.choice(list(b"ACGT"), size=2).astype(np.uint8)) + b[mid:-2], q
        reads.append(b); quals.append(q)
    return idx, synth.ragged_reads(reads, quals)


@pytest.mark.parametrize("read_len", [150, 250])
def test_both_row_widths(read_len):
    idx, (fb, fq, off) = synth_sample(read_len)
    assert (int(np.diff(off.astype(np.int64)).max()) <= 160) == (read_len == 150)
    eng = make_engine(idx, PLAIN)
    try:
        eng.submit_reads(fb, fq, off)
        chosen = sorted(pick_alleles_fast(idx, eng.stats(), 100).values())
        assert len(chosen) == 7
        aln = eng.export_alignments(chosen)
        assert_well_formed(aln, idx)
        assert len(aln) > 100 and int((aln.flags >> 1).sum()) > 0 and np.any((aln.cigar & 15) == 1) and np.any((aln.cigar & 15) == 2)
        assert_pileup_round_trip(eng, chosen, aln)                                              # (a)
        assert_pass1_sums(eng, idx, chosen, aln)                                                # (d)
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. paired
def test_paired_submission_exports_the_same_records_and_mates_share_a_name(tmp_path):
    idx, (fb, fq, off) = synth_sample(150)
    eng = make_engine(idx)
    try:
        eng.submit_reads(fb, fq, off)
        chosen = sorted(pick_alleles_fast(idx, eng.stats(), 100).values())
        single = eng.export_alignments(chosen)
        eng.reset_sample()
        eng.submit_reads(fb, fq, off, paired=True)
        paired = eng.export_alignments(chosen)
        assert len(single) > 0 and same_arrays(single, paired)
        p = str(tmp_path / "p.sam")
        samout.write_sam(p, idx, chosen, paired, True)
        names = [l.split("\t")[0] for l in open(p) if not l.startswith("@")]
        assert sorted(names) == sorted("r%d" % (int(r) >> 1) for r in paired.read_index)
        ri = set(int(r) for r in paired.read_index)
        both = [r for r in ri if r % 2 == 0 and r + 1 in ri]
        assert both and all(names.count("r%d" % (r >> 1)) >= 2 for r in both)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. the sample's state
def test_an_export_changes_nothing_of_the_sample(tmp_path):
    idx, (fb, fq, off) = synth_sample(150)
    eng = make_engine(idx)
    try:
        assert len(eng.export_alignments([0])) == 0                                             # before any submission
        with pytest.raises(MlstError, match="two chosen alleles"):
            eng.export_alignments([0, 1])                                                       # two alleles of one locus
        with pytest.raises(MlstError, match="no finished export"):                              # a refused export leaves none behind
            eng._check(eng.lib.mlst_alignments_fetch(eng._h, *([None] * 12)), "mlst_alignments_fetch")
        eng.submit_reads(fb, fq, off)
        s0 = eng.stats()
        chosen = sorted(pick_alleles_fast(idx, s0, 100).values())
        p0 = eng.pileup(chosen)
        eng.typing_enqueue(penalty=100)
        aln = eng.export_alignments(chosen)                                                     # between enqueue and fetch
        st, dev_chosen, letters = eng.typing_fetch()
        assert sorted(dev_chosen.values()) == chosen and len(aln) > 0
        fx.assert_stats_equal(st, s0)
        p1 = eng.pileup(chosen)
        assert all(np.array_equal(p0[a], p1[a]) for a in chosen)
        s1 = eng.stats()
        fx.assert_stats_equal(s1, s0)
        assert np.array_equal(s1.counters, s0.counters)
        assert same_arrays(aln, eng.export_alignments(chosen))                                  # and the export itself repeats
        # a stream of ready-made alignments is open: refused
        eng.reset_sample()
        names = [idx.label(a) for a in range(idx.n_alleles)]
        eng.bam_open(1, *samin.bam_ref_table(idx, names, None), skip_bytes=0)
        with pytest.raises(MlstError, match="BAM stream is open"):
            eng.export_alignments(chosen)
        eng.reset_sample()
        # no read on a locus: a header-only file
        rnd = np.random.default_rng(3).choice(list(b"ACGT"), size=(200, 150)).astype(np.uint8)
        eng.submit_reads(*synth.flatten_reads(rnd, np.full_like(rnd, ord("I"))))
        none = eng.export_alignments(chosen)
        assert len(none) == 0 and len(none.cigar) == 0 and len(none.seq) == 0
        p = str(tmp_path / "none.sam")
        samout.write_sam(p, idx, chosen, none, False)
        assert all(l.startswith("@") for l in open(p)) and sum(1 for _ in open(p)) == 2 + len(chosen)
    finally:
        eng.close()


def test_a_fetch_without_an_export_is_refused():
    eng = make_engine(fx.ecoli_small(40, 5)[1])
    try:
        with pytest.raises(MlstError, match="no finished export"):
            eng._check(eng.lib.mlst_alignments_fetch(eng._h, *([None] * 12)), "mlst_alignments_fetch")
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. end to end
def test_cli_write_sam_round_trips_through_both_sam_readers(tmp_path):
    db, idx = fx.ecoli_small(40, 5)
    _, (fb, fq, off) = synth_sample(150)
    fastq = tmp_path / "small.fastq"
    with open(fastq, "wb") as f:
        for k in range(len(off) - 1):
            f.write(b"@x%d\n%s\n+\n%s\n" % (k, fb[int(off[k]):int(off[k + 1])].tobytes(), fq[int(off[k]):int(off[k + 1])].tobytes()))
    base = ["type", str(fastq), "-d", db.path, "--quiet", "--min_accuracy", "0", "--nloci", "0"]      # (the .nfo is written whatever the coverage)
    assert cli.main(base + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(base + ["-o", str(tmp_path / "sam"), "--write-sam"]) == 0
    assert os.listdir(tmp_path / "plain") == ["small.nfo"] and sorted(os.listdir(tmp_path / "sam")) == ["small.nfo", "small.sam"]
    assert open(tmp_path / "plain" / "small.nfo", "rb").read() == open(tmp_path / "sam" / "small.nfo", "rb").read()
    sam = str(tmp_path / "sam" / "small.sam")
    eng = make_engine(idx)
    try:
        eng.submit_reads(fb, fq, off)
        eng.typing_enqueue(penalty=100)
        _, dev_chosen, _ = eng.typing_fetch()
        chosen = [dev_chosen[l] for l in sorted(dev_chosen)]
        assert [l.rstrip("\n") for l in open(sam) if l.startswith("@SQ")] == ["@SQ\tSN:%s\tLN:%d" % (idx.label(a), len(idx.sequence(a))) for a in chosen]
        want = eng.pileup(chosen)
        targs = TypingArgs()
        host = samin.AlignmentSample(idx, targs).add_file(sam)
        assert len(host._rec) == len(eng.export_alignments(chosen)) > 0
        got_host = host.pileup(eng, chosen)
        lit = samin_ref.pileup_python(idx, host, chosen)
        eng2 = make_engine(idx)
        try:
            got_dev = samin.SamSample(idx, targs, eng2).add_file(sam).pileup(eng2, chosen)
        finally:
            eng2.close()
        for a in chosen:
            assert np.array_equal(got_host[a], want[a]) and np.array_equal(lit[a], want[a]) and np.array_equal(got_dev[a], want[a]), a
    finally:
        eng.close()
