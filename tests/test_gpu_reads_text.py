"""mlst_reads_text_open / _next / _close (csrc/reads_text.h), Engine.export_reads_text, samout.write_reads and `cli type --write-reads`:
the reads that have an alignment as FASTQ text formatted on the device, byte for byte against samout.reads_fastq_rule.

Which reads are written is decided by the ORACLE, not by a device export: orc_pass1_dense gives, per read and allele, the best score
align_pair reaches over the read's work items, so a read has a record iff its best score over all alleles is >= the floor of its
length and > 0 (`aligned_by_oracle`).  The agreement with the full export on the same engine is a test of its own."""
import atexit
import ctypes as C
import functools
import os
import re
import shutil
import sqlite3
import tempfile

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
import read_names_cases as rc
from metamlst_amd import cli, samin, samout, synth
from metamlst_amd.engine import MlstError, _ptr
from metamlst_amd.fastq import prep_fastq, trim_adapters
from metamlst_amd.index import load_index
from test_gpu_align_export import CAP, corpus_oracle, corpus_reads, make_engine, synth_sample

pytestmark = pytest.mark.gpu

FQT_GROUP = 1024                                  # csrc/fastq_tile.h: entries per workgroup of the offsets' scan
LIMIT = r"too small: the text and the tables of one read may need (\d+) bytes"
_TMP = tempfile.mkdtemp(prefix="mlst_reads_text_")
atexit.register(shutil.rmtree, _TMP, True)


# ------------------------------------------------------------------ the yardstick
def aligned_by_oracle(idx, fb, fq, off) -> list:
    """the reads (0-based in the submission) with at least one record: the oracle's seeded pass over every read"""
    orc = oracle_lib.Oracle(idx)
    orc.submit_reads(fb, fq, off)
    sc, _, _ = orc.pass1_dense()
    best = sc.max(axis=1).astype(np.int64)
    n = np.diff(np.asarray(off).astype(np.int64))
    return [k for k in range(len(n)) if n[k] > 0 and best[k] > 0 and best[k] >= ac.floor_score(int(n[k]))]


def reads_map(fb, fq, off, base: int = 0) -> dict:
    """{read index: (bases, raw Phred)} of a submission (qualities arrive as Phred + 33)"""
    return {base + k: (fb[int(off[k]):int(off[k + 1])].tobytes(), bytes(max(0, min(int(x) - 33, 127)) for x in fq[int(off[k]):int(off[k + 1])]))
            for k in range(len(off) - 1)}


def rule_bytes(idx, flat, paired=False, names=None, base: int = 0) -> bytes:
    fb, fq, off = flat
    return b"".join(samout.reads_fastq_rule(reads_map(fb, fq, off, base), [base + k for k in aligned_by_oracle(idx, fb, fq, off)], paired, names))


def flat_of_text(text: bytes):
    recs = rc.fastq_records(text)
    return synth.ragged_reads([s for _, s, _ in recs], [q for _, _, q in recs])


def names_of_text(texts, interleave=False) -> dict:
    """{read index: kept name} of every read of the texts with a legal name (a superset of the retained ones does no harm)"""
    heads = rc.yardstick(texts, interleave=interleave)
    return rc.kept(heads, list(heads))


def planted(idx, a: int, at: int, n: int, strand: int = 0) -> bytes:
    s = idx.sequence(a).upper().encode()[at:at + n]
    assert len(s) == n
    return ac.rc(s) if strand else s


def export(eng, paired=False, round_bytes=0) -> bytes:
    return b"".join(eng.export_reads_text(paired=paired, round_bytes=round_bytes))


def records_of(body: bytes) -> list:
    """[(name, SEQ, QUAL)] of FASTQ text, its shape checked"""
    lines = body.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    out = []
    for k in range(0, len(lines) - 1, 4):
        assert lines[k][:1] == b"@" and lines[k + 2] == b"+" and len(lines[k + 1]) == len(lines[k + 3]) and re.fullmatch(rb"[ACGTN]*", lines[k + 1])
        out.append((lines[k][1:], lines[k + 1], lines[k + 3]))
    return out


# ------------------------------------------------------------------ 1. the crafted corpus
@pytest.fixture(scope="module")
def corpus_engine():
    eng = make_engine(ac.corpus().idx)
    eng.submit_reads(*corpus_reads())
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def corpus_rule(base: int = 0) -> bytes:
    return rule_bytes(ac.corpus().idx, corpus_reads(), base=base)


def test_corpus_bytes_are_the_rule_whatever_the_rounds(corpus_engine):
    eng = corpus_engine
    _, so = corpus_oracle()
    fx.assert_stats_equal(eng.stats(), so)
    want = corpus_rule()
    n_want = want.count(b"\n") // 4
    assert n_want > 100 and n_want < len(corpus_reads()[2]) - 1                           # some reads of the corpus have no record
    assert export(eng) == want
    with pytest.raises(MlstError, match=LIMIT) as e:
        export(eng, round_bytes=1)
    bound = int(re.search(LIMIT, str(e.value)).group(1))
    chunks = list(eng.export_reads_text(round_bytes=bound))                              # the smallest value the planner accepts
    assert b"".join(chunks) == want and len(chunks) > 20 and all(c.endswith(b"\n") and c.count(b"\n") % 4 == 0 for c in chunks)
    few = list(eng.export_reads_text(round_bytes=4 * bound + 17))                        # a handful of reads per round
    assert b"".join(few) == want and 1 < len(few) < len(chunks)
    with pytest.raises(MlstError, match=LIMIT) as e2:
        export(eng, round_bytes=bound - 1)
    assert "may need %d bytes" % bound in str(e2.value) and "-5" in str(e2.value)        # MLST_E_LIMIT
    assert samout.write_reads(os.path.join(_TMP, "corpus.fastq"), eng, False) == n_want
    assert open(os.path.join(_TMP, "corpus.fastq"), "rb").read() == want


# ------------------------------------------------------------------ 2. agreement with the full export
def test_names_seq_and_qual_agree_with_the_full_export(corpus_engine):
    eng, idx = corpus_engine, ac.corpus().idx
    fq = {name: (seq, qual) for name, seq, qual in records_of(export(eng))}
    sam = b"".join(eng.export_sam_text(idx))
    seen, strands = set(), set()
    for line in sam.splitlines():
        f = line.split(b"\t")
        name, flag, seq, qual = f[0], int(f[1]), f[9], f[10]
        assert name in fq, name
        seen.add(name); strands.add(flag & 16)
        if flag & 16:
            assert (ac.rc(seq), qual[::-1]) == fq[name], name
        else:
            assert (seq, qual) == fq[name], name
    assert seen == set(fq) and strands == {0, 16}


# ------------------------------------------------------------------ 3. edges of the writer
LENGTHS = [50, 51, 52, 53, 54, 63, 64, 65, 127, 128, 129, 160, 161, 319, 320]      # (54: with it the sample of reads up to 160 bases meets all 16 residue pairs)
NAME_LENS = [1, 2, 3, 4, 5, 254]


def writer_text(idx, lengths) -> bytes:
    """one read per (length, name length): planted on an allele, both strands, varied qualities; every third name is one the rule
    refuses (an inner `@`), so r<k> of varying width stands between the kept names"""
    out, k = [], 0
    letters = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
    for n in lengths:
        for nl in NAME_LENS:
            a = (7 * k) % idx.n_alleles
            seq = planted(idx, a, (3 * k) % 40, n, k & 1)
            qual = bytes(33 + (k + 5 * t) % 61 for t in range(n))
            name = bytes(letters[(k + t) % len(letters)] for t in range(nl))
            if (k // len(NAME_LENS) + k) % 3 == 2:
                name = name[:nl // 2] + b"@" + name[nl // 2 + 1:]                      # no legal QNAME: the read keeps r<k>
            out.append(b"@" + name + b" d\n" + seq + b"\n+\n" + qual + b"\n")
            k += 1
    return b"".join(out)


@pytest.mark.parametrize("wide", [False, True], ids=["160", "320"])
def test_every_head_and_tail_of_the_copy_at_every_destination_residue(wide):
    idx = fx.ecoli_small(8)[1]
    lengths = LENGTHS if wide else [n for n in LENGTHS if n <= 160]
    text = writer_text(idx, lengths)
    eng = make_engine(idx)
    try:
        eng.set_read_names(True)
        assert eng.submit_fastq(text) == len(lengths) * len(NAME_LENS)
        got = export(eng)
        names = names_of_text([text])
        want = rule_bytes(idx, flat_of_text(text), names=names)
        assert got == want
        recs = records_of(got)
        assert len(recs) == len(lengths) * len(NAME_LENS), "a planted read is missing from the rule's own set"
        assert max(len(s) for _, s, _ in recs) == (320 if wide else 160)
        assert {len(n) for n, _, _ in recs} >= {1, 2, 3, 4, 5, 254} and any(re.fullmatch(rb"r\d+", n) for n, _, _ in recs)
        # the copies: (destination address mod 4, bytes mod 4) of SEQ and of QUAL -- head = (4 - address) & 3, tail = (n - head) & 3
        met, at = set(), 0
        for name, seq, _ in recs:
            n = len(seq)
            met |= {((at + len(name) + 2) & 3, n & 3), ((at + len(name) + 5 + n) & 3, n & 3)}
            at += 2 * n + len(name) + 6
        assert at == len(got) and met == {(d, t) for d in range(4) for t in range(4)}, sorted(met)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. edges of the marker
@functools.lru_cache(maxsize=None)
def marker_index():
    """locus `big`: 129 alleles that share their first 100 columns' ancestry and are unrelated behind them, so a read from columns
    100.. of one allele has a record with that allele alone; locus `small`: 8 ordinary alleles"""
    path = os.path.join(_TMP, "marker.db")
    for p in (path, path + ".mlstidx"):
        if os.path.exists(p):
            os.remove(p)
    synth.make_db(path, {"spM": [("big", 300), ("small", 300)]}, {("spM", "big"): 129, ("spM", "small"): 8}, n_profiles=4, seed=911)
    rng = np.random.default_rng(912)
    conn = sqlite3.connect(path)
    for rid, s in list(conn.execute("SELECT recID, sequence FROM alleles WHERE gene='big'")):
        s2 = s[:100] + bytes(rng.choice(list(b"ACGT"), size=200).astype(np.uint8)).decode()
        conn.execute("UPDATE alleles SET sequence=?, alignedSequence=? WHERE recID=?", (s2, s2, rid))
    conn.commit()
    conn.close()
    return load_index(path, cache=False)


def mutated_behind_a_seed(idx, a: int, at: int, n: int = 60) -> bytes:
    """20 bases of the allele (one seed), then n - 20 bases that all differ from it: 40 points, under the floor of 60 bases (52)"""
    s = planted(idx, a, at, n)
    return s[:20] + bytes(ac.other_base(c) for c in s[20:])


def test_the_marker_finds_a_record_at_every_turn_edge_and_nothing_else():
    idx = marker_index()
    big, small = idx.locus_index("spM", "big"), idx.locus_index("spM", "small")
    b0, s0 = int(idx.locus_begin[big]), int(idx.locus_begin[small])
    assert int(idx.locus_count[big]) == 129
    rng = np.random.default_rng(5)
    noise = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    bad = bytearray(planted(idx, b0 + 20, 120, 60))
    for p in range(22, 60, 7):                                                           # a seed, then six mismatches: AS under --minscore 80
        bad[p] = ac.other_base(bad[p])
    with_n = bytearray(planted(idx, b0 + 30, 125, 150)); with_n[75] = ord("N")
    reads = [planted(idx, b0 + 63, 120, 150),            # 0: its only record is the 64th pair of the walk: the last lane of the first turn
             noise(150),                                 # 1: off the loci
             planted(idx, b0 + 64, 110, 150, 1),         # 2: the 65th: the first lane of the second turn
             planted(idx, b0 + 127, 130, 150),           # 3: the 128th
             planted(idx, b0 + 128, 105, 150, 1),        # 4: the 129th: a third turn with one lane
             planted(idx, b0, 120, 150),                 # 5: the first
             mutated_behind_a_seed(idx, b0 + 10, 150),   # 6: retained (a seed of the allele) and without a record
             bytes(bad),                                 # 7: every record fails the AS / XM filter
             planted(idx, s0 + 3, 40, 100),              # 8: an ordinary read: a record with every allele of its locus
             bytes(with_n),                              # 9: an N, and qualities past 93
             mutated_behind_a_seed(idx, s0 + 1, 200)]    # 10: as 6, the last read of the sample
    quals = [b"I" * len(r) for r in reads]
    quals[9] = bytes(33 + (60 + t) % 128 for t in range(150))
    flat = synth.ragged_reads(reads, quals)
    # the construction is what it says: the oracle's records per read
    orc = oracle_lib.Oracle(idx)
    orc.submit_reads(*flat)
    sc = orc.pass1_dense()[0]
    hits = [sorted(int(a) for a in np.nonzero(sc[k] >= max(1, ac.floor_score(len(r))))[0]) for k, r in enumerate(reads)]
    assert hits[0] == [b0 + 63] and hits[2] == [b0 + 64] and hits[3] == [b0 + 127] and hits[4] == [b0 + 128] and hits[5] == [b0] and hits[7] == [b0 + 20]
    assert ac.floor_score(60) <= int(sc[7].max()) < 80
    assert hits[1] == hits[6] == hits[10] == [] and hits[8] == list(range(s0, s0 + 8)) and hits[9] == [b0 + 30]
    assert aligned_by_oracle(idx, *flat) == [0, 2, 3, 4, 5, 7, 8, 9]
    eng = make_engine(idx)
    try:
        eng.submit_reads(*flat)
        retained = set(int(it[0]) for it in eng.items(CAP).tolist())
        assert {6, 10} <= retained and 1 not in retained                                 # retained, yet without a record
        st = eng.stats()
        assert int(st.n_hits[b0 + 20]) == 0 and int(st.n_hits[b0 + 63]) == 1             # read 7's record is counted nowhere
        got = export(eng)
        assert got == rule_bytes(idx, flat)
        recs = records_of(got)
        assert [n for n, _, _ in recs] == [b"r0", b"r2", b"r3", b"r4", b"r5", b"r7", b"r8", b"r9"]
        assert recs[7][1][75:76] == b"N" and recs[7][2] == bytes(min((60 + t) % 128, 93) + 33 for t in range(150)) and b"~" in recs[7][2]
        assert recs[1][1] == reads[2] and recs[3][1] == reads[4]                         # read orientation: never turned to the reference strand
        assert b"".join(eng.export_reads_text(round_bytes=36 * 129)) == got              # a read per round: the bound of `big` is its tables'
    finally:
        eng.close()


@pytest.mark.parametrize("count", [1, 62, 63, 64, 65, FQT_GROUP - 2, FQT_GROUP - 1, FQT_GROUP, FQT_GROUP + 1])
def test_reads_in_one_round_at_the_edges_of_the_scan(count):
    """`count` written reads in one round (the offsets' table holds count + 1 entries), off-locus reads between them"""
    idx = fx.ecoli_small(8)[1]
    rng = np.random.default_rng(count)
    reads = []
    for k in range(count):
        reads.append(planted(idx, (5 * k) % idx.n_alleles, (11 * k) % 200, 50 + (13 * k) % 101, k & 1))
        if k % 9 == 4:
            reads.append(bytes(rng.choice(list(b"ACGT"), size=80).astype(np.uint8)))
    flat = synth.ragged_reads(reads, [bytes(33 + (k + t) % 42 for t in range(len(r))) for k, r in enumerate(reads)])
    eng = make_engine(idx)
    try:
        eng.submit_reads(*flat)
        chunks = list(eng.export_reads_text())
        assert len(chunks) == 1 and chunks[0].count(b"\n") == 4 * count
        assert chunks[0] == rule_bytes(idx, flat)
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. pairs
def pair_reads(idx):
    """pair 0: both mates aligned; pair 1: only the first; pair 2: only the second; pair 3: both, on two loci; pair 4: none"""
    rng = np.random.default_rng(8)
    noise = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    l1 = int(idx.locus_begin[1])
    return [(planted(idx, 2, 30, 120), planted(idx, 2, 200, 100, 1)), (planted(idx, 5, 60, 150), noise(150)), (noise(90), planted(idx, 1, 10, 90, 1)),
            (planted(idx, 3, 100, 75), planted(idx, l1 + 2, 50, 140, 1)), (noise(100), noise(100))]


def test_each_mate_stands_alone_and_carries_its_suffix():
    idx = fx.ecoli_small(8)[1]
    pairs = pair_reads(idx)
    reads = [m for p in pairs for m in p]
    flat = synth.ragged_reads(reads, [b"F" * len(r) for r in reads])
    assert aligned_by_oracle(idx, *flat) == [0, 1, 2, 5, 6, 7]
    eng = make_engine(idx)
    try:
        eng.submit_reads(*flat, paired=True)
        got = export(eng, paired=True)
        assert got == rule_bytes(idx, flat, paired=True)
        assert [n for n, _, _ in records_of(got)] == [b"r0/1", b"r0/2", b"r1/1", b"r2/2", b"r3/1", b"r3/2"]
        assert [n for n, _, _ in records_of(export(eng))] == [b"r0", b"r1", b"r2", b"r5", b"r6", b"r7"]      # the same sample exported as unpaired reads
        # the reads' own names: the mates share one, the suffix tells them apart; pair 3's name is no legal QNAME
        name = lambda k: [b"@frag:%d" % k, b"@p1", b"@" + b"w" * 254, b"@in@valid", b"@none"][k]
        t1 = b"".join(name(k) + b" 1:N\n" + p[0] + b"\n+\n" + b"F" * len(p[0]) + b"\n" for k, p in enumerate(pairs))
        t2 = b"".join(name(k) + b" 2:N\n" + p[1] + b"\n+\n" + b"F" * len(p[1]) + b"\n" for k, p in enumerate(pairs))
        eng.reset_sample()
        eng.set_read_names(True)
        assert eng.submit_fastq_pair(t1, t2) == 10
        got = export(eng, paired=True)
        assert got == rule_bytes(idx, flat, paired=True, names=names_of_text([t1, t2], interleave=True))
        assert [n for n, _, _ in records_of(got)] == [b"frag:0/1", b"frag:0/2", b"p1/1", b"w" * 254 + b"/2", b"r3/1", b"r3/2"]
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. read indices past 32 bits and ten digits
@pytest.mark.parametrize("base", [2 ** 32 - 3, 10 ** 10 - 3])
def test_read_indices_past_32_bits_and_ten_digits(base):
    cp = ac.corpus()
    eng = make_engine(cp.idx)
    try:
        eng.set_read_index_base(base)
        eng.submit_reads(*corpus_reads())
        got = export(eng)
        assert got == corpus_rule(base)
        ks = [int(n[1:]) for n, _, _ in records_of(got)]
        assert ks == sorted(ks) and (min(ks) < 2 ** 32 <= max(ks) if base < 2 ** 32 else min(ks) < 10 ** 10 <= max(ks))
        assert [(s, q) for _, s, q in records_of(got)] == [(s, q) for _, s, q in records_of(corpus_rule())]
        half = rule_bytes(cp.idx, corpus_reads(), paired=True, base=base)                # and as pairs: k = read index >> 1, eleven digits halved
        assert export(eng, paired=True) == half and half != got
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. prepared and cut reads
def test_the_lines_carry_the_prepared_and_cut_reads():
    idx = fx.ecoli_small(8)[1]
    adapter = "AGATCGGAAGAGC"
    rng = np.random.default_rng(77)
    noise = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    inserts = [planted(idx, 1, 20, 150), planted(idx, 4, 90, 100, 1), planted(idx, 6, 40, 14), planted(idx, 2, 10, 64), noise(120), planted(idx, 7, 0, 149, 1)]
    reads = [inserts[0], inserts[1] + adapter.encode() + noise(37), inserts[2] + adapter.encode() + noise(100), inserts[3] + adapter.encode(), inserts[4],
             inserts[5] + b"A"]
    quals = [bytes(64 + 30 + (k + t) % 11 for t in range(len(r))) for k, r in enumerate(reads)]      # Phred + 64
    quals[0] = quals[0][:120] + bytes([64 + 3]) * 30                                       # a decayed tail: the quality trim cuts it
    raw = b"".join(b"@q%d\n%s\n+\n%s\n" % (k, r, q) for k, (r, q) in enumerate(zip(reads, quals)))
    prep = {"trim5": 3, "trim3": 1, "trim_qual": 20, "phred64": True}
    text, _ = prep_fastq(raw, **prep)
    text, info = trim_adapters(text, adapters=[adapter])
    assert info["trimmed"] == 3
    want = rule_bytes(idx, flat_of_text(text))
    recs = records_of(want)
    # the rule's own answer: the read the cut leaves with 11 bases has no record, the others carry what is left of them
    assert [n for n, _, _ in recs] == [b"r0", b"r1", b"r3", b"r5"]
    assert recs[0][1] == inserts[0][3:120] and recs[1][1] == inserts[1][3:] and recs[2][1] == inserts[3][3:] and recs[3][1] == inserts[5][3:]
    assert recs[1][2] == bytes(q - 31 for q in quals[1][3:100])
    eng = make_engine(idx)
    try:
        eng.set_read_prep(**prep)
        eng.set_read_adapters(adapters=[adapter])
        assert eng.submit_fastq(raw) == len(reads)
        assert export(eng) == want
        eng.reset_sample()
        eng.set_read_prep()
        eng.set_read_adapters()
        assert eng.submit_fastq(raw) == len(reads)
        assert export(eng) != want                                                        # the guard: without the switches it is another sample
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. the export changes nothing
def test_the_export_changes_nothing_and_one_text_export_exists_at_a_time():
    idx, (fb, fq, off) = synth_sample(150)
    eng = make_engine(idx)
    nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()

    def nxt(kind):
        return getattr(eng.lib, "mlst_%s_text_next" % kind)(eng._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done))

    def open_sam():
        labels = [idx.label(a).encode() for a in range(idx.n_alleles)]
        noff = np.zeros(len(labels) + 1, np.uint64); noff[1:] = np.cumsum([len(x) for x in labels])
        flat = np.frombuffer(b"".join(labels), np.uint8)
        eng._check(eng.lib.mlst_alignments_text_open(eng._h, _ptr(flat), _ptr(noff), 0, 0), "mlst_alignments_text_open")
    try:
        assert export(eng) == b""                                                         # a sample with no read: done at once
        eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, 0), "mlst_reads_text_open")
        eng._check(nxt("reads"), "mlst_reads_text_next")
        assert (nb.value, nr.value, done.value) == (0, 0, 1)
        eng._check(eng.lib.mlst_reads_text_close(eng._h), "mlst_reads_text_close")
        with pytest.raises(MlstError, match="no export is open"):
            eng._check(nxt("reads"), "mlst_reads_text_next")
        eng.submit_reads(fb, fq, off)
        s0 = eng.stats()
        sam0 = b"".join(eng.export_sam_text(idx))
        eng.typing_enqueue(penalty=100)
        t0 = eng.typing_fetch()
        eng.typing_enqueue(penalty=100)
        body = export(eng)                                                                # between enqueue and fetch
        t1 = eng.typing_fetch()
        assert body == rule_bytes(idx, (fb, fq, off)) and body.count(b"\n") > 400
        assert t1[1] == t0[1] and t1[2] == t0[2]
        fx.assert_stats_equal(t1[0], s0)
        s1 = eng.stats()
        fx.assert_stats_equal(s1, s0)
        assert np.array_equal(s1.counters, s0.counters)
        assert b"".join(eng.export_sam_text(idx)) == sam0 and export(eng) == body
        # the size of the round, a cap that is too small, the round
        eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, 0), "mlst_reads_text_open")
        eng._check(nxt("reads"), "mlst_reads_text_next")
        assert (nb.value, nr.value, done.value) == (len(body), body.count(b"\n") // 4, 0)
        small = np.zeros(16, np.uint8)
        with pytest.raises(MlstError, match="smaller than the round"):
            eng._check(eng.lib.mlst_reads_text_next(eng._h, _ptr(small), 16, C.byref(nb), C.byref(nr), C.byref(done)), "mlst_reads_text_next")
        # the other kind's _next is refused; opening the SAM export over the open reads export works, and turns the tables
        with pytest.raises(MlstError, match="the open export is the one of mlst_reads_text_open"):
            eng._check(nxt("alignments"), "mlst_alignments_text_next")
        open_sam()
        eng._check(nxt("alignments"), "mlst_alignments_text_next")
        assert nb.value == len(sam0) and done.value == 0
        with pytest.raises(MlstError, match="the open export is the one of mlst_alignments_text_open"):
            eng._check(nxt("reads"), "mlst_reads_text_next")
        eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, 0), "mlst_reads_text_open")    # and back
        big = np.zeros(len(body), np.uint8)
        eng._check(eng.lib.mlst_reads_text_next(eng._h, _ptr(big), len(big), C.byref(nb), C.byref(nr), C.byref(done)), "mlst_reads_text_next")
        assert big.tobytes() == body and done.value == 1
        # reset_sample closes it
        eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, 0), "mlst_reads_text_open")
        eng.reset_sample()
        with pytest.raises(MlstError, match="no export is open"):
            eng._check(nxt("reads"), "mlst_reads_text_next")
        # a stream of ready-made alignments is open: refused
        eng.bam_open(1, *samin.bam_ref_table(idx, [idx.label(a) for a in range(idx.n_alleles)], None), skip_bytes=0)
        with pytest.raises(MlstError, match="BAM stream is open"):
            export(eng)
        eng.reset_sample()
        # reads, retained ones among them, but no record: done at once, and an empty file
        few = [mutated_behind_a_seed(idx, a, 100) for a in (0, 50, 100)] + [bytes(np.random.default_rng(3).choice(list(b"ACGT"), size=150).astype(np.uint8))]
        flat = synth.ragged_reads(few, [b"I" * len(r) for r in few])
        assert aligned_by_oracle(idx, *flat) == []
        eng.submit_reads(*flat)
        assert len(eng.items(CAP)) >= 3
        eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, 0), "mlst_reads_text_open")
        eng._check(nxt("reads"), "mlst_reads_text_next")
        assert (nb.value, nr.value, done.value) == (0, 0, 1)
        p = os.path.join(_TMP, "none.fastq")
        assert samout.write_reads(p, eng, False) == 0 and os.path.getsize(p) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ 9. the command
def isolate_fastq(path, header) -> bytes:
    _, (fb, fq, off) = synth_sample(150)
    text = b"".join(header(k) + b"\n" + fb[int(off[k]):int(off[k + 1])].tobytes() + b"\n+\n" + fq[int(off[k]):int(off[k + 1])].tobytes() + b"\n" for k in range(len(off) - 1))
    open(path, "wb").write(text)
    return text


@pytest.mark.parametrize("names", [False, True], ids=["r<k>", "read-names"])
def test_cli_writes_the_rule_and_the_extract_types_to_the_same_nfo(tmp_path, capsys, names):
    db, idx = fx.ecoli_small(40, 5)
    fastq = tmp_path / "small.fastq"
    text = isolate_fastq(fastq, lambda k: b"@x%d extra" % k if k % 50 else b"@bad@%d" % k)
    flags = ["--write-reads"] + (["--read-names"] if names else [])
    tail = ["-d", db.path, "--min_accuracy", "0", "--nloci", "0"]                        # (the .nfo is written whatever the coverage)
    assert cli.main(["type", str(fastq)] + tail + ["--quiet", "-o", str(tmp_path / "plain")]) == 0
    capsys.readouterr()
    assert cli.main(["type", str(fastq)] + tail + flags + ["-o", str(tmp_path / "first")]) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "first")) == ["small.loci.fastq", "small.nfo"]
    got = open(tmp_path / "first" / "small.loci.fastq", "rb").read()
    want = rule_bytes(idx, flat_of_text(text), names=names_of_text([text]) if names else None)
    assert got == want and len(want) > 10000
    n = want.count(b"\n") // 4
    assert "--write-reads: %d reads with an alignment written\n" % n in out
    assert (b"@x1 " not in got) and ((b"@x" in got) == names) and (b"@r" in got)         # (with the names: the fallbacks keep r<k>)
    nfo = open(tmp_path / "first" / "small.nfo", "rb").read()
    assert nfo == open(tmp_path / "plain" / "small.nfo", "rb").read() and len(nfo) > 0   # the flag changes no .nfo
    # the extract under the sample's own file name, typed again with the same flags
    os.makedirs(tmp_path / "again")
    shutil.copy(tmp_path / "first" / "small.loci.fastq", tmp_path / "again" / "small.fastq")
    assert cli.main(["type", str(tmp_path / "again" / "small.fastq")] + tail + flags + ["--quiet", "-o", str(tmp_path / "second")]) == 0
    assert open(tmp_path / "second" / "small.nfo", "rb").read() == nfo
    again = records_of(open(tmp_path / "second" / "small.loci.fastq", "rb").read())
    assert [(s, q) for _, s, q in again] == [(s, q) for _, s, q in records_of(got)]      # every extracted read aligns again


def test_cli_mates_in_two_files(tmp_path, capsys):
    db, idx = fx.ecoli_small(40, 5)
    _, (fb, fq, off) = synth_sample(150)
    n_pairs = 600
    rec = lambda k, f: b"@m%d %d:N\n" % (k >> 1, f) + fb[int(off[k]):int(off[k + 1])].tobytes() + b"\n+\n" + fq[int(off[k]):int(off[k + 1])].tobytes() + b"\n"
    t1, t2 = b"".join(rec(2 * k, 1) for k in range(n_pairs)), b"".join(rec(2 * k + 1, 2) for k in range(n_pairs))
    (tmp_path / "s_1.fastq").write_bytes(t1)
    (tmp_path / "s_2.fastq").write_bytes(t2)
    assert cli.main(["type", str(tmp_path / "s_1.fastq"), "-2", str(tmp_path / "s_2.fastq"), "-d", db.path, "--min_accuracy", "0", "--nloci", "0", "--write-reads",
                     "-o", str(tmp_path / "out")]) == 0
    out = capsys.readouterr().out
    got = open(tmp_path / "out" / "s_1.loci.fastq", "rb").read()
    flat = synth.ragged_reads([fb[int(off[k]):int(off[k + 1])].tobytes() for k in range(2 * n_pairs)], [fq[int(off[k]):int(off[k + 1])].tobytes() for k in range(2 * n_pairs)])
    want = rule_bytes(idx, flat, paired=True)
    assert got == want and b"/1\n" in got and b"/2\n" in got
    assert "--write-reads: %d reads with an alignment written\n" % (want.count(b"\n") // 4) in out
