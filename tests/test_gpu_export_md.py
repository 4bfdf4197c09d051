"""mlst_set_export_md (csrc/aln_text.h): bowtie2's MD:Z field in the text export, formatted on the device, and `cli type --md`.

The yardstick is the plain-Python rule, samout.md_text through format_record(..., md=True): every record of an export with the switch
on is parsed, formatted again by the rule with the FLAG and XS the file states, and has to give the file's bytes; with the field cut
out the bytes have to be those of the export without the switch, which test_gpu_sam_all.py checks against the oracle.  The independent
inverse of test_samout_md_host.py (the allele's bases rebuilt from SEQ + CIGAR + MD alone) runs over the records as well.

Under local scoring an M span neither starts nor ends on a mismatch -- the aligner clips it -- so the reads of the crafted set that
carry a mismatch in their first and last base show that clip; the turn edges are taken by reads whose M span starts at their first
base (mismatches at M-span columns 62 ... 128)."""
import functools
import os
import re

import numpy as np
import pytest

import align_cases as ac
import fixtures as fx
import oracle_lib
from metamlst_amd import cli, samin, samout, synth
from metamlst_amd.engine import MlstError
from metamlst_amd.typing import pick_alleles_fast
from test_gpu_align_export import corpus_reads, make_engine, synth_sample
from test_samout_md_host import assert_line_inverse

pytestmark = pytest.mark.gpu

CAP = 1 << 16
MD_FIELD = re.compile(rb"\tMD:Z:[0-9A-Z^]+(?=\tYT:Z:UU\n)")


def label_map(idx):
    return {idx.label(a): a for a in range(idx.n_alleles)}


def assert_md_body(idx, body: bytes, plain: bytes, names=None, paired=False):
    """every line of `body` (an export with the switch on) is the rule's line for the record it states, passes the inverse, and is
    the line of `plain` (the export without the switch) but for the field.  Returns the MD texts."""
    lines, plain_lines = body.splitlines(keepends=True), plain.splitlines(keepends=True)
    assert len(lines) == len(plain_lines) and b"MD:Z" not in plain
    l2a, texts = label_map(idx), []
    qn2ri = {v.decode(): k for k, v in (names or {}).items()}
    for line, pl in zip(lines, plain_lines):
        assert MD_FIELD.sub(b"", line) == pl and len(MD_FIELD.findall(line)) == 1, line
        f = line.decode()[:-1].split("\t")
        tags = f[11:]
        xs = int(tags[1][5:]) if tags[1].startswith("XS:i:") else None
        ri = qn2ri[f[0]] if f[0] in qn2ri else int(f[0][1:]) << (1 if paired else 0)
        a = l2a[f[2]]
        tag = {t[:2]: t[5:] for t in tags}
        rec = (ri, (int(f[1]) >> 4) & 1, 0, int(idx.locus_id[a]), a, int(f[3]) - 1, int(tag["AS"]), int(tag["XM"]), samin.parse_cigar(f[5]), f[9].encode(),
               bytes(c - 33 for c in f[10].encode()))
        assert samout.format_record(idx, rec, paired, bool(int(f[1]) & 256), xs, names, md=True) == line, line
        texts.append(assert_line_inverse(idx, l2a, line))
    return texts


# ------------------------------------------------------------------ the crafted corpus
@pytest.fixture(scope="module")
def corpus_engine():
    eng = make_engine(ac.corpus().idx)
    eng.submit_reads(*corpus_reads())
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def corpus_bodies(corpus_engine):
    idx = ac.corpus().idx
    assert corpus_engine.get_export_md() is False
    plain = b"".join(corpus_engine.export_sam_text(idx))                                     # before the switch was ever set
    body = b"".join(corpus_engine.export_sam_text(idx, md=True))
    assert corpus_engine.get_export_md() is False                                            # the keyword puts the switch back
    return plain, body


def test_corpus_bytes_are_the_rule(corpus_engine, corpus_bodies):
    idx = ac.corpus().idx
    plain, body = corpus_bodies
    texts = assert_md_body(idx, body, plain)
    assert len(texts) == int(corpus_engine.stats().counters[0]) > 1000                       # MLST_CNT_TOTAL_RECORDS
    kinds = set()
    for line, t in zip(body.splitlines(), texts):
        cig = line.split(b"\t")[5]
        kinds |= ({"plain"} if t.isdigit() else set()) | ({"del"} if "^" in t else set()) | ({"N"} if "N" in t else set())
        kinds |= {"zero between"} if re.search(r"[A-Z]0[A-Z]", t) else set()
        kinds |= {"three digits"} if re.search(r"[0-9]{3}", t) else set()
        kinds |= {"ins"} if b"I" in cig else set()
        kinds |= {"clip"} if b"S" in cig else set()
    assert kinds >= {"plain", "del", "N", "zero between", "three digits", "ins", "clip"}, kinds


def test_rounds_give_the_same_bytes_and_the_bound_holds(corpus_engine, corpus_bodies):
    cp, eng = ac.corpus(), corpus_engine
    plain, body = corpus_bodies
    s0 = eng.stats()
    with pytest.raises(MlstError, match=r"too small: the records of one read may need \d+ bytes") as e:
        list(eng.export_sam_text(cp.idx, round_bytes=1, md=True))
    bound = int(re.search(r"may need (\d+) bytes", str(e.value)).group(1))
    with pytest.raises(MlstError, match=r"may need \d+ bytes") as e0:
        list(eng.export_sam_text(cp.idx, round_bytes=1))
    bound_off = int(re.search(r"may need (\d+) bytes", str(e0.value)).group(1))
    assert bound > bound_off      # per record 13 n + the longest label + 233 against 10 n + the longest label + 192
    chunks = list(eng.export_sam_text(cp.idx, round_bytes=bound, md=True))
    assert len(chunks) > 5 and b"".join(chunks) == body
    assert b"".join(eng.export_sam_text(cp.idx, round_bytes=4 * bound + 17, md=True)) == body
    with pytest.raises(MlstError, match="too small") as e2:
        list(eng.export_sam_text(cp.idx, round_bytes=bound - 1, md=True))
    assert "may need %d bytes" % bound in str(e2.value)                                      # MLST_E_LIMIT
    # the bytes the message names are at least the longest real line, and every read's lines fit its bound
    assert bound >= max(len(l) for l in body.splitlines(keepends=True))
    per_read = {}
    for l in body.splitlines(keepends=True):
        q = l.split(b"\t", 1)[0]
        per_read[q] = per_read.get(q, 0) + len(l)
    assert max(per_read.values()) <= bound
    assert eng.get_export_md() is False
    assert b"".join(eng.export_sam_text(cp.idx)) == plain                                    # switch off after switch on
    s1 = eng.stats()
    fx.assert_stats_equal(s1, s0)
    assert np.array_equal(s1.counters, s0.counters)


# ------------------------------------------------------------------ what MD adds: the turn edges, the 0 behind a deletion
EDGES = (62, 63, 64, 65, 127, 128)


@functools.lru_cache(maxsize=None)
def crafted():
    """(names, reads, quals) on allele 7 of locus n65 (300 columns, 65 alleles).  `short` reads are at most 160 bases (k_at_decide_160
    takes a sample of them alone), the others make the sample one of k_at_decide_320."""
    cp = ac.corpus()
    l = cp.idx.locus_index(ac.SPA, "n65")
    assert int(cp.idx.locus_count[l]) == 65
    a = int(cp.idx.locus_begin[l]) + 7
    s = cp.seq(a).upper()
    assert len(s) == 300

    def mut(b, at):
        b = bytearray(b)
        for p in at:
            b[p] = ac.other_base(b[p])
        return bytes(b)

    def after_del(lo, cut, k, n):
        """s[lo : cut] + s[cut + k :] to n bases, the base behind the deletion changed to one that is neither it nor the first
        deleted base (so moving the gap does not turn the mismatch into a match)"""
        b = bytearray(s[lo:cut] + s[cut + k:cut + k + n - (cut - lo)])
        at = cut - lo
        b[at] = next(c for c in b"ACGT" if c != b[at] and c != s[cut] and c != s[cut + k - 1])
        return bytes(b)
    out = [
        ("edges150", mut(s[20:170], EDGES)),                                                 # M span = the read: columns 62 ... 128
        ("ends150", mut(s[20:170], (0, 63, 64, 149))),                                       # first and last base: clipped; 63 | 64 shifted by one
        ("pair150", mut(s[30:180], (63, 64))),                                               # neighbours across the turn edge
        ("last_of_turn", mut(s[5:155], (127,))),
        ("del1", after_del(40, 115, 1, 150)),
        ("del3", after_del(40, 115, 3, 150)),
        ("ins100", s[60:110] + b"GT" + s[110:208]),                                          # an insertion inside a 100-column run and more
        ("edges161", mut(s[10:171], EDGES)),
        ("ends161", mut(s[10:171], (0, 63, 64, 160))),
        ("clean320", s[0:300] + bytes(np.random.default_rng(5).choice(list(b"ACGT"), size=20).astype(np.uint8))),      # 320 bases, no mismatch on the allele
    ]
    return a, [n for n, _ in out], [r for _, r in out], [b"I" * len(r) for _, r in out]


def crafted_sample(short: bool):
    a, names, reads, quals = crafted()
    keep = [k for k, r in enumerate(reads) if not short or len(r) <= 160]
    return a, [names[k] for k in keep], [reads[k] for k in keep], [quals[k] for k in keep]


def test_the_gapped_crafted_reads_fire_the_gap_trigger_in_the_oracle():
    """on the CPU: the oracle takes the banded alignment for the planted deletions and the insertion against their allele"""
    cp = ac.corpus()
    a, names, reads, quals = crafted_sample(False)
    orc = oracle_lib.Oracle(cp.idx)
    orc.submit_reads(*synth.ragged_reads(reads, quals))
    _, items = orc.stats(want_items=CAP)
    fired = {}
    for ri, loc, strand, diag, _ in items.tolist():
        r = orc.align_one(reads[ri], quals[ri], a, strand, diag)
        if r["used_dp"] and r["score"] >= ac.floor_score(len(reads[ri])):
            fired[names[ri]] = r
    assert set(fired) >= {"del1", "del3", "ins100"}, sorted(fired)
    assert not set(fired) & {"edges150", "ends150", "pair150", "last_of_turn", "edges161", "ends161", "clean320"}, sorted(fired)


@pytest.mark.parametrize("short", [True, False], ids=["k_at_decide_160", "k_at_decide_320"])
def test_crafted_turn_edges_deletions_and_runs(short):
    cp = ac.corpus()
    idx = cp.idx
    a, names, reads, quals = crafted_sample(short)
    assert (max(len(r) for r in reads) <= 160) == short
    eng = make_engine(idx)
    try:
        eng.submit_reads(*synth.ragged_reads(reads, quals))
        plain = b"".join(eng.export_sam_text(idx))
        eng.set_export_md(True)
        assert eng.get_export_md() is True
        body = b"".join(eng.export_sam_text(idx))                                            # the switch, not the keyword
        eng.set_export_md(False)
        texts = assert_md_body(idx, body, plain)
        assert len(texts) > 65
        own = {}                                                                             # read name -> MD of its record on its own allele
        for line, t in zip(body.splitlines(), texts):
            f = line.split(b"\t")
            if f[2].decode() == idx.label(a):
                own.setdefault(names[int(f[0][1:])], []).append((f[5].decode(), t))
        s = cp.seq(a).upper().decode()
        for tag, lo, n in (("edges150", 20, 150), ("edges161", 10, 161)):
            if tag in names:
                want = "62%s0%s0%s0%s61%s0%s%d" % (s[lo + 62], s[lo + 63], s[lo + 64], s[lo + 65], s[lo + 127], s[lo + 128], n - 129)
                assert own[tag] == [("%dM" % n, want)], own[tag]
        for tag, lo, n in (("ends150", 20, 150), ("ends161", 10, 161)):
            if tag in names:                                                                 # first and last base clipped: columns 62 | 63 of the span
                assert own[tag] == [("1S%dM1S" % (n - 2), "62%s0%s%d" % (s[lo + 63], s[lo + 64], n - 66))], own[tag]
        assert own["pair150"] == [("150M", "63%s0%s85" % (s[93], s[94]))], own["pair150"]
        assert own["last_of_turn"] == [("150M", "127%s22" % s[132])], own["last_of_turn"]
        (cig, t), = own["del1"]
        assert re.fullmatch(r"75M1D75M", cig) and t == "75^%s0%s74" % (s[115], s[116]), own["del1"]
        (cig, t), = own["del3"]
        assert cig == "75M3D75M" and t == "75^%s0%s74" % (s[115:118], s[118]), own["del3"]
        (cig, t), = own["ins100"]
        assert re.fullmatch(r"(49M2I99M|50M2I98M)", cig) and t == "148", own["ins100"]      # (GT or TG: the run is not broken either way)
        if not short:
            assert own["clean320"] == [("300M20S", "300")], own["clean320"]
    finally:
        eng.close()


# ------------------------------------------------------------------ with the reads' own names
def test_read_names_of_1_and_254_bytes_give_the_same_md(tmp_path):
    cp = ac.corpus()
    idx = cp.idx
    a, names, reads, quals = crafted_sample(False)
    heads = [bytes([97 + k]) if k % 2 == 0 else bytes([65 + k]) * 254 for k in range(len(reads))]
    text = b"".join(b"@%s extra words\n%s\n+\n%s\n" % (h, r, q) for h, r, q in zip(heads, reads, quals))
    eng, off = make_engine(idx), make_engine(idx)
    try:
        eng.set_read_names(True)
        eng.submit_fastq(text)
        off.submit_fastq(text)
        want = b"".join(off.export_sam_text(idx, md=True))
        kept = eng.read_names()
        assert kept and set(kept.values()) <= set(heads) and {len(v) for v in kept.values()} == {1, 254}
        plain = b"".join(eng.export_sam_text(idx))
        body = b"".join(eng.export_sam_text(idx, md=True))
        assert_md_body(idx, body, plain, names=kept)
        assert [l.split(b"\t", 1)[1] for l in body.splitlines()] == [l.split(b"\t", 1)[1] for l in want.splitlines()]
        assert [l.split(b"\t", 1)[0] for l in body.splitlines()] == [kept[int(l.split(b"\t", 1)[0][1:])] for l in want.splitlines()]
        bound = lambda e: int(re.search(r"may need (\d+) bytes", str(e.value)).group(1))      # noqa: E731
        with pytest.raises(MlstError, match="too small") as e1:
            list(eng.export_sam_text(idx, round_bytes=1, md=True))
        assert b"".join(eng.export_sam_text(idx, round_bytes=bound(e1), md=True)) == body
    finally:
        eng.close(); off.close()


# ------------------------------------------------------------------ the switch
def test_the_switch_is_no_part_of_the_sample_and_is_refused_while_an_export_is_open():
    idx, (fb, fq, off) = synth_sample(150)
    eng = make_engine(idx)
    try:
        assert eng.get_export_md() is False
        eng.set_export_md(True); eng.set_export_md(False)                                    # before any submission
        eng.submit_reads(fb, fq, off)
        s0 = eng.stats()
        chosen = sorted(pick_alleles_fast(idx, s0, 100).values())
        p0 = eng.pileup(chosen)
        before = b"".join(eng.export_sam_text(idx))
        eng.set_export_md(True)
        on = b"".join(eng.export_sam_text(idx))
        assert eng.get_export_md() is True and on != before
        assert_md_body(idx, on, before)
        gen = eng.export_sam_text(idx, round_bytes=1 << 20)
        first = next(gen)                                                                    # an export is open
        with pytest.raises(MlstError, match="an export is open"):
            eng.set_export_md(False)
        assert eng.get_export_md() is True
        assert on.startswith(first) and first.endswith(b"\n")
        gen.close()
        eng.set_export_md(False)
        assert b"".join(eng.export_sam_text(idx)) == before                                  # switch off after switch on
        s1 = eng.stats()
        fx.assert_stats_equal(s1, s0)
        assert np.array_equal(s1.counters, s0.counters)
        p1 = eng.pileup(chosen)
        assert all(np.array_equal(p0[a], p1[a]) for a in chosen)
        eng.set_export_md(True)
        eng.reset_sample()                                                                   # a reset keeps the switch and closes nothing it needs
        assert eng.get_export_md() is True and list(eng.export_sam_text(idx)) == []
    finally:
        eng.close()


# ------------------------------------------------------------------ end to end
def test_cli_md_in_both_exports(tmp_path):
    db, idx = fx.ecoli_small(40, 5)
    _, (fb, fq, off) = synth_sample(150)
    fastq = tmp_path / "s.fastq"
    with open(fastq, "wb") as f:
        for k in range(len(off) - 1):
            f.write(b"@x%d\n%s\n+\n%s\n" % (k, fb[int(off[k]):int(off[k + 1])].tobytes(), fq[int(off[k]):int(off[k + 1])].tobytes()))
    tail = ["-d", db.path, "--quiet", "--min_accuracy", "0", "--nloci", "0"]
    for out, extra in (("plain", []), ("md", ["--md"])):
        assert cli.main(["type", str(fastq)] + tail + ["-o", str(tmp_path / out), "--log", "--write-sam", "--write-sam-all"] + extra) == 0
    def by_kind(d):      # (the --log file carries the time of its run in its name)
        return {("log" if f.endswith(".out") else f): open(tmp_path / d / f, "rb").read() for f in os.listdir(tmp_path / d)}
    md_files, plain_files = by_kind("md"), by_kind("plain")
    assert sorted(md_files) == sorted(plain_files) == ["log", "s.all.sam", "s.nfo", "s.sam"]
    assert md_files["s.nfo"] == plain_files["s.nfo"] and md_files["log"] == plain_files["log"] and len(md_files["s.nfo"]) > 0 and len(md_files["log"]) > 0
    l2a = label_map(idx)
    for name in ("s.sam", "s.all.sam"):
        with_md = [l for l in open(tmp_path / "md" / name, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]
        plain = [l for l in open(tmp_path / "plain" / name, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]
        assert len(with_md) == len(plain) > 100
        for l, p in zip(with_md, plain):
            assert MD_FIELD.sub(b"", l) == p
            assert_line_inverse(idx, l2a, l)
        assert any(b"^" in MD_FIELD.search(l).group(0) for l in with_md), name
    # the file with MD:Z types to the same .nfo through the device SAM reader and through samin
    nfo = open(tmp_path / "md" / "s.nfo", "rb").read()
    sam = tmp_path / "in" / "s.all.sam"
    os.makedirs(sam.parent)
    os.replace(tmp_path / "md" / "s.all.sam", sam)
    assert cli.main(["type", str(sam), "--alignments"] + tail + ["-o", str(tmp_path / "dev")]) == 0
    assert open(tmp_path / "dev" / "s.nfo", "rb").read() == nfo
    bare = tmp_path / "bare" / "s.all.sam"
    os.makedirs(bare.parent)
    with open(sam, "rb") as f, open(bare, "wb") as g:
        g.writelines(l for l in f if not l.startswith(b"@SQ"))
    assert not samin.read_sam_header(str(bare))
    assert cli.main(["type", str(bare), "--alignments"] + tail + ["-o", str(tmp_path / "host")]) == 0
    assert open(tmp_path / "host" / "s.nfo", "rb").read() == nfo
