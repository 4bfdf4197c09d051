"""mlst_set_read_names (csrc/read_names.h): the names of the retained reads copied out of the FASTQ text on the device, through every
entry that carries FASTQ text, against a plain Python FASTQ reader plus samout.read_qname; the two exports with those names as QNAME
against samout.all_records_rule(..., names=...); the refusals; `cli type --read-names`.

The records the export is compared with come from an engine with the switch off (its text export is checked against the oracle by
test_gpu_sam_all.py): the same reads give the same records, and only the first column may differ."""
import os
import re

import numpy as np
import pytest

import deflate_writer as dw
import fixtures as fx
import read_names_cases as rc
from metamlst_amd import cli, samin, samout
from metamlst_amd.engine import Engine, MlstError, default_params
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_sam_all import assert_rule_bytes, export

pytestmark = pytest.mark.gpu

CAP = 1 << 16
ZERO = {"named": 0, "bytes": 0, "fallbacks": 0, "longest": 0}


def header3(k: int) -> bytes:
    """one of the crafted headers for every third read, an Illumina-style one otherwise"""
    return rc.HEADERS[(k // 3) % len(rc.HEADERS)][0] if k % 3 == 0 else rc.illumina(k)


def mate_header(f: int):
    return lambda k: rc.illumina(2 * k).split(b" ")[0] + b" %d:N:0:ACGT" % (f + 1)


@pytest.fixture(scope="module")
def data():
    idx, reads = rc.sample()
    return idx, reads, rc.fastq_text(reads, header3)


def new_engine(idx, names: bool):
    eng = Engine(0, default_params())
    eng.load_reference(idx)
    if names:
        eng.set_read_names(True)
    return eng


@pytest.fixture(scope="module")
def eng_on(data):
    eng = new_engine(data[0], True)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng_off(data):
    eng = new_engine(data[0], False)
    yield eng
    eng.close()


def retained(eng) -> list:
    return sorted(set(int(it[0]) for it in eng.items(CAP).tolist()))


def assert_names(eng, heads: dict, what=""):
    """Engine.read_names() is the yardstick restricted to the reads in eng.items(), no more and no fewer; the info figures are its counts"""
    ret = retained(eng)
    want = rc.kept(heads, ret)
    got = eng.read_names()
    assert got == want, (what, len(got), len(want), [(k, got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)][:5])
    assert eng.read_names_info() == {"named": len(want), "bytes": sum(len(v) for v in want.values()), "fallbacks": len(ret) - len(want),
                                     "longest": max([len(v) for v in want.values()] or [0])}, what
    return ret, want


def test_one_whole_chunk_many_workgroups_and_the_crafted_headers(data, eng_on):
    """the first record starts at byte 0, the last has no trailing LF; 300 retained reads and more, off-locus reads between them"""
    idx, reads, text = data
    eng_on.reset_sample()
    assert eng_on.get_read_names() is True
    assert eng_on.submit_fastq(text[:-1]) == len(reads) and text[:1] == b"@" and text[-2:-1] != b"\n"
    heads = rc.yardstick([text])
    ret, want = assert_names(eng_on, heads)
    assert len(ret) >= 300 and len(ret) < len(reads) // 2
    gaps = np.diff(ret)
    assert int((gaps > 1).sum()) > 100, "off-locus reads stand between the retained ones"
    # every crafted header is the header of a retained read: both sides of the 254 / 255 byte edge, every reason for a fallback
    seen = set(heads[ri] for ri in ret)
    assert all(h in seen for h, _ in rc.HEADERS), [h[:20] for h, _ in rc.HEADERS if h not in seen]
    assert b"n" * 254 in want.values() and eng_on.read_names_info()["longest"] == 254
    assert all(re.fullmatch(rb"[!-?A-~]{1,254}", v) for v in want.values())


def test_a_stream_cut_at_every_byte_of_a_header_line(data, eng_on):
    idx, reads, _ = data
    few = reads[:240]
    text = rc.fastq_text(few, rc.illumina)
    heads = rc.yardstick([text])
    eng_on.reset_sample()
    assert eng_on.submit_fastq_stream(text, final=True) == len(few)
    ret, want = assert_names(eng_on, heads, "uncut")
    assert len(ret) >= 8
    victim = ret[len(ret) // 2]                                              # a retained read in the middle of the file
    start = sum(len(h) + len(b) + len(q) + 5 for h, (b, q) in zip((rc.illumina(k) for k in range(victim)), few))
    assert text[start:start + len(heads[victim])] == heads[victim]
    for cut in range(start, start + len(heads[victim]) + 2):                 # in front of the `@` ... behind the line's LF
        eng_on.reset_sample()
        n = eng_on.submit_fastq_stream(text[:cut], final=False)
        n += eng_on.submit_fastq_stream(text[cut:], final=True)
        assert n == len(few), cut
        assert eng_on.read_names() == want, cut
    assert eng_on.read_names_info()["named"] == len(want)


def test_crlf_text(data, eng_on):
    idx, reads, _ = data
    few = reads[:600]
    text = rc.fastq_text(few, header3, eol=b"\r\n")
    eng_on.reset_sample()
    assert eng_on.submit_fastq(text) == len(few)
    ret, want = assert_names(eng_on, rc.yardstick([text]), "CRLF")
    assert len(want) > 20 and not any(b"\r" in v for v in want.values())


def blocks_cut_inside_names(text: bytes, spans, seed: int, top: int = 3000) -> list:
    """BGZF blocks of `text` written by deflate_writer's random parser; a block ends inside every span (the names of the retained
    reads), the other blocks hold at most `top` bytes"""
    ends = sorted(set((a + b) // 2 for a, b in spans if b - a >= 2))
    cuts, at = [], 0
    for e in ends + [len(text)]:
        while e - at > top:
            at += top - 7 * (len(cuts) % 5)
            cuts.append(at)
        if e > at:
            cuts.append(e)
            at = e
    out, lo = [], 0
    for k, hi in enumerate(cuts):
        s = dw.random_stream(text[lo:hi], seed + k)
        out.append(dw.bgzf(s.raw, s.data))
        lo = hi
    assert lo == len(text)
    return out


def name_spans(text: bytes, reads_of_text) -> list:
    """(start, end) of the name of every listed record (0-based in the text)"""
    starts, at = [], 0
    for h, b, q in rc.fastq_records(text):
        starts.append(at)
        at += len(h) + len(b) + len(q) + 5
    assert at == len(text)
    return [(starts[r] + 1, starts[r] + 1 + len(samout.read_qname(text[starts[r]:starts[r] + 400].split(b"\n")[0], 0))) for r in reads_of_text]


EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_bgzf_names_straddle_blocks_and_pieces(data, eng_on):
    idx, reads, _ = data
    few = reads[:1200]
    text = rc.fastq_text(few, header3)
    heads = rc.yardstick([text])
    eng_on.reset_sample()
    eng_on.submit_fastq(text)
    ret, want = assert_names(eng_on, heads, "text")
    blocks = blocks_cut_inside_names(text, name_spans(text, ret), 11)
    assert len(blocks) > len(ret)
    for per_piece in (1, 7, len(blocks)):                                    # a block per call, seven, the file at once: every piece ends inside a name
        eng_on.reset_sample()
        n = 0
        for k in range(0, len(blocks), per_piece):
            last = k + per_piece >= len(blocks)
            n += eng_on.submit_fastq_bgzf(b"".join(blocks[k:k + per_piece]) + (EOF_BLOCK if last else b""), final=last)
        assert n == len(few), per_piece
        assert_names(eng_on, heads, "bgzf, %d blocks per call" % per_piece)


def mate_texts(reads, n_pairs: int):
    """two mate files that share names; the second file's reads are 30 bases shorter, so the files fall out of step"""
    t1 = rc.fastq_text([reads[2 * k] for k in range(n_pairs)], mate_header(0))
    t2 = rc.fastq_text([(reads[2 * k + 1][0][:-30], reads[2 * k + 1][1][:-30]) for k in range(n_pairs)], mate_header(1))
    return t1, t2


def test_pairs_as_text_and_as_bgzf_with_one_file_ahead(data, eng_on):
    idx, reads, _ = data
    t1, t2 = mate_texts(reads, 800)
    heads = rc.yardstick([t1, t2], interleave=True)
    eng_on.reset_sample()
    assert eng_on.submit_fastq_pair(t1, t2) == 1600
    ret, want = assert_names(eng_on, heads, "submit_fastq_pair")
    assert len(ret) >= 100 and any(r % 2 == 0 and r + 1 in want and want[r] == want[r + 1] for r in want), "no pair with both mates retained"
    spans1, spans2 = name_spans(t1, [r >> 1 for r in ret if r % 2 == 0]), name_spans(t2, [r >> 1 for r in ret if r % 2 == 1])
    b1, b2 = blocks_cut_inside_names(t1, spans1, 23), blocks_cut_inside_names(t2, spans2, 29, top=1700)
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])),                           # file 1 nine blocks ahead: its records wait for their mates
             (b"".join(b1[9:10]), b"".join(b2[1:30])),                       # then file 2 overtakes
             (b"", b"".join(b2[30:40])),
             (b"".join(b1[10:]) + EOF_BLOCK, b"".join(b2[40:]) + EOF_BLOCK)]
    step = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(EOF_BLOCK, EOF_BLOCK)]
    for what, calls in (("one file ahead", ahead), ("three blocks of each per call", step)):
        eng_on.reset_sample()
        n = sum(eng_on.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
        assert n == 1600, what
        assert_names(eng_on, heads, what)


def test_read_indices_continue_and_the_index_base(data):
    idx, reads, _ = data
    ta, tb = rc.fastq_text(reads[:700], header3), rc.fastq_text(reads[700:1500], header3, first=700)
    eng = new_engine(idx, True)
    try:
        for base in (0, 2 ** 33 + 5):
            eng.reset_sample()
            eng.set_read_index_base(base)
            assert eng.submit_fastq(ta) == 700 and eng.submit_fastq_stream(tb, final=True) == 800
            ret, want = assert_names(eng, rc.yardstick([ta, tb], base=base), base)
            assert min(ret) < base + 700 <= max(ret) and len(want) > 50
    finally:
        eng.close()


def test_reset_empties_the_names_and_keeps_the_switch(data, eng_on):
    idx, reads, text = data
    eng_on.reset_sample()
    eng_on.submit_fastq(text)
    assert eng_on.read_names_info()["named"] > 0
    eng_on.reset_sample()
    assert eng_on.get_read_names() is True and eng_on.read_names() == {} and eng_on.read_names_info() == ZERO
    few = rc.fastq_text(reads[:300], rc.illumina)
    eng_on.submit_fastq(few)
    assert_names(eng_on, rc.yardstick([few]), "after a reset")


def test_an_arena_that_is_too_small_is_said_with_the_bytes_needed(data, monkeypatch):
    idx, reads, text = data
    monkeypatch.setenv("MLST_NAMES_BYTES", "1000")
    eng = new_engine(idx, True)
    try:
        eng.submit_fastq(text)
        ret = retained(eng)
        need = sum(len(v) for v in rc.kept(rc.yardstick([text]), ret).values())
        with pytest.raises(MlstError, match=r"\(-5\).*need %d bytes and the arena holds 1000" % need):
            eng.read_names_info()
        with pytest.raises(MlstError, match=r"\(-5\)"):
            eng.stats()
        eng.reset_sample()
        few = rc.fastq_text(reads[:60], rc.illumina)
        eng.submit_fastq(few)                                                # a sample that fits
        assert_names(eng, rc.yardstick([few]), "after the overflow")
    finally:
        eng.close()


# ------------------------------------------------------------------ the text export
def rule_bytes(idx, recs_off, paired, names) -> bytes:
    return b"".join(samout.all_records_rule(idx, [r.as_tuple(idx) for r in recs_off], paired, names=names))


def bound_of(eng, idx, paired=False) -> int:
    with pytest.raises(MlstError, match=r"\(-5\).*too small: the records of one read may need \d+ bytes") as e:
        list(eng.export_sam_text(idx, paired=paired, round_bytes=1))
    return int(re.search(r"may need (\d+) bytes", str(e.value)).group(1))


def test_export_bytes_unpaired_with_every_kind_of_header(data, eng_on, eng_off, tmp_path):
    idx, reads, text = data
    few = reads[:2500]
    text = rc.fastq_text(few, header3)
    for eng in (eng_on, eng_off):
        eng.reset_sample()
        assert eng.submit_fastq(text) == len(few)
    recs_off, body_off = export(eng_off, idx, tmp_path / "off.all.sam")
    # switch off: the r<k> rule, no name kept, all zeros
    assert_rule_bytes(idx, recs_off, body_off)
    assert eng_off.get_read_names() is False and eng_off.read_names() == {} and eng_off.read_names_info() == ZERO
    assert any(o & 15 in (1, 2) for r in recs_off for o in r.ops), "no banded record in the sample"
    ret, names = assert_names(eng_on, rc.yardstick([text]))
    want = rule_bytes(idx, recs_off, False, names)
    body = b"".join(eng_on.export_sam_text(idx))
    assert body == want and body != body_off
    assert len(body) == len(body_off) + sum(len(names[r.ri]) - len(b"r%d" % r.ri) for r in recs_off if r.ri in names)
    # a banded record behind a name of every length class: its CIGAR, written from the back, lands behind the variable-length QNAME
    gapped = [r for r in recs_off if any(o & 15 in (1, 2) for o in r.ops)]
    assert any(r.ri in names and len(names[r.ri]) > 40 for r in gapped) and any(r.ri not in names for r in gapped)
    # independent of round_bytes; one read per round; a 254-byte name makes the bound longer than the numbered one
    bound, bound_off = bound_of(eng_on, idx), bound_of(eng_off, idx)
    assert bound > bound_off and (bound - bound_off) % (254 - 21) == 0
    chunks = list(eng_on.export_sam_text(idx, round_bytes=bound))
    assert b"".join(chunks) == want and len(chunks) == len(set(r.ri for r in recs_off))
    assert b"".join(eng_on.export_sam_text(idx, round_bytes=3 * bound + 11)) == want
    with pytest.raises(MlstError, match=r"\(-5\).*may need %d bytes" % bound):
        list(eng_on.export_sam_text(idx, round_bytes=bound - 1))
    assert b"".join(eng_off.export_sam_text(idx, round_bytes=bound_off)) == body_off
    # and the export to the chosen alleles with the map: only the first column differs, and it is the read's name
    from metamlst_amd.typing import pick_alleles_fast
    chosen = sorted(pick_alleles_fast(idx, eng_on.stats(), 100).values())
    aln = eng_on.export_alignments(chosen)
    p0, p1 = str(tmp_path / "c0.sam"), str(tmp_path / "c1.sam")
    samout.write_sam(p0, idx, chosen, aln, False)
    samout.write_sam(p1, idx, chosen, aln, False, names=eng_on.read_names())
    l0, l1 = open(p0, "rb").read().split(b"\n"), open(p1, "rb").read().split(b"\n")
    assert len(l0) == len(l1) > 100
    for a, b in zip(l0, l1):
        if a.startswith(b"@") or not a:
            assert a == b
            continue
        ri = int(a.split(b"\t", 1)[0][1:])
        assert b.split(b"\t", 1) == [names.get(ri, b"r%d" % ri), a.split(b"\t", 1)[1]]


def test_export_bytes_pairs_with_shared_names(data, eng_on, eng_off, tmp_path):
    idx, reads, _ = data
    t1, t2 = mate_texts(reads, 1000)
    t1 = t1.replace(rc.illumina(2 * 4).split(b" ")[0], b"@odd@name", 1)    # one pair whose first mate has no legal name: r<read index >> 1>
    for eng in (eng_on, eng_off):
        eng.reset_sample()
        assert eng.submit_fastq_pair(t1, t2) == 2000
    recs_off, _ = export(eng_off, idx, tmp_path / "off.all.sam")                                # (read-index names: they say which mate a record belongs to)
    ret, names = assert_names(eng_on, rc.yardstick([t1, t2], interleave=True))
    want = rule_bytes(idx, recs_off, True, names)
    assert b"".join(eng_on.export_sam_text(idx, paired=True)) == want
    assert b"".join(eng_on.export_sam_text(idx, paired=True, round_bytes=bound_of(eng_on, idx, True))) == want
    q = [l.split(b"\t", 1)[0] for l in want.splitlines()]
    both = [r for r in ret if r % 2 == 0 and r + 1 in names and r in names]
    assert both and all(q.count(names[r]) >= 2 for r in both[:20])                              # mates share a name in the file
    if 8 in ret:
        assert b"r4" in q and 8 not in names


# ------------------------------------------------------------------ refusals
def test_every_other_way_of_adding_reads_is_refused(data):
    idx, reads, text = data
    eng = new_engine(idx, True)
    try:
        fb = np.frombuffer(reads[0][0], np.uint8); fq = np.frombuffer(reads[0][1], np.uint8); off = np.array([0, len(fb)], np.uint64)
        calls = {
            "mlst_submit_reads": lambda: eng.submit_reads(fb, fq, off),
            "mlst_submit_reads_device": lambda: eng.submit_reads_device(0, 0, 0, 1, 150),
            "mlst_submit_packed_device": lambda: eng.submit_packed_device(0, 0, 0, 1, 10, 152),
            "mlst_submit_packed_host": lambda: eng._check(eng.lib.mlst_submit_packed_host(eng._h, None, None, None, 1, 10, 152, 0), "mlst_submit_packed_host"),
            "mlst_submit_fasta": lambda: eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n"),
            "mlst_bam_reads_open": lambda: eng.bam_reads_open(0),
            "mlst_set_read_tiling": lambda: eng.set_read_tiling(150, 25),
        }
        for entry, call in calls.items():
            with pytest.raises(MlstError, match=r"\(-1\): %s: read names are on" % entry):
                call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text[:40000].rsplit(b"\n@M0", 1)[0] + b"\n") > 0              # the handle stays usable
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_names(False)
        assert eng.get_read_names() is True
        eng.set_read_names(True)                                             # (no change: accepted)
        eng.reset_sample()
        eng.set_read_names(False)
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_names(True)
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\).*mlst_set_read_tiling is on"):
            eng.set_read_names(True)
        eng.set_read_tiling(0, 0)
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_names(True)
    finally:
        eng.close()


# ------------------------------------------------------------------ the product
@pytest.mark.parametrize("kind", ["plain text", "-2 on bgzip'd mates"])
def test_cli_read_names_end_to_end(data, tmp_path, capsys, kind):
    idx, reads, _ = data
    db, _ = fx.ecoli_small(40, 5)
    if kind == "plain text":
        text = rc.fastq_text(reads[:3000], rc.illumina)
        fastq = tmp_path / "s.fastq"
        fastq.write_bytes(text)
        files, texts = [str(fastq)], [text]
    else:
        t1, t2 = mate_texts(reads, 1500)
        p1, p2 = tmp_path / "s.fastq.gz", tmp_path / "s_R2.fastq.gz"
        p1.write_bytes(b"".join(bgzf_blocks(t1, (4000, 65280, 1234))))
        p2.write_bytes(b"".join(bgzf_blocks(t2, (3000, 50000))))
        files, texts = [str(p1), "-2", str(p2)], [t1, t2]
    fastq_names = set(samout.read_qname(h, -1) for t in texts for h, _, _ in rc.fastq_records(t))
    tail = ["-d", db.path, "--min_accuracy", "0", "--nloci", "0"]            # (the .nfo is written whatever the coverage)
    assert cli.main(["type"] + files + tail + ["--quiet", "-o", str(tmp_path / "plain"), "--log"]) == 0
    capsys.readouterr()
    assert cli.main(["type"] + files + tail + ["-o", str(tmp_path / "named"), "--log", "--write-sam", "--write-sam-all", "--read-names"]) == 0
    said = capsys.readouterr().out
    m = re.search(r"--read-names: (\d+) reads on the loci keep their names, (\d+) have a name that is no legal QNAME", said)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) == 0
    nfo = open(tmp_path / "plain" / "s.nfo", "rb").read()
    assert nfo == open(tmp_path / "named" / "s.nfo", "rb").read() and len(nfo) > 0
    logs = [sorted(f for f in os.listdir(tmp_path / d) if f.endswith(".out")) for d in ("plain", "named")]
    assert len(logs[0]) == len(logs[1]) == 1
    assert open(tmp_path / "plain" / logs[0][0], "rb").read() == open(tmp_path / "named" / logs[1][0], "rb").read()
    for name in ("s.sam", "s.all.sam"):
        q = [l.split(b"\t", 1)[0] for l in open(tmp_path / "named" / name, "rb") if not l.startswith(b"@")]
        assert len(q) > 100
        assert all(x in fastq_names for x in q), [x for x in q if x not in fastq_names][:5]      # every QNAME is a name of the FASTQ
        assert len(set(q)) > 100
    sam = tmp_path / "in" / "s.all.sam"
    os.makedirs(sam.parent)
    os.replace(tmp_path / "named" / "s.all.sam", sam)
    assert samin.read_sam_header(str(sam))
    assert cli.main(["type", str(sam), "--alignments", "--quiet"] + tail + ["-o", str(tmp_path / "back")]) == 0
    assert open(tmp_path / "back" / "s.nfo", "rb").read() == nfo
