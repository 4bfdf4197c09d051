"""SAM text typed on the device (mlst_sam_open / mlst_submit_sam_text; kernels: csrc/sam_dev.h).  The yardstick is always the
host reader (samin.AlignmentSample) on the same file at the same arguments."""
import glob
import gzip
import json
import os

import numpy as np
import pytest

import golden_util as gu
import samin_ref
from metamlst_amd import db as mdb
from metamlst_amd import samin
from metamlst_amd.index import load_index
from metamlst_amd.typing import TypingArgs, log_table, type_sample
from test_bam_gpu import CASES, assert_stats_equal, chosen_set, host_stats, make_engine, write, write_sam, zoo
from test_golden_typing import parse_args

pytestmark = pytest.mark.gpu

MAX_LINE = 1048576 - 64      # MLST_BAM_MAX_RECORD (include/mlst_policy.h)
FQ_BLOCK = 4096              # bytes of text per workgroup of k_fq_count / k_fq_lines
HD = "@HD\tVN:1.0\tSO:unsorted\n"
SEQ60 = "ACGTTGCATGCAACGTACGTTAGCCGATAGCTTGCAACGTACGGTCAGTCAAGCTTGCAT"      # (the default --min_read_len is 50)


def header(names):
    return HD + "".join("@SQ\tSN:%s\tLN:500\n" % n for n in names)


def line(r, extra=()):
    """a record of test_bam_gpu.zoo as SAM text (write_sam's columns), without its LF"""
    return "\t".join([r[0], str(r[1]), r[2], str(r[3]), str(r[4]), r[5], "*", "0", "0", r[6], r[7]] + list(r[8]) + list(extra))


def rec(qname, rname, AS, seq=SEQ60, qual=None, cigar=None, pos=1, xm=0, tags=None):
    tags = ["AS:i:%d" % AS, "XS:i:1", "XN:i:0", "XM:i:%d" % xm, "XO:i:0", "XG:i:0", "NM:i:0", "YT:Z:UU"] if tags is None else tags
    return (qname, 0, rname, pos, 255, cigar or "%dM" % len(seq), seq, qual or "I" * len(seq), tags)


def put(path, text):
    with open(str(path), "wb") as f:
        f.write(text if isinstance(text, bytes) else text.encode())
    return str(path)


@pytest.fixture(scope="module")
def gold():
    idx = load_index(gu.golden_db())
    return idx, make_engine(idx)


def device_stats(eng, path, filt=None, **kw):
    eng.reset_sample()
    n = eng.submit_sam_file(path, filt, **kw)
    return n, eng.stats()


def chunks_stats(eng, idx, names, pieces):
    """the text given as `pieces` (the last one final) through sam_open / submit_sam_text: (records, statistics)"""
    eng.reset_sample()
    eng.sam_open(1, names, *samin.bam_ref_table(idx, names, None))
    n = 0
    for k, p in enumerate(pieces):
        n += eng.submit_sam_text(p, k == len(pieces) - 1)
    return n, eng.stats()


def with_sq_lines(sam, out):
    """the records of a golden input.sam behind the header bowtie2 writes: an @SQ line per contig (in order of appearance)"""
    als = list(samin.read_alignments(sam))
    names = list(dict.fromkeys(al.rname for al in als if al.rname != "*"))
    body = b"".join(l for l in open(sam, "rb") if not l.startswith(b"@"))
    return put(out, header(names).encode() + body), len(als)


# ------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c) for c in CASES])
def test_golden_cases_through_the_device_path(case, tmp_path):
    targs, prm = parse_args(json.load(open(os.path.join(case, "args.json"))))
    dbp = gu.golden_db()
    idx = load_index(dbp, targs.filter.split(",") if targs.filter else None)
    sam, n_host = with_sq_lines(os.path.join(case, "input.sam"), tmp_path / "input.sam")
    _, want = host_stats(idx, targs, sam)
    eng = make_engine(idx, prm)
    n, got = device_stats(eng, sam, targs.filter or None)
    assert n == n_host
    assert_stats_equal(got, want)
    counts = json.load(open(os.path.join(case, "counts.json")))

    def pileup_fn(chosen):
        return {a: np.array(counts["%s_%s" % idx.loci[int(idx.locus_id[a])]], np.uint32) for a in chosen}

    res = type_sample(idx, got, pileup_fn, mdb.metaMLST_db(dbp), "sampleX", targs)
    assert "".join(r.nfo_line for r in res if r.written).encode() == open(os.path.join(case, "expected.nfo"), "rb").read()
    logf = os.path.join(case, "expected_log.out")
    if os.path.exists(logf):
        assert log_table(idx, got, targs, "x").encode().split(b"\r\n", 1)[1] == open(logf, "rb").read()
    # as it is (no @SQ line), the file's first record is the host's
    from metamlst_amd.engine import HostPathNeeded
    eng.reset_sample()
    with pytest.raises(HostPathNeeded, match="an RNAME that is not among the header's @SQ names at record 0$"):
        eng.submit_sam_file(os.path.join(case, "input.sam"))
    eng.reset_sample()


# ------------------------------------------------------------------ 2. zoo
def test_record_zoo_statistics_and_pileup_equal_the_host_path(gold, tmp_path):
    from metamlst_amd.engine import default_params
    idx, eng = gold
    refs, recs = zoo(idx, 20_000)
    path = write_sam(tmp_path / "zoo.sam", refs, recs)
    chunk = 1 << 20
    assert os.path.getsize(path) >= 5 * chunk
    smp, want = host_stats(idx, None, path)
    n, got = device_stats(eng, path, chunk_bytes=chunk)
    assert n == 20_000 == smp.n_records
    assert_stats_equal(got, want)
    chosen = chosen_set(idx)
    ref = samin_ref.pileup_python(idx, smp, chosen)
    host = smp.pileup(eng, chosen)
    dev = eng.pileup_sam_file(path, chosen, chunk_bytes=chunk)
    assert set(dev) == set(ref) and sum(int(v.sum()) for v in ref.values()) > 1000
    for a in ref:
        assert np.array_equal(dev[a], ref[a]) and np.array_equal(dev[a], host[a]), a
    assert eng.pileup_sam_file(path, []) == {}
    p99 = default_params(); p99.minqual = 99
    e99 = make_engine(idx, p99)
    d99 = e99.pileup_sam_file(path, chosen, chunk_bytes=chunk)
    assert all(int(v.sum()) == 0 for v in d99.values()) and all(int(v.sum()) == 0 for v in smp.pileup(e99, chosen, minqual=99).values())
    # a species filter (the index keeps every species here; the filter acts per record, metamlst.py:114)
    sp = idx.loci[0][0]
    _, wantf = host_stats(idx, TypingArgs(filter=sp), path)
    _, gotf = device_stats(eng, path, sp, chunk_bytes=chunk)
    assert_stats_equal(gotf, wantf)
    assert int(wantf.counters[0]) < int(want.counters[0])
    # the same file gzipped, and the same records in another order
    with gzip.open(path + ".gz", "wb", compresslevel=1) as z:
        z.write(open(path, "rb").read())
    n, gotz = device_stats(eng, path + ".gz", chunk_bytes=chunk)
    assert n == 20_000
    assert_stats_equal(gotz, want)
    order = np.random.default_rng(3).permutation(len(recs))
    shuffled = write_sam(tmp_path / "shuffled.sam", refs, [recs[i] for i in order])
    n, gots = device_stats(eng, shuffled, chunk_bytes=chunk)
    assert n == 20_000
    # sums, hits and counters do not depend on the order; locus_first follows it, and so does the length sequenceBank keeps for a
    # read name that comes twice on a locus (the last record's, Q3) -- on the host reader as on the device
    wants = host_stats(idx, None, shuffled)[1]
    assert_stats_equal(gots, wants)
    assert np.array_equal(gots.sum_score, want.sum_score) and np.array_equal(gots.n_hits, want.n_hits)
    assert np.array_equal(gots.counters[:2], want.counters[:2])
    dev_s = eng.pileup_sam_file(shuffled, chosen, chunk_bytes=chunk)
    assert all(np.array_equal(dev_s[a], ref[a]) for a in ref)


# ------------------------------------------------------------------ 3. cuts
def test_two_chunks_cut_at_every_byte(gold):
    idx, eng = gold
    a0, a1 = idx.label(0), idx.label(idx.n_alleles - 1)
    names = [a0, a1]
    text = (header(names) + line(rec("q1", a0, 200, SEQ60[:55])) + "\r\n" + line(rec("q2", a1, 190, SEQ60, xm=1)) + "\n@CO\ta comment between records\n"
            + line(rec("q1", a0, 180, SEQ60[:52]))).encode()
    assert len(text) < 1500 and not text.endswith(b"\n")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        _, want = host_stats(idx, None, put(d + "/c.sam", text))
    assert int(want.n_hits.sum()) == 3 and int(want.locus_first.min()) == 0
    n, whole = chunks_stats(eng, idx, names, [text])
    assert n == 3
    assert_stats_equal(whole, want)
    for c in range(len(text) + 1):
        n, got = chunks_stats(eng, idx, names, [text[:c], text[c:]])
        assert n == 3, c
        assert_stats_equal(got, want)


# ------------------------------------------------------------------ 4. edges of the line table
def padded(r, size):
    """the record's line made `size` bytes long (its LF counted) by a ZZ:Z: column"""
    base = line(r)
    fill = size - 1 - len(base) - len("\tZZ:Z:")
    assert fill >= 0
    return line(r, ["ZZ:Z:" + "z" * fill]) + "\n"


def edge_records(idx, n):
    """n records of which only the last three are accepted, each on a locus of its own: locus_first tells their record indices"""
    loci = [l for l in range(idx.n_loci)][:3]
    recs = [rec("q%d" % k, idx.label(k % idx.n_alleles), 5) for k in range(n - 3)]
    recs += [rec("last%d" % j, idx.label(int(idx.locus_begin[l])), 250 - j) for j, l in enumerate(loci)]
    return recs


@pytest.mark.parametrize("shift", [-1, 0, 1], ids=["lf-before-last-byte", "lf-on-last-byte", "lf-on-first-byte"])
def test_line_feeds_at_the_block_boundaries(gold, tmp_path, shift):
    idx, eng = gold
    names = [idx.label(a) for a in range(idx.n_alleles)]
    recs = edge_records(idx, 9)
    head = header(names)
    # the LF of record k stands at byte (k + 1) * FQ_BLOCK - 1 + shift of the file (whose first byte is the first of a block)
    first = ((len(head) + 200) // FQ_BLOCK + 1) * FQ_BLOCK + shift - len(head)
    text = (head + padded(recs[0], first) + "".join(padded(r, FQ_BLOCK) for r in recs[1:])).encode()
    lfs = [i for i, b in enumerate(text) if b == 10 and i >= len(head)]
    assert all((i + 1 - shift) % FQ_BLOCK == 0 for i in lfs) and len(lfs) == 9
    path = put(tmp_path / "e.sam", text)
    _, want = host_stats(idx, None, path)
    assert sorted(int(x) for x in want.locus_first if x < 100) == [6, 7, 8]
    n, got = device_stats(eng, path)
    assert n == 9
    assert_stats_equal(got, want)
    # the second chunk begins with an LF / the first one ends with it; the last line without its LF
    for cut in (lfs[3], lfs[3] + 1, lfs[5] - 1):
        for body in (text, text[:-1]):
            n, got = chunks_stats(eng, idx, names, [body[:cut], body[cut:]])
            assert n == 9, (cut, len(body))
            assert_stats_equal(got, want)


@pytest.mark.parametrize("n_rec", [252, 253, 254, 255, 256, 257])
def test_record_index_at_the_edges_of_256_lines(gold, tmp_path, n_rec):
    # (three lines that are no records: the files hold 255 .. 260 lines, 252 .. 257 records)
    idx, eng = gold
    names = [idx.label(a) for a in range(idx.n_alleles)]
    recs = edge_records(idx, n_rec)
    # the names come from the caller here: the file's own header names one contig that no record uses
    lines = [line(r) + "\n" for r in recs]
    text = HD + "@SQ\tSN:unused_x_1\tLN:5\n" + "".join(lines[:100]) + "@CO\tin between\n" + "".join(lines[100:])
    path = put(tmp_path / "n.sam", text)
    _, want = host_stats(idx, None, path)
    assert sorted(int(x) for x in want.locus_first if x < 10_000) == [n_rec - 3, n_rec - 2, n_rec - 1]
    n, got = chunks_stats(eng, idx, names, [text.encode()])
    assert n == n_rec
    assert_stats_equal(got, want)


def test_chunks_of_header_lines_only_without_any_lf_and_empty(gold, tmp_path):
    idx, eng = gold
    names = [idx.label(a) for a in range(idx.n_alleles)]
    recs = edge_records(idx, 12)
    head = header(names).encode()
    body = "".join(line(r) + "\n" for r in recs).encode()
    text = head + body
    _, want = host_stats(idx, None, put(tmp_path / "h.sam", text))
    lf = body.index(b"\n")
    cases = {
        "header-only chunk": [head, body],
        "two header-only chunks": [head[:len(HD)], head[len(HD):], body],
        "a chunk without LF": [head + body[:5], body[5:lf - 3], body[lf - 3:]],
        "chunks of one byte without LF": [head + body[:5], body[5:6], body[6:7], body[7:]],
        "empty final chunk": [text, b""],
        "empty chunks everywhere": [b"", head, b"", body, b""],
        "no LF at the end, empty final chunk": [text[:-1], b""],
        "the last LF alone": [text[:-1], b"\n"],
    }
    for what, pieces in cases.items():
        n, got = chunks_stats(eng, idx, names, pieces)
        assert n == 12, what
        assert_stats_equal(got, want)
    # nothing at all, and a header without records
    for pieces in ([b""], [head], [head[:-1]]):
        n, got = chunks_stats(eng, idx, names, pieces)
        assert n == 0 and int(got.n_hits.sum()) == 0 and int(got.counters[0]) == 0


# ------------------------------------------------------------------ 5. head room
def test_a_line_as_long_as_the_head_room_and_one_byte_more(gold, tmp_path):
    from metamlst_amd.engine import MlstError
    idx, eng = gold
    names = [idx.label(a) for a in range(idx.n_alleles)]
    recs = edge_records(idx, 6)
    head = header(names)

    def build(size):      # record 4 (an accepted one) is `size` bytes long, its LF not counted
        ls = [line(r) + "\n" for r in recs]
        ls[4] = padded(recs[4], size + 1)
        assert len(ls[4]) == size + 1
        return (head + "".join(ls)).encode(), len(head) + sum(len(x) for x in ls[:4])

    text, at = build(MAX_LINE)
    path = put(tmp_path / "fits.sam", text)
    _, want = host_stats(idx, None, path)
    for pieces in ([text], [text[:at + MAX_LINE // 2], text[at + MAX_LINE // 2:]], [text[:at + 7], text[at + 7:at + MAX_LINE - 1], text[at + MAX_LINE - 1:]]):
        n, got = chunks_stats(eng, idx, names, pieces)
        assert n == 6
        assert_stats_equal(got, want)
    n, got = device_stats(eng, path, chunk_bytes=300_000)      # (the line straddles four chunks)
    assert n == 6
    assert_stats_equal(got, want)
    chosen = sorted({int(idx.locus_begin[l]) for l in range(3)})
    smp = samin.AlignmentSample(idx).add_file(path)
    dev, host = eng.pileup_sam_file(path, chosen, chunk_bytes=300_000), smp.pileup(eng, chosen)
    assert all(np.array_equal(dev[a], host[a]) for a in chosen) and sum(int(v.sum()) for v in dev.values()) > 0
    long_text, at = build(MAX_LINE + 1)
    for pieces in ([long_text], [long_text[:at + MAX_LINE // 2], long_text[at + MAX_LINE // 2:]], [long_text[:at + MAX_LINE + 1], long_text[at + MAX_LINE + 1:]]):
        with pytest.raises(MlstError, match=r"\(-5\): a SAM line of more than %d bytes" % MAX_LINE):
            chunks_stats(eng, idx, names, pieces)
    with pytest.raises(MlstError, match="a SAM line of more than"):
        eng.pileup_sam_file(put(tmp_path / "long.sam", long_text), chosen)
    # a good file right afterwards
    n, got = device_stats(eng, path)
    assert n == 6
    assert_stats_equal(got, want)


# ------------------------------------------------------------------ 6. names table
def test_names_table_one_name_prefixes_and_three_thousand_long_names(tmp_path):
    from metamlst_amd import synth
    sp, g = "S" + "p" * 40, "G" + "e" * 40
    synth.make_db(str(tmp_path / "n.db"), {"sp": [("g", 300)], sp: [(g, 300)]}, {("sp", "g"): 11, (sp, g): 3000}, 1)
    idx = load_index(str(tmp_path / "n.db"))
    assert idx.n_alleles == 3011
    eng = make_engine(idx)
    long_names = ["%s_%s_%d" % (sp, g, k) for k in range(1, 3001)]

    def check(names, used):
        recs = [rec("q%d" % k, n, 150 + 7 * k) for k, n in enumerate(used)]
        path = write_sam(tmp_path / "t.sam", [(n, 500) for n in names], recs)
        assert samin.read_sam_header(path) == names
        _, want = host_stats(idx, None, path)
        assert int((want.n_hits > 0).sum()) == len(set(used))
        n, got = device_stats(eng, path)
        assert n == len(used)
        assert_stats_equal(got, want)

    check(["sp_g_1"], ["sp_g_1", "sp_g_1"])                                                   # n_ref = 1
    check(["sp_g_1", "sp_g_10", "sp_g_11"], ["sp_g_11", "sp_g_1", "sp_g_10", "sp_g_1"])      # prefixes of one another
    check(["sp_g_11", "sp_g_10", "sp_g_1"], ["sp_g_1", "sp_g_10", "sp_g_11"])
    check(long_names, [long_names[0], long_names[-1], long_names[1499], long_names[2998], long_names[1]])
    check(long_names + ["sp_g_%d" % k for k in range(1, 12)], [long_names[-1], "sp_g_1", long_names[0], "sp_g_11", long_names[2000]])
    # a name of the header that comes twice, and one that no record uses
    check(["sp_g_2", "sp_g_3", "sp_g_2", "unused_g_1"], ["sp_g_2", "sp_g_3"])


# ------------------------------------------------------------------ 7. hand-over
def _cli(args):
    from metamlst_amd.cli import main
    return main(args)


def _nfo(out, name):
    p = out + "/%s.nfo" % name
    return open(p, "rb").read() if os.path.exists(p) else None


CR_, HI_, NUL_ = "\r", "é", "\0"
# reason -> (how the planted record's line is made from the record, words of the library's message)
PLANTS = {
    "cr-inside": (lambda r: line(r).replace("\t255\t", "\t25" + CR_ + "5\t", 1), "a CR that does not stand in front of an LF"),
    "byte-0x80": (lambda r: line((r[0] + HI_,) + r[1:]), "a byte that is not 7-bit text"),
    "nul": (lambda r: line((r[0] + NUL_,) + r[1:]), "a byte that is not 7-bit text"),
    "14-columns": (lambda r: line(r[:8] + (r[8][:3],)), "fewer than 15 columns"),
    "empty-line": (lambda r: "", "fewer than 15 columns"),
    "flag-plus": (lambda r: line(r[:1] + ("+5",) + r[2:]), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "pos-space": (lambda r: line(r[:3] + (" 5",) + r[4:]), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "pos-underscore": (lambda r: line(r[:3] + ("5_0",) + r[4:]), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "pos-ten-digits": (lambda r: line(r[:3] + ("1000000000",) + r[4:]), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "col12-float": (lambda r: line(r[:8] + (["AS:i:1.5"] + r[8][1:],)), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "col12-one-colon": (lambda r: line(r[:8] + (["AS:5"] + r[8][1:],)), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "col15-text": (lambda r: line(r[:8] + (r[8][:3] + ["YT:Z:UU"] + r[8][4:],)), "a FLAG, POS, 12th or 15th column that is not a plain integer"),
    "rname-unknown": (lambda r: line(r[:2] + ("spQ_gQ_1",) + r[3:]), "an RNAME that is not among the header's @SQ names"),
    "rname-star": (lambda r: line(r[:2] + ("*",) + r[3:]), "an RNAME that is not among the header's @SQ names"),
    "rname-two-parts": (lambda r: line(r[:2] + ("a_b",) + r[3:]), "a contig name that does not split in three at '_'"),
    "as-by-name": (lambda r: line(r, ["AS:i:7x"]), "an AS / XM tag that is not a plain integer"),
    "xm-by-name": (lambda r: line(r, ["XM:Z:"]), "an AS / XM tag that is not a plain integer"),
    "cigar-byte": (lambda r: line(r[:5] + ("4M2Q4M",) + r[6:]), "a CIGAR byte that is no operation"),
    "cigar-length": (lambda r: line(r[:5] + ("268435456M",) + r[6:]), "a CIGAR operation of 2\\^28 bases or more"),
    "qual-length": (lambda r: line(r[:7] + (r[7][:-1],) + r[8:]), "a QUAL that is neither \\* nor as long as SEQ"),
    "qual-byte": (lambda r: line(r[:7] + (" " + r[7][1:],) + r[8:]), "a QUAL byte below 33"),
}


@pytest.fixture(scope="module")
def handover_base(gold):
    idx, _ = gold
    names = [idx.label(a) for a in range(idx.n_alleles)] + ["a_b"]
    chosen = chosen_set(idx)
    # 800 records on loaded contigs; those at 0, 300 and 700 lie on a contig that the pile-up chooses -- the test's and, as the
    # records on these contigs score highest, the command's
    recs = []
    for k in range(800):
        a = chosen[k % len(chosen)] if k in (0, 300, 700) else (k * 7) % idx.n_alleles
        recs.append(rec("q%d" % (k // 2), idx.label(a), 250 if a in chosen else 120 + k % 100, SEQ60, pos=1 + k % 30, xm=k % 4))
    return names, chosen, recs


@pytest.mark.parametrize("why", list(PLANTS))
def test_hand_over_names_the_smallest_record_and_the_command_ends_as_the_host_reader(gold, handover_base, tmp_path, capsys, why):
    from metamlst_amd.engine import HostPathNeeded
    idx, eng = gold
    names, chosen, recs = handover_base
    make, words = PLANTS[why]
    dbp = gu.golden_db()
    for tag, where in (("r0", (0,)), ("r300", (300,)), ("r300r700", (300, 700))):
        lines = [make(r) if k in where else line(r) for k, r in enumerate(recs)]
        path = put(tmp_path / ("%s_%s.sam" % (why, tag)), (header(names) + "\n".join(lines) + "\n").encode("utf-8"))
        eng.reset_sample()
        with pytest.raises(HostPathNeeded, match="host path needed: %s at record %d$" % (words, where[0])):
            eng.submit_sam_file(path, chunk_bytes=40_000)
            eng.pileup_sam_file(path, chosen, chunk_bytes=40_000)
        eng.reset_sample()
        # the host reader on the file, through the typing tail: an exception, or the .nfo the command has to write
        out = str(tmp_path / ("out_%s_%s" % (why, tag)))
        try:
            smp = samin.AlignmentSample(idx, TypingArgs()).add_file(path)
            res = type_sample(idx, smp.stats(), lambda ch: smp.pileup(eng, ch), mdb.metaMLST_db(dbp), "%s_%s" % (why, tag), TypingArgs())
            host_exc, want_nfo = None, "".join(r.nfo_line for r in res if r.written).encode() or None
        except Exception as e:      # noqa: BLE001 -- whatever the host reader raises is what the command has to raise
            host_exc = type(e)
        capsys.readouterr()
        if host_exc is None:
            assert _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--quiet"]) == 0
            assert _nfo(out, "%s_%s" % (why, tag)) == want_nfo
        else:
            with pytest.raises(host_exc):
                _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--quiet"])
        err = capsys.readouterr().err
        assert "host path needed" in err and "at record %d" % where[0] in err and "on the host instead" in err


def test_odd_but_legal_lines_stay_on_the_device(gold, tmp_path):
    idx, eng = gold
    names = [idx.label(a) for a in range(idx.n_alleles)]
    chosen = chosen_set(idx)
    lab = [idx.label(a) for a in chosen]
    seq = SEQ60
    no_xs = ["AS:i:150", "XN:i:0", "XM:i:9", "XO:i:1", "XG:i:0", "NM:i:0", "YT:Z:UU"]      # XS absent: the 15th column is XO
    recs = [
        rec("colon", lab[0], 0, seq, tags=["AS:i:155:7", "XS:i:1", "XN:i:0", "XM:i:1:x", "XO:i:0"]),
        rec("no-xs", lab[1], 0, seq, tags=no_xs),
        rec("lower", lab[2], 160, seq.lower()),
        rec("eq-x", lab[0], 170, seq, cigar="5=1X10M2I2M", pos=3),
        rec("stars", lab[1], 180, "*", qual="*", cigar="*"),
        rec("no-qual", lab[1], 181, seq, qual="*"),
        rec("negative", lab[2], -3, seq, xm=0),
        rec("negative-by-name", lab[2], 150, seq, tags=["AS:i:150", "XS:i:1", "XN:i:0", "XM:i:0", "XO:i:0", "AS:i:-7"]),
        rec("last-wins", lab[0], 150, seq, tags=["AS:i:9", "XS:i:1", "XN:i:0", "XM:i:0", "XO:i:0", "AS:i:junk", "XM:i:junk", "AS:i:190", "XM:i:1"]),
        rec("hard-clip-pad", lab[1], 175, seq, cigar="3H2S10M1P4D6M2N2M5H", pos=7),
        rec("pos-0", lab[0], 177, seq, pos=0),
        rec("pos-negative", lab[0], 178, seq, pos=-4),
        rec("past-the-end", lab[1], 179, seq, pos=100_000),
        rec("trailing-digits", lab[2], 182, seq, cigar="20M7"),
        rec("empty-tag-column", lab[0], 183, seq, tags=["AS:i:183", "XS:i:1", "XN:i:0", "XM:i:0", "XO:i:0", "", "A", "AS", "AS:", "XM:i"]),
        rec("minus-zero", lab[1], 184, seq, tags=["AS:i:184", "XS:i:1", "XN:i:0", "XM:i:-0", "XO:i:0"]),
        rec("nine-digits", lab[2], 185, seq, tags=["AS:i:999999999", "XS:i:1", "XN:i:0", "XM:i:-999999999", "XO:i:0"]),
    ]
    path = write_sam(tmp_path / "odd.sam", [(n, 500) for n in names], recs)
    smp, want = host_stats(idx, None, path)
    assert int(want.counters[0]) == len(recs)
    n, got = device_stats(eng, path)
    assert n == len(recs)
    assert_stats_equal(got, want)
    ref = samin_ref.pileup_python(idx, smp, chosen)
    host = smp.pileup(eng, chosen)
    dev = eng.pileup_sam_file(path, chosen)
    assert sum(int(v.sum()) for v in ref.values()) > 100
    for a in chosen:
        assert np.array_equal(dev[a], ref[a]) and np.array_equal(dev[a], host[a]), a
    # a CIGAR that asks for more bases than SEQ holds (the per-base loop of samin_ref does not take it: the host path alone)
    short = write_sam(tmp_path / "short.sam", [(n, 500) for n in names], recs + [rec("short-seq", lab[2], 176, SEQ60[:50], cigar="40M5I30M")])
    smp2, want2 = host_stats(idx, None, short)
    assert_stats_equal(device_stats(eng, short)[1], want2)
    dev2, host2 = eng.pileup_sam_file(short, chosen), smp2.pileup(eng, chosen)
    assert all(np.array_equal(dev2[a], host2[a]) for a in chosen) and int(dev2[chosen[2]].sum()) > int(dev[chosen[2]].sum())
    # CRLF everywhere: the same answers
    crlf = put(tmp_path / "crlf.sam", open(path, "rb").read().replace(b"\n", b"\r\n"))
    n, got = device_stats(eng, crlf)
    assert n == len(recs)
    assert_stats_equal(got, host_stats(idx, None, crlf)[1])
    devc = eng.pileup_sam_file(crlf, chosen)
    assert all(np.array_equal(devc[a], ref[a]) for a in chosen)


# ------------------------------------------------------------------ 8. CLI
@pytest.mark.parametrize("case", [CASES[0], CASES[-1]], ids=lambda c: os.path.basename(c))
def test_cli_types_sam_and_gzipped_sam_on_the_device(case, tmp_path, capsys, monkeypatch):
    from metamlst_amd import samin as product
    dbp = gu.golden_db()
    argv = [a for a in json.load(open(os.path.join(case, "args.json"))) if a != "--log"]
    sam, _ = with_sq_lines(os.path.join(case, "input.sam"), tmp_path / "sampleX.sam")
    gz = str(tmp_path / "gz") + "/sampleX.sam.gz"
    os.mkdir(str(tmp_path / "gz"))
    with gzip.open(gz, "wb") as z:
        z.write(open(sam, "rb").read())
    made = []
    real = product.SamSample.add_file

    def counted(self, path, *a, **k):
        made.append(self)
        return real(self, path, *a, **k)

    monkeypatch.setattr(product.SamSample, "add_file", counted)
    host_calls = []
    real_host = product.AlignmentSample.add_file
    monkeypatch.setattr(product.AlignmentSample, "add_file", lambda self, p: (host_calls.append(p), real_host(self, p))[1])
    # The yardstick: the host reader on the same file through the same tail.  (The case's expected.nfo was made from its
    # counts.json, not from a pile-up of input.sam -- test_golden_cases_through_the_device_path holds the device's statistics
    # against it; piled up from input.sam itself, by the host reader as by the device, these samples pass no species and the
    # command writes no .nfo.  Where the reference left a log table, the command's table must be that one.)
    targs, prm = parse_args(json.load(open(os.path.join(case, "args.json"))))
    idx = load_index(dbp, targs.filter.split(",") if targs.filter else None)
    eng = make_engine(idx, prm)
    smp = samin.AlignmentSample(idx, targs)
    real_host(smp, sam)
    res = type_sample(idx, smp.stats(), lambda ch: smp.pileup(eng, ch), mdb.metaMLST_db(dbp), "sampleX", targs)
    want = ("".join(r.nfo_line for r in res if r.written).encode() or None, log_table(idx, smp.stats(), targs, "x").encode().split(b"\r\n", 1)[1])
    logf = os.path.join(case, "expected_log.out")
    if os.path.exists(logf):
        assert want[1] == open(logf, "rb").read()

    def typed(path, out):
        assert _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--quiet", "--log"] + argv) == 0
        nfos, logs = glob.glob(out + "/*.nfo"), glob.glob(out + "/*.out")
        assert len(nfos) <= 1 and len(logs) == 1
        name = os.path.basename(logs[0]).rsplit("_", 1)[0]
        return (open(nfos[0], "rb").read().replace(name.encode(), b"sampleX") if nfos else None, open(logs[0], "rb").read().split(b"\r\n", 1)[1])

    for k, path in enumerate((sam, gz)):
        assert typed(path, str(tmp_path / ("out%d" % k))) == want
        assert len(made) == k + 1 and made[k].n_records == smp.n_records and not host_calls      # the device path typed it, the host reader never ran
    io = capsys.readouterr()
    assert "host" not in io.err
    # the file as it is, without @SQ lines: the host reader at once, and not a word about it
    assert typed(os.path.join(case, "input.sam"), str(tmp_path / "out_plain")) == want
    assert len(made) == 2 and len(host_calls) == 1 and "host" not in capsys.readouterr().err


def passing_records(idx, chosen):
    """reads cut from the chosen alleles themselves (they score highest) and weaker records on their neighbours: the sample passes"""
    recs = []
    for k in range(600):
        a = chosen[k % len(chosen)]
        s = idx.sequence(a)
        s = s.decode() if isinstance(s, bytes) else s
        at = (k // len(chosen) * 7) % (len(s) - 59)
        recs.append(rec("q%d" % k, idx.label(a), 120, s[at:at + 60], pos=at + 1))
        recs.append(rec("q%d" % k, idx.label(a + 1), 100, s[at:at + 60], pos=at + 1, xm=2))
    return recs


def test_cli_writes_the_host_readers_nfo_from_the_device_path(gold, handover_base, tmp_path, capsys, monkeypatch):
    """a sample that passes (two species written): the .nfo of the command, typed on the device, is the host reader's"""
    from metamlst_amd import samin as product
    idx, eng = gold
    names, chosen, _ = handover_base
    dbp = gu.golden_db()
    recs = passing_records(idx, chosen)
    path = put(tmp_path / "passes.sam", header(names) + "\n".join(line(r) for r in recs) + "\n")
    smp = samin.AlignmentSample(idx, TypingArgs()).add_file(path)
    res = type_sample(idx, smp.stats(), lambda ch: smp.pileup(eng, ch), mdb.metaMLST_db(dbp), "passes", TypingArgs())
    want = "".join(r.nfo_line for r in res if r.written).encode()
    assert sum(1 for r in res if r.written) == 2 and want
    monkeypatch.setattr(product.AlignmentSample, "add_file", lambda self, p: pytest.fail("the host reader ran"))
    for k, p in enumerate((path, path + ".gz")):
        if k:
            with gzip.open(p, "wb") as z:
                z.write(open(path, "rb").read())
        out = str(tmp_path / ("out%d" % k))
        assert _cli(["type", p, "--alignments", "-d", dbp, "-o", out, "--quiet"]) == 0
        nfos = glob.glob(out + "/*.nfo")
        assert len(nfos) == 1 and open(nfos[0], "rb").read().replace(os.path.basename(nfos[0])[:-4].encode(), b"passes") == want
    assert "host" not in capsys.readouterr().err


def test_kernel_times_count_the_new_kernels(gold, tmp_path):
    idx, eng = gold
    refs, recs = zoo(idx, 500)
    path = write_sam(tmp_path / "k.sam", refs, recs)
    eng.set_profiling(1)
    try:
        eng.reset_kernel_time()
        device_stats(eng, path)
        assert eng.kernel_time(15)[1] == 2 and eng.kernel_time(16)[1] == 1 and eng.kernel_time(17)[1] == 0
        eng.pileup_sam_file(path, chosen_set(idx))
        assert eng.kernel_time(15)[1] == 4 and eng.kernel_time(16)[1] == 1 and eng.kernel_time(17)[1] == 1
        assert all(eng.kernel_time(w)[0] > 0 for w in (15, 16, 17))
    finally:
        eng.set_profiling(0)
        eng.reset_kernel_time()


# ------------------------------------------------------------------ 9. state hygiene
def test_state_hygiene_between_sam_fastq_and_bam_samples(tmp_path):
    import fixtures as fx
    from metamlst_amd import synth
    from metamlst_amd.engine import MlstError
    from test_bam_gpu import STAT_FIELDS
    db, idx = fx.ecoli_small(40)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][2], size=60_000)
    b, q = synth.sample_reads(g, 4000)
    fb, fq, off = synth.flatten_reads(b, q)
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles)]
    recs = []
    for k in range(3000):
        a = (k * 7) % idx.n_alleles
        s = idx.sequence(a)
        s = s.decode() if isinstance(s, bytes) else s
        recs.append(("q%d" % (k // 3), 0, refs[a][0], 1 + k % 50, 255, "100M", s[k % 50:k % 50 + 100], "I" * 100,
                     ["AS:i:%d" % (150 + k % 50), "XS:i:3", "XN:i:0", "XM:i:%d" % (k % 7), "XO:i:0", "XG:i:0", "NM:i:0", "YT:Z:UU"]))
    sam = write_sam(tmp_path / "s.sam", refs, recs)
    bam = write(tmp_path / "s.bam", refs, recs[:2000])
    chosen = sorted({int(idx.locus_begin[l]) for l in range(idx.n_loci)})

    def sam_stats(e):
        e.reset_sample(); e.submit_sam_file(sam, chunk_bytes=200_000); return e.stats()

    def fastq_stats(e):
        e.reset_sample(); e.submit_reads(fb, fq, off); return e.stats()

    def bam_stats(e):
        e.reset_sample(); e.submit_bam_file(bam); return e.stats()

    fresh = {"sam": sam_stats(make_engine(idx)), "fastq": fastq_stats(make_engine(idx)), "bam": bam_stats(make_engine(idx))}
    fresh_pile = make_engine(idx).pileup_sam_file(sam, chosen)
    assert_stats_equal(fresh["sam"], host_stats(idx, None, sam)[1])
    eng = make_engine(idx)
    for kind, fn in (("sam", sam_stats), ("fastq", fastq_stats), ("bam", bam_stats), ("sam", sam_stats)):
        got = fn(eng)
        for f in STAT_FIELDS:
            assert np.array_equal(getattr(got, f), getattr(fresh[kind], f)), (kind, f)
        assert np.array_equal(got.counters, fresh[kind].counters), kind
    pile = eng.pileup_sam_file(sam, chosen)
    assert all(np.array_equal(pile[a], fresh_pile[a]) for a in chosen)
    bpile = eng.pileup_bam_file(bam, chosen)      # (the counts a fetch hands out are the last finished stream's, of either format)
    assert sum(int(v.sum()) for v in bpile.values()) < sum(int(v.sum()) for v in pile.values())
    # while a SAM stream is open the other entries refuse ...
    names = samin.read_sam_header(sam)
    tables = samin.bam_ref_table(idx, names, None)
    eng.reset_sample()
    eng.sam_open(1, names, *tables)
    eng.submit_sam_text(open(sam, "rb").read()[:5000], False)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.submit_fastq(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.submit_reads(fb, fq, off)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.bam_open(1, *tables)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.sam_open(1, names, *tables)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.submit_bam_bgzf(np.fromfile(bam, np.uint8), final=True)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.set_bgzf_verify(True)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.set_read_tiling(150, 50)
    with pytest.raises(MlstError, match="a SAM stream is open"):
        eng.bam_set_capacity(10)
    # ... and the stream goes on where it was
    n = eng.submit_sam_text(open(sam, "rb").read()[5000:], True)
    assert n > 2900
    assert np.array_equal(eng.stats().sum_score, fresh["sam"].sum_score)
    # mlst_sam_open refuses while a FASTQ stream is open, and the text entry needs an open SAM stream
    eng.reset_sample()
    eng.submit_fastq_stream(b"@r\nACGT\n+\nII", False)
    with pytest.raises(MlstError, match="a FASTQ stream is open"):
        eng.sam_open(1, names, *tables)
    eng.reset_sample()
    with pytest.raises(MlstError, match="no SAM stream is open"):
        eng.submit_sam_text(b"x\n", True)
    eng.bam_open(1, *tables)
    with pytest.raises(MlstError, match="no SAM stream is open"):
        eng.submit_sam_text(b"x\n", True)
    eng.reset_sample()
    # the list's bound holds for SAM text too
    eng.bam_set_capacity(100)
    with pytest.raises(MlstError, match=r"\(-4\): more than 100 accepted records on known loci"):
        eng.submit_sam_file(sam)
    eng.bam_set_capacity(0)
    assert np.array_equal(sam_stats(eng).sum_score, fresh["sam"].sum_score)
