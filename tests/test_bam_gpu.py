"""BGZF BAM typed on the device (mlst_bam_open / mlst_submit_bam_bgzf / mlst_bam_pileup_fetch): inflate, record split, the
accumulation of metamlst.py:101-130 and the pile-up of the chosen contigs against the host path (samin.AlignmentSample, pinned by
the reference's own .nfo files in tests/golden/typing) and the literal loop of tests/samin_ref.py."""
import glob
import json
import os
import struct

import numpy as np
import pytest

import bam_writer
import golden_util as gu
import samin_ref
from metamlst_amd import db as mdb
from metamlst_amd import samin
from metamlst_amd.index import load_index
from metamlst_amd.typing import TypingArgs, log_table, type_sample
from test_golden_typing import parse_args

CASES = sorted(glob.glob(os.path.join(gu.GOLD, "typing", "case*")))
STAT_FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")


# ------------------------------------------------------------------ helpers (no device needed)
def sam_to_bam(sam: str, bam: str, extra_refs=()):
    """input.sam -> BAM with bam_writer: the header's @SQ lines if any, else the contigs in order of appearance"""
    als = list(samin.read_alignments(sam))
    refs = []
    for al in als:
        if al.rname != "*" and al.rname not in [r[0] for r in refs]:
            refs.append((al.rname, 5000))
    refs += [r for r in extra_refs if r[0] not in [x[0] for x in refs]]
    recs = [(al.qname, al.flag, al.rname, al.pos, 255, al.cigar, al.seq, al.qual, list(al.tags)) for al in als]
    bam_writer.write_bam(bam, "@HD\tVN:1.0\tSO:unsorted\n", refs, recs)
    return refs, recs


def zoo(idx, n, seed=11):
    """test_samin._records-style records on the contigs of the index, on contigs that are not in it, and on known loci with
    unknown allele numbers; repeated read names on several loci; l_seq = 0 records; XS present / absent (the 4th field is XM / XO)."""
    rng = np.random.default_rng(seed)
    labels = [idx.label(a) for a in range(idx.n_alleles)]
    lens = {idx.label(a): int(idx.off[a + 1] - idx.off[a]) for a in range(idx.n_alleles)}
    sp0, g0 = idx.loci[0]
    other = ["spZ_g9_1", "spZ_g9_2", "%s_%s_99999" % (sp0, g0), "%s_gNEW_1" % sp0]
    refs = [(l, lens[l]) for l in labels] + [(o, 500) for o in other]
    names = [r[0] for r in refs]
    Ls = rng.integers(1, 161, size=n); pick = rng.integers(0, len(names), size=n); ASs = rng.integers(-5, 300, size=n); XSs = rng.integers(0, 300, size=n)
    XMs = rng.integers(0, 9, size=n); XOs = rng.integers(0, 3, size=n); poss = rng.integers(1, 380, size=n)
    letters = np.array(list("ACGTN")); recs = []
    for k in range(n):
        L = int(Ls[k])
        seq = "".join(rng.choice(letters, size=L, p=[.24, .24, .24, .24, .04]))
        qual = "".join(map(chr, (33 + rng.integers(0, 42, size=L)).tolist()))
        kind = k % 5
        if kind == 1 and L > 20:
            cigar = "5S%dM2D%dM3S" % ((L - 8) // 2, L - 8 - (L - 8) // 2)
        elif kind == 2 and L > 20:
            cigar = "4=1X%dM1I5M" % (L - 11)
        elif kind == 3 and L > 30:
            cigar = "2H10M100N%dM1P" % (L - 10)
        else:
            cigar = "%dM" % L
        tags = ["AS:i:%d" % ASs[k]] + (["XS:i:%d" % XSs[k]] if k % 3 else []) + \
               ["XN:i:0", "XM:i:%d" % XMs[k], "XO:i:%d" % XOs[k], "XG:i:0", "NM:i:70000", "YT:Z:UU", "ZA:A:x", "ZF:f:1.5"]
        if k % 17 == 0:
            qual = "*"
        if k % 29 == 0:
            seq, qual, cigar = "*", "*", "*"
        recs.append(("read%d" % (k // 20), [0, 16, 256, 272][k % 4], names[int(pick[k])], int(poss[k]), 255, cigar, seq, qual, tags))
    return refs, recs


def write(path, refs, recs):
    bam_writer.write_bam(str(path), "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs), refs, recs)
    return str(path)


def write_sam(path, refs, recs):
    with open(str(path), "w") as f:
        f.write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs))
        for r in recs:
            f.write("\t".join([r[0], str(r[1]), r[2], str(r[3]), str(r[4]), r[5], "*", "0", "0", r[6], r[7]] + list(r[8])) + "\n")
    return str(path)


def flip_in_block(raw: bytes, k: int) -> bytes:
    """the file with one byte of the text of its k-th BGZF block changed (bit 5 of a byte in its middle): the block rebuilt as a stored
    deflate block that keeps the old trailer, so it inflates to the right length and fails only its CRC-32"""
    import zlib
    at = 0
    for _ in range(k):
        at += struct.unpack_from("<H", raw, at + 16)[0] + 1
    bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
    text = bytearray(zlib.decompress(raw[at + 18:at + bsize - 8], -15))
    at_x = text.find(b"xxxxxxxx", len(text) // 2)      # (a letter of a reference name where the block holds the long names of the tests)
    text[at_x if at_x >= 0 else len(text) // 2] ^= 0x20
    comp = b"\x01" + struct.pack("<HH", len(text), len(text) ^ 0xFFFF) + bytes(text)
    blk = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp + bytes(raw[at + bsize - 8:at + bsize])
    return bytes(raw[:at]) + blk + bytes(raw[at + bsize:])


def record_size(r):
    qn, _, _, _, _, cigar, seq, _, tags = r
    nops = sum(1 for ch in ("" if cigar == "*" else cigar) if not ch.isdigit())
    L = 0 if seq == "*" else len(seq)
    return 4 + 32 + len(qn) + 1 + 4 * nops + (L + 1) // 2 + L + sum(len(bam_writer._aux(t)) for t in tags)


def header_size(refs):
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    return 12 + len(text) + sum(9 + len(n) for n, _ in refs)


def host_stats(idx, targs, path):
    smp = samin.AlignmentSample(idx, targs).add_file(path)
    return smp, smp.stats()


def assert_stats_equal(got, want, first=True):
    for f in STAT_FIELDS if first else STAT_FIELDS[:3]:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert [int(x) for x in got.counters[:2]] == [int(x) for x in want.counters[:2]]


# ------------------------------------------------------------------ CPU
def test_bam_header_reader_returns_names_table_and_where_the_records_begin(tmp_path):
    idx = load_index(gu.golden_db())
    refs = [("spLong_gene%04d_%d" % (k, k) + "x" * 40, 1000 + k) for k in range(3000)] + [(idx.label(0), 10), ("a_b", 5)]
    _, recs = zoo(idx, 50)
    recs = [(r[0], r[1], refs[k % len(refs)][0], r[3], r[4], r[5], r[6], r[7], r[8]) for k, r in enumerate(recs)]
    path = write(tmp_path / "h.bam", refs, recs)
    names, coff, skip = samin.read_bam_header(path)
    assert names == [r[0] for r in refs] and header_size(refs) > 3 * 60000 and coff > 0
    import gzip
    whole = gzip.open(path, "rb").read()
    rest = gzip.GzipFile(fileobj=__import__("io").BytesIO(open(path, "rb").read()[coff:])).read()
    assert rest[skip:] == whole[header_size(refs):] and len(rest[skip:]) == sum(record_size(r) for r in recs)
    ra, rl, rf = samin.bam_ref_table(idx, names, None)
    assert ra[-2] == 0 and rl[-2] == int(idx.locus_id[0]) and rf[-2] == 1 and rf[-1] == 2 and ra[0] == -1 and rl[0] == -1 and rf[0] == 1
    sp = idx.loci[0][0]
    assert samin.bam_ref_table(idx, names, sp)[2][-2] == 1 and samin.bam_ref_table(idx, names, "nobody")[2][-2] == 0
    assert samin.is_bgzf_bam(path) and not samin.is_bgzf_bam(os.path.join(CASES[0], "input.sam"))


def test_the_zoo_raises_nowhere_on_the_host_path():
    idx = load_index(gu.golden_db())
    refs, recs = zoo(idx, 3000)
    smp = samin.AlignmentSample(idx)
    for r in recs:
        smp.add(samin.Alignment(r[0], r[1], r[2], r[3], r[5], r[6], r[7], r[8]))
    st = smp.stats()
    assert int(st.counters[0]) == 3000 and 0 < int(st.counters[1]) < 3000 and int(st.n_hits.sum()) > 100


# ------------------------------------------------------------------ GPU
def make_engine(idx, prm=None, verify=False):
    from metamlst_amd.engine import Engine
    eng = Engine(0, prm)
    eng.load_reference(idx)
    eng.set_bgzf_verify(verify)
    return eng


def device_stats(eng, path, filt=None, **kw):
    eng.reset_sample()
    n = eng.submit_bam_file(path, filt, **kw)
    return n, eng.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c) for c in CASES])
def test_golden_cases_through_the_device_path(case, tmp_path):
    targs, prm = parse_args(json.load(open(os.path.join(case, "args.json"))))
    dbp = gu.golden_db()
    idx = load_index(dbp, targs.filter.split(",") if targs.filter else None)
    sam = os.path.join(case, "input.sam")
    bam = str(tmp_path / "input.bam")
    sam_to_bam(sam, bam)
    _, want = host_stats(idx, targs, sam)
    eng = make_engine(idx, prm)
    n, got = device_stats(eng, bam, targs.filter or None)
    assert n == len(list(samin.read_alignments(sam)))
    assert_stats_equal(got, want)
    counts = json.load(open(os.path.join(case, "counts.json")))

    def pileup_fn(chosen):
        return {a: np.array(counts["%s_%s" % idx.loci[int(idx.locus_id[a])]], np.uint32) for a in chosen}

    res = type_sample(idx, got, pileup_fn, mdb.metaMLST_db(dbp), "sampleX", targs)
    assert "".join(r.nfo_line for r in res if r.written).encode() == open(os.path.join(case, "expected.nfo"), "rb").read()
    logf = os.path.join(case, "expected_log.out")
    if os.path.exists(logf):
        assert log_table(idx, got, targs, "x").encode().split(b"\r\n", 1)[1] == open(logf, "rb").read()


@pytest.fixture(scope="module")
def zoo_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("zoo")
    idx = load_index(gu.golden_db())
    refs, recs = zoo(idx, 200_000)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(recs))
    shuffled = [recs[i] for i in order]
    rid = {n: i for i, (n, _) in enumerate(refs)}
    by_pos = sorted(recs, key=lambda r: (rid[r[2]], r[3]))
    return idx, refs, {"zoo": write(d / "zoo.bam", refs, recs), "shuffled": write(d / "shuffled.bam", refs, shuffled), "sorted": write(d / "sorted.bam", refs, by_pos)}


def chosen_set(idx):
    return sorted({int(idx.locus_begin[l]) + (l % int(idx.locus_count[l])) for l in range(idx.n_loci)})


@pytest.mark.gpu
def test_record_zoo_statistics_and_pileup_equal_the_host_path(zoo_files):
    from metamlst_amd.engine import default_params
    idx, refs, files = zoo_files
    smp, want = host_stats(idx, None, files["zoo"])
    eng = make_engine(idx, verify=True)
    n, got = device_stats(eng, files["zoo"], chunk_bytes=3 << 20)
    assert n == 200_000
    assert_stats_equal(got, want)
    chosen = chosen_set(idx)
    ref = samin_ref.pileup_python(idx, smp, chosen)
    host = smp.pileup(eng, chosen)
    dev = eng.pileup_bam_file(files["zoo"], chosen, chunk_bytes=3 << 20)
    assert set(dev) == set(ref) and sum(int(v.sum()) for v in ref.values()) > 1000
    for a in ref:
        assert np.array_equal(dev[a], ref[a]) and np.array_equal(dev[a], host[a]), a
    assert eng.pileup_bam_file(files["zoo"], []) == {}
    p99 = default_params(); p99.minqual = 99
    e99 = make_engine(idx, p99)
    d99 = e99.pileup_bam_file(files["zoo"], chosen)
    assert all(int(v.sum()) == 0 for v in d99.values()) and all(int(v.sum()) == 0 for v in smp.pileup(e99, chosen, minqual=99).values())
    # a species filter (the index keeps every species here; the filter acts per record, metamlst.py:114)
    sp = idx.loci[0][0]
    targs = TypingArgs(filter=sp)
    _, wantf = host_stats(idx, targs, files["zoo"])
    _, gotf = device_stats(eng, files["zoo"], sp)
    assert_stats_equal(gotf, wantf)
    assert int(wantf.counters[0]) < int(want.counters[0])


@pytest.mark.gpu
def test_chunking_serial_mode_long_records_and_the_head_room(zoo_files, tmp_path, monkeypatch):
    idx, refs, files = zoo_files
    _, want = host_stats(idx, None, files["zoo"])
    eng = make_engine(idx)
    names, lo, skip = samin.read_bam_header(files["zoo"])
    table = samin.bam_ref_table(idx, names, None)
    data = np.fromfile(files["zoo"], np.uint8)[lo:]

    def feed(e, cuts):
        e.reset_sample()
        e.bam_open(1, *table, skip_bytes=skip)
        at, total = 0, 0
        for c in cuts + [data.size]:
            last = c == data.size
            n, used = e.submit_bam_bgzf(data[at:c], final=last, partial=not last)
            total += n; at += used
        assert at == data.size
        return total, e.stats()

    n1, one = feed(eng, [])
    rng = np.random.default_rng(8)
    cuts = sorted(int(x) for x in rng.integers(70_000, data.size - 70_000, size=9))
    n2, many = feed(eng, cuts)
    assert n1 == n2 == 200_000
    assert_stats_equal(one, want); assert_stats_equal(many, want)
    monkeypatch.setenv("MLST_BGZF_PIPE", "0")
    e0 = make_engine(idx)
    n3, serial = feed(e0, cuts)
    assert n3 == 200_000
    assert_stats_equal(serial, want)
    monkeypatch.delenv("MLST_BGZF_PIPE")
    # a record larger than a cell (long read), one larger than 64 KiB (long Z tag), in between ordinary ones
    _, recs = zoo(idx, 2000, seed=4)
    lab = idx.label(0)
    big_read = ("long1", 0, lab, 1, 255, "40000M", "ACGT" * 10000, "I" * 40000, ["AS:i:200", "XS:i:1", "XN:i:0", "XM:i:0", "XO:i:0", "XG:i:0", "NM:i:0", "YT:Z:UU"])
    big_tag = ("long2", 0, lab, 1, 255, "50M", "A" * 50, "I" * 50, ["AS:i:200", "XS:i:1", "XN:i:0", "XM:i:0", "ZZ:Z:" + "k" * 150_000])
    mixed = recs[:700] + [big_read] + recs[700:1400] + [big_tag] + recs[1400:]
    path = write(tmp_path / "big.bam", refs, mixed)
    _, wantb = host_stats(idx, None, path)
    nb, gotb = device_stats(eng, path)
    assert nb == len(mixed)
    assert_stats_equal(gotb, wantb)
    nb, gotb = device_stats(eng, path, chunk_bytes=1 << 16)
    assert nb == len(mixed)
    assert_stats_equal(gotb, wantb)
    from metamlst_amd.engine import MlstError
    huge = ("long3", 0, lab, 1, 255, "50M", "A" * 50, "I" * 50, ["AS:i:200", "XS:i:1", "XN:i:0", "XM:i:0", "ZZ:Z:" + "k" * 1_100_000])
    path = write(tmp_path / "huge.bam", refs, recs[:100] + [huge] + recs[100:200])
    eng.reset_sample()
    with pytest.raises(MlstError, match=r"\(-5\)"):      # MLST_E_LIMIT
        eng.submit_bam_file(path)
    eng.reset_sample()


@pytest.mark.gpu
def test_list_grows_over_many_pieces_of_the_shortest_accepted_records(tmp_path):
    """records of one base with four one-byte tags (60 bytes each, all accepted, all on known loci), fed in pieces of 64 KiB: the
    sequenceBank list has to have room for the piece in flight and the one being queued, far below mlst_bam_set_capacity's bound"""
    from metamlst_amd.engine import default_params
    idx = load_index(gu.golden_db())
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles)]
    recs = [(chr(65 + k % 26), 0, refs[k % len(refs)][0], 1, 255, "1M", "ACGT"[k % 4], "I", ["AS:i:100", "XS:i:0", "XN:i:0", "XM:i:0"]) for k in range(120_000)]
    path = write(tmp_path / "short.bam", refs, recs)
    targs = TypingArgs(min_read_len=1)
    prm = default_params(); prm.min_read_len = 1
    _, want = host_stats(idx, targs, path)
    assert int(want.counters[1]) == 0 and int(want.n_hits.sum()) == len(recs)
    eng = make_engine(idx, prm)
    n, got = device_stats(eng, path, chunk_bytes=1 << 16)
    assert n == len(recs) and os.path.getsize(path) > 5 * (1 << 16)
    assert_stats_equal(got, want)


@pytest.mark.gpu
def test_order_of_the_records_does_not_matter(zoo_files):
    idx, refs, files = zoo_files
    eng = make_engine(idx)
    chosen = chosen_set(idx)
    base = None
    for name in ("zoo", "shuffled", "sorted"):
        smp, want = host_stats(idx, None, files[name])
        _, got = device_stats(eng, files[name])
        assert_stats_equal(got, want)                       # (locus_first follows the order, as on the host, and so does the
        dev = eng.pileup_bam_file(files[name], chosen)      # length sequenceBank keeps for a read name: the last record's)
        if base is None:
            base = (got, dev)
        assert np.array_equal(got.sum_score, base[0].sum_score) and np.array_equal(got.n_hits, base[0].n_hits)
        assert np.array_equal(got.counters[:2], base[0].counters[:2])
        host = smp.pileup(eng, chosen)
        assert set(dev) == set(host)
        for a in dev:
            assert np.array_equal(dev[a], host[a]) and np.array_equal(dev[a], base[1][a])


@pytest.mark.gpu
def test_record_split_is_exact_where_the_text_spells_record_heads(tmp_path):
    """Qualities that spell plausible record heads (block_size 80, refID 0, a one-byte name, no CIGAR, no SEQ; tiled every 84
    bytes so that the heads chain), placed so that one of them begins exactly at a cell start: the guess of that cell is wrong and
    the chain walk has to correct it."""
    idx = load_index(gu.golden_db())
    refs, recs = zoo(idx, 30_000, seed=6)
    fake = bytes([80, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 1]) + bytes(71)      # 84 bytes: a head + the NUL of its name + filler
    lab = idx.label(0)
    out, at, planted = [], header_size(refs), 0
    cell = 32768
    for r in recs:
        nxt = (at // cell + 1) * cell
        if 2100 <= nxt - at < 2400 and planted < 40:
            L = 4000
            q0 = at + 4 + 32 + 6 + 4 + L // 2                      # where the qualities of the planted record begin (name "fool\0" + 1 digit, one CIGAR op)
            shift = (nxt - q0) % 84
            qual = (fake * 60)[84 - shift:][:L] if shift else (fake * 60)[:L]
            rec = ("fool%d" % (planted % 10), 0, lab, 1, 255, "%dM" % L, "ACGT" * (L // 4), "".join(chr(33 + b) for b in qual),
                   ["AS:i:250", "XS:i:1", "XN:i:0", "XM:i:0", "XO:i:0", "XG:i:0", "NM:i:0", "YT:Z:UU"])
            assert q0 <= nxt < q0 + L - 200 and bytes(ord(c) - 33 for c in rec[7])[nxt - q0:nxt - q0 + 13] == fake[:13]
            out.append(rec); at += record_size(rec); planted += 1
        out.append(r); at += record_size(r)
    assert planted >= 20
    path = write(tmp_path / "fool.bam", refs, out)
    assert samin.read_bam_header(path)[1:] == (0, header_size(refs))      # one call: the cells begin with the file's text
    _, want = host_stats(idx, None, path)
    eng = make_engine(idx)
    n, got = device_stats(eng, path)
    assert n == len(out)
    assert_stats_equal(got, want)
    assert eng.debug_bam_split(0) >= planted // 2          # cells entered from their true start after a wrong guess
    # the hook: every third cell's guess thrown away
    eng.debug_bam_split(3)
    n, got = device_stats(eng, path)
    assert n == len(out)
    assert_stats_equal(got, want)
    assert eng.debug_bam_split(0) > 10
    n, got = device_stats(eng, path)
    assert_stats_equal(got, want)


def _cli(args):
    from metamlst_amd.cli import main
    return main(args)


def _typed(path, dbp, out, extra=()):
    """`cli type --alignments --log` on the file: (the .nfo's bytes or None where no species passes, the log table)"""
    assert _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--log", "--quiet"] + list(extra)) == 0
    name = os.path.basename(path).rsplit(".", 1)[0]
    nfo = open(out + "/%s.nfo" % name, "rb").read().replace(name.encode(), b"X") if os.path.exists(out + "/%s.nfo" % name) else None
    logs = glob.glob(out + "/%s_*.out" % name)
    assert len(logs) == 1
    return nfo, open(logs[0], "rb").read().split(b"\r\n", 1)[1]


@pytest.mark.gpu
def test_fallbacks_to_the_host_path_and_damaged_files(tmp_path, capsys):
    from metamlst_amd.engine import HostPathNeeded, MlstError
    dbp = gu.golden_db()
    idx = load_index(dbp)
    case = CASES[0]
    refs, recs = sam_to_bam(os.path.join(case, "input.sam"), str(tmp_path / "ok.bam"), extra_refs=[("a_b", 100)])
    eng = make_engine(idx)
    r0 = recs[0]
    odd = {"three": r0[:8] + (r0[8][:3],), "yt4": r0[:8] + (r0[8][:3] + ["YT:Z:UU"] + r0[8][3:],), "unmapped": r0[:2] + ("*",) + r0[3:], "name": r0[:2] + ("a_b",) + r0[3:],
           "xmA": r0[:8] + (r0[8][:3] + ["XM:A:1"] + r0[8][4:],)}      # (a digit of type A: the host's int() takes it, the device leaves it to the host)
    raised = 0
    for name, rec in odd.items():
        mixed = recs[:5] + [rec] + recs[5:]
        path = write(tmp_path / (name + ".bam"), refs, mixed)
        eng.reset_sample()
        with pytest.raises(HostPathNeeded, match="at record 5"):
            eng.submit_bam_file(path)
        eng.reset_sample()
        # the command behaves as the host path does: same exception type, or the same .nfo (the host path is what reads SAM text)
        try:
            samin.AlignmentSample(idx, TypingArgs()).add_file(path)
            host_exc = None
        except Exception as e:
            host_exc = type(e)
        out = str(tmp_path / ("out_" + name))
        capsys.readouterr()
        if host_exc is None:
            sam = write_sam(tmp_path / (name + ".sam"), refs, mixed)
            assert _typed(path, dbp, out) == _typed(sam, dbp, out + "_sam")
        else:
            raised += 1
            with pytest.raises(host_exc):
                _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--quiet"])
        assert "host path needed" in capsys.readouterr().err      # the command says which path typed the sample
    assert raised == 4
    # pass 2 alone: an XM tag by name that is no integer, behind four integer fields -- pass 1 takes the record, the pile-up cannot
    from metamlst_amd.typing import pick_alleles_fast
    picked = {idx.label(a) for a in pick_alleles_fast(idx, host_stats(idx, None, str(tmp_path / "ok.bam"))[1], 100).values()}
    r0 = next(r for r in recs if r[2] in picked)                   # a record on a contig the command will choose
    late = r0[:8] + (list(r0[8]) + ["XM:Z:1"],)
    mixed = recs[:5] + [late] + recs[5:]
    path = write(tmp_path / "late.bam", refs, mixed)
    smp, want = host_stats(idx, None, path)
    n, got = device_stats(eng, path)
    assert n == len(mixed)
    assert_stats_equal(got, want)
    a_late = smp.label2a[r0[2]]
    with pytest.raises(HostPathNeeded, match="AS / XM"):
        eng.pileup_bam_file(path, [a_late])
    assert eng.pileup_bam_file(path, []) == {}                     # (a record on a contig that was not chosen is not looked at)
    eng.reset_sample()
    capsys.readouterr()
    out = str(tmp_path / "out_late")
    got_late = _typed(path, dbp, out)
    assert "host path needed: an AS / XM tag" in capsys.readouterr().err
    assert got_late == _typed(write_sam(tmp_path / "late.sam", refs, mixed), dbp, out + "_sam")
    # a flipped byte inside a block that keeps its length: a block of records (the device's check) ...
    good = str(tmp_path / "ok.bam")
    bad = str(tmp_path / "flipped.bam")
    open(bad, "wb").write(flip_in_block(open(good, "rb").read(), 0))
    out = str(tmp_path / "out_bad")
    capsys.readouterr()
    assert _cli(["type", bad, "--alignments", "-d", dbp, "-o", out, "--quiet"]) == 1
    assert "CRC mismatch" in capsys.readouterr().err and not glob.glob(out + "/*.nfo")
    assert _cli(["type", bad, "--alignments", "-d", dbp, "-o", out, "--quiet", "--no-verify-crc"]) == 0
    # ... and a block that holds nothing but reference names of the header (the host's check: these blocks never reach the device)
    many = refs + [("spLong_gene%04d_%d" % (k, k) + "x" * 40, 1000 + k) for k in range(3000)]
    wide = write(tmp_path / "wide.bam", many, recs)
    names, lo, skip = samin.read_bam_header(wide, verify_crc=True)
    assert names == [r[0] for r in many] and lo > 0
    raw = open(wide, "rb").read()
    offs, at = [], 0
    while at < len(raw):
        offs.append(at); at += struct.unpack_from("<H", raw, at + 16)[0] + 1
    k = offs.index(lo) - 1                                          # the block in front of the records' block: names of the header only
    assert k >= 3
    badh = str(tmp_path / "wide_flipped.bam")
    open(badh, "wb").write(flip_in_block(raw, k))
    assert samin.read_bam_header(badh)[0] != names                  # (unchecked, a reference name comes out changed)
    from metamlst_amd.fastq import BgzfCrcError
    with pytest.raises(BgzfCrcError):
        samin.read_bam_header(badh, verify_crc=True)
    out = str(tmp_path / "out_badh")
    capsys.readouterr()
    assert _cli(["type", badh, "--alignments", "-d", dbp, "-o", out, "--quiet"]) == 1
    assert "CRC mismatch" in capsys.readouterr().err and not glob.glob(out + "/*.nfo")
    assert _cli(["type", badh, "--alignments", "-d", dbp, "-o", out, "--quiet", "--no-verify-crc"]) == 0
    capsys.readouterr()
    assert _typed(wide, dbp, out + "_ok") == _typed(good, dbp, out + "_ok")      # (the same records behind a short header)
    assert "host path needed" not in capsys.readouterr().err
    # a truncated file: the last record is cut
    refs2, recs2 = zoo(idx, 5000, seed=2)
    full = np.frombuffer(b"".join([open(write(tmp_path / "t.bam", refs2, recs2), "rb").read()]), np.uint8)
    names, lo, skip = samin.read_bam_header(str(tmp_path / "t.bam"))
    # drop the last data block and the EOF marker: the stream ends inside a record
    offs, at = [], 0
    while at < full.size:
        offs.append(at); at += int(struct.unpack_from("<H", full, at + 16)[0]) + 1
    cut = full[lo:offs[-2]]
    eng.reset_sample()
    eng.bam_open(1, *samin.bam_ref_table(idx, names, None), skip_bytes=skip)
    with pytest.raises(MlstError, match="truncated"):
        eng.submit_bam_bgzf(cut, final=True)
    eng.reset_sample()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[-1]], ids=lambda c: os.path.basename(c))
def test_cli_end_to_end_bam_equals_sam(case, tmp_path, capsys):
    dbp = gu.golden_db()
    argv = json.load(open(os.path.join(case, "args.json")))
    argv = [a for a in argv if a != "--log"]
    sam = str(tmp_path / "smp.sam"); bam = str(tmp_path / "smp.bam")
    open(sam, "wb").write(open(os.path.join(case, "input.sam"), "rb").read())
    sam_to_bam(sam, bam)
    outs = {}
    for kind, path in (("sam", sam), ("bam", bam)):
        out = str(tmp_path / ("out_" + kind))
        assert _cli(["type", path, "--alignments", "-d", dbp, "-o", out, "--log", "--quiet"] + argv) == 0
        nfo = open(out + "/smp.nfo", "rb").read() if os.path.exists(out + "/smp.nfo") else None
        logs = glob.glob(out + "/smp_*.out")
        assert len(logs) == 1
        outs[kind] = (nfo, open(logs[0], "rb").read().split(b"\r\n", 1)[1])
    assert outs["sam"] == outs["bam"]
    assert "host path needed" not in capsys.readouterr().err      # the BAM was typed by the device path


@pytest.mark.gpu
def test_state_hygiene_between_bam_and_fastq_samples(tmp_path):
    import fixtures as fx
    from metamlst_amd import synth
    from metamlst_amd.engine import MlstError
    db, idx = fx.ecoli_small(40)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][2], size=60_000)
    b, q = synth.sample_reads(g, 4000)
    fb, fq, off = synth.flatten_reads(b, q)
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles)]
    recs = []
    for k in range(3000):
        a = (k * 7) % idx.n_alleles
        recs.append(("q%d" % (k // 3), 0, refs[a][0], 1 + k % 50, 255, "100M", idx.sequence(a)[k % 50:k % 50 + 100].decode() if isinstance(idx.sequence(a), bytes) else idx.sequence(a)[k % 50:k % 50 + 100],
                     "I" * 100, ["AS:i:%d" % (150 + k % 50), "XS:i:3", "XN:i:0", "XM:i:%d" % (k % 7), "XO:i:0", "XG:i:0", "NM:i:0", "YT:Z:UU"]))
    bam = write(tmp_path / "s.bam", refs, recs)

    def fastq_stats(e):
        e.reset_sample(); e.submit_reads(fb, fq, off); return e.stats()

    fresh_f = fastq_stats(make_engine(idx))
    fresh_b = device_stats(make_engine(idx), bam)[1]
    _, want_b = host_stats(idx, None, bam)
    assert_stats_equal(fresh_b, want_b)
    eng = make_engine(idx)
    for _ in range(2):
        sb = device_stats(eng, bam)[1]
        sf = fastq_stats(eng)
        for f in STAT_FIELDS:
            assert np.array_equal(getattr(sb, f), getattr(fresh_b, f)) and np.array_equal(getattr(sf, f), getattr(fresh_f, f)), f
        assert np.array_equal(sb.counters, fresh_b.counters) and np.array_equal(sf.counters, fresh_f.counters)
    # a FASTQ entry while a BAM stream is open is refused; the BAM entry needs an open stream
    names, lo, skip = samin.read_bam_header(bam)
    eng.reset_sample()
    eng.bam_open(1, *samin.bam_ref_table(idx, names, None), skip_bytes=skip)
    with pytest.raises(MlstError, match="BAM stream is open"):
        eng.submit_reads(fb, fq, off)
    with pytest.raises(MlstError, match="BAM stream is open"):
        eng.submit_fastq(b"@r\nACGT\n+\nIIII\n")
    eng.reset_sample()
    with pytest.raises(MlstError, match="no BAM stream"):
        eng.submit_bam_bgzf(np.fromfile(bam, np.uint8)[lo:], final=True)
    assert np.array_equal(fastq_stats(eng).sum_score, fresh_f.sum_score)
