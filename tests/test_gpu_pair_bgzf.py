"""bgzip'd mate files inflated and paired on the GPU (mlst_submit_fastq_bgzf_pair): the statistics are those of the same mates
as text through mlst_submit_fastq_pair, however the two files are blocked, compressed and cut into calls; `cli type R1 -2 R2`
takes that path when both files are BGZF; errors leave no carry behind."""
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

import fixtures as fx
from metamlst_amd import synth
from metamlst_amd.engine import pair_file_cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bgzf_block(data: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_blocks(raw: bytes, sizes=(65280,), level: int = 6, empty_every: int = 0) -> list:
    """raw in blocks of sizes[0], sizes[1], ... (cycled), an empty block after every empty_every-th, the EOF block last"""
    out, at, k = [], 0, 0
    while at < len(raw):
        n = sizes[k % len(sizes)]
        out.append(bgzf_block(raw[at:at + n], level))
        at += n
        k += 1
        if empty_every and k % empty_every == 0:
            out.append(bgzf_block(b"", level))
    out.append(bgzf_block(b"", level))
    return out


def mates(n_pairs=6000, short2=0, seed=0):
    """(index, text of R1, text of R2, names shared): R2's reads cut to 150 - short2 bases"""
    db, idx = fx.ecoli_small(80)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][2], size=100_000)
    b, q = synth.sample_pairs(g, n_pairs=n_pairs, seed=synth.SEED + seed)
    texts = []
    for rows, suf, cut in ((slice(0, None, 2), b" 1:N:0", 0), (slice(1, None, 2), b" 2:N:0", short2)):
        bb, qq = b[rows], q[rows]
        L = bb.shape[1] - cut
        texts.append(b"".join(b"@p%d%s\n" % (k, suf) + bb[k, :L].tobytes() + b"\n+\n" + qq[k, :L].tobytes() + b"\n" for k in range(len(bb))))
    return db, idx, texts[0], texts[1]


def records(text: bytes) -> list:
    lines = text.split(b"\n")
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def test_pair_file_cuts_keep_the_files_in_step():
    """The feeder's byte ranges: contiguous, covering both files, about the same fraction of each, a quarter-size first call."""
    for s1, s2, chunk in ((100, 50, 40), (10_000_000, 3_000_000, 1_000_000), (5 << 30, 1 << 20, 512 << 20), (7, 0, 3), (0, 9, 4)):
        cuts = pair_file_cuts(s1, s2, chunk)
        assert cuts[0][0] == 0 and cuts[0][2] == 0 and cuts[-1][1] == s1 and cuts[-1][3] == s2
        for a, b in zip(cuts, cuts[1:]):
            assert a[1] == b[0] and a[3] == b[2]
        for lo1, hi1, lo2, hi2 in cuts:
            assert hi1 >= lo1 and hi2 >= lo2
            assert (hi1 - lo1) + (hi2 - lo2) <= chunk + 2
            if s1 and s2:
                assert abs(hi1 / s1 - hi2 / s2) <= 1.0 / min(s1, s2) + 1e-9      # the same fraction of each file
        if s1 + s2 > chunk:
            assert (cuts[0][1] + cuts[0][3]) <= chunk // 4 + 2 < (cuts[1][1] - cuts[1][0]) + (cuts[1][3] - cuts[1][2])
    assert pair_file_cuts(0, 0, 10) == [(0, 0, 0, 0)]


@pytest.fixture(scope="module")
def data():
    return mates(short2=30)


def _engine(idx):
    from metamlst_amd.engine import Engine
    eng = Engine(0)
    eng.load_reference(idx)
    return eng


def _feed(eng, calls):
    n = 0
    for k, (c1, c2) in enumerate(calls):
        n += eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1))
    return n


def _calls(blocks1, blocks2, sizes1, sizes2):
    """blocks of both files grouped into calls of the given compressed sizes (cycled), in step by call number"""
    def groups(blocks, sizes):
        out, cur, k = [], b"", 0
        for bl in blocks:
            cur += bl
            if len(cur) >= sizes[k % len(sizes)]:
                out.append(cur); cur = b""; k += 1
        out.append(cur)
        return out
    g1, g2 = groups(blocks1, sizes1), groups(blocks2, sizes2)
    n = max(len(g1), len(g2))
    return list(zip(g1 + [b""] * (n - len(g1)), g2 + [b""] * (n - len(g2))))


@pytest.mark.gpu
def test_pair_bgzf_matches_the_text_path(data, monkeypatch):
    _, idx, t1, t2 = data
    n_rec = len(records(t1))
    eng = _engine(idx)
    assert eng.submit_fastq_pair(t1, t2) == 2 * n_rec
    want = eng.stats()
    equal1, equal2 = bgzf_blocks(t1), bgzf_blocks(t2)
    odd1 = bgzf_blocks(t1, (65280,), level=1)
    odd2 = bgzf_blocks(t2, (17, 1000, 65280, 4321, 17, 9000), level=9, empty_every=2)
    cases = {
        "equal blocks, one call": [(b"".join(equal1), b"".join(equal2))],
        "equal blocks, a block per call": _calls(equal1, equal2, (1,), (1,)),
        "level 1 / level 9 irregular, one call": [(b"".join(odd1), b"".join(odd2))],
        "level 1 / level 9 irregular, 70-90 kB calls": _calls(odd1, odd2, (70_000, 90_000, 80_000), (90_000, 70_000)),
        "R2 first, then R1": [(b"", b"".join(odd2)), (b"".join(odd1), b"")],
    }
    for name, calls in cases.items():
        eng.reset_sample()
        assert _feed(eng, calls) == 2 * n_rec, name
        fx.assert_stats_equal(eng.stats(), want)
    # the file feeder: raw reads cut anywhere (the library takes each buffer's whole blocks), small calls and one call
    d = tempfile.mkdtemp(prefix="mlst_pbz_")
    p1, p2 = os.path.join(d, "s_R1.fastq.gz"), os.path.join(d, "s_R2.fastq.gz")
    open(p1, "wb").write(b"".join(odd1))
    open(p2, "wb").write(b"".join(odd2))
    for chunk in (80_000, 1 << 30):
        eng.reset_sample()
        assert eng.submit_fastq_bgzf_pair_files(p1, p2, chunk_bytes=chunk) == 2 * n_rec
        fx.assert_stats_equal(eng.stats(), want)
    eng.close()
    # the serial form on a fresh engine
    monkeypatch.setenv("MLST_BGZF_PIPE", "0")
    eng = _engine(idx)
    for calls in (cases["level 1 / level 9 irregular, 70-90 kB calls"], cases["equal blocks, one call"]):
        eng.reset_sample()
        assert _feed(eng, calls) == 2 * n_rec
        fx.assert_stats_equal(eng.stats(), want)
    eng.close()


@pytest.mark.gpu
def test_sample_files_route_bgzf_mates_to_the_gpu(data, monkeypatch):
    """cli.submit_sample_files on two BGZF mate files never goes through the host pairing (fastq.pair_chunks)."""
    from metamlst_amd import cli, fastq
    _, idx, t1, t2 = data
    eng = _engine(idx)
    eng.submit_fastq_pair(t1, t2)
    want = eng.stats()
    d = tempfile.mkdtemp(prefix="mlst_pbz_")
    p1, p2 = os.path.join(d, "s_R1.fastq.gz"), os.path.join(d, "s_R2.fastq.gz")
    open(p1, "wb").write(b"".join(bgzf_blocks(t1)))
    open(p2, "wb").write(b"".join(bgzf_blocks(t2, (30_000, 65280), level=9)))

    def host_pairing(*a, **k):
        raise AssertionError("bgzip'd mates went through the host pairing")
    monkeypatch.setattr(fastq, "pair_chunks", host_pairing)
    monkeypatch.setattr(cli, "pair_chunks", host_pairing, raising=False)
    eng.reset_sample()
    cli.submit_sample_files(eng, [p1, p2], True, 1 << 20)
    fx.assert_stats_equal(eng.stats(), want)
    eng.close()


@pytest.mark.gpu
def test_pair_bgzf_errors_leave_no_carry(data):
    from metamlst_amd.engine import MlstError
    _, idx, t1, t2 = data
    r1, r2 = records(t1), records(t2)
    eng = _engine(idx)
    single = b"".join(r1[:500])
    eng.submit_fastq(single)
    want_single = eng.stats()
    z = lambda text, **k: b"".join(bgzf_blocks(text, **k))      # noqa: E731
    bad2 = bgzf_blocks(t2, (20_000,))
    corrupt = bytearray(bad2[3])
    corrupt[18] = 0x07                                        # BFINAL = 1, BTYPE = 3 (reserved): not deflate data
    cases = [
        ("R2 one record short", [(z(t1), z(b"".join(r2[:-1])))], "different numbers of records"),
        ("R2 one record long", [(z(t1), z(t2 + r2[0]))], "different numbers of records"),
        ("a corrupt block in R2", [(z(t1), b"".join(bad2[:3]) + bytes(corrupt) + b"".join(bad2[4:]))], "corrupt deflate data.*file 2"),
        ("R1 ends inside a quality line", [(z(t1[:-40]), z(t2))], "malformed FASTQ"),
        ("R1 ends behind a sequence line", [(z(t1[:t1.rindex(b"\n+\n") + 1]), z(t2))], "mate file 1 does not end with a whole record"),
        ("R2 short, cut into calls", _calls(bgzf_blocks(t1, (9000,)), bgzf_blocks(b"".join(r2[:-3]), (7000,)), (1,), (1,)), "different numbers of records"),
    ]
    for name, calls, match in cases:
        eng.reset_sample()
        with pytest.raises(MlstError, match=match):
            _feed(eng, calls)
        eng.reset_sample()
        assert eng.submit_fastq(single) == 500, name
        fx.assert_stats_equal(eng.stats(), want_single)
    # an error in the middle of a stream drops it as well: the next call starts a new one
    eng.reset_sample()
    calls = _calls(bgzf_blocks(t1, (9000,)), bgzf_blocks(t2, (7000,)), (1,), (1,))
    eng.submit_fastq_bgzf_pair(calls[0][0], calls[0][1], final=False)
    with pytest.raises(MlstError, match="paired BGZF stream is open"):
        eng.submit_fastq(single)
    eng.reset_sample()
    assert eng.submit_fastq(single) == 500
    fx.assert_stats_equal(eng.stats(), want_single)
    # two empty files: no reads
    eng.reset_sample()
    assert eng.submit_fastq_bgzf_pair(z(b""), z(b""), final=True) == 0
    assert eng.submit_fastq_bgzf_pair(b"", b"", final=True) == 0
    assert int(eng.stats().counters[0]) == 0
    eng.close()


def _run_cli(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "metamlst_amd.cli"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.gpu
def test_cli_bgzf_mates_count_a_pair_once_per_locus():
    """`cli type R1.fastq.gz -2 R2.fastq.gz` on bgzip'd mates sharing names: the .nfo of the same mates as text, and the
    coverage column of the API's paired=True result."""
    from metamlst_amd import db as mdb
    from metamlst_amd.typing import TypingArgs, type_sample
    db, idx, t1, t2 = mates(n_pairs=int(100_000 * 20 / 300), seed=5)
    eng = _engine(idx)
    eng.submit_fastq_pair(t1, t2)
    res = type_sample(idx, eng.stats(), eng.pileup, mdb.metaMLST_db(db.path), "x", TypingArgs(), out_dir=None)
    want = sorted((gene, str(v[3])) for r in res for gene, v in r.closest.items())
    eng.close()
    assert len(want) == 7

    def coverage_column(stdout):
        rows = [ln.split() for ln in stdout.splitlines() if ln.startswith("  ") and not ln.startswith("  ->") and len(ln.split()) == 5]
        return sorted((r[0], r[1]) for r in rows)

    d = tempfile.mkdtemp(prefix="mlst_pbz_cli_")
    nfo = {}
    for kind in ("text", "bgzf"):
        sub = os.path.join(d, kind)
        os.mkdir(sub)
        paths = []
        for name, text in (("s_R1.fastq", t1), ("s_R2.fastq", t2)):
            p = os.path.join(sub, name + (".gz" if kind == "bgzf" else ""))
            open(p, "wb").write(b"".join(bgzf_blocks(text, (65280,) if name == "s_R1.fastq" else (20_000, 65280), level=6)) if kind == "bgzf" else text)
            paths.append(p)
        out = os.path.join(sub, "out")
        stdout = _run_cli(["type", paths[0], "-2", paths[1], "-d", db.path, "-o", out])
        assert coverage_column(stdout) == want, (kind, stdout[-1500:])
        nfo[kind] = open(os.path.join(out, "s_R1.nfo"), "rb").read()
    assert nfo["text"] and nfo["text"] == nfo["bgzf"]
