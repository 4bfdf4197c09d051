"""BGZF block CRC-32s verified on the GPU (k_bgzf_crc behind the decoders; mlst_set_bgzf_verify, `cli type` by default).
The reference for a CRC is zlib.crc32; every comparison is exact."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import fixtures as fx
from metamlst_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 65279, 65280, 65535, 65536)


def deflate(data: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def bgzf_raw(raw: bytes, data: bytes, crc=None) -> bytes:
    """a BGZF block around a deflate stream; crc: what the trailer says (default: the CRC-32 of data)"""
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(raw) + 25) + raw
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc, len(data)))


def bgzf_block(data: bytes, level: int = 6) -> bytes:
    return bgzf_raw(deflate(data, level), data)


def fastq_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(60, 151))
        out.append(b"@read%d/%d\n%s\n+\n%s\n" % (seed, k, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), bytes(rng.integers(35, 74, L, dtype=np.uint8))))
    return b"".join(out)


def set_decoder(monkeypatch, mode: str) -> None:
    monkeypatch.setenv("MLST_INFLATE_MODE", mode[0])      # (read when an engine inflates for the first time)
    monkeypatch.setenv("MLST_INFLATE_TOK", "2" if mode == "2c" else "1")


@pytest.mark.parametrize("mode", ["2", "2c", "1"])
def test_crc_values_equal_zlib(mode, monkeypatch):
    """Engine.bgzf_block_crcs against zlib.crc32: every size x content x level, with empty blocks between, in one call of several
    thousand blocks and in calls of one block, behind each of the three decoders."""
    from metamlst_amd.engine import Engine
    set_decoder(monkeypatch, mode)
    rng = np.random.default_rng(17)
    fq = fastq_text(600, 3)
    assert len(fq) >= 65536
    blocks, want, singles = [], [], []
    for n in SIZES:
        for kind, data in (("zero", bytes(n)), ("ff", b"\xff" * n), ("random", bytes(rng.integers(0, 256, n, dtype=np.uint8))), ("fastq", fq[7:7 + n])):
            for level in (0, 1, 6, 9):
                raw = deflate(data, level)
                if len(raw) + 26 > 65536:         # (a BGZF block holds at most 64 KiB: 65,535 incompressible or stored bytes do not fit the format)
                    continue
                b = bgzf_raw(raw, data, crc=0x12345678)      # whatever the trailer says
                blocks.append(b)
                want.append(zlib.crc32(data) & 0xFFFFFFFF)
                if level == 6:
                    singles.append((b, want[-1]))
                if len(blocks) % 3 == 0:
                    blocks.append(bgzf_block(b""))
    # up to several thousand blocks: FASTQ text in blocks of odd sizes (the text offsets of the blocks take every alignment)
    at, k = 0, 0
    while len(want) < 4200:
        n = 1 + (k * 7919) % 3001
        data = fq[at % 50000:at % 50000 + n]
        blocks.append(bgzf_block(data, (1, 6)[k & 1]))
        want.append(zlib.crc32(data) & 0xFFFFFFFF)
        at += n
        k += 1
    eng = Engine(0)
    got = eng.bgzf_block_crcs(b"".join(blocks))
    assert got.dtype == np.uint32 and len(got) == len(want)
    bad = np.nonzero(got != np.array(want, np.uint32))[0]
    assert len(bad) == 0, "first differing blocks: %s" % [(int(i), hex(int(got[i])), hex(want[i])) for i in bad[:5]]
    for b, w in singles:
        assert eng.bgzf_block_crcs(b).tolist() == [w]
    assert eng.last_crc_ms > 0.0
    assert eng.bgzf_block_crcs(bgzf_block(b"")).tolist() == []
    eng.close()


def test_single_bit_flips_are_caught_with_verification_on_and_pass_with_it_off():
    """2,000 seeded single-bit flips over the deflate data and the four CRC bytes of a level-6 and of a level-1 block of FASTQ, each fed
    inside a run of 64 good blocks through mlst_selftest_inflate_device.  On: an error that names the damaged block, or the original
    text (a flip of padding bits), and at least 90 % errors -- zlib's own checks (deflate error, wrong length) catch about 30 %.
    Off: today's behaviour -- at least one flip is accepted with different text."""
    from metamlst_amd.engine import Engine, MlstError
    fq = fastq_text(700, 5)
    good = [bgzf_block(fq[1000 * k:1000 * k + 3000], (1, 6)[k & 1]) for k in range(64)]
    good_text = [fq[1000 * k:1000 * k + 3000] for k in range(64)]
    eng = Engine(0)
    for level in (6, 1):
        data = fq[20000:40000]
        raw = deflate(data, level)
        rng = np.random.default_rng(100 + level)
        flips = rng.integers(0, 8 * (len(raw) + 4), 2000)
        for on in (True, False):
            eng.set_bgzf_verify(on)
            assert eng.bgzf_verify is on
            errors, same, accepted_wrong = 0, 0, 0
            for j, bit in enumerate(flips.tolist()):
                blk = bytearray(bgzf_raw(raw, data))
                blk[18 + bit // 8] ^= 1 << (bit % 8)          # deflate data from byte 18 on, the CRC behind it
                pos = j % 65
                want = b"".join(good_text[:pos]) + data + b"".join(good_text[pos:])
                try:
                    out = eng.inflate_bgzf(b"".join(good[:pos]) + bytes(blk) + b"".join(good[pos:]))
                except MlstError as e:
                    m = re.search(r"BGZF block (\d+)", str(e))
                    assert m and int(m.group(1)) == pos, (level, on, bit, str(e))
                    errors += 1
                    continue
                if out == want:
                    same += 1
                else:
                    accepted_wrong += 1
            print("level %d, verification %s: %d errors, %d accepted with the original text, %d accepted with different text"
                  % (level, "on" if on else "off", errors, same, accepted_wrong))
            if on:
                assert accepted_wrong == 0
                assert errors >= 0.9 * len(flips)
            else:
                assert accepted_wrong >= 1
    eng.close()


@pytest.fixture(scope="module")
def sample():
    """(index, FASTQ text of 6,000 reads of a genome of the small database)"""
    db, idx = fx.ecoli_small(80)
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][2], size=100_000)
    b, q = synth.sample_reads(g, 6000)
    text = b"".join(b"@r%d\n" % k + b[k].tobytes() + b"\n+\n" + q[k].tobytes() + b"\n" for k in range(len(b)))
    return db, idx, text


def _engine(idx, verify=True):
    from metamlst_amd.engine import Engine
    eng = Engine(0)
    eng.load_reference(idx)
    eng.set_bgzf_verify(verify)
    return eng


def records(text: bytes) -> list:
    lines = text.split(b"\n")
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def damage_payload(block: bytes) -> bytes:
    """one payload byte of a stored block changed (the raw inflate succeeds, the text differs)"""
    b = bytearray(block)
    assert b[18] == 0x01                          # BFINAL, stored
    b[18 + 5 + 20] ^= 0x20
    return bytes(b)


def damage_crc(block: bytes) -> bytes:
    b = bytearray(block)
    b[-8] ^= 0x01
    return bytes(b)


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_mismatch_names_the_block_in_every_piece_of_a_split_chunk(sample, pipe, monkeypatch):
    """A chunk of 40,000 blocks is split by the library into pieces of 16,384, 15,424 and 8,192 blocks (MLST_BGZF_PIPE=0: one launch):
    a stored block with a changed byte and a good block with a changed CRC field are reported with their number in the chunk,
    wherever they lie; a sound chunk passes."""
    from metamlst_amd.engine import MlstError
    monkeypatch.setenv("MLST_BGZF_PIPE", pipe)
    _, idx, text = sample
    recs = records(text)
    blocks = [bgzf_block(recs[k % len(recs)], 0 if k % 5 == 0 else 1) for k in range(40_000)]
    eng = _engine(idx)
    assert eng.submit_fastq_bgzf(b"".join(blocks) + bgzf_block(b""), final=True) == 40_000
    for k in (100, 20_000, 39_000):               # multiples of five: stored blocks
        for how in (damage_payload, damage_crc):
            eng.reset_sample()
            bad = how(blocks[k])
            with pytest.raises(MlstError, match=r"CRC mismatch in BGZF block %d of the chunk \(stored 0x[0-9a-f]{8}, computed 0x[0-9a-f]{8}\)" % k):
                eng.submit_fastq_bgzf(b"".join(blocks[:k]) + bad + b"".join(blocks[k + 1:]), final=True)
    # a deflate error is numbered the same way (in the chunk, not in the piece the library cut)
    for k in (101, 20_001, 39_001):
        eng.reset_sample()
        b = bytearray(blocks[k])
        b[18] = 0x07                              # BFINAL = 1, BTYPE = 3 (reserved): not deflate data
        with pytest.raises(MlstError, match=r"corrupt deflate data in BGZF block %d of the chunk \(code" % k):
            eng.submit_fastq_bgzf(b"".join(blocks[:k]) + bytes(b) + b"".join(blocks[k + 1:]), final=True)
    # the values in the message
    eng.reset_sample()
    with pytest.raises(MlstError, match="computed 0x%08x" % (zlib.crc32(recs[100 % len(recs)]) & 0xFFFFFFFF)):
        eng.submit_fastq_bgzf(b"".join(blocks[:100]) + damage_crc(blocks[100]) + b"".join(blocks[101:200]), final=True)
    eng.close()


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_mismatch_on_the_paired_entry_names_the_file(sample, pipe, monkeypatch):
    from metamlst_amd.engine import MlstError
    monkeypatch.setenv("MLST_BGZF_PIPE", pipe)
    _, idx, text = sample
    recs = records(text)
    f1 = [bgzf_block(b"".join(recs[k:k + 40]), 0) for k in range(0, 3000, 40)]
    f2 = [bgzf_block(b"".join(recs[k:k + 25]), 0) for k in range(3000, 6000, 25)]
    eof = bgzf_block(b"")
    eng = _engine(idx)
    assert eng.submit_fastq_bgzf_pair(b"".join(f1) + eof, b"".join(f2) + eof, final=True) == 6000
    for file, blocks, k in ((1, f1, 0), (1, f1, 74), (2, f2, 0), (2, f2, 61), (2, f2, 119)):
        for how in (damage_payload, damage_crc):
            eng.reset_sample()
            bad = b"".join(blocks[:k]) + how(blocks[k]) + b"".join(blocks[k + 1:]) + eof
            with pytest.raises(MlstError, match=r"CRC mismatch in BGZF block %d of file %d in the chunk \(stored" % (k, file)):
                eng.submit_fastq_bgzf_pair(bad if file == 1 else b"".join(f1) + eof, bad if file == 2 else b"".join(f2) + eof, final=True)
    eng.close()


@pytest.mark.parametrize("mode", ["2", "2c", "1"])
def test_a_deflate_error_is_reported_before_a_crc_mismatch(sample, mode, monkeypatch):
    from metamlst_amd.engine import MlstError
    set_decoder(monkeypatch, mode)
    _, idx, text = sample
    recs = records(text)
    blocks = [bgzf_block(b"".join(recs[k:k + 30]), 6) for k in range(0, 3000, 30)]
    b = bytearray(damage_crc(blocks[37]))
    b[18] = 0x07                                  # BFINAL = 1, BTYPE = 3 (reserved): not deflate data -- and the CRC field is wrong too
    eng = _engine(idx)
    with pytest.raises(MlstError, match="corrupt deflate data in BGZF block 37 of the chunk"):
        eng.submit_fastq_bgzf(b"".join(blocks[:37]) + bytes(b) + b"".join(blocks[38:]) + bgzf_block(b""), final=True)
    # ... also when another block has only a wrong CRC
    eng.reset_sample()
    with pytest.raises(MlstError, match="corrupt deflate data in BGZF block 37 of the chunk"):
        eng.submit_fastq_bgzf(b"".join(blocks[:5]) + damage_crc(blocks[5]) + b"".join(blocks[6:37]) + bytes(b) + b"".join(blocks[38:]) + bgzf_block(b""), final=True)
    eng.close()


def test_state_after_a_mismatch(sample):
    """As test_pair_bgzf_errors_leave_no_carry: after the failure and reset_sample a plain submit_fastq gives what a fresh engine
    gives; the switch refuses to change while a stream is open."""
    from metamlst_amd.engine import MlstError
    _, idx, text = sample
    recs = records(text)
    single = b"".join(recs[:500])
    eng = _engine(idx)
    eng.submit_fastq(single)
    want = eng.stats()
    blocks = [bgzf_block(text[at:at + 9000], 0) for at in range(0, len(text), 9000)]      # records straddle the blocks: carries
    eof = bgzf_block(b"")
    half = len(blocks) // 2
    for k in (3, half + 2):
        bad = blocks[:k] + [damage_payload(blocks[k])] + blocks[k + 1:]
        eng.reset_sample()
        with pytest.raises(MlstError, match="CRC mismatch in BGZF block"):
            eng.submit_fastq_bgzf(b"".join(bad[:half]), final=False)
            eng.submit_fastq_bgzf(b"".join(bad[half:]) + eof, final=True)
        eng.reset_sample()
        assert eng.submit_fastq(single) == 500
        fx.assert_stats_equal(eng.stats(), want)
    f2 = [bgzf_block(b"".join(recs[k:k + 25]), 0) for k in range(0, 3000, 25)]
    eng.reset_sample()
    with pytest.raises(MlstError, match="CRC mismatch in BGZF block 7 of file 2"):
        eng.submit_fastq_bgzf_pair(b"".join(f2) + eof, b"".join(f2[:7]) + damage_crc(f2[7]) + b"".join(f2[8:]) + eof, final=True)
    eng.reset_sample()
    assert eng.submit_fastq(single) == 500
    fx.assert_stats_equal(eng.stats(), want)
    # the switch while a stream is open
    eng.reset_sample()
    eng.submit_fastq_bgzf(b"".join(blocks[:half]), final=False)
    with pytest.raises(MlstError, match="stream is open"):
        eng.set_bgzf_verify(False)
    assert eng.bgzf_verify is True
    eng.submit_fastq_bgzf(b"".join(blocks[half:]) + eof, final=True)
    eng.set_bgzf_verify(False)
    assert eng.bgzf_verify is False
    eng.reset_sample()
    eng.submit_fastq_bgzf_pair(b"".join(f2[:60]), b"".join(f2[:50]), final=False)
    with pytest.raises(MlstError, match="stream is open"):
        eng.set_bgzf_verify(True)
    eng.reset_sample()
    eng.set_bgzf_verify(True)
    eng.close()


def test_good_files_give_the_same_statistics_on_and_off(sample):
    _, idx, text = sample
    recs = records(text)
    t1, t2 = b"".join(recs[:3000]), b"".join(recs[3000:])
    z = lambda t, n: b"".join(bgzf_block(t[at:at + n], 6) for at in range(0, len(t), n)) + bgzf_block(b"")      # noqa: E731
    eng = _engine(idx, verify=False)
    eng.submit_fastq(text)
    want = eng.stats()
    eng.reset_sample()
    eng.submit_fastq_pair(t1, t2)
    want_pair = eng.stats()
    for on in (False, True):
        eng.reset_sample()
        eng.set_bgzf_verify(on)
        assert eng.submit_fastq_bgzf(z(text, 50_000), final=True) == 6000
        fx.assert_stats_equal(eng.stats(), want)
        eng.reset_sample()
        assert eng.submit_fastq_bgzf_pair(z(t1, 30_000), z(t2, 41_000), final=True) == 6000
        fx.assert_stats_equal(eng.stats(), want_pair)
    eng.close()


def run_cli(args, env=None):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.update(env or {})
    return subprocess.run([sys.executable, "-m", "metamlst_amd.cli"] + args, env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)


def test_the_command_checks_by_default(sample, tmp_path):
    """cli type: a damaged bgzip'd file ends the command with the mismatch and the file's name and no .nfo; --no-verify-crc types it;
    a sound file gives the same .nfo bytes either way; a folder with one damaged sample types the others and fails at the end;
    --gpus 2 (two ranks on one GPU) reports damage in a boundary block (host) and in an interior block (device)."""
    db, idx, text = sample
    blocks = [bgzf_block(text[at:at + 30_000], 0) for at in range(0, len(text), 30_000)]
    eof = bgzf_block(b"")
    good = tmp_path / "good.fastq.gz"
    good.write_bytes(b"".join(blocks) + eof)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).tolist()

    def damaged(name, k):
        p = tmp_path / name
        p.write_bytes(b"".join(blocks[:k]) + damage_payload(blocks[k]) + b"".join(blocks[k + 1:]) + eof)
        return p

    bad = damaged("bad.fastq.gz", 5)
    common = ["-d", db.path, "--quiet"]
    r = run_cli(["type", str(bad), "-o", str(tmp_path / "o1")] + common)
    assert r.returncode != 0 and "CRC mismatch in BGZF block 5" in r.stderr and str(bad) in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "Traceback" not in r.stderr
    assert not os.path.exists(tmp_path / "o1" / "bad.nfo")
    r = run_cli(["type", str(bad), "-o", str(tmp_path / "o2"), "--no-verify-crc"] + common)
    assert r.returncode == 0, r.stderr
    nfo = {}
    for flag in ([], ["--no-verify-crc"]):
        out = tmp_path / ("o3" + "".join(flag))
        r = run_cli(["type", str(good), "-o", str(out)] + flag + common)
        assert r.returncode == 0, r.stderr
        nfo[len(flag)] = open(out / "good.nfo", "rb").read()
    assert nfo[0] == nfo[1] and len(nfo[0]) > 0
    # a folder of three samples, the second damaged
    folder = tmp_path / "samples"
    folder.mkdir()
    for name, src in (("a.fastq.gz", good), ("b.fastq.gz", bad), ("c.fastq.gz", good)):
        (folder / name).write_bytes(src.read_bytes())
    r = run_cli(["type", str(folder), "-o", str(tmp_path / "o4")] + common)
    assert r.returncode != 0 and "CRC mismatch" in r.stderr and "b.fastq.gz" in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "Traceback" not in r.stderr
    assert len(open(tmp_path / "o4" / "a.nfo", "rb").read()) > 0 and len(open(tmp_path / "o4" / "c.nfo", "rb").read()) > 0
    assert not os.path.exists(tmp_path / "o4" / "b.nfo")
    # two ranks: the boundary block is the host's, an interior block of rank 1's range the device's
    one_gpu = {"MLST_ONE_GPU": "1", "MLST_BACKEND": "gloo"}
    size = offs[-1] + len(eof)
    kb = next(i for i, o in enumerate(offs) if o >= size // 2)
    for name, k, side in (("boundary.fastq.gz", kb, "BGZF block at byte %d" % offs[kb]), ("interior.fastq.gz", len(blocks) - 2, "CRC mismatch in BGZF block")):
        p = damaged(name, k)
        r = run_cli(["type", str(p), "-o", str(tmp_path / ("o5" + name)), "--gpus", "2"] + common, one_gpu)
        assert r.returncode != 0 and "CRC mismatch" in r.stderr and side in r.stderr and str(p) in r.stderr, (name, r.returncode, r.stdout, r.stderr)
        # the rank's own report (its handler ran), not an uncaught exception on the way out
        assert re.search(r"^rank [01]: %s: " % re.escape(str(p)), r.stderr, re.M) and "Traceback" not in r.stderr, r.stderr
        assert not os.path.exists(tmp_path / ("o5" + name) / (name.split(".")[0] + ".nfo"))
    r = run_cli(["type", str(good), "-o", str(tmp_path / "o6"), "--gpus", "2"] + common, one_gpu)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "o6" / "good.nfo", "rb").read() == nfo[0]
