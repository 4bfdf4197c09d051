"""What the three BGZF entries say about a buffer that is not a run of whole blocks (csrc/bgzf_host.h lists the blocks, every entry
words its own refusal): the texts engine.py and the callers depend on, and the bytes a non-final call reports as consumed when its
buffer ends inside a block.  Every input is three blocks of a few hundred bytes; N comes from the blocks' own sizes."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import bam_writer
import fixtures as fx
from metamlst_amd import samin
from metamlst_amd.engine import MlstError

pytestmark = pytest.mark.gpu


def bgzf_block(data: bytes, isize=None) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) if isize is None else isize))


def three(raw: bytes) -> list:
    n = (len(raw) + 2) // 3
    return [raw[k:k + n] for k in range(0, len(raw), n)]


def fastq_text(tag: bytes, n=6, seed=5) -> bytes:
    rng = np.random.default_rng(seed)
    return b"".join(b"@%s%d\n" % (tag, k) + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)) + b"\n+\n" + b"I" * 100 + b"\n" for k in range(n))


def variants(raw: bytes) -> dict:
    """the three blocks of raw as they are, with bytes that are no header in place of the second, with a second block whose trailer
    claims 65,537 bytes, and cut in the middle of the third; `at`: where the second block starts, `cut_at`: where the third does"""
    a, b, c = (bgzf_block(p) for p in three(raw))
    assert all(100 < len(x) < 1000 for x in (a, b, c))
    return {"whole": a + b + c, "junk": a + b"x" * 40 + c, "claims": a + bgzf_block(three(raw)[1], 65537) + c, "cut": a + b + c[:len(c) // 2],
            "at": len(a), "cut_at": len(a) + len(b)}


@pytest.fixture(scope="module", params=[None, "0"], ids=["piped", "MLST_BGZF_PIPE=0"])
def eng(request):
    """one engine per setting of MLST_BGZF_PIPE (read once per handle, by the first BGZF call), a tiny synthetic reference"""
    import os
    from metamlst_amd.engine import Engine
    old = os.environ.pop("MLST_BGZF_PIPE", None)
    if request.param is not None:
        os.environ["MLST_BGZF_PIPE"] = request.param
    e = Engine(0)
    e.load_reference(fx.ecoli_small(20)[1])
    e.submit_fastq_bgzf(bgzf_block(b""), final=True)      # (the switch is read here)
    yield e
    os.environ.pop("MLST_BGZF_PIPE", None)
    if old is not None:
        os.environ["MLST_BGZF_PIPE"] = old
    e.close()


def p8(buf):
    a = np.frombuffer(buf, np.uint8)
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def fastq_call(e, buf, final, consumed=False):
    n, used = C.c_uint64(), C.c_uint64()
    e._check(e.lib.mlst_submit_fastq_bgzf(e._h, p8(buf), len(buf), int(final), 0, C.byref(n), C.byref(used) if consumed else None), "mlst_submit_fastq_bgzf")
    return int(n.value), int(used.value)


def pair_call(e, b1, b2, final, consumed=False):
    n, u1, u2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
    e._check(e.lib.mlst_submit_fastq_bgzf_pair(e._h, p8(b1), len(b1), p8(b2), len(b2), int(final), C.byref(n), C.byref(u1) if consumed else None,
                                               C.byref(u2) if consumed else None), "mlst_submit_fastq_bgzf_pair")
    return int(n.value), int(u1.value), int(u2.value)


def refusal(call, *args):
    with pytest.raises(MlstError) as ei:
        call(*args)
    return str(ei.value)


# ------------------------------------------------------------------ mlst_submit_fastq_bgzf
def test_fastq_entry(eng):
    v = variants(fastq_text(b"r"))
    eng.reset_sample()
    assert refusal(fastq_call, eng, v["junk"], True).endswith("not a whole BGZF block at byte %d of the chunk" % v["at"])
    assert refusal(fastq_call, eng, v["claims"], True).endswith("BGZF block at byte %d claims 65537 bytes of data" % v["at"])
    assert refusal(fastq_call, eng, v["cut"], True).endswith("not a whole BGZF block at byte %d of the chunk" % v["cut_at"])      # (a final call)
    assert refusal(fastq_call, eng, v["cut"], False).endswith("not a whole BGZF block at byte %d of the chunk" % v["cut_at"])     # (nobody asked how much was taken)
    # a non-final call whose buffer ends inside the third block: taken up to that block, and the stream goes on from there
    eng.reset_sample()
    n1, used = fastq_call(eng, v["cut"], False, consumed=True)
    assert used == v["cut_at"]
    n2, _ = fastq_call(eng, v["whole"][used:], True)
    assert n1 + n2 == 6


# ------------------------------------------------------------------ mlst_submit_fastq_bgzf_pair
def test_mate_file_entry(eng):
    v1, v2 = variants(fastq_text(b"a", seed=6)), variants(fastq_text(b"b", seed=7))
    eng.reset_sample()
    assert refusal(pair_call, eng, v1["whole"], v2["junk"], True).endswith("not a whole BGZF block at byte %d of file 2 in the chunk" % v2["at"])
    assert refusal(pair_call, eng, v1["whole"], v2["claims"], True).endswith("BGZF block at byte %d of file 2 claims 65537 bytes of data" % v2["at"])
    assert refusal(pair_call, eng, v1["junk"], v2["whole"], True).endswith("not a whole BGZF block at byte %d of file 1 in the chunk" % v1["at"])
    assert refusal(pair_call, eng, v1["claims"], v2["junk"], True).endswith("BGZF block at byte %d of file 1 claims 65537 bytes of data" % v1["at"])
    eng.reset_sample()
    n1, u1, u2 = pair_call(eng, v1["whole"], v2["cut"], False, consumed=True)
    assert (u1, u2) == (len(v1["whole"]), v2["cut_at"])
    n2, _, _ = pair_call(eng, b"", v2["whole"][u2:], True)
    assert n1 + n2 == 12
    eng.reset_sample()
    assert eng.submit_fastq(fastq_text(b"r")) == 6      # (the stream is closed)


# ------------------------------------------------------------------ mlst_submit_bam_bgzf
def bam_records(idx, tmp_path):
    """six records on the first contigs of the reference; -> the inflated records, the reference names of the header"""
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(4)]
    tags = ["AS:i:-5", "XS:i:-20", "XN:i:0", "XM:i:1", "XO:i:0", "XG:i:0", "NM:i:1", "YT:Z:UU"]
    recs = [("read%d" % k, 0, refs[k % 4][0], 1 + k, 255, "100M", "ACGT" * 25, "I" * 100, tags) for k in range(6)]
    path = str(tmp_path / "six.bam")
    bam_writer.write_bam(path, "@HD\tVN:1.0\tSO:unsorted\n", refs, recs)
    names, lo, skip = samin.read_bam_header(path)
    assert lo == 0
    raw = open(path, "rb").read()
    size = struct.unpack_from("<H", raw, 16)[0] + 1
    return zlib.decompress(raw[18:size - 8], -15)[skip:], names


def test_bam_entry(eng, tmp_path):
    text, names = bam_records(eng.index, tmp_path)
    v = variants(text)
    table = samin.bam_ref_table(eng.index, names)

    def closed_and_usable():
        assert refusal(eng.submit_bam_bgzf, v["whole"], True).endswith("no BAM stream is open (mlst_bam_open)")
        eng.reset_sample()
        assert eng.submit_fastq(fastq_text(b"r")) == 6

    eng.reset_sample()
    for what, text_end in (("junk", "not a whole BGZF block at byte %d of the chunk" % v["at"]), ("claims", "BGZF block at byte %d claims 65537 bytes of data" % v["at"]),
                           ("cut", "not a whole BGZF block at byte %d of the chunk" % v["cut_at"])):
        eng.bam_open(1, *table)
        assert refusal(eng.submit_bam_bgzf, v[what], True).endswith(text_end)
        closed_and_usable()
    eng.reset_sample()
    eng.bam_open(1, *table)
    n1, used = eng.submit_bam_bgzf(v["cut"], final=False, partial=True)
    assert used == v["cut_at"]
    n2, _ = eng.submit_bam_bgzf(v["whole"][used:], final=True)
    assert n1 + n2 == 6
    closed_and_usable()
