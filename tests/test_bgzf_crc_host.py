"""BGZF block CRCs, the host's share: the boundary blocks of a byte range of a bgzip'd FASTQ are inflated on the host with a raw
inflate that checks nothing (fastq.bgzf_range_plan); with verify_crc their text must have the CRC-32 of the block's trailer
(zlib.crc32 is the reference).  And the command lists its switch."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from metamlst_amd.fastq import bgzf_range_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bgzf_block(data: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def fastq_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(60, 151))
        out.append(b"@r%d\n%s\n+\n%s\n" % (k, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), bytes(rng.integers(35, 74, L, dtype=np.uint8))))
    return b"".join(out)


def test_range_plan_checks_the_crc_of_the_blocks_the_host_inflates(tmp_path):
    text = fastq_text(3000, 11)
    blocks = [bgzf_block(text[at:at + 9000], 0) for at in range(0, len(text), 9000)] + [bgzf_block(b"", 0)]      # stored blocks
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).tolist()
    good = tmp_path / "good.fastq.gz"
    good.write_bytes(b"".join(blocks))
    size, world = offs[-1], 3
    ranges = [(size * r // world, size * (r + 1) // world if r + 1 < world else size) for r in range(world)]
    plans = [bgzf_range_plan(str(good), lo, hi) for lo, hi in ranges]
    assert [bgzf_range_plan(str(good), lo, hi, verify_crc=True) for lo, hi in ranges] == plans      # a sound file: the same plan
    # the boundary block of ranks 0 / 1: the first block that starts at or behind the boundary
    k = next(i for i, o in enumerate(offs) if o >= ranges[1][0])
    bad = bytearray(b"".join(blocks))
    at = offs[k] + 18 + 5 + 100                     # header, the stored block's five bytes, then payload
    bad[at] ^= 0x04
    damaged = tmp_path / "damaged.fastq.gz"
    damaged.write_bytes(bytes(bad))
    for r in (0, 1):                                # both ranks inflate this block (the tail of one, the head of the other)
        with pytest.raises(ValueError, match=r"CRC mismatch in the BGZF block at byte %d \(stored 0x[0-9a-f]{8}, computed 0x[0-9a-f]{8}\)" % offs[k]):
            bgzf_range_plan(str(damaged), *ranges[r], verify_crc=True)
    want_crc = zlib.crc32(text[9000 * k:9000 * (k + 1)]) & 0xFFFFFFFF
    with pytest.raises(ValueError, match="stored 0x%08x" % want_crc):
        bgzf_range_plan(str(damaged), *ranges[1], verify_crc=True)
    # without the check: the plan of today, with the changed byte in it
    p0, p1 = bgzf_range_plan(str(damaged), *ranges[0], verify_crc=False), bgzf_range_plan(str(damaged), *ranges[1])
    assert p0["mid"] == plans[0]["mid"] and p1["mid"] == plans[1]["mid"]
    assert len(p0["tail"]) == len(plans[0]["tail"]) and len(p1["head"]) == len(plans[1]["head"])
    assert p0["tail"] + p1["head"] != plans[0]["tail"] + plans[1]["head"]
    assert bgzf_range_plan(str(damaged), *ranges[2], verify_crc=True) == plans[2]                    # rank 2 never reads that block


def test_cli_type_lists_the_switch():
    r = subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "type", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--no-verify-crc" in r.stdout
