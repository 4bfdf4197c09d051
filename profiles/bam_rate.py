#!/usr/bin/env python3
"""Rate of BAM input: a synthetic bowtie2-shaped BGZF BAM (records of 150 bases, ~20 records per read name, tags AS XS XN XM XO XG
NM MD YT, zlib level 6 blocks) typed (a) by the host path (samin.AlignmentSample.add_file + .stats() + .pileup) and (b) on the device
(Engine.submit_bam_file + stats, Engine.pileup_bam_file), both on the SAME file.  One JSON line; the figures of profiles/bam_gpu.md
come from it.  N_RECORDS [2000000]; CHUNK_BYTES [64 MiB] of compressed bytes per call of the device path.
The script is a driver: it writes the file, then runs the two GPU steps as child processes of their own (`--step host|device DIR`),
each under its own time limit, the second only if the first ended well; nothing is tried again.  The device step checks its
statistics and pile-up against what the host step left in DIR."""
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd import samin, synth  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402
from metamlst_amd.typing import pick_alleles_fast  # noqa: E402


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_bam(path, idx, n, seed=1):
    """n records, 20 per read name: the read's best allele and 19 neighbours of the same locus"""
    rng = np.random.default_rng(seed)
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles)]
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs)))
    for nm, ln in refs:
        out += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    nib = np.array([1, 2, 4, 8], np.uint8)
    with open(path, "wb") as f:
        def flush(final=False):
            nonlocal out
            while len(out) >= 65280 or (final and out):
                f.write(bgzf_block(bytes(out[:65280]))); del out[:65280]
        for r in range((n + 19) // 20):
            l = int(rng.integers(0, idx.n_loci)); b0 = int(idx.locus_begin[l]); cnt = int(idx.locus_count[l])
            codes = nib[rng.integers(0, 4, size=150)]
            packed = ((codes[0::2] << 4) | codes[1::2]).tobytes(); qual = rng.integers(20, 41, size=150).astype(np.uint8).tobytes()
            name = b"read%d\0" % r
            for k in range(min(20, n - 20 * r)):
                a = b0 + (r + k) % cnt; pos = int(rng.integers(0, max(1, refs[a][1] - 150)))
                aux = (b"ASC" + bytes([max(0, 250 - 6 * k)]) + b"XSC" + bytes([200]) + b"XNC\0" + b"XMC" + bytes([k % 6]) + b"XOC\0XGC\0" + b"NMC" + bytes([k % 6])
                       + b"MDZ150\0YTZUU\0")
                body = struct.pack("<iiBBHHHiiii", a, pos, len(name), 255, 4680, 1, 0 if k == 0 else 256, 150, -1, -1, 0) + name + struct.pack("<I", 150 << 4) + packed + qual + aux
                out += struct.pack("<i", len(body)) + body
            flush()
        flush(True)
        f.write(bgzf_block(b""))
    return len(text)


N = int(os.environ.get("N_RECORDS", "2000000"))
CHUNK = int(os.environ.get("CHUNK_BYTES", str(64 << 20)))
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")


def step_host(d):
    idx = load_index(d + "/e.db")
    eng = Engine(0)
    eng.load_reference(idx)
    t0 = time.perf_counter()
    smp = samin.AlignmentSample(idx).add_file(d + "/big.bam")
    st = smp.stats()
    t1 = time.perf_counter()
    chosen = sorted(pick_alleles_fast(idx, st, 100).values())
    t2 = time.perf_counter()
    pile = smp.pileup(eng, chosen)
    t3 = time.perf_counter()
    np.savez(d + "/host.npz", chosen=np.array(chosen), counters=st.counters, **{f: getattr(st, f) for f in FIELDS}, **{"p%d" % a: pile[a] for a in chosen})
    print(json.dumps({"pass1_s": t1 - t0, "pileup_s": t3 - t2, "records_per_s": N / ((t1 - t0) + (t3 - t2))}))


def step_device(d):
    import threading

    import torch
    idx = load_index(d + "/e.db")
    eng = Engine(0)
    eng.load_reference(idx)
    eng.set_bgzf_verify(os.environ.get("VERIFY", "1") == "1")
    torch.cuda.synchronize()
    base_free = torch.cuda.mem_get_info()[0]
    low = [base_free]
    stop = threading.Event()

    def watch():      # the least free device memory seen while the sample is typed (polled: a lower bound of the peak)
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    th = threading.Thread(target=watch, daemon=True)
    th.start()
    best, small = None, None
    for rep in range(6):      # three runs with CHUNK_BYTES a call, then three with an eighth of it (several pieces: copy and kernels overlap)
        chunk = CHUNK if rep < 3 else max(1 << 20, CHUNK // 8)
        if rep == 3:
            best, small = None, best
        eng.reset_sample()
        t0 = time.perf_counter()
        n = eng.submit_bam_file(d + "/big.bam", chunk_bytes=chunk)
        st = eng.stats()
        t1 = time.perf_counter()
        chosen = sorted(pick_alleles_fast(idx, st, 100).values())
        t2 = time.perf_counter()
        pile = eng.pileup_bam_file(d + "/big.bam", chosen, chunk_bytes=chunk)
        t3 = time.perf_counter()
        assert n == N
        cur = {"pass1_s": t1 - t0, "pass2_s": t3 - t2, "records_per_s": N / ((t1 - t0) + (t3 - t2))}
        if best is None or cur["records_per_s"] > best["records_per_s"]:
            best = cur
    stop.set(); th.join()
    best, small = small, best
    best["eighth_chunks"] = {k: small[k] for k in ("pass1_s", "pass2_s", "records_per_s")}
    best["peak_device_bytes_of_the_stream"] = int(base_free - low[0])
    h = np.load(d + "/host.npz")
    assert all(np.array_equal(getattr(st, f), h[f]) for f in FIELDS) and np.array_equal(st.counters[:2], h["counters"][:2]), "statistics differ from the host path"
    assert chosen == [int(a) for a in h["chosen"]] and all(np.array_equal(pile[a], h["p%d" % a]) for a in chosen), "pile-up differs from the host path"
    best["equal_to_host"] = True
    print(json.dumps(best))


if len(sys.argv) == 4 and sys.argv[1] == "--step":
    {"host": step_host, "device": step_device}[sys.argv[2]](sys.argv[3])
    sys.exit(0)

d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
idx = load_index(db.path)
write_bam(d + "/big.bam", idx, N)
import gzip  # noqa: E402

inflated = 0
with gzip.open(d + "/big.bam", "rb") as z:
    while True:
        blk = z.read(1 << 24)
        if not blk:
            break
        inflated += len(blk)
out = {"records": N, "bgzf_bytes": os.path.getsize(d + "/big.bam"), "inflated_bytes": inflated, "chunk_bytes": CHUNK}
for name, limit in (("host", int(os.environ.get("HOST_TIMEOUT", "600"))), ("device", int(os.environ.get("DEVICE_TIMEOUT", "180")))):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, d], stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:      # a step that failed or ran out of time ends the run: nothing is started behind it
        print(json.dumps(dict(out, failed=name, returncode=r.returncode)))
        sys.exit(1)
    out[name] = json.loads(r.stdout.strip().splitlines()[-1])
out["device"]["pass1_GBps_inflated"] = inflated / out["device"]["pass1_s"] / 1e9
out["device"]["pass2_GBps_inflated"] = inflated / out["device"]["pass2_s"] / 1e9
out["speedup_records_per_s"] = out["device"]["records_per_s"] / out["host"]["records_per_s"]
print(json.dumps(out))
