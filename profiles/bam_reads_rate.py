#!/usr/bin/env python3
"""Rate of typing the READS of a BAM: N_READS [2000000] reads of 150 bases as an unaligned BGZF BAM (zlib level 6 blocks) typed
(a) by the only route there was before: samin.bam_reads_fastq on the host feeding Engine.submit_fastq,
(b) on the device: Engine.submit_bam_reads_file (best of three; reads/s and GB/s of inflated bytes; the device-memory high-water mark of the process from a fourth, untimed run),
(c) the same reads as bgzip'd FASTQ through Engine.submit_fastq_bgzf_file (best of three): what the rest of the input side allows.
One JSON line; the figures of profiles/bam_reads.md come from it.  The script is a driver: it writes the two files, then runs each
leg as a child process of its own (`--step host|device|fastq DIR`) under its own time limit, the next only if the one before ended
well; nothing is tried again.  Legs (b) and (c) check their statistics against what leg (a) left in DIR."""
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

N = int(os.environ.get("N_READS", "2000000"))
CHUNK = int(os.environ.get("CHUNK_BYTES", str(64 << 20)))
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_files(d, db):
    """the reads of an isolate as an unaligned BAM (FLAG 4, no reference) and as bgzip'd FASTQ, the same reads in the same order"""
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][3], size=2_000_000)
    b, q = synth.sample_reads(g, N, read_len=150)
    fb, fq, off = synth.flatten_reads(b, q)
    lut = np.full(256, 15, np.uint8); lut[[65, 67, 71, 84]] = [1, 2, 4, 8]
    text = "@HD\tVN:1.6\tSO:unsorted\n"
    bam = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 0))
    fastq = bytearray()
    with open(d + "/reads.bam", "wb") as fbam, open(d + "/reads.fastq.gz", "wb") as ffq:
        def flush(buf, f, final=False):
            while len(buf) >= 65280 or (final and buf):
                f.write(bgzf_block(bytes(buf[:65280]))); del buf[:65280]
        for r in range(N):
            lo, hi = int(off[r]), int(off[r + 1])
            nib = lut[fb[lo:hi]]
            if nib.size & 1:
                nib = np.append(nib, 0)
            name = b"read%d" % r
            body = (struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, hi - lo, -1, -1, 0) + name + b"\0"
                    + ((nib[0::2] << 4) | nib[1::2]).tobytes() + (fq[lo:hi] - 33).tobytes())
            bam += struct.pack("<i", len(body)) + body
            fastq += b"@" + name + b"\n" + fb[lo:hi].tobytes() + b"\n+\n" + fq[lo:hi].tobytes() + b"\n"
            if r % 256 == 0:
                flush(bam, fbam); flush(fastq, ffq)
        flush(bam, fbam, True); flush(fastq, ffq, True)
        fbam.write(bgzf_block(b"")); ffq.write(bgzf_block(b""))


def engine(d):
    idx = load_index(d + "/e.db")
    eng = Engine(0)
    eng.load_reference(idx)
    return eng


def step_host(d):
    eng = engine(d)
    t0 = time.perf_counter()
    n = sum(eng.submit_fastq(chunk) for chunk in samin.bam_reads_fastq(d + "/reads.bam"))
    st = eng.stats()
    t1 = time.perf_counter()
    assert n == N
    np.savez(d + "/host.npz", counters=st.counters, **{f: getattr(st, f) for f in FIELDS})
    print(json.dumps({"seconds": t1 - t0, "reads_per_s": N / (t1 - t0)}))


def best_of_three(d, submit):
    """three timed runs with nothing beside them, then a fourth, untimed one with a thread polling the free device memory"""
    import threading

    import torch
    eng = engine(d)
    best = None
    for _ in range(3):
        eng.reset_sample()
        t0 = time.perf_counter()
        n = submit(eng)
        st = eng.stats()
        t1 = time.perf_counter()
        assert n == N
        best = t1 - t0 if best is None else min(best, t1 - t0)
    h = np.load(d + "/host.npz")
    assert all(np.array_equal(getattr(st, f), h[f]) for f in FIELDS) and all(int(st.counters[c]) == int(h["counters"][c]) for c in (0, 1, 2, 4, 5, 6)), "statistics differ from leg (a)"
    torch.cuda.synchronize()
    total = torch.cuda.mem_get_info()[1]
    first = torch.cuda.mem_get_info()[0]
    low, stop = [first], threading.Event()

    def watch():      # the least free device memory seen during the run (polled: a lower bound of the peak)
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    th = threading.Thread(target=watch, daemon=True)
    th.start()
    eng.reset_sample(); submit(eng); eng.stats()
    stop.set(); th.join()
    # (figures of the whole device as the runtime reports them: the index, the engine's state and the buffers of the three runs before are in `before`)
    return {"seconds": best, "reads_per_s": N / best, "device_bytes_in_use_before": int(total - first), "device_bytes_in_use_high_water": int(total - low[0]), "equal_to_host": True}


def step_device(d):
    print(json.dumps(best_of_three(d, lambda eng: eng.submit_bam_reads_file(d + "/reads.bam", chunk_bytes=CHUNK))))


def step_fastq(d):
    print(json.dumps(best_of_three(d, lambda eng: eng.submit_fastq_bgzf_file(d + "/reads.fastq.gz"))))


if len(sys.argv) == 4 and sys.argv[1] == "--step":
    {"host": step_host, "device": step_device, "fastq": step_fastq}[sys.argv[2]](sys.argv[3])
    sys.exit(0)

d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
write_files(d, db)
names, lo, skip = samin.read_bam_header(d + "/reads.bam")
inflated = 12 + 23 + N * 36 + sum(len(b"read%d" % r) + 1 for r in range(N)) + N * 225
out = {"reads": N, "bam_bytes": os.path.getsize(d + "/reads.bam"), "bam_inflated_bytes": inflated, "fastq_bgzf_bytes": os.path.getsize(d + "/reads.fastq.gz"),
       "chunk_bytes": CHUNK}
for name, limit in (("host", int(os.environ.get("HOST_TIMEOUT", "900"))), ("device", int(os.environ.get("DEVICE_TIMEOUT", "180"))),
                    ("fastq", int(os.environ.get("DEVICE_TIMEOUT", "180")))):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, d], stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:      # a leg that failed or ran out of time ends the run: nothing is started behind it
        print(json.dumps(dict(out, failed=name, returncode=r.returncode)))
        sys.exit(1)
    out[name] = json.loads(r.stdout.strip().splitlines()[-1])
out["device"]["GBps_inflated"] = inflated / out["device"]["seconds"] / 1e9
out["device_over_host"] = out["device"]["reads_per_s"] / out["host"]["reads_per_s"]
out["device_over_fastq_bgzf"] = out["device"]["reads_per_s"] / out["fastq"]["reads_per_s"]
print(json.dumps(out))
