#!/usr/bin/env python3
"""Rate of typing long reads from an unaligned BAM (`cli type hifi.bam --long-bam-reads`, mlst_set_read_tiling on a reads stream):
N_LONG [50,000] reads of 10,000 bases and N_SHORT [1,000,000] reads of 600 bases, drawn from a 5 Mb genome with a planted ST, as an
unaligned BGZF BAM (FLAG 4, no reference, zlib level 1 blocks of 65,280 bytes) and the same reads as bgzip'd FASTQ, at --tile 150,25
and 300,150.
(a) what had to be done before: samin.bam_reads_fastq on the host into a FASTQ file, fastq.tile_fastq over it feeding
    Engine.submit_fastq with tiling off -- one run; the conversion's and the tiling's share are given separately;
(b) the tiled BAM stream: Engine.set_read_tiling + submit_bam_reads_file (best of three after a warm-up, with the range), and one more
    run under HIP events for k_bamt_count + k_fqt_scan + k_fqt_add (id 13) and k_bamt_emit (id 14);
(c) the same reads as bgzip'd FASTQ through the tiled FASTQ path: submit_fastq_bgzf_file (best of three, with the range).
(b) and (c) must give the statistics of (a), bit for bit.  The script is a driver: it writes the files of a case, then runs each leg
as a child process of its own (`--step host|device|fastq DIR CASE`) under its own time limit, the next only if the one before ended
well; nothing is tried again.  One JSON line per case and one in all; the table goes into profiles/bam_long_reads.md between its
`rates` markers."""
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd import samin, synth  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.fastq import tile_fastq  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

N_SHORT = int(os.environ.get("N_SHORT", "1000000"))
N_LONG = int(os.environ.get("N_LONG", "50000"))
CASES = {"long": (N_LONG, 10_000), "short": (N_SHORT, 600)}
TILES = ((150, 25), (300, 150))
CHUNK = int(os.environ.get("CHUNK_BYTES", str(64 << 20)))
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")
COUNTERS = (0, 1, 2, 4, 5, 6)
NAME = 12      # b"r%010d\0"


def bgzf_block(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(comp) + 25).to_bytes(2, "little") + comp
            + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + len(data).to_bytes(4, "little"))


def write_bgzf(path, data):
    mv = memoryview(data)
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as f:      # (zlib releases the GIL)
        for blk in ex.map(lambda i: bgzf_block(mv[i:i + 65280]), range(0, len(mv), 65280)):
            f.write(blk)
        f.write(bgzf_block(b""))


def write_files(d, case, genome):
    """n reads of `length` (even) bases from either strand of the genome, Phred of base i of read r: (7 i + r) % 41, as
    d/<case>.bam (unmapped records) and d/<case>.fastq.gz (bgzip), the same reads under the same names in the same order"""
    n, length = CASES[case]
    rng = np.random.default_rng(7 + length)
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    nib = np.zeros(256, np.uint8)
    nib[[65, 67, 71, 84]] = [1, 2, 4, 8]
    fq_rec = 1 + NAME + length + 3 + length + 1      # "@" name-with-LF-for-NUL bases "\n+\n" quals "\n"
    bam_rec = 4 + 32 + NAME + length // 2 + length
    head = struct.pack("<iiiBBHHHiiii", bam_rec - 4, -1, -1, NAME, 0, 4680, 0, 4, length, -1, -1, 0)
    text = "@HD\tVN:1.6\tSO:unsorted\n"
    bam = np.empty(12 + len(text) + n * bam_rec, np.uint8)
    bam[:12 + len(text)] = np.frombuffer(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 0), np.uint8)
    rows = bam[12 + len(text):].reshape(n, bam_rec)
    fq = np.empty((n, fq_rec), np.uint8)
    step = max(1, (64 << 20) // length)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        start = rng.integers(0, len(genome) - length, size=hi - lo)
        b = genome[start[:, None] + np.arange(length)[None, :]]
        rev = rng.random(hi - lo) < 0.5
        b[rev] = comp[b[rev][:, ::-1]]
        q = ((7 * np.arange(length)[None, :] + np.arange(lo, hi)[:, None]) % 41).astype(np.uint8)
        names = np.frombuffer(b"".join(b"r%010d\0" % r for r in range(lo, hi)), np.uint8).reshape(-1, NAME)
        rows[lo:hi, :36] = np.frombuffer(head, np.uint8)
        rows[lo:hi, 36:36 + NAME] = names
        nb = nib[b]
        rows[lo:hi, 36 + NAME:36 + NAME + length // 2] = (nb[:, 0::2] << 4) | nb[:, 1::2]
        rows[lo:hi, 36 + NAME + length // 2:] = q
        fq[lo:hi, 0] = ord("@")
        fq[lo:hi, 1:1 + NAME] = names
        fq[lo:hi, NAME] = 10      # (the NUL that ends QNAME: the line end here)
        fq[lo:hi, 1 + NAME:1 + NAME + length] = b
        fq[lo:hi, 1 + NAME + length:4 + NAME + length] = np.frombuffer(b"\n+\n", np.uint8)
        fq[lo:hi, 4 + NAME + length:fq_rec - 1] = q + 33
        fq[lo:hi, fq_rec - 1] = 10
    write_bgzf(d + "/%s.bam" % case, bam)
    write_bgzf(d + "/%s.fastq.gz" % case, fq.reshape(-1))
    return {"reads": n, "bases": length, "bam_inflated_bytes": int(bam.size), "bam_bytes": os.path.getsize(d + "/%s.bam" % case),
            "fastq_text_bytes": int(fq.size), "fastq_bgzf_bytes": os.path.getsize(d + "/%s.fastq.gz" % case)}


def engine(d):
    eng = Engine(0)
    eng.load_reference(load_index(d + "/e.db"))
    return eng


def step_host(d, case):
    eng = engine(d)
    out = {}
    t0 = time.perf_counter()
    with open(d + "/host.fastq", "wb") as f:
        for chunk in samin.bam_reads_fastq(d + "/%s.bam" % case):
            f.write(chunk)
    out["bam_reads_fastq_s"] = time.perf_counter() - t0
    for tile in TILES:
        eng.reset_sample()
        eng.set_read_tiling(0, 0)
        host, n = 0.0, 0
        t0 = time.perf_counter()
        it = tile_fastq(d + "/host.fastq", *tile)
        while True:
            t = time.perf_counter()
            c = next(it, None)
            host += time.perf_counter() - t
            if c is None:
                break
            n += eng.submit_fastq(c)
        st = eng.stats()
        t1 = time.perf_counter()
        np.savez(d + "/host_%s_%d.npz" % (case, tile[0]), counters=st.counters, n=n, **{f: getattr(st, f) for f in FIELDS})
        out["%d,%d" % tile] = {"reads": n, "tile_fastq_s": host, "submit_s": t1 - t0 - host, "seconds": out["bam_reads_fastq_s"] + t1 - t0}
    os.unlink(d + "/host.fastq")
    print(json.dumps(out))


def best_of_three(d, case, submit, events):
    eng = engine(d)
    out = {}
    for tile in TILES:
        h = np.load(d + "/host_%s_%d.npz" % (case, tile[0]))
        eng.reset_sample()
        eng.set_read_tiling(*tile)
        submit(eng)      # (buffers allocated, graphs captured)
        runs = []
        for _ in range(3):
            eng.reset_sample()
            t0 = time.perf_counter()
            n = submit(eng)
            st = eng.stats()
            runs.append(time.perf_counter() - t0)
            assert n == int(h["n"]), (n, int(h["n"]))
            assert all(np.array_equal(getattr(st, f), h[f]) for f in FIELDS) and all(int(st.counters[c]) == int(h["counters"][c]) for c in COUNTERS), "statistics differ from leg (a)"
        o = {"reads": n, "seconds": min(runs), "range": [min(runs), max(runs)], "equal_to_host": True, "info": eng.read_tiling_info()}
        if events:      # (a run of its own: events switch the graph replay off)
            eng.set_profiling(1)
            eng.reset_kernel_time()
            eng.reset_sample()
            submit(eng)
            eng.stats()
            (ms_scan, n_scan), (ms_emit, n_emit) = eng.kernel_time(13), eng.kernel_time(14)
            eng.set_profiling(0)
            o.update(pieces_cut=n_scan, count_scan_add_ms=ms_scan, rounds=n_emit, emit_ms=ms_emit)
        out["%d,%d" % tile] = o
    print(json.dumps(out))


def step_device(d, case):
    best_of_three(d, case, lambda eng: eng.submit_bam_reads_file(d + "/%s.bam" % case, chunk_bytes=CHUNK), True)


def step_fastq(d, case):
    best_of_three(d, case, lambda eng: eng.submit_fastq_bgzf_file(d + "/%s.fastq.gz" % case), False)


if len(sys.argv) == 5 and sys.argv[1] == "--step":
    {"host": step_host, "device": step_device, "fastq": step_fastq}[sys.argv[2]](sys.argv[3], sys.argv[4])
    sys.exit(0)

d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][7], size=5_000_000)
out = {"chunk_bytes": CHUNK, "cases": {}}
for case in CASES:
    c = write_files(d, case, genome)
    for name, limit in (("host", int(os.environ.get("HOST_TIMEOUT", "600"))), ("device", int(os.environ.get("DEVICE_TIMEOUT", "180"))),
                        ("fastq", int(os.environ.get("DEVICE_TIMEOUT", "180")))):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, d, case], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:      # a leg that failed or ran out of time ends the run: nothing is started behind it
            print(json.dumps(dict(out, failed=[case, name], returncode=r.returncode)))
            sys.exit(1)
        c[name] = json.loads(r.stdout.strip().splitlines()[-1])
    out["cases"][case] = c
    print(json.dumps({case: c}), flush=True)
    os.unlink(d + "/%s.bam" % case)
    os.unlink(d + "/%s.fastq.gz" % case)
print(json.dumps(out))
rows = ["| reads | tile | windows + uncut | leg | seconds (range) | Mreads/s | |", "|---|---|---|---|---|---|---|"]
for case, c in out["cases"].items():
    label = "%d x %d" % (c["reads"], c["bases"])
    for tile in ("%d,%d" % t for t in TILES):
        a, b, f = c["host"][tile], c["device"][tile], c["fastq"][tile]
        rows.append("| %s | %s | %d | (a) bam_reads_fastq + tile_fastq + submit_fastq (one run) | %.2f, of which conversion %.2f, tile_fastq %.2f | %.3f | |"
                    % (label, tile, a["reads"], a["seconds"], c["host"]["bam_reads_fastq_s"], a["tile_fastq_s"], a["reads"] / a["seconds"] / 1e6))
        rows.append("| %s | %s | %d | (b) tiled submit_bam_reads_file | %.4f (%.4f-%.4f) | %.1f | (b) / (a) = %.0f, (b) / (c) = %.2f; %.1f GB/s of inflated BAM |"
                    % (label, tile, b["reads"], b["seconds"], b["range"][0], b["range"][1], b["reads"] / b["seconds"] / 1e6, a["seconds"] / b["seconds"], f["seconds"] / b["seconds"],
                       c["bam_inflated_bytes"] / b["seconds"] / 1e9))
        rows.append("| %s | %s | %d | (c) tiled submit_fastq_bgzf_file | %.4f (%.4f-%.4f) | %.1f | |" % (label, tile, f["reads"], f["seconds"], f["range"][0], f["range"][1], f["reads"] / f["seconds"] / 1e6))
rows += ["", "| reads | tile | pieces with a cut read | k_bamt_count + k_fqt_scan + k_fqt_add ms (all pieces) | rounds | k_bamt_emit ms (all rounds) |", "|---|---|---|---|---|---|"]
for case, c in out["cases"].items():
    for tile in ("%d,%d" % t for t in TILES):
        b = c["device"][tile]
        rows.append("| %d x %d | %s | %d | %.3f | %d | %.3f |" % (c["reads"], c["bases"], tile, b["pieces_cut"], b["count_scan_add_ms"], b["rounds"], b["emit_ms"]))
body = "\n".join(rows) + "\n\n```\n%s\n```\n" % json.dumps(out)
md = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bam_long_reads.md")
old = open(md).read() if os.path.exists(md) else "# Long reads of a BAM cut into windows on the device\n\n<!-- rates -->\n<!-- /rates -->\n"
a, b = old.index("<!-- rates -->") + len("<!-- rates -->"), old.index("<!-- /rates -->")
with open(md, "w") as f:
    f.write(old[:a] + "\n" + body + old[b:])
