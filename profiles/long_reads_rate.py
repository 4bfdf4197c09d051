#!/usr/bin/env python3
"""Rate of typing long reads (`cli type --long-reads`, mlst_set_read_tiling): N_SHORT [1,000,000] records of 600 bases (merged pairs)
and N_LONG [50,000] records of 10,000 bases, drawn from a 5 Mb genome with a planted ST, at --tile 150,25 and 300,150.
(a) on the device: Engine.set_read_tiling + submit_fastq of the text in chunks of 256 MB, and submit_fastq_bgzf_file of the bgzip'd
    file; three runs each after a warm-up, medians; reads/s counts windows plus uncut records, GB/s the FASTQ text of the records;
(b) what had to be done before: fastq.tile_fastq on the host feeding submit_fastq with tiling off -- one run; the host's share (the
    time inside tile_fastq) is given separately, and the rest (copies, kernels: LEN / STEP times the text over the link) alone;
(c) k_fqt_count + k_fqt_scan + k_fqt_add and k_fqt_emit per chunk, from HIP events (a run of its own: events switch the graph replay off).
The statistics of (a) and (b) must be equal.  One JSON line; the table goes into profiles/long_reads.md between its `rates` markers."""
import json
import os
import statistics
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
from metamlst_amd import synth  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.fastq import tile_fastq  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

N_SHORT = int(os.environ.get("N_SHORT", "1000000"))
N_LONG = int(os.environ.get("N_LONG", "50000"))
TILES = ((150, 25), (300, 150))
CHUNK = 256 << 20
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")


def fastq_text(genome, n, length, seed):
    """n records of `length` bases from either strand of the genome as one uint8 array; Phred of base i of record r: (7 i + r) % 41"""
    rng = np.random.default_rng(seed)
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    name = 13      # b"@r%010d\n"
    rec = name + length + 3 + length + 1
    out = np.empty((n, rec), np.uint8)
    for lo in range(0, n, 65536):
        hi = min(n, lo + 65536)
        start = rng.integers(0, len(genome) - length, size=hi - lo)
        b = genome[start[:, None] + np.arange(length)[None, :]]
        rev = rng.random(hi - lo) < 0.5
        b[rev] = comp[b[rev][:, ::-1]]
        out[lo:hi, :name] = np.frombuffer(b"".join(b"@r%010d\n" % r for r in range(lo, hi)), np.uint8).reshape(-1, name)
        out[lo:hi, name:name + length] = b
        out[lo:hi, name + length:name + length + 3] = np.frombuffer(b"\n+\n", np.uint8)
        out[lo:hi, name + length + 3:rec - 1] = ((7 * np.arange(length)[None, :] + np.arange(lo, hi)[:, None]) % 41 + 33).astype(np.uint8)
        out[lo:hi, rec - 1] = 10
    return out.reshape(-1), rec


def bgzf_block(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(comp) + 25).to_bytes(2, "little") + comp
            + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + len(data).to_bytes(4, "little"))


def write_bgzf(path, text):
    mv = memoryview(text)
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as f:      # (zlib releases the GIL)
        for blk in ex.map(lambda i: bgzf_block(mv[i:i + 65280]), range(0, len(mv), 65280)):
            f.write(blk)
        f.write(bgzf_block(b""))


def run_text(eng, text, rec, tile):
    eng.reset_sample()
    eng.set_read_tiling(*tile)
    per = max(1, CHUNK // rec) * rec
    t0 = time.perf_counter()
    n = sum(eng.submit_fastq(text[at:at + per]) for at in range(0, text.size, per))
    st = eng.stats()
    return time.perf_counter() - t0, n, st


def run_bgzf(eng, path, tile):
    eng.reset_sample()
    eng.set_read_tiling(*tile)
    t0 = time.perf_counter()
    n = eng.submit_fastq_bgzf_file(path)
    st = eng.stats()
    return time.perf_counter() - t0, n, st


def run_host(eng, path, tile):
    eng.reset_sample()
    eng.set_read_tiling(0, 0)
    host, n = 0.0, 0
    t0 = time.perf_counter()
    it = tile_fastq(path, *tile)
    while True:
        t = time.perf_counter()
        c = next(it, None)
        host += time.perf_counter() - t
        if c is None:
            break
        n += eng.submit_fastq(c)
    st = eng.stats()
    return time.perf_counter() - t0, host, n, st


d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
idx = load_index(d + "/e.db")
genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][7], size=5_000_000)
eng = Engine(0)
eng.load_reference(idx)
out = {"n_short": N_SHORT, "n_long": N_LONG, "cases": []}
for label, n_rec, length in (("%d x 600" % N_SHORT, N_SHORT, 600), ("%d x 10000" % N_LONG, N_LONG, 10_000)):
    text, rec = fastq_text(genome, n_rec, length, 7 + length)
    plain, bz = d + "/r%d.fastq" % length, d + "/r%d.fastq.gz" % length
    text.tofile(plain)
    write_bgzf(bz, text)
    for tile in TILES:
        run_text(eng, text, rec, tile)      # (buffers allocated, graphs captured)
        run_bgzf(eng, bz, tile)
        legs = {"text": [run_text(eng, text, rec, tile) for _ in range(3)], "bgzf": [run_bgzf(eng, bz, tile) for _ in range(3)]}
        info = eng.read_tiling_info()
        th, host_s, nh, sth = run_host(eng, plain, tile)
        n_reads = legs["text"][0][1]
        assert nh == n_reads and legs["bgzf"][0][1] == n_reads, (nh, n_reads, legs["bgzf"][0][1])
        for leg in legs.values():
            assert all(np.array_equal(getattr(leg[0][2], f), getattr(sth, f)) for f in FIELDS), "statistics differ"
        eng.set_profiling(1)
        eng.reset_kernel_time()
        run_text(eng, text, rec, tile)
        (ms_scan, n_scan), (ms_emit, n_emit), (ms_pack, _) = eng.kernel_time(13), eng.kernel_time(14), eng.kernel_time(6)
        eng.set_profiling(0)
        c = {"records": label, "tile": "%d,%d" % tile, "reads": n_reads, "text_gb": text.size / 1e9, "bgzf_gb": os.path.getsize(bz) / 1e9, "info": info,
             "chunks": n_scan, "count_scan_add_ms_per_chunk": ms_scan / max(1, n_scan), "emit_ms_per_chunk": ms_emit / max(1, n_emit), "parse_and_pack_ms_total": ms_pack,
             "host": {"seconds": th, "tile_fastq_s": host_s, "rest_s": th - host_s, "reads_per_s": n_reads / th, "reads_per_s_without_tiling_time": n_reads / (th - host_s)}}
        for name, leg in legs.items():
            t = statistics.median(x[0] for x in leg)
            c[name] = {"seconds": t, "range": [min(x[0] for x in leg), max(x[0] for x in leg)], "reads_per_s": n_reads / t, "text_gb_per_s": text.size / 1e9 / t}
        out["cases"].append(c)
        print(json.dumps(c), flush=True)
    del text
print(json.dumps(out))
rows = ["| records | tile | reads | path | seconds (range) | Mreads/s | GB/s of text |", "|---|---|---|---|---|---|---|"]
for c in out["cases"]:
    for name, lab in (("text", "tiled submit_fastq, plain text"), ("bgzf", "tiled submit_fastq_bgzf_file")):
        o = c[name]
        rows.append("| %s | %s | %d | %s | %.3f (%.3f-%.3f) | %.1f | %.2f |" % (c["records"], c["tile"], c["reads"], lab, o["seconds"], o["range"][0], o["range"][1], o["reads_per_s"] / 1e6, o["text_gb_per_s"]))
    h = c["host"]
    rows.append("| %s | %s | %d | tile_fastq + submit_fastq (one run) | %.2f, of which tile_fastq %.2f | %.2f (%.1f without the tiling time) | |"
                % (c["records"], c["tile"], c["reads"], h["seconds"], h["tile_fastq_s"], h["reads_per_s"] / 1e6, h["reads_per_s_without_tiling_time"] / 1e6))
rows += ["", "| records | tile | chunks | k_fqt_count + k_fqt_scan + k_fqt_add ms / chunk | k_fqt_emit ms / chunk |", "|---|---|---|---|---|"]
rows += ["| %s | %s | %d | %.3f | %.3f |" % (c["records"], c["tile"], c["chunks"], c["count_scan_add_ms_per_chunk"], c["emit_ms_per_chunk"]) for c in out["cases"]]
body = "\n".join(rows) + "\n\n```\n%s\n```\n" % json.dumps(out)
md = os.path.join(os.path.dirname(os.path.abspath(__file__)), "long_reads.md")
old = open(md).read() if os.path.exists(md) else "# Long reads cut into windows on the device\n\n<!-- rates -->\n<!-- /rates -->\n"
a, b = old.index("<!-- rates -->") + len("<!-- rates -->"), old.index("<!-- /rates -->")
with open(md, "w") as f:
    f.write(old[:a] + "\n" + body + old[b:])
