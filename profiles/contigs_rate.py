#!/usr/bin/env python3
"""Rate of typing assemblies (`cli type --contigs`): one GENOME_MB [5] Mb assembly in 40 contigs (70-column lines), and N_FOLDER [64]
of them as a folder.
(a) the path of the commit before: fastq.tile_fasta on the host feeding Engine.submit_fastq, one file after the other;
(b) on the device: Engine.submit_fasta_file; for the folder `cli type folder/ --contigs` (multigpu.type_many_samples).
Both in this process, five runs each, alternated; medians.  Shares of a single-genome run: `host` is the time spent making the input
(tile_fasta's text / reading the file's chunks), `device` the rest (copies, kernels, the wait for the statistics).  The folder
baseline types every file (tile_fasta + submit_fastq + typing tail) on one engine without writing .nfo files, which favours it.
One JSON line, and profiles/contigs.md next to this script."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd import synth  # noqa: E402
from metamlst_amd.cli import main  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.fastq import fasta_chunks, tile_fasta  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

MB = float(os.environ.get("GENOME_MB", "5"))
N_FOLDER = int(os.environ.get("N_FOLDER", "64"))
TILE = (150, 25, 50)
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")


def write_assembly(path, db, row, seed):
    g, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][row], size=int(MB * 1e6), seed=seed)
    s = g.tobytes()
    cuts = np.linspace(0, len(s), 41).astype(int)
    with open(path, "wb") as f:
        for k in range(40):
            c = s[cuts[k]:cuts[k + 1]]
            f.write(b">contig%d\n" % k + b"".join(c[i:i + 70] + b"\n" for i in range(0, len(c), 70)))


def timed_iter(it, box):
    """the iterator's items, the time spent inside it added to box[0]"""
    while True:
        t = time.perf_counter()
        try:
            x = next(it)
        except StopIteration:
            box[0] += time.perf_counter() - t
            return
        box[0] += time.perf_counter() - t
        yield x


def run_host(eng, path):
    eng.reset_sample()
    host = [0.0]
    t0 = time.perf_counter()
    n = sum(eng.submit_fastq(c) for c in timed_iter(tile_fasta(path, *TILE), host))
    st = eng.stats()
    return time.perf_counter() - t0, host[0], n, st


def run_device(eng, path):
    eng.reset_sample()
    host = [0.0]
    t0 = time.perf_counter()
    n = sum(eng.submit_fasta(c, *TILE)[1] for c in timed_iter(fasta_chunks(path, 64 << 20), host))
    st = eng.stats()
    return time.perf_counter() - t0, host[0], n, st


d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
idx = load_index(d + "/e.db")
os.mkdir(d + "/asm")
for k in range(N_FOLDER):
    write_assembly(d + "/asm/g%03d.fna" % k, db, k % 50, 1000 + k)
one = d + "/asm/g000.fna"
eng = Engine(0)
eng.load_reference(idx)
run_host(eng, one); run_device(eng, one)      # (buffers allocated, graphs captured)
legs = {"host": [], "device": []}
for _ in range(5):
    for name, fn in (("host", run_host), ("device", run_device)):
        legs[name].append(fn(eng, one))
assert legs["host"][0][2] == legs["device"][0][2]
assert all(np.array_equal(getattr(legs["host"][0][3], f), getattr(legs["device"][0][3], f)) for f in FIELDS), "statistics differ"
n_reads = legs["host"][0][2]
out = {"genome_mb": MB, "reads_per_genome": n_reads, "file_bytes": os.path.getsize(one), "n_folder": N_FOLDER}
for name in legs:
    tot = statistics.median(x[0] for x in legs[name]); host = statistics.median(x[1] for x in legs[name])
    out[name] = {"seconds": tot, "host_s": host, "device_s": tot - host, "genomes_per_s": 1 / tot, "reads_per_s": n_reads / tot}
files = sorted(os.path.join(d, "asm", f) for f in os.listdir(d + "/asm"))
folder = {"host": [], "device": []}
for r in range(5):
    t0 = time.perf_counter()
    for f in files:
        eng.reset_sample()
        for c in tile_fasta(f, *TILE):
            eng.submit_fastq(c)
        eng.typing_enqueue(); eng.typing_fetch()
    folder["host"].append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    assert main(["type", d + "/asm", "--contigs", "-d", d + "/e.db", "-o", d + "/out%d" % r, "--quiet"]) == 0
    folder["device"].append(time.perf_counter() - t0)      # (includes the command's start: database, engines, index upload)
for name in folder:
    t = statistics.median(folder[name])
    out["folder_" + name] = {"seconds": t, "genomes_per_s": N_FOLDER / t, "reads_per_s": N_FOLDER * n_reads / t}
out["device_over_host"] = out["device"]["reads_per_s"] / out["host"]["reads_per_s"]
out["folder_device_over_host"] = out["folder_device"]["reads_per_s"] / out["folder_host"]["reads_per_s"]
print(json.dumps(out))
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "contigs.md"), "w") as f:
    f.write("# Typing assemblies: contigs tiled on the host and on the device\n\n`python profiles/contigs_rate.py` (medians of five alternated runs; "
            "%g Mb genome in 40 contigs, %d reads at --tile 150,25; folder of %d).\n\n" % (MB, n_reads, N_FOLDER))
    f.write("| path | seconds | host share s | device share s | genomes/s | reads/s |\n|---|---|---|---|---|---|\n")
    for name, label in (("host", "tile_fasta + submit_fastq"), ("device", "submit_fasta_file")):
        o = out[name]
        f.write("| %s | %.4f | %.4f | %.4f | %.1f | %.3g |\n" % (label, o["seconds"], o["host_s"], o["device_s"], o["genomes_per_s"], o["reads_per_s"]))
    for name, label in (("folder_host", "folder: one file after the other, host tiling"), ("folder_device", "folder: cli type folder/ --contigs")):
        o = out[name]
        f.write("| %s | %.3f | | | %.1f | %.3g |\n" % (label, o["seconds"], o["genomes_per_s"], o["reads_per_s"]))
    f.write("\n```\n%s\n```\n" % json.dumps(out))
