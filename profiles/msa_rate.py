#!/usr/bin/env python3
"""Rate of the centre-star alignment behind `merge --outseqformat A --aligner gpu` (mlst_msa_align + mlst_msa_fetch, csrc/msa_dev.h).
Inputs: the alleles of one PubMLST-shaped locus (`secondary_skewed` of bench.py: thousands of near-identical alleles of 450-500
bases with length variants) at 3,000 and at 8,209 sequences, and 50 sequences of 4,000 bases.
Timed: Engine.align_center_star, i.e. the copy of the sequences to the device, every kernel and the fetch of the rows (median of five
calls after one warm-up call), and the device time per DP cell, cells = sum over the rows of len(row) * len(centre).
Next to it: the host statement metamlst_amd.msa.center_star on HOST_ROWS [200] rows of the same input (the centre's row included),
scaled by pairs to the whole input and marked so, and MUSCLE where a binary is installed.
One JSON line, and profiles/msa.md next to this script."""
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.msa import center_star, pick_center  # noqa: E402

HOST_ROWS = int(os.environ.get("HOST_ROWS", "200"))


def locus(n_rows, length, seed):
    """Alleles of one locus: an ancestor, every row with 0-8 SNPs; one row in five carries an indel of 1-12 bases."""
    rng = random.Random(seed)
    anc = bytes(rng.choice(b"ACGT") for _ in range(length))
    rows = [anc]
    while len(rows) < n_rows:
        b = bytearray(anc)
        for _ in range(rng.randint(0, 8)):
            b[rng.randrange(len(b))] = rng.choice(b"ACGT")
        if rng.random() < 0.2:
            at, g = rng.randrange(len(b)), rng.randint(1, 12)
            if rng.random() < 0.5:
                del b[at:at + g]
            else:
                b[at:at] = bytes(rng.choice(b"ACGT") for _ in range(g))
        rows.append(bytes(b))
    return rows


def muscle_seconds(seqs):
    exe = shutil.which("muscle")
    if exe is None:
        return None
    fa = "".join(">s%d\n%s\n" % (k, q.decode()) for k, q in enumerate(seqs)).encode()
    t0 = time.perf_counter()
    subprocess.run([exe], input=fa, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    return time.perf_counter() - t0


eng = Engine(0)
out = {"host_rows": HOST_ROWS, "inputs": []}
for name, seqs in (("locus of 3,000 alleles, ~470 bases", locus(3000, 470, 1)), ("locus of 8,209 alleles, ~470 bases", locus(8209, 470, 2)),
                   ("50 sequences of ~4,000 bases", locus(50, 4000, 3))):
    c = pick_center(seqs)
    cells = sum(len(q) for k, q in enumerate(seqs) if k != c) * len(seqs[c])
    eng.align_center_star(seqs)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = eng.align_center_star(seqs)
        times.append(time.perf_counter() - t0)
    t = statistics.median(times)
    sub = seqs[:HOST_ROWS] if c < HOST_ROWS else [seqs[c]] + seqs[:HOST_ROWS - 1]
    t0 = time.perf_counter()
    want = center_star(sub)
    th = time.perf_counter() - t0
    sub_got = eng.align_center_star(sub)
    assert sub_got[0] == want[0] and sub_got[1] == want[1], "device and statement differ on " + name
    tm = muscle_seconds(seqs)
    out["inputs"].append({"name": name, "sequences": len(seqs), "width": len(got[1][0]), "dp_cells": cells, "engine_s": t, "engine_runs_s": times,
                          "engine_ns_per_cell": t / cells * 1e9, "host_subset_rows": len(sub), "host_subset_s": th,
                          "host_scaled_s": th * (len(seqs) - 1) / max(1, len(sub) - 1), "muscle_s": tm})
print(json.dumps(out))
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "msa.md"), "w") as f:
    f.write("# Centre-star alignment of a locus' alleles: engine, host statement, MUSCLE\n\n`python profiles/msa_rate.py` (engine: median of five "
            "calls of Engine.align_center_star, copy-in and fetch included; host statement: metamlst_amd.msa.center_star on the first %d rows, "
            "scaled by pairs to the whole input; the engine's rows for that subset are compared with the statement's before anything is written).\n\n"
            % HOST_ROWS)
    f.write("| input | sequences | row width | DP cells | engine s | engine ns per cell | statement s (subset) | statement s (scaled) | MUSCLE s |\n|---|---|---|---|---|---|---|---|---|\n")
    for o in out["inputs"]:
        f.write("| %s | %d | %d | %.3g | %.4f | %.4f | %.2f (%d rows) | %.1f | %s |\n" % (
            o["name"], o["sequences"], o["width"], o["dp_cells"], o["engine_s"], o["engine_ns_per_cell"], o["host_subset_s"], o["host_subset_rows"],
            o["host_scaled_s"], "not installed" if o["muscle_s"] is None else "%.1f" % o["muscle_s"]))
    f.write("\nThe engine's time per cell is the wall time of the whole call over the cells of the DP, so it holds the traceback, the write-out and "
            "the copies too.  A wave computes up to 64 cells per step of its wavefront, and a call keeps as many waves busy as it has rows.\n\n"
            "```\n%s\n```\n" % json.dumps(out))
