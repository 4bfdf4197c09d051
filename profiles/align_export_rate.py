#!/usr/bin/env python3
"""Cost of the alignment export behind `cli type --write-sam` (mlst_alignments_export + mlst_alignments_fetch, csrc/aln_export.h).
Samples: cfg1 of SURVEY.md 8(d) -- one isolate genome of 4.6 Mb, 100 k single-end reads of 150 bases, DB-ecoli (7 loci x 1,430
alleles) -- and the same model with 2 M reads.  Each is submitted and typed (mlst_typing_enqueue), then
  * Engine.pileup(chosen)            -- the pile-up the export restates, host copy of the counts included;
  * mlst_alignments_export           -- both of its waits included;
  * mlst_alignments_fetch            -- the copies of the record arrays to the host
are timed by a host clock around calls that end in a device synchronise: median of RUNS [7] calls after one warm-up call each.
Then the wall time of `python -m metamlst_amd.cli type <cfg1>.fastq` as a process of its own, without and with --write-sam,
alternating, CLI_RUNS [3] each (without the flag the command runs the code it ran before the flag existed).
`BENCH_AB='<ms per step of the commit before> <ms per step of this one> ...'` (pairs, alternating runs of bench.py --gpus 1 on one
machine in one session) and `KERNEL_RESOURCES=<text>` are copied into the report when set: bench.py never calls the export.
One JSON line, and profiles/align_export.md next to this script."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
import numpy as np  # noqa: E402

from metamlst_amd import synth  # noqa: E402
from metamlst_amd.engine import Engine, _ptr  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

RUNS = int(os.environ.get("RUNS", "7"))
CLI_RUNS = int(os.environ.get("CLI_RUNS", "3"))


def timed(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, [t * 1e3 for t in ts]


out = {"runs": RUNS, "samples": []}
with tempfile.TemporaryDirectory() as tmp:
    db = synth.make_ecoli_db(tmp + "/ecoli.db", alleles_per_locus=1430, n_profiles=5000)
    idx = load_index(tmp + "/ecoli.db")
    genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][3])
    eng = Engine(0)
    eng.load_reference(idx)
    fastq = None
    for name, n_reads in (("cfg1: 100 k reads", 100_000), ("2 M reads", 2_000_000)):
        b, q = synth.sample_reads(genome, n_reads)
        fb, fq, off = synth.flatten_reads(b, q)
        if fastq is None:
            fastq = tmp + "/cfg1.fastq"
            with open(fastq, "wb") as f:
                for k in range(n_reads):
                    f.write(b"@r%d\n" % k + b[k].tobytes() + b"\n+\n" + q[k].tobytes() + b"\n")
        eng.reset_sample()
        eng.submit_reads(fb, fq, off)
        eng.typing_enqueue(penalty=100)
        _, dev_chosen, _ = eng.typing_fetch()
        chosen = [dev_chosen[l] for l in sorted(dev_chosen)]
        ch = np.ascontiguousarray(chosen, np.uint32)
        n_items = len(eng.items(1 << 20))
        aln = eng.export_alignments(chosen)
        piled, again = eng.pileup(chosen), eng.pileup_alignments(chosen, *aln.pileup_arrays())
        assert all(np.array_equal(piled[a], again[a]) for a in chosen), "the exported records do not pile up to the pile-up's counts"
        nr, nc, ns = C.c_uint64(), C.c_uint64(), C.c_uint64()
        fields = [getattr(aln, f) for f in ("read_index", "allele", "pos0", "as_", "xm", "diag", "flags", "cigar_off", "cigar", "seq_off", "seq", "qual")]
        t_pile = timed(lambda: eng.pileup(chosen))
        t_exp = timed(lambda: eng._check(eng.lib.mlst_alignments_export(eng._h, _ptr(ch), len(ch), C.byref(nr), C.byref(nc), C.byref(ns)), "export"))
        t_fetch = timed(lambda: eng._check(eng.lib.mlst_alignments_fetch(eng._h, *[_ptr(x) for x in fields]), "fetch"))
        out["samples"].append({"name": name, "reads": n_reads, "items": n_items, "chosen": len(chosen), "records": len(aln), "banded_records": int((aln.flags >> 1).sum()),
                               "cigar_ops": len(aln.cigar), "bases": len(aln.seq), "pileup_ms": t_pile[0], "pileup_runs_ms": t_pile[1],
                               "export_ms": t_exp[0], "export_runs_ms": t_exp[1], "fetch_ms": t_fetch[0], "fetch_runs_ms": t_fetch[1]})
    eng.close()
    cli = {"without": [], "with": []}
    for r in range(CLI_RUNS + 1):                          # (the first pair warms the file cache and the index cache: dropped)
        for key, extra in (("without", []), ("with", ["--write-sam"])):
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "type", fastq, "-d", tmp + "/ecoli.db", "-o", "%s/out_%s_%d" % (tmp, key, r), "--quiet"] + extra,
                           cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
            if r:
                cli[key].append(time.perf_counter() - t0)
    a = open("%s/out_without_1/cfg1.nfo" % tmp, "rb").read()
    assert a == open("%s/out_with_1/cfg1.nfo" % tmp, "rb").read() and os.path.getsize("%s/out_with_1/cfg1.sam" % tmp) > 0
    out["cli_cfg1"] = {"without_s": cli["without"], "with_s": cli["with"], "sam_bytes": os.path.getsize("%s/out_with_1/cfg1.sam" % tmp)}
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_export.md"), "w") as f:
    f.write("# The alignment export (`cli type --write-sam`): what it costs\n\n`python profiles/align_export_rate.py` on one MI355X.  Host clock around calls "
            "that end in a device synchronise; median of %d calls after one warm-up call (every run is in the JSON below).  The exported records were piled up by "
            "`mlst_pileup_alignments` and compared with `mlst_pileup` before anything was timed.\n\n" % RUNS)
    f.write("| sample | work items | records (banded) | CIGAR operations | bases | pile-up ms | export ms | fetch ms |\n|---|---|---|---|---|---|---|---|\n")
    for s in out["samples"]:
        f.write("| %s | %d | %d (%d) | %d | %d | %.3f | %.3f | %.3f |\n" % (s["name"], s["items"], s["records"], s["banded_records"], s["cigar_ops"], s["bases"],
                                                                          s["pileup_ms"], s["export_ms"], s["fetch_ms"]))
    f.write("\nBoth samples are isolates: a few hundred to a few thousand of their reads lie on the seven loci, so the export is a handful of short launches and its "
            "two waits -- a sum of latencies, not a rate.  The pile-up column is `Engine.pileup` of the same alleles (launches, one wait, the copy of the counts).\n\n")
    c = out["cli_cfg1"]
    f.write("`cli type cfg1.fastq` as a process of its own, wall seconds, alternating, after one dropped pair: without the flag %s; with `--write-sam` %s (the file: "
            "%d bytes; the `.nfo` files are the same bytes).  Without the flag the command runs what it ran before the flag existed (one untaken branch).\n\n"
            % (", ".join("%.2f" % x for x in c["without_s"]), ", ".join("%.2f" % x for x in c["with_s"]), c["sam_bytes"]))
    if ab:
        f.write("`bench.py --gpus 1 --steps 20 --warmup 5`, ms per step, alternating runs in one session on one machine (the library of the commit before "
                "against this one's; the entry is never called there): before %s; this commit %s.\n\n"
                % (", ".join("%.4f" % x for x in ab[0::2]), ", ".join("%.4f" % x for x in ab[1::2])))
    else:
        f.write("`bench.py` against the commit before: not measured in this run (BENCH_AB not given).\n\n")
    if os.environ.get("KERNEL_RESOURCES"):
        f.write("Compiler's resource report of the new kernels (`-Rpass-analysis=kernel-resource-usage`, gfx950):\n\n%s\n\n" % os.environ["KERNEL_RESOURCES"])
    f.write("`--write-sam --md` (MD:Z in every record): the field is formatted on the host, by `samout.md_text` inside `samout.write_sam`, one walk of the record's CIGAR next to the one `gap_figures` makes; the device export and fetch above are the same calls with and without it.  Wall time of `cli type --write-sam` with and without `--md`: not measured.  The device-formatted field of `--write-sam-all`: profiles/sam_all.md.\n\n")
    f.write("```\n%s\n```\n" % json.dumps(out))
