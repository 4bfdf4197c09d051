#!/usr/bin/env python3
"""Rate of the reads export behind `cli type --write-reads` (mlst_reads_text_open / _next / _close, csrc/reads_text.h) next to the full
alignment export (mlst_alignments_text_*, csrc/aln_text.h) on the same engine and sample: the 2 M-read isolate of
profiles/sam_all_rate.py on DB-ecoli (7 loci x 1,430 alleles; one genome of 4.6 Mb, single-end reads of 150 bases), and MANY_READS
[2000] reads drawn from the loci themselves (every read aligns: the text is no longer small beside the tables).
Each export is timed by a host clock around calls that end in a device synchronise, median of RUNS [5] after one warm-up:
  * open          -- the item list to the host, the sort, the round plan (at_plan, shared by both), the uploads;
  * open + first  -- open, then _next(NULL, 0): the first round decided (k_at_decide, k_at_dp), then k_at_reads and the scan over the
                     pairs (full export) or k_rt_mark and the scan over the reads (reads export);
  * whole         -- open + every round with its formatting and its copy into page-locked host memory + close;
  * copy          -- hipMemcpy of the same number of bytes from device memory into the same page-locked buffer, alone.
Engine.kernel_time covers the kernels of pass 1 only, so the export's stages are told apart by these host clocks.
`BENCH_AB='<before> <this> ...'` (ms per step of bench.py --gpus 1 --steps 20 --warmup 5, alternating processes, a build of the commit
before against this one's) and `SAM_ALL_AB='<before> <this> ...'` (whole export of the isolate by profiles/sam_all_rate.py, ms, likewise)
are copied into the report when set: neither ever calls the reads export.  `FROM_JSON=<file>` renders the report again from a saved
JSON line of this script without measuring (the A/B figures of a later run are added that way); `AB_NOTE=<text>` adds a line to that section.
One JSON line, and profiles/reads_text.md next to this script."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = int(os.environ.get("RUNS", "5"))
MANY_READS = int(os.environ.get("MANY_READS", "2000"))
ISOLATE_READS = int(os.environ.get("ISOLATE_READS", "2000000"))
ROUND_BYTES = int(os.environ.get("ROUND_MB", "256")) << 20


def timed(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, [t * 1e3 for t in ts]


def locus_reads(idx, n_reads, rng):
    """reads of 150 bases cut from alleles of the loaded loci, Phred 40, every 50th base changed (profiles/sam_all_rate.py)"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for _ in range(n_reads):
        a = int(rng.integers(idx.n_alleles))
        s = np.frombuffer(idx.sequence(a).upper().encode(), np.uint8).copy()
        at = int(rng.integers(0, max(1, len(s) - 150)))
        r = s[at:at + 150]
        r[25::50] = acgt[(np.searchsorted(acgt, r[25::50]) + 1) % 4]
        reads.append(r.tobytes())
    return synth.ragged_reads(reads, [b"I" * len(r) for r in reads])


FROM_JSON = os.environ.get("FROM_JSON")      # render the report again from a saved JSON line (no GPU): the A/B figures may come later


def measure():
    global np, synth      # (locus_reads above uses them)
    import __graft_entry__ as ge

    ge.build()
    import numpy as np
    import torch

    from metamlst_amd import synth
    from metamlst_amd.engine import Engine, _ptr, pinned_array
    from metamlst_amd.index import load_index

    out = {"runs": RUNS, "round_bytes": ROUND_BYTES, "samples": []}
    hip = C.CDLL("libamdhip64.so")
    with tempfile.TemporaryDirectory() as tmp:
        db = synth.make_ecoli_db(tmp + "/ecoli.db", alleles_per_locus=1430, n_profiles=5000)
        idx = load_index(tmp + "/ecoli.db")
        genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][3])
        eng = Engine(0)
        eng.load_reference(idx)
        labels = [idx.label(a).encode() for a in range(idx.n_alleles)]
        noff = np.zeros(len(labels) + 1, np.uint64); noff[1:] = np.cumsum([len(x) for x in labels])
        names = np.frombuffer(b"".join(labels), np.uint8)
        nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()
        opens = {"sam": lambda: eng._check(eng.lib.mlst_alignments_text_open(eng._h, _ptr(names), _ptr(noff), 0, ROUND_BYTES), "open"),
                 "reads": lambda: eng._check(eng.lib.mlst_reads_text_open(eng._h, 0, ROUND_BYTES), "open")}
        nexts = {"sam": eng.lib.mlst_alignments_text_next, "reads": eng.lib.mlst_reads_text_next}
        closes = {"sam": eng.lib.mlst_alignments_text_close, "reads": eng.lib.mlst_reads_text_close}
        rng = np.random.default_rng(11)
        for name, make in (("isolate, %d reads" % ISOLATE_READS, lambda: synth.flatten_reads(*synth.sample_reads(genome, ISOLATE_READS))),
                           ("many items, %d on-locus reads" % MANY_READS, lambda: locus_reads(idx, MANY_READS, rng))):
            fb, fq, off = make()
            eng.reset_sample()
            eng.submit_reads(fb, fq, off)
            st = eng.stats()
            items = eng.items(1 << 20)
            s = {"name": name, "reads": len(off) - 1, "items": len(items), "reads_with_items": len(set(int(x[0]) for x in items.tolist()))}
            chunks = {"sam": list(eng.export_sam_text(idx, round_bytes=ROUND_BYTES)), "reads": list(eng.export_reads_text(round_bytes=ROUND_BYTES))}
            assert sum(c.count(b"\n") for c in chunks["sam"]) == int(st.counters[0]), "the full export does not hold the records pass 1 counted"
            qnames = set()
            for c in chunks["sam"]:
                qnames.update(l.split(b"\t", 1)[0] for l in c.splitlines())
            got = [l[1:] for c in chunks["reads"] for l in c.split(b"\n")[0::4] if l]
            assert got == sorted(qnames, key=lambda q: int(q[1:])), "the reads export does not hold the QNAMEs of the full export"
            biggest = max([len(c) for cs in chunks.values() for c in cs] + [1])
            buf = pinned_array(biggest)
            dev = torch.empty(biggest, dtype=torch.uint8, device="cuda")
            for kind in ("sam", "reads"):
                cs = chunks[kind]

                def whole():
                    opens[kind]()
                    while True:
                        eng._check(nexts[kind](eng._h, _ptr(buf), len(buf), C.byref(nb), C.byref(nr), C.byref(done)), "next")
                        if done.value:
                            break
                    eng._check(closes[kind](eng._h), "close")

                def first():      # (open is inside: subtract it)
                    opens[kind]()
                    eng._check(nexts[kind](eng._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done)), "next")
                    eng._check(closes[kind](eng._h), "close")

                def copy():
                    for c in cs:
                        assert hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(dev.data_ptr()), C.c_size_t(len(c)), 2) == 0      # hipMemcpyDeviceToHost

                t_o, t_f, t_w, t_c = timed(lambda: (opens[kind](), eng._check(closes[kind](eng._h), "close"))), timed(first), timed(whole), timed(copy)
                s[kind] = {"bytes": sum(len(c) for c in cs), "rounds": len(cs), "records": sum(c.count(b"\n") for c in cs) // (4 if kind == "reads" else 1),
                           "open_ms": t_o[0], "open_runs_ms": t_o[1], "open_first_round_ms": t_f[0], "open_first_round_runs_ms": t_f[1],
                           "whole_ms": t_w[0], "whole_runs_ms": t_w[1], "copy_ms": t_c[0], "copy_runs_ms": t_c[1]}
            out["samples"].append(s)
        eng.close()
    return out


out = json.loads(open(FROM_JSON).read().strip().splitlines()[-1]) if FROM_JSON else measure()
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
sab = [float(x) for x in os.environ.get("SAM_ALL_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
out["sam_all_isolate_whole_ms"] = {"before": sab[0::2], "this": sab[1::2]}
print(json.dumps(out))


def ab_line(what, unit, b, t):
    return ("%s, %s, alternating processes, before / this / before / this on one machine (a build of the commit before against this one's): before %s; this commit %s.  "
            "Difference of the means %+.4f %s; spread of the runs of the commit before itself %.4f %s.\n"
            % (what, unit, ", ".join("%.4f" % x for x in b), ", ".join("%.4f" % x for x in t), statistics.mean(t) - statistics.mean(b), unit.split(" ")[0], max(b) - min(b), unit.split(" ")[0]))


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "reads_text.md"), "w") as f:
    f.write("# The reads export (`cli type --write-reads`, `mlst_reads_text_*`, `csrc/reads_text.h`): its rate next to the full export's\n\n"
            "`python profiles/reads_text_rate.py` on one MI355X.  Host clock around calls that end in a device synchronise; median of %d calls after one warm-up call (every "
            "run is in the JSON below).  Database: 7 loci x 1,430 alleles.  Both exports run on the same engine over the same sample, round budget %d MiB; before anything was "
            "timed the full export's record count was compared with pass 1's MLST_CNT_TOTAL_RECORDS and the names of the reads export with the set of QNAMEs of the full "
            "export.  whole = open + every round into page-locked memory + close.\n\n" % (RUNS, ROUND_BYTES >> 20))
    f.write("| sample | work items | reads with an item | export | records / reads written | text bytes | rounds | open ms | open + first round decided ms | whole ms | copy alone ms |\n"
            "|---|---|---|---|---|---|---|---|---|---|---|\n")
    for s in out["samples"]:
        for kind, label in (("sam", "full (`--write-sam-all`)"), ("reads", "reads (`--write-reads`)")):
            k = s[kind]
            f.write("| %s | %d | %d | %s | %d | %d | %d | %.3f | %.3f | %.3f | %.3f |\n" % (
                s["name"], s["items"], s["reads_with_items"], label, k["records"], k["bytes"], k["rounds"], k["open_ms"], k["open_first_round_ms"], k["whole_ms"], k["copy_ms"]))
    f.write("\nThe expectation was that the reads export is no slower than the full export without `--md`: it runs the same decide kernels and writes far fewer bytes.\n\n")
    for s in out["samples"]:
        a, r = s["sam"], s["reads"]
        f.write("* %s: reads export %.3f ms against %.3f ms (%.2f x), %d bytes against %d.  Of the reads export's time %.3f ms is the open (the host's sort and plan, shared "
                "with the full export: %.3f ms there) and %.3f ms the first round up to its size (decide, banded list, `k_rt_mark`, scan); the full export spends %.3f ms "
                "from open to the first round's size and the rest on %d rounds of formatting and copying.\n"
                % (s["name"], r["whole_ms"], a["whole_ms"], a["whole_ms"] / r["whole_ms"] if r["whole_ms"] > 0 else float("nan"), r["bytes"], a["bytes"], r["open_ms"],
                   a["open_ms"], r["open_first_round_ms"] - r["open_ms"], a["open_first_round_ms"], a["rounds"]))
    f.write("\n`Engine.kernel_time` times the kernels of pass 1 only; the stages above are host clocks around synchronising calls.\n")
    f.write("\n## With the flag absent: against the commit before\n\n")
    if ab:
        f.write("* " + ab_line("`bench.py --gpus 1 --steps 20 --warmup 5`", "ms per step", ab[0::2], ab[1::2]))
    else:
        f.write("* `bench.py` against the commit before: not measured in this run (BENCH_AB not given).\n")
    if sab:
        f.write("* " + ab_line("`profiles/sam_all_rate.py`, whole export of the 2 M-read isolate", "ms (median of its runs)", sab[0::2], sab[1::2]))
    else:
        f.write("* `profiles/sam_all_rate.py` against the commit before: not measured in this run (SAM_ALL_AB not given).\n")
    if os.environ.get("AB_NOTE"):      # what else was measured against the commit before, in the measurer's words
        f.write("* %s\n" % os.environ["AB_NOTE"])
    if os.environ.get("KERNEL_RESOURCES"):
        f.write("\nCompiler's resource report of the new kernels (`-Rpass-analysis=kernel-resource-usage`, gfx950; no kernel uses scratch, and the report of every kernel of "
                "the commit before is unchanged):\n\n%s\n" % os.environ["KERNEL_RESOURCES"])
    f.write("\n```\n%s\n```\n" % json.dumps(out))
