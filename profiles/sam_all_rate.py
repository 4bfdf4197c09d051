#!/usr/bin/env python3
"""Rate of the full alignment export behind `cli type --write-sam-all` (mlst_alignments_text_open / _next / _close, csrc/aln_text.h).
Samples on DB-ecoli (7 loci x 1,430 alleles, cfg2's database of SURVEY.md 8(d)):
  * an isolate: one genome of 4.6 Mb, 2 M single-end reads of 150 bases -- a few thousand work items;
  * many items: MANY_READS [2000] reads of 150 bases drawn from the seven loci themselves (every read is an item or two, each
    against 1,430 alleles: ~1,400 records per read), the shape of a metagenome's on-locus reads;
  * small: SMALL_READS [100] such reads, also written by the plain-Python rule (samout.all_records_rule over the parsed records), for scale.
Each is submitted, then timed by a host clock around calls that end in a device synchronise, median of RUNS [5] after one warm-up:
  * open          -- mlst_alignments_text_open: the item list to the host, the sort, the round plan, the uploads;
  * open + decide -- open, then mlst_alignments_text_next(NULL, 0): the first round's alignment, per-read figures, lengths and scan;
  * whole         -- open + every round with its formatting and its copy into page-locked host memory + close (ROUND_MB [256]);
  * copy          -- hipMemcpy of the same number of bytes from device memory into the same page-locked buffer, alone.
"export alone" is whole - copy (derived; the copy is not overlapped with the kernels).  With `--md` every sample is exported again with
mlst_set_export_md on (MD:Z in every record): open + decide and whole with the switch on, then whole with it off once more (the
off leg's own spread), reported beside the bytes the field adds.  `BENCH_AB='<ms per step of the commit
before> <ms per step of this one> ...'` (pairs, alternating runs of bench.py --gpus 1 --steps 20 --warmup 5 on one machine in one
session) and `KERNEL_RESOURCES=<text>` are copied into the report when set: bench.py never calls the export.
One JSON line, and profiles/sam_all.md next to this script."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metamlst_amd import samin, samout, synth  # noqa: E402
from metamlst_amd.engine import Engine, _ptr, pinned_array  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

RUNS = int(os.environ.get("RUNS", "5"))
MANY_READS = int(os.environ.get("MANY_READS", "2000"))
SMALL_READS = int(os.environ.get("SMALL_READS", "100"))
ROUND_BYTES = int(os.environ.get("ROUND_MB", "256")) << 20
MD = "--md" in sys.argv[1:]


def timed(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, [t * 1e3 for t in ts]


def locus_reads(idx, n_reads, rng):
    """reads of 150 bases cut from alleles of the loaded loci, Phred 40, every 50th base changed"""
    reads = []
    for k in range(n_reads):
        a = int(rng.integers(idx.n_alleles))
        s = np.frombuffer(idx.sequence(a).upper().encode(), np.uint8).copy()
        at = int(rng.integers(0, max(1, len(s) - 150)))
        r = s[at:at + 150]
        r[25::50] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), r[25::50]) + 1) % 4]
        reads.append(r.tobytes())
    return synth.ragged_reads(reads, [b"I" * len(r) for r in reads])


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
    rng = np.random.default_rng(11)
    nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()

    def t_open():
        eng._check(eng.lib.mlst_alignments_text_open(eng._h, _ptr(names), _ptr(noff), 0, ROUND_BYTES), "open")

    def t_close():
        eng._check(eng.lib.mlst_alignments_text_close(eng._h), "close")

    for name, make in (("isolate, 2 M reads", lambda: synth.flatten_reads(*synth.sample_reads(genome, 2_000_000))),
                       ("many items, %d on-locus reads" % MANY_READS, lambda: locus_reads(idx, MANY_READS, rng)),
                       ("small, %d on-locus reads" % SMALL_READS, lambda: locus_reads(idx, SMALL_READS, rng))):
        fb, fq, off = make()
        eng.reset_sample()
        eng.submit_reads(fb, fq, off)
        st = eng.stats()
        n_items = len(eng.items(1 << 20))
        chunks = list(eng.export_sam_text(idx, round_bytes=ROUND_BYTES))
        n_bytes, n_recs, biggest = sum(len(c) for c in chunks), sum(c.count(b"\n") for c in chunks), max([len(c) for c in chunks] + [1])
        assert n_recs == int(st.counters[0]), "the export does not hold the records pass 1 counted"
        if MD:      # the same export with MD:Z: its bytes size the buffers too
            chunks_md = list(eng.export_sam_text(idx, round_bytes=ROUND_BYTES, md=True))
            assert sum(c.count(b"\n") for c in chunks_md) == n_recs and all(b"\tMD:Z:" in c for c in chunks_md)
            biggest = max([len(c) for c in chunks_md] + [biggest])
        buf = pinned_array(biggest)
        dev = torch.empty(biggest, dtype=torch.uint8, device="cuda")

        def whole():
            t_open()
            while True:
                eng._check(eng.lib.mlst_alignments_text_next(eng._h, _ptr(buf), len(buf), C.byref(nb), C.byref(nr), C.byref(done)), "next")
                if done.value:
                    break
            t_close()

        def decide():      # (open is inside: subtract it)
            t_open()
            eng._check(eng.lib.mlst_alignments_text_next(eng._h, None, 0, C.byref(nb), C.byref(nr), C.byref(done)), "next")
            t_close()

        def copy():
            for c in chunks:
                assert hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(dev.data_ptr()), C.c_size_t(len(c)), 2) == 0      # hipMemcpyDeviceToHost

        t_o = timed(lambda: (t_open(), t_close()))
        t_d = timed(decide)
        t_w = timed(whole)
        t_c = timed(copy)
        s = {"name": name, "reads": len(off) - 1, "items": n_items, "records": n_recs, "bytes": n_bytes, "rounds": len(chunks),
             "open_ms": t_o[0], "open_runs_ms": t_o[1], "open_decide_first_round_ms": t_d[0], "open_decide_first_round_runs_ms": t_d[1],
             "whole_ms": t_w[0], "whole_runs_ms": t_w[1], "copy_ms": t_c[0], "copy_runs_ms": t_c[1]}
        if MD:
            eng.set_export_md(True)
            t_dm, t_wm = timed(decide), timed(whole)
            eng.set_export_md(False)
            t_w2 = timed(whole)
            s["md"] = {"bytes": sum(len(c) for c in chunks_md), "rounds": len(chunks_md), "open_decide_first_round_ms": t_dm[0], "open_decide_first_round_runs_ms": t_dm[1],
                       "whole_ms": t_wm[0], "whole_runs_ms": t_wm[1], "whole_off_again_ms": t_w2[0], "whole_off_again_runs_ms": t_w2[1]}
        if name.startswith("small"):      # the same records through the plain-Python rule
            path = tmp + "/small.all.sam"
            with open(path, "wb") as f:
                f.write(samout.sam_all_header(idx).encode() + b"".join(chunks))
            label2a = {idx.label(a): a for a in range(idx.n_alleles)}
            tuples = []
            for al in samin.read_alignments(path):
                tags = {t[:2]: t[5:] for t in al.tags}
                a = label2a[al.rname]
                tuples.append((int(al.qname[1:]), (al.flag >> 4) & 1, 0, int(idx.locus_id[a]), a, al.pos - 1, int(tags["AS"]), int(tags["XM"]), samin.parse_cigar(al.cigar),
                               al.seq.encode(), bytes(c - 33 for c in al.qual.encode())))
            t0 = time.perf_counter()
            lines = samout.all_records_rule(idx, tuples, False)
            s["python_rule_ms"] = (time.perf_counter() - t0) * 1e3
            s["python_rule_same_bytes"] = b"".join(lines) == b"".join(chunks)
        out["samples"].append(s)
    eng.close()
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))


def rate(n, ms):
    return n / (ms * 1e-3) if ms > 0 else float("nan")


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "sam_all.md"), "w") as f:
    f.write("# The full alignment export (`cli type --write-sam-all`): its rate\n\n`python profiles/sam_all_rate.py` on one MI355X.  Host clock around calls that end "
            "in a device synchronise; median of %d calls after one warm-up call (every run is in the JSON below).  Database: 7 loci x 1,430 alleles.  Before anything "
            "was timed the export's record count was compared with pass 1's MLST_CNT_TOTAL_RECORDS.\n\n" % RUNS)
    f.write("The item list is sorted on the HOST inside `mlst_alignments_text_open` (a `std::sort` of a permutation over the downloaded item list, per item, never per "
            "record), not with the device radix sort of the BAM stream: the key (64-bit read index, locus, strand, diagonal) does not fit one 64-bit radix key, and the "
            "same per-item host pass plans the rounds.  Its cost is the `open` column.\n\n")
    f.write("| sample | work items | records | text bytes | rounds | open ms | open + first round decided ms | whole export ms | copy alone ms | records/s, GB/s with the copy-out | "
            "records/s, GB/s of the export alone (whole - copy) |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
    for s in out["samples"]:
        alone = s["whole_ms"] - s["copy_ms"]
        f.write("| %s | %d | %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3g, %.3f | %.3g, %.3f |\n" % (
            s["name"], s["items"], s["records"], s["bytes"], s["rounds"], s["open_ms"], s["open_decide_first_round_ms"], s["whole_ms"], s["copy_ms"],
            rate(s["records"], s["whole_ms"]), rate(s["bytes"], s["whole_ms"]) / 1e9, rate(s["records"], alone), rate(s["bytes"], alone) / 1e9))
    small = [s for s in out["samples"] if "python_rule_ms" in s]
    if small:
        s = small[0]
        f.write("\nThe plain-Python rule (`samout.all_records_rule`, the specification) over the %d records of the small sample: %.1f ms, %.3g records/s (the same bytes: %s); "
                "the device export of that sample: %.3f ms whole.\n" % (s["records"], s["python_rule_ms"], rate(s["records"], s["python_rule_ms"]), s["python_rule_same_bytes"], s["whole_ms"]))
    if MD:
        f.write("\n## With `--md` (`mlst_set_export_md`): MD:Z in every record\n\nThe same samples exported again with the switch on, then with it off once more; "
                "whole export = open + every round into page-locked memory + close, median of %d.\n\n" % RUNS)
        f.write("| sample | records | text bytes off | text bytes on | open + first round decided ms off / on | whole ms off | whole ms on | whole ms off again | time on against off | bytes on against off |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for s in out["samples"]:
            m = s["md"]
            f.write("| %s | %d | %d | %d | %.3f / %.3f | %.3f | %.3f | %.3f | %+.2f %% | %+.2f %% |\n" % (
                s["name"], s["records"], s["bytes"], m["bytes"], s["open_decide_first_round_ms"], m["open_decide_first_round_ms"], s["whole_ms"], m["whole_ms"], m["whole_off_again_ms"],
                100.0 * (m["whole_ms"] / s["whole_ms"] - 1.0), 100.0 * (m["bytes"] / s["bytes"] - 1.0)))
    else:
        f.write("\nThe `--md` leg (MD:Z in every record, switch off against on): not measured in this run (`--md` not given).\n")
    if os.environ.get("MD_OFF_AB"):      # whole export of the isolate with the switch off: a build of the commit before against this one's
        f.write("\n%s\n" % os.environ["MD_OFF_AB"])
    if ab:
        b, t = ab[0::2], ab[1::2]
        f.write("\n`bench.py --gpus 1 --steps 20 --warmup 5`, ms per step, alternating runs in one session on one machine (a build of the commit before against this one's; "
                "the entry is never called there): before %s; this commit %s.  Difference of the means %.4f ms; spread between the alternating runs: before %.4f ms, this commit %.4f ms.\n"
                % (", ".join("%.4f" % x for x in b), ", ".join("%.4f" % x for x in t), statistics.mean(t) - statistics.mean(b), max(b) - min(b), max(t) - min(t)))
    else:
        f.write("\n`bench.py` against the commit before: not measured in this run (BENCH_AB not given).\n")
    if os.environ.get("KERNEL_RESOURCES"):
        f.write("\nCompiler's resource report of the new kernels (`-Rpass-analysis=kernel-resource-usage`, gfx950; no kernel uses scratch):\n\n%s\n" % os.environ["KERNEL_RESOURCES"])
    f.write("\n```\n%s\n```\n" % json.dumps(out))
