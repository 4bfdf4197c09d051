#!/usr/bin/env python3
"""What adapter removal (`mlst_set_read_adapters`, csrc/read_adapt.h; `cli type --adapter`) costs, on the two end-to-end legs of
`bench.py --full` -- FASTQ text -> ST and bgzip -> ST on E2E_READS [48,000,000] reads of its cfg3 workload (150 bases each), the same
1 Mi-record chunks and BGZF pieces, page-locked -- in the manner of profiles/read_prep_rate.py:
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs RUNS [5]
    times after a warm-up with the library MLST_LIB names (a build of the commit before: its csrc/ and include/ compiled with build()'s
    flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...}; AB_LOG names the file that gathers those lines
    for the report.  The yardstick is the spread of the parent's own runs.
  * switch on, with 1 adapter (illumina) and with 4 (illumina, nextera, smallrna and the 33-letter TruSeq read 1 adapter), min_overlap
    3 and 10 % errors: this commit runs RUNS times on either leg; then one text run under mlst_set_profiling gives k_ra_cut's time alone
    (mlst_get_kernel_time 19) next to the parse + pack slot (6).  The reads carry no planted adapter: the kernel looks at every start
    of every read whatever it finds, and about 2 % of them lose their last bases by chance.
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' (pairs of alternating `bench.py --gpus 1 --steps 20
--warmup 5` processes, MLST_LIB naming the library) is copied into the report.  One JSON line, and profiles/read_adapters.md next to
this script."""
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metamlst_amd import synth  # noqa: E402
from metamlst_amd.engine import Engine, pinned_array  # noqa: E402
from metamlst_amd.fastq import ADAPTER_NAMES  # noqa: E402

E2E_READS = int(os.environ.get("E2E_READS", "48000000"))
RUNS = int(os.environ.get("RUNS", "5"))
MODE = os.environ.get("MODE", "all")
LABEL = os.environ.get("LABEL", "this")
AB_LOG = os.environ.get("AB_LOG", "")
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
ON = {"1": [ADAPTER_NAMES["illumina"]],
      "4": [ADAPTER_NAMES["illumina"], ADAPTER_NAMES["nextera"], ADAPTER_NAMES["smallrna"], "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"]}
out = {"runs": RUNS, "adapters_on": ON, "min_overlap": 3, "error_permille": 100}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_pieces(text: np.ndarray, n: int) -> tuple[list, int]:
    view = memoryview(text)
    with ThreadPoolExecutor(THREADS) as ex:      # zlib releases the GIL
        parts = list(ex.map(lambda at: bgzf_block(bytes(view[at:at + 65280])), range(0, len(text), 65280)))
    per_piece = 65536 if n >= 40_000_000 else 16384
    pieces = []
    for a in range(0, len(parts), per_piece):
        blob = b"".join(parts[a:a + per_piece]) + (bgzf_block(b"") if a + per_piece >= len(parts) else b"")
        pb = pinned_array(len(blob))
        pb[:] = np.frombuffer(blob, np.uint8)
        pieces.append(pb)
    return pieces, len(parts)


import bench  # noqa: E402

argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--pipeline", "1"] + (["--reads", str(E2E_READS)] if E2E_READS < 48_000_000 else [])
args = bench.parse_args()
sys.argv = argv
device = torch.device("cuda", 0)
torch.cuda.set_device(0)
tmp = tempfile.mkdtemp(prefix="mlst_adapt_")
w = bench.build_workload("cfg3", args, lambda: Engine(0), torch, device, 0, 1, tmp)
this = w.engines[0]
packed, qrows, lens, n_total = w.batches[0]
n, L = min(E2E_READS, n_total), args.read_len
rec = 16 + 2 * L
text = pinned_array(n * rec)
for at in range(0, n, 1 << 20):
    c = min(1 << 20, n - at)
    text[at * rec:(at + c) * rec] = synth.resident_to_fastq_text(torch, packed, qrows, n_total, w.wpr, w.qstride, at, c, L).cpu().numpy()
say("text made:", n, "reads,", text.size, "bytes")
CHUNK = 1 << 20      # records per submission of the text leg (bench.py's)


def run_text(eng):
    t0 = time.perf_counter()
    for at in range(0, n, CHUNK):
        eng.submit_fastq(text[at * rec:min(n, at + CHUNK) * rec])
    eng.typing_enqueue(penalty=100)
    st, chosen, _ = eng.typing_fetch()
    return time.perf_counter() - t0, (st.sum_score.tobytes(), st.n_hits.tobytes(), tuple(sorted(chosen.items())))


def run_bgzip(eng, pieces):
    t0 = time.perf_counter()
    got = sum(eng.submit_fastq_bgzf(pc, final=(k == len(pieces) - 1)) for k, pc in enumerate(pieces))
    eng.typing_enqueue(penalty=100)
    st, chosen, _ = eng.typing_fetch()
    t = time.perf_counter() - t0
    assert got == n
    return t, (st.sum_score.tobytes(), st.n_hits.tobytes(), tuple(sorted(chosen.items())))


def timed(eng, fn, runs: int) -> list:
    """runs of fn after one warm-up; every run must leave the same statistics"""
    ts, ref = [], None
    for r in range(runs + 1):
        eng.reset_sample()
        eng.synchronize()
        t, key = fn(eng)
        ref = key if ref is None else ref
        assert key == ref, "the statistics differ between the runs"
        if r:
            ts.append(t)
    return ts


res = {"reads": n, "read_len": L, "text_bytes": int(text.size)}
res["text_off_s"] = timed(this, run_text, RUNS)
say("text, switch off:", res["text_off_s"])
pieces, n_blocks = bgzf_pieces(text, n)
res["bgzf_blocks"], res["pieces"], res["compressed_bytes"] = n_blocks, len(pieces), sum(int(p.size) for p in pieces)
res["bgzip_off_s"] = timed(this, lambda e: run_bgzip(e, pieces), RUNS)
say("bgzip, switch off:", res["bgzip_off_s"])
if MODE == "off":
    print(json.dumps({"label": LABEL, "reads": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}))
    sys.exit(0)
assert this.get_read_adapters()["adapters"] == [] and this.read_adapters_info()["trimmed"] == 0
res["on"] = {}
for name, adapters in ON.items():
    r = res["on"][name] = {}
    this.reset_sample()
    this.set_read_adapters(adapters)
    r["text_s"] = timed(this, run_text, RUNS)
    r["info"] = this.read_adapters_info()
    say("text, %s adapter(s):" % name, r["text_s"], r["info"])
    r["bgzip_s"] = timed(this, lambda e: run_bgzip(e, pieces), RUNS)
    say("bgzip, %s adapter(s):" % name, r["bgzip_s"])
    assert this.read_adapters_info() == r["info"] and 0 < r["info"]["trimmed"] < n // 4
    # k_ra_cut alone: one text run with an event pair around every kernel group (the runs above were made without)
    this.reset_sample()
    this.set_profiling(1)
    this.reset_kernel_time()
    run_text(this)
    r["k_ra_cut_ms"], r["k_ra_cut_launches"] = this.kernel_time(19)
    r["parse_pack_ms"] = this.kernel_time(6)[0]
    this.set_profiling(0)
this.reset_sample()
this.set_read_adapters()
out["e2e"] = res
procs = [json.loads(l) for l in open(AB_LOG) if l.startswith("{")] if AB_LOG and os.path.exists(AB_LOG) else []
procs = [p for p in procs if p.get("reads") == n] + [{"label": "this", "reads": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}]
out["off_processes"] = procs
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))


def rate(ts):
    return n / min(ts) / 1e6


def spread(ts):
    return (max(ts) / min(ts) - 1) * 100


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_adapters.md"), "w") as f:
    f.write("# Adapter removal (`mlst_set_read_adapters`, `csrc/read_adapt.h`; `cli type --adapter`): what it costs\n\n"
            "`python profiles/read_adapters_rate.py` on one MI355X; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
            "%d reads of %d bases of `bench.py`'s cfg3 workload, %d bytes of FASTQ text in chunks of 1 Mi records, %d BGZF blocks (level 6) in %d pieces, all page-locked; a run = "
            "every submission + `typing_enqueue` + `typing_fetch`.\n\n" % (n, L, res["text_bytes"], res["bgzf_blocks"], res["pieces"]))
    f.write("## Switch off: against the commit before\n\n")
    if any(p["label"] == "parent" for p in procs):
        f.write("Alternating processes on one machine, one build each (the commit before compiled from its own sources with the same flags), every process makes the same "
                "bytes and runs either leg %d times after a warm-up.\n\n| leg | process | seconds per run | best, Mreads/s |\n|---|---|---|---|\n" % RUNS)
        for leg, key in (("FASTQ text -> ST", "text_off_s"), ("bgzip -> ST", "bgzip_off_s")):
            for k, p in enumerate(procs):
                f.write("| %s | %d: %s | %s | %.1f |\n" % (leg, k + 1, p["label"], ", ".join("%.4f" % x for x in p[key]), rate(p[key])))
        for leg, key in (("FASTQ text -> ST", "text_off_s"), ("bgzip -> ST", "bgzip_off_s")):
            pa = [x for p in procs if p["label"] == "parent" for x in p[key]]
            th = [x for p in procs if p["label"] == "this" for x in p[key]]
            f.write("\n%s: median of this commit's runs against the median of the parent's %+.2f %% (best against best %+.2f %%); the parent's own runs lie between %.4f and "
                    "%.4f s, %.2f %% of their best.  %s\n"
                    % (leg, (statistics.median(th) / statistics.median(pa) - 1) * 100, (min(th) / min(pa) - 1) * 100, min(pa), max(pa), spread(pa),
                       "This commit's median lies inside the parent's spread." if statistics.median(th) <= max(pa) else "This commit's median lies OUTSIDE the parent's spread."))
    else:
        f.write("Not measured in this run (no AB_LOG with runs of the parent).\n")
    b, t = ab[0::2], ab[1::2]
    if len(b) >= 2 and len(t) >= 1:
        f.write("\nHeadline step, `bench.py --gpus 1 --steps 20 --warmup 5`, ms per step, alternating processes before / this on one machine: before %s; this commit %s.  "
                "Difference of the medians %+.4f ms (of the means %+.4f ms); spread of the runs of the commit before itself %.4f ms.\n"
                % (", ".join("%.4f" % x for x in b), ", ".join("%.4f" % x for x in t), statistics.median(t) - statistics.median(b), statistics.mean(t) - statistics.mean(b),
                   max(b) - min(b)))
    else:
        f.write("\nHeadline step: not measured in this run.\n")
    f.write("\n## Switch on: `--adapter`, min_overlap 3, 10 %% errors\n\nThe same text (no adapter planted: what is cut is cut by chance), this commit, %d runs after a warm-up -- behind "
            "the switch-off runs, not alternating with them.  Reported, not gated.\n\n| leg | switch | seconds per run | best, Mreads/s |\n|---|---|---|---|\n" % RUNS)
    for leg, k_off, k_on in (("FASTQ text -> ST", "text_off_s", "text_s"), ("bgzip -> ST", "bgzip_off_s", "bgzip_s")):
        for p in procs:
            if p["label"] == "parent":
                f.write("| %s | off, parent | %s | %.1f |\n" % (leg, ", ".join("%.4f" % x for x in p[k_off]), rate(p[k_off])))
        f.write("| %s | off, this | %s | %.1f |\n" % (leg, ", ".join("%.4f" % x for x in res[k_off]), rate(res[k_off])))
        for name in ON:
            f.write("| %s | %s adapter(s), this | %s | %.1f |\n" % (leg, name, ", ".join("%.4f" % x for x in res["on"][name][k_on]), rate(res["on"][name][k_on])))
    f.write("\n")
    for name, adapters in ON.items():
        r = res["on"][name]
        f.write("%s adapter(s) (%s): %d reads cut, %d bases removed, %d left without a base.  `k_ra_cut` alone (one text run under `mlst_set_profiling`, event pairs around the "
                "kernel): %.3f ms in %d launches = %.1f us per chunk of 1 Mi reads of %d bases, %.2f %% of the best text run and %.2f %% of the best bgzip run; the parse + pack "
                "group of the same run (slot 6): %.3f ms.\n\n"
                % (name, ", ".join(adapters), r["info"]["trimmed"], r["info"]["bases_removed"], r["info"]["emptied"], r["k_ra_cut_ms"], r["k_ra_cut_launches"],
                   1e3 * r["k_ra_cut_ms"] / max(1, r["k_ra_cut_launches"]), L, r["k_ra_cut_ms"] / 10 / min(r["text_s"]), r["k_ra_cut_ms"] / 10 / min(r["bgzip_s"]), r["parse_pack_ms"]))
    one, four = (1e3 * res["on"][k]["k_ra_cut_ms"] / max(1, res["on"][k]["k_ra_cut_launches"]) for k in ("1", "4"))
    f.write("Against `k_rp_qtrim` (218 us per 1 Mi reads, profiles/read_prep.md): %.1f times its time with one adapter, %.1f times with four.  (What the kernel's assembly "
            "says about these figures is read by hand and kept in DESIGN.md 4.3, with the commit it was read from.)\n" % (one / 218.0, four / 218.0))
    f.write("\n```\n%s\n```\n" % json.dumps(out))
