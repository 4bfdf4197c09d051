#!/usr/bin/env python3
"""What the sliding-window quality cuts (`mlst_set_read_window`, csrc/read_window.h; `cli type --cut-front / --cut-right / --cut-tail`) cost, on
the two end-to-end legs of `bench.py --full` -- FASTQ text -> ST and bgzip -> ST on E2E_READS [48,000,000] reads of its cfg3 workload (150
bases each), the same 1 Mi-record chunks and BGZF pieces, page-locked -- in the manner of profiles/read_filter_rate.py:
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs RUNS [5]
    times after a warm-up with the library MLST_LIB names (a build of the commit before: its csrc/ and include/ compiled with build()'s
    flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...}; AB_LOG names the file that gathers those lines
    for the report.  The yardstick is the spread of the parent's own runs.
  * switch on, with `right 4,20` alone and with all three operations (front 1,3, right 4,15, tail 1,3: the Trimmomatic recipe), on the
    text as it is (no dip planted) and on a copy in which 30 % of the reads hold eight bases of Phred 2 in their middle: this commit runs
    RUNS times on the text leg; then one text run under mlst_set_profiling gives k_rw_cut's time alone (mlst_get_kernel_time 24), and one
    run with --trim-qual 20, all three windows and the read filters gives k_rp_qtrim (18), k_rw_cut (24) and k_rf_filter (23) side by side.
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' (pairs of alternating `bench.py --gpus 1 --steps 20
--warmup 5` processes, MLST_LIB naming the library) is copied into the report.  Every process of a measurement is started under a time
limit of its own (`timeout -k 10 SECONDS python profiles/read_window_rate.py`), and the next one only behind a clean exit.  One JSON line,
and profiles/read_window.md next to this script."""
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

E2E_READS = int(os.environ.get("E2E_READS", "48000000"))
RUNS = int(os.environ.get("RUNS", "5"))
MODE = os.environ.get("MODE", "all")
LABEL = os.environ.get("LABEL", "this")
AB_LOG = os.environ.get("AB_LOG", "")
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
ON = {"right": {"right": (4, 20)}, "all": {"front": (1, 3), "right": (4, 15), "tail": (1, 3)}}
FILTERS = {"poly": "G", "min_length": 30, "max_n": 5, "complexity": 30, "mean_qual": 20}
out = {"runs": RUNS, "settings_on": ON}


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
tmp = tempfile.mkdtemp(prefix="mlst_window_")
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
assert this.get_read_window() == {"front": None, "right": None, "tail": None} and this.read_window_info()["shortened"] == 0
# a copy of the text in which 30 % of the reads hold eight bases of Phred 2 in their middle (the bases stay)
text0 = text
text30 = pinned_array(n * rec)
text30[:] = text0
rows30 = text30.reshape(n, rec)
ks = np.arange(n)
for a in range(51):
    sel = ks[(ks % 10 < 3) & ((ks * 7) % 51 == a)]
    rows30[sel, 15 + L + 40 + a:15 + L + 48 + a] = ord("#")
res["on"] = {}
for share, body in (("0", text0), ("30", text30)):
    text = body
    for name, setting in ON.items():
        r = res["on"][name + "_" + share] = {"setting": name, "planted_percent": int(share)}
        this.reset_sample()
        this.set_read_window()
        if share == "30":
            r["text_off_s"] = timed(this, run_text, RUNS)
        this.reset_sample()
        this.set_read_window(**setting)
        r["text_s"] = timed(this, run_text, RUNS)
        r["info"] = this.read_window_info()
        say("text, %s, %s %% planted:" % (name, share), r["text_s"], r["info"])
        # k_rw_cut alone: one text run with an event pair around every kernel group (the runs above were made without)
        this.reset_sample()
        this.set_profiling(1)
        this.reset_kernel_time()
        run_text(this)
        r["k_rw_cut_ms"], r["k_rw_cut_launches"] = this.kernel_time(24)
        r["parse_pack_ms"] = this.kernel_time(6)[0]
        this.set_profiling(0)
    # the three per-read kernels of the chain that read the quality line side by side, on one run
    this.reset_sample()
    this.set_read_window(**ON["all"])
    this.set_read_prep(trim_qual=20)
    this.set_read_filter(**FILTERS)
    this.set_profiling(1)
    this.reset_kernel_time()
    run_text(this)
    res["side_by_side_" + share] = {name: list(this.kernel_time(slot)) for name, slot in (("k_rp_qtrim", 18), ("k_rw_cut", 24), ("k_rf_filter", 23))}
    this.set_profiling(0)
    this.reset_sample()
    this.set_read_prep()
    this.set_read_filter()
    this.set_read_window()
text = text0
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


def per_chunk(ms, launches):
    return 1e3 * ms / max(1, launches)


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_window.md"), "w") as f:
    f.write("# Sliding-window quality cuts (`mlst_set_read_window`, `csrc/read_window.h`; `cli type --cut-front / --cut-right / --cut-tail`): what they cost\n\n"
            "`python profiles/read_window_rate.py` on one MI355X; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
            "%d reads of %d bases of `bench.py`'s cfg3 workload%s, %d bytes of FASTQ text in chunks of 1 Mi records, %d BGZF blocks (level 6) in %d pieces, all page-locked; a run = "
            "every submission + `typing_enqueue` + `typing_fetch`.\n\n" % (n, L, "" if n >= 48_000_000 else " (a REDUCED run: the script's default is 48,000,000)", res["text_bytes"], res["bgzf_blocks"], res["pieces"]))
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
    f.write("\n## Switch on\n\nThis commit, %d runs after a warm-up on the text leg -- behind the switch-off runs, not alternating with them.  Reported, not gated.  right: "
            "`--cut-right 4,20`; all: `--cut-front 1,3 --cut-right 4,15 --cut-tail 1,3`.  Planted: the share of reads in which eight bases in the middle were given Phred 2.  "
            "`k_rw_cut`: one text run under `mlst_set_profiling`, event pairs around the kernel, per chunk of 1 Mi reads.\n\n"
            "| setting | planted | seconds per run | best, Mreads/s | switch off on the same text, best | reads cut | bases removed | `k_rw_cut`, us per 1 Mi reads | parse + pack (slot 6), ms |\n"
            "|---|---|---|---|---|---|---|---|---|\n" % RUNS)
    for key, r in res["on"].items():
        off = r.get("text_off_s", res["text_off_s"])
        i = r["info"]
        f.write("| %s | %d %% | %s | %.1f | %.1f | %d | %d | %.1f | %.3f |\n"
                % (r["setting"], r["planted_percent"], ", ".join("%.4f" % x for x in r["text_s"]), rate(r["text_s"]), rate(off), i["shortened"],
                   i["front_bases"] + i["right_bases"] + i["tail_bases"], per_chunk(r["k_rw_cut_ms"], r["k_rw_cut_launches"]), r["parse_pack_ms"]))
    f.write("\nThe per-read kernels of the chain that read the quality line, on one run each (`--trim-qual 20`, all three windows, `--trim-poly-g --min-length 30 --max-n 5 "
            "--low-complexity 30 --min-mean-qual 20`), us per chunk of 1 Mi reads:\n\n| planted | `k_rp_qtrim` | `k_rw_cut` | `k_rf_filter` |\n|---|---|---|---|\n")
    for share in ("0", "30"):
        s = res["side_by_side_" + share]
        f.write("| %s %% | %.1f | %.1f | %.1f |\n" % (share, per_chunk(*s["k_rp_qtrim"]), per_chunk(*s["k_rw_cut"]), per_chunk(*s["k_rf_filter"])))
    rr = res["on"]["right_0"]
    f.write("\nBytes per read: right is the one full pass and loads every quality byte twice, 16 bytes per load (the leading chunk and the one `w` bytes behind it; 26 bytes of "
            "offsets and length besides); front and tail leave inside their first loads on a good read.  At %.1f us per 1 Mi reads `right 4,20` moves %.0f GB/s of quality "
            "bytes counted once.  If that lies well above `k_rf_filter`'s pass, the lead is the 16-lanes-per-read mapping DESIGN.md names for the filter (coalesced rows "
            "instead of a 16-byte load per lane at a stride of a record); it was not built.\n"
            % (per_chunk(rr["k_rw_cut_ms"], rr["k_rw_cut_launches"]), (1 << 20) * 1.0 * L / per_chunk(rr["k_rw_cut_ms"], rr["k_rw_cut_launches"]) / 1e3))
    f.write("\nBuild (`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`), `k_rw_cut`: 58 VGPRs, 0 AGPRs, 66 SGPRs, no scratch, no spill of either kind, "
            "no LDS, 8 waves per SIMD (`k_rp_qtrim` 52 / 53, `k_rf_filter` 64 / 81).  One mapping was built (a thread per read).\n")
    f.write("\nNot measured: bgzip -> ST with the switch on, `.gz` input, other read lengths, a real library's quality profile, the sub-wave mapping.\n")
    f.write("\n```\n%s\n```\n" % json.dumps(out))
