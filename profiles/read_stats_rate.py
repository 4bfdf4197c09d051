#!/usr/bin/env python3
"""What the per-cycle read statistics (`mlst_set_read_stats`, csrc/read_stats.h; `cli type --read-stats`) cost, on the two end-to-end
legs of `bench.py --full` -- FASTQ text -> ST and bgzip -> ST on E2E_READS [48,000,000] reads of its cfg3 workload (150 bases each),
the same 1 Mi-record chunks and BGZF pieces, page-locked -- in the manner of profiles/read_adapters_rate.py:
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs RUNS [5]
    times after a warm-up with the library MLST_LIB names (a build of the commit before: its csrc/ and include/ compiled with build()'s
    flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...}; AB_LOG names the file that gathers those lines
    for the report.  The yardstick is the spread of the parent's own runs.
  * switch on, with no trims (one launch of k_rs_count per chunk: raw) and with --trim5 5 --trim3 5 --trim-qual 20 and one adapter
    (two launches: raw and prepared), each against the same setting with the switch off: this commit runs RUNS times on either leg;
    then one text run under mlst_set_profiling gives k_rs_count's time alone (mlst_get_kernel_time 20) next to k_rp_qtrim (18),
    k_ra_cut (19) and the parse + pack group they all run inside (6; k_pack_text has no slot of its own).
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' (pairs of alternating `bench.py --gpus 1 --steps 20
--warmup 5` processes, MLST_LIB naming the library) is copied into the report.  One JSON line, and profiles/read_stats.md next to
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
SETTINGS = {"no trims": ({}, None),
            "all trims + 1 adapter": ({"trim5": 5, "trim3": 5, "trim_qual": 20}, [ADAPTER_NAMES["illumina"]])}
out = {"runs": RUNS, "settings": {k: [p, a] for k, (p, a) in SETTINGS.items()}}


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
tmp = tempfile.mkdtemp(prefix="mlst_rstats_")
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
assert this.get_read_stats() is False and this.read_stats_info() == {"raw_launches": 0, "prepared_launches": 0, "table_bytes": 0}
res["on"] = {}
for name, (prep, adapters) in SETTINGS.items():
    r = res["on"][name] = {}
    for on in (False, True):
        this.reset_sample()
        this.set_read_prep(**prep)
        this.set_read_adapters(adapters)
        this.set_read_stats(on)
        key = "on" if on else "off"
        r["text_%s_s" % key] = timed(this, run_text, RUNS)
        r["bgzip_%s_s" % key] = timed(this, lambda e: run_bgzip(e, pieces), RUNS)
        say("%s, switch %s: text" % (name, key), r["text_%s_s" % key], "bgzip", r["bgzip_%s_s" % key])
    info = this.read_stats_info()
    st = this.read_stats()
    assert st["raw"][0]["reads"] == n and st["raw"][0]["bases"] == n * L and st["prepared_counted"] == bool(prep or adapters)
    r["launches"], r["prepared_bases"] = info, int(st["prepared"][0]["bases"])
    # k_rs_count alone: one text run with an event pair around every kernel group (the runs above were made without)
    this.reset_sample()
    this.set_profiling(1)
    this.reset_kernel_time()
    run_text(this)
    r["k_rs_count_ms"], r["k_rs_count_launches"] = this.kernel_time(20)
    r["k_rp_qtrim_ms"], r["k_rp_qtrim_launches"] = this.kernel_time(18)
    r["k_ra_cut_ms"], r["k_ra_cut_launches"] = this.kernel_time(19)
    r["parse_pack_ms"] = this.kernel_time(6)[0]
    this.set_profiling(0)
this.reset_sample()
this.set_read_stats(False)
this.set_read_prep()
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


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_stats.md"), "w") as f:
    f.write("# Per-cycle read statistics (`mlst_set_read_stats`, `csrc/read_stats.h`; `cli type --read-stats`): what they cost\n\n"
            "`python profiles/read_stats_rate.py` on one MI355X; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
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
    f.write("\n## Switch on\n\nThe same text, this commit, %d runs after a warm-up, the switch off and on under the same read preparation -- behind the switch-off runs "
            "above, not alternating with them.  Reported, not gated.\n\n| leg | setting | switch | seconds per run | best, Mreads/s |\n|---|---|---|---|---|\n" % RUNS)
    for leg, stem in (("FASTQ text -> ST", "text"), ("bgzip -> ST", "bgzip")):
        for name in SETTINGS:
            for key in ("off", "on"):
                ts = res["on"][name]["%s_%s_s" % (stem, key)]
                f.write("| %s | %s | %s | %s | %.1f |\n" % (leg, name, key, ", ".join("%.4f" % x for x in ts), rate(ts)))
    f.write("\n")
    for name in SETTINGS:
        r = res["on"][name]
        per = 1e3 * r["k_rs_count_ms"] / max(1, r["k_rs_count_launches"])
        counted = n * L + (r["prepared_bases"] if r["launches"]["prepared_launches"] else 0)      # bases over all launches of the sample
        text_bytes_per_launch = 2.0 * counted / max(1, r["k_rs_count_launches"])
        f.write("%s: %d raw and %d prepared launches over the sample.  `k_rs_count` alone (one text run under `mlst_set_profiling`, event pairs around the kernel): %.3f ms in %d "
                "launches = %.1f us per launch over a chunk of 1 Mi reads of %d bases, %.2f %% of the best text run with the switch on and %.2f %% of the best bgzip run; best "
                "against best the switch costs %+.2f %% on the text leg and %+.2f %% on the bgzip leg.  Of the same run: `k_rp_qtrim` %.3f ms in %d launches, `k_ra_cut` %.3f ms "
                "in %d launches, the parse + pack group all of them run inside (slot 6; `k_pack_text` has no slot of its own) %.3f ms.  A launch reads 2 bytes per base, on average "
                "%.0f MB of text the parser has just touched: %.0f GB/s against 8 TB/s of HBM -- %s.\n\n"
                % (name, r["launches"]["raw_launches"], r["launches"]["prepared_launches"], r["k_rs_count_ms"], r["k_rs_count_launches"], per, L,
                   r["k_rs_count_ms"] / 10 / min(r["text_on_s"]), r["k_rs_count_ms"] / 10 / min(r["bgzip_on_s"]),
                   (min(r["text_on_s"]) / min(r["text_off_s"]) - 1) * 100, (min(r["bgzip_on_s"]) / min(r["bgzip_off_s"]) - 1) * 100,
                   r["k_rp_qtrim_ms"], r["k_rp_qtrim_launches"], r["k_ra_cut_ms"], r["k_ra_cut_launches"], r["parse_pack_ms"],
                   text_bytes_per_launch / 1e6, text_bytes_per_launch / (per * 1e-6) / 1e9 if per else 0.0,
                   "the time does not follow the bytes" if per and text_bytes_per_launch / (per * 1e-6) < 2e12 else "the time follows the bytes"))
    one = res["on"]["no trims"]
    per = 1e3 * one["k_rs_count_ms"] / max(1, one["k_rs_count_launches"])
    adds = 2.0 * L * (1 << 20)      # one quality add and one letter add per base
    f.write("Against `k_rp_qtrim` (218 us per 1 Mi reads, profiles/read_prep.md): %.2f times its time per launch.  LDS adds: %.0f M per launch (one quality and one letter add per "
            "base) = %.0f G adds/s over the device, %.1f adds per CU and clock at 2.4 GHz on 256 CUs -- a 64-lane `ds_add_u32` retires at most 32 adds per clock and CU when no "
            "two lanes meet on a bank, so this is the figure the time is held against (DESIGN.md 4.3).\n" % (per / 218.0, adds / 1e6, adds / (per * 1e-6) / 1e9 if per else 0.0,
                                                                                                              adds / (per * 1e-6) / 2.4e9 / 256 if per else 0.0))
    f.write("\n```\n%s\n```\n" % json.dumps(out))
