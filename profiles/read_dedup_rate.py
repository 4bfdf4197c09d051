#!/usr/bin/env python3
"""What duplicate removal (`mlst_set_read_dedup`, csrc/read_dedup.h; `cli type --dedup`) costs, on the two end-to-end legs of
`bench.py --full` -- FASTQ text -> ST and bgzip -> ST on E2E_READS [48,000,000] reads of its cfg3 workload (150 bases each), the same
1 Mi-record chunks and BGZF pieces, page-locked -- in the manner of profiles/read_adapters_rate.py:
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs RUNS [5]
    times after a warm-up with the library MLST_LIB names (a build of the commit before: its csrc/ and include/ compiled with build()'s
    flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...}; AB_LOG names the file that gathers those lines
    for the report.  The yardstick is the spread of the parent's own runs.
  * switch on, on three texts of the same size: the workload's own reads (what the rule finds among them is reported: they hold some exact copies of their own), a text
    in which about 30 % of the reads are copies of earlier reads picked at random, and an amplicon-like text in which about 95 % of the
    reads are copies of ONE read (one slot's atomicMin is hit by most units).  This commit runs RUNS times on either leg; then one text
    run under mlst_set_profiling gives the three launches' time together (mlst_get_kernel_time 21) next to the parse + pack slot (6).
    LEGS=text leaves the bgzip leg out (the compression of three texts takes the host minutes).
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' (pairs of alternating `bench.py --gpus 1 --steps 20
--warmup 5` processes, MLST_LIB naming the library) is copied into the report.  One JSON line, and profiles/read_dedup.md next to
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

E2E_READS = int(os.environ.get("E2E_READS", "48000000"))
RUNS = int(os.environ.get("RUNS", "5"))
MODE = os.environ.get("MODE", "all")
LABEL = os.environ.get("LABEL", "this")
AB_LOG = os.environ.get("AB_LOG", "")
LEGS = os.environ.get("LEGS", "text,bgzip").split(",")
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
out = {"runs": RUNS, "legs": LEGS}


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
tmp = tempfile.mkdtemp(prefix="mlst_dedup_")
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
pieces, n_blocks = (bgzf_pieces(text, n) if "bgzip" in LEGS else ([], 0))
res["bgzf_blocks"], res["pieces"], res["compressed_bytes"] = n_blocks, len(pieces), sum(int(p.size) for p in pieces)
res["bgzip_off_s"] = timed(this, lambda e: run_bgzip(e, pieces), RUNS) if pieces else []
say("bgzip, switch off:", res["bgzip_off_s"])
if MODE == "off":
    print(json.dumps({"label": LABEL, "reads": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}))
    sys.exit(0)
assert this.get_read_dedup() is False and this.read_dedup_info()["units"] == 0

# the three texts: rows of the text are records of one size, so a copy of a read is a copy of its row
rows = text.reshape(n, rec)
original = np.array(rows)      # (pageable: the source of the copies)
rng = np.random.default_rng(2026)


def plant(share: float, one: bool) -> None:
    """rows <- the original, then about `share` of the rows replaced by copies: of row 0 (one), else of an earlier row that stays itself"""
    rows[:] = original
    if share <= 0:
        return
    gone = rng.random(n) < share
    gone[0] = False
    where = np.nonzero(gone)[0]
    if one:
        rows[where] = original[0]
        return
    stay = np.nonzero(~gone)[0]
    before = np.searchsorted(stay, where)      # rows in front of `where` that stay: at least row 0
    src = stay[(rng.random(len(where)) * before).astype(np.int64)]
    for a in range(0, len(where), 1 << 22):
        rows[where[a:a + (1 << 22)]] = original[src[a:a + (1 << 22)]]


res["on"] = {}
for name, share, one in (("0", 0.0, False), ("30", 0.30, False), ("95", 0.95, True)):
    r = res["on"][name] = {}
    plant(share, one)
    this.reset_sample()
    this.set_read_dedup(False)
    r["text_off_s"] = timed(this, run_text, 2)      # the same text without the switch: what the copies alone change
    this.reset_sample()
    this.set_read_dedup(True)
    r["text_s"] = timed(this, run_text, RUNS)
    r["info"] = this.read_dedup_info()
    say("text, %s %% copies:" % name, r["text_s"], "off:", r["text_off_s"], r["info"])
    if "bgzip" in LEGS:
        pcs, _ = bgzf_pieces(text, n)
        r["bgzip_s"] = timed(this, lambda e: run_bgzip(e, pcs), RUNS)
        say("bgzip, %s %% copies:" % name, r["bgzip_s"])
        assert this.read_dedup_info() == r["info"]
        del pcs
    else:
        r["bgzip_s"] = []
    # the three launches alone: one text run with an event pair around every kernel group (the runs above were made without)
    this.reset_sample()
    this.set_profiling(1)
    this.reset_kernel_time()
    run_text(this)
    r["k_dd_ms"], r["k_dd_launches"] = this.kernel_time(21)
    r["parse_pack_ms"] = this.kernel_time(6)[0]
    this.set_profiling(0)
this.reset_sample()
this.set_read_dedup(False)
out["e2e"] = res
procs = [json.loads(l) for l in open(AB_LOG) if l.startswith("{")] if AB_LOG and os.path.exists(AB_LOG) else []
procs = [p for p in procs if p.get("reads") == n] + [{"label": "this", "reads": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}]
out["off_processes"] = procs
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))


def rate(ts):
    return n / min(ts) / 1e6 if ts else float("nan")


def spread(ts):
    return (max(ts) / min(ts) - 1) * 100


def secs(ts):
    return ", ".join("%.4f" % x for x in ts) if ts else "not measured"


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_dedup.md"), "w") as f:
    f.write("# Duplicate removal (`mlst_set_read_dedup`, `csrc/read_dedup.h`; `cli type --dedup`): what it costs\n\n"
            "`python profiles/read_dedup_rate.py` on one MI355X; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
            "%d reads of %d bases of `bench.py`'s cfg3 workload, %d bytes of FASTQ text in chunks of 1 Mi records, %d BGZF blocks (level 6) in %d pieces, all page-locked; a run = "
            "every submission + `typing_enqueue` + `typing_fetch`.  Legs measured: %s.\n\n" % (n, L, res["text_bytes"], res["bgzf_blocks"], res["pieces"], ", ".join(LEGS)))
    if n < 48_000_000 - 64:
        f.write("A REDUCED run: E2E_READS = %d, not the 48,000,000 of `bench.py --full`; the table ends at %d slots, not 2^27.  The rates at 48 M reads were not measured.\n\n"
                % (E2E_READS, res["on"]["0"]["info"]["slots"]))
    f.write("## Switch off: against the commit before\n\n")
    if any(p["label"] == "parent" for p in procs):
        f.write("Alternating processes on one machine, one build each (the commit before compiled from its own sources with the same flags), every process makes the same "
                "bytes and runs either leg %d times after a warm-up.\n\n| leg | process | seconds per run | best, Mreads/s |\n|---|---|---|---|\n" % RUNS)
        legs = [(leg, key) for leg, key in (("FASTQ text -> ST", "text_off_s"), ("bgzip -> ST", "bgzip_off_s")) if all(p[key] for p in procs)]
        for leg, key in legs:
            for k, p in enumerate(procs):
                f.write("| %s | %d: %s | %s | %.1f |\n" % (leg, k + 1, p["label"], secs(p[key]), rate(p[key])))
        for leg, key in legs:
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
    f.write("\n## Switch on: `--dedup`\n\nThree texts of the same size, this commit, %d runs after a warm-up (the same text without the switch: 2 runs) -- behind the switch-off "
            "runs, not alternating with them.  Reported, not gated.\n\n| leg | text | switch | seconds per run | best, Mreads/s |\n|---|---|---|---|---|\n" % RUNS)
    for name in res["on"]:
        r = res["on"][name]
        f.write("| FASTQ text -> ST | %s %% copies | off | %s | %.1f |\n" % (name, secs(r["text_off_s"]), rate(r["text_off_s"])))
        f.write("| FASTQ text -> ST | %s %% copies | on | %s | %.1f |\n" % (name, secs(r["text_s"]), rate(r["text_s"])))
        f.write("| bgzip -> ST | %s %% copies | on | %s | %.1f |\n" % (name, secs(r["bgzip_s"]), rate(r["bgzip_s"])))
    f.write("\n")
    for name in res["on"]:
        r = res["on"][name]
        i = r["info"]
        per = 1e3 * r["k_dd_ms"] / max(1, r["k_dd_launches"])
        f.write("%s %% copies: %d units, %d duplicates (%.2f %%), %d distinct keys, %d clashes, %d slots at the end (%.2f GB); levels %s.  `k_dd_insert` + `k_dd_sign` + `k_dd_mark` "
                "(one text run under `mlst_set_profiling`, one event pair around the three): %.3f ms in %d chunks = %.1f us per chunk of 1 Mi reads of %d bases, %.2f %% of the best "
                "text run; %.2f times `k_ra_cut`'s 428 us (profiles/read_adapters.md); the parse + pack group of the same run (slot 6): %.3f ms.\n\n"
                % (name, i["units"], i["duplicates"], 100.0 * i["duplicates"] / max(1, i["units"]), i["distinct"], i["clashes"], i["slots"], i["slots"] * 28 / 1e9, i["levels"],
                   r["k_dd_ms"], r["k_dd_launches"], per, L, r["k_dd_ms"] / 10 / min(r["text_s"]), per / 428.0, r["parse_pack_ms"]))
    f.write("\n```\n%s\n```\n" % json.dumps(out))
