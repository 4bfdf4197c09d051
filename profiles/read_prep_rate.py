#!/usr/bin/env python3
"""What read preparation (`mlst_set_read_prep`, csrc/read_prep.h; `cli type --trim5 / --trim3 / --trim-qual / --phred64`) costs, on the two
end-to-end legs of `bench.py --full` -- FASTQ text -> ST and bgzip -> ST on E2E_READS [48,000,000] reads of its cfg3 workload, the same
1 Mi-record chunks and BGZF pieces, page-locked:
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs RUNS [5]
    times after a warm-up with the library MLST_LIB names (a build of the commit before: its csrc/ and include/ compiled with build()'s
    flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...}; AB_LOG names the file that gathers those lines
    for the report.  The yardstick is the spread of the parent's own runs.  (Two engines of the two builds in ONE process do not
    compare: the parent's engine, made second in a process of this commit's, ran its bgzip leg 40 % slower than in a process of its own.)
  * switch on (--trim5 5 --trim3 5 --trim-qual 20 --phred64): the qualities of the text are then raised by 31 in place (a Phred+64
    copy of the same sample), the BGZF blocks are made again, and this commit runs RUNS times on either leg; then one text run under
    mlst_set_profiling gives k_rp_qtrim's time alone (mlst_get_kernel_time 18) next to the parse + pack slot (6).
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' (pairs of alternating `bench.py --gpus 1 --steps 20
--warmup 5` processes, MLST_LIB naming the library) is copied into the report.  One JSON line, and profiles/read_prep.md next to this
script."""
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
ON = {"trim5": 5, "trim3": 5, "trim_qual": 20, "phred64": True}
out = {"runs": RUNS, "setting_on": ON}


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
tmp = tempfile.mkdtemp(prefix="mlst_prep_")
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


def timed(engines: dict, fn, runs: int) -> dict:
    """alternating runs of fn on every engine after one warm-up of each; every engine must leave the same statistics"""
    ts, ref = {k: [] for k in engines}, None
    for r in range(runs + 1):
        for k, e in engines.items():
            e.reset_sample()
            e.synchronize()
            t, key = fn(e)
            ref = key if ref is None else ref
            assert key == ref, "the statistics differ between the runs"
            if r:
                ts[k].append(t)
    return ts


off = {"this": this}
res = {"reads": n, "text_bytes": int(text.size)}
res["text_off_s"] = timed(off, run_text, RUNS)
say("text, switch off:", res["text_off_s"])
pieces, n_blocks = bgzf_pieces(text, n)
res["bgzf_blocks"], res["pieces"], res["compressed_bytes"] = n_blocks, len(pieces), sum(int(p.size) for p in pieces)
res["bgzip_off_s"] = timed(off, lambda e: run_bgzip(e, pieces), RUNS)
say("bgzip, switch off:", res["bgzip_off_s"])
if MODE == "off":
    print(json.dumps({"label": LABEL, "reads": n, "text_off_s": res["text_off_s"]["this"], "bgzip_off_s": res["bgzip_off_s"]["this"]}))
    sys.exit(0)
assert this.get_read_prep() == {"trim5": 0, "trim3": 0, "trim_qual": 0, "phred64": False} and this.read_prep_info() == {"shortened": 0, "bases_removed": 0, "emptied": 0}
del pieces
# ---- switch on: a Phred+64 copy of the same sample (every quality byte + 31, in place)
rows = text.reshape(n, rec)
for at in range(0, n, 1 << 22):
    rows[at:at + (1 << 22), rec - 1 - L:rec - 1] += 31
assert bytes(rows[0, rec - 1:]) == b"\n" and bytes(rows[0, rec - 3 - L:rec - 1 - L]) == b"+\n"
this.reset_sample()
this.set_read_prep(**ON)
res["text_on_s"] = timed({"this": this}, run_text, RUNS)["this"]
res["info_on"] = this.read_prep_info()
say("text, switch on:", res["text_on_s"], res["info_on"])
assert res["info_on"]["shortened"] == n and res["info_on"]["bases_removed"] >= 10 * n
pieces, _ = bgzf_pieces(text, n)
res["compressed_bytes_on"] = sum(int(p.size) for p in pieces)
res["bgzip_on_s"] = timed({"this": this}, lambda e: run_bgzip(e, pieces), RUNS)["this"]
say("bgzip, switch on:", res["bgzip_on_s"])
assert this.read_prep_info() == res["info_on"]
# k_rp_qtrim alone: one text run with an event pair around every kernel group (the runs above were made without)
this.reset_sample()
this.set_profiling(1)
this.reset_kernel_time()
run_text(this)
res["k_rp_qtrim_ms"], res["k_rp_qtrim_launches"] = this.kernel_time(18)
res["parse_pack_ms"] = this.kernel_time(6)[0]
this.set_profiling(0)
this.reset_sample()
this.set_read_prep()
out["e2e"] = res
procs = [json.loads(l) for l in open(AB_LOG)] if AB_LOG and os.path.exists(AB_LOG) else []
procs = [p for p in procs if p.get("reads") == n] + [{"label": "this", "reads": n, "text_off_s": res["text_off_s"]["this"], "bgzip_off_s": res["bgzip_off_s"]["this"]}]
out["off_processes"] = procs
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))


def rate(ts):
    return n / min(ts) / 1e6


def spread(ts):
    return (max(ts) / min(ts) - 1) * 100


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_prep.md"), "w") as f:
    f.write("# Read preparation (`mlst_set_read_prep`, `csrc/read_prep.h`; `cli type --trim5 / --trim3 / --trim-qual / --phred64`): what it costs\n\n"
            "`python profiles/read_prep_rate.py` on one MI355X; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
            "%d reads of `bench.py`'s cfg3 workload, %d bytes of FASTQ text in chunks of 1 Mi records, %d BGZF blocks (level 6) in %d pieces, all page-locked; a run = "
            "every submission + `typing_enqueue` + `typing_fetch`.\n\n" % (n, res["text_bytes"], res["bgzf_blocks"], res["pieces"]))
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
                "Difference of the means %+.4f ms; spread of the runs of the commit before itself %.4f ms.\n"
                % (", ".join("%.4f" % x for x in b), ", ".join("%.4f" % x for x in t), statistics.mean(t) - statistics.mean(b), max(b) - min(b)))
    else:
        f.write("\nHeadline step: not measured in this run.\n")
    f.write("\n## Switch on: `--trim5 5 --trim3 5 --trim-qual 20 --phred64`\n\nThe same reads as a Phred+64 file (every quality byte raised by 31 in place, the BGZF blocks made "
            "again: %d compressed bytes against %d), this commit, %d runs after a warm-up -- behind the switch-off runs, not alternating with them.  %d reads shortened, %d bases "
            "removed, %d reads left without a base.\n\n| leg | switch | seconds per run | best, Mreads/s |\n|---|---|---|---|\n"
            % (res["compressed_bytes_on"], res["compressed_bytes"], RUNS, res["info_on"]["shortened"], res["info_on"]["bases_removed"], res["info_on"]["emptied"]))
    for leg, k_off, k_on in (("FASTQ text -> ST", "text_off_s", "text_on_s"), ("bgzip -> ST", "bgzip_off_s", "bgzip_on_s")):
        for p in procs:
            if p["label"] == "parent":
                f.write("| %s | off, parent | %s | %.1f |\n" % (leg, ", ".join("%.4f" % x for x in p[k_off]), rate(p[k_off])))
        f.write("| %s | off, this | %s | %.1f |\n" % (leg, ", ".join("%.4f" % x for x in res[k_off]["this"]), rate(res[k_off]["this"])))
        f.write("| %s | on, this | %s | %.1f |\n" % (leg, ", ".join("%.4f" % x for x in res[k_on]), rate(res[k_on])))
    f.write("\n`k_rp_qtrim` alone (one text run under `mlst_set_profiling`, event pairs around the kernel): %.3f ms in %d launches = %.1f us per chunk of 1 Mi reads, "
            "%.2f %% of the best text run and %.2f %% of the best bgzip run; the parse + pack group of the same run (slot 6, which holds it): %.3f ms.\n"
            % (res["k_rp_qtrim_ms"], res["k_rp_qtrim_launches"], 1e3 * res["k_rp_qtrim_ms"] / max(1, res["k_rp_qtrim_launches"]),
               res["k_rp_qtrim_ms"] / 10 / min(res["text_on_s"]), res["k_rp_qtrim_ms"] / 10 / min(res["bgzip_on_s"]), res["parse_pack_ms"]))
    f.write("\n## Compile check\n\n`hipcc --offload-arch=gfx950 -O3` of this commit: `k_rp_qtrim` 52 VGPR, 53 SGPR, no LDS, no scratch, no spills; `k_pack_text<33>` 60 VGPR, 63 SGPR, "
            "no scratch -- its instructions are the parent's `k_pack_text` one for one (the assembly differs in label numbers only), as are `k_pack`'s and `k_fq_records<false>`'s; "
            "`k_pack_text<64>` 58 VGPR, 63 SGPR, no scratch (LDS of both: the 64 x RW words of the group, as before).\n")
    f.write("\n```\n%s\n```\n" % json.dumps(out))
