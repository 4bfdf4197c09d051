#!/usr/bin/env python3
"""What mate overlap trimming (`mlst_set_read_pair_overlap`, csrc/read_overlap.h; `cli type -2 MATES --pair-overlap`) costs, in the manner
of profiles/read_adapters_rate.py, on E2E_PAIRS [24,000,000] pairs of 150-base mates of a synthetic isolate (a 2 Mb genome with the alleles
of one ST of a 7 x 300 allele database embedded, fragments uniform over it, Phred 40, page-locked text in chunks of 512 Ki pairs):
  * switch off, this commit against the commit before, in alternating PROCESSES on one machine: MODE=off runs the two legs -- FASTQ text
    -> ST and bgzip -> ST, the pairs without read-through as unpaired text -- RUNS [3] times after a warm-up with the library MLST_LIB
    names (a build of the commit before with build()'s flags; MLST_LIB_ALLOW_MISSING=1) and prints one JSON line {"label": LABEL, ...};
    AB_LOG names the file that gathers those lines for the report.  The yardstick is the spread of the parent's own runs.
  * switch on: three sets of pairs -- no read-through (inserts 300 - 500), 30 % and 100 % read-through (inserts 40 - 149, the mates
    running into two different adapters) -- submitted as pairs (interleaved text, what `-2` hands over), each RUNS times with the switch
    off and on; then one run under mlst_set_profiling gives k_po_cut alone (mlst_get_kernel_time 22), and one more with
    mlst_set_read_adapters (one adapter) in front gives k_ra_cut (19) beside it on the same run.
  * the kernel's own word operations per pair (a word step: one 64-bit word of mate 1 against two funnel-shifted words of the reversed
    mate 2), counted here from the rule's offsets, beside the measured time.
The headline step is bench.py's own: BENCH_AB='<ms per step before> <this> ...' is copied into the report.  One JSON line, and
profiles/read_overlap.md next to this script."""
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
from metamlst_amd.index import load_index  # noqa: E402

PAIRS = int(os.environ.get("E2E_PAIRS", "24000000"))
RUNS = int(os.environ.get("RUNS", "3"))
MODE = os.environ.get("MODE", "all")
LABEL = os.environ.get("LABEL", "this")
AB_LOG = os.environ.get("AB_LOG", "")
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
L = 150
HEAD = 14                      # "@" + twelve digits + "\n"
REC = HEAD + 2 * L + 4         # a record: header, sequence, "+", qualities
CHUNK = 1 << 20                # records per submission (512 Ki pairs)
ADAPTER = "AGATCGGAAGAGC"
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def pair_text(genome: np.ndarray, n: int, share: float, seed: int) -> np.ndarray:
    """interleaved text of n pairs (page-locked); `share` of them have an insert shorter than the mates"""
    rng = np.random.default_rng(seed)
    ad = [np.concatenate([np.frombuffer(ADAPTER.encode(), np.uint8), synth._ACGT[rng.integers(0, 4, size=L, dtype=np.uint8)]]) for _ in range(2)]
    text = pinned_array(2 * n * REC)
    rows = text.reshape(2 * n, REC)
    col = np.arange(L)
    for at in range(0, n, 1 << 18):
        c = min(1 << 18, n - at)
        insert = np.where(rng.random(c) < share, rng.integers(40, L, size=c), rng.integers(300, 501, size=c))
        start = rng.integers(0, len(genome) - 500, size=c)
        inside = col[None, :] < insert[:, None]
        m1 = np.where(inside, genome[start[:, None] + np.minimum(col[None, :], insert[:, None] - 1)], ad[0][np.maximum(col[None, :] - insert[:, None], 0)])
        m2 = np.where(inside, COMP[genome[start[:, None] + np.maximum(insert[:, None] - 1 - col[None, :], 0)]], ad[1][np.maximum(col[None, :] - insert[:, None], 0)])
        r = rows[2 * at:2 * (at + c)]
        r[:, 0] = ord("@")
        ids = np.repeat(np.arange(at, at + c), 2)
        for d in range(12):
            r[:, 12 - d] = 48 + (ids // 10 ** d) % 10
        r[:, 13] = 10
        r[0::2, HEAD:HEAD + L] = m1
        r[1::2, HEAD:HEAD + L] = m2
        r[:, HEAD + L] = 10
        r[:, HEAD + L + 1] = ord("+")
        r[:, HEAD + L + 2] = 10
        r[:, HEAD + L + 3:HEAD + 2 * L + 3] = 73
        r[:, REC - 1] = 10
    return text


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_pieces(text: np.ndarray) -> tuple[list, int]:
    view = memoryview(text)
    with ThreadPoolExecutor(THREADS) as ex:      # zlib releases the GIL
        parts = list(ex.map(lambda at: bgzf_block(bytes(view[at:at + 65280])), range(0, len(text), 65280)))
    pieces = []
    for a in range(0, len(parts), 16384):
        blob = b"".join(parts[a:a + 16384]) + (bgzf_block(b"") if a + 16384 >= len(parts) else b"")
        pb = pinned_array(len(blob))
        pb[:] = np.frombuffer(blob, np.uint8)
        pieces.append(pb)
    return pieces, len(parts)


def finish(eng, t0):
    eng.typing_enqueue(penalty=100)
    st, chosen, _ = eng.typing_fetch()
    return time.perf_counter() - t0, (st.sum_score.tobytes(), st.n_hits.tobytes(), tuple(sorted(chosen.items())))


def run_text(eng, text, paired):
    t0 = time.perf_counter()
    for at in range(0, len(text), CHUNK * REC):
        eng.submit_fastq(text[at:at + CHUNK * REC], paired=paired)
    return finish(eng, t0)


def run_bgzip(eng, pieces):
    t0 = time.perf_counter()
    for k, pc in enumerate(pieces):
        eng.submit_fastq_bgzf(pc, final=(k == len(pieces) - 1))
    return finish(eng, t0)


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


def spread(ts):
    return (max(ts) / min(ts) - 1) * 100


OPS = 30      # 32-bit vector operations of one word step, counted by hand in k_po_cut's source: two 64-bit funnel shifts (2 x 6), XOR (2), fold (4),
#               three ANDs and a NOT (8), two popcounts with their add (2), the carry of the two words (0: renamed) and the loop's own (2)


def report(out: dict) -> None:
    """profiles/read_overlap.md from the JSON line of a run"""
    n, res, procs = out["pairs"], out["e2e"], out["off_processes"]
    ab = [x for pair in zip(out["bench_ms_per_step"]["before"], out["bench_ms_per_step"]["this"]) for x in pair]
    name = out["device"]["name"]

    def rate(ts):
        return 2 * n / min(ts) / 1e6
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_overlap.md"), "w") as f:
        f.write("# Mate overlap trimming (`mlst_set_read_pair_overlap`, `csrc/read_overlap.h`; `cli type -2 MATES --pair-overlap`): what it costs\n\n"
                "`python profiles/read_overlap_rate.py` on one %s; host clock around calls that end in a device synchronise; every run is in the JSON below.  "
                "%d pairs of %d-base mates (E2E_PAIRS; the script's default is 24 M) of a synthetic isolate, %d bytes of interleaved FASTQ text in chunks of 512 Ki pairs, "
                "page-locked; a run = every submission + `typing_enqueue` + `typing_fetch`.\n\n" % (name, n, L, res["text_bytes"]))
        f.write("## Switch off: against the commit before\n\n")
        if any(p["label"] == "parent" for p in procs):
            f.write("Alternating processes on one machine, one build each (the commit before compiled from its own sources with the same flags); every process makes the same bytes "
                    "(the pairs without read-through, as unpaired text; %d BGZF blocks at level 6 in %d pieces) and runs either leg %d times after a warm-up.\n\n"
                    "| leg | process | seconds per run | best, Mreads/s |\n|---|---|---|---|\n" % (res["bgzf_blocks"], res["pieces"], RUNS))
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
        f.write("\n## Switch on: pairs as `-2` hands them over, defaults (30 / 5 / 20 %%)\n\nThis commit, %d runs after a warm-up each, behind the switch-off runs, not alternating "
                "with them.  Reported, not gated.\n\n| read-through | switch | seconds per run | best, Mreads/s | pairs cut | bases removed |\n|---|---|---|---|---|---|\n" % RUNS)
        for share, r in res["on"].items():
            f.write("| %s %% | off | %s | %.1f | | |\n" % (share, ", ".join("%.4f" % x for x in r["off_s"]), rate(r["off_s"])))
            f.write("| %s %% | on | %s | %.1f | %d | %d |\n" % (share, ", ".join("%.4f" % x for x in r["on_s"]), rate(r["on_s"]), r["info"]["trimmed_pairs"], r["info"]["bases_removed"]))
        f.write("\n## `k_po_cut` itself\n\nOne text run under `mlst_set_profiling` (event pairs around the kernel), then one more with `mlst_set_read_adapters` (%s) in front, "
                "which gives `k_ra_cut` on the same run (with the adapter cut in front, mate 1 of a read-through pair reaches `k_po_cut` already cut).\n\n"
                "| read-through | k_po_cut, us per 1 Mi pairs | parse + pack group (6), ms | with the adapter: k_ra_cut, us per 1 Mi pairs (2 Mi reads) | k_po_cut behind it |\n|---|---|---|---|---|\n" % ADAPTER)
        mi = (1 << 20) / n
        for share, r in res["on"].items():
            f.write("| %s %% | %.1f | %.3f | %.1f | %.1f |\n" % (share, 1e3 * r["k_po_cut_ms"] * mi, r["parse_pack_ms"], 1e3 * r["with_adapter"]["k_ra_cut_ms"] * mi, 1e3 * r["with_adapter"]["k_po_cut_ms"] * mi))
        r = res["on"]["0"]
        cu, khz = out["device"]["compute_units"], out["device"]["clock_khz"]
        f.write("\nWord operations: a %d / %d pair has %d offsets and %d word steps (one 64-bit word of mate 1 against two funnel-shifted words of the reversed mate 2), about %d "
                "32-bit vector operations each by a count of the source by hand (not of the assembly): %.0f lane operations per pair.  " % (L, L, r["offsets_per_pair"], r["word_steps_per_pair"], OPS, OPS * r["word_steps_per_pair"]))
        if not khz:
            khz = int(os.environ.get("CLOCK_KHZ", "2400000"))
            f.write("(The device reported no clock: CLOCK_KHZ, by default the 2.4 GHz peak engine clock of the MI355X's data sheet, stands in.)  ")
        if khz:
            bound = (1 << 20) * OPS * r["word_steps_per_pair"] / (cu * 64.0 * khz * 1e3) * 1e6
            f.write("At %d CUs x 64 lanes x %.2f GHz that is %.1f us per 1 Mi pairs if every lane of every cycle did such an operation; the kernel takes %.1f us without read-through, "
                    "%.1f times that bound (the conversion of the mates, the LDS reads, the barriers and the lanes of a last round without an offset are the rest; the assembly was not read).\n"
                    % (cu, khz / 1e6, bound, 1e3 * r["k_po_cut_ms"] * mi, 1e3 * r["k_po_cut_ms"] * mi / bound))
        else:
            f.write("The device's clock was not reported, so no bound is given.\n")
        f.write("\nNot measured: `.gz` and bgzip'd mates with the switch on, `--gpus N`, reads of other lengths, a real library.\n")
        f.write("\n```\n%s\n```\n" % json.dumps(out))


if os.environ.get("REPORT_FROM"):      # the report again from the JSON line of an earlier run, without a GPU
    report(json.loads(open(os.environ["REPORT_FROM"]).read().strip().splitlines()[-1]))
    sys.exit(0)
torch.cuda.set_device(0)
tmp = tempfile.mkdtemp(prefix="mlst_overlap_")
db = synth.make_ecoli_db(tmp + "/s.db", alleles_per_locus=300, n_profiles=20)
idx = load_index(tmp + "/s.db")
genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][3], size=2_000_000)
eng = Engine(0)
eng.load_reference(idx)
n = PAIRS
out = {"runs": RUNS, "pairs": n, "read_len": L}
texts = {0: pair_text(genome, n, 0.0, 1)}
say("text made:", n, "pairs,", texts[0].size, "bytes")
res = {"text_bytes": int(texts[0].size)}
res["text_off_s"] = timed(eng, lambda e: run_text(e, texts[0], False), RUNS)
say("text, unpaired, switch off:", res["text_off_s"])
pieces, res["bgzf_blocks"] = bgzf_pieces(texts[0])
res["pieces"] = len(pieces)
res["bgzip_off_s"] = timed(eng, lambda e: run_bgzip(e, pieces), RUNS)
say("bgzip, unpaired, switch off:", res["bgzip_off_s"])
if MODE == "off":
    print(json.dumps({"label": LABEL, "pairs": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}))
    sys.exit(0)
del pieces
res["on"] = {}
props = torch.cuda.get_device_properties(0)
for share in (0, 30, 100):
    text = texts.get(share)
    if text is None:
        text = pair_text(genome, n, share / 100.0, 1 + share)
    r = res["on"][str(share)] = {}
    eng.reset_sample()
    eng.set_read_pair_overlap(False)
    r["off_s"] = timed(eng, lambda e: run_text(e, text, True), RUNS)
    eng.reset_sample()
    eng.set_read_pair_overlap(True)
    r["on_s"] = timed(eng, lambda e: run_text(e, text, True), RUNS)
    info = eng.read_pair_overlap_info()
    hist = info.pop("insert_hist")
    r["info"] = info
    say("%d %% read-through: off" % share, r["off_s"], "on", r["on_s"], info)
    assert info["pairs"] == n and abs(info["trimmed_pairs"] - n * share / 100.0) <= 0.01 * n + 100, info
    eng.reset_sample()
    eng.set_profiling(1)
    eng.reset_kernel_time()
    run_text(eng, text, True)
    r["k_po_cut_ms"], r["k_po_cut_launches"] = eng.kernel_time(22)
    r["parse_pack_ms"] = eng.kernel_time(6)[0]
    eng.reset_sample()
    eng.set_read_adapters([ADAPTER])
    eng.reset_kernel_time()
    run_text(eng, text, True)
    r["with_adapter"] = {"k_ra_cut_ms": eng.kernel_time(19)[0], "k_po_cut_ms": eng.kernel_time(22)[0], "launches": eng.kernel_time(22)[1]}
    eng.set_profiling(0)
    eng.reset_sample()
    eng.set_read_adapters()
    eng.set_read_pair_overlap(False)
    # the kernel's word steps per pair, from the rule's offsets: o = -(n2 - 30) .. n1 - 30, the words of mate 1 under the overlap
    steps = sum(((min(L, o + L) - 1) >> 5) - (max(0, o) >> 5) + 1 for o in range(-(L - 30), L - 30 + 1))
    r["word_steps_per_pair"], r["offsets_per_pair"] = steps, 2 * (L - 30) + 1
    del text
out["e2e"] = res
out["device"] = {"name": props.name, "compute_units": props.multi_processor_count, "clock_khz": getattr(props, "clock_rate", 0)}
procs = [json.loads(l) for l in open(AB_LOG) if l.startswith("{")] if AB_LOG and os.path.exists(AB_LOG) else []
procs = [p for p in procs if p.get("pairs") == n] + [{"label": "this", "pairs": n, "text_off_s": res["text_off_s"], "bgzip_off_s": res["bgzip_off_s"]}]
out["off_processes"] = procs
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
print(json.dumps(out))

report(out)
