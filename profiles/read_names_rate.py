#!/usr/bin/env python3
"""What `cli type --read-names` (mlst_set_read_names, csrc/read_names.h) costs, switch on against switch off in one process:
  * end to end, bgzip -> ST, on the E2E_READS [48,000,000] reads of `bench.py --full`'s end_to_end leg (its cfg3 workload, its BGZF
    blocks and pieces, page-locked): submit_fastq_bgzf of every piece, typing_enqueue, typing_fetch.  With the switch on a text slot
    is released behind pass 1 of its piece instead of behind k_pack_text, so the inflate of the piece after next waits longer: this
    leg shows that cost.  Alternating runs, RUNS [3] of each after one warm-up of each, every run in the JSON.
  * the `--write-sam-all` export of ISOLATE_READS [2,000,000] reads of one isolate on DB-ecoli (7 loci x 1,430 alleles, the isolate
    of profiles/sam_all.md) whose FASTQ names are 40 bytes (Illumina length): open + every round into page-locked memory + close,
    median of EXPORT_RUNS [5] after a warm-up; and the text -> pass 1 submission of the same sample.
PARTS [e2e,export] picks the legs.  The switch-off comparison with the commit before is made of separate processes (another build of
the library: MLST_LIB) and copied into the report when given: BENCH_AB='<ms per step before> <ms per step this> ...' (pairs,
alternating runs of bench.py --gpus 1 --steps 20 --warmup 5) and SAM_ALL_AB='<whole export ms of the isolate before> <this> ...'
(alternating runs of profiles/sam_all_rate.py).  One JSON line, and profiles/read_names.md next to this script."""
import ctypes as C
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
from metamlst_amd.engine import Engine, _ptr, pinned_array  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402

E2E_READS = int(os.environ.get("E2E_READS", "48000000"))
ISOLATE_READS = int(os.environ.get("ISOLATE_READS", "2000000"))
RUNS = int(os.environ.get("RUNS", "3"))
EXPORT_RUNS = int(os.environ.get("EXPORT_RUNS", "5"))
PARTS = os.environ.get("PARTS", "e2e,export").split(",")
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
out = {"runs": RUNS, "export_runs": EXPORT_RUNS}


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def e2e_leg():
    """bench.py's end_to_end bgzip leg, run with the switch off and on"""
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--pipeline", "1"] + (["--reads", str(E2E_READS)] if E2E_READS < 48_000_000 else [])
    args = bench.parse_args()
    sys.argv = argv
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="mlst_names_")
    w = bench.build_workload("cfg3", args, lambda: Engine(0), torch, device, 0, 1, tmp)
    eng = w.engines[0]
    packed, qrows, lens, n_total = w.batches[0]
    n, L = min(E2E_READS, n_total), args.read_len
    rec = 16 + 2 * L
    text = np.empty(n * rec, np.uint8)
    for at in range(0, n, 1 << 20):
        c = min(1 << 20, n - at)
        text[at * rec:(at + c) * rec] = synth.resident_to_fastq_text(torch, packed, qrows, n_total, w.wpr, w.qstride, at, c, L).cpu().numpy()
    view = memoryview(text)
    with ThreadPoolExecutor(THREADS) as ex:      # zlib releases the GIL
        parts = list(ex.map(lambda at: bgzf_block(bytes(view[at:at + 65280])), range(0, len(text), 65280)))
    header = bytes(text[:rec]).split(b"\n")[0]
    del text, view
    per_piece = 65536 if n >= 40_000_000 else 16384
    pieces = []
    for a in range(0, len(parts), per_piece):
        blob = b"".join(parts[a:a + per_piece]) + (bgzf_block(b"") if a + per_piece >= len(parts) else b"")
        pb = pinned_array(len(blob))
        pb[:] = np.frombuffer(blob, np.uint8)
        pieces.append(pb)
    n_blocks, comp_bytes = len(parts), sum(int(p.size) for p in pieces)
    del parts

    def run(on):
        eng.reset_sample()
        eng.set_read_names(on)
        eng.synchronize()
        t0 = time.perf_counter()
        got = 0
        for k, pc in enumerate(pieces):
            got += eng.submit_fastq_bgzf(pc, final=(k == len(pieces) - 1))
        eng.typing_enqueue(penalty=100)
        st, chosen, _ = eng.typing_fetch()
        t = time.perf_counter() - t0
        assert got == n
        return t, (st.sum_score.tobytes(), st.n_hits.tobytes(), tuple(sorted(chosen.items()))), eng.read_names_info()

    ref = None
    ts = {False: [], True: []}
    info = None
    for k in range(RUNS + 1):
        for on in (False, True):
            t, key, inf = run(on)
            ref = key if ref is None else ref
            assert key == ref, "the statistics differ between the runs"
            if on:
                info = inf
            else:
                assert inf == {"named": 0, "bytes": 0, "fallbacks": 0, "longest": 0}
            if k:
                ts[on].append(t)
    eng.reset_sample()
    eng.set_read_names(False)
    out["e2e"] = {"reads": n, "first_header": header.decode("ascii", "replace"), "bgzf_blocks": n_blocks, "compressed_bytes": comp_bytes, "pieces": len(pieces),
                  "off_s": ts[False], "on_s": ts[True], "names": info,
                  "off_Mreads_per_s": n / min(ts[False]) / 1e6, "on_Mreads_per_s": n / min(ts[True]) / 1e6}


def export_leg():
    """the full export of an isolate with 40-byte names, and its submission as text"""
    with tempfile.TemporaryDirectory() as tmp:
        db = synth.make_ecoli_db(tmp + "/ecoli.db", alleles_per_locus=1430, n_profiles=5000)
        idx = load_index(tmp + "/ecoli.db")
        genome, _ = synth.make_genome(db, "ecoli", db.profiles["ecoli"][3])
        N, L = ISOLATE_READS, 150
        head = b"@M01234:567:000000000-ABCDE:1:1:000000000 1:N:0:ACGT\n"      # 40 bytes of name, a description behind it
        H = len(head)
        rec = H + 2 * L + 4
        rows = np.empty((N, rec), np.uint8)
        rows[:, :H] = np.frombuffer(head, np.uint8)
        num = np.arange(N)
        for k in range(9):
            rows[:, 40 - k] = 48 + (num // 10 ** k) % 10
        for at in range(0, N, 1 << 20):
            c = min(1 << 20, N - at)
            b, q = synth.sample_reads(genome, c, seed=synth.SEED + at)
            rows[at:at + c, H:H + L] = b
            rows[at:at + c, H + L + 3:H + 2 * L + 3] = q
        rows[:, H + L] = 10; rows[:, H + L + 1] = ord("+"); rows[:, H + L + 2] = 10; rows[:, rec - 1] = 10
        text = rows.reshape(-1)
        step = (1 << 20) * rec
        eng = Engine(0)
        eng.load_reference(idx)
        labels = [idx.label(a).encode() for a in range(idx.n_alleles)]
        noff = np.zeros(len(labels) + 1, np.uint64); noff[1:] = np.cumsum([len(x) for x in labels])
        names = np.frombuffer(b"".join(labels), np.uint8)
        nb, nr, done = C.c_uint64(), C.c_uint64(), C.c_int()
        res = {"reads": N, "name_bytes": 40}
        for on in (False, True):
            def submit():
                eng.reset_sample()
                eng.set_read_names(on)
                eng.synchronize()
                t0 = time.perf_counter()
                for at in range(0, len(text), step):
                    eng.submit_fastq(text[at:at + step])
                eng.synchronize()
                return time.perf_counter() - t0
            submit()
            t_sub = [submit() for _ in range(EXPORT_RUNS)]
            chunks = list(eng.export_sam_text(idx))
            n_bytes, n_recs, biggest = sum(len(c) for c in chunks), sum(c.count(b"\n") for c in chunks), max([len(c) for c in chunks] + [1])
            first = chunks[0].split(b"\t", 1)[0] if chunks else b""
            assert n_recs == int(eng.stats().counters[0]) and (first.startswith(b"M01234:567:") if on else first.startswith(b"r"))
            buf = pinned_array(biggest)
            del chunks

            def whole():
                eng._check(eng.lib.mlst_alignments_text_open(eng._h, _ptr(names), _ptr(noff), 0, 256 << 20), "open")
                while True:
                    eng._check(eng.lib.mlst_alignments_text_next(eng._h, _ptr(buf), len(buf), C.byref(nb), C.byref(nr), C.byref(done)), "next")
                    if done.value:
                        break
                eng._check(eng.lib.mlst_alignments_text_close(eng._h), "close")
            whole()
            tw = []
            for _ in range(EXPORT_RUNS):
                t0 = time.perf_counter(); whole(); tw.append((time.perf_counter() - t0) * 1e3)
            res["on" if on else "off"] = {"records": n_recs, "bytes": n_bytes, "whole_ms": statistics.median(tw), "whole_runs_ms": tw,
                                          "submit_s": statistics.median(t_sub), "submit_runs_s": t_sub, "names": eng.read_names_info()}
        eng.close()
        out["export"] = res


if "e2e" in PARTS:
    e2e_leg()
if "export" in PARTS:
    export_leg()
ab = [float(x) for x in os.environ.get("BENCH_AB", "").split()]
sab = [float(x) for x in os.environ.get("SAM_ALL_AB", "").split()]
out["bench_ms_per_step"] = {"before": ab[0::2], "this": ab[1::2]}
out["sam_all_isolate_whole_ms"] = {"before": sab[0::2], "this": sab[1::2]}
print(json.dumps(out))

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "read_names.md"), "w") as f:
    f.write("# `cli type --read-names` (`mlst_set_read_names`, `csrc/read_names.h`): what it costs\n\n`python profiles/read_names_rate.py` on one MI355X; host clock "
            "around calls that end in a device synchronise; every run is in the JSON below.\n\n")
    f.write("## Switch off: against the commit before\n\n")
    for what, unit, xs in (("`bench.py --gpus 1 --steps 20 --warmup 5`, ms per step", "ms", ab),
                           ("`profiles/sam_all_rate.py`, whole export of the 2 M-read isolate, ms (median of 5)", "ms", sab)):
        b, t = xs[0::2], xs[1::2]
        if len(b) >= 2 and len(t) >= 1:
            f.write("* %s, alternating processes, before / this / before / this on one machine (a build of the commit before against this one's): before %s; this commit %s.  "
                    "Difference of the means %+.4f %s; spread of the runs of the commit before itself %.4f %s.\n"
                    % (what, ", ".join("%.4f" % x for x in b), ", ".join("%.4f" % x for x in t), statistics.mean(t) - statistics.mean(b), unit, max(b) - min(b), unit))
        else:
            f.write("* %s: not measured in this run.\n" % what)
    if "e2e" in out:
        e = out["e2e"]
        f.write("\n## Switch on against off: bgzip -> ST end to end\n\n%d reads of `bench.py`'s cfg3 workload (headers like `%s`), %d BGZF blocks in %d pieces from page-locked memory, "
                "`submit_fastq_bgzf` of every piece + `typing_enqueue` + `typing_fetch`; alternating runs after one warm-up of each; the statistics and the chosen alleles "
                "were equal in every run.\n\n| switch | seconds per run | best, Mreads/s |\n|---|---|---|\n| off | %s | %.1f |\n| on | %s | %.1f |\n\n"
                % (e["reads"], e["first_header"], e["bgzf_blocks"], e["pieces"], ", ".join("%.4f" % x for x in e["off_s"]), e["off_Mreads_per_s"],
                   ", ".join("%.4f" % x for x in e["on_s"]), e["on_Mreads_per_s"]))
        f.write("Best run on against best run off: %+.2f %%; spread of the runs with the switch off: %.2f %% of their best.  Names kept: %d (%d bytes, longest %d), fallbacks %d.\n"
                % ((min(e["on_s"]) / min(e["off_s"]) - 1) * 100, (max(e["off_s"]) / min(e["off_s"]) - 1) * 100, e["names"]["named"], e["names"]["bytes"], e["names"]["longest"],
                   e["names"]["fallbacks"]))
    if "export" in out:
        x = out["export"]
        f.write("\n## Switch on against off: the `--write-sam-all` export of an isolate with %d-byte names\n\n%d reads of 150 bases of one isolate on 7 loci x 1,430 alleles, FASTQ text "
                "submitted in chunks of 1 Mi records; export = open + every round into page-locked memory + close, median of %d after a warm-up.\n\n"
                "| switch | records | text bytes | whole export ms | records/s | GB/s | text -> pass 1, s (median) |\n|---|---|---|---|---|---|---|\n" % (x["name_bytes"], x["reads"], EXPORT_RUNS))
        for k in ("off", "on"):
            s = x[k]
            f.write("| %s | %d | %d | %.3f | %.3g | %.2f | %.4f |\n" % (k, s["records"], s["bytes"], s["whole_ms"], s["records"] / (s["whole_ms"] * 1e-3),
                                                                        s["bytes"] / (s["whole_ms"] * 1e-3) / 1e9, s["submit_s"]))
        f.write("\nExport on against off: %+.2f %% time for %+.2f %% bytes; submission on against off: %+.2f %%.  Names kept: %d (%d bytes).\n"
                % ((x["on"]["whole_ms"] / x["off"]["whole_ms"] - 1) * 100, (x["on"]["bytes"] / x["off"]["bytes"] - 1) * 100,
                   (x["on"]["submit_s"] / x["off"]["submit_s"] - 1) * 100, x["on"]["names"]["named"], x["on"]["names"]["bytes"]))
    f.write("\n```\n%s\n```\n" % json.dumps(out))
