"""The examiner waves of k_route_probe (MLST_PROBE_EXAM_WAVES) on the bench's cfg3 workload: one process, resident batches, one
engine per setting.  Per setting and batch the statistics, all counters and the sorted candidate list are compared with the first
setting's (bit-exact), then the sieve's kernels are timed alone (HIP events, ms per submission, median of --launches).

    python3 profiles/probe_examiners.py [--settings 0,1,2,4,2+idle] [--batches 2] [--launches 12] [--out FILE]

A setting is the number of examiner waves; "N+idle" adds MLST_RT_DEBUG=16 (the ring is bypassed: 16 - N streaming waves, the
examiners wait and do nothing, k_route_verify examines everything -- what giving up N streaming waves costs by itself).
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("sieve", "sieve_route", "sieve_probe", "sieve_verify", "seed")


def env_of(setting):
    n, _, idle = setting.partition("+")
    ev = {"MLST_PROBE_EXAM_WAVES": str(int(n))}
    if idle:
        ev["MLST_RT_DEBUG"] = "16"
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="0,1,2,4,2+idle")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    import bench
    from metamlst_amd.engine import Engine
    device = torch.device("cuda:0")
    settings = a.settings.split(",")
    args = types.SimpleNamespace(alleles=0, reads=a.reads, genome_size=0, species=150, genomes=20, read_len=150)
    engines = []

    def factory():
        e = Engine(0)
        engines.append(e)
        return e

    w = bench.build_workload("cfg3", args, factory, torch, device, 0, a.batches, tempfile.mkdtemp())
    while len(engines) < len(settings):      # (build_workload makes one engine per batch)
        e = Engine(0)
        e.load_reference(w.idx)
        engines.append(e)
    out = {"reads": int(w.batches[0][3]), "settings": {}}
    ref = {}
    for s, e in zip(settings, engines):
        ev = env_of(s)
        os.environ.update(ev)      # both switches are read at submission time
        rec = {"same_as_first": True, "ring_full": [], "candidates": [], "parked": []}
        for b in range(a.batches):
            packed, qrows, lens, n = w.batches[b]
            e.reset_sample()
            e.submit_packed_device(packed.data_ptr(), qrows.data_ptr(), lens.data_ptr(), n, w.wpr, w.qstride)
            st = e.stats()
            full, cand = e.debug_route_probe()
            key = (st.sum_score.copy(), st.n_hits.copy(), st.locus_len_sum.copy(), st.locus_first.copy(), np.asarray(st.counters).copy(), cand)
            if b not in ref:
                ref[b] = key
            elif not all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(ref[b], key)):
                rec["same_as_first"] = False
            rec["ring_full"].append(full); rec["candidates"].append(int(cand.size)); rec["parked"].append(int(st.counters[7]))
        packed, qrows, lens, n = w.batches[0]
        e.set_profiling(1)
        t = {k: [] for k in KERNELS}
        for _ in range(a.launches):
            e.reset_sample()
            e.reset_kernel_time()
            e.submit_packed_device(packed.data_ptr(), qrows.data_ptr(), lens.data_ptr(), n, w.wpr, w.qstride)
            e.synchronize()
            for k in KERNELS:
                t[k].append(e.kernel_time(k)[0])
        e.set_profiling(0)
        for k in ev:
            os.environ.pop(k, None)
        rec["ms_per_submission"] = {k: round(float(np.median(v)), 4) for k, v in t.items()}
        rec["ms_min"] = {k: round(float(min(v)), 4) for k, v in t.items()}
        out["settings"][s] = rec
        print(s, rec, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["same_as_first"] for r in out["settings"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
