"""Examiner waves of the routed sieve's consumer (k_route_probe, MLST_PROBE_EXAM_WAVES): with 1, 2 or 4 of the workgroup's 16
waves examining the parked entries out of the LDS ring, the candidate list, the counters and the per-allele statistics equal
those of the separate launch (the switch at 0, k_route_verify examines everything) -- the candidate set is a set of flag bits
OR-ed by idempotent atomics, so neither who examines an entry nor when can change it.

Two inputs on a database forced onto the routed sieve:
  ordinary   reads of one isolate: the ring never fills (fall-back counter 0)
  crowded    the same reads with every fourth replaced by ONE on-locus read, behind two tiles of poly-A / poly-T reads.  Poly-A
             reads alone never reach the ring (nothing of them passes the filter; their tiles overflow the regions and become
             candidates outright, tests/test_gpu_baseline_sizes.py); it is the copies that crowd the owners of that read's nine
             seeds: each of their workgroups sees ~30 k passing entries within a few microseconds, 56 blocks at once against a
             ring of 16, so blocks leave through the global list (fall-back counter > 0) and k_route_verify examines them.

Every GPU step is a child process with its own time limit; after a time-out nothing more is started."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from metamlst_amd import synth
from metamlst_amd.index import load_index  # noqa: F401  (the children load the index from the same path)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TMP = tempfile.mkdtemp(prefix="mlst_exam_")
EXAM = (1, 2, 4)
STEP_SECONDS = 300
_state = {"timed_out": None}

CHILD = r"""
import sys
import numpy as np
from metamlst_amd.engine import Engine
from metamlst_amd.index import load_index
db, inp, out = sys.argv[1:4]
idx = load_index(db)
d = np.load(inp)
eng = Engine(0)
eng.load_reference(idx)
assert eng.sieve_info()["kind"] == "routed"
eng.submit_reads(d["fb"], d["fq"], d["off"])
s = eng.stats()
full, cand = eng.debug_route_probe()
np.savez(out, sum_score=s.sum_score, n_hits=s.n_hits, locus_len_sum=s.locus_len_sum, locus_first=s.locus_first,
         counters=np.asarray(s.counters, np.uint64), cand=cand, ring_full=np.uint64(full))
"""


def _inputs():
    if "db" not in _state:
        sdb = synth.make_full_db(os.path.join(_TMP, "exam.db"), n_species=12, alleles_per_locus=60, n_profiles=20)
        sp = sorted(sdb.profiles)[0]
        g, starts = synth.make_genome(sdb, sp, sdb.profiles[sp][3], size=400_000)
        b, q = synth.sample_reads(g, 120_000)
        fb, fq, off = synth.flatten_reads(b, q)
        np.savez(os.path.join(_TMP, "ordinary.npz"), fb=fb, fq=fq, off=off)
        at = min(int(v) for v in starts.values())
        on_locus = g[at + 40:at + 190]
        assert on_locus.size == 150
        cb, cq = b.copy(), q.copy()
        cb[::4] = on_locus
        cq[::4] = 73
        poly = np.full((2048, 150), ord("A"), np.uint8)
        poly[1::2] = ord("T")
        fb, fq, off = synth.flatten_reads(np.concatenate([poly, cb]), np.concatenate([np.full((2048, 150), 73, np.uint8), cq]))
        np.savez(os.path.join(_TMP, "crowded.npz"), fb=fb, fq=fq, off=off)
        _state["db"] = sdb.path
    return _state["db"]


def _run(name, exam):
    """one submission in a child of its own, under its own time limit; a time-out ends every GPU step of this module"""
    key = (name, exam)
    if key in _state:
        return _state[key]
    if _state["timed_out"]:
        pytest.fail("not started: the GPU step %s timed out earlier" % (_state["timed_out"],))
    db = _inputs()
    out = os.path.join(_TMP, "%s_%d.npz" % (name, exam))
    env = dict(os.environ, MLST_SIEVE="routed", MLST_PROBE_EXAM_WAVES=str(exam),
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    env.pop("MLST_RT_DEBUG", None)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, db, os.path.join(_TMP, name + ".npz"), out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        _state["timed_out"] = key
        pytest.fail("GPU step %s ran longer than %d s" % (key, STEP_SECONDS))
    assert r.returncode == 0, (key, r.returncode, r.stderr[-2000:])
    _state[key] = dict(np.load(out))
    return _state[key]


def _assert_same(a, b, what):
    for k in ("cand", "counters", "sum_score", "n_hits", "locus_len_sum", "locus_first"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, a[k][:12], b[k][:12])


@pytest.mark.parametrize("exam", EXAM)
def test_ordinary_input_equals_the_separate_launch_and_never_fills_the_ring(exam):
    ref, got = _run("ordinary", 0), _run("ordinary", exam)
    print("ordinary E=%d: candidates %d parked %d ring_full %d" % (exam, got["cand"].size, int(got["counters"][7]), int(got["ring_full"])))
    assert ref["cand"].size > 500 and int(ref["counters"][7]) > 500 and int(ref["ring_full"]) == 0
    _assert_same(ref, got, ("ordinary", exam))
    assert int(got["ring_full"]) == 0


@pytest.mark.parametrize("exam", EXAM)
def test_crowded_owners_fill_the_ring_and_the_fall_back_keeps_the_result(exam):
    ref, got = _run("crowded", 0), _run("crowded", exam)
    print("crowded E=%d: candidates %d parked %d ring_full %d" % (exam, got["cand"].size, int(got["counters"][7]), int(got["ring_full"])))
    assert ref["cand"].size > 30_000 and int(ref["ring_full"]) == 0      # (no ring at 0: nothing to fall back from)
    _assert_same(ref, got, ("crowded", exam))
    assert int(got["ring_full"]) > 0
