"""The write-out of the routed sieve's producer (k_route, MLST_ROUTE_WRITEOUT): with every owner's segment placed in LDS at
an index congruent to the owner's carry count modulo four and read back 16 bytes per lane (the default), the candidate list,
the counters and the per-allele statistics equal those of the write-out of rounds 2-6 (the switch at 0), and the per-allele
statistics equal those of the LDS sieve, which shares none of the routed code (its candidate list may differ: not compared).

Inputs on a database forced onto the routed sieve, the smallest at which the write-out can go wrong:
  n1 .. n3000  tile edges: 1, 63, 1,024, 1,025 and 3,000 reads of one isolate; the last tile is partly empty
  big          120,000 reads, also with one and with two producer workgroups (MLST_ROUTE_BLOCKS): every owner's carry lives
               through 60-120 tiles and takes every length from 0 to 15; the two-workgroup case again with 8-wave workgroups
  ragged       reads cut to lengths spread over 0 .. 150, some under 20 bases (no seed): lanes and whole runs without a
               seed, and the dummy entries they produce
  crowded      the input of tests/test_gpu_probe_examiners.py: two poly-A / poly-T tiles that overflow their regions (the
               tile is not routed, its reads become candidates) in front of reads of which every fourth is ONE on-locus
               read -- the owners of its nine seeds receive streams of several hundred entries per tile, more than one
               pass of the write-out

Every GPU step is a child process with its own time limit; after a time-out nothing more is started."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from metamlst_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TMP = tempfile.mkdtemp(prefix="mlst_wo_")
STEP_SECONDS = 300
EDGES = ("n1", "n63", "n1024", "n1025", "n3000")
# group of inputs that one child process submits (an engine each) -> (inputs, environment on top of the mode's)
GROUPS = {
    "edges": (EDGES + ("ragged",), {}),
    "big": (("big",), {}),
    "crowded": (("crowded",), {}),
    "big_b1": (("big",), {"MLST_ROUTE_BLOCKS": "1"}),
    "big_b2": (("big",), {"MLST_ROUTE_BLOCKS": "2"}),
    "big_b2w8": (("big",), {"MLST_ROUTE_BLOCKS": "2", "MLST_ROUTE_WAVES": "8"}),
}
# mode -> (environment, sieve the child must find)
MODES = {
    "new": ({"MLST_SIEVE": "routed"}, "routed"),
    "old": ({"MLST_SIEVE": "routed", "MLST_ROUTE_WRITEOUT": "0"}, "routed"),
    "lds": ({}, "lds"),
}
STATS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")
_state = {"timed_out": None}

CHILD = r"""
import sys
import numpy as np
from metamlst_amd.engine import Engine
from metamlst_amd.index import load_index
db, kind, tmp, tag = sys.argv[1:5]
idx = load_index(db)
for name in sys.argv[5:]:
    d = np.load(tmp + "/" + name + ".npz")
    eng = Engine(0)
    eng.load_reference(idx)
    assert eng.sieve_info()["kind"] == kind, eng.sieve_info()
    eng.submit_reads(d["fb"], d["fq"], d["off"])
    s = eng.stats()
    cand = eng.debug_route_probe()[1] if kind == "routed" else np.zeros(0, np.uint32)
    np.savez(tmp + "/" + tag + "_" + name + ".npz", sum_score=s.sum_score, n_hits=s.n_hits, locus_len_sum=s.locus_len_sum,
             locus_first=s.locus_first, counters=np.asarray(s.counters, np.uint64), cand=cand)
    del eng
"""


def _inputs():
    if "db" not in _state:
        sdb = synth.make_full_db(os.path.join(_TMP, "wo.db"), n_species=12, alleles_per_locus=60, n_profiles=20)
        sp = sorted(sdb.profiles)[0]
        g, starts = synth.make_genome(sdb, sp, sdb.profiles[sp][3], size=400_000)
        b, q = synth.sample_reads(g, 120_000)

        def save(name, bb, qq):
            fb, fq, off = synth.flatten_reads(bb, qq)
            np.savez(os.path.join(_TMP, name + ".npz"), fb=fb, fq=fq, off=off)

        save("big", b, q)
        for name in EDGES:
            n = int(name[1:])
            save(name, b[:n], q[:n])
        # ragged: the first 30,000 reads cut to lengths 0 .. 150 (the first few fixed: none, one base, one short of a seed, exactly a seed, whole)
        rb, rq = b[:30_000], q[:30_000]
        lens = np.random.default_rng(7).integers(0, 151, size=rb.shape[0])
        lens[:5] = (0, 1, 19, 20, 150)
        assert int((lens < 20).sum()) > 1000 and int(lens.max()) == 150
        keep = np.arange(150)[None, :] < lens[:, None]
        off = np.zeros(rb.shape[0] + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        np.savez(os.path.join(_TMP, "ragged.npz"), fb=rb[keep], fq=rq[keep], off=off)
        # crowded (tests/test_gpu_probe_examiners.py)
        at = min(int(v) for v in starts.values())
        on_locus = g[at + 40:at + 190]
        assert on_locus.size == 150
        cb, cq = b.copy(), q.copy()
        cb[::4] = on_locus
        cq[::4] = 73
        poly = np.full((2048, 150), ord("A"), np.uint8)
        poly[1::2] = ord("T")
        save("crowded", np.concatenate([poly, cb]), np.concatenate([np.full((2048, 150), 73, np.uint8), cq]))
        _state["db"] = sdb.path
    return _state["db"]


def _run(group, mode):
    """the submissions of one group in a child of its own, under its own time limit; a time-out ends every GPU step of this module"""
    key = (group, mode)
    if key in _state:
        return _state[key]
    if _state["timed_out"]:
        pytest.fail("not started: the GPU step %s timed out earlier" % (_state["timed_out"],))
    db = _inputs()
    names, genv = GROUPS[group]
    menv, kind = MODES[mode]
    env = {k: v for k, v in os.environ.items() if k not in ("MLST_SIEVE", "MLST_ROUTE_WRITEOUT", "MLST_ROUTE_BLOCKS", "MLST_ROUTE_WAVES", "MLST_RT_DEBUG")}
    env.update(menv)
    env.update(genv)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])
    tag = "%s_%s" % (group, mode)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, db, kind, _TMP, tag] + list(names), env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        _state["timed_out"] = key
        pytest.fail("GPU step %s ran longer than %d s" % (key, STEP_SECONDS))
    assert r.returncode == 0, (key, r.returncode, r.stderr[-2000:])
    _state[key] = {n: dict(np.load(os.path.join(_TMP, "%s_%s.npz" % (tag, n)))) for n in names}
    return _state[key]


def _assert_same(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, a[k][:12], b[k][:12])


def _check(group, name, lds_group):
    new, old, lds = _run(group, "new")[name], _run(group, "old")[name], _run(lds_group, "lds")[name]
    print("%s/%s: candidates %d (switch at 0: %d), hits %d, parked %d" % (group, name, new["cand"].size, old["cand"].size,
                                                                          int(new["n_hits"].sum()), int(new["counters"][7])))
    _assert_same(old, new, ("cand", "counters") + STATS, (group, name, "write-out 0 / default"))
    _assert_same(lds, new, STATS, (group, name, "LDS sieve / routed"))
    return new


@pytest.mark.parametrize("name", EDGES)
def test_tile_edges(name):
    got = _check("edges", name, "edges")
    if int(name[1:]) >= 1024:
        assert got["cand"].size > 0 and int(got["n_hits"].sum()) > 0


@pytest.mark.parametrize("group", ("big", "big_b1", "big_b2", "big_b2w8"))
def test_carry_over_many_tiles(group):
    got = _check(group, "big", "big")
    assert got["cand"].size > 500 and int(got["counters"][7]) > 500
    _assert_same(_run("big", "new")["big"], got, ("cand",) + STATS, (group, "any number of producer workgroups"))


def test_mixed_read_lengths():
    got = _check("edges", "ragged", "edges")
    assert got["cand"].size > 50 and int(got["n_hits"].sum()) > 0


def test_crowded_owners_and_overflowing_tiles():
    got = _check("crowded", "crowded", "crowded")
    cand = got["cand"]
    # the two poly-A / poly-T tiles are not routed: all their reads are candidates; the copies behind them are routed and found
    assert int((cand < 2048).sum()) == 2048 and int((cand >= 2048).sum()) > 30_000
