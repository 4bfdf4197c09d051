"""Every words-per-read instantiation of the three sieves, seed by seed: the one-seed corpus of tests/sieve_cases.py on the GPU,
held against the plain model of tests/sieve_model.py (which tests/test_sieve_model.py ties to the oracle) and the oracle itself.

For every row width W = 2 .. 20 and each of the LDS, the global and the routed sieve (the routed one also with 8-wave producer
workgroups, MLST_ROUTE_WAVES=8, and without examiner waves, MLST_PROBE_EXAM_WAVES=0), on a mixed submission (the masked path)
and on one whose reads all hold NT = W - 1 seeds (the all_full path), and on one paired submission at W = 8:

  1. no seed is lost        the candidate list (mlst_debug_route_probe copies d_cand whichever sieve ran; one submission per
                            sample, so the counter is the submission's own) holds every read the model requires -- a read with
                            ONE database seed at a chosen slot of a chosen row width, at chosen lanes, groups and tiles
  2. nothing unexplained    candidates outside `may` (the reads whose packed row shows a database seed; mates with them) are
                            fingerprint false positives: with S seeds that are not in K, at most eight of 65,535 non-zero
                            fingerprints per bucket and at most chain + 1 buckets per probe, their mean is below
                            S * 8 * (chain + 1) / 65535 (far below: the first level comes first); the cap is twice that plus 4,
                            the spread of a count whose mean is below ~15.  A tile that became candidates outright (an
                            overflowing region) would break it: random backgrounds do not overflow.  They did: the cases
                            routed / routed_exam0 W = 2, 4 (mixed and full) and 6 (full) and routed_waves8 W = 2, 4 found every
                            full tile of narrow rows unrouted -- 3,400 candidates of 3,400 reads -- because k_route's sort
                            buffer and regions had room for the few dummy entries of 150-base reads only ("Narrow
                            rows"; fixed in k_route's SCAP and ensure_route_buffers)
  3. pass 1 = the oracle    sums, hits, lengths, first reads, counters and the sorted item list, bit for bit: k_seed, k_retain,
                            both forms of k_ext_prep / k_extend and k_accumulate under every row width
  4. the text path          the same reads as FASTQ text (k_pack_text with that row width): the width the engine chose is W,
                            statistics and items are the same

One child process per sieve configuration (the switches are read when the reference is loaded) with its own time limit runs
every submission on one engine; after a time-out nothing more is started.  The model's and the oracle's answers are computed
once per submission."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fixtures as fx
import oracle_lib
import sieve_cases as sc
import sieve_model as sm
from metamlst_amd.engine import MLST_CNT_N
from metamlst_amd.typing import SampleStats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TMP = tempfile.mkdtemp(prefix="mlst_words_")
STEP_SECONDS = 300
CAP = 1 << 13
# configuration -> (environment, the sieve the child must find)
CONFIGS = {
    "lds": ({"MLST_SIEVE": "lds"}, "lds"),
    "global": ({"MLST_SIEVE": "global"}, "global"),
    "routed": ({"MLST_SIEVE": "routed"}, "routed"),
    "routed_waves8": ({"MLST_SIEVE": "routed", "MLST_ROUTE_WAVES": "8"}, "routed"),
    "routed_exam0": ({"MLST_SIEVE": "routed", "MLST_PROBE_EXAM_WAVES": "0"}, "routed"),
}
SWITCHES = ("MLST_SIEVE", "MLST_ROUTE_WRITEOUT", "MLST_ROUTE_BLOCKS", "MLST_ROUTE_WAVES", "MLST_PROBE_EXAM_WAVES", "MLST_RT_DEBUG",
            "MLST_GBM_BITS", "MLST_SIEVE_BLOCKS")
STATS = ("sum_score", "n_hits", "locus_len_sum", "locus_first", "counters")
_state = {"timed_out": None}

CHILD = r"""
import sys
import numpy as np
from metamlst_amd.engine import Engine
from metamlst_amd.index import load_index
db, kind, tmp, tag, cap = sys.argv[1:6]
eng = Engine(0)
eng.load_reference(load_index(db, cache=False))
info = eng.sieve_info()
assert info["kind"] == kind, info
out = {"n_seeds": np.uint64(info["n_seeds"]), "chain": np.uint64(info["longest_chain"])}
for name in sys.argv[6:]:
    d = np.load(tmp + "/" + name + ".npz")
    paired = bool(d["paired"])
    for path in ("reads", "text"):
        eng.reset_sample()
        if path == "reads":
            eng.submit_reads(d["fb"], d["fq"], d["off"], paired=paired)
        else:
            assert eng.submit_fastq(d["text"], paired=paired) == len(d["off"]) - 1
        s = eng.stats()
        pre = name + "/" + path + "/"
        for k in ("sum_score", "n_hits", "locus_len_sum", "locus_first"):
            out[pre + k] = getattr(s, k)
        out[pre + "counters"] = np.asarray(s.counters, np.uint64)
        out[pre + "items"] = eng.items(int(cap))
        out[pre + "cand"] = eng.debug_route_probe()[1]
        if path == "text":
            out[pre + "wpr"] = np.uint64(eng.debug_last_packed()[3])
eng.close()
np.savez(tmp + "/" + tag + ".npz", **out)
"""


def _name(W, kind):
    return "w%02d_%s" % (W, kind)


def _inputs():
    if "db" not in _state:
        for W, kind in sc.all_submissions():
            sub = sc.submission(W, kind)
            np.savez(os.path.join(_TMP, _name(W, kind) + ".npz"), fb=sub.fb, fq=sub.fq, off=sub.off, paired=sub.paired,
                     text=np.frombuffer(sub.text(), np.uint8))
        _state["db"] = sc.database().path
    return _state["db"]


def _run(config):
    """every submission under one sieve configuration, in a child of its own under its own time limit; a time-out ends every GPU
    step of this module"""
    if config in _state:
        return _state[config]
    if _state["timed_out"]:
        pytest.fail("not started: the GPU step %s timed out earlier" % (_state["timed_out"],))
    db = _inputs()
    cenv, kind = CONFIGS[config]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(cenv)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])
    names = [_name(W, k) for W, k in sc.all_submissions()]
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, db, kind, _TMP, config, str(CAP)] + names, env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        _state["timed_out"] = config
        pytest.fail("GPU step %s ran longer than %d s" % (config, STEP_SECONDS))
    assert r.returncode == 0, (config, r.returncode, r.stderr[-2000:])
    _state[config] = dict(np.load(os.path.join(_TMP, config + ".npz")))
    return _state[config]


@functools.lru_cache(maxsize=None)
def oracle_says(W, kind):
    """The specification's statistics and sorted items for a submission, computed once and shared."""
    sub = sc.submission(W, kind)
    orc = oracle_lib.Oracle(sc.database().idx)
    orc.submit_reads(sub.fb, sub.fq, sub.off, paired=sub.paired)
    so, items = orc.stats(want_items=CAP)
    assert len(items) < CAP
    return so, fx.sorted_items(items)


def _stats_of(got, pre):
    return SampleStats(*(got[pre + k] for k in STATS[:4]), got[pre + "counters"][:MLST_CNT_N])


def cap_of(sub, chain):
    """Most candidates that nothing explains (point 2 of the module's text)."""
    return 2.0 * sub.foreign * 8 * (chain + 1) / 65535.0 + 4.0


def check_candidates(config, W, kind, got):
    sub = sc.submission(W, kind)
    cand = got[_name(W, kind) + "/reads/cand"].astype(np.int64)
    assert cand.size == np.unique(cand).size and (cand.size == 0 or int(cand.max()) < len(sub.reads)), "not a set of read indices"
    is_cand = np.zeros(len(sub.reads), bool)
    is_cand[cand] = True
    unexplained = int((is_cand & ~sub.may).sum())
    cap = cap_of(sub, int(got["chain"]))
    planted = sum(r.what == "planted" for r in sub.reads)
    print("sieve words: %s W=%d %s: reads %d, planted %d, required %d, candidates %d, unexplained %d (cap %.1f, S = %d, chain %d)"
          % (config, W, kind, len(sub.reads), planted, int(sub.must.sum()), cand.size, unexplained, cap, sub.foreign, int(got["chain"])))
    lost = np.nonzero(sub.must & ~is_cand)[0]
    assert lost.size == 0, "%s: %d required reads are no candidates; (W, length, slot, strand, lane, group, tile), what: %s" % (
        config, lost.size, [(sub.where(i), sub.reads[i].what, sub.reads[i].key) for i in lost[:24]])
    assert unexplained <= cap, "%s W=%d %s: %d candidates that no seed explains, cap %.1f: %s" % (
        config, W, kind, unexplained, cap, [(sub.where(i), sub.reads[i].what) for i in np.nonzero(is_cand & ~sub.may)[0][:24]])
    assert np.array_equal(np.sort(got[_name(W, kind) + "/text/cand"].astype(np.int64)), np.sort(cand)), "the text path's candidates differ"


def check_pass1(W, kind, got):
    so, items_o = oracle_says(W, kind)
    for path in ("reads", "text"):
        pre = _name(W, kind) + "/" + path + "/"
        try:
            fx.assert_stats_equal(_stats_of(got, pre), so)
            assert np.array_equal(fx.sorted_items(got[pre + "items"]), items_o), "items differ"
        except AssertionError as e:
            raise AssertionError("W=%d %s, %s path: %s" % (W, kind, path, str(e)[:600])) from None
    assert int(so.n_hits.sum()) > 0 or W == 2                         # (a 32-base read scores at most 64: few records under the narrowest row)
    assert int(got[_name(W, kind) + "/text/wpr"]) == W, "the engine packed the text into rows of another width"


@pytest.mark.parametrize("W", sc.WIDTHS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_no_seed_is_lost_and_nothing_unexplained_is_kept(config, W):
    got = _run(config)
    assert int(got["n_seeds"]) == sm.n_canonical(sc.database().model.K), "the model and the builder disagree on K"
    for kind in ("mixed", "full"):
        check_candidates(config, W, kind, got)


@pytest.mark.parametrize("W", sc.WIDTHS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_pass_one_under_every_width_equals_the_oracle(config, W):
    got = _run(config)
    for kind in ("mixed", "full"):
        check_pass1(W, kind, got)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_paired_submission_keeps_the_mates_of_planted_reads(config):
    got = _run(config)
    sub = sc.submission(8, "paired")
    assert sub.paired and int(sub.must.sum()) > int(sc.submission(8, "mixed").must.sum())      # mates are required with their planted reads
    check_candidates(config, 8, "paired", got)
    check_pass1(8, "paired", got)
