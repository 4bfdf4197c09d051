"""The crafted alignment cases (tests/align_cases.py) on the CPU: every case's predicted path is confirmed by the oracle, and a
plain Python restatement of the ungapped alignment and of the gap trigger (written from DESIGN section 2 and
include/mlst_policy.h) equals the oracle on the pairs of the corpus."""
import functools

import numpy as np
import pytest

import align_cases as ac
import oracle_lib
from metamlst_amd.engine import default_params

P0, SHIFT = 0x7FFF, 16                 # MLST_P0, MLST_P_SHIFT
CODE = {c: k for k, c in enumerate(b"ACGT")}
CODE.update({c: k for k, c in enumerate(b"acgt")})


@functools.lru_cache(maxsize=None)
def world():
    cp = ac.corpus()
    return cp, oracle_lib.Oracle(cp.idx)


@functools.lru_cache(maxsize=None)
def case_facts(name):
    """What the oracle says of one case on its own: (items, counters)."""
    cp, orc = world()
    c = next(c for c in cp.cases if c.name == name)
    fb, fq, off, _ = cp.layout([c], lanes=False)
    orc.submit_reads(fb, fq, off)
    s, items = orc.stats(want_items=32)
    return items, s.counters.copy()


# ---------------------------------------------------------------------------------------------------------------------
# The restatement: Python integers, one column at a time.

def oriented(bases: bytes, quals: bytes, strand: int):
    """Codes (0..3, 4 = anything else) and Phred of the read in the orientation of the allele."""
    code = [CODE.get(c, 4) for c in bases]
    ph = [max(0, q - 33) for q in quals]
    if strand:
        code = [3 - c if c < 4 else 4 for c in reversed(code)]
        ph = ph[::-1]
    return code, ph


def restated(bases, quals, allele_seq: bytes, strand: int, diag: int, p):
    """Ungapped local alignment of the read on diagonal `diag` (allele column = read column + diag) on the packed value
    (score << 16) | (127 - xo) << 8 | (255 - xm), and the gap-trigger decision."""
    code, ph = oriented(bases, quals, strand)
    n, m = len(code), len(allele_seq)
    run = best = P0
    start, first, last = 0, -1, -1
    mm_total = overlap = 0
    for i in range(n):
        j = i + diag
        if j < 0 or j >= m:
            continue
        if overlap == 0:
            start = i
        overlap += 1
        a = CODE.get(allele_seq[j], 4)
        if code[i] < 4 and a < 4 and code[i] == a:
            run += p.match_bonus << SHIFT
        else:
            pen = p.n_penalty if (code[i] > 3 or a > 3) else p.mm_min + (p.mm_max - p.mm_min) * min(ph[i], 40) // 40
            run -= (pen << SHIFT) + 1              # the xm field counts down
            mm_total += 1
        if run <= P0:                               # nothing worth keeping: the next column starts from the empty alignment
            run, start = P0, i + 1
        elif run > best:                            # the first column that reaches the maximum ends the alignment
            best, first, last = run, start, i
    score, xm = best >> SHIFT, P0 - (best & 0xFFFF)
    floor_n = int(p.minscore_const + p.minscore_coef * np.log(n))
    clipped = overlap - (last - first + 1 if last >= 0 else 0)
    if p.gap_trigger_mm < 0:
        trigger = True
    else:
        trigger = mm_total > p.gap_trigger_mm and score >= floor_n and clipped >= p.gap_trigger_clip and 2 * (mm_total - xm) >= clipped
    return dict(score=score, xm=xm, mm_total=mm_total, first=first, last=last, trigger=int(trigger))


ALL_ALLELES = ("mm_over_255", "gap_trigger", "block_phase")


@pytest.mark.parametrize("group", ac.GROUPS)
def test_python_restatement_equals_the_oracle(group):
    cp, orc = world()
    p = default_params()
    idx = cp.idx
    bad, n_pairs = [], 0
    for c in cp.of(group):
        items, _ = case_facts(c.name)
        fl = ac.floor_score(len(c.bases))
        for _, locus, strand, diag, _ in items.tolist():
            for a in range(int(idx.locus_begin[locus]), int(idx.locus_begin[locus] + idx.locus_count[locus])):
                pol = orc.align_one(c.bases, c.quals, a, strand, diag, mode=0)
                if group not in ALL_ALLELES and not (pol["score"] >= fl and pol["score"] > 0):
                    continue
                ung = orc.align_one(c.bases, c.quals, a, strand, diag, mode=1)
                r = restated(c.bases, c.quals, cp.seq(a), strand, diag, p)
                want = dict(score=ung["score"], xm=ung["xm"], mm_total=ung["mm_total"],
                            first=ung["cols"][0][0] if ung["cols"] else -1, last=ung["cols"][-1][0] if ung["cols"] else -1, trigger=pol["used_dp"])
                n_pairs += 1
                if r != want:
                    bad.append((c.name, a, strand, diag, r, want))
    assert not bad, "%d of %d pairs differ, first: %s" % (len(bad), n_pairs, bad[:3])
    assert n_pairs > 0


# ---------------------------------------------------------------------------------------------------------------------
# Predicted paths.

def prediction_failures(c, orc, idx):
    e, out = c.expect, []
    items, cnt = case_facts(c.name)
    n, fl = len(c.bases), ac.floor_score(len(c.bases))
    if "items" in e and len(items) != e["items"]:
        out.append("items %d, predicted %d" % (len(items), e["items"]))
    if "records" in e and int(cnt[0]) != e["records"]:
        out.append("records %d, predicted %d" % (int(cnt[0]), e["records"]))
    if "q1" in e and (int(cnt[0]) == 1) != e["q1"]:
        out.append("records %d, predicted q1=%s" % (int(cnt[0]), e["q1"]))
    if "dp_pairs" in e and int(cnt[6]) != e["dp_pairs"]:
        out.append("DP_PAIRS %d, predicted %d" % (int(cnt[6]), e["dp_pairs"]))
    for k, pr in enumerate(e.get("pairs", ())):
        locus = int(idx.locus_id[pr["allele"]])
        it = [x for x in items.tolist() if x[1] == locus and x[2] == pr["strand"]]
        if len(it) != 1:
            out.append("pair %d: %d items on locus %d strand %d" % (k, len(it), locus, pr["strand"]))
            continue
        if it[0][3] != pr["diag"]:
            out.append("pair %d: item on diagonal %d, predicted %d" % (k, it[0][3], pr["diag"]))
            continue
        if "votes" in e and k == 0 and it[0][4] != e["votes"]:
            out.append("votes %d, predicted %d" % (it[0][4], e["votes"]))
        pol = orc.align_one(c.bases, c.quals, pr["allele"], pr["strand"], pr["diag"], mode=0)
        for key in ("score", "xm", "xo", "mm_total", "used_dp"):
            if key in pr and pol[key] != pr[key]:
                out.append("pair %d: %s %d, predicted %d" % (k, key, pol[key], pr[key]))
        if "record" in pr and (pol["score"] >= fl and pol["score"] > 0) != pr["record"]:
            out.append("pair %d: score %d against floor %d, predicted record=%s" % (k, pol["score"], fl, pr["record"]))
        if "ungapped_score" in pr:
            u = orc.align_one(c.bases, c.quals, pr["allele"], pr["strand"], pr["diag"], mode=1)["score"]
            if u != pr["ungapped_score"]:
                out.append("pair %d: ungapped score %d, predicted %d" % (k, u, pr["ungapped_score"]))
    return out


@pytest.mark.parametrize("group", ac.GROUPS)
def test_every_predicted_path_is_confirmed_by_the_oracle(group):
    cp, orc = world()
    bad = {}
    for c in cp.of(group):
        f = prediction_failures(c, orc, cp.idx)
        if f:
            bad[c.name] = f
    assert not bad, "%d cases: %s" % (len(bad), list(bad.items())[:5])


def test_the_corpus_reaches_the_edges_it_names():
    """The corpus-wide properties of the issue: every block-origin of the list, mismatch counts on both sides of 255, both
    outcomes of the trigger, reads with 0 / 1 / 2 records, the allele counts around the wave size."""
    cp, orc = world()
    diags = {pr["diag"] for c in cp.cases if c.group == "overhang_start" for pr in c.expect["pairs"]}
    assert {-1, -31, -32, -33, -64, -65} <= diags
    assert cp.groups() == list(ac.GROUPS)
    assert set(range(32)) == {pr["diag"] % 32 for c in cp.of("block_phase") for pr in c.expect["pairs"] if "perfect" in c.name}
    for strand in (0, 1):                                  # both strands at the phases next to a block edge
        assert {0, 1, 31} <= {pr["diag"] % 32 for c in cp.of("block_phase") for pr in c.expect["pairs"] if "perfect" in c.name and pr["strand"] == strand}
    assert sum("dp_pairs" in c.expect for c in cp.cases) > 1000 and {c.expect.get("dp_pairs") for c in cp.cases} >= {0, 1}
    mm = {pr["mm_total"] for c in cp.of("mm_over_255") for pr in c.expect["pairs"]}
    assert {250, 255, 256, 257, 272} <= mm
    fired = {pr["used_dp"] for c in cp.of("gap_trigger") for pr in c.expect["pairs"] if "used_dp" in pr}
    assert fired == {0, 1}
    recs = {int(case_facts(c.name)[1][0]) for c in cp.of("q1_records")}
    assert {0, 1, 2} <= recs
    assert {int(x) for x in cp.idx.locus_count} >= {1, 2, 63, 64, 65, 127, 128, 129, 256, 257}
    assert 1000 < len(cp.cases) < 5000
    assert len({c.name for c in cp.cases}) == len(cp.cases)


def test_banded_between_ungapped_and_exhaustive_on_the_gap_trigger_group():
    cp, orc = world()
    cases = cp.of("gap_trigger")
    fb, fq, off, _ = cp.layout(cases, lanes=False)
    orc.submit_reads(fb, fq, off)
    ex = orc.exhaustive()[0]
    n = 0
    for k, c in enumerate(cases):
        items, _ = case_facts(c.name)
        for _, locus, strand, diag, _ in items.tolist():
            for a in range(int(cp.idx.locus_begin[locus]), int(cp.idx.locus_begin[locus] + cp.idx.locus_count[locus])):
                u = orc.align_one(c.bases, c.quals, a, strand, diag, mode=1)["score"]
                g = orc.align_one(c.bases, c.quals, a, strand, diag, mode=2)["score"]
                assert u <= g <= int(ex[k, a]), (c.name, a, u, g, int(ex[k, a]))
                n += 1
    assert n >= 12 * len(cases)             # (the smallest locus of the group has 12 alleles)


def path_counts(cp, orc, p=None):
    """Per group, from the oracle: cases, items, (item, allele) pairs, pairs with a record, pairs whose aligned span is walked
    (mm_total above the trigger and a score at the floor), pairs the banded Smith-Waterman takes, items the fast pass settles,
    items left to the pair-by-pair pass (a tracked pair) and items left to k_accumulate because they hold exactly one record."""
    p = p or default_params()
    idx, rows = cp.idx, {}
    for g in cp.groups():
        r = dict(cases=0, items=0, pairs=0, records=0, walked=0, banded=0, fast=0, slow=0, single=0)
        for c in cp.of(g):
            r["cases"] += 1
            items, _ = case_facts(c.name)
            fl = ac.floor_score(len(c.bases))
            for _, locus, strand, diag, _ in items.tolist():
                rec = trk = 0
                for a in range(int(idx.locus_begin[locus]), int(idx.locus_begin[locus] + idx.locus_count[locus])):
                    pol = orc.align_one(c.bases, c.quals, a, strand, diag, mode=0)
                    ung = orc.align_one(c.bases, c.quals, a, strand, diag, mode=1)
                    r["pairs"] += 1
                    rec += pol["score"] >= fl and pol["score"] > 0
                    r["walked"] += ung["mm_total"] > p.gap_trigger_mm and ung["score"] >= fl
                    trk += pol["used_dp"]
                r["items"] += 1; r["records"] += rec; r["banded"] += trk
                r["slow" if trk else "single" if (p.xm_field_quirk and rec == 1) else "fast"] += 1
        rows[g] = r
    return rows


if __name__ == "__main__":
    cp_, orc_ = world()
    keys = ("cases", "items", "pairs", "records", "walked", "banded", "fast", "slow", "single")
    print("| group | " + " | ".join(keys) + " |")
    print("|---|" + "---|" * len(keys))
    tot = dict.fromkeys(keys, 0)
    for g_, r_ in path_counts(cp_, orc_).items():
        print("| `%s` | " % g_ + " | ".join(str(r_[k]) for k in keys) + " |")
        for k in keys:
            tot[k] += r_[k]
    print("| all | " + " | ".join(str(tot[k]) for k in keys) + " |")
