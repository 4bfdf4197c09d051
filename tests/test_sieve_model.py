"""The plain model of the sieve's contract (tests/sieve_model.py) against the specification -- no GPU.

`must(read)` -- some slot's window has no N and is a database seed with at most 16 postings -- has to say exactly what the
oracle says by reporting at least one work item for the read: over the crafted alignment corpus (tests/align_cases.py) and
over every submission of the one-seed corpus (tests/sieve_cases.py), read by read.  That ties the model the GPU tests hold
the candidate lists against (tests/test_gpu_sieve_words.py) to DESIGN section 2, not to the engine."""
import functools

import numpy as np
import pytest

import align_cases as ac
import oracle_lib
import sieve_cases as sc
import sieve_model as sm


def reads_with_items(idx, fb, fq, off) -> np.ndarray:
    orc = oracle_lib.Oracle(idx)
    orc.submit_reads(fb, fq, off)
    _, items = orc.stats(want_items=1 << 16)
    assert len(items) < 1 << 16
    has = np.zeros(len(off) - 1, bool)
    has[items[:, 0]] = True
    return has


def test_slots_hand_worked():
    assert sm.slots(19) == [] and sm.slots(0) == []
    assert sm.slots(20) == [0] and sm.slots(35) == [0]              # the second seed would end on base 36
    assert sm.slots(36) == [0, 16] and sm.slots(37) == [0, 16]
    assert sm.slots(320) == [16 * t for t in range(19)] and sm.slots(320)[-1] + 20 == 320 - 12
    assert [len(sm.slots(16 * W)) for W in sc.WIDTHS] == [W - 1 for W in sc.WIDTHS]      # a full row holds NT = W - 1 seeds
    assert [len(sm.slots(16 * W - 12)) for W in sc.WIDTHS] == [W - 1 for W in sc.WIDTHS]  # .. from 16 (W - 2) + 20 bases on
    assert [len(sm.slots(16 * W - 13)) for W in sc.WIDTHS] == [W - 2 for W in sc.WIDTHS]


def test_the_model_handles_n_and_case_as_stated():
    db = sc.database()
    k = db.keys[0]
    m = db.model
    assert m.must(k) and m.must(k.lower()) and m.may(k) and not m.must(k[:19])
    i = next(i for i in range(20) if k[i] != ord("A"))
    assert not m.must(k[:i] + b"N" + k[i + 1:])
    if ord("A") in k:
        j = k.index(b"A")
        held = k[:j] + b"N" + k[j + 1:]
        assert not m.must(held) and m.may(held)                     # the packed row holds the key itself
        flagged = [t == j for t in range(20)]                       # the same said with the packed row's N bit
        assert not m.must(k, nmask=flagged) and m.may(k, nmask=flagged)
    assert not m.must(db.y17) and not m.may(db.y17) and m.must(db.x16) and m.must(db.palindrome)


@functools.lru_cache(maxsize=None)
def _align_corpus():
    cp = ac.corpus()
    fb, fq, off, _ = cp.layout(list(cp.cases), lanes=False)
    return cp, sm.Model(cp.idx), sm.split(fb, off), reads_with_items(cp.idx, fb, fq, off)


def test_must_equals_the_oracle_has_an_item_on_the_alignment_corpus():
    cp, model, reads, has = _align_corpus()
    must = np.array([model.must(r) for r in reads])
    bad = np.nonzero(must != has)[0]
    assert bad.size == 0, [(cp.cases[i].name, bool(must[i]), bool(has[i])) for i in bad[:10]]
    assert int(has.sum()) > 1000 and int((~has).sum()) >= 6        # both answers occur (too short, off the end, 17 postings)


def test_the_model_counts_the_keys_the_oracle_builds():
    for idx, model in ((ac.corpus().idx, _align_corpus()[1]), (sc.database().idx, sc.database().model)):
        assert len(model.K) == oracle_lib.Oracle(idx).n_keys()      # (the oracle, too, keeps both orientations)
    K = sc.database().model.K                                      # canonical keys: a pair counts once, the palindrome is its own pair
    assert sm.n_canonical(K) == (len(K) + sum(w == sm.revcomp(w) for w in K)) // 2 and sc.database().palindrome in K


@pytest.mark.parametrize("W,kind", sc.all_submissions(), ids=lambda v: str(v))
def test_must_equals_the_oracle_has_an_item_on_the_one_seed_corpus(W, kind):
    sub = sc.submission(W, kind)
    has = reads_with_items(sc.database().idx, sub.fb, sub.fq, sub.off)
    own = np.array([sc.database().model.must(r.bases) for r in sub.reads])      # (without the mates of a paired submission)
    bad = np.nonzero(own != has)[0]
    assert bad.size == 0, [(sub.where(i), sub.reads[i].what, bool(own[i]), bool(has[i])) for i in bad[:10]]
    # what the submission is for: every slot of the row width planted on both strands, in a row of that width
    n_full = 16 * W
    slots_planted = {(r.slot, r.strand) for r in sub.reads if r.what == "planted" and len(r.bases) == n_full}
    assert slots_planted == {(t, s) for t in range(W - 1) for s in (0, 1)}
    assert len(sub.reads) == sc.N_READS and sc.wpr_of(max(len(r.bases) for r in sub.reads)) == W
    if kind == "full":
        assert all(len(sm.slots(len(r.bases))) >= W - 1 for r in sub.reads)
    else:
        assert any(len(sm.slots(len(r.bases))) < W - 1 for r in sub.reads)
