"""mlst_set_read_adapters (csrc/read_adapt.h): 3' adapters removed on the device before the reads are packed.  The yardstick is that of
test_gpu_read_prep.py: the engine with the switch ON and the RAW text must leave what the same engine leaves with the switch OFF and
the text fastq.trim_adapters(fastq.prep_fastq(...)) writes -- the packed rows byte for byte (mlst_debug_last_packed), the typed
statistics, the counters -- through every entry that takes FASTQ text; then the exports, the refusals and the life cycle, and
`cli type --adapter`.  adapter_cut itself is pinned by hand in test_read_adapters_host.py.  The rule is the project's own (modelled on
`cutadapt -a ADAPTER --no-indels`); nothing here claims cutadapt's bytes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import read_names_cases as rc
import test_gpu_read_prep as rp
from metamlst_amd import cli
from metamlst_amd.engine import Engine, MlstError, default_params
from metamlst_amd.fastq import ADAPTER_NAMES, adapter_cut, prep_fastq, trim_adapters
from test_gpu_bam_reads import assert_typed_equal, typed
from test_gpu_pair_bgzf import bgzf_blocks
from test_gpu_sam_all import assert_rule_bytes, export
from test_read_adapters_host import KNOWN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A = ADAPTER_NAMES["illumina"]                              # 13 letters
T33 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"                  # 33: it begins with A -- a tie between two adapters wherever fewer than 14 letters overlap
X32 = "CTGTCTCTTATACACATCTCCGAGCCCACGAGAC"[:32]            # 32
AN = "AGATCGNAAGAGC"                                       # an adapter N


def letters(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


_rng = np.random.default_rng(64)
R64 = letters(_rng, 64).decode()                           # 64
R63 = letters(_rng, 63).decode()                           # 63
_n40 = bytearray(letters(_rng, 40))
N40_PLAIN = bytes(_n40).decode()                           # what a read carries
for _at in (5, 20, 33, 36, 38):
    _n40[_at] = ord("N")
N40 = bytes(_n40).decode()                                 # 40 letters with Ns in both 32-letter words
OFF = {"adapters": [], "min_overlap": 0, "error_permille": 0}
SETTINGS = [{"adapters": [A]},
            {"adapters": [A, T33, X32, ADAPTER_NAMES["nextera"]]},
            {"adapters": [R64, R63], "min_overlap": 5},
            {"adapters": ["G", "TCA"]},                                              # 1 and 3 letters: nearly every read is cut, at its first TCA
            {"adapters": [AN], "min_overlap": 1, "error_permille": 200},
            {"adapters": [N40, A, T33, X32, ADAPTER_NAMES["nextera"], ADAPTER_NAMES["smallrna"], R64, R63]}]      # the most the switch takes
FOUR = SETTINGS[1]
PLANTED = [A, T33, X32, ADAPTER_NAMES["nextera"], R64, R63, AN.replace("N", "T"), A.lower(), N40_PLAIN]


def ids(s):
    return "%s mo=%s e=%s" % (",".join("%d" % len(a) for a in s["adapters"]), s.get("min_overlap", 3), s.get("error_permille", 100))


def full(setting):
    """what get_read_adapters answers under the setting"""
    return {"adapters": [(a.decode() if isinstance(a, bytes) else a).upper() for a in setting["adapters"]], "min_overlap": setting.get("min_overlap", 3), "error_permille": setting.get("error_permille", 100)} if setting.get("adapters") else OFF


def zero(setting):
    return {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0] * len(setting.get("adapters", []))}


def budget(L: int, permille: int = 100) -> int:
    return (L * permille) // 1000


def mutate(a: bytes, count: int) -> bytes:
    """a with `count` letters replaced by another one, spread over it (never the first)"""
    out = bytearray(a)
    for j in range(count):
        at = (j * len(a)) // count + 1
        out[at:at + 1] = bytes(out[at:at + 1]).translate(bytes.maketrans(b"ACGT", b"CGTA"))
    return bytes(out)


def crafted_reads(idx) -> list:
    """[(bases, note)]: the reads by hand, all at Phred 40"""
    lb = rp.locus_bases
    a, t33, r64, r63 = A.encode(), T33.encode(), R64.encode(), R63.encode()
    out = []
    for k, n in enumerate([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 319, 320]):      # total lengths
        out.append((lb(idx, n, k), "plain"))
        t = min(n, 5)
        out.append((lb(idx, n - t, k + 20) + a[:t], "the first letters of the adapter at the 3' end"))
        out.append(((a + lb(idx, n, k + 40))[:n], "begins with the adapter"))
        out.append(((lb(idx, n // 2, k + 60) + r64 + lb(idx, n, k + 80))[:n], "64 letters from the middle on"))
    tail = lb(idx, 150, 3)
    for p in range(150):                                       # an adapter start at every p of one 150-base read
        out.append(((lb(idx, p, p) + a + tail)[:150], "start %d" % p))
    front = lb(idx, 100, 11)
    for L, ad in ((2, a), (3, a), (9, a), (10, a), (19, t33), (20, t33), (63, r64), (64, r64), (63, r63), (13, a), (33, t33)):      # the edges of the error budget
        for more in (0, 1):
            mis = budget(L) + more
            read = front + mutate(ad[:L], mis)
            cut = adapter_cut(read, [ad])[0]
            assert cut == (100 if not more and L >= 3 else len(read)), (L, more, cut)      # (checked on the host: the plant is what it says)
            out.append((read, "L %d with %d mismatches" % (L, mis)))
    out.append((front + b"AGATCGNAAGAGC" + b"TT", "a read N: one mismatch"))
    out.append((front + b"AGATCGNAA", "a read N under budget 0"))
    out.append((front + b"AGNTCGNAAGAGC", "two read Ns"))
    out.append(((front + a + b"ACGTAC").lower(), "lower case"))
    out.append((front.lower() + a, "lower-case read, upper-case adapter"))
    out.append((front + b"AGATCGTAAGAGC", "under the adapter N"))
    out.append((front[:10] + a + front[10:20] + a, "a tie between two starts"))
    out.append((front[:30] + b"TCA" + front[30:40] + b"TCA", "a tie between two starts of the 3-letter adapter"))
    out.append((front + a[:7], "a tie between two adapters"))
    out.append((mutate(a, 1) + b"TTTT" + a, "the exact one beats the leftmost"))
    out.append((a + front, "begins with the adapter"))
    out.append((a.lower(), "is the adapter"))
    out.append((r64 + front, "begins with the 64-letter adapter"))
    out.append((r63[:40], "is the first 40 letters of the 63-letter adapter"))
    n40 = N40_PLAIN.encode()
    for L in (3, 6, 21, 32, 33, 34, 36, 37, 39, 40):          # the 40-letter adapter with Ns over the 3' end: 32 < n - p < 64 among them
        out.append((front + n40[:L], "%d letters of the adapter with Ns" % L))
        out.append((front[:L] + mutate(n40[:L], budget(L)), "... from base %d on, at its budget" % L))
    out.append((front + n40 + front[:17], "the adapter with Ns, 17 bases behind it"))
    long_ = lb(idx, 320, 17)
    for p in (52, 58, 63, 64, 65, 122, 127, 186, 191, 250, 255, 300, 307, 317):      # straddling the 64-base window edges of a 320-base read
        out.append(((long_[:p] + a + long_)[:320], "13 letters from %d on" % p))
        out.append(((long_[:p] + r64 + long_)[:320], "64 letters from %d on" % p))
        out.append(((long_[:p] + mutate(t33, 3) + long_)[:320], "33 letters, 3 mismatches, from %d on" % p))
    for p in (60, 149):                                        # a non-ACGT base only inside the removed part
        out.append((lb(idx, p, p) + a + b"NNRN" + lb(idx, 20, p + 1), "non-ACGT bases behind the adapter"))
        out.append((lb(idx, p, p) + a[:6] + b"N" + a[7:] + b"ACGT", "a non-ACGT base inside the adapter"))
    return out


@functools.lru_cache(maxsize=None)
def sample():
    """(index, [(bases, [Phred])]): test_gpu_read_prep's sample -- about 3,000 reads of 36 - 320 bases on and off the loci, one in three
    with a decayed tail --, one read in three with read-through (an insert shorter than the read, then one of the adapters and what
    follows it), and the crafted reads spread through every group of 64"""
    idx, base = rp.sample()
    rng = np.random.default_rng(13)
    reads = []
    for k, (b, q) in enumerate(base):
        n = len(b)
        if k % 3 == 1 and n >= 40:
            ins = int(rng.integers(20, n))
            b = (b[:ins] + PLANTED[(k // 3) % len(PLANTED)].encode() + letters(rng, n))[:n]
        reads.append((b, q))
    crafted = [(b, [40] * len(b)) for b, _ in crafted_reads(idx)]
    total = len(reads) + len(crafted)
    for k, c in enumerate(crafted):      # evenly over the file: every group of 64 reads holds some
        reads.insert(k * total // len(crafted), c)
    return idx, reads


@functools.lru_cache(maxsize=None)
def raw_text(base: int = 33) -> bytes:
    return rp.fastq_text(sample()[1], base)


@functools.lru_cache(maxsize=None)
def expected(which: int, prep: tuple = ()):
    """(the text the engine must behave as if given, the adapter counters, the preparation counters) for SETTINGS[which] behind the
    read preparation `prep` (items of a dict); computed once"""
    p = dict(prep)
    text, pinfo = prep_fastq(raw_text(rp.base_of(p)), **p) if p else (raw_text(), dict(rp.ZERO))
    cut, info = trim_adapters(text, **SETTINGS[which])
    return cut, info, pinfo


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, default_params())
    e.load_reference(sample()[0])
    yield e
    e.close()


def begin(eng, setting, prep=rp.OFF):
    eng.reset_sample()
    eng.set_read_prep(**prep)
    eng.set_read_adapters(**setting)
    assert eng.get_read_adapters() == full(setting) and eng.get_read_prep() == dict(rp.OFF, **prep)


def left_behind(eng):
    return eng.debug_last_packed(), typed(eng), eng.read_adapters_info(), eng.read_prep_info()


def add_infos(*infos):
    return {"trimmed": sum(i["trimmed"] for i in infos), "bases_removed": sum(i["bases_removed"] for i in infos), "emptied": sum(i["emptied"] for i in infos),
            "per_adapter": [sum(v) for v in zip(*(i["per_adapter"] for i in infos))]}


# ------------------------------------------------------------------ one whole chunk
@pytest.mark.parametrize("which", range(len(SETTINGS)), ids=[ids(s) for s in SETTINGS])
def test_one_whole_chunk_equals_the_cut_text(eng, which):
    setting = SETTINGS[which]
    idx, reads = sample()
    raw = raw_text()
    want_text, want_info, _ = expected(which)
    assert want_info["trimmed"] > 200 and all(v > 0 for v in want_info["per_adapter"]) and want_info["emptied"] > 0
    begin(eng, setting)
    assert eng.submit_fastq(raw) == len(reads)
    got = left_behind(eng)
    begin(eng, {})
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert want[2] == zero({}) and got[2] == want_info, (got[2], want_info)
    assert got[3] == want[3] == rp.ZERO                                      # the counters of the read preparation are its own
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2]
    if which in (0, 1, 2, 5):
        assert int(got[1][0].n_hits.sum()) > 100 and len(got[1][1]) > 100, "the statistics are empty"
        assert (lens & 0x8000).any() and int((lens & 0x7FFF).max()) == 320
    # the guard: the raw text without the switch is another sample -- an engine that ignored the setting would pass otherwise
    begin(eng, {})
    eng.submit_fastq(raw)
    plain = eng.debug_last_packed()
    assert not (np.array_equal(plain[2], lens) and plain[1].shape == got[0][1].shape and np.array_equal(plain[1], got[0][1]))
    if which == 0:      # a non-ACGT base only inside the removed part: bit 15 is the cut read's
        assert int(((plain[2] & 0x8000) != 0).sum()) > int(((lens & 0x8000) != 0).sum())


def test_the_known_answers_on_the_device(eng):
    """the table of test_read_adapters_host.py, the lengths by hand, without trim_adapters in between"""
    for adapters in ([b"AGATCGGAAGAGC"], [b"AGATCGNAAGAGC"], [b"AGATCGGTT", b"AGATCGGAA"], [b"AGATCGGAAGAGC", T33.encode()]):
        rows = [(r, n, k) for r, ads, n, k in KNOWN if ads == adapters]
        assert rows
        begin(eng, {"adapters": adapters})
        assert eng.submit_fastq(rp.fastq_text([(r, [40] * len(r)) for r, _, _ in rows])) == len(rows)
        lens = eng.debug_last_packed()[2]
        assert [int(v) & 0x7FFF for v in lens] == [n for _, n, _ in rows], adapters
        cut = [(r, n, k) for r, n, k in rows if k >= 0]
        assert eng.read_adapters_info() == {"trimmed": len(cut), "bases_removed": sum(len(r) - n for r, n, _ in cut), "emptied": sum(n == 0 for _, n, _ in cut),
                                            "per_adapter": [sum(k == j for _, _, k in cut) for j in range(len(adapters))]}


# ------------------------------------------------------------------ a stream
def test_a_stream_cut_at_every_byte_of_a_sequence_line(eng):
    idx, reads = sample()
    few = [(b[:90], q[:90]) for b, q in reads[400:520]]
    victim = 60
    few[victim] = (rp.locus_bases(idx, 50, 5) + A.encode() + rp.locus_bases(idx, 27, 6), [40] * 90)
    raw = rp.fastq_text(few)
    want_text, want_info = trim_adapters(raw, **FOUR)
    begin(eng, {})
    assert eng.submit_fastq(want_text) == len(few)
    want_reads, want_typed = rp.reads_of(eng), typed(eng)
    assert want_reads[victim][0] & 0x7FFF == 50 and want_info["trimmed"] > 20
    start = sum(len(rc.illumina(k)) + 2 * len(b) + 5 for k, (b, _) in enumerate(few[:victim])) + len(rc.illumina(victim)) + 1
    assert raw[start:start + 90] == few[victim][0]
    for cut in range(start - 1, start + 90 + 2):      # in front of the sequence line ... behind its LF
        begin(eng, FOUR)
        n = eng.submit_fastq_stream(raw[:cut], final=False)
        got = rp.reads_of(eng) if n else []
        n += eng.submit_fastq_stream(raw[cut:], final=True)
        got += rp.reads_of(eng)
        assert n == len(few) and got == want_reads, cut
        assert eng.read_adapters_info() == want_info, cut
    assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ mates
def mate_reads(n_pairs: int):
    """test_gpu_read_prep's mates of different lengths; every seventh first mate and every eleventh second mate begins with an adapter"""
    m1, m2 = rp.mate_reads(sample()[1], n_pairs)
    m1 = [((A.encode() + b)[:len(b)], q) if k % 7 == 0 else (b, q) for k, (b, q) in enumerate(m1)]
    m2 = [((X32.encode() + b)[:len(b)], q) if k % 11 == 0 else (b, q) for k, (b, q) in enumerate(m2)]
    return m1, m2


def test_mates_of_different_lengths_where_one_mate_empties(eng):
    m1, m2 = mate_reads(700)
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    (p1, i1), (p2, i2) = trim_adapters(t1, **FOUR), trim_adapters(t2, **FOUR)
    assert i1["emptied"] >= 700 // 7 - 20 and i2["emptied"] >= 700 // 11 - 20
    begin(eng, FOUR)
    assert eng.submit_fastq_pair(t1, t2) == 1400
    got = left_behind(eng)
    begin(eng, {})
    assert eng.submit_fastq_pair(p1, p2) == 1400
    want = left_behind(eng)
    assert got[2] == add_infos(i1, i2)
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    lens = got[0][2] & 0x7FFF
    assert ((lens[0::2] == 0) & (lens[1::2] > 0)).any() and ((lens[0::2] > 0) & (lens[1::2] == 0)).any() and len(got[1][1]) > 20


# ------------------------------------------------------------------ bgzip
def cuts_inside_sequence_lines(text: bytes, sizes) -> int:
    at, spans = 0, []
    for k, line in enumerate(text.split(b"\n")):
        if k % 4 == 1:
            spans.append((at, at + len(line)))
        at += len(line) + 1
    starts = np.array([s for s, _ in spans])
    n, cut, j = 0, 0, 0
    while cut + sizes[j % len(sizes)] < len(text):
        cut += sizes[j % len(sizes)]
        j += 1
        i = int(np.searchsorted(starts, cut, side="right")) - 1
        n += i >= 0 and spans[i][0] < cut < spans[i][1]
    return n


def test_bgzip_with_blocks_cut_inside_sequence_lines(eng):
    """with all four preparation flags on: Phred+64 text, the trims, then the adapters"""
    idx, reads = sample()
    few = reads[:1300]
    raw = rp.fastq_text(few, 64)
    sizes = (4099, 6007, 9001, 2503)
    assert cuts_inside_sequence_lines(raw, sizes) > 10
    blocks = bgzf_blocks(raw, sizes)
    prepared, pinfo = prep_fastq(raw, **rp.ALL4)
    want_text, want_info = trim_adapters(prepared, **FOUR)
    assert want_info["trimmed"] > 100
    begin(eng, {})
    eng.submit_fastq(want_text)
    want_typed = typed(eng)
    for per_call in (1, 7, len(blocks)):
        begin(eng, FOUR, rp.ALL4)
        n = sum(eng.submit_fastq_bgzf(b"".join(blocks[k:k + per_call]), final=k + per_call >= len(blocks)) for k in range(0, len(blocks), per_call))
        assert n == len(few), per_call
        assert eng.read_adapters_info() == want_info and eng.read_prep_info() == pinfo, per_call
        assert_typed_equal(typed(eng), want_typed)


def test_bgzipd_mates_with_one_file_ahead(eng):
    m1, m2 = mate_reads(600)
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    (p1, i1), (p2, i2) = trim_adapters(t1, **FOUR), trim_adapters(t2, **FOUR)
    begin(eng, {})
    assert eng.submit_fastq_pair(p1, p2) == 1200
    want_typed = typed(eng)
    b1, b2 = bgzf_blocks(t1, (3001, 4507))[:-1], bgzf_blocks(t2, (1777, 2999))[:-1]
    eof = bgzf_blocks(b"")[-1]
    assert len(b1) > 12 and len(b2) > 45
    ahead = [(b"".join(b1[:9]), b"".join(b2[:1])),                           # file 1 nine blocks ahead: its records wait for their mates
             (b"".join(b1[9:10]), b"".join(b2[1:30])),                       # then file 2 overtakes
             (b"", b"".join(b2[30:40])),
             (b"".join(b1[10:]) + eof, b"".join(b2[40:]) + eof)]
    step = [(b"".join(b1[k:k + 3]), b"".join(b2[k:k + 3])) for k in range(0, max(len(b1), len(b2)), 3)] + [(eof, eof)]
    for what, calls in (("one file ahead", ahead), ("three blocks of each per call", step)):
        begin(eng, FOUR)
        n = sum(eng.submit_fastq_bgzf_pair(c1, c2, final=(k == len(calls) - 1)) for k, (c1, c2) in enumerate(calls))
        assert n == 1200, what
        assert eng.read_adapters_info() == add_infos(i1, i2), what
        assert_typed_equal(typed(eng), want_typed)


# ------------------------------------------------------------------ the combinations
def test_all_four_preparation_flags_then_the_adapters(eng):
    idx, reads = sample()
    prep = tuple(sorted(rp.ALL4.items()))
    want_text, want_info, pinfo = expected(1, prep)
    alone = expected(1)[1]
    assert want_info != alone and want_info["trimmed"] > 200 and pinfo["shortened"] > 200      # the order matters: the trims change what the adapters meet
    begin(eng, FOUR, rp.ALL4)
    assert eng.submit_fastq(raw_text(64)) == len(reads)
    got = left_behind(eng)
    begin(eng, {})
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert got[2] == want_info and got[3] == pinfo and want[2] == zero({}) and want[3] == rp.ZERO
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])


def row_width(text: bytes) -> tuple:
    """(wpr, qstride) of the packed rows of FASTQ text: those of its longest read (fq_pack_submit)"""
    longest = max(len(l) for l in text.split(b"\n")[1::4])
    return max(2, ((longest + 15) // 16 + 1) & ~1), max(8, (longest + 7) & ~7)


def test_rows_are_as_wide_as_the_prepared_cut_text_when_every_longest_read_is_cut(eng):
    """trims and adapters both on, every longest prepared read (147 bases) cut to 97: the rows are those of 97 bases, through the text
    parse and through the pair-records parse (the longest length is fed by the last of the two kernels alone)"""
    idx, _ = sample()
    reads = []
    for k in range(320):
        if k % 4 == 0:
            b = rp.locus_bases(idx, 100, k) + A.encode() + rp.locus_bases(idx, 37, k + 1)
        else:
            b = rp.locus_bases(idx, 36 + (k * 7) % 65, k)
        q = [40] * len(b)
        if k % 4 == 1:
            q[-5:] = [2] * 5
        reads.append((b, q))
    prep = {"trim5": 3, "trim_qual": 20}
    raw = rp.fastq_text(reads)
    prepared, pinfo = prep_fastq(raw, **prep)
    want_text, want_info = trim_adapters(prepared, [A])
    assert row_width(prepared) == (10, 152) and row_width(want_text) == (8, 104) and want_info["trimmed"] >= 80
    begin(eng, {})
    assert eng.submit_fastq(want_text) == len(reads)
    want = left_behind(eng)
    assert want[0][3:] == (8, 104)
    begin(eng, {"adapters": [A]}, prep)
    assert eng.submit_fastq(raw) == len(reads)
    got = left_behind(eng)
    assert got[0][3:] == (8, 104), got[0][3:]
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])
    assert got[2] == want_info and got[3] == pinfo
    # mates, bgzip'd: the pair-records parse
    m1, m2 = reads[0::2], reads[1::2]
    t1, t2 = rp.fastq_text(m1, header=rp.mate_header(0)), rp.fastq_text(m2, header=rp.mate_header(1))
    c1, c2 = (trim_adapters(prep_fastq(t, **prep)[0], [A])[0] for t in (t1, t2))
    assert max(row_width(c1), row_width(c2)) == (8, 104) and row_width(prep_fastq(t1, **prep)[0]) == (10, 152)
    begin(eng, {})
    assert eng.submit_fastq_pair(c1, c2) == len(reads)
    want = left_behind(eng)
    begin(eng, {"adapters": [A]}, prep)
    assert eng.submit_fastq_bgzf_pair(b"".join(bgzf_blocks(t1, (7001,))), b"".join(bgzf_blocks(t2, (5003,))), final=True) == len(reads)
    got = left_behind(eng)
    assert len(got[0][2]) == len(reads) and got[0][3:] == (8, 104), got[0][3:]
    rp.assert_packed_equal(got[0], want[0])
    assert_typed_equal(got[1], want[1])


def test_export_bytes_are_those_of_the_cut_text(eng, tmp_path):
    idx, reads = sample()
    raw = raw_text()
    want_text = expected(1)[0]
    begin(eng, {})
    eng.submit_fastq(want_text)
    recs_off, body_off = export(eng, idx, tmp_path / "off.all.sam")
    md_off = b"".join(eng.export_sam_text(idx, md=True))
    begin(eng, FOUR)
    eng.submit_fastq(raw)
    recs_on, body_on = export(eng, idx, tmp_path / "on.all.sam")
    assert body_on == body_off and len(recs_on) > 100
    assert_rule_bytes(idx, recs_on, body_on)
    assert b"".join(eng.export_sam_text(idx, md=True)) == md_off
    # once with the reads' own names: the header lines are not touched, so the names are the file's
    other = Engine(0, default_params())
    try:
        other.load_reference(idx)
        out = []
        for setting, text in ((FOUR, raw), ({}, want_text)):
            other.reset_sample()
            other.set_read_adapters(**setting)
            other.set_read_names(True)
            other.submit_fastq(text)
            out.append((b"".join(other.export_sam_text(idx, md=True)), other.read_names()))
        assert out[0] == out[1] and len(out[0][1]) > 100
        heads = rc.yardstick([raw])
        assert all(heads[ri].startswith(b"@" + nm) for ri, nm in out[0][1].items())
        assert out[0][0] != md_off and len(out[0][0].splitlines()) == len(md_off.splitlines())
    finally:
        other.close()


# ------------------------------------------------------------------ refusals and life cycle
def test_every_other_way_of_adding_reads_is_refused():
    idx, reads = sample()
    text = rp.fastq_text(reads[:400])
    eng = Engine(0, default_params())
    try:
        eng.load_reference(idx)
        assert eng.get_read_adapters() == OFF and eng.read_adapters_info() == zero({})
        for bad, why in (({"adapters": "AGAX"}, "outside ACGTN"), ({"adapters": "ACGT,NNN"}, "adapter 2 holds only N"), ({"adapters": ",".join(["ACGT"] * 9)}, "more than 8 adapters"),
                         ({"adapters": "A" * 65}, "longer than 64 letters"), ({"adapters": "ACGT,"}, "adapter 2 is empty"), ({"adapters": "ACGT", "min_overlap": 0}, "min_overlap 0 is outside 1..64"),
                         ({"adapters": "ACGT", "min_overlap": 65}, "min_overlap 65 is outside 1..64"), ({"adapters": "ACGT", "error_permille": 501}, "error_permille 501 exceeds 500")):
            with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_adapters: .*" + why):
                eng.set_read_adapters(**bad)
        assert eng.get_read_adapters() == OFF
        eng.set_read_adapters(["a" * 64] + ["ACGTN"] * 7, 64, 500)               # the limits are taken
        assert eng.get_read_adapters() == {"adapters": ["A" * 64] + ["ACGTN"] * 7, "min_overlap": 64, "error_permille": 500}
        assert eng.lib.mlst_set_read_adapters(eng._h, None, 3, 100) == 0 and eng.get_read_adapters() == OFF      # NULL: off
        eng.set_read_adapters("acgt")
        assert eng.lib.mlst_set_read_adapters(eng._h, b"", 0, 9999) == 0 and eng.get_read_adapters() == OFF      # "": off, whatever the numbers
        fb = np.frombuffer(reads[0][0], np.uint8); fq = np.frombuffer(bytes(v + 33 for v in reads[0][1]), np.uint8); off = np.array([0, len(fb)], np.uint64)
        calls = {
            "mlst_submit_reads": lambda: eng.submit_reads(fb, fq, off),
            "mlst_submit_reads_device": lambda: eng.submit_reads_device(0, 0, 0, 1, 150),
            "mlst_submit_packed_device": lambda: eng.submit_packed_device(0, 0, 0, 1, 10, 152),
            "mlst_submit_packed_host": lambda: eng._check(eng.lib.mlst_submit_packed_host(eng._h, None, None, None, 1, 10, 152, 0), "mlst_submit_packed_host"),
            "mlst_submit_fasta": lambda: eng.submit_fasta(b">c\n" + b"ACGT" * 100 + b"\n"),
            "mlst_bam_reads_open": lambda: eng.bam_reads_open(0),
            "mlst_set_read_tiling": lambda: eng.set_read_tiling(150, 25),
        }
        eng.set_read_adapters(A)
        for entry, call in calls.items():
            with pytest.raises(MlstError, match=r"\(-1\): %s: adapter removal is on \(mlst_set_read_adapters\)" % entry):
                call()
        assert eng.get_read_tiling() == (0, 0)
        assert eng.submit_fastq(text) == 400                                 # the handle stays usable
        want_info = trim_adapters(text, [A])[1]
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_adapters"):
            eng.set_read_adapters()
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads: mlst_set_read_adapters"):
            eng.set_read_adapters(A, 4)
        eng.set_read_adapters(A.lower())                                     # (no change: accepted)
        assert eng.get_read_adapters() == full({"adapters": [A]}) and eng.read_adapters_info() == want_info and want_info["trimmed"] > 50
        eng.reset_sample()                                                   # keeps the setting, zeroes the counters
        assert eng.get_read_adapters() == full({"adapters": [A]}) and eng.read_adapters_info() == zero({"adapters": [A]})
        eng.submit_fastq_stream(text[:1000], final=False)                    # a stream is open
        with pytest.raises(MlstError, match=r"\(-1\).*stream is open"):
            eng.set_read_adapters()
        eng.reset_sample()
        eng.set_read_adapters()
        eng.submit_reads(fb, fq, off)                                        # off again: every entry is open
        with pytest.raises(MlstError, match=r"\(-1\).*the sample holds reads"):
            eng.set_read_adapters(A)
        eng.reset_sample()
        eng.set_read_tiling(150, 25)
        with pytest.raises(MlstError, match=r"\(-1\): mlst_set_read_adapters: mlst_set_read_tiling is on"):
            eng.set_read_adapters(A)
        eng.set_read_adapters()                                              # (off behind a tile: nothing to refuse)
        eng.set_read_tiling(0, 0)
        # switched off afterwards, a plain submission is a fresh engine's
        eng.reset_sample()
        eng.set_read_adapters(**FOUR)
        eng.submit_fastq(text)
        eng.reset_sample()
        eng.set_read_adapters()
        eng.submit_fastq(text)
        got = left_behind(eng)
        fresh = Engine(0, default_params())
        try:
            fresh.load_reference(idx)
            fresh.submit_fastq(text)
            want = left_behind(fresh)
        finally:
            fresh.close()
        assert got[2] == want[2] == zero({})
        rp.assert_packed_equal(got[0], want[0])
        assert_typed_equal(got[1], want[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ the command
def read_through(reads, seed: int = 5):
    """two reads in three get read-through: the read is the insert, then the Illumina adapter and up to 20 further bases"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (b, q) in enumerate(reads):
        if k % 3 and len(b) + len(A) <= 320:
            more = letters(rng, int(rng.integers(0, 21)))
            b2 = (b + A.encode() + more)[:320]
            out.append((b2, list(q) + [38] * (len(b2) - len(b))))
        else:
            out.append((b, q))
    return out


@functools.lru_cache(maxsize=None)
def command_sample():
    """(the reads with read-through, the clean reads): test_gpu_read_prep's planted sample.  The clean reads are what the rule leaves
    of the others -- the planted reads themselves but for the few that lose bases by chance (about 2 % at --adapter-min-overlap 3)"""
    clean = rp.planted_sample()
    raw = read_through(clean)
    text, info = trim_adapters(rp.fastq_text(raw), [A])
    recs = text.split(b"\n")[1::4]
    same = sum(r == b for r, (b, _) in zip(recs, clean))
    assert same >= 0.96 * len(clean) and info["trimmed"] >= 0.6 * len(clean)
    return raw, clean, text, info


LINE = "adapter removal: %d reads cut, %d bases removed, %d reads left without a base (" + A + " %d)"


def test_cli_adapter_types_read_through_as_the_clean_reads(tmp_path, monkeypatch, capsys):
    raw, clean, clean_text, info = command_sample()
    for d, text in (("raw", rp.fastq_text(raw)), ("clean", clean_text)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / "s.fastq").write_bytes(text)
    rp.run_type(monkeypatch, capsys, tmp_path / "clean", ["s.fastq", "--quiet"], tmp_path / "o_clean")
    said = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--adapter", "illumina"], tmp_path / "o_raw")
    rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--quiet"], tmp_path / "o_noflag")
    want, got, wrong = rp.written(tmp_path / "o_clean"), rp.written(tmp_path / "o_raw"), rp.written(tmp_path / "o_noflag")
    assert sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    assert got == want
    assert LINE % (info["trimmed"], info["bases_removed"], info["emptied"], info["per_adapter"][0]) in said, said[-300:]
    assert wrong != want                                                     # without the flag the adapter tails are typed
    quiet = rp.run_type(monkeypatch, capsys, tmp_path / "raw", ["s.fastq", "--adapter", A.lower(), "--quiet"], tmp_path / "o_quiet")
    assert "adapter removal" not in quiet and rp.written(tmp_path / "o_quiet") == want
    # a sample without adapters: the same bytes with and without the flags (an exact, whole adapter is in none of the clean reads)
    strict = ["--adapter", "illumina", "--adapter-min-overlap", "13", "--adapter-error-rate", "0"]
    assert trim_adapters(clean_text, [A], 13, 0)[1]["trimmed"] == 0
    said = rp.run_type(monkeypatch, capsys, tmp_path / "clean", ["s.fastq"] + strict, tmp_path / "o_strict")
    assert rp.written(tmp_path / "o_strict") == want and LINE % (0, 0, 0, 0) in said


def test_cli_adapter_on_a_folder_and_mates(tmp_path, monkeypatch, capsys):
    raw, clean, _, _ = command_sample()
    raw_dir, cut_dir = tmp_path / "raw", tmp_path / "cut"
    for d in (raw_dir, cut_dir):
        os.makedirs(d / "in")
    n = len(raw) // 2
    m1, m2 = raw[0:2 * n:2], raw[1:2 * n:2]
    texts = {"m_1.fastq": rp.fastq_text(m1, header=rp.mate_header(0)), "m_2.fastq": rp.fastq_text(m2, header=rp.mate_header(1))}
    third = len(raw) // 3
    texts.update({"in/f%d.fastq" % k: rp.fastq_text(raw[k * third:(k + 1) * third] + raw[:400]) for k in range(3)})
    infos = {}
    two = [A, T33[13:]]
    for name, text in texts.items():
        (raw_dir / name).write_bytes(text)
        cut, infos[name] = trim_adapters(text, two, 4, 125)
        (cut_dir / name).write_bytes(cut)
    flags = ["--adapter", "illumina," + T33[13:].lower(), "--adapter-min-overlap", "4", "--adapter-error-rate", "0.125"]
    for what, args, names in (("folder", ["in"], ["in/f0.fastq", "in/f1.fastq", "in/f2.fastq"]), ("mates", ["m_1.fastq", "-2", "m_2.fastq"], ["m_1.fastq", "m_2.fastq"])):
        said = rp.run_type(monkeypatch, capsys, raw_dir, args + flags, tmp_path / ("o_raw_" + what))
        rp.run_type(monkeypatch, capsys, cut_dir, args + ["--quiet"], tmp_path / ("o_cut_" + what))
        got, want = rp.written(tmp_path / ("o_raw_" + what)), rp.written(tmp_path / ("o_cut_" + what))
        assert got == want and len(want) == 2 * (3 if what == "folder" else 1) and all(len(v) > 0 for v in want.values()), what
        total = add_infos(*(infos[f] for f in names))
        line = "adapter removal: %d reads cut, %d bases removed, %d reads left without a base (%s %d, %s %d)" % (
            total["trimmed"], total["bases_removed"], total["emptied"], A, total["per_adapter"][0], T33[13:], total["per_adapter"][1])
        assert line in said and total["trimmed"] > 500, (what, said[-400:])
    # with the read preparation and the exports: they carry the prepared, cut SEQ / QUAL
    prep_flags, prep = ["--trim5", "7", "--trim-qual", "20"], {"trim5": 7, "trim_qual": 20}
    text = rp.fastq_text(raw)
    (raw_dir / "s.fastq").write_bytes(text)
    (cut_dir / "s.fastq").write_bytes(trim_adapters(prep_fastq(text, **prep)[0], two, 4, 125)[0])
    more = ["--quiet", "--write-sam", "--write-sam-all", "--md", "--read-names"]
    rp.run_type(monkeypatch, capsys, raw_dir, ["s.fastq"] + more + flags + prep_flags, tmp_path / "x_raw")
    rp.run_type(monkeypatch, capsys, cut_dir, ["s.fastq"] + more, tmp_path / "x_cut")
    got, want = rp.written(tmp_path / "x_raw"), rp.written(tmp_path / "x_cut")
    assert got == want and sorted(want) == ["s.all.sam", "s.nfo", "s.out", "s.sam"] and want["s.all.sam"].count(b"\n") > 500


def test_cli_two_ranks_equal_one_process(tmp_path):
    """in the manner of test_gpu_multirank.py: two ranks on the one GPU, gloo collectives"""
    raw, clean, clean_text, info = command_sample()
    db, _ = fx.ecoli_small(40, 5)
    (tmp_path / "s.fastq").write_bytes(rp.fastq_text(raw))
    os.makedirs(tmp_path / "p")
    (tmp_path / "p" / "s.fastq").write_bytes(clean_text)
    env = dict(os.environ, MLST_FASTQ_CHUNK=str(256 << 10), MLST_ONE_GPU="1", MLST_BACKEND="gloo")      # several chunks per rank
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    tail = ["-d", db.path, "--min_accuracy", "0", "--nloci", "0", "--log"]
    outs = []
    for cwd, args in ((tmp_path, ["--adapter", "illumina", "--gpus", "2", "-o", str(tmp_path / "two")]), (tmp_path / "p", ["--quiet", "-o", str(tmp_path / "one")])):
        r = subprocess.run([sys.executable, "-m", "metamlst_amd.cli", "type", "s.fastq"] + tail + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    got, want = rp.written(tmp_path / "two"), rp.written(tmp_path / "one")
    assert got == want and sorted(want) == ["s.nfo", "s.out"] and len(want["s.nfo"]) > 0
    lines = [l for l in outs[0].splitlines() if l.startswith("adapter removal:")]
    assert lines == [LINE % (info["trimmed"], info["bases_removed"], info["emptied"], info["per_adapter"][0])]


def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    monkeypatch.chdir(tmp_path)
    tail = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]
    for args, why in ((["s.fastq", "--alignments"], "--adapter: with --alignments the records are what they are"),
                      (["c.fa", "--contigs"], "--adapter: --contigs cuts assemblies into windows"),
                      (["s.fastq", "--long-reads"], "--adapter: --long-reads cuts reads into windows"),
                      ([str(bam), "--long-bam-reads"], "--adapter: --long-bam-reads cuts reads into windows"),
                      ([str(bam)], "--adapter: the reads of a BAM are taken as they are stored: FASTQ input only")):
        assert cli.main(["type"] + args + ["--adapter", "nextera"] + tail) == 1
        assert why in capsys.readouterr().out, args
    for flags, why in ((["--adapter-min-overlap", "5"], "--adapter-min-overlap belongs to --adapter"),
                       (["--adapter-error-rate", "0.2"], "--adapter-error-rate belongs to --adapter"),
                       (["--adapter", "AGAX"], "--adapter: adapter 'AGAX' holds a letter outside ACGTN"),
                       (["--adapter", "illumina,NNNN"], "--adapter: adapter 'NNNN' holds only N"),
                       (["--adapter", ",".join(["smallrna"] * 9)], "--adapter: 9 adapters: 1 to 8 are taken"),
                       (["--adapter", "A" * 65], "--adapter: an adapter holds 65 letters: 1 to 64 are taken"),
                       (["--adapter", "illumina", "--adapter-min-overlap", "0"], "--adapter: min_overlap 0 is outside 1..64"),
                       (["--adapter", "illumina", "--adapter-error-rate", "0.6"], "--adapter: --adapter-error-rate takes a number from 0 to 0.5, not 0.6")):
        assert cli.main(["type", "s.fastq"] + flags + tail) == 1
        assert why in capsys.readouterr().out, flags
    assert not os.path.exists(tmp_path / "o")
