"""The crafted texts of tests/fasta_edges.py hold what they say (CPU): every offset points at the bytes it names, the slid probe
puts every transition on, behind and in front of every edge, the turn texts span the turns they claim, the contig counts stand
where the entry's table guess needs them, and no GPU case tiles into more than 40,000 reads."""
import pytest

import fasta_edges as fe

MAX_READS = 40_000


def cell(p):
    return p // fe.CELL


def test_the_probe_holds_every_transition_where_it_says():
    text, at = fe.probe()
    assert 300 <= len(text) <= 1000
    assert set(at) == set(fe.PROBE_PATTERNS)
    for name, pattern in fe.PROBE_PATTERNS.items():
        assert fe.find(pattern, text, at[name]), (name, text[at[name]:at[name] + 8])
        assert 0 < at[name] < len(text) - 1      # (slid by one byte either way, it is still a byte of the probe)
    # header lines hold no LF of their own; a sequence-line '>' is not at a line start; the empty contig is empty
    assert text[at["> inside a sequence line"]:][:1] in b"ACGT" and text[at["> inside a sequence line"] - 1:][:1] != b"\n"
    fq, contigs = fe.yardstick(text)
    lens = [len(l) for l in fq.split(b"\n")[1::4]]
    assert contigs == 6 and len(lens) == fe.PROBE_READS == fe.count_reads(text)
    names = [n[1:].split(b"_")[0] for n in fq.split(b"\n")[0::4][:-1]]
    assert [names.count(b"%d" % c) for c in range(6)] == [1, 2, 0, 3, 1, 1]      # contigs of 100, 151, 0, 176, 60, 50 bases
    assert sorted(set(lens)) == [50, 60, 100, 150]


@pytest.mark.parametrize("edge", [fe.THREAD, fe.WAVE, fe.CELL])
def test_the_slid_probe_puts_every_transition_on_every_side_of_the_edge(edge):
    p, at = fe.probe()
    text, info = fe.slide(edge)
    assert text.startswith(b">pad0_")
    assert len(info["copies"]) == (len(p) if edge > fe.THREAD else fe.THREAD)
    for j, off in info["copies"]:
        assert text[off:off + len(p)] == p and (off + j) % edge == 0
        assert text[off - 2:off] == b"x\n" or text[off - 1:off] == b"\n"      # behind its padding header
    for name, t in at.items():
        seen = {(off + t) % edge for _, off in info["copies"]}
        assert {edge - 1, 0, 1} <= seen, (name, sorted(seen)[:5])
        for _, off in info["copies"]:
            assert fe.find(fe.PROBE_PATTERNS[name], text, off + t)
    fq, contigs = fe.yardstick(text)
    assert contigs == 7 * len(info["copies"])      # the padding header and the probe's six
    assert fq.count(b"\n") // 4 == fe.PROBE_READS * len(info["copies"]) <= MAX_READS
    if edge == fe.CELL:
        assert len({(off + j) // fe.CELL for j, off in info["copies"]}) == len(p)      # every copy has a cell edge of its own
        assert 0 < fe.count_reads(text, (36, 100, 36)) <= MAX_READS


def test_the_turn_texts_span_the_turns_they_claim():
    texts = fe.turn_texts()
    assert sorted(texts) == ["hdr_over_turn", "seq_over_turn", "turn_without_line_start", "turn_without_line_start_seq"]
    edge = fe.TURN * fe.CELL
    for name, (text, info) in texts.items():
        lo, hi = info["span"]
        line = text[lo:hi]
        assert b"\n" not in line and text[hi:hi + 1] == b"\n"
        n_cells = (len(text) + fe.CELL - 1) // fe.CELL
        assert n_cells > info["min_cells"]
        header = name in ("hdr_over_turn", "turn_without_line_start")
        assert (text[lo - 1:lo + 1] == b"\n>") == header
        if not header:
            assert text[lo - 10:lo] == b">one_line\n" and set(line) <= set(b"ACGT")
        if name.endswith("over_turn"):
            assert info["min_cells"] == fe.TURN and n_cells < 2 * fe.TURN
            assert cell(lo) <= fe.TURN - 3 and cell(hi) >= fe.TURN + 2      # two whole cells and more on either side of the edge
            assert lo < edge < hi
            assert len(line) == 40_000 if header else True
            assert text[:edge - 4 * fe.CELL].count(b"\n>fill") > 500      # 70-column filler contigs in front
        else:
            assert info["min_cells"] == 2 * fe.TURN
            assert cell(lo) < fe.TURN and cell(hi) >= 2 * fe.TURN      # begins in turn 1, ends in turn 3
            assert b"\n" not in text[fe.TURN * fe.CELL:2 * fe.TURN * fe.CELL]      # a whole turn without a line start
            assert 8_300_000 < len(text) < 8_700_000
        assert info["tile"] == ((320, 320, 50) if name == "turn_without_line_start_seq" else (150, 150, 50))
        assert 0 < fe.count_reads(text, info["tile"]) <= MAX_READS, name
    # behind the header over the turn edge: a contig whose bases a kind stuck at "sequence" would mix with the header's letters
    text, info = texts["hdr_over_turn"]
    assert text[info["span"][1]:].split(b">")[0].count(b"\n") == 7 and len(text[info["span"][1]:].split(b">")[0].replace(b"\n", b"")) == 400


def test_contig_counts_against_the_table_guess():
    text, info = fe.many_contigs()
    assert (len(text), info["guess"], info["contigs"]) == (371_248, 6_824, 2_500)
    assert (b"\n" + text).count(b"\n>") == info["contigs"] and 2 * fe.TURN < info["contigs"] < info["guess"] == len(text) // 64 + 1024
    assert fe.count_reads(text) == 6_426 <= MAX_READS
    text, info = fe.tiny_contigs()
    assert (len(text), info["guess"], info["contigs"]) == (25_200, 1_417, 3_000)
    assert (b"\n" + text).count(b"\n>") == info["contigs"] > len(text) // 64 + 1024 == info["guess"]
    assert fe.count_reads(text, (4, 2, 1)) == 5_400 and fe.count_reads(text, (150, 25, 1)) == 2_700
    big, binfo = fe.tiny_contigs(9000)
    assert binfo["contigs"] == 9_000 > 3_000 > binfo["guess"]      # (kept tables of 3,000 entries: no growth in front of the first pass, a repeat behind it)
    assert fe.count_reads(big, (4, 2, 1)) == 16_200 <= MAX_READS


@pytest.mark.parametrize("first", fe.START_RUNS)
def test_the_runs_of_contigs_without_reads(first):
    text, info = fe.empty_runs(first)
    assert info["runs"] == [(0, first), (first + 2, 300), (first + 304, 300)] and info["contigs"] == first + 604
    assert info["contigs"] < len(text) // 64 + 1024      # (no table growth: that is another test's)
    for tile, per in (((150, 25, 50), 11 + 2), ((320, 1, 50), 81 + 1)):
        fq, contigs = fe.yardstick(text, tile)
        assert contigs == info["contigs"]
        with_reads = sorted({int(n[1:].split(b"_")[0]) for n in fq.split(b"\n")[0::4][:-1]})
        assert with_reads == [first, first + 1, first + 302, first + 303]
        assert fq.count(b"\n") // 4 == 2 * per <= MAX_READS
    assert text.startswith(b">none0\n>") and text.endswith(b"\n>none%d\n" % (info["contigs"] - 1))      # a run at the very start, a run at the very end, both with contigs of no bases


def test_the_endings():
    texts = fe.endings()
    assert len(texts) == len(fe.ENDINGS) * len(fe.END_LENGTHS) + 2
    assert sorted({n % 16 for n in fe.END_LENGTHS}) == [0, 1, 15] and {4096, 4097} <= set(fe.END_LENGTHS)
    want = {"bases": rb"[ACGT]{55}\Z", "bases_lf": rb"[ACGT]{55}\n\Z", "bases_crlf": rb"[ACGT]{55}\r\n\Z", "lf_gt": rb"[ACGT]\n>\Z", "lf_gt_name": rb"[ACGT]\n>name\Z",
            "gt_alone": rb">e*\Z", "gt_lf_alone": rb">e*\n\Z", "bases_cr": rb"[ACGT]{55}\r\Z"}
    assert sorted(want) == sorted(fe.ENDINGS)
    import re
    for (name, n), text in texts.items():
        assert len(text) == n and text[:1] == b">"
        assert re.search(want[name], text, re.S), (name, n, text[-12:])
        if name.startswith("gt_"):
            assert re.fullmatch(want[name], text, re.S) and fe.yardstick(text) == (b"", 1)
        else:
            fq, contigs = fe.yardstick(text)      # tile_fasta accepts every one of them, "bases_cr" too: strip() takes the CR off
            assert contigs == 3 + name.startswith("lf_gt")
            assert [len(l) for l in fq.split(b"\n")[1::4]] == [150, 150, 150, 150, 150, 150, 130, 55]
    assert texts[("gt_alone", 1)] == b">" and texts[("gt_lf_alone", 2)] == b">\n"
    same = {fe.yardstick(texts[(name, 607)])[0] for name in fe.ENDINGS if not name.startswith("gt_")}
    assert len(same) == 1      # the ending changes no read


def test_the_three_cells_and_the_bytes_the_refusals_overwrite():
    text, at = fe.three_cells()
    assert len(text) == 3 * fe.CELL and text.count(b">") == 1
    for k in ("t3", "last", "cell2", "cell0_end", "line_start"):
        assert text[at[k]:at[k] + 2].isalpha() and text[at[k] - 1:at[k]] in (b"A", b"C", b"G", b"T", b"\n"), k
    assert (at["t3"] % 16, at["last"] % 16, cell(at["t3"]), cell(at["last"]), cell(at["cell2"])) == (3, 15, 0, 0, 2)
    assert at["cell2"] % 16 not in (0, 15) and at["cell0_end"] == fe.CELL - 1
    assert text[at["line_start"] - 1:at["line_start"]] == b"\n" and cell(at["line_start"]) == 1
    assert 0 < at["hdr"] < text.index(b"\n")
    # what the device refuses, tile_fasta's strip() accepts where the byte stands at a line's start: the reads differ by one base
    a = fe.yardstick(fe.with_bytes(text, (at["line_start"], b" ")))[0]
    assert a.count(b"\n") == fe.yardstick(text)[0].count(b"\n") and a != fe.yardstick(text)[0]
    assert fe.with_bytes(text, (5, b"xy"), (9, b"z"))[4:10] == text[4:5] + b"xy" + text[7:9] + b"z"
