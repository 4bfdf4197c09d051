"""The device FASTA tiler (mlst_submit_fasta, csrc/fasta_dev.h) at its thread, wave, cell and turn edges: the crafted texts of
tests/fasta_edges.py (their figures: tests/test_fasta_edges_host.py), every submission against fastq.tile_fasta's text packed on the
host (fe.assert_rows_equal).  Engine.fasta_info() says which path a call took: the second turn of the one-workgroup kernels and
the repeat of a call whose contig tables were too small are asserted, not inferred from sizes.  profiles/contigs.md lists the
deliberate errors each of these tests was seen to catch."""
import functools

import pytest

import fasta_edges as fe
import fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return fx.ecoli_small(80)


def make_engine(ref):
    from metamlst_amd.engine import Engine
    eng = Engine(0)
    eng.load_reference(ref[1])
    return eng


@pytest.fixture(scope="module")
def eng(ref):
    return make_engine(ref)


@functools.lru_cache(maxsize=None)
def turn_texts():
    return fe.turn_texts()


def refused(eng, text, byte, why, tile=fe.TILE):
    """the call is refused naming `byte` and the reason; nothing of it was submitted"""
    from metamlst_amd.engine import HostPathNeeded
    eng.reset_sample()
    with pytest.raises(HostPathNeeded, match=r"%s at byte %d$" % (why, byte)):
        eng.submit_fasta(text, *tile)
    st = eng.stats()
    assert int(st.counters[2]) == 0 and int(st.n_hits.sum()) == 0


WS, CR = "white space inside a sequence line", "a CR without its LF in a sequence line"


# ------------------------------------------------------------------ 1. thread, wave and cell edges
@pytest.mark.parametrize("edge", [fe.THREAD, fe.WAVE, fe.CELL])
def test_probe_slid_over_every_thread_wave_and_cell_edge(eng, edge):
    text, info = fe.slide(edge)
    n = fe.PROBE_READS * len(info["copies"])
    assert fe.assert_rows_equal(eng, text, fe.TILE, n) == (7 * len(info["copies"]), n)
    if edge == fe.CELL:
        fe.assert_rows_equal(eng, text, (36, 100, 36))


# ------------------------------------------------------------------ 2. turns of k_fa_state
@pytest.mark.parametrize("name", ["seq_over_turn", "hdr_over_turn", "turn_without_line_start", "turn_without_line_start_seq"])
def test_a_line_over_the_turn_edge_keeps_its_kind(eng, name):
    text, info = turn_texts()[name]
    n_contigs, _ = fe.assert_rows_equal(eng, text, info["tile"])
    cells, contigs, _, passes = eng.fasta_info()
    assert cells == (len(text) + fe.CELL - 1) // fe.CELL > info["min_cells"]      # k_fa_state and k_fa_scan(0) ran a second (third) turn
    assert (contigs, passes) == (n_contigs, 1)


# ------------------------------------------------------------------ 3. turns of k_fa_scan over the contigs
def test_more_than_1024_contigs_scan_in_turns(eng):
    text, info = fe.many_contigs()
    assert fe.assert_rows_equal(eng, text, fe.TILE, 6426) == (info["contigs"], 6426)
    cells, contigs, entries, passes = eng.fasta_info()
    assert contigs == info["contigs"] > 2 * fe.TURN and passes == 1 and entries >= info["guess"] > contigs


# ------------------------------------------------------------------ 4. the repeat with grown tables
def test_contig_tables_grow_and_the_call_repeats(ref):
    eng = make_engine(ref)
    text, info = fe.tiny_contigs()
    assert fe.assert_rows_equal(eng, text, (4, 2, 1), 5400) == (3000, 5400)
    assert eng.fasta_info() == ((len(text) + fe.CELL - 1) // fe.CELL, 3000, 3000, 2)
    fe.assert_rows_equal(eng, text, (4, 2, 1), 5400)
    assert eng.fasta_info()[2:] == (3000, 1)      # the grown tables are kept
    fe.assert_rows_equal(eng, fe.probe()[0], fe.TILE, fe.PROBE_READS)      # max_len and the row width follow the call, not the call before
    assert eng.fasta_info()[1:] == (6, 3000, 1)
    big, binfo = fe.tiny_contigs(9000)
    assert binfo["guess"] < 3000
    fe.assert_rows_equal(eng, big, (4, 2, 1), 16200)
    assert eng.fasta_info()[1:] == (9000, 9000, 2)
    fe.assert_rows_equal(eng, fe.probe()[0], fe.TILE, fe.PROBE_READS)


def test_the_longest_read_is_that_of_the_repeated_pass(ref):
    """At 150,25,1 every read of tiny_contigs() is a whole contig of 1 to 9 bases.  In the first pass the last contig the small
    tables hold seems to reach to the end of the sequence, so that pass sees a read of 150 bases: the rows are 2 words wide only
    if the repeat starts the maximum again."""
    eng = make_engine(ref)
    text, _ = fe.tiny_contigs()
    fe.assert_rows_equal(eng, text, (150, 25, 1), 2700)
    assert eng.fasta_info()[3] == 2
    assert eng.debug_last_packed()[3:] == (2, 16)


# ------------------------------------------------------------------ 5. k_fa_reads' search over contigs without reads
@pytest.mark.parametrize("first", fe.START_RUNS)
def test_runs_of_contigs_without_reads(eng, first):
    text, info = fe.empty_runs(first)
    for tile in (fe.TILE, (320, 1, 50)):
        assert fe.assert_rows_equal(eng, text, tile)[0] == info["contigs"]
        assert eng.fasta_info()[3] == 1


# ------------------------------------------------------------------ 6. the end of the text
ENDINGS = fe.endings()


@pytest.mark.parametrize("name,length", sorted(ENDINGS), ids=["%s-%d" % k for k in sorted(ENDINGS)])
def test_endings(eng, name, length):
    text = ENDINGS[(name, length)]
    if name == "bases_cr":
        refused(eng, text, length - 1, CR)
    else:
        n_contigs, n_reads = fe.assert_rows_equal(eng, text, fe.TILE)
        assert (n_contigs, n_reads) == ((1, 0) if name.startswith("gt_") else (3 + name.startswith("lf_gt"), 8))
        assert eng.fasta_info()[:2] == ((length + fe.CELL - 1) // fe.CELL, n_contigs)
    fe.assert_rows_equal(eng, fe.probe()[0], fe.TILE, fe.PROBE_READS)


# ------------------------------------------------------------------ 7. refusals
def test_the_smallest_offending_byte_is_reported(eng):
    text, at = fe.three_cells()
    probe = fe.probe()[0]

    def then_fine():
        fe.assert_rows_equal(eng, probe, fe.TILE, fe.PROBE_READS)

    fe.assert_rows_equal(eng, text, fe.TILE)
    # two offenders in two workgroups: the one in front is named, whichever workgroup came first
    refused(eng, fe.with_bytes(text, (at["cell2"], b" "), (at["t3"], b"\x0b")), at["t3"], WS); then_fine()
    # two in neighbouring threads of one wave
    refused(eng, fe.with_bytes(text, (at["last"], b"\x0c"), (at["last"] + 1, b"\t")), at["last"], WS); then_fine()
    # a CR is judged by its successor, which another workgroup's cell holds
    refused(eng, fe.with_bytes(text, (at["cell0_end"], b"\r")), at["cell0_end"], CR); then_fine()
    fe.assert_rows_equal(eng, fe.with_bytes(text, (at["cell0_end"], b"\r\n")), fe.TILE)
    # a CR that IS an offence in front of white space that is one too: the smaller byte, with its own reason
    refused(eng, fe.with_bytes(text, (at["t3"], b"\r"), (at["cell2"], b"\t")), at["t3"], CR); then_fine()
    # white space in a header is no offence
    fe.assert_rows_equal(eng, fe.with_bytes(text, (at["hdr"], b" \t\x0b\x0c")), fe.TILE)
    # at the START of a sequence line strip() would take it off: the text goes to the host
    for ws in (b" ", b"\t"):
        refused(eng, fe.with_bytes(text, (at["line_start"], ws)), at["line_start"], WS); then_fine()


# ------------------------------------------------------------------ 8. buffers reused at a smaller and a larger size
def test_big_then_small_then_big(ref):
    eng = make_engine(ref)
    text, info = turn_texts()["seq_over_turn"]
    for src, tile in ((text, info["tile"]), (fe.probe()[0], fe.TILE), (text, info["tile"])):
        fe.assert_rows_equal(eng, src, tile)
        assert eng.fasta_info()[0] == (len(src) + fe.CELL - 1) // fe.CELL
