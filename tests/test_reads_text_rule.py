"""The host side of `cli type --write-reads` (no GPU): samout.reads_fastq_rule -- the rule csrc/reads_text.h is held to -- on hand-written
cases, every combination the command refuses before it makes an engine, and the three symbols of the C ABI in the built library."""
import ctypes as C
import os

import pytest

from metamlst_amd import cli, samout
from metamlst_amd import engine as eng_mod

READS = {
    0: (b"ACGT", bytes([0, 1, 2, 3])),
    3: (b"acgtNRn-", bytes([40, 41, 93, 94, 127, 2, 30, 60])),      # lower case is the letter, everything else is N; Phred clamps at 93
    4: (b"GGGGGG", bytes([10] * 6)),
    5: (b"TTTT", bytes([20] * 4)),
    2 ** 32 + 7: (b"CA", bytes([33, 34])),
    10 ** 10 + 1: (b"A", bytes([0])),
}


def test_record_letters_clamp_and_order():
    got = samout.reads_fastq_rule(READS, [5, 3, 0], False)
    assert got == [b"@r0\nACGT\n+\n!\"#$\n", b"@r3\nACGTNNNN\n+\nIJ~~~#?]\n", b"@r5\nTTTT\n+\n5555\n"]
    assert samout.reads_fastq_rule(READS, [0, 3, 5], False) == got                      # the order of `aligned` is not the file's
    assert all(r.count(b"\n") == 4 and b"\r" not in r for r in got)
    assert chr(93 + 33) == "~" and samout._QUAL_TAB[94] == samout._QUAL_TAB[93] == 126 and samout._QUAL_TAB[92] == 125


def test_a_read_with_several_records_is_written_once():
    assert samout.reads_fastq_rule(READS, [4, 4, 4, 0, 4, 0], False) == samout.reads_fastq_rule(READS, [0, 4], False)
    assert len(samout.reads_fastq_rule(READS, [4] * 1000, False)) == 1


def test_an_empty_set_gives_no_record():
    assert samout.reads_fastq_rule(READS, [], False) == [] == samout.reads_fastq_rule({}, (), True, {})


def test_pairs_carry_the_mate_suffix_and_each_mate_stands_alone():
    # pair 2 = reads 4 and 5: both aligned; pair 0: only the first; pair 1: only the second
    got = samout.reads_fastq_rule(READS, [0, 3, 4, 5], True)
    assert [r.split(b"\n", 1)[0] for r in got] == [b"@r0/1", b"@r1/2", b"@r2/1", b"@r2/2"]
    assert [r.split(b"\n", 1)[1] for r in got] == [r.split(b"\n", 1)[1] for r in samout.reads_fastq_rule(READS, [0, 3, 4, 5], False)]


def test_names_and_fallbacks():
    names = {3: b"M01:7:x", 4: b"pair", 5: b"pair", 0: b""}                            # an empty entry is a fallback, as a missing one is
    got = samout.reads_fastq_rule(READS, [0, 3, 4, 5, 2 ** 32 + 7], False, names)
    assert [r.split(b"\n", 1)[0] for r in got] == [b"@r0", b"@M01:7:x", b"@pair", b"@pair", b"@r%d" % (2 ** 32 + 7)]
    got = samout.reads_fastq_rule(READS, [0, 3, 4, 5, 2 ** 32 + 7, 10 ** 10 + 1], True, names)
    assert [r.split(b"\n", 1)[0] for r in got] == [b"@r0/1", b"@M01:7:x/2", b"@pair/1", b"@pair/2", b"@r%d/2" % (2 ** 31 + 3), b"@r%d/2" % (5 * 10 ** 9)]
    assert samout.reads_fastq_rule(READS, [3], False, None) == samout.reads_fastq_rule(READS, [3], False) == samout.reads_fastq_rule(READS, [3], False, {})


def test_reads_may_be_a_sequence():
    seq = [(b"AC", b"\x01\x02"), (b"GT", b"\x03\x04")]
    assert samout.reads_fastq_rule(seq, [1], False) == [b"@r1\nGT\n+\n$%\n"]


# ------------------------------------------------------------------ the command's refusals
@pytest.fixture()
def no_engine(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an Engine was created")
    monkeypatch.setattr(cli, "Engine", refuse)
    monkeypatch.setattr("metamlst_amd.multigpu.launch_ranks", refuse, raising=False)


def files(tmp_path):
    for f in ("a.sam", "a.fastq", "b.fastq"):
        (tmp_path / f).write_bytes(b"" if f.endswith(".sam") else b"@a\nACGT\n+\nIIII\n")
    os.mkdir(tmp_path / "many")
    for f in ("x.fastq", "y.fastq"):
        (tmp_path / "many" / f).write_bytes(b"@a\nACGT\n+\nIIII\n")
    return {k: str(tmp_path / k) for k in ("a.sam", "a.fastq", "b.fastq", "many")}


@pytest.mark.parametrize("argv, words", [
    (["a.sam", "--alignments"], "--write-reads writes the engine's own alignments: with --alignments the file is the input"),
    (["a.fastq", "b.fastq"], "--write-reads takes one sample: several samples or a folder are typed without it"),
    (["many"], "--write-reads takes one sample: several samples or a folder are typed without it"),
    (["a.fastq", "--gpus", "2"], "--write-reads takes one GPU: a rank of --gpus N holds its own reads' alignments only"),
])
def test_cli_refuses_what_write_sam_refuses(tmp_path, capsys, no_engine, argv, words):
    f = files(tmp_path)
    argv = [f.get(x, x) for x in argv]
    assert cli.main(["type"] + argv + ["--write-reads", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]) == 1
    assert words in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "out")


def test_cli_refuses_world_size_above_one(tmp_path, capsys, no_engine, monkeypatch):
    f = files(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["type", f["a.fastq"], "--write-reads", "-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]) == 1
    assert "--write-reads takes one GPU" in capsys.readouterr().out


def test_read_names_and_md_beside_write_reads(tmp_path, capsys, no_engine):
    f = files(tmp_path)
    tail = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "out")]
    # --read-names is accepted with --write-reads alone: the command gets to the database, which is not there
    assert cli.main(["type", f["a.fastq"], "--write-reads", "--read-names"] + tail) == 1
    assert capsys.readouterr().out.startswith("Failed to connect to the database")
    # without any export flag its refusal keeps its words
    assert cli.main(["type", f["a.fastq"], "--read-names"] + tail) == 1
    assert "--read-names: it names the reads of an export: give --write-sam or --write-sam-all" in capsys.readouterr().out
    # its other refusals stay
    assert cli.main(["type", f["a.fastq"], "--long-reads", "--write-reads", "--read-names"] + tail) == 1
    assert "--read-names: --long-reads cuts reads into windows" in capsys.readouterr().out
    assert cli.main(["type", f["a.fastq"], f["b.fastq"], "--write-reads", "--read-names"] + tail) == 1
    assert "--read-names: it names the reads of one sample's export" in capsys.readouterr().out
    # --md still asks for one of the two SAM flags
    assert cli.main(["type", f["a.fastq"], "--write-reads", "--md"] + tail) == 1
    assert "--md: it adds MD:Z to the records of an export: give --write-sam or --write-sam-all" in capsys.readouterr().out
    assert cli.main(["type", f["a.fastq"], "--write-reads", "--write-sam", "--md"] + tail) == 1
    assert capsys.readouterr().out.startswith("Failed to connect to the database")
    # the flag alone, on a command line it goes with, gets past the checks
    assert cli.main(["type", f["a.fastq"], "--write-reads"] + tail) == 1
    assert capsys.readouterr().out.startswith("Failed to connect to the database")
    assert not os.path.exists(tmp_path / "out")


# ------------------------------------------------------------------ the C ABI
def test_the_three_symbols_are_in_the_built_library():
    lib = eng_mod.load_library()
    u64p, intp = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    want = {"mlst_reads_text_open": [C.c_int, C.c_uint64],
            "mlst_reads_text_next": [C.c_void_p, C.c_uint64, u64p, u64p, intp],      # (the text: a plain address, as every byte buffer of the library)
            "mlst_reads_text_close": []}
    for name, args in want.items():
        fn = getattr(lib, name)                                                          # AttributeError: the symbol is missing
        assert fn.restype is C.c_int, name
        assert len(fn.argtypes) == 1 + len(args) and list(fn.argtypes[1:]) == args, (name, fn.argtypes)
    # the header states them
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(eng_mod.__file__))), "include", "mlst.h")).read()
    assert "int mlst_reads_text_open(mlst_handle* h, int paired, uint64_t round_bytes" in text
    assert "int mlst_reads_text_next(mlst_handle* h, uint8_t* text, uint64_t cap, uint64_t* n_bytes, uint64_t* n_reads, int* done);" in text
    assert "int mlst_reads_text_close(mlst_handle* h);" in text
