"""fastq.window_cut / fastq.cut_windows, the rule mlst_set_read_window applies on the device (include/mlst.h; csrc/read_window.h), pinned
by hand; the refusals and bad values of `cli type --cut-front / --cut-right / --cut-tail`, each with its sentence and before any GPU use;
the three symbols in header and engine.py; the command's line on a stub engine.  No GPU is needed.  The rule is the project's own
(modelled on fastp's cut_front / cut_right / cut_tail); nothing here claims fastp's or Trimmomatic's bytes."""
import argparse
import os

import pytest

from metamlst_amd import cli, read_chain
from metamlst_amd import engine as eng_mod
from metamlst_amd.fastq import WINDOW_COUNTERS, check_read_window, cut_windows, prep_fastq, qtrim_len, window_cut
from test_gpu_pair_bgzf import bgzf_blocks

F, R, T = (4, 20), (4, 20), (4, 20)
DIP = [40] * 10 + [2] * 4 + [40] * 10
# (Phred values, front, right, tail, f, the end behind right, e): values [f, e) remain -- every number written by hand, none produced
# by the rule.  A window of four at Q 20 needs a sum of 80
KNOWN = [
    # front: n = 0, 1, W - 1, W, W + 1; a sum of exactly Q * w passes, one less fails
    ([], F, None, None, 0, 0, 0),
    ([40], F, None, None, 0, 1, 1),                                    # n < W: the window is the read
    ([19], F, None, None, 1, 1, 1),                                    # ... and fails: left without a base, f = n
    ([20, 20, 20], F, None, None, 0, 3, 3),                            # 60 >= 20 * 3
    ([20, 20, 19], F, None, None, 3, 3, 3),                            # 59
    ([20, 20, 20, 20], F, None, None, 0, 4, 4),                        # 80
    ([20, 20, 20, 19], F, None, None, 4, 4, 4),                        # 79
    ([19, 20, 20, 20, 21], F, None, None, 1, 5, 5),                    # 79, then 81
    ([19, 20, 20, 20, 20], F, None, None, 1, 5, 5),                    # 79, then 80
    ([19, 20, 20, 20, 19], F, None, None, 5, 5, 5),                    # 79, 79: no window passes
    ([2, 2, 2, 40, 40, 40, 40, 2], F, None, None, 1, 8, 8),            # 46, then 84: the passing window keeps its two bad first values
    # W = 1: bases below Q are dropped from that end (Trimmomatic's LEADING / TRAILING)
    ([5, 19, 20, 3, 40], (1, 20), None, None, 2, 5, 5),
    ([40, 3, 20, 19, 5], None, None, (1, 20), 0, 5, 3),
    ([5, 19, 20, 3, 40, 19], (1, 20), None, (1, 20), 2, 6, 5),
    ([19, 19], (1, 20), None, (1, 20), 2, 2, 2),
    # right: a dip in the middle; the good bases at the front of the first bad window stay
    (DIP, None, R, None, 0, 10, 10),                                   # 122, 84, then 46 at s = 9: q[9] = 40 stays
    ([30, 30, 30, 30, 30, 30, 5, 5, 30, 30], None, R, None, 0, 6, 6),  # 95, then 70 at s = 4: two good bases stay
    ([40, 40, 40, 40, 0, 0, 0, 40, 40], None, R, None, 0, 4, 4),       # 120, 80 (passes), then 40 at s = 3: one stays
    ([40, 40, 40, 40, 10, 40, 10, 10, 40], None, R, None, 0, 4, 4),    # 130, 130, 100, then 70 at s = 4, which begins on a bad base: none stays
    ([20, 20, 19], None, R, None, 0, 2, 2),                            # n = W - 1: 59 < 60
    ([20, 20, 20], None, R, None, 0, 3, 3),
    ([20, 20, 20, 19], None, R, None, 0, 3, 3),                        # n = W
    ([20, 20, 20, 20, 19], None, R, None, 0, 4, 4),                    # n = W + 1: only the last window fails
    ([20, 20, 20, 20, 20], None, R, None, 0, 5, 5),
    ([19], None, R, None, 0, 0, 0),                                    # n = 1: emptied by right
    ([2] * 9, None, R, None, 0, 0, 0),
    # tail
    ([40] * 8 + [2, 2, 2], None, None, T, 0, 11, 10),                  # 46, then 84: the passing window keeps its bad last values
    ([19, 20, 20], None, None, T, 0, 3, 0),                            # n = W - 1: 59
    ([20, 20, 20], None, None, T, 0, 3, 3),
    ([20], None, None, T, 0, 1, 1),                                    # n = 1
    ([20, 20, 20, 20], None, None, T, 0, 4, 4),                        # n = W: 80
    ([20, 20, 20, 19], None, None, T, 0, 4, 0),                        # 79: emptied by tail
    ([20, 20, 20, 20, 19], None, None, T, 0, 5, 4),                  # n = W + 1: 79, then 80
    ([19, 20, 20, 20, 19], None, None, T, 0, 5, 0),
    ([], None, None, T, 0, 0, 0),
    # front empties the read: right and tail see nothing
    ([5, 5, 5, 5, 5, 5], F, R, T, 6, 6, 6),
    # tail empties what right left
    ([25, 25, 25, 25, 25, 0, 0, 0, 0], None, R, (2, 30), 0, 5, 0),      # right: 75 at s = 2, three stay; tail: every pair is 50 < 60
    # all three: LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15
    ([2, 2, 30, 30, 30, 30, 30, 30, 10, 10, 10, 10, 30, 2], (1, 3), (4, 15), (1, 3), 2, 8, 8),      # right: 100, 80, 60 (passes), 40 at s = 8
    # all three with different (W, Q): front 39, 50 -> f = 1; right [30, 30, 0] = 60 < 75 at s = 13, two stay; tail 60, 60, then 70
    ([9, 30, 20, 30, 30, 30, 30, 30, 30, 40, 20, 40, 30, 30, 30, 0, 40], (2, 20), (3, 25), (2, 35), 1, 15, 13),
]


def zero_info(**kw) -> dict:
    return dict(dict.fromkeys(WINDOW_COUNTERS, 0), **kw)


def rec(name: str, seq: bytes, qual: bytes, eol: bytes = b"\n") -> bytes:
    return b"@" + name.encode() + eol + seq + eol + b"+" + eol + qual + eol


def bases(n: int) -> bytes:
    return (b"ACGTTGCA" * 41)[:n]


def info_of(rows) -> dict:
    """the counters of the rows, from the numbers written by hand"""
    info = zero_info()
    for q, _, _, _, f, er, e in rows:
        n = len(q)
        for name, cut in (("front", f), ("right", n - er), ("tail", er - e)):
            info[name + "_reads"] += cut > 0
            info[name + "_bases"] += cut
        info["shortened"] += e - f != n
        info["emptied"] += e - f != n and e == f
    return info


# ------------------------------------------------------------------ the rule
def test_known_answers():
    for k, (q, front, right, tail, f, er, e) in enumerate(KNOWN):
        assert window_cut(q, front, right, tail) == (f, e), (k, q)
        assert window_cut(q, front, right, None) == (f, er), (k, q)      # (the end behind right is what it is without tail)
        s = bases(len(q))
        ql = bytes(v + 33 for v in q)
        text, info = cut_windows(rec("r", s, ql), front, right, tail)
        assert text == rec("r", s[f:e], ql[f:e]), (k, q)
        assert info == info_of([KNOWN[k]]), (k, info)


def test_the_table_covers_what_it_says():
    for which in (1, 2, 3):
        alone = [row for row in KNOWN if [x is not None for x in row[1:4]] == [j == which for j in (1, 2, 3)]]
        assert {len(row[0]) for row in alone} >= {1, 3, 4, 5} | ({0} if which != 2 else set()), which      # n = 1, W - 1, W, W + 1
    assert any(all(x is not None for x in row[1:4]) and 0 < row[4] < row[6] < row[5] < len(row[0]) for row in KNOWN)      # all three cut one read
    assert any(row[1] and row[4] == len(row[0]) > 0 for row in KNOWN) and any(row[3] and row[6] == row[4] < row[5] for row in KNOWN)
    assert qtrim_len(DIP, 20) == len(DIP) and window_cut(DIP, right=R) == (0, 10)      # the dip that --trim-qual keeps


def test_a_window_of_one_drops_the_bases_below_q_from_that_end():
    q = [7, 30, 2, 29, 30, 31, 3, 30, 30, 29, 12]
    for Q in (1, 3, 13, 30, 31, 32):
        front = next((i for i, v in enumerate(q) if v >= Q), len(q))
        back = next((i + 1 for i in range(len(q) - 1, -1, -1) if q[i] >= Q), 0)
        assert window_cut(q, front=(1, Q)) == (front, len(q)), Q
        assert window_cut(q, tail=(1, Q)) == (0, back), Q
        assert window_cut(q, front=(1, Q), tail=(1, Q)) == ((front, back) if front < len(q) else (len(q), len(q))), Q


def test_the_counters_of_the_table_as_one_text():
    for front, right, tail in {tuple(row[1:4]) for row in KNOWN}:
        rows = [row for row in KNOWN if tuple(row[1:4]) == (front, right, tail)]
        text = b"".join(rec("r%d" % k, bases(len(row[0])), bytes(v + 33 for v in row[0])) for k, row in enumerate(rows))
        want = b"".join(rec("r%d" % k, bases(len(row[0]))[row[4]:row[6]], bytes(v + 33 for v in row[0][row[4]:row[6]])) for k, row in enumerate(rows))
        assert cut_windows(text, front, right, tail) == (want, info_of(rows)), (front, right, tail)
        assert cut_windows(text.replace(b"\n", b"\r\n"), front, right, tail) == (want, info_of(rows))      # CRLF in, LF out
    everything = info_of([row for row in KNOWN if row[1:4] == (F, R, T)] + [KNOWN[-1], KNOWN[-2], KNOWN[-3]])
    assert all(everything[name] > 0 for name in WINDOW_COUNTERS), everything
    text = rec("a", b"ACGT", b"IIII")
    assert cut_windows(text) == (text, zero_info())
    with pytest.raises(ValueError, match="not a whole number of 4-line records"):
        cut_windows(b"@a\nACGT\n+\n", right=R)
    with pytest.raises(ValueError, match="different sequence and quality lengths"):
        cut_windows(rec("a", b"ACGT", b"II"), right=R)


def test_the_phred_base_and_the_clamps():
    # Phred+64: 'h' is 40, '@' 0 -- 160, 120, 80, then 40 at s = 3, one stays; the characters are written back at +33, as prep_fastq writes them
    text = rec("r", b"ACGTACGT", b"hhhh@@@@")
    assert cut_windows(text, right=R, phred64=True) == (rec("r", b"ACGT", b"IIII"), zero_info(shortened=1, right_reads=1, right_bases=4))
    assert cut_windows(text, right=R) == (text, zero_info())      # read as Phred+33 they are 71 and 31: every window passes
    assert cut_windows(text, right=R, phred64=True) == cut_windows(prep_fastq(text, phred64=True)[0], right=R)
    # a character below the base counts 0: under +64 '5' (53) and '?' (63); under +33 a blank (32) -- 0 + 2 reaches 2 * 1, -1 + 2 would not
    assert cut_windows(rec("r", b"ACGT", b"hh5?"), tail=(1, 1), phred64=True) == (rec("r", b"AC", b"II"), zero_info(shortened=1, tail_reads=1, tail_bases=2))
    assert cut_windows(rec("r", b"AC", b" #"), front=(2, 1)) == (rec("r", b"AC", b" #"), zero_info())
    assert cut_windows(rec("r", b"AC", b" \""), front=(2, 1)) == (rec("r", b"", b""), zero_info(shortened=1, front_reads=1, front_bases=2, emptied=1))
    # a character above base + 127 counts 127: 127 + 0 < 64 * 2, where 222 + 0 would pass; the first value stays
    assert cut_windows(rec("r", b"AC", b"\xff!"), right=(2, 64)) == (rec("r", b"A", b"\xff"), zero_info(shortened=1, right_reads=1, right_bases=1))
    assert cut_windows(rec("r", b"AC", b"\xff!"), right=(2, 63)) == (rec("r", b"AC", b"\xff!"), zero_info())      # 127 >= 126


def test_the_settings_that_are_refused():
    for bad, why in (({"front": (0, 20)}, "front window 0 is outside 1..320"), ({"right": (321, 20)}, "right window 321 is outside 1..320"),
                     ({"tail": (4, 0)}, "tail quality 0 is outside 1..93"), ({"front": (4, 94)}, "front quality 94 is outside 1..93"),
                     ({"right": (4,)}, r"right \(4,\): an operation is \(W, Q\)"), ({"tail": 4}, r"tail 4: an operation is \(W, Q\)"),
                     ({"right": (4.5, 20)}, "an operation is"), ({"front": ("a", "b")}, "an operation is"), ({"tail": (-1, 20)}, "tail window -1 is outside 1..320")):
        with pytest.raises(ValueError, match=why):
            check_read_window(**bad)
        with pytest.raises(ValueError, match=why):
            cut_windows(rec("a", b"ACGT", b"IIII"), **bad)
        with pytest.raises(ValueError, match=why):
            window_cut([40] * 4, **bad)
    assert check_read_window() == [0] * 6 and check_read_window((1, 1), (320, 93), [4, 15]) == [1, 1, 320, 93, 4, 15]
    assert check_read_window(tail=(4, 20)) == [0, 0, 0, 0, 4, 20]


# ------------------------------------------------------------------ the ABI
def test_the_symbols_are_declared_and_bound():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlst.h")) as f:
        header = f.read()
    for name in ("mlst_set_read_window", "mlst_get_read_window", "mlst_read_window_info"):
        assert "int %s(mlst_handle*" % name in header, name
    assert "typedef struct { uint32_t front_w, front_q, right_w, right_q, tail_w, tail_q; } mlst_read_window;" in header
    assert all(hasattr(eng_mod.Engine, name) for name in ("set_read_window", "get_read_window", "read_window_info"))


# ------------------------------------------------------------------ the command
HEAD = "quality windows (--cut-front, --cut-right, --cut-tail): "
WAYS = (["--cut-front", "4,20"], ["--cut-right", "4,20"], ["--cut-tail", "1,3"])


def test_cli_refusals_each_with_its_reason(tmp_path, monkeypatch, capsys):
    """before any GPU use: none of them needs a database that exists"""
    (tmp_path / "s.fastq").write_bytes(b"@r 1\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r 2\nACGT\n+\nIIII\n")
    (tmp_path / "c.fa").write_bytes(b">c\nACGT\n")
    os.makedirs(tmp_path / "in")
    for k in range(2):
        (tmp_path / "in" / ("f%d.fastq" % k)).write_bytes(b"@r\nACGT\n+\nIIII\n")
    bam = tmp_path / "r.bam"
    bam.write_bytes(b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    tail_ = ["-d", str(tmp_path / "none.db"), "-o", str(tmp_path / "o")]
    for flags in WAYS:
        for args, why in ((["s.fastq", "--alignments"], "with --alignments the records are what they are: the file holds alignments, not reads to cut"),
                          (["c.fa", "--contigs"], "--contigs cuts assemblies into windows, and an assembly has no qualities"),
                          (["s.fastq", "--long-reads"], "--long-reads cuts reads into windows, and a window is cut from the record as it stands"),
                          ([str(bam), "--long-bam-reads"], "--long-bam-reads cuts reads into windows, and a window is cut from the record as it stands"),
                          ([str(bam)], "a reads BAM stores raw Phred and its own strand, and its reads are not cut: FASTQ input only"),
                          (["in"], "several samples or a folder are typed without them (the rule is per read: summing the counters of the samples is the follow-up)"),
                          (["s.fastq", "t.fastq"], "several samples or a folder are typed without them (the rule is per read: summing the counters of the samples is the follow-up)"),
                          (["s.fastq", "--gpus", "2"], "one GPU: the counters of the ranks of --gpus N are not summed yet (the follow-up)")):
            assert cli.main(["type"] + args + flags + tail_) == 1, (args, flags)
            assert HEAD + why in capsys.readouterr().out, (args, flags)
    # a front cut and the mates' overlap; right and tail go with it
    assert cli.main(["type", "s.fastq", "-2", "t.fastq", "--pair-overlap", "--cut-front", "4,20"] + tail_) == 1
    said = capsys.readouterr().out
    assert said.startswith(HEAD + "--cut-front goes with no --pair-overlap, which places the insert's end by --trim5 alone") and "true insert bases" in said
    for flag in ("--cut-front", "--cut-right", "--cut-tail"):
        for value, why in (("4", "%s W,Q takes two numbers, not '4'"), ("4,", "%s W,Q takes two numbers, not '4,'"), ("a,b", "%s W,Q takes two numbers, not 'a,b'"),
                           ("4,20,1", "%s W,Q takes two numbers, not '4,20,1'"), ("0,20", "%s W,Q: a window holds 1 to 320 bases, not 0"),
                           ("321,20", "%s W,Q: a window holds 1 to 320 bases, not 321"), ("4,0", "%s W,Q: a quality is 1 to 93, not 0"), ("4,94", "%s W,Q: a quality is 1 to 93, not 94")):
            assert cli.main(["type", "s.fastq", flag, value] + tail_) == 1, (flag, value)
            assert capsys.readouterr().out == why % flag + "\n", (flag, value)
    # accepted where --adapter is accepted on one sample: the command goes on to the database, which does not exist
    every = ["--cut-front", "1,3", "--cut-tail", "1,3", "--cut-right", "4,15", "--min-length", "36"]
    for args in (["s.fastq"] + every, ["s.fastq,t.fastq"] + every, ["s.fastq", "-2", "t.fastq"] + every, ["s.fastq", "-2", "t.fastq", "--pair-overlap", "--cut-right", "320,93", "--cut-tail", "1,1"],
                 ["s.fastq", "-2", "t.fastq", "--cut-front", "4,20", "--trim5", "1", "--trim-qual", "20", "--phred64", "--adapter", "illumina", "--read-stats", "--dedup", "--trim-poly-g",
                  "--write-sam", "--write-sam-all", "--write-reads", "--read-names"]):
        assert cli.main(["type"] + args + tail_) == 1, args
        assert capsys.readouterr().out.startswith("Failed to connect to the database"), args
    assert read_chain.WINDOW.parse(argparse.Namespace(cut_right="4,15")) == {"front": None, "right": (4, 15), "tail": None}
    assert read_chain.WINDOW.parse(argparse.Namespace(cut_front="1,3", cut_tail=" 320, 93")) == {"front": (1, 3), "right": None, "tail": (320, 93)}
    assert read_chain.WINDOW.parse(argparse.Namespace()) is None
    assert not os.path.exists(tmp_path / "o")


def test_the_stage_stands_directly_behind_the_preparation():
    for order in (read_chain.STAGES, read_chain.REFUSAL_ORDER, read_chain.REPORT_ORDER):
        assert order[0] is read_chain.PREP and order[1] is read_chain.WINDOW and len(order) == 7
    assert read_chain.WINDOW not in read_chain.SUMMING
    assert (read_chain.WINDOW.key, read_chain.WINDOW.setter, read_chain.WINDOW.counters) == ("window", "set_read_window", "read_window_info")


INFO = {"shortened": 1234, "front_reads": 56, "front_bases": 789, "right_reads": 1000, "right_bases": 43210, "tail_reads": 7, "tail_bases": 8, "emptied": 9}
LINE = "quality windows: 1234 reads cut (front 56 reads / 789 bases, right 1000 reads / 43210 bases, tail 7 reads / 8 bases), 9 reads left without a base"


class StubEngine:
    """records the set_read_* calls and answers read_*_info() from fixed dicts; no library is loaded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("set_read_"):
            return lambda *args, **kw: self.calls.append((name, args, kw))
        raise AttributeError(name)

    def read_prep_info(self):
        return {"shortened": 5, "bases_removed": 50, "emptied": 1}

    def read_window_info(self):
        return dict(INFO)

    def read_adapters_info(self):
        return {"trimmed": 7, "bases_removed": 70, "emptied": 2, "per_adapter": [7]}


def test_the_commands_line_on_a_stub_engine(tmp_path, capsys):
    assert read_chain.read_window_line(INFO) == LINE and cli.read_window_line is read_chain.read_window_line
    a = cli._type_parser(argparse.ArgumentParser().add_subparsers()).parse_args(["x.fastq", "--trim5", "1", "--cut-front", "1,3", "--cut-right", "4,15", "--adapter", "illumina", "-d", "none.db"])
    chain = read_chain.parse(a, cli.expand_samples(a.READS))
    assert list(chain) == ["prep", "window", "adapters"] and chain["window"] == {"front": (1, 3), "right": (4, 15), "tail": None}
    eng = StubEngine()
    read_chain.apply(eng, chain)
    assert eng.calls[:2] == [("set_read_prep", (), {"trim5": 1, "trim3": 0, "trim_qual": 0, "phred64": False}),
                             ("set_read_window", (), {"front": (1, 3), "right": (4, 15), "tail": None})] and eng.calls[2][0] == "set_read_adapters"
    read_chain.report(eng, chain, False, False, str(tmp_path / "s"))
    said = capsys.readouterr().out.splitlines()
    assert said[0].startswith("read preparation: ") and said[1] == LINE and said[2].startswith("adapter removal: ") and len(said) == 3
    read_chain.report(eng, chain, False, True, str(tmp_path / "s"))
    assert capsys.readouterr().out == ""
