"""The command side of the read chain (metamlst_amd/read_chain.py): what `cli type` answers to the flags of the six stages before any
engine or database is opened -- every stage against every condition it is accepted or refused under, every bad value, the order of
the refusals -- held to the answers recorded in tests/golden/cli_read_chain.json; then the table's apply, report and sums on a stub
engine.  No GPU and no library are needed.

The golden file is the project's own output: `PYTHONPATH=. python tests/test_read_chain_cli_host.py` writes it from the commit it is
run on (it was written from the commit before read_chain.py existed)."""
import argparse
import contextlib
import io
import json
import os
import sys

from metamlst_amd import cli, multigpu
from test_gpu_pair_bgzf import bgzf_blocks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_read_chain.json")

# every way of turning a stage on, in the order the stages refuse
FLAGS = {"prep": [["--trim5", "1"], ["--trim3", "1"], ["--trim-qual", "20"], ["--phred64"]],
         "adapters": [["--adapter", "illumina"]],
         "filter": [["--trim-poly-g"], ["--trim-poly-x"], ["--min-length", "30"], ["--max-n", "5"], ["--low-complexity", "30"], ["--min-mean-qual", "20"]],
         "stats": [["--read-stats"]], "dedup": [["--dedup"]], "overlap": [["--pair-overlap"]]}
SUMMING = {"prep", "adapters", "filter"}      # (accepted for a folder and --gpus N: their counters add up)
# the inputs that make the nine conditions hold, and the plain ones; (READS and what goes with them, WORLD_SIZE or None)
INPUTS = [(["s.fastq", "--alignments"], None), (["c.fa", "--contigs"], None), (["s.fastq", "--long-reads"], None), (["r.bam", "--long-bam-reads"], None),
          (["r.bam"], None), (["s.fastq", "t.fastq"], None), (["in"], None), (["s.fastq", "--gpus", "2"], None), (["s.fastq", "-2", "t.fastq", "--gpus", "2"], None),
          (["s.fastq"], 2), (["s.fastq"], None), (["s.fastq,t.fastq", "-2", "t.fastq"], None), (["s.fastq", "-2", "t.fastq"], None), (["s.fastq", "-2", "u.fastq"], None)]
BAD_VALUES = [["--trim-qual", "94"], ["--trim5", "70000"], ["--trim3=-1"],
              ["--adapter-min-overlap", "5"], ["--adapter-error-rate", "0.2"], ["--adapter", "AGAX"], ["--adapter", "illumina,NNNN"],
              ["--adapter", ",".join(["smallrna"] * 9)], ["--adapter", "A" * 65], ["--adapter", "illumina", "--adapter-min-overlap", "0"],
              ["--adapter", "illumina", "--adapter-error-rate", "0.6"],
              ["--pair-overlap-min", "20"], ["--pair-overlap-diff", "2"], ["--pair-overlap-rate", "0.1"], ["--pair-overlap", "--pair-overlap-min", "7"],
              ["--pair-overlap", "--pair-overlap-min", "321"], ["--pair-overlap", "--pair-overlap-diff", "65"], ["--pair-overlap", "--pair-overlap-rate", "0.6"],
              ["--trim-poly-g", "--trim-poly-x"], ["--poly-min", "12"], ["--poly-min", "12", "--min-length", "30"], ["--trim-poly-g", "--poly-min", "0"],
              ["--trim-poly-x", "--poly-min", "321"], ["--min-length", "0"], ["--min-length", "321"], ["--max-n", "4294967295"], ["--low-complexity", "101"],
              ["--low-complexity", "0"], ["--min-mean-qual", "94"]]
# a stage's bad value against the refusal of the stage in front of it and of the one behind it; --read-names in front of all, --md behind
ORDER = [["s.fastq", "--alignments", "--trim5", "1", "--adapter", "AGAX"], ["s.fastq", "--alignments", "--trim5", "70000", "--adapter", "illumina"],
         ["s.fastq", "--alignments", "--adapter", "illumina", "--min-length", "0"], ["s.fastq", "--alignments", "--adapter", "AGAX", "--min-length", "30"],
         ["in", "--min-length", "0", "--read-stats"], ["in", "--read-stats", "--dedup", "--pair-overlap-min", "20"], ["in", "--dedup", "--pair-overlap", "--pair-overlap-min", "7"],
         ["s.fastq", "--alignments", "--read-names", "--trim5", "1"], ["in", "--md", "--dedup"], ["in", "--write-sam", "--read-stats"], ["s.fastq", "--md", "--trim5", "70000"]]


def command_lines() -> list:
    """[(arguments behind `type`, WORLD_SIZE or None)]: the fixed list"""
    out = []
    for stage, ways in FLAGS.items():
        for flags in ways:
            for reads, world in INPUTS:
                if world is None or stage not in SUMMING:      # (a rank that is not refused goes on to open its GPU)
                    out.append((reads + flags, world))
    out += [(["s.fastq", "-2", "t.fastq"] + flags, None) for flags in BAD_VALUES]
    names = list(FLAGS)
    for reads in (["s.fastq", "--alignments"], ["in"]):
        out += [(reads + FLAGS[x][0] + FLAGS[y][0], None) for i, x in enumerate(names) for y in names[i + 1:]]
    out += [(args, None) for args in ORDER]
    every = [f for ways in FLAGS.values() for f in ways[0]]
    return out + [(["s.fastq", "-2", "t.fastq"] + every + ["--write-sam", "--read-names", "--md"], None)]


def answers(folder: str, read_out) -> dict:
    """{command line: [exit code, stdout]} of the fixed list, run in folder against a database that does not exist; read_out() gives
    what was printed since it was last called.  --gpus N that is not refused ends in launch_ranks, which is replaced by a line."""
    here, launch, world_was = os.getcwd(), multigpu.launch_ranks, os.environ.pop("WORLD_SIZE", None)
    os.chdir(folder)
    for name, text in (("s.fastq", b"@r 1\nACGT\n+\nIIII\n"), ("t.fastq", b"@r 2\nACGT\n+\nIIII\n"), ("u.fastq", b"@other 2\nACGT\n+\nIIII\n"), ("c.fa", b">c\nACGT\n"),
                       ("in/f0.fastq", b"@r\nACGT\n+\nIIII\n"), ("in/f1.fastq", b"@r\nACGT\n+\nIIII\n"), ("r.bam", b"".join(bgzf_blocks(b"BAM\x01" + bytes(8))))):
        os.makedirs(os.path.dirname(name) or ".", exist_ok=True)
        with open(name, "wb") as f:
            f.write(text)
    multigpu.launch_ranks = lambda n, argv: print("launch_ranks(%d)" % n) or 0
    out = {}
    try:
        for args, world in command_lines():
            if world is not None:
                os.environ["WORLD_SIZE"] = str(world)
            try:
                rc = cli.main(["type"] + args + ["-d", "none.db", "-o", "o"])
            finally:
                os.environ.pop("WORLD_SIZE", None)
            out[("WORLD_SIZE=%d " % world if world else "") + " ".join(args)] = [rc, read_out()]
        assert not os.path.exists("o")      # (refused, or no database: nothing is written)
    finally:
        multigpu.launch_ranks = launch
        os.chdir(here)
        if world_was is not None:
            os.environ["WORLD_SIZE"] = world_was
    return out


def test_the_command_answers_as_recorded(tmp_path, capsys):
    got = answers(str(tmp_path), lambda: capsys.readouterr().out)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for line in want:
        assert got[line] == want[line], line
    for stage, ways in FLAGS.items():      # one accepted line per stage, at the least
        reads = ["s.fastq", "-2", "t.fastq"] if stage == "overlap" else ["s.fastq"]
        assert got[" ".join(reads + ways[0])][0] == 1 and got[" ".join(reads + ways[0])][1].startswith("Failed to connect to the database"), stage


# ------------------------------------------------------------------ the table on a stub engine
try:      # (the commit the golden file was written from has no such module)
    from metamlst_amd import read_chain
except ImportError:
    read_chain = None
PREP = {"shortened": 5, "bases_removed": 50, "emptied": 1}
ADAPT = {"trimmed": 7, "bases_removed": 70, "emptied": 2, "per_adapter": [3, 4]}
FILTER = {"tail_trimmed": 1000, "tail_bases": 43210, "per_letter": [1, 2, 990, 7], "tail_emptied": 3, "failed_short": 40, "failed_n": 30, "failed_complexity": 20,
          "failed_quality": 10, "filtered_bases": 9876}
OVERLAP = {"pairs": 1000, "overlapping": 333, "trimmed_pairs": 300, "reads_trimmed": 590, "bases_removed": 12345, "emptied": 2, "insert_hist": [0] * 100 + [333] + [0] * 923}
DEDUP = {"reads": 2000, "units": 1000, "duplicates": 333, "reads_removed": 666, "bases_removed": 99900, "distinct": 667, "clashes": 0, "slots": 4096, "levels": [600, 50, 10, 4, 2, 1, 0, 0]}


class StubEngine:
    """records the set_read_* calls and answers read_*_info() from the fixed dicts above; no library is loaded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("set_read_"):
            return lambda *args, **kw: self.calls.append((name, args, kw))
        raise AttributeError(name)

    def read_prep_info(self):
        return dict(PREP)

    def read_adapters_info(self):
        return dict(ADAPT)

    def read_filter_info(self):
        return dict(FILTER)

    def read_pair_overlap_info(self):
        return dict(OVERLAP)

    def read_dedup_info(self):
        return dict(DEDUP)

    def read_stats(self):
        from metamlst_amd.fastq import read_stats
        s = read_stats(b"@a\nACGTN\n+\nIIII!\n@b\nGGCCA\n+\nIIIII\n")
        return {"raw": s, "prepared": s, "prepared_counted": False}


def chain_of(*args):
    """the chain of `type` + args, as the command makes it"""
    a = cli._type_parser(argparse.ArgumentParser().add_subparsers()).parse_args(list(args) + ["-d", "none.db"])
    return read_chain.parse(a, cli.expand_samples(a.READS))


def all_on(tmp_path):
    (tmp_path / "s.fastq").write_bytes(b"@r 1\nACGT\n+\nIIII\n")
    (tmp_path / "t.fastq").write_bytes(b"@r 2\nACGT\n+\nIIII\n")
    return chain_of(str(tmp_path / "s.fastq"), "-2", str(tmp_path / "t.fastq"), "--trim5", "1", "--trim3", "2", "--trim-qual", "20", "--phred64", "--adapter", "illumina,ACGTAC",
                    "--adapter-min-overlap", "5", "--adapter-error-rate", "0.2", "--read-stats", "--dedup", "--pair-overlap", "--pair-overlap-min", "20",
                    "--pair-overlap-rate", "0.1", "--trim-poly-g", "--poly-min", "12", "--min-length", "30", "--max-n", "0")


def test_apply_makes_the_calls_of_the_command_before_it(tmp_path):
    eng = StubEngine()
    read_chain.apply(eng, all_on(tmp_path))
    assert eng.calls == [("set_read_prep", (), {"trim5": 1, "trim3": 2, "trim_qual": 20, "phred64": True}),
                         ("set_read_adapters", (), {"adapters": ["AGATCGGAAGAGC", "ACGTAC"], "min_overlap": 5, "error_permille": 200}),
                         ("set_read_stats", (True,), {}), ("set_read_dedup", (True,), {}),
                         ("set_read_pair_overlap", (True,), {"min_overlap": 20, "max_mismatches": 5, "error_permille": 100}),
                         ("set_read_filter", (), {"poly": "G", "poly_min": 12, "min_length": 30, "max_n": 0, "complexity": 0, "mean_qual": 0})]
    eng = StubEngine()
    read_chain.apply(eng, chain_of("x.fastq", "--dedup"))
    assert eng.calls == [("set_read_dedup", (True,), {})]
    eng = StubEngine()
    read_chain.apply(eng, chain_of("x.fastq"))
    assert eng.calls == []


def test_report_prints_the_six_stages_in_their_order(tmp_path, capsys):
    chain = all_on(tmp_path)
    assert sorted(chain) == ["adapters", "dedup", "filter", "overlap", "prep", "stats"]
    read_chain.report(StubEngine(), chain, True, False, str(tmp_path / "s"))
    said = capsys.readouterr().out.splitlines()
    assert said == ["read preparation: 5 reads shortened, 50 bases removed, 1 reads left without a base",
                    "adapter removal: 7 reads cut, 70 bases removed, 2 reads left without a base (AGATCGGAAGAGC 3, ACGTAC 4)",
                    cli.read_filter_line(FILTER), cli.read_pair_overlap_line(OVERLAP)] + cli.read_stats_lines(StubEngine().read_stats()) + [cli.read_dedup_line(DEDUP, True)]
    assert said[4].startswith("read statistics (raw, side 0): 2 reads, 10 bases") and len(said) == 6
    with open(tmp_path / "s.readstats.tsv", "rb") as f:
        table = f.read()
    os.remove(tmp_path / "s.readstats.tsv")
    read_chain.report(StubEngine(), chain, True, True, str(tmp_path / "s"))
    assert capsys.readouterr().out == ""
    with open(tmp_path / "s.readstats.tsv", "rb") as f:      # the file is written all the same
        assert f.read() == table and table


def test_one_sum_for_every_stage_and_the_stages_that_sum():
    zero = {k: [0] * len(v) if isinstance(v, list) else 0 for k, v in FILTER.items()}
    assert read_chain.add_infos(FILTER, FILTER) == {k: [2 * x for x in v] if isinstance(v, list) else 2 * v for k, v in FILTER.items()}
    assert read_chain.add_infos(zero, FILTER) == FILTER and cli._sum_filter_infos([FILTER, FILTER, zero]) == read_chain.add_infos(FILTER, FILTER)
    other = {"trimmed": 1, "bases_removed": 13, "emptied": 0, "per_adapter": [1, 0]}
    assert read_chain.add_infos(ADAPT, other) == {"trimmed": 8, "bases_removed": 83, "emptied": 2, "per_adapter": [4, 4]}
    assert ADAPT["per_adapter"] == [3, 4] and other["per_adapter"] == [1, 0]      # (the inputs stay as they are)
    assert read_chain.add_infos(PREP, PREP) == {"shortened": 10, "bases_removed": 100, "emptied": 2}
    assert {s.key for s in read_chain.SUMMING} == {"prep", "adapters", "filter"}
    zeros = {s.key: s.zero(cfg) for s, cfg in ((s, {"adapters": ["A", "C", "G"]}) for s in read_chain.SUMMING)}
    assert zeros == {"prep": {"shortened": 0, "bases_removed": 0, "emptied": 0}, "adapters": {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0, 0, 0]},
                     "filter": zero}


if __name__ == "__main__":      # write the golden file from the commit this is run on
    import tempfile
    box = io.StringIO()

    def read_out():
        text = box.getvalue()
        box.seek(0)
        box.truncate()
        return text
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(box):
        got = answers(tmp, read_out)
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d command lines -> %s" % (len(got), GOLDEN), file=sys.stderr)
