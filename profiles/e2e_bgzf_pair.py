#!/usr/bin/env python3
"""bgzip'd mate files -> pass-1 statistics: the same reads (a) as ONE bgzip'd file through Engine.submit_fastq_bgzf_file and
(b) as two mate files through Engine.submit_fastq_bgzf_pair_files (mlst_submit_fastq_bgzf_pair: inflated and paired on the
GPU), both read from files; (b)'s statistics must equal those of the mates as text through mlst_submit_fastq_pair.  The old
route of bgzip'd mates (fastq.pair_chunks: host gzip + host pairing -> submit_fastq_pair) is timed on a slice.
    python profiles/e2e_bgzf_pair.py [reads] [level] [database: small | cfg3]"""
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd import fastq, synth  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402


def block(args):
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000      # reads in all (N / 2 pairs)
LEVEL = int(sys.argv[2]) if len(sys.argv) > 2 else 6
DB = sys.argv[3] if len(sys.argv) > 3 else "small"
N -= N % 2
d = tempfile.mkdtemp()
if DB == "cfg3":      # bench.py's cfg3 database: 150 species x 7 loci x 300 alleles
    db = synth.make_full_db(d + "/e.db", n_species=150, alleles_per_locus=300, n_profiles=200)
    sp = db.species[0]
else:
    db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
    sp = "ecoli"
idx = load_index(db.path)
g, _ = synth.make_genome(db, sp, db.profiles[sp][3], size=1_000_000)
L = 150
rec = 16 + 2 * L
rows = np.empty((N, rec), np.uint8)
for at in range(0, N, 1 << 20):
    c = min(1 << 20, N - at)
    b, q = synth.sample_reads(g, c, seed=synth.SEED + at)
    rows[at:at + c, 12:12 + L] = b
    rows[at:at + c, 15 + L:15 + 2 * L] = q
rows[:, :12] = np.frombuffer(b"@r000000000\n", np.uint8)      # fixed-width names: read 2k and 2k + 1 (mates) share name k
num = np.arange(N) // 2
for k in range(9):
    rows[:, 10 - k] = 48 + (num // 10 ** k) % 10
rows[:, 12 + L] = 10; rows[:, 13 + L] = ord("+"); rows[:, 14 + L] = 10; rows[:, 15 + 2 * L] = 10
raw1, raw2 = rows[0::2].tobytes(), rows[1::2].tobytes()
del rows
t0 = time.perf_counter()
with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
    parts1 = list(ex.map(block, [(raw1[at:at + 65280], LEVEL) for at in range(0, len(raw1), 65280)]))
    parts2 = list(ex.map(block, [(raw2[at:at + 65280], LEVEL) for at in range(0, len(raw2), 65280)]))
eof = block((b"", LEVEL))
p1, p2, p12 = d + "/s_R1.fastq.gz", d + "/s_R2.fastq.gz", d + "/s.fastq.gz"
with open(p1, "wb") as f:
    f.write(b"".join(parts1) + eof)
with open(p2, "wb") as f:
    f.write(b"".join(parts2) + eof)
with open(p12, "wb") as f:      # the same reads in one file: R1's blocks, then R2's
    f.write(b"".join(parts1) + b"".join(parts2) + eof)
del parts1, parts2
print("compressed in %.1f s: %.1f + %.1f MB -> %.1f + %.1f MB" % (time.perf_counter() - t0, len(raw1) / 1e6, len(raw2) / 1e6,
      os.path.getsize(p1) / 1e6, os.path.getsize(p2) / 1e6), file=sys.stderr, flush=True)

out = {"reads": N, "pairs": N // 2, "database": DB, "text_bytes": len(raw1) + len(raw2), "bgzf_bytes": os.path.getsize(p1) + os.path.getsize(p2), "level": LEVEL}
eng = Engine(0)
eng.load_reference(idx)


def key(st):
    return (st.sum_score.tobytes(), st.n_hits.tobytes(), st.locus_len_sum.tobytes(), st.locus_first.tobytes(), tuple(int(x) for x in st.counters[:4]))


def timed(name, fn, runs=3):
    ts = []
    for _ in range(runs):
        eng.reset_sample()
        eng.synchronize()
        t0 = time.perf_counter()
        n = fn()
        st = eng.stats()
        ts.append(time.perf_counter() - t0)
    t = min(ts[1:]) if len(ts) > 1 else ts[0]
    out[name] = {"s": round(t, 4), "Mreads_per_s": round(n / t / 1e6, 1), "reads": int(n), "all_runs_s": [round(x, 4) for x in ts]}
    print(name, out[name], file=sys.stderr, flush=True)
    return st


# the reference statistics: the mates as text, 2 M records per file and call
per = 2_000_000 * rec
st_text = timed("text_pair", lambda: sum(eng.submit_fastq_pair(raw1[a:a + per], raw2[a:a + per]) for a in range(0, len(raw1), per)), runs=1)
st_one = timed("bgzf_one_file", lambda: eng.submit_fastq_bgzf_file(p12))
st_pair = timed("bgzf_pair_files", lambda: eng.submit_fastq_bgzf_pair_files(p1, p2))
assert key(st_pair) == key(st_text), "the paired bgzip path differs from the text path"
assert out["bgzf_pair_files"]["reads"] == N and out["bgzf_one_file"]["reads"] == N
out["pair_over_one_file"] = round(out["bgzf_pair_files"]["Mreads_per_s"] / out["bgzf_one_file"]["Mreads_per_s"], 3)

# the old route on a slice: fastq.pair_chunks (host gzip, host pairing) -> submit_fastq_pair
S = min(N // 2, 400_000)
q1, q2 = d + "/t_R1.fastq.gz", d + "/t_R2.fastq.gz"
for path, raw in ((q1, raw1), (q2, raw2)):
    with open(path, "wb") as f:
        f.write(b"".join(block((raw[at:min(at + 65280, S * rec)], LEVEL)) for at in range(0, S * rec, 65280)) + eof)
timed("host_pair_chunks_slice", lambda: sum(eng.submit_fastq_pair(c1, c2) for c1, c2 in fastq.pair_chunks(q1, q2, 128 << 20)), runs=2)
eng.close()
print(json.dumps(out))
