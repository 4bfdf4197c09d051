#!/usr/bin/env python3
"""Rate of SAM text input: a synthetic bowtie2-shaped file (records of 150 bases, 20 records per read name, tags AS XS XN XM XO XG
NM MD YT) written as SAM text and, record for record, as a BGZF BAM, then typed
  (a) on the device from the text (Engine.submit_sam_file + stats, Engine.pileup_sam_file), N_RECORDS [2000000] records;
  (b) by the host reader (samin.AlignmentSample.add_file + .stats() + .pileup) on the text of the first HOST_RECORDS [200000] records,
      so that it ends -- the device step types that file too and must give the same statistics and pile-up;
  (c) on the device from the BAM (Engine.submit_bam_file, Engine.pileup_bam_file), the same N_RECORDS records.
One JSON line, and the measured block of profiles/sam_gpu.md (OUT_MD; the text between the two marker lines is replaced, the rest
of the note is kept).  CHUNK_BYTES [64 MiB] per call.
The script is a driver: it writes the files, then runs the GPU steps as child processes of their own (`--step host|sam|bam DIR`),
each under its own time limit, the next only if the one before ended well; nothing is tried again."""
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from metamlst_amd import samin, synth  # noqa: E402
from metamlst_amd.engine import Engine  # noqa: E402
from metamlst_amd.index import load_index  # noqa: E402
from metamlst_amd.typing import pick_alleles_fast  # noqa: E402

N = int(os.environ.get("N_RECORDS", "2000000"))
N_HOST = min(N, int(os.environ.get("HOST_RECORDS", "200000")))
CHUNK = int(os.environ.get("CHUNK_BYTES", str(64 << 20)))
OUT_MD = os.environ.get("OUT_MD", os.path.join(ROOT, "profiles", "sam_gpu.md"))
LINK_GBPS = 50.0      # what a host-to-device copy from page-locked memory reaches (profiles/h2d_rate.py)
FIELDS = ("sum_score", "n_hits", "locus_len_sum", "locus_first")
BEGIN, END = "<!-- sam_rate.py: measured -->", "<!-- sam_rate.py: end -->"


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_files(d, idx, n, n_host, seed=1):
    """n records, 20 per read name (the read's best allele and 19 neighbours of the same locus), as big.sam, big.bam and -- the
    first n_host of them -- host.sam"""
    rng = np.random.default_rng(seed)
    refs = [(idx.label(a), int(idx.off[a + 1] - idx.off[a])) for a in range(idx.n_alleles)]
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs)))
    for nm, ln in refs:
        out += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    nib = np.array([1, 2, 4, 8], np.uint8)
    letter = np.frombuffer(b"ACGT", np.uint8)
    with open(d + "/big.bam", "wb") as fb, open(d + "/big.sam", "wb") as fs, open(d + "/host.sam", "wb") as fh:
        fs.write(text.encode()); fh.write(text.encode())

        def flush(final=False):
            nonlocal out
            while len(out) >= 65280 or (final and out):
                fb.write(bgzf_block(bytes(out[:65280]))); del out[:65280]
        done = 0
        for r in range((n + 19) // 20):
            l = int(rng.integers(0, idx.n_loci)); b0 = int(idx.locus_begin[l]); cnt = int(idx.locus_count[l])
            base = rng.integers(0, 4, size=150)
            codes = nib[base]
            packed = ((codes[0::2] << 4) | codes[1::2]).tobytes(); q = rng.integers(20, 41, size=150).astype(np.uint8)
            qual = q.tobytes(); seq_t = letter[base].tobytes(); qual_t = (q + 33).astype(np.uint8).tobytes()
            name = b"read%d" % r
            lines = []
            for k in range(min(20, n - 20 * r)):
                a = b0 + (r + k) % cnt; pos = int(rng.integers(0, max(1, refs[a][1] - 150)))
                AS, xm, flag = max(0, 250 - 6 * k), k % 6, 0 if k == 0 else 256
                aux = (b"ASC" + bytes([AS]) + b"XSC" + bytes([200]) + b"XNC\0" + b"XMC" + bytes([xm]) + b"XOC\0XGC\0" + b"NMC" + bytes([xm]) + b"MDZ150\0YTZUU\0")
                body = struct.pack("<iiBBHHHiiii", a, pos, len(name) + 1, 255, 4680, 1, flag, 150, -1, -1, 0) + name + b"\0" + struct.pack("<I", 150 << 4) + packed + qual + aux
                out += struct.pack("<i", len(body)) + body
                lines.append(b"%s\t%d\t%s\t%d\t255\t150M\t*\t0\t0\t%s\t%s\tAS:i:%d\tXS:i:200\tXN:i:0\tXM:i:%d\tXO:i:0\tXG:i:0\tNM:i:%d\tMD:Z:150\tYT:Z:UU\n"
                             % (name, flag, refs[a][0].encode(), pos + 1, seq_t, qual_t, AS, xm, xm))
            blob = b"".join(lines)
            fs.write(blob)
            if done < n_host:
                fh.write(b"".join(lines[:n_host - done]))
            done += len(lines)
            flush()
        flush(True)
        fb.write(bgzf_block(b""))


def engine_for(d):
    idx = load_index(d + "/e.db")
    eng = Engine(0)
    eng.load_reference(idx)
    return idx, eng


def step_host(d):
    idx, eng = engine_for(d)
    t0 = time.perf_counter()
    smp = samin.AlignmentSample(idx).add_file(d + "/host.sam")
    st = smp.stats()
    t1 = time.perf_counter()
    chosen = sorted(pick_alleles_fast(idx, st, 100).values())
    t2 = time.perf_counter()
    pile = smp.pileup(eng, chosen)
    t3 = time.perf_counter()
    np.savez(d + "/host.npz", chosen=np.array(chosen), counters=st.counters, **{f: getattr(st, f) for f in FIELDS}, **{"p%d" % a: pile[a] for a in chosen})
    print(json.dumps({"records": N_HOST, "pass1_s": t1 - t0, "pileup_s": t3 - t2, "records_per_s": N_HOST / ((t1 - t0) + (t3 - t2))}))


def timed(eng, idx, submit, pileup, path, reps=3):
    """best of `reps`: (figures, statistics, chosen alleles, pile-up)"""
    best = None
    for _ in range(reps):
        eng.reset_sample()
        t0 = time.perf_counter()
        n = submit(path, chunk_bytes=CHUNK)
        st = eng.stats()
        t1 = time.perf_counter()
        chosen = sorted(pick_alleles_fast(idx, st, 100).values())
        t2 = time.perf_counter()
        pile = pileup(path, chosen, chunk_bytes=CHUNK)
        t3 = time.perf_counter()
        cur = {"records": int(n), "pass1_s": t1 - t0, "pass2_s": t3 - t2, "records_per_s": n / ((t1 - t0) + (t3 - t2))}
        if best is None or cur["records_per_s"] > best["records_per_s"]:
            best = cur
    return best, st, chosen, pile


def step_sam(d):
    idx, eng = engine_for(d)
    # the host reader's file first: the same answers
    small, st, chosen, pile = timed(eng, idx, eng.submit_sam_file, eng.pileup_sam_file, d + "/host.sam", reps=1)
    h = np.load(d + "/host.npz")
    assert all(np.array_equal(getattr(st, f), h[f]) for f in FIELDS) and np.array_equal(st.counters[:2], h["counters"][:2]), "statistics differ from the host reader"
    assert chosen == [int(a) for a in h["chosen"]] and all(np.array_equal(pile[a], h["p%d" % a]) for a in chosen), "pile-up differs from the host reader"
    best, st, chosen, pile = timed(eng, idx, eng.submit_sam_file, eng.pileup_sam_file, d + "/big.sam")
    assert best["records"] == N
    best["host_file"] = small
    best["equal_to_host_reader"] = True
    # per kernel (HIP events; a run of its own: events end the overlap of a chunk's copy with the kernels before it)
    eng.set_profiling(1); eng.reset_kernel_time(); eng.reset_sample()
    eng.submit_sam_file(d + "/big.sam", chunk_bytes=CHUNK)
    eng.pileup_sam_file(d + "/big.sam", chosen, chunk_bytes=CHUNK)
    best["kernel_ms"] = {name: {"ms": eng.kernel_time(w)[0], "entries": eng.kernel_time(w)[1]} for w, name in ((15, "line table"), (16, "k_sam_accumulate"), (17, "k_sam_pileup"))}
    eng.set_profiling(0)
    np.savez(d + "/sam.npz", chosen=np.array(chosen), counters=st.counters, **{f: getattr(st, f) for f in FIELDS}, **{"p%d" % a: pile[a] for a in chosen})
    # the file read alone (page cache warm, as for the runs above)
    t0 = time.perf_counter()
    with open(d + "/big.sam", "rb") as f:
        while f.read(CHUNK):
            pass
    best["file_read_s"] = time.perf_counter() - t0
    print(json.dumps(best))


def step_bam(d):
    idx, eng = engine_for(d)
    best, st, chosen, pile = timed(eng, idx, eng.submit_bam_file, eng.pileup_bam_file, d + "/big.bam")
    assert best["records"] == N
    h = np.load(d + "/sam.npz")
    assert all(np.array_equal(getattr(st, f), h[f]) for f in FIELDS) and np.array_equal(st.counters[:2], h["counters"][:2]), "statistics differ between SAM and BAM"
    assert chosen == [int(a) for a in h["chosen"]] and all(np.array_equal(pile[a], h["p%d" % a]) for a in chosen), "pile-up differs between SAM and BAM"
    best["equal_to_sam"] = True
    print(json.dumps(best))


def write_note(out):
    s, b, h = out["sam"], out["bam"], out["host"]
    gb = out["sam_bytes"] / 1e9
    rows = [
        "| path | records | pass 1 s | pass 2 s | records/s | GB/s of text, pass 1 / pass 2 |",
        "|---|---|---|---|---|---|",
        "| device, SAM text | %d | %.3f | %.3f | %.3g | %.2f / %.2f |" % (s["records"], s["pass1_s"], s["pass2_s"], s["records_per_s"], gb / s["pass1_s"], gb / s["pass2_s"]),
        "| device, BGZF BAM of the same records | %d | %.3f | %.3f | %.3g | (%.2f GB of BAM) |" % (b["records"], b["pass1_s"], b["pass2_s"], b["records_per_s"], out["bam_bytes"] / 1e9),
        "| host reader, first %d records | %d | %.3f | %.3f | %.3g | |" % (h["records"], h["records"], h["pass1_s"], h["pileup_s"], h["records_per_s"]),
        "| device, SAM text, the host reader's file | %d | %.3f | %.3f | %.3g | |" % (s["host_file"]["records"], s["host_file"]["pass1_s"], s["host_file"]["pass2_s"], s["host_file"]["records_per_s"]),
    ]
    k = s["kernel_ms"]
    body = [BEGIN, "", "`profiles/sam_rate.py`, %d records, %.3f GB of SAM text, chunks of %d MiB, best of three runs (the file in the page cache)." % (out["records"], gb, CHUNK >> 20), ""]
    body += rows + [""]
    body += ["Device against host reader on the same file: %.0f times the records/s.  Against the link's ~%.0f GB/s the text moves at %.1f %% (pass 1) and %.1f %% (pass 2)."
             % (s["host_file"]["records_per_s"] / h["records_per_s"], LINK_GBPS, 100 * gb / s["pass1_s"] / LINK_GBPS, 100 * gb / s["pass2_s"] / LINK_GBPS), ""]
    body += ["Per kernel group (`mlst_get_kernel_time`, HIP events, a run of its own over both passes):", "",
             "| which | kernels | ms | entries | GB/s of text |", "|---|---|---|---|---|",
             "| 15 | k_fq_count, k_fq_scan, k_fq_lines, k_sam_flags (both passes) | %.2f | %d | %.1f |" % (k["line table"]["ms"], k["line table"]["entries"], 2 * gb / max(k["line table"]["ms"], 1e-9) * 1e3),
             "| 16 | k_sam_accumulate | %.2f | %d | %.1f |" % (k["k_sam_accumulate"]["ms"], k["k_sam_accumulate"]["entries"], gb / max(k["k_sam_accumulate"]["ms"], 1e-9) * 1e3),
             "| 17 | k_sam_pileup | %.2f | %d | %.1f |" % (k["k_sam_pileup"]["ms"], k["k_sam_pileup"]["entries"], gb / max(k["k_sam_pileup"]["ms"], 1e-9) * 1e3), "",
             "Reading the file alone (no device): %.3f s, %.2f GB/s." % (s["file_read_s"], gb / s["file_read_s"]), "", END]
    block = "\n".join(body)
    old = open(OUT_MD).read() if os.path.exists(OUT_MD) else "# SAM text on the device\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + block + old[old.index(END) + len(END):]
    else:
        new = old.rstrip("\n") + "\n\n" + block + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(OUT_MD)), exist_ok=True)
    with open(OUT_MD, "w") as f:
        f.write(new)


if len(sys.argv) == 4 and sys.argv[1] == "--step":
    {"host": step_host, "sam": step_sam, "bam": step_bam}[sys.argv[2]](sys.argv[3])
    sys.exit(0)

d = tempfile.mkdtemp()
db = synth.make_ecoli_db(d + "/e.db", alleles_per_locus=300, n_profiles=50)
idx = load_index(db.path)
write_files(d, idx, N, N_HOST)
out = {"records": N, "sam_bytes": os.path.getsize(d + "/big.sam"), "bam_bytes": os.path.getsize(d + "/big.bam"), "chunk_bytes": CHUNK}
for name, limit in (("host", int(os.environ.get("HOST_TIMEOUT", "300"))), ("sam", int(os.environ.get("DEVICE_TIMEOUT", "180"))), ("bam", int(os.environ.get("DEVICE_TIMEOUT", "180")))):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, d], stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:      # a step that failed or ran out of time ends the run: nothing is started behind it
        print(json.dumps(dict(out, failed=name, returncode=r.returncode)))
        sys.exit(1)
    out[name] = json.loads(r.stdout.strip().splitlines()[-1])
out["speedup_over_host_reader"] = out["sam"]["host_file"]["records_per_s"] / out["host"]["records_per_s"]
write_note(out)
print(json.dumps(out))
