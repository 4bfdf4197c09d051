"""FASTQ -> (bases, quals, offsets) batches for mlst_submit_reads (host part).

The reference never reads FASTQ itself (bowtie2 does, outside the tree); this is the minimal host
reader so the engine can be fed the same files.  Plain or gzip, 4-line records, Phred+33."""
from __future__ import annotations

import gzip
import os
import threading

import numpy as np


def _open(path: str):
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def read_batches(path: str, batch_reads: int = 2_000_000, max_len: int = 320):
    """Yield (bases uint8[], quals uint8[], off uint64[n+1], names list[bytes]) per batch.
    Reads longer than max_len are truncated (the packed format holds 320 bases)."""
    seqs, quals, names = [], [], []
    with _open(path) as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().rstrip(b"\r\n")
            f.readline()
            q = f.readline().rstrip(b"\r\n")
            if len(q) != len(s):
                raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
            names.append(h[1:].split()[0] if len(h) > 1 else b"")
            seqs.append(s[:max_len])
            quals.append(q[:max_len])
            if len(seqs) == batch_reads:
                yield _pack(seqs, quals, names)
                seqs, quals, names = [], [], []
    if seqs:
        yield _pack(seqs, quals, names)


def _pack(seqs, quals, names):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.frombuffer(b"".join(seqs), np.uint8).copy(), np.frombuffer(b"".join(quals), np.uint8).copy(), off, names)


def interleave(path1: str, path2: str, batch_pairs: int = 1_000_000, max_len: int = 320):
    """Paired files -> batches with mates at rows 2k, 2k+1 (the layout mlst_submit_reads(paired=1) expects)."""
    for (b1, q1, o1, n1), (b2, q2, o2, n2) in zip(read_batches(path1, batch_pairs, max_len), read_batches(path2, batch_pairs, max_len)):
        if len(o1) != len(o2):
            raise ValueError("paired FASTQ files have different numbers of reads")
        seqs, quals = [], []
        for k in range(len(o1) - 1):
            seqs += [b1[int(o1[k]):int(o1[k + 1])].tobytes(), b2[int(o2[k]):int(o2[k + 1])].tobytes()]
            quals += [q1[int(o1[k]):int(o1[k + 1])].tobytes(), q2[int(o2[k]):int(o2[k + 1])].tobytes()]
        yield _pack(seqs, quals, [x for p in zip(n1, n2) for x in p])


def record_start(buf, pos: int = 0) -> int:
    """Offset of the first FASTQ record that starts at or after `pos` in `buf` (bytes-like), -1 if none can be told.
    A record starts at a line that begins with '@' whose next-but-one line begins with '+': a quality line may begin
    with '@' too, but then the line two further on is a sequence line, which never begins with '+' (4-line records)."""
    n = len(buf)
    if pos <= 0:
        p = 0
    else:
        p = buf.find(b"\n", pos - 1) + 1          # first line start at or after pos (pos itself when buf[pos-1] is a newline)
        if p == 0:
            return -1
    while p < n:
        e1 = buf.find(b"\n", p)
        if e1 < 0:
            return -1
        e2 = buf.find(b"\n", e1 + 1)
        if e2 < 0 or e2 + 1 >= n:
            return -1
        if buf[p] == 0x40 and buf[e2 + 1] == 0x2B:
            return p
        p = e1 + 1
    return -1


def last_record_start(buf, window: int = 1 << 16) -> int:
    """Offset of the last record that starts in `buf` (so that buf[:offset] holds whole records), -1 if none.  Only the
    tail of the buffer is looked at: the window doubles until it holds a record start."""
    n = len(buf)
    w = min(window, n)
    while True:
        lo = n - w
        best, p = -1, record_start(buf, lo) if lo else record_start(buf, 0)
        while p >= 0:
            best = p
            nxt = buf.find(b"\n", p)
            p = record_start(buf, nxt + 1) if nxt >= 0 else -1
        if best >= 0 or w == n:
            return best
        w = min(n, w * 4)


# ---- plain files: positional reads by a few threads into buffers that are used again
# One Python thread moves ~1 GB/s from the page cache through f.read() + slicing (two or three copies of every byte): a
# sample of a million reads took 0.3 s to reach the library, which needs 7 ms for it.  os.preadv releases the GIL, so a few
# threads fill one numpy buffer side by side (no copy afterwards: the chunk handed to the library is a view of it), and
# the buffers go round (a fresh 256 MB array costs its page faults again).
_READ_PIECE = 4 << 20
_pool_lock = threading.Lock()
_pool_bufs: list = []          # idle buffers (uint8 arrays), at most _POOL_MAX of them
_POOL_MAX = int(os.environ.get("MLST_READ_POOL", "20"))      # (four feeder threads keep four buffers each in flight: a pool that holds fewer
                                                             # frees and allocates page-locked memory between samples -- ~50 ms per 256 MB buffer)
_readers = None


def _reader_pool():
    global _readers
    if _readers is None:
        with _pool_lock:      # (first called by four feeder threads at once: one pool, not four)
            if _readers is None:
                from concurrent.futures import ThreadPoolExecutor
                _readers = ThreadPoolExecutor(max(2, min(int(os.environ.get("MLST_READ_THREADS", "32")), (os.cpu_count() or 2) // 2)), thread_name_prefix="fastq-read")
    return _readers


_alloc = None                  # set_buffer_allocator: n bytes -> uint8 array (page-locked memory when a GPU runtime is there)


def set_buffer_allocator(fn) -> None:
    """Where the read buffers of text_chunks(reuse=True) come from: fn(n_bytes) -> uint8 array, None = numpy.  The CLI passes
    engine.pinned_array: a chunk then crosses the link as one DMA transfer instead of through the runtime's staging copy."""
    global _alloc
    with _pool_lock:
        if fn is _alloc:
            return
        _alloc = fn
        old = list(_pool_bufs)      # (dropped after the lock is released: freeing page-locked memory takes milliseconds per buffer)
        _pool_bufs.clear()
    del old


def _take_buffer(n: int) -> np.ndarray:
    with _pool_lock:
        for k, b in enumerate(_pool_bufs):
            if b.size >= n:
                return _pool_bufs.pop(k)
        if len(_pool_bufs) >= _POOL_MAX:
            _pool_bufs.pop(0)
        fn = _alloc
    size = max(1 << 20, 1 << (int(n) - 1).bit_length())      # powers of two: a buffer fits the next file's chunks too
    if fn is not None:
        try:
            return fn(size)
        except Exception:      # noqa: BLE001 -- no page-locked memory to be had: ordinary memory does
            pass
    return np.empty(size, np.uint8)


def _give_buffer(b: np.ndarray) -> None:
    with _pool_lock:
        if len(_pool_bufs) < _POOL_MAX:
            _pool_bufs.append(b)


def _pread_into(fd: int, buf: np.ndarray, lo: int, hi: int) -> None:
    """bytes [lo, hi) of the file into buf[:hi - lo], pieces of 4 MB read side by side"""
    mv = memoryview(buf)

    def piece(a: int) -> None:
        e = min(a + _READ_PIECE, hi)
        at = a
        while at < e:
            got = os.preadv(fd, [mv[at - lo:e - lo]], at)
            if got <= 0:
                raise OSError("short read at byte %d" % at)
            at += got

    starts = range(lo, hi, _READ_PIECE)
    if len(starts) <= 1:
        for a in starts:
            piece(a)
    else:
        list(_reader_pool().map(piece, starts))


def raw_chunks(path: str, chunk_bytes: int = 256 << 20, lo: int = 0, hi: int | None = None, margin: int = 1 << 17,
               reuse: bool = False, ring: list | None = None):
    """Bytes [lo, hi) of a file in pieces of chunk_bytes, cut anywhere: yields (buf, n) with the piece at buf[margin:margin + n]
    and `margin` free bytes in front of it -- room for what the consumer carries over from the piece before (the cut-off BGZF
    block of Engine.submit_fastq_bgzf_file).  Positional reads by a few threads; reuse / ring as in text_chunks."""
    size = os.path.getsize(path)
    hi = size if hi is None else min(hi, size)
    if ring is None:
        ring = []
    fd = os.open(path, os.O_RDONLY)
    try:
        at = lo
        while at < hi:
            n = min(chunk_bytes, hi - at)
            if reuse and len(ring) >= 4:
                buf = ring.pop(0)
                if buf.size < margin + n:
                    _give_buffer(buf)
                    buf = _take_buffer(margin + n)
            else:
                buf = _take_buffer(margin + n) if reuse else np.empty(margin + n, np.uint8)
            if reuse:
                ring.append(buf)
            _pread_into(fd, buf[margin:], at, at + n)
            at += n
            yield buf, n
    finally:
        os.close(fd)


def release_buffers(ring: list) -> None:
    """The consumer is done with every chunk of a text_chunks(reuse=True, ring=ring) walk: its buffers may serve the next file."""
    while ring:
        _give_buffer(ring.pop())


def _plain_chunks(path: str, chunk_bytes: int, start: int, end: int | None, reuse: bool, ring: list | None = None):
    """text_chunks for an uncompressed file (same chunks, same byte ranges): positional reads, chunks are uint8 arrays.
    reuse=True: a chunk's memory is used again once the consumer has taken the chunk after the next THREE (prefetch() holds two,
    the consumer one) -- for consumers that are done with a chunk when they ask for the next; reuse=False: every chunk its own array.
    The walk never hands its buffers to another walk by itself -- its last chunks may still be in the consumer's hands when it
    ends: a consumer that passes `ring` gets the buffers listed there and gives them back with release_buffers(ring)."""
    size = os.path.getsize(path)
    if size == 0:
        return
    fd = os.open(path, os.O_RDONLY)
    if ring is None:
        ring = []
    try:
        def peek(lo: int, n: int) -> bytes:
            return os.pread(fd, max(0, min(n, size - lo)), lo)

        examined = [0]

        def first_start(at: int) -> int:
            """first record start at or after byte `at` (absolute), -1 if none can be told"""
            if at <= 0:
                return 0
            w = 1 << 16
            while True:
                head = peek(at - 1, w)                       # one byte early: a record that starts exactly at `at` counts
                examined[0] = at - 1 + len(head)
                s0 = record_start(head, 1)
                if s0 >= 0:
                    return at - 1 + s0
                if examined[0] >= size or w >= (64 << 20):
                    return -1
                w *= 4

        pos = first_start(start) if start else 0
        if pos < 0:
            if end is not None and examined[0] < end:
                raise ValueError("%s: no FASTQ record boundary after byte %d" % (path, start))
            return                                           # the range holds the inside of the file's last record only
        if end is not None and pos >= end:
            return                                           # the first record at or after `start` belongs to the next range
        stop = size
        if end is not None and end < size:
            s1 = first_start(end)                            # the record that starts last before `end` is ours in full
            stop = s1 if s1 >= 0 else size
        while pos < stop:
            e = min(pos + chunk_bytes, stop)
            cut = e
            if e < stop:                                     # cut at the last record start inside [pos, e)
                w = 1 << 16
                while True:
                    lo = max(pos, e - w)
                    k = last_record_start(peek(lo, e - lo))
                    if k > 0 or (k == 0 and lo > pos):
                        cut = lo + k
                        break
                    if lo == pos:                            # no whole record in the chunk (a record longer than it): read on
                        chunk_bytes *= 2
                        cut = -1
                        break
                    w *= 4
                if cut < 0:
                    continue
            n = cut - pos
            if reuse and len(ring) >= 4:
                buf = ring.pop(0)
                if buf.size < n:
                    _give_buffer(buf)
                    buf = _take_buffer(n)
            else:
                buf = _take_buffer(n) if reuse else np.empty(n, np.uint8)
            _pread_into(fd, buf, pos, cut)
            if reuse:
                ring.append(buf)
            chunk = buf[:n]
            if cut < size or n > 4096 or chunk.tobytes().strip():      # (a file's whitespace-only tail is not a chunk)
                yield chunk
            pos = cut
    finally:
        os.close(fd)


def text_chunks(path: str, chunk_bytes: int = 256 << 20, start: int = 0, end: int | None = None, reuse: bool = False, ring: list | None = None):
    """Yield byte chunks of an uncompressed (or .gz) FASTQ that each hold whole records, for Engine.submit_fastq.
    The host never scans the text: a chunk is cut at the last record start found in its tail (record_start); parsing
    happens on the GPU.  start / end (plain files only) restrict the walk to the records that START in the byte range
    [start, end): the first record is found by resynchronising at `start`, the last one is completed beyond `end` --
    N ranks given consecutive ranges read every record exactly once and touch only their share of the file.
    Plain files are read by positional reads of a few threads (_plain_chunks; reuse: see there); .gz through gzip."""
    gz = path.endswith(".gz")
    if gz and (start or end is not None):
        raise ValueError("byte ranges need an uncompressed FASTQ (gzip has no random access; bgzip files are sharded by block)")
    if not gz:
        yield from _plain_chunks(path, chunk_bytes, start, end, reuse, ring)
        return
    carry = b""
    with _open(path) as f:
        pos = 0
        if start:
            f.seek(start - 1)                      # one byte early: a record that starts exactly at `start` is ours
            pos = start - 1
            head = f.read(1 << 16)
            while True:
                s0 = record_start(head, 1)
                if s0 >= 0 or len(head) >= (64 << 20):
                    break
                more = f.read(len(head))
                if not more:
                    break
                head += more
            if s0 < 0:
                if end is not None and pos + len(head) < end:
                    raise ValueError("%s: no FASTQ record boundary after byte %d" % (path, start))
                return                              # the range holds the inside of the file's last record only
            if end is not None and pos + s0 >= end:
                return                              # the first record at or after `start` belongs to the next range
            carry = head[s0:]
            pos += len(head)
        done = False
        while not done:
            want = chunk_bytes - len(carry) if len(carry) < chunk_bytes else 0
            block = f.read(want) if want else b""
            data = carry + block if carry else block
            base = pos - len(carry)                 # file offset of data[0]
            pos += len(block)
            eof = want > 0 and len(block) < want
            if end is not None and base + len(data) > end:
                # the record that starts last before `end` is ours in full; what follows belongs to the next range
                cut = record_start(data, max(end - base, 0))
                while cut < 0 and not eof:          # the boundary record is not complete yet
                    more = f.read(1 << 16)
                    if not more:
                        eof = True
                        break
                    data += more
                    pos += len(more)
                    cut = record_start(data, max(end - base, 0))
                if cut < 0:
                    cut = len(data)                 # nothing starts after `end`: the range runs to the end of the file
                if cut:
                    yield data[:cut]
                return
            if eof:
                if data.strip():
                    yield data
                return
            cut = last_record_start(data)
            if cut <= 0:
                carry = data                        # no whole record yet (a record longer than the chunk): read on
                chunk_bytes *= 2
                continue
            yield data[:cut]
            carry = data[cut:]


def _count_newlines(buf: np.ndarray, n: int) -> tuple[list, list]:
    """newlines of buf[:n] per piece of 4 MB, counted side by side (numpy's comparison and count release the GIL)"""
    starts = list(range(0, n, _READ_PIECE))

    def one(a: int) -> int:
        return int(np.count_nonzero(buf[a:min(a + _READ_PIECE, n)] == 10))

    counts = [one(a) for a in starts] if len(starts) <= 1 else list(_reader_pool().map(one, starts))
    return starts, counts


def _after_newline(buf: np.ndarray, n: int, starts: list, counts: list, which: int) -> int:
    """offset just behind the which-th newline (1-based) of buf[:n]"""
    seen = 0
    for a, c in zip(starts, counts):
        if seen + c >= which:
            piece = buf[a:min(a + _READ_PIECE, n)]
            return a + int(np.flatnonzero(piece == 10)[which - seen - 1]) + 1
        seen += c
    raise AssertionError("fewer newlines than counted")


def _plain_pair_chunks(path1: str, path2: str, chunk_bytes: int, reuse: bool, ring: list | None):
    """pair_chunks for two uncompressed files: the same windows and cuts, read by positional reads of a few threads into
    buffers (reuse / ring: as in _plain_chunks, eight buffers deep -- two per pair), newlines counted side by side."""
    s1, s2 = os.path.getsize(path1), os.path.getsize(path2)
    fd1, fd2 = os.open(path1, os.O_RDONLY), os.open(path2, os.O_RDONLY)
    if ring is None:
        ring = []
    o1 = o2 = 0

    def window(fd, off, size):
        n = min(chunk_bytes, size - off)
        if reuse and len(ring) >= 8:
            buf = ring.pop(0)
            if buf.size < n + 1:
                _give_buffer(buf)
                buf = _take_buffer(n + 1)
        else:
            buf = _take_buffer(n + 1) if reuse else np.empty(n + 1, np.uint8)
        if reuse:
            ring.append(buf)
        if n:
            _pread_into(fd, buf, off, off + n)
        eof = off + n == size
        nv = n
        if eof and n and buf[n - 1] != 10:
            buf[n] = 10                                     # an unterminated last line ends here
            nv = n + 1
        return buf, n, nv, eof

    try:
        while True:
            A, n1, v1, e1 = window(fd1, o1, s1)
            B, n2, v2, e2 = window(fd2, o2, s2)
            st1, c1 = _count_newlines(A, v1)
            st2, c2 = _count_newlines(B, v2)
            k = min(sum(c1), sum(c2)) // 4
            if k == 0:
                blank1, blank2 = not A[:v1].tobytes().strip(), not B[:v2].tobytes().strip()
                if e1 and e2:
                    if not (blank1 and blank2):
                        raise ValueError("paired FASTQ files hold different numbers of records (%s, %s)" % (path1, path2))
                    return
                if (e1 and blank1) or (e2 and blank2):
                    raise ValueError("paired FASTQ files hold different numbers of records (%s, %s)" % (path1, path2))
                chunk_bytes *= 2
                continue
            a, b = _after_newline(A, v1, st1, c1, 4 * k), _after_newline(B, v2, st2, c2, 4 * k)
            yield A[:a], B[:b]
            o1 += min(a, n1); o2 += min(b, n2)
    finally:
        os.close(fd1); os.close(fd2)


def pair_chunks(path1: str, path2: str, chunk_bytes: int = 128 << 20, reuse: bool = False, ring: list | None = None):
    """Two FASTQ files of mates -> (chunk1, chunk2) pairs holding the SAME number of whole records each, in file order,
    for Engine.submit_fastq_pair (the k-th record of one file is the mate of the k-th record of the other).  Here the
    host does count lines -- the two cuts have to fall after the same record number.  Uncompressed files: _plain_pair_chunks
    (threads; reuse / ring as in text_chunks); gzip: one thread through gzip."""
    if not path1.endswith(".gz") and not path2.endswith(".gz"):
        yield from _plain_pair_chunks(path1, path2, chunk_bytes, reuse, ring)
        return

    def newlines(buf):
        return np.flatnonzero(np.frombuffer(buf, np.uint8) == 10)

    with _open(path1) as f1, _open(path2) as f2:
        c1 = c2 = b""
        e1 = e2 = False
        while True:
            if not e1 and len(c1) < chunk_bytes:
                b = f1.read(chunk_bytes - len(c1)); e1 = not b; c1 += b
            if not e2 and len(c2) < chunk_bytes:
                b = f2.read(chunk_bytes - len(c2)); e2 = not b; c2 += b
            if e1 and c1 and not c1.endswith(b"\n"):
                c1 += b"\n"
            if e2 and c2 and not c2.endswith(b"\n"):
                c2 += b"\n"
            n1, n2 = newlines(c1), newlines(c2)
            k = min(len(n1), len(n2)) // 4
            if k == 0:
                if e1 and e2:
                    if c1.strip() or c2.strip():
                        raise ValueError("paired FASTQ files hold different numbers of records (%s, %s)" % (path1, path2))
                    return
                if (e1 and not c1.strip()) or (e2 and not c2.strip()):
                    raise ValueError("paired FASTQ files hold different numbers of records (%s, %s)" % (path1, path2))
                chunk_bytes *= 2
                continue
            a, b = int(n1[4 * k - 1]) + 1, int(n2[4 * k - 1]) + 1
            yield c1[:a], c2[:b]
            c1, c2 = c1[a:], c2[b:]


def pair_cuts(path1: str, path2: str, chunk_bytes: int = 128 << 20) -> list[tuple[int, int, int, int]]:
    """(offset 1, bytes 1, offset 2, bytes 2) of the chunk pairs pair_chunks yields, for uncompressed files: ONE rank walks the
    mate files (the cuts have to fall after the same record number in both, so somebody has to count lines) and the others
    read their chunks by offset (multigpu.submit_fastq_shard)."""
    cuts, o1, o2 = [], 0, 0
    s1, s2 = os.path.getsize(path1), os.path.getsize(path2)
    for c1, c2 in pair_chunks(path1, path2, chunk_bytes):
        n1, n2 = min(len(c1), s1 - o1), min(len(c2), s2 - o2)      # (a newline added behind an unterminated last line is not in the file)
        cuts.append((o1, n1, o2, n2))
        o1 += n1; o2 += n2
    return cuts


def read_pair_cut(path1: str, path2: str, cut: tuple[int, int, int, int]) -> tuple[bytes, bytes]:
    out = []
    for path, off, n in ((path1, cut[0], cut[1]), (path2, cut[2], cut[3])):
        with open(path, "rb") as f:
            f.seek(off)
            b = f.read(n)
        out.append(b if b.endswith(b"\n") or not b else b + b"\n")
    return out[0], out[1]


def mates_share_names(path1: str, path2: str) -> bool:
    """True when the first records of the two mate files carry the same read name (the part of the header line before
    the first blank): `@x 1:N:0` / `@x 2:N:0` do, `@x/1` / `@x/2` do not -- and neither would they share a QNAME in the
    SAM that bowtie2 -U writes."""
    with _open(path1) as f1, _open(path2) as f2:
        h1, h2 = f1.readline().split(), f2.readline().split()
    return bool(h1) and bool(h2) and h1[0] == h2[0]


class prefetch:
    """Run the iterator `it` in a thread, `depth` items ahead: file reads (which release the GIL) overlap the consumer's
    GPU submissions.  Exceptions of the producer are raised in the consumer.  The thread starts at once (not at the first
    next()): a caller that opens the reader of sample k + 1 before it consumes sample k has the first chunks of k + 1
    read meanwhile."""

    def __init__(self, it, depth: int = 2):
        import queue
        self._q: queue.Queue = queue.Queue(maxsize=depth)
        self._end = object()
        self._done = False

        def work():
            try:
                for x in it:
                    self._q.put(x)
                self._q.put(self._end)
            except BaseException as e:      # noqa: BLE001 -- handed to the consumer
                self._q.put(e)

        self._t = threading.Thread(target=work, daemon=True)
        self._t.start()

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        x = self._q.get()
        if x is self._end:
            self._done = True
            raise StopIteration
        if isinstance(x, BaseException):
            self._done = True
            raise x
        return x


def fasta_chunks(path: str, chunk_bytes: int = 64 << 20, reuse: bool = False, ring: list | None = None):
    """Yield byte chunks of a FASTA file that each hold whole contigs, for Engine.submit_fasta: a chunk is cut in front of the
    last '>' that starts a line inside it (the last b"\n>"), and a contig longer than chunk_bytes makes its chunk as long as it
    needs; the chunks one after the other are the file.  Plain files: positional reads into uint8 arrays (reuse / ring as in
    text_chunks: pooled, page-locked when set_buffer_allocator says so).  .gz files (bgzip'd ones included) are inflated here on
    the host and yield bytes: a compressed genome is a few dozen BGZF blocks, not worth a device inflate."""
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive")
    if path.endswith(".gz"):
        with _open(path) as f:
            held = b""
            while True:
                piece = f.read(chunk_bytes)
                if not piece:
                    break
                held += piece
                cut = held.rfind(b"\n>") if len(held) >= chunk_bytes else -1
                if cut >= 0:
                    yield held[:cut + 1]
                    held = held[cut + 1:]
            if held:
                yield held
        return
    size = os.path.getsize(path)
    if size == 0:
        return
    if ring is None:
        ring = []
    fd = os.open(path, os.O_RDONLY)
    try:
        pos = 0
        while pos < size:
            e = min(pos + chunk_bytes, size)
            cut = e
            if e < size:      # the last b"\n>" inside [pos, e): looked for from the back, window by window
                cut, hi, w = -1, e, 1 << 16
                while hi > pos + 1:
                    lo = max(pos, hi - w)
                    k = os.pread(fd, hi - lo, lo).rfind(b"\n>")
                    if k >= 0 and lo + k + 1 > pos:
                        cut = lo + k + 1
                        break
                    if lo == pos:
                        break
                    hi, w = lo + 1, w * 4      # (one byte of overlap: a b"\n>" across the windows' edge)
                lo = e - 1
                while cut < 0:                 # one contig fills the chunk: up to the next header, wherever that is
                    piece = os.pread(fd, 1 << 20, lo)
                    k = piece.find(b"\n>")
                    if k >= 0:
                        cut = lo + k + 1
                    elif lo + len(piece) >= size:
                        cut = size
                    else:
                        lo += len(piece) - 1
            n = cut - pos
            if reuse and len(ring) >= 4:
                buf = ring.pop(0)
                if buf.size < n:
                    _give_buffer(buf)
                    buf = _take_buffer(n)
            else:
                buf = _take_buffer(n) if reuse else np.empty(n, np.uint8)
            _pread_into(fd, buf, pos, cut)
            if reuse:
                ring.append(buf)
            yield buf[:n]
            pos = cut
    finally:
        os.close(fd)


def tile_fasta(path: str, read_len: int = 150, stride: int = 25, min_len: int = 50, chunk_reads: int = 500_000):
    """Contigs / an assembled genome as input (the modality of the reference's mlst.py, which BLASTs contigs against
    the alleles; BLAST is not in the tree -- here the contigs go through the same alignment path as reads): every
    contig is cut into overlapping windows (read_len bases every stride bases, the last window flush with the contig
    end), written as FASTQ text with Phred 40 and handed to Engine.submit_fastq in chunks.  Contigs shorter than
    min_len are skipped, shorter than read_len become one read.  Read names: <contig index>_<0-based start>."""
    if read_len < 1 or stride < 1:
        raise ValueError("read_len and stride must be positive")

    def contigs():
        name, parts = None, []
        with _open(path) as f:
            for line in f:
                if line.startswith(b">"):
                    if name is not None:
                        yield b"".join(parts)
                    name, parts = line, []
                elif name is not None:
                    parts.append(line.strip())
        if name is not None:
            yield b"".join(parts)

    out, n_out = [], 0
    for ci, seq in enumerate(contigs()):
        seq = seq.upper()
        n = len(seq)
        if n < min_len:
            continue
        starts = list(range(0, max(n - read_len, 0) + 1, stride))
        if n > read_len and starts[-1] != n - read_len:
            starts.append(n - read_len)
        for st in starts:
            w = seq[st:st + read_len]
            out.append(b"@%d_%d\n%s\n+\n%s\n" % (ci, st, w, b"I" * len(w)))
            n_out += 1
            if n_out == chunk_reads:
                yield b"".join(out)
                out, n_out = [], 0
    if out:
        yield b"".join(out)


def tile_fastq(path: str, read_len: int = 150, stride: int = 25, chunk_reads: int = 500_000):
    """Long reads as input (merged pairs, amplicons, ONT / HiFi): the packed formats hold 320 bases, so a record of more than
    read_len bases is cut into overlapping windows the way tile_fasta cuts a contig (read_len bases every stride bases, the last
    window flush with the record's end), each window with the same slice of the quality line.  Yields FASTQ text in chunks of
    chunk_reads records for Engine.submit_fastq.  Records keep their order; a record of at most read_len bases (an empty one
    included) goes out unchanged as one record; there is no min_len (short reads are filtered where they always were).  Bases
    are not touched (N, lower case: the parser's business); line ends become LF.  Window names: <name>_<0-based start>.
    The windows are unpaired reads of their own (MLST_LONG_READ_WINDOWS, include/mlst_policy.h).  This is the rule
    mlst_set_read_tiling applies on the device; it serves single-stream .gz input and the tests."""
    if read_len < 1 or stride < 1:
        raise ValueError("read_len and stride must be positive")
    out, n_out = [], 0
    with _open(path) as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().rstrip(b"\r\n")
            f.readline()
            q = f.readline().rstrip(b"\r\n")
            h = h.rstrip(b"\r\n")
            if not h and not s and not q:
                continue                                     # blank lines at the end of the file
            if len(q) != len(s):
                raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
            n = len(s)
            if n <= read_len:
                out.append(b"%s\n%s\n+\n%s\n" % (h, s, q))
                n_out += 1
            else:
                name = h.split()[0] if h.split() else b"@"
                starts = list(range(0, n - read_len + 1, stride))
                if starts[-1] != n - read_len:
                    starts.append(n - read_len)
                for st in starts:
                    out.append(b"%s_%d\n%s\n+\n%s\n" % (name, st, s[st:st + read_len], q[st:st + read_len]))
                n_out += len(starts)
            if n_out >= chunk_reads:
                yield b"".join(out)
                out, n_out = [], 0
    if out:
        yield b"".join(out)


def qtrim_len(q, T: int) -> int:
    """The 3' quality trim on Phred values q (cutadapt -q T / bwa aln -q T, no minimum length): how many values remain.  The sum of
    T - q[i] is walked from the last value down; the walk ends at the first negative sum; the cut is where the sum first reached its
    largest value (an equal sum further down does not move it).  T = 0: nothing is trimmed."""
    n = len(q)
    if T <= 0:
        return n
    s = best = 0
    cut = n
    for i in range(n - 1, -1, -1):
        s += T - q[i]
        if s < 0:
            break
        if s > best:
            best, cut = s, i
    return cut


def prep_fastq(text: bytes, trim5: int = 0, trim3: int = 0, trim_qual: int = 0, phred64: bool = False) -> tuple[bytes, dict]:
    """The FASTQ text the engine behaves as if it had been given under Engine.set_read_prep(trim5, trim3, trim_qual, phred64), and
    the counters of Engine.read_prep_info().  This is the rule mlst_set_read_prep applies on the device (csrc/read_prep.h); it serves
    the tests and whoever wants the prepared file -- the command never calls it.  Per record, header and '+' line untouched, line
    ends LF, in this order:
      1. Phred: q[i] = clamp(character - base, 0, 127), base 64 under phred64, else 33; written back as the character q[i] + 33.
      2. Fixed trims (bowtie2 -5 / -3): a = min(trim5, n), n1 = max(0, n - trim5 - trim3); bases and qualities [a, a + n1) remain.
      3. qtrim_len(q[a : a + n1], trim_qual) of them remain.
      4. A read left without a base stays a record with an empty sequence and an empty quality line.
    Each mate of a pair is prepared on its own (prepare each file).  Counters: shortened (reads whose length changed),
    bases_removed, emptied (reads of length >= 1 that end with no base)."""
    if trim5 < 0 or trim3 < 0 or trim_qual < 0:
        raise ValueError("trims must not be negative")
    base = 64 if phred64 else 33
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    out = []
    info = {"shortened": 0, "bases_removed": 0, "emptied": 0}
    for k in range(0, len(lines), 4):
        h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k:k + 4])
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
        n = len(s)
        q = [min(max(c - base, 0), 127) for c in ql]
        a = min(trim5, n)
        n1 = max(0, n - trim5 - trim3)
        n2 = qtrim_len(q[a:a + n1], trim_qual)
        if n2 != n:
            info["shortened"] += 1
            info["bases_removed"] += n - n2
            info["emptied"] += n2 == 0
        out.append(b"%s\n%s\n%s\n%s\n" % (h, s[a:a + n2], p, bytes(v + 33 for v in q[a:a + n2])))
    return b"".join(out), info


ADAPTER_NAMES = {"illumina": "AGATCGGAAGAGC", "nextera": "CTGTCTCTTATA", "smallrna": "TGGAATTCTCGG"}      # (the three Trim Galore knows)


def check_adapters(adapters, min_overlap: int = 3, error_permille: int = 100) -> list:
    """The adapters of Engine.set_read_adapters as a list of upper-case bytes; ValueError for a setting mlst_set_read_adapters refuses:
    a letter outside ACGTN, an adapter of only Ns, an empty one, more than 8 adapters, one longer than 64 letters, min_overlap outside
    1..64, error_permille outside 0..500.  adapters: one str / bytes with commas between the adapters, or a sequence of them."""
    if isinstance(adapters, (str, bytes, bytearray)):
        adapters = (adapters.encode() if isinstance(adapters, str) else bytes(adapters)).split(b",")
    out = [(a.encode() if isinstance(a, str) else bytes(a)).upper() for a in adapters]
    if not 1 <= len(out) <= 8:
        raise ValueError("%d adapters: 1 to 8 are taken" % len(out))
    for a in out:
        if not 1 <= len(a) <= 64:
            raise ValueError("an adapter holds %d letters: 1 to 64 are taken" % len(a))
        if a.strip(b"ACGTN"):
            raise ValueError("adapter %r holds a letter outside ACGTN" % a.decode("latin-1"))
        if not a.strip(b"N"):
            raise ValueError("adapter %r holds only N" % a.decode())
    if not 1 <= int(min_overlap) <= 64:
        raise ValueError("min_overlap %r is outside 1..64" % (min_overlap,))
    if not 0 <= int(error_permille) <= 500:
        raise ValueError("error_permille %r is outside 0..500" % (error_permille,))
    return out


def adapter_cut(seq: bytes, adapters, min_overlap: int = 3, error_permille: int = 100) -> tuple[int, int]:
    """Where a 3' adapter is removed from the read seq: (new length, index of the adapter), or (len(seq), -1) when none is found.  The
    rule is the project's own, modelled on `cutadapt -a ADAPTER --no-indels --times 1`; it does not claim cutadapt's bytes.
      * A candidate is an adapter k (m letters of ACGTN) and a start p, 0 <= p <= n - min(min_overlap, m).  Its overlap is
        L = min(m, n - p): the adapter lies inside the read or hangs over its 3' end, never over the 5' end.
      * Position i < L matches if adapter[i] is N or the read's byte at p + i, upper-cased, equals adapter[i]: a non-ACGT byte of the
        read, N included, matches only an adapter N.  mism = L - matches.
      * The candidate is valid if mism <= (L * error_permille) // 1000 (integers).
      * The cut is the valid candidate with the most matches; among equals the smallest p, then the smallest k.  Bases [0, p) remain."""
    ads = check_adapters(adapters, min_overlap, error_permille)
    s = np.frombuffer(bytes(seq).upper(), np.uint8)
    n = len(s)
    best, cut, which = 0, n, -1
    for k, a in enumerate(ads):
        m = len(a)
        last = n - min(min_overlap, m)                      # the last start
        if last < 0:
            continue
        matches = np.zeros(last + 1, np.int64)              # per start p
        for i in range(min(m, n)):                          # letter i lies on base p + i, inside the read for p < n - i
            top = min(last + 1, n - i)
            matches[:top] += 1 if a[i] == 78 else (s[i:i + top] == a[i])      # (78: 'N')
        L = np.minimum(m, n - np.arange(last + 1))
        valid = L - matches <= (L * error_permille) // 1000
        if valid.any():
            p = int(np.where(valid, matches, -1).argmax())  # the most matches, the smallest p among equals
            if which < 0 or matches[p] > best or (matches[p] == best and p < cut):
                best, cut, which = int(matches[p]), p, k
    return cut, which


def trim_adapters(text: bytes, adapters, min_overlap: int = 3, error_permille: int = 100) -> tuple[bytes, dict]:
    """The FASTQ text the engine behaves as if it had been given under Engine.set_read_adapters(adapters, min_overlap, error_permille),
    and the counters of Engine.read_adapters_info().  This is the rule mlst_set_read_adapters applies on the device
    (csrc/read_adapt.h, adapter_cut per read); it serves the tests and whoever wants the cut file -- the command never calls it.  Per
    record, header and '+' line untouched, line ends LF: bases and quality characters [0, adapter_cut(...)[0]) remain; a read left
    without a base stays a record with two empty lines.  One adapter is removed per read; each mate of a pair is cut on its own (cut
    each file).  Behind read preparation: trim_adapters(prep_fastq(text, ...)[0], ...).  Counters: trimmed (reads cut), bases_removed,
    emptied (reads of length >= 1 cut at 0), per_adapter (reads cut, by adapter)."""
    ads = check_adapters(adapters, min_overlap, error_permille)
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    out = []
    info = {"trimmed": 0, "bases_removed": 0, "emptied": 0, "per_adapter": [0] * len(ads)}
    for k in range(0, len(lines), 4):
        h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k:k + 4])
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
        cut, which = adapter_cut(s, ads, min_overlap, error_permille)
        if which >= 0:
            info["trimmed"] += 1
            info["bases_removed"] += len(s) - cut
            info["emptied"] += cut == 0
            info["per_adapter"][which] += 1
        out.append(b"%s\n%s\n%s\n%s\n" % (h, s[:cut], p, ql[:cut]))
    return b"".join(out), info


_PO_COMP = bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(c, 78) for c in range(256))      # the complement of a folded letter (N stays N)


def check_pair_overlap(min_overlap: int = 30, max_mismatches: int = 5, error_permille: int = 200) -> None:
    """ValueError for a setting mlst_set_read_pair_overlap refuses: min_overlap outside 8..320, max_mismatches outside 0..64,
    error_permille outside 0..500"""
    for name, v, lo, hi in (("min_overlap", min_overlap, 8, 320), ("max_mismatches", max_mismatches, 0, 64), ("error_permille", error_permille, 0, 500)):
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError("%s %r is outside %d..%d" % (name, v, lo, hi))


def pair_overlap(seq1: bytes, seq2: bytes, min_overlap: int = 30, max_mismatches: int = 5, error_permille: int = 200):
    """Where the reverse complement of mate 2 lies on mate 1: (o, matches), or None when the mates do not overlap.  The rule is the
    project's own, modelled on fastp's overlap analysis (no indels); it does not claim fastp's bytes.
      * Letters are folded as dedup_fastq folds them: A C G T in either case stand for themselves, every other byte is N.  c2 is the
        reverse complement of mate 2 (the complement of N is N).
      * A candidate is an offset o: letter j of c2 lies on letter o + j of mate 1, -(n2 - min_overlap) <= o <= n1 - min_overlap.  Its
        overlap is positions max(0, o) .. min(n1, o + n2) - 1 of mate 1, L of them; a candidate with L < min_overlap is none (so a mate
        shorter than min_overlap has no candidate).
      * A position matches if both letters are one of ACGT and equal: an N on either side is a mismatch.  mism = L - matches.
      * The candidate is valid if mism <= max_mismatches and mism <= (L * error_permille) // 1000 (integers).
      * The valid candidate with the most matches is chosen; among equals the smallest o.
    Limits: an insert shorter than min_overlap is not seen (that is adapter_cut's job), and two mates of one low-complexity repeat
    can overlap at a wrong offset."""
    check_pair_overlap(min_overlap, max_mismatches, error_permille)
    s1 = np.frombuffer(bytes(seq1).translate(_DD_FOLD), np.uint8)
    c2 = np.frombuffer(bytes(seq2).translate(_DD_FOLD).translate(_PO_COMP)[::-1], np.uint8)
    n1, n2 = len(s1), len(c2)
    if n1 < min_overlap or n2 < min_overlap:
        return None
    o = np.arange(-(n2 - min_overlap), n1 - min_overlap + 1)
    full = np.zeros(n1 + n2 - 1, np.int64)                   # matches per offset -(n2 - 1) .. n1 - 1
    for letter in b"ACGT":
        full += np.correlate((s1 == letter).astype(np.int64), (c2 == letter).astype(np.int64), "full")
    matches = full[o + (n2 - 1)]
    L = np.minimum(n1, o + n2) - np.maximum(0, o)
    mism = L - matches
    valid = (L >= min_overlap) & (mism <= max_mismatches) & (mism <= (L * error_permille) // 1000)
    if not valid.any():
        return None
    k = int(np.where(valid, matches, -1).argmax())           # the most matches, the smallest o among equals
    return int(o[k]), int(matches[k])


def trim_pair_overlap(text: bytes, min_overlap: int = 30, max_mismatches: int = 5, error_permille: int = 200, trim5: int = 0) -> tuple[bytes, dict]:
    """The interleaved paired FASTQ text (records 2j, 2j + 1) the engine behaves as if it had been given under
    Engine.set_read_pair_overlap(min_overlap, max_mismatches, error_permille), and the counters of Engine.read_pair_overlap_info().
    This is the rule mlst_set_read_pair_overlap applies on the device (csrc/read_overlap.h, pair_overlap per pair); it serves the tests
    and whoever wants the cut file -- the command never calls it.  When the insert is shorter than the reads, both mates run through it
    into the adapter; the overlap of the mates says where the insert ends, and no adapter sequence is needed.
      * For a pair with a chosen candidate (o, matches) the insert ends at I = o + n2 + trim5 in the coordinates of either prepared mate
        (trim5: the --trim5 in force, which took that many bases from the front of both mates).  Mate 1 keeps min(n1, I) letters, mate 2
        min(n2, I); sequence and quality lines are both cut.  Header and '+' line untouched, line ends LF.
      * A pair without a candidate stays as it is, and so does one whose I cuts neither mate (mates that overlap in their middles).
      * A mate left without a base stays a record with two empty lines (rule 4 of prep_fastq).
      * Behind prep_fastq and trim_adapters, in front of dedup_fastq.
    Counters: pairs, overlapping (pairs with a candidate), trimmed_pairs, reads_trimmed, bases_removed, emptied (mates of length >= 1
    left without a base) and insert_hist (1,024 bins, indexed by min(o + n2 + 2 * trim5, 1023): the fragment length in the file's
    coordinates; each overlapping pair is counted once).
    Limits: pair_overlap's.  Not done here: correcting mismatching bases inside the overlap, merging the mates into one read."""
    check_pair_overlap(min_overlap, max_mismatches, error_permille)
    if trim5 < 0:
        raise ValueError("trim5 must not be negative")
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    if len(lines) % 8:
        raise ValueError("paired FASTQ text holds %d records: not whole pairs" % (len(lines) // 4))
    out = []
    info = {"pairs": 0, "overlapping": 0, "trimmed_pairs": 0, "reads_trimmed": 0, "bases_removed": 0, "emptied": 0, "insert_hist": [0] * 1024}
    for k in range(0, len(lines), 8):
        pair = []
        for m in (0, 4):
            h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k + m:k + m + 4])
            if len(s) != len(ql):
                raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
            pair.append([h, s, p, ql])
        info["pairs"] += 1
        hit = pair_overlap(pair[0][1], pair[1][1], min_overlap, max_mismatches, error_permille)
        if hit is not None:
            n2 = len(pair[1][1])
            info["overlapping"] += 1
            info["insert_hist"][min(hit[0] + n2 + 2 * trim5, 1023)] += 1
            end = hit[0] + n2 + trim5
            cut = 0
            for r in pair:
                n = len(r[1])
                if end < n:
                    cut += 1
                    info["bases_removed"] += n - end
                    info["emptied"] += end == 0
                    r[1], r[3] = r[1][:end], r[3][:end]
            info["reads_trimmed"] += cut
            info["trimmed_pairs"] += cut > 0
        out += [b"%s\n%s\n%s\n%s\n" % tuple(r) for r in pair]
    return b"".join(out), info


def pair_overlap_median(hist) -> int:
    """The median insert of insert_hist (the lower median; 0 for an empty histogram)"""
    total = sum(int(v) for v in hist)
    seen = 0
    for k, v in enumerate(hist):
        seen += int(v)
        if total and 2 * seen >= total:
            return k
    return 0


def check_read_filter(letters=b"", poly_min: int = 10, min_length: int = 0, max_n=None, complexity: int = 0, mean_qual: int = 0) -> int:
    """The tail letters of Engine.set_read_filter as mlst_read_filter's poly_mask (bit 0 = A, 1 = C, 2 = G, 3 = T); ValueError for a
    setting mlst_set_read_filter refuses: a letter outside ACGT, poly_min outside 1..320 (looked at only with letters), min_length
    outside 0..320, complexity outside 0..100, mean_qual outside 0..93, and a max_n that is no unsigned 32-bit count (None: no limit)."""
    letters = (letters.encode() if isinstance(letters, str) else bytes(letters)).upper()
    if letters.strip(b"ACGT"):
        raise ValueError("tail letters %r: only A, C, G and T are taken" % letters.decode("latin-1"))
    rows = [("min_length", min_length, 0, 320), ("complexity", complexity, 0, 100), ("mean_qual", mean_qual, 0, 93)]
    if letters:
        rows.insert(0, ("poly_min", poly_min, 1, 320))
    if max_n is not None:
        rows.append(("max_n", max_n, 0, 0xFFFFFFFE))
    for name, v, lo, hi in rows:
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError("%s %r is outside %d..%d" % (name, v, lo, hi))
    return sum(1 << b"ACGT".index(c) for c in set(letters))


def poly_tail(seq: bytes, letters=b"G", min_len: int = 10) -> tuple[int, int]:
    """Where a tail of one letter is cut from the 3' end of the read seq: (new length, index of the letter in ACGT), or (len(seq), -1)
    when nothing is cut.  Two-colour machines (NovaSeq, NextSeq) call G where a cluster gives no signal, so the reads of short inserts
    and of dying clusters end in a run of G of high quality.  The rule is the project's own, modelled on fastp's --trim_poly_g /
    --trim_poly_x; it does not claim fastp's bytes.  Integers only.
      * The sequence is folded to upper case; a byte that is none of A C G T matches no letter.
      * For a letter X of `letters` and a tail length L in 1..n, mism(L) is the number of the last L bases that are not X.
      * L is valid if L >= min_len, the base at n - L is X (the tail begins on its letter) and mism(L) <= min(5, L // 8).
      * The cut is the largest valid L over all letters: n - L bases remain.  Two letters cannot share a valid L, so there is no tie.
      * The tail may step over a mismatch onto an earlier X: (ACGT) * 10 + G * 10 is cut to 38, not 40 -- the G of the last ACGT lies
        one T in front of the run, and twelve bases with one mismatch are a valid tail.  That is the rule.
    The walk from the 3' end stops at a letter's sixth mismatch: no longer tail of that letter can be valid."""
    mask = check_read_filter(letters, min_len)
    s = bytes(seq).translate(_DD_FOLD)
    n = len(s)
    best, which = 0, -1
    for x, X in enumerate(b"ACGT"):
        if not (mask >> x) & 1:
            continue
        mism = 0
        for L in range(1, n + 1):
            if s[n - L] != X:
                mism += 1
                if mism > 5:
                    break
            elif L >= min_len and mism <= min(5, L // 8) and L > best:
                best, which = L, x
    return n - best, which


def read_fails(seq: bytes, quals: bytes, min_length: int = 0, max_n=None, complexity: int = 0, mean_qual: int = 0) -> int:
    """Which filter the read (sequence and Phred+33 quality characters, n of each) fails: 0 = none, else the first that holds of
      1. too short:      0 < n < min_length;
      2. too many N:     more than max_n bytes that are none of A C G T in either case (None: no limit);
      3. low complexity: n >= 2 and 100 * d < complexity * (n - 1), d = the positions i in [0, n - 1) whose folded letters at i and i + 1
                         differ, every byte that is none of A C G T folded to N (fastp's measure, in integers);
      4. low quality:    sum(q) < mean_qual * n, q = clamp(character - 33, 0, 127).
    A read of length 0 fails nothing.  Integers only."""
    check_read_filter(b"", 10, min_length, max_n, complexity, mean_qual)
    s = bytes(seq).translate(_DD_FOLD)
    n = len(s)
    if len(quals) != n:
        raise ValueError("sequence and quality lengths differ")
    if n == 0:
        return 0
    if n < min_length:
        return 1
    if max_n is not None and sum(c == 78 for c in s) > max_n:
        return 2
    if n >= 2 and 100 * sum(s[i] != s[i + 1] for i in range(n - 1)) < complexity * (n - 1):
        return 3
    if sum(min(max(c - 33, 0), 127) for c in bytes(quals)) < mean_qual * n:
        return 4
    return 0


FILTER_REASONS = ("failed_short", "failed_n", "failed_complexity", "failed_quality")      # read_fails' 1..4


def filter_fastq(text: bytes, letters=b"", poly_min: int = 10, min_length: int = 0, max_n=None, complexity: int = 0, mean_qual: int = 0) -> tuple[bytes, dict]:
    """The FASTQ text the engine behaves as if it had been given under Engine.set_read_filter(letters, poly_min, min_length, max_n,
    complexity, mean_qual), and the counters of Engine.read_filter_info().  This is the rule mlst_set_read_filter applies on the device
    (csrc/read_filter.h); it serves the tests and whoever wants the filtered file -- the command never calls it.  Per record, header and
    '+' line untouched, line ends LF:
      1. poly_tail(sequence, letters, poly_min) of the bases and quality characters remain (letters empty: no tail trim).
      2. read_fails judges the read as it stands then; a read that fails stays a record with empty sequence and quality lines (rule 5 of
         dedup_fastq), and so does a read that was one tail.
      3. Each mate of a pair is treated on its own (filter each file): the partner of a failed mate stays.
    Its place in the chain: behind trim_pair_overlap(trim_adapters(prep_fastq(...))) and in front of dedup_fastq.  Under --phred64
    prep_fastq stands in front and has rewritten the quality characters to +33 already.
    Counters: tail_trimmed (reads whose tail was cut), tail_bases, per_letter (reads cut, by A, C, G, T), tail_emptied (reads of
    length >= 1 that were one tail), failed_short, failed_n, failed_complexity, failed_quality (reads emptied, by the first reason),
    filtered_bases (the bases those reads held behind the tail trim)."""
    check_read_filter(letters, poly_min, min_length, max_n, complexity, mean_qual)
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    out = []
    info = {"tail_trimmed": 0, "tail_bases": 0, "per_letter": [0, 0, 0, 0], "tail_emptied": 0, "failed_short": 0, "failed_n": 0,
            "failed_complexity": 0, "failed_quality": 0, "filtered_bases": 0}
    for k in range(0, len(lines), 4):
        h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k:k + 4])
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
        cut, which = poly_tail(s, letters, poly_min) if letters else (len(s), -1)
        if which >= 0:
            info["tail_trimmed"] += 1
            info["tail_bases"] += len(s) - cut
            info["per_letter"][which] += 1
            info["tail_emptied"] += cut == 0
        why = read_fails(s[:cut], ql[:cut], min_length, max_n, complexity, mean_qual)
        if why:
            info[FILTER_REASONS[why - 1]] += 1
            info["filtered_bases"] += cut
            cut = 0
        out.append(b"%s\n%s\n%s\n%s\n" % (h, s[:cut], p, ql[:cut]))
    return b"".join(out), info


WINDOW_COUNTERS = ("shortened", "front_reads", "front_bases", "right_reads", "right_bases", "tail_reads", "tail_bases", "emptied")      # mlst_read_window_info's order


def check_read_window(front=None, right=None, tail=None) -> list:
    """The three operations of Engine.set_read_window as mlst_read_window's six numbers [front_w, front_q, right_w, right_q, tail_w,
    tail_q] (0, 0 for an operation that is None: off); ValueError for what mlst_set_read_window refuses and for what is no operation:
    anything but None or a pair (W, Q) of integers, W outside 1..320, Q outside 1..93."""
    out = []
    for name, op in (("front", front), ("right", right), ("tail", tail)):
        if op is None:
            out += [0, 0]
            continue
        try:
            w, q = op
            ok = int(w) == w and int(q) == q
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("%s %r: an operation is (W, Q), two whole numbers, or None" % (name, op))
        if not 1 <= int(w) <= 320:
            raise ValueError("%s window %r is outside 1..320" % (name, w))
        if not 1 <= int(q) <= 93:
            raise ValueError("%s quality %r is outside 1..93" % (name, q))
        out += [int(w), int(q)]
    return out


def _window_steps(q, front, right, tail) -> tuple[int, int, int]:      # (f, e behind right, e behind tail) of window_cut
    n = len(q)
    f, e = 0, n
    P = [0] * (n + 1)      # P[i] = sum(q[:i]): the sum of a window [a, a + w) is P[a + w] - P[a]
    for i, v in enumerate(q):
        P[i + 1] = P[i] + v
    if front is not None and n > 0:
        W, Q = front
        w = min(W, n)
        f = next((s for s in range(n - w + 1) if P[s + w] - P[s] >= Q * w), n)
    if right is not None and n - f > 0:
        W, Q = right
        w = min(W, n - f)
        bad = next((s for s in range(f, n - w + 1) if P[s + w] - P[s] < Q * w), None)
        if bad is not None:
            k = 0
            while q[bad + k] >= Q:      # (one value of a failing window is below Q: k < w)
                k += 1
            e = bad + k
    er = e
    if tail is not None and e - f > 0:
        W, Q = tail
        w = min(W, e - f)
        e = next((t for t in range(e, f + w - 1, -1) if P[t] - P[t - w] >= Q * w), f)
    return f, er, e


def window_cut(q, front=None, right=None, tail=None) -> tuple[int, int]:
    """Where the sliding-window quality cuts leave the read with the Phred values q[0..n): (f, e), values [f, e) remain.  The rule is the
    project's own, in integers, modelled on fastp's cut_front / cut_right / cut_tail; it claims neither fastp's nor Trimmomatic's bytes.
    Each operation is (W, Q), W in 1..320, Q in 1..93, or None = off; pass(a, w) is sum(q[a : a + w]) >= Q * w.  In this order:
      1. front.  If n > 0: w = min(W, n); f = the smallest s in [0, n - w] with pass(s, w); none: f = n, the read is left without a base.
         Off: f = 0.
      2. right, on [f, n).  If n - f > 0: w = min(W, n - f); s* = the smallest s in [f, n - w] with not pass(s, w); none: e = n; otherwise
         e = s* + k, k = the number of leading values of that window that are >= Q (the good bases at the front of the first bad
         window stay; k < w always).  Off: e = n.
      3. tail, on [f, e).  If e - f > 0: w = min(W, e - f); t = the largest t in [f + w, e] with pass(t - w, w); none: t = f.  e = t.
    W = 1 gives Trimmomatic's LEADING:Q / TRAILING:Q (bases below Q are dropped from that end); right=(4, 15) is the model of
    SLIDINGWINDOW:4:15.  A read that front empties answers (n, n)."""
    check_read_window(front, right, tail)
    f, _, e = _window_steps(list(q), front, right, tail)
    return f, e


def cut_windows(text: bytes, front=None, right=None, tail=None, phred64: bool = False) -> tuple[bytes, dict]:
    """The FASTQ text the engine behaves as if it had been given under Engine.set_read_window(front, right, tail), and the counters of
    Engine.read_window_info().  This is the rule mlst_set_read_window applies on the device (csrc/read_window.h, window_cut per read); it
    serves the tests and whoever wants the cut file -- the command never calls it.  Per record, header and '+' line untouched, line ends
    LF: q[i] = clamp(character - base, 0, 127), base 64 under phred64, else 33, exactly as step 1 of prep_fastq; bases and quality
    characters [f, e) of window_cut(q, ...) remain (under phred64 the characters are written back as q[i] + 33, as prep_fastq writes
    them; else they stay the file's); a read left without a base stays a record with two empty lines.  Each mate of a pair is cut on its
    own (cut each file).  Its place in the chain: directly behind prep_fastq -- which has rewritten Phred+64 text to +33 already, so
    phred64 stays False there -- and in front of trim_adapters: filter_fastq(trim_pair_overlap(trim_adapters(cut_windows(prep_fastq(...)))))
    , then dedup_fastq.
    Counters: shortened (reads whose length changed), front_reads / front_bases, right_reads / right_bases, tail_reads / tail_bases
    (reads cut by the operation and the bases it removed; a read emptied by front adds all n of its bases to front_bases), emptied
    (reads of length >= 1 left without a base)."""
    check_read_window(front, right, tail)
    base = 64 if phred64 else 33
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    out = []
    info = dict.fromkeys(WINDOW_COUNTERS, 0)
    for k in range(0, len(lines), 4):
        h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k:k + 4])
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
        n = len(s)
        q = [min(max(c - base, 0), 127) for c in ql]
        f, er, e = _window_steps(q, front, right, tail)
        for name, cut in (("front", f), ("right", n - er), ("tail", er - e)):
            if cut:
                info[name + "_reads"] += 1
                info[name + "_bases"] += cut
        if e - f != n:
            info["shortened"] += 1
            info["emptied"] += e == f
        out.append(b"%s\n%s\n%s\n%s\n" % (h, s[f:e], p, bytes(v + 33 for v in q[f:e]) if phred64 else ql[f:e]))
    return b"".join(out), info


DEDUP_LEVELS = (1, 2, 3, 4, 5, 10, 50, 500)      # the lower edges of the eight levels: keys that occur 1, 2, 3, 4, 5-9, 10-49, 50-499, >= 500 times
_DD_FOLD = bytes(c if c in b"ACGT" else (c & 0xDF if (c & 0xDF) in b"ACGT" else 78) for c in range(256))      # a letter as the engine aligns it (78: 'N')


def dedup_level(count: int) -> int:
    """The level (0..7) of a key that occurs `count` >= 1 times"""
    return sum(count >= e for e in DEDUP_LEVELS) - 1


def dedup_fastq(text: bytes, paired: bool = False) -> tuple[bytes, dict]:
    """The FASTQ text the engine behaves as if it had been given under Engine.set_read_dedup(), and the counters of
    Engine.read_dedup_info().  This is the rule mlst_set_read_dedup applies on the device (csrc/read_dedup.h) -- there on 128-bit
    hashes of the keys (MLST_DEDUP_KEY of include/mlst_policy.h), here on the letters themselves; it serves the tests and whoever
    wants the deduplicated file -- the command never calls it.
      1. A read's letters are its sequence line as the engine aligns it: A, C, G, T in either case stand for themselves, every other
         byte is N (pack_group's N bit, _RS_COL's folding).  Its key is (length, folded letters); qualities and names play no part.
      2. Unpaired: a read is a duplicate if an earlier read of the text has the same key.  The first occurrence is kept.
      3. paired (records 2j and 2j + 1): pair j is a duplicate if an earlier pair has the same key for mate 1 AND for mate 2, in that
         order (swapped mates are not duplicates); both mates of a duplicate pair go, otherwise both stay.
      4. A read of length 0 -- a pair whose mates are both empty -- is neither a duplicate nor a first occurrence; a pair with one
         empty mate takes part as it is.
      5. A duplicate stays a record: header and '+' line untouched, sequence and quality lines empty, line ends LF.
      6. Only the same orientation counts: a reverse complement is no duplicate.
      7. Behind the preparation: dedup_fastq(trim_adapters(prep_fastq(text, ...)[0], ...)[0], paired).
    Counters: reads (records seen), units (reads or pairs that took part), duplicates (units removed), reads_removed, bases_removed,
    distinct (keys), levels (eight: the distinct keys that occur 1, 2, 3, 4, 5-9, 10-49, 50-499 and >= 500 times)."""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    if paired and len(lines) % 8:
        raise ValueError("paired FASTQ text holds %d records: not whole pairs" % (len(lines) // 4))
    recs = []
    for k in range(0, len(lines), 4):
        h, s, p, ql = (x[:-1] if x.endswith(b"\r") else x for x in lines[k:k + 4])
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % h[:60])
        recs.append([h, s, p, ql])
    info = {"reads": len(recs), "units": 0, "duplicates": 0, "reads_removed": 0, "bases_removed": 0, "distinct": 0, "levels": [0] * 8}
    step = 2 if paired else 1
    seen = {}
    for j in range(0, len(recs), step):
        unit = recs[j:j + step]
        key = tuple(r[1].translate(_DD_FOLD) for r in unit)
        if not any(key):
            continue
        info["units"] += 1
        if key in seen:
            seen[key] += 1
            info["duplicates"] += 1
            for r in unit:
                info["reads_removed"] += 1
                info["bases_removed"] += len(r[1])
                r[1] = r[3] = b""
        else:
            seen[key] = 1
    info["distinct"] = len(seen)
    for c in seen.values():
        info["levels"][dedup_level(c)] += 1
    return b"".join(b"%s\n%s\n%s\n%s\n" % tuple(r) for r in recs), info


# the table block of mlst_read_stats_fetch in 64-bit words (MLST_RS_* of include/mlst.h): reads, bases, clamped_low, padding, then
RS_LEN, RS_BASE, RS_QUAL, RS_GC, RS_READQUAL, RS_WORDS = 4, 325, 1925, 32005, 32106, 32200
_RS_COL = np.full(256, 4, np.int64)      # letter -> column of base[c]: A, C, G, T in either case, 4 = every other byte (pack_group's N bit)
for _k, _c in enumerate(b"ACGT"):
    _RS_COL[_c] = _RS_COL[_c | 0x20] = _k


def read_stats_empty() -> dict:
    """One side's tables, all zero"""
    return {"reads": 0, "bases": 0, "clamped_low": 0, "len_hist": np.zeros(321, np.int64), "base": np.zeros((320, 5), np.int64),
            "qual": np.zeros((320, 94), np.int64), "gc_hist": np.zeros(101, np.int64), "readqual_hist": np.zeros(94, np.int64)}


def read_stats_sum(a: dict, b: dict) -> dict:
    """The tables of two texts counted into one side: every figure is additive"""
    return {k: a[k] + b[k] for k in a}


def read_stats_equal(a: dict, b: dict, skip=()) -> bool:
    return all(np.array_equal(a[k], b[k]) for k in a if k not in skip)


def read_stats(text: bytes, phred64: bool = False, side: int = 0, paired: bool = False) -> list:
    """The tables Engine.read_stats() holds for FASTQ text under Engine.set_read_stats(): [side 0, side 1], each a dict of reads, bases,
    clamped_low (int) and len_hist (321), base (320 x 5), qual (320 x 94), gc_hist (101), readqual_hist (94) as numpy int64.  This is the
    rule mlst_set_read_stats counts by on the device (csrc/read_stats.h); it serves the tests and the docs -- the command never calls it.
    Sides: paired -- record 2k is side 0 and record 2k + 1 side 1 (interleaved text); else every record counts into `side`.
    Per side, over its records (a record of more than 320 bases is refused, as the engine refuses it):
      reads, bases = the sum of lengths; len_hist[n]: reads of length n (a read of length 0 counts here and in reads only);
      base[c][0..4]: letters A, C, G, T (either case) and other at cycle c -- other is every byte the packed rows mark non-ACGT;
      qual[c][v]: v = min(clamp(character - base, 0, 127), 93) at cycle c, base 64 under phred64, else 33, the character 0..255
        (under base 33 every character of 128 and above lands in bin 93);
      gc_hist[(100 * (#G + #C)) // n] and readqual_hist[(sum of v) // n] for reads of length n >= 1;
      clamped_low: quality characters below the base.
    The stage "raw" of the engine is read_stats(text, phred64=...) of the file; "prepared" is
    read_stats(trim_adapters(prep_fastq(text, ...)[0], ...)[0]) with base 33 (prep_fastq writes Phred + 33)."""
    base = 64 if phred64 else 33
    if side not in (0, 1):
        raise ValueError("side is %r, not 0 or 1" % (side,))
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("FASTQ text holds %d lines: not a whole number of 4-line records" % len(lines))
    if paired and len(lines) % 8:
        raise ValueError("paired FASTQ text holds %d records: not whole pairs" % (len(lines) // 4))
    out = [read_stats_empty(), read_stats_empty()]
    cyc, col, val = ([], []), ([], []), ([], [])
    for k in range(0, len(lines), 4):
        s, ql = (x[:-1] if x.endswith(b"\r") else x for x in (lines[k + 1], lines[k + 3]))
        if len(s) != len(ql):
            raise ValueError("FASTQ record with different sequence and quality lengths: %r" % lines[k][:60])
        n = len(s)
        if n > 320:
            raise ValueError("a FASTQ read is longer than 320 bases")
        sd = (k // 4) & 1 if paired else side
        t = out[sd]
        t["reads"] += 1
        t["bases"] += n
        t["len_hist"][n] += 1
        if not n:
            continue
        c = _RS_COL[np.frombuffer(s, np.uint8)]
        ch = np.frombuffer(ql, np.uint8).astype(np.int64)
        v = np.minimum(np.clip(ch - base, 0, 127), 93)
        t["clamped_low"] += int((ch < base).sum())
        t["gc_hist"][(100 * int(((c == 1) | (c == 2)).sum())) // n] += 1
        t["readqual_hist"][int(v.sum()) // n] += 1
        cyc[sd].append(np.arange(n)); col[sd].append(c); val[sd].append(v)
    for sd in (0, 1):
        if cyc[sd]:
            cc, bb, vv = np.concatenate(cyc[sd]), np.concatenate(col[sd]), np.concatenate(val[sd])
            out[sd]["base"] += np.bincount(cc * 5 + bb, minlength=1600).reshape(320, 5)
            out[sd]["qual"] += np.bincount(cc * 94 + vv, minlength=320 * 94).reshape(320, 94)
    return out


def read_stats_text(stats: dict, sample: str, phred64: bool | None = None, prepared: bool | None = None) -> bytes:
    """The report file of `cli type --read-stats`, <out>/<sample>.readstats.tsv.  stats: {"raw": [side 0, side 1], "prepared": [...]}
    as Engine.read_stats() returns it (its keys "phred_base" and "prepared_counted" stand in for phred64 / prepared when those are
    None).  The format is the project's own and claims no other tool's bytes: integers only, tab-separated, LF line ends.
      #metamlst-readstats<TAB>1                      format version
      #sample<TAB><sample>
      #phred_base<TAB>33 | 64
      #stages<TAB>raw | raw,prepared                 the stages that were counted (prepared: only where a trim or an adapter ran)
      #columns<TAB>table<TAB>stage<TAB>side<TAB>index<TAB>values
    then, per counted stage (raw, prepared) and side (0; 1 only where it holds reads), rows `table stage side index values...`:
      total    index 0, values reads, bases, clamped_low
      len      index = length, value = reads of that length; non-zero rows only
      base     index = cycle 0 .. longest read - 1, values A, C, G, T, other
      qual     index = cycle 0 .. longest read - 1, values for Phred 0 .. the highest non-empty bin of that stage's and side's table
      gc       index = GC percent 0 .. 100, value = reads; non-zero rows only
      readqual index = mean Phred, value = reads; non-zero rows only"""
    base = (64 if phred64 else 33) if phred64 is not None else int(stats.get("phred_base", 33))
    with_prep = bool(stats.get("prepared_counted", False)) if prepared is None else bool(prepared)
    stages = ["raw"] + (["prepared"] if with_prep else [])
    out = ["#metamlst-readstats\t1", "#sample\t%s" % sample, "#phred_base\t%d" % base, "#stages\t%s" % ",".join(stages),
           "#columns\ttable\tstage\tside\tindex\tvalues"]
    for stage in stages:
        for side in (0, 1):
            t = stats[stage][side]
            if side and not int(t["reads"]):
                continue
            key = "\t%s\t%d\t" % (stage, side)
            out.append("total" + key + "0\t%d\t%d\t%d" % (int(t["reads"]), int(t["bases"]), int(t["clamped_low"])))
            nz = np.flatnonzero(t["len_hist"])
            out += ["len" + key + "%d\t%d" % (i, int(t["len_hist"][i])) for i in nz]
            longest = int(nz[-1]) if len(nz) else 0
            out += ["base" + key + "%d\t" % c + "\t".join(str(int(x)) for x in t["base"][c]) for c in range(longest)]
            qn = np.flatnonzero(t["qual"].sum(axis=0))
            top = int(qn[-1]) + 1 if len(qn) else 0
            out += ["qual" + key + "%d\t" % c + "\t".join(str(int(x)) for x in t["qual"][c][:top]) for c in range(longest)]
            out += ["gc" + key + "%d\t%d" % (i, int(t["gc_hist"][i])) for i in np.flatnonzero(t["gc_hist"])]
            out += ["readqual" + key + "%d\t%d" % (i, int(t["readqual_hist"][i])) for i in np.flatnonzero(t["readqual_hist"])]
    return ("\n".join(out) + "\n").encode()


def phred_hint(stats: dict, phred64: bool | None = None) -> str | None:
    """One sentence of advice on the Phred base from the raw tables of both sides, or None.  Under base 33: at least 1,000 bases
    counted and no quality below Phred 31 (character '@') -- the file looks like Phred+64.  Under base 64: a quality character below
    64 was seen (clamped_low) -- the file is not Phred+64.  The hint only advises; nothing applies it."""
    base = (64 if phred64 else 33) if phred64 is not None else int(stats.get("phred_base", 33))
    raw = stats["raw"]
    bases = sum(int(t["bases"]) for t in raw)
    if base == 33:
        if bases >= 1000 and not sum(int(t["qual"][:, :31].sum()) for t in raw):
            return ("read statistics: no quality character below '@' in %d bases -- the file looks like Phred+64 (Illumina 1.3 - 1.7): "
                    "type it with --phred64" % bases)
        return None
    low = sum(int(t["clamped_low"]) for t in raw)
    if low:
        return ("read statistics: %d quality characters lie below '@' (64) -- the file does not look like Phred+64: "
                "type it without --phred64" % low)
    return None


def _bgzf_block_size(buf, off: int) -> int:
    """Total size of the BGZF block that starts at buf[off], 0 if the header is incomplete, -1 if it is not BGZF."""
    if len(buf) - off < 18:
        return 0
    if buf[off] != 0x1F or buf[off + 1] != 0x8B or buf[off + 2] != 8 or not (buf[off + 3] & 4):
        return -1
    xlen = buf[off + 10] | (buf[off + 11] << 8)
    if len(buf) - off < 12 + xlen:
        return 0
    o = 0
    while o + 4 <= xlen:
        p = off + 12 + o
        slen = buf[p + 2] | (buf[p + 3] << 8)
        if buf[p] == 66 and buf[p + 1] == 67 and slen == 2:
            return (buf[p + 4] | (buf[p + 5] << 8)) + 1
        o += 4 + slen
    return -1


def is_bgzf(path: str) -> bool:
    with open(path, "rb") as f:
        return _bgzf_block_size(f.read(4096), 0) > 0


def bgzf_chunks(path: str, chunk_bytes: int = 256 << 20):
    """Yield (compressed bytes holding whole BGZF blocks, is_last) for Engine.submit_fastq_bgzf.  The only host work is
    walking the block headers; inflating and parsing happen on the GPU."""
    carry = b""
    pending = None
    with open(path, "rb") as f:
        while True:
            block = f.read(chunk_bytes)
            data = carry + block
            off = 0
            while True:
                n = _bgzf_block_size(data, off)
                if n < 0:
                    raise ValueError("%s: not a BGZF block at byte offset %d of a chunk" % (path, off))
                if n == 0 or off + n > len(data):
                    break
                off += n
            if pending is not None:
                yield pending, False
            pending = data[:off] if off else None
            carry = data[off:]
            if not block:
                break
    if carry:
        raise ValueError("%s: truncated BGZF block at the end of the file" % path)
    yield (pending if pending is not None else b""), True


# ---- byte ranges of a bgzip'd FASTQ (one range per GPU: metamlst_amd/multigpu.py) -------------------------------------
def bgzf_find_block(f, pos: int, size: int) -> int:
    """Offset of the first BGZF block that starts at or after `pos` (`size` when there is none).  A candidate -- the gzip
    magic with the FEXTRA flag and a 'BC' subfield -- counts when the block it announces is followed by another valid
    header or by the end of the file (deflate data may contain the magic bytes by chance)."""
    if pos <= 0:
        return 0
    at = pos
    while at < size:
        f.seek(at)
        win = f.read((1 << 17) + 64)
        if len(win) < 18:
            return size
        i = 0
        while True:
            i = win.find(b"\x1f\x8b\x08\x04", i)
            if i < 0 or i + 18 > len(win):
                break
            n = _bgzf_block_size(win, i)
            if n > 0:
                nxt = at + i + n
                if nxt == size:
                    return at + i
                if nxt < size:
                    f.seek(nxt)
                    h2 = f.read(64)
                    n2 = _bgzf_block_size(h2, 0)
                    if n2 > 0 or (n2 == 0 and len(h2) >= 18 and h2[:4] == b"\x1f\x8b\x08\x04"):
                        return at + i
            i += 1
        at += 1 << 17
    return size


class BgzfCrcError(ValueError):
    """the text of the BGZF block at file offset `offset` does not have the CRC-32 of the block's trailer (host-inflated blocks)"""

    def __init__(self, offset: int, stored: int, computed: int):
        super().__init__("CRC mismatch in the BGZF block at byte %d (stored 0x%08x, computed 0x%08x)" % (offset, stored, computed))
        self.offset, self.stored, self.computed = offset, stored, computed


def _bgzf_read_block(f, off: int, verify_crc: bool = False):
    """(total compressed size, inflated text) of the block at `off`; (0, b"") at the end of the file.  verify_crc: the text
    must have the CRC-32 of the block's trailer (the raw inflate checks nothing): BgzfCrcError (a ValueError) with the block's offset."""
    import zlib
    f.seek(off)
    head = f.read(18)
    if len(head) < 18:
        return 0, b""
    n = _bgzf_block_size(head, 0)
    if n == 0:                                     # extra field longer than usual: read more of the header
        f.seek(off)
        head = f.read(4096)
        n = _bgzf_block_size(head, 0)
    if n <= 0:
        raise ValueError("not a BGZF block at byte %d" % off)
    f.seek(off)
    blk = f.read(n)
    xlen = blk[10] | (blk[11] << 8)
    text = zlib.decompress(blk[12 + xlen:n - 8], -15)
    if verify_crc:
        stored, got = int.from_bytes(blk[n - 8:n - 4], "little"), zlib.crc32(text) & 0xFFFFFFFF
        if stored != got:
            raise BgzfCrcError(off, stored, got)
    return n, text


def bgzf_split(f, block_off: int, size: int, verify_crc: bool = False):
    """Where the records of two neighbouring byte ranges part, for the range boundary at the block that starts at
    `block_off`: -> (end, text, p).  `text` is the inflated text of the blocks block_off .. end, `p` the offset in it of
    the first record that starts behind the first line break (record_start(text, 1)): text[:p] completes the last record
    of the range before, text[p:] opens the range behind.  Both ranks evaluate this same function, so they agree.  At
    the end of the file p = len(text).  verify_crc: as _bgzf_read_block, for every block inflated here."""
    text, at = b"", block_off
    while at < size:
        n, t = _bgzf_read_block(f, at, verify_crc)
        if n == 0:
            break
        at += n
        text += t
        p = record_start(text, 1)
        if p >= 0:
            return at, text, p
    return at, text, len(text)


def bgzf_range_plan(path: str, lo: int, hi: int, verify_crc: bool = False):
    """What the rank owning compressed bytes [lo, hi) of a bgzip'd FASTQ submits: {head: text to submit first (host
    inflated), mid: (first, end) compressed byte range of whole blocks to submit as BGZF, tail: text that completes the
    last record}.  A range without a block start owns nothing.  verify_crc: every block inflated here (the boundary blocks,
    which never reach the device's check) must have the CRC-32 of its trailer: ValueError naming the block's file offset.
    With the device's check on for `mid`, every block of a sharded file is checked by whoever inflates it."""
    size = os.path.getsize(path)
    hi = min(hi, size)
    with open(path, "rb") as f:
        b_lo = bgzf_find_block(f, lo, size)
        b_hi = bgzf_find_block(f, hi, size) if hi < size else size
        if b_lo >= b_hi:
            return {"head": b"", "mid": (b_lo, b_lo), "tail": b""}
        if lo > 0:
            e_lo, t_lo, p_lo = bgzf_split(f, b_lo, size, verify_crc)
        else:
            e_lo, t_lo, p_lo = b_lo, b"", 0
        if b_hi < size:
            e_hi, t_hi, p_hi = bgzf_split(f, b_hi, size, verify_crc)
        else:
            e_hi, t_hi, p_hi = size, b"", 0
        if e_lo > b_hi:
            # the blocks inflated for the head reach into the next range (tiny ranges): both cuts lie in t_lo.
            # text position of block b_hi inside t_lo = inflated size of the blocks b_lo .. b_hi
            pos, at = 0, b_lo
            while at < b_hi:
                n, t = _bgzf_read_block(f, at, verify_crc)
                at += n
                pos += len(t)
            cut = pos + p_hi if b_hi < size else len(t_lo)
            if e_hi > e_lo:                       # the next boundary's record start lies beyond what the head inflated
                f_text, at = t_lo, e_lo
                while at < e_hi:
                    n, t = _bgzf_read_block(f, at, verify_crc)
                    at += n
                    f_text += t
                t_lo = f_text
            return {"head": t_lo[p_lo:max(cut, p_lo)], "mid": (b_hi, b_hi), "tail": b""}
        return {"head": t_lo[p_lo:], "mid": (e_lo, b_hi), "tail": t_hi[:p_hi]}
