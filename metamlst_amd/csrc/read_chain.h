// The read chain on the host ("The read chain"): what strings the eight read-preparation stages of the FASTQ path together.  The kernels are
// in csrc/read_names.h, read_prep.h, read_window.h, read_adapt.h, read_stats.h, read_dedup.h, read_overlap.h and read_filter.h, the state of
// each stage in mlst_handle (h->rn, rp, rw, ra, rs, dd, po, rf).  Here, once for all of them: which entries a switch closes (chain_refuse), when a switch may
// change (chain_gate), the order of the stages over a parsed chunk (chain_apply), the counters' first use and read-back (chain_ctr,
// chain_fetch), what a new sample and the end of the handle do (chain_reset, chain_free), and the public setters and readers.
// A new stage is one row in chain_refuse, one line in chain_apply, chain_reset and chain_free, and its setter.
// Host code only; included by mlst_engine.hip behind mlst_handle, fail, HIPCHK, Prof, dmalloc, grid_for, dd_clear and the declarations of
// bz_flush, bam_is_open and bam_kind.
#pragma once

// ---- which entries take prepared reads
// With a switch on, reads come from the FASTQ text and BGZF entries only, where the chain runs: every other way of adding reads, and
// mlst_set_read_tiling (a window has no name and no mate, and is cut from the record as it stands), is refused.  The first switch
// that is on, in this order, gives the message
static int chain_refuse(mlst_handle* h, const char* entry) {
    if (!h) return MLST_OK;
    const struct { bool on; const char* fmt; } rows[] = {
        {h->rn.on, "%s: read names are on (mlst_set_read_names) and only the FASTQ text and BGZF entries carry names"},
        {h->rp.on, "%s: read preparation is on (mlst_set_read_prep) and only the FASTQ text and BGZF entries apply it"},
        {h->ra.on, "%s: adapter removal is on (mlst_set_read_adapters) and only the FASTQ text and BGZF entries apply it"},
        {h->rs.on, "%s: read statistics are on (mlst_set_read_stats) and only the FASTQ text and BGZF entries count their reads"},
        {h->dd.on, "%s: duplicate removal is on (mlst_set_read_dedup) and only the FASTQ text and BGZF entries apply it"},
        {h->po.on, "%s: mate overlap trimming is on (mlst_set_read_pair_overlap) and only the paired FASTQ text and BGZF entries apply it"},
        {h->rf.on, "%s: the read filter is on (mlst_set_read_filter) and only the FASTQ text and BGZF entries apply it"},
        {h->rw.on, "%s: the quality windows are on (mlst_set_read_window) and only the FASTQ text and BGZF entries apply them"},
    };
    for (const auto& r : rows) if (r.on) return fail(h, MLST_E_INVALID, r.fmt, entry);
    return MLST_OK;
}

// ---- when a switch may change
// Only while no stream is open and the sample holds no reads: one sample is prepared one way, and a read submitted without a switch
// has no name to give.  name: the setter; changes: the call would leave another setting than it found; turns_on: the switch is on
// afterwards; tile_text: the setter's sentence on mlst_set_read_tiling, whole (nullptr: the stream checks alone, mlst_set_read_stats_side)
static int chain_gate(mlst_handle* h, const char* name, bool changes, bool turns_on, const char* tile_text) {
    if (h->bz_pend.on || h->bzp.on || h->pair_open || h->fq_carry_len) return fail(h, MLST_E_INVALID, "a FASTQ stream is open (its last chunk was not marked final)");
    if (bam_is_open(h)) return fail(h, MLST_E_INVALID, "a %s stream is open (its last chunk was not marked final)", bam_kind(h));
    if (!tile_text) return MLST_OK;
    if (changes && h->reads_seen) return fail(h, MLST_E_INVALID, "the sample holds reads: %s changes only before the first submission or behind mlst_reset_sample (a read index base counts as reads)", name);
    if (turns_on && h->tile.read_len) return fail(h, MLST_E_INVALID, "%s", tile_text);
    return MLST_OK;
}

// ---- counters: first use and read-back
// one zeroed counter struct on the device, allocated by the first submission that needs it
template <typename T> static int chain_ctr(mlst_handle* h, T** p) {
    if (*p) return MLST_OK;
    HIPCHK(h, dmalloc(p, (u64)1)); HIPCHK(h, hipMemsetAsync(*p, 0, sizeof(T), h->stream));
    return MLST_OK;
}
// a stage's counters on the host: all zero with the switch off (live == false) or before the first use.  The pointer is taken by
// address: a BGZF piece in flight is part of the sample, and the flush that submits it may be the first use
template <typename T> static int chain_fetch(mlst_handle* h, bool live, T* const* d_ctr, T* c) {
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }
    memset(c, 0, sizeof *c);
    if (!live || !*d_ctr) return MLST_OK;
    HIPCHK(h, hipMemcpyAsync(c, *d_ctr, sizeof *c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLST_OK;
}

// ---- a new sample, the end of the handle
// the counters, tables and keys are the sample's; the switches, their settings and the dedup table's size stay (the side of
// mlst_set_read_stats_side is 0 again)
static int chain_reset(mlst_handle* h) {
    if (h->rn.d_ctr) HIPCHK(h, hipMemsetAsync(h->rn.d_ctr, 0, sizeof(RnCtr), h->stream));      // (the name arena is empty)
    if (h->rp.d_ctr) HIPCHK(h, hipMemsetAsync(h->rp.d_ctr, 0, sizeof(RpCtr), h->stream));
    if (h->ra.d_ctr) HIPCHK(h, hipMemsetAsync(h->ra.d_ctr, 0, sizeof(RaCtr), h->stream));
    if (h->rs.d_tab) HIPCHK(h, hipMemsetAsync(h->rs.d_tab, 0, 4ull * RS_WORDS * 8, h->stream));
    h->rs.side = 0; h->rs.launches[0] = h->rs.launches[1] = 0;
    if (h->dd.d_mem) { int rc = dd_clear(h, h->dd.tab); if (rc) return rc; }
    if (h->dd.d_ctr) HIPCHK(h, hipMemsetAsync(h->dd.d_ctr, 0, sizeof(DdCtr), h->stream));
    h->dd.units_seen = h->dd.reads = 0;
    if (h->po.d_ctr) HIPCHK(h, hipMemsetAsync(h->po.d_ctr, 0, sizeof(PoCtr), h->stream));
    h->po.pairs = 0;
    if (h->rf.d_ctr) HIPCHK(h, hipMemsetAsync(h->rf.d_ctr, 0, sizeof(RfCtr), h->stream));
    if (h->rw.d_ctr) HIPCHK(h, hipMemsetAsync(h->rw.d_ctr, 0, sizeof(RwCtr), h->stream));
    return MLST_OK;
}
// (the name arena is freed with the retained-read store it is sized by: free_state)
static void chain_free(mlst_handle* h) {
    hipFree(h->rp.d_ctr); hipFree(h->ra.d_ctr); hipFree(h->rs.d_tab); hipFree(h->po.d_ctr); hipFree(h->rf.d_ctr); hipFree(h->rw.d_ctr);
    hipFree(h->dd.d_mem); hipFree(h->dd.d_ctr); hipFree(h->dd.d_slot_of); hipFree(h->dd.d_key2);
}

// ---- the stages over one parsed chunk
// mlst_set_read_names: the name arena, allocated by the first submission under the switch (csrc/read_names.h)
static int rn_ensure(mlst_handle* h) {
    auto& N = h->rn;
    if (N.d_ctr) return MLST_OK;
    { int rc = chain_ctr(h, &N.d_ctr); if (rc) return rc; }
    HIPCHK(h, dmalloc(&N.d_bytes, N.want_bytes)); N.cap_bytes = N.want_bytes;
    HIPCHK(h, dmalloc(&N.d_off, h->E.cap_ret)); HIPCHK(h, dmalloc(&N.d_len, h->E.cap_ret));
    return MLST_OK;
}
// the counters of the name arena; an arena that was too small is reported here (the next entry that looks)
static int rn_fetch(mlst_handle* h, RnCtr* c) {
    memset(c, 0, sizeof *c);
    if (!h->rn.d_ctr) return MLST_OK;
    HIPCHK(h, hipMemcpyAsync(c, h->rn.d_ctr, sizeof *c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (c->err) return fail(h, MLST_E_LIMIT, "the read names need %llu bytes and the arena holds %llu: raise MLST_NAMES_BYTES", (unsigned long long)c->bytes, (unsigned long long)h->rn.cap_bytes);
    return MLST_OK;
}
// one launch of k_rs_count over the chunk's reads as offsets and lengths stand now: stage 0 in front of k_rp_qtrim (which rewrites the
// offsets in place), stage 1 behind the last kernel that shortens reads.  At most one workgroup per CU, fewer for few reads (each
// flushes its LDS tables once); a paired chunk takes an even number, a workgroup counting one side
static int rs_launch(mlst_handle* h, u64 n_reads, u32* d_flags, int paired, int stage) {
    auto& S = h->rs;
    if (!S.d_tab) { HIPCHK(h, dmalloc(&S.d_tab, 4ull * RS_WORDS)); HIPCHK(h, hipMemsetAsync(S.d_tab, 0, 4ull * RS_WORDS * 8, h->stream)); }
    if (!S.n_cu) { HIPCHK(h, hipDeviceGetAttribute(&S.n_cu, hipDeviceAttributeMultiprocessorCount, h->device)); if (S.n_cu < 2) S.n_cu = 2; }
    u64 want = (n_reads + RS_WG_READS - 1) / RS_WG_READS; if (want < 1) want = 1;
    u32 grid = (u32)std::min<u64>(want, (u64)S.n_cu);
    if (paired) { grid = (grid + 1) & ~1u; if (grid > (u32)S.n_cu) grid -= 2; if (grid < 2) grid = 2; }
    u64* const tab = S.d_tab + (u64)stage * 2 * RS_WORDS;
    Prof pf(h, 20);      // (mlst_get_kernel_time 20: k_rs_count alone)
    if (h->rp.set.phred_base == 64) hipLaunchKernelGGL(k_rs_count<64>, dim3(grid), dim3(1024), 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, (const u64*)h->d_fq_qoff,
                                                       (const u16*)h->d_lens, n_reads, paired ? 1u : 0u, S.side, stage == 0 ? 1u : 0u, (const u32*)d_flags, tab);
    else hipLaunchKernelGGL(k_rs_count<33>, dim3(grid), dim3(1024), 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, (const u64*)h->d_fq_qoff,
                            (const u16*)h->d_lens, n_reads, paired ? 1u : 0u, S.side, stage == 0 ? 1u : 0u, (const u32*)d_flags, tab);
    S.launches[stage]++;
    return MLST_OK;
}
// mlst_set_read_dedup: the table, the counters and the per-unit scratch in front of a chunk of n_units units.  The table holds at least
// two slots per unit submitted so far and in this chunk -- the host knows both numbers without a read-back; one that is too small is
// replaced by the next power of two that is not, and k_dd_rehash moves the keys
static int dd_ensure(mlst_handle* h, u64 n_units) {
    auto& D = h->dd;
    { int rc = chain_ctr(h, &D.d_ctr); if (rc) return rc; }
    if (D.cap_units < n_units) {
        hipFree(D.d_slot_of); hipFree(D.d_key2); D.d_slot_of = nullptr; D.d_key2 = nullptr; D.cap_units = 0;
        HIPCHK(h, dmalloc(&D.d_slot_of, n_units)); HIPCHK(h, dmalloc(&D.d_key2, n_units)); D.cap_units = n_units;
    }
    u64 slots = D.tab.slots, tag_mask = D.tab.tag_mask;
    if (!slots) {      // the first table: the two environment switches are read here
        slots = 1ull << 22; tag_mask = ~0ull;
        if (const char* e = getenv("MLST_DEDUP_SLOTS")) {
            const long long v = atoll(e);
            if (v < 64 || v > (1ll << 31) || (v & (v - 1))) return fail(h, MLST_E_INVALID, "MLST_DEDUP_SLOTS is %s: a power of two from 64 to 2^31 is taken", e);
            slots = (u64)v;
        }
        if (const char* e = getenv("MLST_DEDUP_TAG_BITS")) {
            const int v = atoi(e);
            if (v < 0 || v > 64 || !(e[0] >= '0' && e[0] <= '9')) return fail(h, MLST_E_INVALID, "MLST_DEDUP_TAG_BITS is %s: 0 to 64 is taken", e);
            tag_mask = v >= 64 ? ~0ull : (1ull << v) - 1;
        }
    }
    const u64 need = 2 * (D.units_seen + n_units);
    while (slots < need && slots < (1ull << 31)) slots <<= 1;
    if (slots < need) return fail(h, MLST_E_LIMIT, "mlst_set_read_dedup: %llu units need more than 2^31 slots", (unsigned long long)(D.units_seen + n_units));
    if (slots == D.tab.slots) return MLST_OK;
    u8* mem = nullptr;
    if (dmalloc(&mem, slots * 28) != hipSuccess) { (void)hipGetLastError(); return fail(h, MLST_E_LIMIT, "mlst_set_read_dedup: the table of %llu slots needs %llu bytes of device memory", (unsigned long long)slots, (unsigned long long)(slots * 28)); }
    const DdTab T = {reinterpret_cast<u64*>(mem), reinterpret_cast<u64*>(mem + slots * 8), reinterpret_cast<u64*>(mem + slots * 16), reinterpret_cast<u32*>(mem + slots * 24), slots, tag_mask};
    int rc = dd_clear(h, T);
    if (!rc && D.d_mem) {
        hipLaunchKernelGGL(k_dd_rehash, dim3(grid_for(D.tab.slots, 256)), dim3(256), 0, h->stream, D.tab, T, D.d_ctr);
        const hipError_t e = hipStreamSynchronize(h->stream);      // (the old table is freed behind its last reader)
        if (e != hipSuccess) rc = fail(h, MLST_E_HIP, "k_dd_rehash: %s", hipGetErrorString(e));
    }
    if (rc) { hipFree(mem); return rc; }
    hipFree(D.d_mem); D.d_mem = mem; D.tab = T;
    return MLST_OK;
}
// the three launches of mlst_set_read_dedup over a chunk's reads as their lengths stand now.  Chunks are queued on h->stream one behind
// the other (each ends in a read-back), so the launches of consecutive chunks run in read-index order -- for the pipelined BGZF
// entries too, whose other two streams only copy and inflate
static int dd_apply(mlst_handle* h, u64 n_reads, u32* d_flags, int paired) {
    auto& D = h->dd;
    const u64 n_units = paired ? n_reads / 2 : n_reads;
    if (paired && (n_reads & 1)) return fail(h, MLST_E_INVALID, "mlst_set_read_dedup: a paired chunk holds %llu records: the mates of a pair are compared within one chunk", (unsigned long long)n_reads);
    if (!n_units) return MLST_OK;
    int rc = dd_ensure(h, n_units); if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
    {
        Prof pf(h, 21);      // (mlst_get_kernel_time 21: k_dd_insert, k_dd_sign and k_dd_mark together)
        const dim3 grid(grid_for(n_units, 256)), block(256);
        hipLaunchKernelGGL(k_dd_insert, grid, block, 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, (const u16*)h->d_lens, n_units, paired ? 1u : 0u,
                           D.units_seen, D.tab, D.d_slot_of, D.d_key2, (const u32*)d_flags, D.d_ctr);
        hipLaunchKernelGGL(k_dd_sign, grid, block, 0, h->stream, n_units, D.units_seen, D.tab, (const u32*)D.d_slot_of, (const u64*)D.d_key2, (const u32*)d_flags, D.d_ctr);
        hipLaunchKernelGGL(k_dd_mark, grid, block, 0, h->stream, h->d_lens, n_units, paired ? 1u : 0u, D.units_seen, D.tab, (const u32*)D.d_slot_of, (const u64*)D.d_key2,
                           d_flags, D.d_ctr);
    }
    HIPCHK(h, hipGetLastError());
    D.units_seen += n_units; D.reads += n_reads;
    return MLST_OK;
}
// mlst_set_read_pair_overlap's launch over a chunk's pairs as their lengths stand now.  At most three workgroups of eight waves per CU
// (what its registers let a CU hold; each flushes its histogram in LDS once), fewer for few pairs
static int po_apply(mlst_handle* h, u64 n_reads, u32* d_flags, int paired) {
    auto& O = h->po;
    if (!paired) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: an unpaired FASTQ submission: mate overlap trimming is on and takes pairs (the paired entries; `-2` with mates that share their names)");
    if (n_reads & 1) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: a paired chunk holds %llu records: the mates of a pair are laid on each other within one chunk", (unsigned long long)n_reads);
    const u64 n_pairs = n_reads / 2;
    if (!n_pairs) return MLST_OK;
    { int rc = chain_ctr(h, &O.d_ctr); if (rc) return rc; }
    if (!O.n_cu) { HIPCHK(h, hipDeviceGetAttribute(&O.n_cu, hipDeviceAttributeMultiprocessorCount, h->device)); if (O.n_cu < 1) O.n_cu = 1; }
    PoSet S = O.set;
    S.trim5 = h->rp.on ? h->rp.set.trim5 : 0u;
    HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
    {
        Prof pf(h, 22);      // (mlst_get_kernel_time 22: k_po_cut alone)
        const u32 grid = (u32)std::min<u64>((n_pairs + PO_WAVES - 1) / PO_WAVES, 3ull * (u64)O.n_cu);
        hipLaunchKernelGGL(k_po_cut, dim3(grid), dim3(64 * PO_WAVES), 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, h->d_lens, n_pairs, S, d_flags, O.d_ctr);
    }
    HIPCHK(h, hipGetLastError());
    O.pairs += n_pairs;
    return MLST_OK;
}
// The parser has left offsets and lengths of n_reads reads of h->d_fq_text and the longest length in flags[0].  The chain, in its one
// order, queued in front of the read-back of the flags (no synchronisation added): raw statistics, quality trim, quality windows, adapter cut, mate
// overlap, tail trim and read filter, prepared statistics, duplicate removal.  flags[0] is zeroed in front of every kernel that shortens reads, so the last one
// alone feeds the longest length the host reads (an atomicMax with the shorter lengths would leave the longer one standing).
// The prepared tables are counted only behind a stage that shortens: with none, launches[1] stays 0 and mlst_read_stats_fetch hands out
// the raw tables for them.  Never with a tile (chain_refuse)
static int chain_apply(mlst_handle* h, u64 n_reads, u32* d_flags, int paired) {
    const RpSet& P = h->rp.set;
    const bool trims = h->rp.on && (P.trim5 | P.trim3 | P.trim_qual);      // (the Phred base alone is k_pack_text's)
    int rc = MLST_OK;
    if (h->rs.on) { rc = rs_launch(h, n_reads, d_flags, paired, 0); if (rc) return rc; }
    if (trims) {
        rc = chain_ctr(h, &h->rp.d_ctr); if (rc) return rc;
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
        Prof pf(h, 18);      // (mlst_get_kernel_time 18: k_rp_qtrim alone)
        hipLaunchKernelGGL(k_rp_qtrim, dim3(grid_for(n_reads, 256)), dim3(256), 0, h->stream, (const u8*)h->d_fq_text, h->d_fq_soff, h->d_fq_qoff, h->d_lens, n_reads, P,
                           d_flags, h->rp.d_ctr);
    }
    if (h->rw.on) {      // (quality before adapters: cutadapt's and fastp's order; the first stage behind k_rp_qtrim that moves a read's start)
        rc = chain_ctr(h, &h->rw.d_ctr); if (rc) return rc;
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
        Prof pf(h, 24);      // (mlst_get_kernel_time 24: k_rw_cut alone)
        hipLaunchKernelGGL(k_rw_cut, dim3(grid_for(n_reads, 256)), dim3(256), 0, h->stream, (const u8*)h->d_fq_text, h->d_fq_soff, h->d_fq_qoff, h->d_lens, n_reads, h->rw.set,
                           P.phred_base, d_flags, h->rw.d_ctr);
    }
    if (h->ra.on) {
        rc = chain_ctr(h, &h->ra.d_ctr); if (rc) return rc;
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
        Prof pf(h, 19);      // (mlst_get_kernel_time 19: k_ra_cut alone)
        hipLaunchKernelGGL(k_ra_cut, dim3(grid_for(n_reads, 256)), dim3(256), 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, h->d_lens, n_reads, h->ra.set,
                           d_flags, h->ra.d_ctr);
    }
    if (h->po.on) { rc = po_apply(h, n_reads, d_flags, paired); if (rc) return rc; }      // (zeroes flags[0] itself; refuses unpaired and odd chunks)
    if (h->rf.on) {      // (behind the mates' overlap: the filter judges the read as it is aligned)
        rc = chain_ctr(h, &h->rf.d_ctr); if (rc) return rc;
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 4, h->stream));
        Prof pf(h, 23);      // (mlst_get_kernel_time 23: k_rf_filter alone)
        hipLaunchKernelGGL(k_rf_filter, dim3(grid_for(n_reads, 256)), dim3(256), 0, h->stream, (const u8*)h->d_fq_text, (const u64*)h->d_fq_soff, (const u64*)h->d_fq_qoff, h->d_lens,
                           n_reads, h->rf.set, P.phred_base, d_flags, h->rf.d_ctr);
    }
    if (h->rs.on && (trims || h->rw.on || h->ra.on || h->po.on || h->rf.on)) { rc = rs_launch(h, n_reads, d_flags, paired, 1); if (rc) return rc; }
    if (h->dd.on) { rc = dd_apply(h, n_reads, d_flags, paired); if (rc) return rc; }      // (zeroes flags[0] itself; the prepared tables stay what they are)
    return MLST_OK;
}

// ---- the switches and their readers (include/mlst.h)
// the retained reads' names (csrc/read_names.h)
extern "C" int mlst_set_read_names(mlst_handle* h, int on) {
    if (!h) return MLST_E_INVALID;
    { int rc_ = chain_gate(h, "mlst_set_read_names", (on != 0) != h->rn.on, on != 0, "mlst_set_read_tiling is on: a window has no name"); if (rc_) return rc_; }
    h->rn.on = on != 0;
    return MLST_OK;
}
extern "C" int mlst_get_read_names(mlst_handle* h, int* on) {
    if (!h || !on) return fail(h, MLST_E_INVALID, "NULL argument");
    *on = h->rn.on ? 1 : 0;
    return MLST_OK;
}
extern "C" int mlst_read_names_info(mlst_handle* h, uint64_t out[4]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }      // (a BGZF piece in flight is part of the sample)
    RnCtr c; { int rc_ = rn_fetch(h, &c); if (rc_) return rc_; }
    out[0] = c.done - c.fallbacks; out[1] = c.bytes; out[2] = c.fallbacks; out[3] = c.longest;
    return MLST_OK;
}
extern "C" int mlst_read_names_fetch(mlst_handle* h, uint64_t* read_index, uint64_t* off, uint8_t* bytes) {
    if (!h || !read_index || !off || !bytes) return fail(h, MLST_E_INVALID, "NULL argument");
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }
    RnCtr c; { int rc_ = rn_fetch(h, &c); if (rc_) return rc_; }
    off[0] = 0;
    if (!c.done) return MLST_OK;
    std::vector<u64> ridx(c.done), noff(c.done); std::vector<u16> nlen(c.done); std::vector<u8> arena(c.bytes ? c.bytes : 1);
    HIPCHK(h, hipMemcpyAsync(ridx.data(), h->E.ret_ridx, c.done * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(noff.data(), h->rn.d_off, c.done * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(nlen.data(), h->rn.d_len, c.done * 2, hipMemcpyDeviceToHost, h->stream));
    if (c.bytes) HIPCHK(h, hipMemcpyAsync(arena.data(), h->rn.d_bytes, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u64 n = 0, at = 0;
    for (u64 s = 0; s < c.done; s++) {      // the slots with a name, in slot order
        if (!nlen[s]) continue;
        if (noff[s] + nlen[s] > c.bytes) return fail(h, MLST_E_HIP, "name arena inconsistent at slot %llu", (unsigned long long)s);
        read_index[n] = ridx[s]; memcpy(bytes + at, arena.data() + noff[s], nlen[s]); at += nlen[s]; off[++n] = at;
    }
    return MLST_OK;
}
// reads prepared before they are packed (csrc/read_prep.h)
extern "C" int mlst_set_read_prep(mlst_handle* h, const mlst_read_prep* p) {
    if (!h) return MLST_E_INVALID;
    const RpSet want = p ? RpSet{p->trim5, p->trim3, p->trim_qual, p->phred_base} : RpSet{0, 0, 0, 33};
    if (want.phred_base != 33 && want.phred_base != 64) return fail(h, MLST_E_INVALID, "mlst_set_read_prep: phred_base is %u, not 33 or 64", want.phred_base);
    if (want.trim_qual > 93) return fail(h, MLST_E_INVALID, "mlst_set_read_prep: trim_qual %u exceeds 93", want.trim_qual);
    if (want.trim5 > 65535 || want.trim3 > 65535) return fail(h, MLST_E_INVALID, "mlst_set_read_prep: a trim exceeds 65535 bases");
    const RpSet& cur = h->rp.set;
    const bool same = want.trim5 == cur.trim5 && want.trim3 == cur.trim3 && want.trim_qual == cur.trim_qual && want.phred_base == cur.phred_base;
    const bool on = (want.trim5 | want.trim3 | want.trim_qual) != 0 || want.phred_base != 33;
    { int rc_ = chain_gate(h, "mlst_set_read_prep", !same, on, "mlst_set_read_prep: mlst_set_read_tiling is on and a window is cut from the record as it stands"); if (rc_) return rc_; }
    h->rp.set = want; h->rp.on = on;
    return MLST_OK;
}
extern "C" int mlst_get_read_prep(mlst_handle* h, mlst_read_prep* out) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    out->trim5 = h->rp.set.trim5; out->trim3 = h->rp.set.trim3; out->trim_qual = h->rp.set.trim_qual; out->phred_base = h->rp.set.phred_base;
    return MLST_OK;
}
extern "C" int mlst_read_prep_info(mlst_handle* h, uint64_t out[4]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    RpCtr c; { int rc_ = chain_fetch(h, h->rp.on, &h->rp.d_ctr, &c); if (rc_) return rc_; }
    out[0] = c.shortened; out[1] = c.removed; out[2] = c.emptied; out[3] = 0;
    return MLST_OK;
}
// 3' adapters removed before the reads are packed (csrc/read_adapt.h)
extern "C" int mlst_set_read_adapters(mlst_handle* h, const char* adapters, uint32_t min_overlap, uint32_t error_permille) {
    if (!h) return MLST_E_INVALID;
    RaSet want = {}; std::string text;
    if (adapters && *adapters) {
        if (min_overlap < 1 || min_overlap > RA_MAX_LEN) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: min_overlap %u is outside 1..%d", min_overlap, RA_MAX_LEN);
        if (error_permille > 500) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: error_permille %u exceeds 500", error_permille);
        want.permille = error_permille; want.min_overlap = min_overlap;
        for (const char* c = adapters;; c++) {      // letter by letter; ',' or the end closes an adapter
            if (want.K >= RA_MAX_ADAPTERS) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: more than %d adapters", RA_MAX_ADAPTERS);
            RaAd& A = want.ad[want.K];
            if (*c == ',' || !*c) {
                if (!A.m) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: adapter %u is empty", want.K + 1);
                if (!(A.care[0] | A.care[1])) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: adapter %u holds only N", want.K + 1);
                A.mo = min_overlap < A.m ? min_overlap : A.m;
                want.K++;
                if (!*c) break;
                text.push_back(',');
                continue;
            }
            const char up = (char)(*c & 0xDF);
            const char* at = (up && !(*c & 0x80)) ? strchr("ACGTN", up) : nullptr;
            if (!at) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: adapter %u holds a letter outside ACGTN (byte 0x%02x)", want.K + 1, (unsigned)(unsigned char)*c);
            if (A.m >= RA_MAX_LEN) return fail(h, MLST_E_INVALID, "mlst_set_read_adapters: adapter %u is longer than %d letters", want.K + 1, RA_MAX_LEN);
            const u32 w = A.m >> 5, sh = 2 * (A.m & 31);
            if (up == 'N') A.anyn[w] |= 1ull << sh;
            else { A.code[w] |= (u64)(at - "ACGTN") << sh; A.care[w] |= 1ull << sh; }
            A.m++;
            text.push_back(up);
        }
    }
    const bool same = text == h->ra.text && want.permille == h->ra.set.permille && want.min_overlap == h->ra.set.min_overlap;
    { int rc_ = chain_gate(h, "mlst_set_read_adapters", !same, want.K != 0, "mlst_set_read_adapters: mlst_set_read_tiling is on and a window is cut from the record as it stands"); if (rc_) return rc_; }
    h->ra.set = want; h->ra.text = text; h->ra.on = want.K != 0;
    return MLST_OK;
}
extern "C" int mlst_get_read_adapters(mlst_handle* h, char* adapters, uint64_t cap, uint32_t* min_overlap, uint32_t* error_permille) {
    if (!h) return MLST_E_INVALID;
    if (adapters) {
        if (cap < h->ra.text.size() + 1) return fail(h, MLST_E_INVALID, "mlst_get_read_adapters: the buffer holds %llu bytes, %llu are needed", (unsigned long long)cap, (unsigned long long)(h->ra.text.size() + 1));
        memcpy(adapters, h->ra.text.c_str(), h->ra.text.size() + 1);
    }
    if (min_overlap) *min_overlap = h->ra.set.min_overlap;
    if (error_permille) *error_permille = h->ra.set.permille;
    return MLST_OK;
}
extern "C" int mlst_get_read_adapters_info(mlst_handle* h, uint64_t out[12]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    RaCtr c; { int rc_ = chain_fetch(h, h->ra.on, &h->ra.d_ctr, &c); if (rc_) return rc_; }
    out[0] = c.trimmed; out[1] = c.removed; out[2] = c.emptied; out[3] = h->ra.set.K;
    for (int k = 0; k < RA_MAX_ADAPTERS; k++) out[4 + k] = c.per_adapter[k];
    return MLST_OK;
}
// per-cycle read statistics (csrc/read_stats.h)
extern "C" int mlst_set_read_stats(mlst_handle* h, int on) {
    if (!h) return MLST_E_INVALID;
    { int rc_ = chain_gate(h, "mlst_set_read_stats", (on != 0) != h->rs.on, on != 0, "mlst_set_read_stats: mlst_set_read_tiling is on and the windows of a read would be counted, not the read"); if (rc_) return rc_; }
    h->rs.on = on != 0;
    return MLST_OK;
}
extern "C" int mlst_get_read_stats(mlst_handle* h, int* on) {
    if (!h || !on) return fail(h, MLST_E_INVALID, "NULL argument");
    *on = h->rs.on ? 1 : 0;
    return MLST_OK;
}
extern "C" int mlst_set_read_stats_side(mlst_handle* h, int side) {
    if (!h) return MLST_E_INVALID;
    if (side != 0 && side != 1) return fail(h, MLST_E_INVALID, "mlst_set_read_stats_side: side is %d, not 0 or 1", side);
    { int rc_ = chain_gate(h, nullptr, false, false, nullptr); if (rc_) return rc_; }
    h->rs.side = (u32)side;
    return MLST_OK;
}
// (the tables are an array, not a counter struct, and one of four is copied: chain_fetch does not fit)
extern "C" int mlst_read_stats_fetch(mlst_handle* h, int stage, int side, uint64_t* out, uint64_t cap) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    if ((stage != 0 && stage != 1) || (side != 0 && side != 1)) return fail(h, MLST_E_INVALID, "mlst_read_stats_fetch: stage %d, side %d: each is 0 or 1", stage, side);
    if (cap < RS_WORDS) return fail(h, MLST_E_INVALID, "mlst_read_stats_fetch: the buffer holds %llu words, %d are needed", (unsigned long long)cap, RS_WORDS);
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }      // (a BGZF piece in flight is part of the sample)
    memset(out, 0, (size_t)RS_WORDS * 8);
    if (!h->rs.on || !h->rs.d_tab) return MLST_OK;
    if (stage == 1 && !h->rs.launches[1]) stage = 0;      // no stage shortened a read (chain_apply): the prepared read is the raw one
    HIPCHK(h, hipMemcpyAsync(out, h->rs.d_tab + ((u64)stage * 2 + (u64)side) * RS_WORDS, (size_t)RS_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLST_OK;
}
extern "C" int mlst_read_stats_info(mlst_handle* h, uint64_t out[4]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }
    const bool live = h->rs.on && h->rs.d_tab;
    out[0] = live ? h->rs.launches[0] : 0; out[1] = live ? h->rs.launches[1] : 0; out[2] = h->rs.d_tab ? 4ull * RS_WORDS * 8 : 0; out[3] = 0;
    return MLST_OK;
}
// exact duplicates emptied before the reads are packed (csrc/read_dedup.h)
extern "C" int mlst_set_read_dedup(mlst_handle* h, int on) {
    if (!h) return MLST_E_INVALID;
    { int rc_ = chain_gate(h, "mlst_set_read_dedup", (on != 0) != h->dd.on, on != 0, "mlst_set_read_dedup: mlst_set_read_tiling is on and the windows of a read would be compared, not the read"); if (rc_) return rc_; }
    h->dd.on = on != 0;
    return MLST_OK;
}
extern "C" int mlst_get_read_dedup(mlst_handle* h, int* on) {
    if (!h || !on) return fail(h, MLST_E_INVALID, "NULL argument");
    *on = h->dd.on ? 1 : 0;
    return MLST_OK;
}
// (k_dd_levels runs between the flush and the copy: chain_fetch does not fit)
extern "C" int mlst_read_dedup_info(mlst_handle* h, uint64_t out[16]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    hipSetDevice(h->device);
    { int rc_ = bz_flush(h); if (rc_) return rc_; }      // (a BGZF piece in flight is part of the sample)
    for (int k = 0; k < 16; k++) out[k] = 0;
    if (!h->dd.on || !h->dd.d_ctr || !h->dd.d_mem) return MLST_OK;
    DdCtr c; memset(&c, 0, sizeof c);
    HIPCHK(h, hipMemsetAsync(h->dd.d_ctr->levels, 0, sizeof c.levels, h->stream));      // (counted anew by every call)
    hipLaunchKernelGGL(k_dd_levels, dim3(grid_for(h->dd.tab.slots, 256, 4096)), dim3(256), 0, h->stream, h->dd.tab, h->dd.d_ctr);
    HIPCHK(h, hipMemcpyAsync(&c, h->dd.d_ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (c.err) return fail(h, MLST_E_HIP, "mlst_set_read_dedup: a probe ran through the whole table");
    out[0] = h->dd.reads; out[1] = c.units; out[2] = c.dups; out[3] = c.reads_removed; out[4] = c.bases_removed; out[5] = c.distinct; out[6] = c.clashes;
    out[7] = h->dd.tab.slots;
    for (int k = 0; k < 8; k++) out[8 + k] = c.levels[k];
    return MLST_OK;
}
// the one combination of two stages that is refused, in both orders (mlst_set_read_pair_overlap, mlst_set_read_window)
#define RW_PO_TEXT "a front cut (mlst_set_read_window, front_w != 0) and mate overlap trimming (mlst_set_read_pair_overlap) do not combine: the overlap places " \
                   "the insert's end by trim5 alone (I = o + n2 + trim5: both mates lost the same number of 5' bases), and a front cut per read would make it cut true insert bases"
// adapter read-through cut from the overlap of the mates (csrc/read_overlap.h)
extern "C" int mlst_set_read_pair_overlap(mlst_handle* h, int on, uint32_t min_overlap, uint32_t max_mismatches, uint32_t error_permille) {
    if (!h) return MLST_E_INVALID;
    if (on) {
        if (min_overlap < 8 || min_overlap > PO_MAX_LEN) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: min_overlap %u is outside 8..%d", min_overlap, PO_MAX_LEN);
        if (max_mismatches > 64) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: max_mismatches %u is outside 0..64", max_mismatches);
        if (error_permille > 500) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: error_permille %u is outside 0..500", error_permille);
        if (h->rw.set.front_w) return fail(h, MLST_E_INVALID, "mlst_set_read_pair_overlap: %s", RW_PO_TEXT);
    }
    const bool same = (on != 0) == h->po.on && (!on || (min_overlap == h->po.set.min_overlap && max_mismatches == h->po.set.max_mism && error_permille == h->po.set.permille));
    { int rc_ = chain_gate(h, "mlst_set_read_pair_overlap", !same, on != 0, "mlst_set_read_pair_overlap: mlst_set_read_tiling is on and takes unpaired text, whose windows have no mate"); if (rc_) return rc_; }
    h->po.on = on != 0;
    if (on) { h->po.set.min_overlap = min_overlap; h->po.set.max_mism = max_mismatches; h->po.set.permille = error_permille; }
    return MLST_OK;
}
extern "C" int mlst_get_read_pair_overlap(mlst_handle* h, int* on, uint32_t* min_overlap, uint32_t* max_mismatches, uint32_t* error_permille) {
    if (!h || !on) return fail(h, MLST_E_INVALID, "NULL argument");
    *on = h->po.on ? 1 : 0;
    if (min_overlap) *min_overlap = h->po.set.min_overlap;
    if (max_mismatches) *max_mismatches = h->po.set.max_mism;
    if (error_permille) *error_permille = h->po.set.permille;
    return MLST_OK;
}
// (PoCtr holds the 8 KB histogram: kept off the caller's stack)
extern "C" int mlst_read_pair_overlap_info(mlst_handle* h, uint64_t out[8]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    PoCtr* const pc = new PoCtr;
    int rc = chain_fetch(h, h->po.on, &h->po.d_ctr, pc);
    if (!rc) { out[0] = h->po.on ? h->po.pairs : 0; out[1] = pc->overlapping; out[2] = pc->trimmed_pairs; out[3] = pc->reads_trimmed; out[4] = pc->bases_removed; out[5] = pc->emptied; out[6] = 0; out[7] = 0; }
    delete pc;
    return rc;
}
extern "C" int mlst_read_pair_overlap_hist(mlst_handle* h, uint64_t* out, uint64_t cap) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    if (cap < PO_HIST) return fail(h, MLST_E_INVALID, "mlst_read_pair_overlap_hist: the buffer holds %llu words, %d are needed", (unsigned long long)cap, PO_HIST);
    PoCtr* const pc = new PoCtr;
    int rc = chain_fetch(h, h->po.on, &h->po.d_ctr, pc);
    if (!rc) memcpy(out, pc->hist, sizeof pc->hist);
    delete pc;
    return rc;
}
// poly-G / poly-X tails trimmed and reads filtered before the reads are packed (csrc/read_filter.h)
extern "C" int mlst_set_read_filter(mlst_handle* h, const mlst_read_filter* f) {
    if (!h) return MLST_E_INVALID;
    RfSet want = {0, 10, 0, RF_NO_LIMIT, 0, 0};      // (off)
    if (f) {
        if (f->poly_mask > 15) return fail(h, MLST_E_INVALID, "mlst_set_read_filter: poly_mask %u is outside 0..15 (bits 0..3: A, C, G, T)", f->poly_mask);
        if (f->poly_mask && (f->poly_min < 1 || f->poly_min > RF_MAX_LEN)) return fail(h, MLST_E_INVALID, "mlst_set_read_filter: poly_min %u is outside 1..%d", f->poly_min, RF_MAX_LEN);
        if (f->min_length > RF_MAX_LEN) return fail(h, MLST_E_INVALID, "mlst_set_read_filter: min_length %u is outside 0..%d", f->min_length, RF_MAX_LEN);
        if (f->complexity_pct > 100) return fail(h, MLST_E_INVALID, "mlst_set_read_filter: complexity_pct %u is outside 0..100", f->complexity_pct);
        if (f->mean_qual > 93) return fail(h, MLST_E_INVALID, "mlst_set_read_filter: mean_qual %u is outside 0..93", f->mean_qual);
        want = RfSet{f->poly_mask, f->poly_mask ? f->poly_min : 10u, f->min_length, f->max_n, f->complexity_pct, f->mean_qual};
    }
    const RfSet& cur = h->rf.set;
    const bool same = want.poly_mask == cur.poly_mask && want.poly_min == cur.poly_min && want.min_length == cur.min_length && want.max_n == cur.max_n &&
                      want.complexity_pct == cur.complexity_pct && want.mean_qual == cur.mean_qual;
    const bool on = want.poly_mask != 0 || want.min_length != 0 || want.max_n != RF_NO_LIMIT || want.complexity_pct != 0 || want.mean_qual != 0;
    { int rc_ = chain_gate(h, "mlst_set_read_filter", !same, on, "mlst_set_read_filter: mlst_set_read_tiling is on and a window is cut from the record as it stands"); if (rc_) return rc_; }
    h->rf.set = want; h->rf.on = on;
    return MLST_OK;
}
extern "C" int mlst_get_read_filter(mlst_handle* h, mlst_read_filter* out) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    const RfSet& S = h->rf.set;
    out->poly_mask = S.poly_mask; out->poly_min = S.poly_min; out->min_length = S.min_length; out->max_n = S.max_n; out->complexity_pct = S.complexity_pct; out->mean_qual = S.mean_qual;
    return MLST_OK;
}
extern "C" int mlst_read_filter_info(mlst_handle* h, uint64_t out[16]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    RfCtr c; { int rc_ = chain_fetch(h, h->rf.on, &h->rf.d_ctr, &c); if (rc_) return rc_; }
    out[0] = c.tail_trimmed; out[1] = c.tail_bases;
    for (int k = 0; k < 4; k++) { out[2 + k] = c.per_letter[k]; out[7 + k] = c.failed[k]; }
    out[6] = c.tail_emptied; out[11] = c.filtered_bases;
    for (int k = 12; k < 16; k++) out[k] = 0;
    return MLST_OK;
}
// sliding-window quality cuts before the reads are packed (csrc/read_window.h)
extern "C" int mlst_set_read_window(mlst_handle* h, const mlst_read_window* w) {
    if (!h) return MLST_E_INVALID;
    RwSet want = {0, 0, 0, 0, 0, 0};      // (off)
    if (w) {
        const struct { const char* name; u32 w, q; } ops[] = {{"front", w->front_w, w->front_q}, {"right", w->right_w, w->right_q}, {"tail", w->tail_w, w->tail_q}};
        for (const auto& o : ops) {
            if (o.w > RW_MAX_W) return fail(h, MLST_E_INVALID, "mlst_set_read_window: %s_w %u is outside 0..%d", o.name, o.w, RW_MAX_W);
            if (o.w && (o.q < 1 || o.q > 93)) return fail(h, MLST_E_INVALID, "mlst_set_read_window: %s_q %u is outside 1..93", o.name, o.q);
        }
        want = RwSet{w->front_w, w->front_w ? w->front_q : 0u, w->right_w, w->right_w ? w->right_q : 0u, w->tail_w, w->tail_w ? w->tail_q : 0u};
    }
    if (want.front_w && h->po.on) return fail(h, MLST_E_INVALID, "mlst_set_read_window: %s", RW_PO_TEXT);
    const RwSet& cur = h->rw.set;
    const bool same = want.front_w == cur.front_w && want.front_q == cur.front_q && want.right_w == cur.right_w && want.right_q == cur.right_q &&
                      want.tail_w == cur.tail_w && want.tail_q == cur.tail_q;
    const bool on = (want.front_w | want.right_w | want.tail_w) != 0;
    { int rc_ = chain_gate(h, "mlst_set_read_window", !same, on, "mlst_set_read_window: mlst_set_read_tiling is on and a window is cut from the record as it stands"); if (rc_) return rc_; }
    h->rw.set = want; h->rw.on = on;
    return MLST_OK;
}
extern "C" int mlst_get_read_window(mlst_handle* h, mlst_read_window* out) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    const RwSet& S = h->rw.set;
    out->front_w = S.front_w; out->front_q = S.front_q; out->right_w = S.right_w; out->right_q = S.right_q; out->tail_w = S.tail_w; out->tail_q = S.tail_q;
    return MLST_OK;
}
extern "C" int mlst_read_window_info(mlst_handle* h, uint64_t out[8]) {
    if (!h || !out) return fail(h, MLST_E_INVALID, "NULL argument");
    RwCtr c; { int rc_ = chain_fetch(h, h->rw.on, &h->rw.d_ctr, &c); if (rc_) return rc_; }
    out[0] = c.shortened; out[1] = c.front_reads; out[2] = c.front_bases; out[3] = c.right_reads; out[4] = c.right_bases; out[5] = c.tail_reads; out[6] = c.tail_bases;
    out[7] = c.emptied;
    return MLST_OK;
}
