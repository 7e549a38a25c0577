// export.hip -- tc_export_live / tc_import_live: live limiter state out of an engine as an arena, and merged into another one
#include "engine.hpp"
#include "export_kernels.hpp"

// Neither call touches the host-side state of the batch path: no batch count, no operation of the cleanup policy, no sweep in
// front or behind, no grouping hint.  What they move is what any key work on the engine's stream moves: the hand-over of the
// key table between the two streams (k_done / m_done) and the end of the "sweep beside the newest evaluation" chain.

template <bool KEYS>
static void export_launch(tc_engine* e, hipStream_t s, const xp::Page& p, const xp::Work& w, const xp::Out& o) {
    const dim3 grid(w.tiles), block(xp::THREADS);
    hipLaunchKernelGGL((xp::k_count<KEYS>), grid, block, 0, s, p, e->kt, w);
    hipLaunchKernelGGL((xp::k_scan<KEYS>), dim3(1), block, 0, s, w, o);
    auto last = xp::k_scatter<KEYS>;
    // key mode: the scatter's completion is m_done, which the key stage, sweep or rebuild of any later call waits for before it
    // may write what these kernels read (peek.hip: peek_launch)
    TC_LAUNCH(KEYS ? e->m_done : (hipEvent_t) nullptr, last, grid, block, 0, s, p, e->kt, w, o);
}

extern "C" int tc_export_live(tc_engine* e, const void* xp_) {
    if (!e || !xp_) return TC_E_INVALID_ARG;
    tc_export x;
    memcpy(&x, xp_, sizeof(uint32_t)); // (struct_size first: nothing beyond it is read from a shorter struct)
    if (x.struct_size < sizeof(tc_export)) return TC_E_INVALID_ARG;
    memcpy(&x, xp_, sizeof x);
    TC_CHECK_POISON(e);
    auto bad = [&](const char* what) { return fail(e, TC_E_INVALID_ARG, (std::string("tc_export_live: ") + what).c_str()); };
    if (e->fixed) return fail(e, TC_E_UNSUPPORTED, "tc_export_live: TC_CFG_FIXED_PARAMS engines keep no expiry column to export");
    if (x.flags != 0) return bad("flags must be 0");
    if (x.n_slots == 0 || x.first_slot >= e->capacity || x.n_slots > e->capacity - x.first_slot) return bad("the page is not inside the capacity");
    if (x.world > krt::MAX_WORLD) return bad("world must be 0..64");
    if (x.world >= 2 && !e->key_mode) return bad("world >= 2 filters by key owner: key-mode engines only");
    if (x.world >= 2 && (x.only < 0 || x.only >= (int32_t)x.world)) return bad("`only` is not a destination");
    if (!x.out_tat || !x.out_expiry || !x.out_count) return bad("out_tat / out_expiry / out_count is NULL");
    if (e->key_mode ? (!x.out_key_bytes || !x.out_key_off) : !x.out_slot) return bad(e->key_mode ? "out_key_bytes / out_key_off is NULL" : "out_slot is NULL");
    TC_HIP(e, hipSetDevice(e->device));
    hipStream_t own = cur_stream(e), s = x.stream ? (hipStream_t)x.stream : own;

    xp::Page p;
    p.cells = e->cells;
    p.first = x.first_slot, p.end = x.first_slot + x.n_slots;
    p.tile0 = x.first_slot / xp::TILE;
    p.now = x.now_ns;
    p.mod = krt::make_mod(x.world >= 2 ? x.world : 1u);
    p.only = x.world >= 2 ? (uint32_t)x.only : 0u;
    xp::Work w;
    w.tiles = (uint32_t)((p.end - 1) / xp::TILE - p.tile0 + 1);
    // scratch: [ bytes per tile: u64 [tiles] | entries per tile: u32 [tiles] | "it fits": u32 ].  Nothing to clear: k_count and
    // k_scan write every word before it is read.  One scratch: exports are ordered one behind the other (below).
    const size_t need = (size_t)w.tiles * 12 + 4;
    if (need > e->export_ws_bytes) {
        if (e->export_ws) {
            TC_HIP(e, hipDeviceSynchronize()); // (whatever stream the last export ran on)
            (void)hipFree(e->export_ws);
            e->export_ws = nullptr, e->export_ws_bytes = 0;
        }
        TC_HIP(e, hipMalloc(&e->export_ws, 2 * need));
        e->export_ws_bytes = 2 * need;
    }
    w.tile_bytes = reinterpret_cast<unsigned long long*>(e->export_ws);
    w.tile_entries = reinterpret_cast<uint32_t*>(e->export_ws + (size_t)w.tiles * 8);
    w.fits = w.tile_entries + w.tiles;
    xp::Out o;
    o.slot = x.out_slot, o.key_bytes = x.out_key_bytes, o.key_off = x.out_key_off, o.tat = x.out_tat, o.expiry = x.out_expiry;
    o.count = reinterpret_cast<unsigned long long*>(x.out_count);
    o.count_host = reinterpret_cast<volatile unsigned long long*>(x.out_count_host);
    o.tag = x.tag;
    o.cap_entries = x.cap_entries, o.cap_bytes = x.cap_bytes;

    // A stream of the caller's: the export goes behind everything the engine's stream holds (the evaluations that wrote the
    // cells), and the engine's stream goes on behind the export (the next evaluation must not write what it reads).
    if (s != own) {
        if (!e->export_fence) TC_HIP(e, hipEventCreateWithFlags(&e->export_fence, hipEventDisableTiming));
        TC_HIP(e, hipEventRecord(e->export_fence, own));
        TC_HIP(e, hipStreamWaitEvent(s, e->export_fence, 0));
    }
    if (e->key_mode) { // key work on the engine's stream: behind the key stream's last stage
        if (e->k_busy) TC_HIP(e, hipStreamWaitEvent(s, e->k_done, 0));
        aside_reset(e);
        export_launch<true>(e, s, p, w, o);
        e->m_busy = true;
        e->k_busy = false;
    } else {
        export_launch<false>(e, s, p, w, o);
    }
    TC_HIP(e, hipGetLastError());
    if (s != own) {
        TC_HIP(e, hipEventRecord(e->export_fence, s));
        TC_HIP(e, hipStreamWaitEvent(own, e->export_fence, 0));
    }
    return TC_E_OK;
}

extern "C" int tc_import_live(tc_engine* e, const void* mp) {
    if (!e || !mp) return TC_E_INVALID_ARG;
    tc_import m;
    memcpy(&m, mp, sizeof(uint32_t));
    if (m.struct_size < sizeof(tc_import)) return TC_E_INVALID_ARG;
    memcpy(&m, mp, sizeof m);
    TC_CHECK_POISON(e);
    auto bad = [&](const char* what) { return fail(e, TC_E_INVALID_ARG, (std::string("tc_import_live: ") + what).c_str()); };
    if (e->fixed) return fail(e, TC_E_UNSUPPORTED, "tc_import_live: TC_CFG_FIXED_PARAMS engines keep no expiry column to merge into");
    if (m.flags != 0) return bad("flags must be 0");
    if (m.n == 0 || m.n > e->max_batch) return bad("n must be 1 .. max_batch");
    if (!m.tat || !m.expiry || !m.out_count) return bad("tat / expiry / out_count is NULL");
    if (e->key_mode ? (!m.key_bytes || !m.key_off) : !m.slot) return bad(e->key_mode ? "key_bytes / key_off is NULL" : "slot is NULL");
    TC_HIP(e, hipSetDevice(e->device));
    hipStream_t s = cur_stream(e);
    xp::Merge g;
    g.cells = e->cells, g.capacity = e->capacity;
    g.slot = m.slot, g.tat = m.tat, g.expiry = m.expiry;
    g.n = (uint32_t)m.n;
    g.out_count = reinterpret_cast<unsigned long long*>(m.out_count);
    if (e->key_mode) { // the insert stage as a key batch runs it: k_probe, k_bind, k_follow; duplicates share a slot
        TC_TRY(resolve_keys_device(e, m.key_bytes, m.key_off, g.n, true, e->k_slot, false));
        g.slot = e->k_slot;
    }
    const dim3 grid(nblocks(m.n)), block(xp::THREADS);
    static_assert(xp::THREADS == BLOCK, "nblocks() counts blocks of BLOCK threads");
    hipLaunchKernelGGL(xp::k_merge_expiry, grid, block, 0, s, g);
    TC_LAUNCH(e->key_mode ? e->m_done : (hipEvent_t) nullptr, xp::k_merge_tat, grid, block, 0, s, g);
    TC_HIP(e, hipGetLastError());
    if (!e->key_mode) return TC_E_OK;
    // did a key of this import (or of an asynchronous batch before it) fail to get a slot?  The one wait of the call.
    uint32_t flag = 0;
    TC_HIP(e, hipMemcpyAsync(&flag, e->kt.error_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    TC_HIP(e, hipStreamSynchronize(s));
    if (flag) {
        TC_HIP(e, hipMemsetAsync(e->kt.error_flag, 0, sizeof flag, s));
        return fail(e, TC_E_TABLE_FULL, "key table full: some entries were rejected (out_count[1]); the others were merged");
    }
    return poisoned(e);
}
