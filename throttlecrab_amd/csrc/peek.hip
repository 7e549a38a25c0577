// peek.hip -- tc_peek_batch_keys / tc_peek_batch_slots: what rate_limit WOULD answer, for a whole batch, with nothing changed
#include "engine.hpp"
#include "peek_kernels.hpp"

// The calls touch no host-side state of the engine either: no batch count, no operation count of the cleanup policy, no sweep in
// front or behind (auto_sweep_before / auto_sweep_after are not called), no seal of a TC_CFG_FIXED_PARAMS engine's plans, no
// grouping set, no hint.  What they do move is the hand-over of the key table between the two streams that work on it (below) and
// the "a sweep may go beside the newest evaluation" chain, which a call between a key batch and its sweep ends (aside_reset).

// host arrays of a peek -> the engine's staging buffers (the batch path's: stage_keys / e->stage, nothing of its own), on the
// engine's stream; `d` gets the device pointers.  Every copy goes through copy_async or the one-launch copy (tc_debug_fail_copy).
static int peek_stage_inputs(tc_engine* e, const Batch& b, bool keys, Batch& d) {
    const uint64_t n = b.n;
    hipStream_t s = cur_stream(e);
    const int64_t* hin[5] = {b.max_burst, b.count_per_period, b.period, b.quantity, b.now_ns};
    const int64_t** din[5] = {&d.max_burst, &d.count_per_period, &d.period, &d.quantity, &d.now_ns};
    if (keys) {
        if (b.key_off[n] < b.key_off[0]) return fail(e, TC_E_INVALID_ARG, "key_off must not decrease");
        TC_TRY(stage_keys(e, b.key_bytes, b.key_off, n, &d.key_bytes, &d.key_off, &b)); // (the request columns ride along)
    } else {
        const void* c_src[6] = {b.slot};
        void* c_dst[6];
        size_t c_bytes[6] = {n * sizeof(uint32_t)};
        uint32_t c_n = 1;
        TC_TRY(stage_need(e, e->stage.slot, e->max_batch));
        c_dst[0] = e->stage.slot;
        for (int j = 0; j < 5; ++j) {
            if (!hin[j]) continue;
            TC_TRY(stage_need(e, e->stage.in[j], e->max_batch));
            c_src[c_n] = hin[j], c_dst[c_n] = e->stage.in[j], c_bytes[c_n] = n * sizeof(int64_t);
            ++c_n;
        }
        TC_TRY(stage_in_multi(e, c_src, c_dst, c_bytes, c_n, s));
        d.slot = e->stage.slot;
    }
    for (int j = 0; j < 5; ++j)
        if (hin[j]) *din[j] = e->stage.in[j];
    if (b.flags & TC_B_PLAN_DICT) { // the compact columns as they are: the kernel reads the dictionary itself (peek_kernels.hpp)
        tc_engine::Stage& st = e->stage;
        TC_TRY(stage_need(e, st.dict, (size_t)65536 * 3));
        TC_TRY(stage_need(e, st.plan_id, e->max_batch));
        if (b.quantity32) TC_TRY(stage_need(e, st.q32, e->max_batch));
        const void* c_src[3] = {b.plan_dict, b.plan_id, b.quantity32};
        void* c_dst[3] = {st.dict, st.plan_id, st.q32};
        const size_t c_bytes[3] = {(size_t)b.n_plans * 3 * sizeof(int64_t), (size_t)n * sizeof(uint16_t), b.quantity32 ? (size_t)n * sizeof(uint32_t) : 0};
        TC_TRY(stage_in_multi(e, c_src, c_dst, c_bytes, 3, s));
        d.plan_dict = st.dict, d.plan_id = st.plan_id, d.quantity32 = b.quantity32 ? st.q32 : nullptr;
    }
    return TC_E_OK;
}

// `d`: a validated peek whose every pointer is a device pointer -> one launch on the engine's stream
static int peek_launch(tc_engine* e, const Batch& d, bool keys) {
    hipStream_t s = cur_stream(e);
    Params p;
    memset(&p, 0, sizeof p);
    p.n = (uint32_t)d.n;
    p.slot = d.slot;
    p.burst = d.max_burst, p.count = d.count_per_period, p.period = d.period, p.q = d.quantity, p.now = d.now_ns;
    p.burst_s = d.max_burst_scalar, p.count_s = d.count_per_period_scalar, p.period_s = d.period_scalar;
    p.q_s = d.quantity_scalar, p.now_s = d.now_ns_scalar;
    p.allowed = d.allowed, p.status = d.status, p.decisions = d.decisions, p.throttle = d.throttle;
    p.cells = e->cells, p.tat8 = e->tat8;
    p.rate_id = e->rate_id, p.classes = e->classes, p.uniform_class = e->uniform_id;
    p.capacity = e->capacity;
    if (e->fixed) p.flags |= F_FIXED;
    if (d.flags & TC_B_REGISTERED_PARAMS) p.flags |= F_REGISTERED | (e->uniform_id ? F_UNIFORM_CLASS : 0u);
    const pk::Keys k{d.key_bytes, d.key_off};
    const pk::Dict dc{d.plan_dict, d.plan_id, d.quantity32, d.n_plans};
    const dim3 grid((p.n + pk::THREADS - 1) / pk::THREADS), block(pk::THREADS);
    if (!keys) { // nothing but the engine's stream works on a slot engine's cells
        if (e->fixed) hipLaunchKernelGGL((pk::k_peek<false, true>), grid, block, 0, s, p, e->kt, k, dc);
        else hipLaunchKernelGGL((pk::k_peek<false, false>), grid, block, 0, s, p, e->kt, k, dc);
        TC_HIP(e, hipGetLastError());
        return TC_E_OK;
    }
    // The key table is worked on by the key stream too (key stages of TC_B_INPUTS_READY batches, sweeps that went aside), and the
    // two streams hand it to each other through k_done / m_done (keys.hip: resolve_keys_device).  A peek is key work on the
    // engine's stream: it goes behind the key stream's last stage (which covers every call that has returned: the evaluations
    // of those batches are on this stream already), and its own completion is m_done, which the key stage, sweep or rebuild of
    // any later call waits for before it may write what this kernel reads.  The event rides on the kernel's completion signal:
    // no event record, no synchronisation.
    if (e->k_busy) TC_HIP(e, hipStreamWaitEvent(s, e->k_done, 0));
    aside_reset(e); // (a later sweep goes behind this, on the engine's stream)
    auto kern = pk::k_peek<true, false>;
    TC_LAUNCH(e->m_done, kern, grid, block, 0, s, p, e->kt, k, dc);
    TC_HIP(e, hipGetLastError());
    e->m_busy = true;
    e->k_busy = false;
    return TC_E_OK;
}

static int peek_batch(tc_engine* e, const tc_batch* bp, void* out, bool keys) {
    if (!e || !bp || bp->struct_size < offsetof(tc_batch, n_segments)) return TC_E_INVALID_ARG;
    TC_CHECK_POISON(e);
    const char* const who = keys ? "tc_peek_batch_keys" : "tc_peek_batch_slots";
    auto bad = [&](int code, const char* what) { return fail(e, code, (std::string(who) + ": " + what).c_str()); };
    Batch b;
    memcpy(static_cast<tc_batch*>(&b), bp, std::min<size_t>(bp->struct_size, sizeof(tc_batch)));
    b.throttle = static_cast<tc_throttle*>(out);
    if (keys && !e->key_mode) return bad(TC_E_UNSUPPORTED, "engine was created without TC_CFG_KEY_MODE");
    if (!keys && e->key_mode) return bad(TC_E_INVALID_ARG, "key-mode engine: slots are assigned by the key table; use tc_peek_batch_keys");
    if (b.flags & TC_B_ASYNC) return bad(TC_E_UNSUPPORTED, "TC_B_ASYNC: a peek of host arrays is synchronous");
    if (b.flags & TC_B_GROUPED_OUTPUT) return bad(TC_E_UNSUPPORTED, "TC_B_GROUPED_OUTPUT: a peek is not grouped, row i answers request i");
    if (b.flags & TC_B_UNIQUE_SLOTS) return bad(TC_E_UNSUPPORTED, "TC_B_UNIQUE_SLOTS: the requests of a peek do not see one another anyway");
    if (b.n_segments) return bad(TC_E_UNSUPPORTED, "a segmented slot column (n_segments > 0) cannot be peeked");
    if (b.n == 0) return TC_E_OK;
    if (b.n > e->max_batch) return bad(TC_E_BATCH_TOO_LARGE, "batch larger than max_batch");
    if (b.allowed_bits || b.limit || b.remaining || b.reset_after_ns || b.retry_after_ns || b.result4 || b.order)
        return bad(TC_E_INVALID_ARG, "a peek writes decisions, allowed, status and `out` only; every other output pointer must be NULL");
    if (!b.decisions && !b.allowed && !b.status && !b.throttle) return bad(TC_E_INVALID_ARG, "no output: give decisions, allowed, status or `out`");
    if (((uintptr_t)b.throttle & 15u) || ((uintptr_t)b.decisions & 15u)) return bad(TC_E_INVALID_ARG, "`out` / decisions must be 16-byte aligned");
    if (keys) {
        if (!b.key_bytes || !b.key_off) return bad(TC_E_INVALID_ARG, "key_bytes/key_off is NULL");
        if (b.flags & TC_B_REGISTERED_PARAMS) return bad(TC_E_INVALID_ARG, "registered params do not apply to string keys");
    } else {
        if (!b.slot) return bad(TC_E_INVALID_ARG, "slot column is NULL");
        if (e->fixed && !(b.flags & TC_B_REGISTERED_PARAMS)) return bad(TC_E_UNSUPPORTED, "TC_CFG_FIXED_PARAMS: peeks use the registered plans (TC_B_REGISTERED_PARAMS)");
    }
    TC_TRY(dict_check(e, b));
    if (!(b.flags & TC_B_PLAN_DICT)) b.plan_dict = nullptr, b.plan_id = nullptr, b.quantity32 = nullptr, b.n_plans = 0;
    TC_HIP(e, hipSetDevice(e->device));
    if (b.flags & TC_B_DEVICE_PTRS) return peek_launch(e, b, keys); // asynchronous on the engine's stream
    // host arrays (pinned or pageable): staged, run, copied back, waited for
    Batch d = b;
    TC_TRY(peek_stage_inputs(e, b, keys, d)); // (a failed copy: TC_E_HIP, nothing was launched)
    TC_TRY(stage_outputs(e, b, d));
    TC_TRY(peek_launch(e, d, keys));
    TC_TRY(copy_outputs_back(e, b, cur_stream(e)));
    TC_HIP(e, hipStreamSynchronize(cur_stream(e)));
    return poisoned(e);
}

extern "C" int tc_peek_batch_keys(tc_engine* e, const tc_batch* bp, void* out) { return peek_batch(e, bp, out, true); }
extern "C" int tc_peek_batch_slots(tc_engine* e, const tc_batch* bp, void* out) { return peek_batch(e, bp, out, false); }
