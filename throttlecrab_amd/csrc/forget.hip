// forget.hip -- tc_forget_batch: named keys (or slots) leave the engine, on the device, ordered like any other key work
#include "engine.hpp"
#include "forget_kernels.hpp"

// Like the peeks and export / import, the call touches no host-side state of the batch path: no batch count, no operation of the
// cleanup policy, no sweep in front or behind, no seal of a TC_CFG_FIXED_PARAMS engine's plans, no grouping hint.  What it moves
// is the hand-over of the key table between the two streams (k_done / m_done) and the end of the "sweep beside the newest
// evaluation" chain.

template <bool KEYS, bool FIXED>
static void forget_launch(tc_engine* e, hipStream_t s, const fk::Args& a) {
    hipLaunchKernelGGL((fk::k_forget_find<KEYS, FIXED>), dim3((a.n + fk::THREADS - 1) / fk::THREADS), dim3(fk::THREADS), 0, s, a, e->kt);
    auto last = fk::k_forget_apply<KEYS, FIXED>;
    // key mode: the removal's completion is m_done, which the key stage, sweep or rebuild of any later call waits for before it
    // may touch the table (peek.hip: peek_launch)
    TC_LAUNCH(KEYS ? e->m_done : (hipEvent_t) nullptr, last, dim3((a.n + fk::APPLY_THREADS - 1) / fk::APPLY_THREADS), dim3(fk::APPLY_THREADS), 0, s, a, e->kt);
}

extern "C" int tc_forget_batch(tc_engine* e, const void* fp) {
    if (!e || !fp) return TC_E_INVALID_ARG;
    tc_forget f;
    memcpy(&f, fp, sizeof(uint32_t)); // (struct_size first: nothing beyond it is read from a shorter struct)
    if (f.struct_size < sizeof(tc_forget)) return TC_E_INVALID_ARG;
    memcpy(&f, fp, sizeof f);
    TC_CHECK_POISON(e);
    auto bad = [&](const char* what) { return fail(e, TC_E_INVALID_ARG, (std::string("tc_forget_batch: ") + what).c_str()); };
    if (f.flags != 0) return bad("flags must be 0");
    if (f.n == 0 || f.n > e->max_batch) return bad("n must be 1 .. max_batch");
    if (!f.out_count) return bad("out_count is NULL");
    if (e->key_mode ? (!f.key_bytes || !f.key_off) : !f.slot) return bad(e->key_mode ? "key_bytes / key_off is NULL" : "slot is NULL");
    TC_HIP(e, hipSetDevice(e->device));
    hipStream_t s = cur_stream(e);

    fk::Args a;
    memset(&a, 0, sizeof a);
    a.cells = e->cells, a.tat8 = e->tat8;
    a.rate_id = e->rate_id, a.classes = e->classes, a.uniform_class = e->uniform_id;
    a.capacity = (uint32_t)e->capacity;
    a.n = (uint32_t)f.n;
    a.slot = f.slot;
    a.found = e->k_slot;
    a.key_bytes = f.key_bytes, a.key_off = f.key_off;
    a.now = f.now_ns;
    a.was_live = f.was_live;
    a.out_count = reinterpret_cast<unsigned long long*>(f.out_count);
    a.denied = e->denied;
    a.counters = e->counters;

    if (e->key_mode) { // key work on the engine's stream: behind the key stream's last stage
        if (e->k_busy) TC_HIP(e, hipStreamWaitEvent(s, e->k_done, 0));
        aside_reset(e);
        forget_launch<true, false>(e, s, a);
        e->m_busy = true;
        e->k_busy = false;
    } else if (e->fixed) {
        forget_launch<false, true>(e, s, a);
    } else {
        forget_launch<false, false>(e, s, a);
    }
    TC_HIP(e, hipGetLastError());
    return TC_E_OK;
}
