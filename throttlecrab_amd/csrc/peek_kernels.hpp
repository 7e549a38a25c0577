// peek_kernels.hpp -- read-only batch queries (tc_peek_batch_keys / tc_peek_batch_slots) for gfx950.
//
// Answer i is what RateLimiter::rate_limit (rate_limiter.rs:102-250) would return for request i if it were the next and only
// request: tc::gcra_step<true> on a COPY of the key's cell, the copy thrown away.  The reference has no such call -- its
// quantity-0 request stores the clamped TAT and a new TTL (rate_limiter.rs:158-195) and inserts an unknown key.
//
// One launch, one lane per request, 256 threads, grid ceil(n / 256); nothing is shared between lanes: no LDS, no atomics, no wait
// on another workgroup, and NO STORE to anything but the caller's output arrays -- the key table, the cells, the counters, the
// denial counters and the hints are only ever read (a `const` view would say so, but ev::Params is the evaluation kernels'
// argument block and is reused here so that ev::write_out packs the records of both paths).
//
// Load schedule of a lane (every step's loads are issued before the step's values are needed by the next):
//   1. its own columns: plan id -> dictionary row (or the triple), quantity, timestamp; for slots the slot id
//   2. KEYS: kt::probe_request<false> -- offsets, key words, hash, then the chain from the hash's home position (tombstones are
//      stepped over, an empty entry ends it, a hit is confirmed by the full key: inside the 32-byte entry up to 16 bytes, against
//      the slot's KeyRec / the overflow arena beyond).  The probe loop is key_table.hpp's, not a copy of it.
//   3. the cell gather: one 16-byte load ({tat, expiry}), or the 8-byte TAT of a TC_CFG_FIXED_PARAMS engine; an absent key, or a
//      slot out of range, loads nothing
//   4. (ei, dvt): derived from the triple (two IEEE divisions' worth of ALU work) resp. read from the registered class table
//      (rate_id -> class, two dependent loads) in the shadow of the cell gather, which nothing before step 5 waits for
//   5. the step on the copy, then one 16-byte store per tc_throttle, two per tc_decision, a byte each for allowed / status.
// The plans of a TC_B_PLAN_DICT batch are read from the dictionary HERE (2 bytes per request + a table that stays in L2) instead
// of being expanded into three 8-byte columns by mk::k_expand_plans first: that launch writes 24-28 bytes per request which this
// one would read back, for a call whose whole traffic is ~50 bytes per request.
#pragma once

#include "eval_kernels.hpp"

namespace pk {

using tc::Cell;
using tc::Decision;

constexpr int THREADS = 256;

struct Keys {
    const uint8_t* bytes; // the arena
    const uint32_t* off;  // [n + 1]
};
struct Dict {             // TC_B_PLAN_DICT (id == nullptr: the batch carries columns / scalars, or registered plans)
    const int64_t* plans; // [n_plans][3]
    const uint16_t* id;   // [n]
    const uint32_t* q32;  // [n] or nullptr
    uint32_t n_plans;
};

template <bool KEYS, bool FIXED>
__global__ __launch_bounds__(THREADS) void k_peek(ev::Params p, kt::Table t, Keys k, Dict dc) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= p.n) return;
    const bool registered = (p.flags & ev::F_REGISTERED) != 0u; // (wave-uniform, like every test of a pointer below)
    // 1. the request's own columns
    int64_t q = 0, now = 0, burst = 0, count = 0, period = 0;
    if (!registered) {
        q = dc.q32 ? (int64_t)dc.q32[i] : (p.q ? p.q[i] : p.q_s);
        now = p.now ? p.now[i] : p.now_s;
        if (dc.id) {
            const uint32_t id = dc.id[i];
            const bool known = id < dc.n_plans; // an index beyond the dictionary decodes to (0, 0, 0): TC_INVALID_RATE_LIMIT
            const int64_t* row = dc.plans + 3u * (size_t)(known ? id : 0u);
            const int64_t b0 = row[0], c0 = row[1], p0 = row[2];
            burst = known ? b0 : 0, count = known ? c0 : 0, period = known ? p0 : 0;
        } else {
            burst = p.burst ? p.burst[i] : p.burst_s;
            count = p.count ? p.count[i] : p.count_s;
            period = p.period ? p.period[i] : p.period_s;
        }
    }
    // 2. the key work: read-only (INSERT = false claims nothing, recycles nothing, raises no error flag)
    uint32_t slot;
    if (KEYS) {
        uint32_t ax;
        uint64_t h;
        bool recycled;
        kt::probe_request<false>(t, k.bytes, k.off, p.n, i, slot, ax, h, recycled); // slot = kt::NO_SLOT: no such key
    } else {
        slot = p.slot[i];
    }
    // 3. the cell gather (an absent key is the reference's "first request": a vacant cell)
    const bool have = slot < p.capacity;
    Cell raw;
    raw.tat = FIXED ? tc::TAT_VACANT : 0;
    raw.expiry = 0;
    if (have) raw = ev::load_raw<FIXED>(p, slot);
    // 4. validation and rate: derive_request's precedence (quantity, triple, domain), as the evaluation kernels' make_req
    ev::Req r;
    if (registered) {
        r = ev::make_req(p, i, slot); // (slots only: a slot out of range is TC_INTERNAL, a slot without a plan TC_INVALID_RATE_LIMIT)
    } else {
        r.q = q, r.now = now, r.limit = burst, r.ei = 0, r.dvt = 0;
        if (!KEYS && !have) r.status = tc::ST_INTERNAL; // (what tc_rate_limit_batch_slots answers for such a slot)
        else r.status = tc::derive_request(burst, count, period, q, now, r.ei, r.dvt);
    }
    // 5. the step, on the copy
    Decision d;
    d.allowed = false;
    d.remaining = d.reset_after = d.retry_after = 0;
    if (r.status == tc::ST_OK) {
        Cell c = FIXED ? tc::fixed_cell(raw.tat, r.dvt) : raw;
        d = tc::gcra_step<true>(c, r.ei, r.dvt, r.q, r.now);
    }
    ev::write_out<true>(p, i, r, d);
}

} // namespace pk
