// forget_kernels.hpp -- tc_forget_batch: a caller-named set of keys (or slots) leaves the engine, whatever their expiry (gfx950).
//
// The reference never removes a key (its HashMap grows; entries go when they have expired and a cleanup runs).  Here the table has
// a fixed size, so "forget" does to the named keys what the sweep does to expired ones -- mk::unbind_slot, the body k_sweep_fixup
// runs per slot -- and a forgotten key is then exactly a key that was never seen.
//
// Two launches, A before B on one stream, one lane per request (A: 256 threads, no LDS, no barrier; B: 1024 threads, 132 bytes of
// LDS, two barriers); neither waits for another workgroup.
//   A  k_forget_find   READ-ONLY on the engine.  Keys: kt::probe_request<false> (key_table.hpp's probe loop, not a copy: tombstones
//                      are stepped over, an empty entry ends the chain, a hit is confirmed by the full key) -> the slot, or
//                      kt::NO_SLOT, into the per-request slot scratch.  Then, if the caller asked for was_live, the cell gather:
//                      the expiry word (wide layout) or the TAT and the slot's plan id (fixed layout) are requested together,
//                      nothing is looked at before both are on their way.  Lane 0 zeroes out_count.
//   B  k_forget_apply  the removal.  A target may be named by many lanes (duplicates in the call), by lanes of different waves and
//                      blocks; exactly ONE of them must remove it, and they find out who without hashing or sorting anything:
//                      every lane clears the target's word with a returning atomic, and the lane that got the word back as it was
//                      before anybody cleared it is the owner --
//                        keys          fetch_and on the aligned 32-bit word of `bound` that holds the slot's byte, clearing that
//                                      byte alone; owner: saw the byte non-zero
//                        slots, wide   64-bit exchange of the cell's expiry word with 0; owner: got a non-zero expiry back (and
//                                      then stores tat = 0)
//                        slots, fixed  64-bit exchange of tat8[s] with TAT_VACANT; owner: got another value back
//                      The owner tests liveness on the old value and, in key mode, runs mk::unbind_slot.  Everything counted goes
//                      through wave ballots, and the waves' counts meet in LDS: ONE atomicAdd per block on out_count[0],
//                      out_count[1], TC_CNT_LIVE_SLOTS, the block's `tombs` shard and the free stack's pointer (an owner's place in
//                      the stretch that atomic reserved: the owners of the waves before + its rank inside its wave's ballot).
//                      Measured, 1 Mi keys over 10 M resident (tools/forgetbench.py): with one atomic per WAVE and word -- 16 384
//                      of them on each of four single words, ~13 ns apiece, as every kernel here that tried it found -- the call
//                      took 482 us; with one per block of 1024, 184 us.
// Why two launches: was_live and the probes must see the table as it was when the call began -- the second lane of a duplicated
// key would otherwise find it gone, and a probe chain would be walked through an entry that another lane is turning into a
// tombstone at that moment.  In one fused launch both are races.
#pragma once

#include "maintenance_kernels.hpp"

namespace fk {

using tc::Cell;

constexpr int THREADS = 256;        // k_forget_find (the probe's registers: as pk::k_peek)
constexpr int APPLY_THREADS = 1024; // k_forget_apply: the fewer blocks, the fewer atomics on the five shared words

struct Args {
    Cell* cells;                   // wide layout
    int64_t* tat8;                 // fixed layout
    const uint16_t* rate_id;       // fixed layout: the slots' plans (expiry = tat + dvt)
    const tc::RateClass* classes;
    uint32_t uniform_class;        // != 0: every slot carries this plan
    uint32_t capacity;
    uint32_t n;
    const uint32_t* slot;          // slot mode: the caller's column
    uint32_t* found;               // key mode: slot of request i or kt::NO_SLOT (A writes, B reads)
    const uint8_t* key_bytes;      // key mode: the arena
    const uint32_t* key_off;
    int64_t now;
    uint8_t* was_live;             // [n] or nullptr
    unsigned long long* out_count; // [2]
    uint32_t* denied;              // key mode + TC_CFG_TRACK_DENIED
    unsigned long long* counters;
};

// fixed layout: the plan's delay variation tolerance of slot `sl` (id 0, the all-zero class: no plan -- such a slot is vacant)
__device__ __forceinline__ int64_t fixed_dvt(const Args& a, uint32_t id) { return a.classes[a.uniform_class ? a.uniform_class : id].dvt; }

template <bool KEYS, bool FIXED>
__global__ __launch_bounds__(THREADS) void k_forget_find(Args a, kt::Table t) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i == 0u) a.out_count[0] = 0ull, a.out_count[1] = 0ull; // (B adds to them)
    if (i >= a.n) return;
    uint32_t sl;
    if (KEYS) {
        uint32_t ax;
        uint64_t h;
        bool recycled;
        kt::probe_request<false>(t, a.key_bytes, a.key_off, a.n, i, sl, ax, h, recycled); // INSERT = false: nothing is written
        a.found[i] = sl;
    } else {
        sl = a.slot[i];
    }
    if (a.was_live == nullptr) return; // (uniform over the grid)
    const bool have = sl < a.capacity; // (kt::NO_SLOT is not)
    bool live;
    if (FIXED) {
        const int64_t tat = a.tat8[have ? sl : 0u];
        const uint32_t id = a.uniform_class ? 0u : a.rate_id[have ? sl : 0u];
        live = have && tc::fixed_cell(tat, fixed_dvt(a, id)).expiry > (uint64_t)a.now;
    } else {
        live = have && a.cells[sl].expiry > (uint64_t)a.now; // the reference's strict test (adaptive_cleanup.rs:248)
    }
    a.was_live[i] = live ? (uint8_t)1 : (uint8_t)0;
}

template <bool KEYS, bool FIXED>
__global__ __launch_bounds__(APPLY_THREADS) void k_forget_apply(Args a, kt::Table t) {
    const uint32_t i = blockIdx.x * APPLY_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (no lane leaves early: the ballots and the barriers below are reached by whole blocks)
    const uint32_t sl = i < a.n ? (KEYS ? a.found[i] : a.slot[i]) : kt::NO_SLOT;
    const bool have = sl < a.capacity;
    bool owner = false, live = false;
    if (KEYS) {
        if (have) {
            // (`bound` is 256-byte aligned and its block padded to 256: the last slots' word lies inside it)
            uint32_t* word = reinterpret_cast<uint32_t*>(t.bound + (sl & ~3u));
            const uint32_t sh = 8u * (sl & 3u);
            const uint32_t old = __hip_atomic_fetch_and(word, ~(0xFFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            owner = ((old >> sh) & 0xFFu) != 0u;
        }
        if (owner) { // nobody else touches this slot's cell, record, counters or entry in this launch
            live = a.cells[sl].expiry > (uint64_t)a.now;
            mk::unbind_slot(a.cells, t, a.denied, sl); // (the tombstone is counted in the wave's shard below, not the entry's)
        }
    } else if (FIXED) {
        if (have) {
            const uint32_t id = a.uniform_class ? 0u : a.rate_id[sl];
            const int64_t old = (int64_t)__hip_atomic_exchange(reinterpret_cast<unsigned long long*>(&a.tat8[sl]), (unsigned long long)tc::TAT_VACANT,
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            owner = old != tc::TAT_VACANT;
            live = owner && tc::fixed_cell(old, fixed_dvt(a, id)).expiry > (uint64_t)a.now;
        }
    } else {
        if (have) {
            static_assert(sizeof(Cell::expiry) == 8 && sizeof(unsigned long long) == 8, "the expiry word is exchanged whole");
            const uint64_t old = __hip_atomic_exchange(reinterpret_cast<unsigned long long*>(&a.cells[sl].expiry), 0ull, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
            owner = old != 0ull;
            live = old > (uint64_t)a.now;
            if (owner) a.cells[sl].tat = 0;
        }
    }
    // the waves' ballot counts meet in LDS: one atomic per BLOCK and counter (see the header of this file)
    __shared__ uint32_t s_own[APPLY_THREADS / 64], s_live[APPLY_THREADS / 64];
    __shared__ int s_base;
    const unsigned long long m_own = __ballot(owner), m_live = __ballot(live);
    if (lane == 0) s_own[wave] = (uint32_t)__popcll(m_own), s_live[wave] = (uint32_t)__popcll(m_live);
    __syncthreads();
    uint32_t before = 0, total = 0, total_live = 0;
    for (int w = 0; w < APPLY_THREADS / 64; ++w) {
        if (w < wave) before += s_own[w];
        total += s_own[w];
        total_live += s_live[w];
    }
    if (total == 0u) return; // (block-uniform)
    if (threadIdx.x == 0) {
        atomicAdd(&a.out_count[0], (unsigned long long)total);
        if (total_live) atomicAdd(&a.out_count[1], (unsigned long long)total_live);
        if (KEYS) {
            atomicAdd(&a.counters[TC_CNT_LIVE_SLOTS], 0ull - (unsigned long long)total);
            atomicAdd(&t.tombs[blockIdx.x % kt::TOMB_SHARDS], total); // (the shards sum to the count)
            s_base = atomicAdd(t.free_top, (int)total);
        }
    }
    if (KEYS) {
        __syncthreads();
        // (bound slots + free slots == capacity, so the stretch lies inside the stack; a table that broke that is not written past)
        const int at = s_base + (int)before + (int)__popcll(m_own & ((1ull << lane) - 1ull));
        if (owner && at >= 0 && (uint32_t)at < t.capacity) t.free_slots[at] = sl;
    }
}

} // namespace fk
