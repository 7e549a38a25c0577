// export_kernels.hpp -- live limiter state out of an engine and into another (tc_export_live / tc_import_live) for gfx950.
//
// EXPORT: an ordered, variable-length compaction of the live entries of a page of slots into the project's own arena form
// (key bytes + offsets[count + 1], beside them the source slot, TAT and expiry of every entry): entry k is the k-th live
// slot of the page, in ascending slot order.  "Live" is the reference's strict test, expiry > now; on a key-mode engine the
// slot must be bound and, with world >= 2, its key must belong to destination `only` under tc_route_keys_host's map -- taken
// from the hash the slot's record stores, the key bytes are not hashed again.  Read-only: no cell, table word or counter is
// written.
//
// Three launches, none of which waits for another workgroup (as key_route.hpp):
//   k_count    one block per TILE of consecutive slots (tiles are aligned on multiples of TILE, so the `bound` bytes of a
//              tile are whole 16-byte words; a page that starts or ends inside a tile masks the slots outside it): the tile's
//              `bound` bytes as packed words into LDS, the 16-byte cells coalesced (round j of a thread is slot
//              tile + j * 256 + thread), the KeyRec header word (hash, length) of live bound slots only; (entries, bytes) per
//              tile by wave ballot / wave sum and one LDS step -> one pair per tile
//   k_scan     one block: exclusive prefixes of both rows over the tiles, the totals to out_count and to the caller's pinned
//              words (the tag last), the "it fits" word, and the offset that closes the arena
//   k_scatter  one block per tile: the same flags again, ranked by wave ballot + the LDS prefix over (round, wave), lengths by
//              a wave scan + the same prefix; slot, TAT, expiry and offset of consecutive live lanes go to consecutive
//              entries.  Key bytes: the waves walk their live keys one at a time, 64 lanes over the bytes of one key -- from
//              the KeyRec line, or from the current half of the overflow arena for keys over 112 bytes -- into an LDS stage
//              that keeps the OUTPUT's address modulo 16, and the stage goes out in aligned 16-byte pieces (single bytes at
//              its two ends, which neighbouring tiles share a piece with).  A tile's keys come in offset order, so what does
//              not fit the stage is a suffix of the tile: those keys are copied straight to the arena by their wave.
// If the page's totals exceed the room the caller gave (or 2^32 - 1 bytes: offsets are 32-bit), k_scatter does nothing.
// Slot-mode engines: the <false> variants, without `bound`, records and bytes.
//
// IMPORT (the merge, behind the key table's unchanged insert stage in key mode): over everything one call aims at a slot,
//     expiry' = max(resident expiry, imported expiries)
//     tat'    = max(imported tats, and the resident tat iff the resident expiry != 0)
// -- commutative and associative, so duplicates and order cannot matter; never more permissive than either source (a larger
// TAT is more quota used), resident as long as either would be.  TATs are any int64 (tc_store_set_if_not_exists_with_ttl stores
// what it is given), and a vacant cell's TAT word (0) must not take part.  Two launches, A before B on one stream:
//   A  k_merge_expiry  unsigned 64-bit atomic max on the cell's expiry, keeping the old value.  An entry takes part only with
//                      expiry != 0, so after the first such atomic on a cell its expiry is non-zero for good: EXACTLY ONE
//                      entry per vacant cell sees old == 0, and that one stores INT64_MIN -- the identity of a signed max --
//                      into the cell's TAT.  Nothing else writes a TAT in A, and nothing reads one.
//   B  k_merge_tat     signed 64-bit atomic max on the cell's TAT.  When B starts, every cell that was vacant holds INT64_MIN
//                      and every other cell its resident TAT, so the maxima are the rule above whatever order they land in
//                      (imported INT64_MIN included: the maximum of a set that holds only it).  B also counts the entries.
// A cell is 16 bytes read and written as one by the evaluations; nothing evaluates between A and B (one stream).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcra_math.hpp"
#include "key_route.hpp" // krt::Mod, krt::owner_of, krt::wave_exclusive
#include "key_table.hpp"

namespace xp {

constexpr int THREADS = 256, PER = 8, WAVES = THREADS / 64;
constexpr uint32_t TILE = THREADS * PER;  // 2 048 slots
constexpr uint32_t STAGE = 48 * 1024;     // staged key bytes of a tile (+ 16: the stage keeps the output's address modulo 16)

struct Page {
    const tc::Cell* cells;
    uint64_t first, end; // slots [first, end)
    uint64_t tile0;      // first / TILE: block b works on slots [(tile0 + b) * TILE, + TILE)
    int64_t now;
    krt::Mod mod;        // world < 2: every live key
    uint32_t only;
};
struct Work {
    unsigned long long* tile_bytes; // [tiles] key bytes per tile -> exclusive prefix
    uint32_t* tile_entries;         // [tiles] live entries per tile -> exclusive prefix
    uint32_t* fits;                 // the page's totals fit the outputs
    uint32_t tiles;
};
struct Out {
    uint32_t* slot;
    uint8_t* key_bytes;
    uint32_t* key_off;
    int64_t* tat;
    uint64_t* expiry;
    unsigned long long* count;               // device [2]
    volatile unsigned long long* count_host; // NULL or pinned [3]
    unsigned long long tag;
    uint64_t cap_entries, cap_bytes;
};

#if defined(__HIPCC__)
// what a thread knows of its PER slots of the tile (round j: slot tile + j * THREADS + thread)
struct Items {
    int64_t tat[PER];
    uint64_t expiry[PER];
    uint32_t len[PER];
    bool live[PER];
};

// reached by every thread of the block (one barrier in key mode)
template <bool KEYS>
__device__ __forceinline__ void classify(const Page& p, const kt::Table& t, uint64_t t0, uint8_t* s_bound, Items& it) {
    if (KEYS) { // the tile's `bound` bytes: 128 threads, one aligned 16-byte word each (single bytes at the table's end)
        if (threadIdx.x < TILE / 16u) {
            const uint64_t at = t0 + (uint64_t)threadIdx.x * 16u;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (at + 16u <= t.capacity) {
                v = *reinterpret_cast<const uint4*>(t.bound + at);
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t b = 0; b < 16u; ++b)
                    if (at + b < t.capacity && t.bound[at + b]) w[b >> 2] |= 1u << (8u * (b & 3u));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(s_bound + threadIdx.x * 16u) = v;
        }
        __syncthreads();
    }
    bool want[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) { // every cell is requested before one is looked at
        const uint64_t s = t0 + (uint64_t)j * THREADS + threadIdx.x;
        want[j] = s >= p.first && s < p.end && (!KEYS || s_bound[j * THREADS + threadIdx.x] != 0);
        tc::Cell c;
        c.tat = 0, c.expiry = 0;
        if (want[j]) c = tc::load_cell(&p.cells[s]);
        it.tat[j] = c.tat, it.expiry[j] = c.expiry;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        it.live[j] = want[j] && it.expiry[j] > (uint64_t)p.now;
        it.len[j] = 0;
    }
    if (KEYS) {
        uint4 h[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) { // hash, length, position: the first 16 bytes of the slot's record line
            h[j] = make_uint4(0u, 0u, 0u, 0u);
            if (it.live[j]) h[j] = *reinterpret_cast<const uint4*>(&t.rec[t0 + (uint64_t)j * THREADS + threadIdx.x]);
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (!it.live[j]) continue;
            it.len[j] = h[j].z == kt::NO_SLOT ? 0u : h[j].z;
            if (p.mod.world >= 2u) it.live[j] = krt::owner_of(p.mod, (uint64_t)h[j].x | ((uint64_t)h[j].y << 32)) == p.only;
            if (!it.live[j]) it.len[j] = 0;
        }
    }
}

template <bool KEYS>
static __global__ __launch_bounds__(THREADS) void k_count(Page p, kt::Table t, Work w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_bound[KEYS ? TILE : 16u];
    __shared__ uint32_t s_e[WAVES];
    __shared__ unsigned long long s_b[WAVES];
    Items it;
    classify<KEYS>(p, t, (p.tile0 + blockIdx.x) * TILE, s_bound, it);
    uint32_t entries = 0; // (the same in every lane of a wave)
    unsigned long long bytes = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        entries += (uint32_t)__popcll(__ballot(it.live[j]));
        bytes += it.len[j];
    }
    if (KEYS)
        for (int off = 32; off > 0; off >>= 1) bytes += __shfl_down(bytes, off, 64);
    if ((threadIdx.x & 63) == 0) s_e[threadIdx.x >> 6] = entries, s_b[threadIdx.x >> 6] = bytes;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < WAVES; ++k) entries += s_e[k], bytes += s_b[k];
        // (agent scope: the rows travel between kernels whose blocks sit on different XCDs, as key_route.hpp's)
        __hip_atomic_store(&w.tile_entries[blockIdx.x], entries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.tile_bytes[blockIdx.x], bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one block: exclusive prefixes over the tiles (each thread a contiguous piece), totals, "it fits", the closing offset
template <bool KEYS>
static __global__ __launch_bounds__(THREADS) void k_scan(Work w, Out o) {
    __shared__ unsigned long long s_e[THREADS], s_b[THREADS];
    const uint32_t per = (w.tiles + THREADS - 1) / THREADS;
    const uint32_t lo = min(threadIdx.x * per, w.tiles), hi = min(lo + per, w.tiles);
    unsigned long long se = 0, sb = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        se += __hip_atomic_load(&w.tile_entries[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sb += __hip_atomic_load(&w.tile_bytes[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_e[threadIdx.x] = se, s_b[threadIdx.x] = sb;
    __syncthreads();
    for (uint32_t off = 1; off < THREADS; off <<= 1) { // Hillis-Steele over 256 pairs in LDS
        const unsigned long long oe = threadIdx.x >= off ? s_e[threadIdx.x - off] : 0ull, ob = threadIdx.x >= off ? s_b[threadIdx.x - off] : 0ull;
        __syncthreads();
        s_e[threadIdx.x] += oe, s_b[threadIdx.x] += ob;
        __syncthreads();
    }
    unsigned long long re = s_e[threadIdx.x] - se, rb = s_b[threadIdx.x] - sb;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t ce = __hip_atomic_load(&w.tile_entries[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long cb = __hip_atomic_load(&w.tile_bytes[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.tile_entries[k], (uint32_t)re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (< capacity < 2^32)
        __hip_atomic_store(&w.tile_bytes[k], rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        re += ce, rb += cb;
    }
    if (threadIdx.x == THREADS - 1) {
        const unsigned long long entries = s_e[THREADS - 1], bytes = s_b[THREADS - 1];
        const bool fits = entries <= o.cap_entries && bytes <= o.cap_bytes && bytes <= 0xFFFFFFFFull;
        __hip_atomic_store(w.fits, fits ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.count[0] = entries, o.count[1] = bytes;
        if (KEYS && fits) o.key_off[entries] = (uint32_t)bytes; // (entries == 0: the arena's only offset, 0)
        if (o.count_host) {
            o.count_host[0] = entries, o.count_host[1] = bytes;
            __threadfence_system();
            o.count_host[2] = o.tag;
            __threadfence_system();
        }
    }
}

template <bool KEYS>
static __global__ __launch_bounds__(THREADS) void k_scatter(Page p, kt::Table t, Work w, Out o) {
    if (__hip_atomic_load(w.fits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return; // (uniform over the grid)
    __shared__ __attribute__((aligned(16))) uint8_t s_bound[KEYS ? TILE : 16u];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[KEYS ? STAGE + 16u : 16u];
    __shared__ uint32_t s_cnt[PER * WAVES], s_byt[PER * WAVES]; // per (round, wave) -> exclusive prefix in that order
    __shared__ uint32_t s_end;                                  // bytes of the tile that went through the stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t t0 = (p.tile0 + blockIdx.x) * TILE;
    Items it;
    classify<KEYS>(p, t, t0, s_bound, it);
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t rank[PER], rel[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const unsigned long long m = __ballot(it.live[j]);
        rank[j] = (uint32_t)__popcll(m & lt);
        uint32_t total = 0;
        rel[j] = KEYS ? krt::wave_exclusive(it.len[j], total) : 0u;
        if (lane == 0) s_cnt[j * WAVES + wave] = (uint32_t)__popcll(m), s_byt[j * WAVES + wave] = total;
    }
    if (threadIdx.x == 0) s_end = 0u;
    __syncthreads();
    if (wave == 0) { // lane k: (round, wave) pair k
        uint32_t total;
        const uint32_t c = lane < PER * WAVES ? s_cnt[lane] : 0u, b = lane < PER * WAVES ? s_byt[lane] : 0u;
        const uint32_t ce = krt::wave_exclusive(c, total), be = krt::wave_exclusive(b, total);
        if (lane < PER * WAVES) s_cnt[lane] = ce, s_byt[lane] = be;
    }
    __syncthreads();
    const uint32_t ebase = __hip_atomic_load(&w.tile_entries[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long bbase = __hip_atomic_load(&w.tile_bytes[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t my_end = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { // consecutive live lanes, consecutive entries
        rel[j] += s_byt[j * WAVES + wave];
        if (!it.live[j]) continue;
        const uint64_t g = (uint64_t)ebase + s_cnt[j * WAVES + wave] + rank[j];
        if (o.slot) o.slot[g] = (uint32_t)(t0 + (uint64_t)j * THREADS + threadIdx.x);
        o.tat[g] = it.tat[j];
        o.expiry[g] = it.expiry[j];
        if (KEYS) {
            o.key_off[g] = (uint32_t)(bbase + rel[j]);
            if (rel[j] + it.len[j] <= STAGE) my_end = max(my_end, rel[j] + it.len[j]);
        }
    }
    if (!KEYS) return;
    if (my_end) atomicMax(&s_end, my_end);
    uint8_t* const dst = o.key_bytes + bbase;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 15u);
    const uint8_t* const ovf = t.overflow + (uint64_t)*t.overflow_half * t.overflow_bytes;
#pragma unroll
    for (int j = 0; j < PER; ++j) { // the wave's live keys of round j, one at a time, 64 lanes over one key's bytes
        unsigned long long m = __ballot(it.live[j] && it.len[j] != 0u);
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const uint32_t ln = __shfl(it.len[j], k, 64), rl = __shfl(rel[j], k, 64);
            const kt::KeyRec& kr = t.rec[t0 + (uint64_t)j * THREADS + (uint32_t)wave * 64u + (uint32_t)k];
            const uint8_t* src = kr.bytes;
            if (ln > kt::INLINE_KEY) {
                uint64_t off;
                __builtin_memcpy(&off, kr.bytes, 8);
                src = ovf + off;
            }
            if (rl + ln <= STAGE) {
                for (uint32_t b = lane; b < ln; b += 64u) s_stage[pad + rl + b] = src[b];
            } else { // (a suffix of the tile: everything behind the first key that does not fit)
                for (uint32_t b = lane; b < ln; b += 64u) dst[rl + b] = src[b];
            }
        }
    }
    __syncthreads();
    // the stage -> the arena: aligned 16-byte pieces of the OUTPUT, single bytes at the two ends
    const uint32_t staged = s_end;
    const uint32_t head = min((16u - pad) & 15u, staged), words = (staged - head) / 16u, tail0 = head + words * 16u;
    for (uint32_t i = threadIdx.x; i < words; i += THREADS)
        *reinterpret_cast<uint4*>(dst + head + i * 16u) = *reinterpret_cast<const uint4*>(&s_stage[pad + head + i * 16u]);
    for (uint32_t i = threadIdx.x; i < head + (staged - tail0); i += THREADS) {
        const uint32_t b = i < head ? i : tail0 + (i - head);
        dst[b] = s_stage[pad + b];
    }
}

// ---- import: the merge (see the header comment for the argument) ----------------------------------------------------
struct Merge {
    tc::Cell* cells;
    uint64_t capacity;
    const uint32_t* slot; // [n] (key mode: what the insert stage resolved; kt::NO_SLOT = the key found no slot)
    const int64_t* tat;
    const uint64_t* expiry;
    uint32_t n;
    unsigned long long* out_count; // [2]: merged, rejected
};

static __global__ __launch_bounds__(THREADS) void k_merge_expiry(Merge m) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i == 0) m.out_count[0] = 0ull, m.out_count[1] = 0ull; // (k_merge_tat adds)
    if (i >= m.n) return;
    const uint32_t s = m.slot[i];
    const uint64_t ex = m.expiry[i];
    if (ex == 0 || s >= m.capacity) return;
    tc::Cell* c = &m.cells[s];
    const unsigned long long old = __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(&c->expiry), (unsigned long long)ex, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
    if (old == 0ull) __hip_atomic_store(reinterpret_cast<long long*>(&c->tat), (long long)INT64_MIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static __global__ __launch_bounds__(THREADS) void k_merge_tat(Merge m) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const bool valid = i < m.n;
    bool ok = false;
    if (valid) {
        const uint32_t s = m.slot[i];
        ok = m.expiry[i] != 0 && s < m.capacity;
        if (ok) __hip_atomic_fetch_max(reinterpret_cast<long long*>(&m.cells[s].tat), (long long)m.tat[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t merged = (uint32_t)__popcll(__ballot(ok)), rejected = (uint32_t)__popcll(__ballot(valid && !ok));
    if ((threadIdx.x & 63) == 0) {
        if (merged) atomicAdd(&m.out_count[0], (unsigned long long)merged);
        if (rejected) atomicAdd(&m.out_count[1], (unsigned long long)rejected);
    }
}
#endif // __HIPCC__

} // namespace xp
