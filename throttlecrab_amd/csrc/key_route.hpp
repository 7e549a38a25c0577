// key_route.hpp -- routing of a STRING-KEY batch to the GPUs that own its keys (gfx950): a stable, variable-length
// partition of a key arena (bytes + offsets[n + 1]) by owner, in HBM.
//
// owner(key) = mix64(hash(key) ^ SALT) mod world, exactly what tc_route_keys_host computes (the hash is kt::hash_key on the
// host and kt::request_hash on the device: the same value bit for bit), so who owns a key does not depend on where the
// batch was split.  Every destination's share comes out as a complete arena of its own -- bytes, offsets that start at 0,
// count + 1 of them -- that tc_rate_limit_batch_keys takes as it stands (TC_B_DEVICE_PTRS) or that is copied to a peer.
//
// Three launches, none of which waits for another workgroup (route_kernels.hpp's one-pass forms pay off because a slot id
// costs 12 instructions; here the bytes dominate, and a router that cannot stall is worth more than a saved launch):
//   k_count    one lane per key, tiles of TILE keys: hash -> owner (kept in a u8 column: the scatter does not hash again),
//              keys and bytes per destination and tile into two [world][tiles] rows
//   k_scan     one block per destination: exclusive prefix of both rows over the tiles, the totals
//   k_scatter  one block per tile: the tile's keys are counting-sorted by destination in LDS (stable), their lengths are
//              scanned in that order, and offsets, positions and bytes go out destination by destination
//   k_publish  (callers that poll pinned host memory) totals, then the caller's tag
//
// The bytes of a tile.  A tile's keys are ONE contiguous range of the input arena, and what the tile contributes to a
// destination is ONE contiguous range of that destination's output.  So the range is loaded into LDS coalesced (16
// bytes per lane where the address allows), and written back in 16-byte pieces of the OUTPUT: a lane takes an aligned
// 16-byte piece of some destination's range, finds the key its first byte belongs to by a binary search over the LDS
// scan, and walks on from there (a piece of short keys spans two or three of them).
// A tile whose bytes do not fit the staging buffer (STAGE bytes: 512 keys of up to 64 bytes do; keys can have any
// length) takes the same loop with its source bytes read from the arena instead of from LDS -- a direct global path,
// chosen over staging in pieces because the output side is the same code, such tiles are rare (keys over 64 bytes are
// a few per cent of the reference's workloads), and a lane's 16 consecutive source bytes share one or two memory lines.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "key_table.hpp" // kt::request_hash, kt::mix64

namespace krt {

constexpr int THREADS = 256, PER = 2;
constexpr uint32_t TILE = THREADS * PER; // keys per tile
constexpr uint32_t MAX_WORLD = 64;
constexpr uint32_t STAGE = 33 * 1024;    // staged bytes of a tile (+ 16: the tile keeps its alignment modulo 16 in LDS)
constexpr uint64_t SALT = 0xa5a5a5a5a5a5a5a5ull;

// x mod world for world <= 64 without a division: 2^32 mod world and floor(2^32 / world), made on the host
struct Mod {
    uint32_t world, inv, p32;
};
inline Mod make_mod(uint32_t world) {
    Mod m;
    m.world = world;
    m.inv = world > 1 ? (uint32_t)(((uint64_t)1 << 32) / world) : 0u;
    m.p32 = (uint32_t)((((uint64_t)1 << 32)) % world);
    return m;
}
// v mod world (world >= 2): floor(v * inv / 2^32) is the quotient or one less, so one conditional subtraction
__host__ __device__ __forceinline__ uint32_t mod32(const Mod& m, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t q = __umulhi(v, m.inv);
#else
    const uint32_t q = (uint32_t)(((uint64_t)v * m.inv) >> 32);
#endif
    uint32_t r = v - q * m.world;
    if (r >= m.world) r -= m.world;
    return r;
}
// x = hi * 2^32 + lo:  x mod w = ((hi mod w) * (2^32 mod w) + lo mod w) mod w -- equal to the host's `%` by arithmetic
__host__ __device__ __forceinline__ uint32_t owner_of(const Mod& m, uint64_t hash) {
    if (m.world < 2u) return 0u;
    const uint64_t x = kt::mix64(hash ^ SALT);
    return mod32(m, mod32(m, (uint32_t)(x >> 32)) * m.p32 + mod32(m, (uint32_t)x));
}

struct Work {
    uint32_t* tile_keys;  // [world][tiles] keys per destination and tile -> exclusive prefix over the tiles
    uint32_t* tile_bytes; // [world][tiles] ... and their bytes
    uint8_t* owner;       // [n]
    uint32_t* totals;     // [2 * world]: keys per destination, then bytes per destination (the caller's out_count)
    uint32_t tiles;
    volatile uint32_t* host_totals; // NULL or pinned host memory [2 * world + 1]: the totals, then `tag` (written last)
    uint32_t tag;
};

#if defined(__HIPCC__)
// lanes of the wave that are valid and carry my destination (`bits` ballots)
__device__ __forceinline__ unsigned long long same_owner(bool valid, uint32_t owner, int bits) {
    unsigned long long mm = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const unsigned long long bb = __ballot((owner >> b) & 1u);
        mm &= ((owner >> b) & 1u) ? bb : ~bb;
    }
    return mm;
}

static __global__ __launch_bounds__(THREADS) void k_count(const uint8_t* __restrict__ key_bytes, const uint32_t* __restrict__ key_off, uint32_t n,
                                                          Mod m, Work w) {
    __shared__ uint32_t s_k[MAX_WORLD], s_b[MAX_WORLD];
    if (threadIdx.x < MAX_WORLD) s_k[threadIdx.x] = s_b[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int bits = m.world > 1 ? 32 - __clz((int)m.world - 1) : 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int j = 0; j < PER; ++j) {
        const uint32_t i = blockIdx.x * TILE + j * THREADS + threadIdx.x;
        const bool valid = i < n;
        uint32_t owner = 0, len = 0;
        if (valid) {
            len = key_off[i + 1] - key_off[i];
            owner = owner_of(m, kt::request_hash(key_bytes, key_off, n, i));
            w.owner[i] = (uint8_t)owner;
        }
        // keys: one LDS add per destination and wave step.  Bytes: the lengths differ from lane to lane, so no ballot can
        // sum them; every lane adds its own (the LDS atomic unit takes same-address adds one per clock: 64 clocks at
        // worst, against the several hundred of the hash above)
        const unsigned long long mm = same_owner(valid, owner, bits);
        if (valid && (mm & lt) == 0ull) atomicAdd(&s_k[owner], (uint32_t)__popcll(mm));
        if (valid && len) atomicAdd(&s_b[owner], len);
    }
    __syncthreads();
    // (agent scope: the rows travel between kernels whose blocks sit on different XCDs, see route_kernels.hpp)
    if (threadIdx.x < m.world) {
        __hip_atomic_store(&w.tile_keys[(size_t)threadIdx.x * w.tiles + blockIdx.x], s_k[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.tile_bytes[(size_t)threadIdx.x * w.tiles + blockIdx.x], s_b[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one block per destination: exclusive prefix of its two rows over the tiles (each thread a contiguous piece), totals
static __global__ __launch_bounds__(THREADS) void k_scan(Work w, uint32_t world) {
    __shared__ uint32_t s_part[THREADS];
    const uint32_t per = (w.tiles + THREADS - 1) / THREADS;
    const uint32_t lo = min(threadIdx.x * per, w.tiles), hi = min(lo + per, w.tiles);
    for (int which = 0; which < 2; ++which) {
        uint32_t* row = (which ? w.tile_bytes : w.tile_keys) + (size_t)blockIdx.x * w.tiles;
        uint32_t sum = 0;
        for (uint32_t t = lo; t < hi; ++t) sum += __hip_atomic_load(&row[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads(); // (s_part of the first row has been read)
        s_part[threadIdx.x] = sum;
        __syncthreads();
        for (uint32_t off = 1; off < THREADS; off <<= 1) { // Hillis-Steele over 256 values in LDS
            const uint32_t o = threadIdx.x >= off ? s_part[threadIdx.x - off] : 0u;
            __syncthreads();
            s_part[threadIdx.x] += o;
            __syncthreads();
        }
        uint32_t run = s_part[threadIdx.x] - sum;
        for (uint32_t t = lo; t < hi; ++t) {
            const uint32_t c = __hip_atomic_load(&row[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&row[t], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            run += c;
        }
        if (threadIdx.x == THREADS - 1)
            __hip_atomic_store(&w.totals[which * world + blockIdx.x], s_part[THREADS - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// exclusive prefix of v over the 64 lanes of a wave; `total` = the sum
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t& total) {
    const int lane = threadIdx.x & 63;
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    total = __shfl(incl, 63, 64);
    return incl - v;
}

// one block per tile.  `only` >= 0: that destination's keys alone, from the start of the outputs; -1: every segment, one
// after the other: segment d starts at key (sum of the counts before d), its count + 1 offsets at out_off[that + d], its
// bytes at (sum of the bytes before d).
static __global__ __launch_bounds__(THREADS) void k_scatter(const uint8_t* __restrict__ key_bytes, const uint32_t* __restrict__ key_off, uint32_t n,
                                                            uint32_t world, Work w, int only, uint8_t* __restrict__ out_bytes,
                                                            uint32_t* __restrict__ out_off, uint32_t* __restrict__ out_pos) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[STAGE + 16]; // the tile's input bytes, at their address modulo 16
    __shared__ uint32_t s_off[TILE + 1];                 // the tile's input offsets
    __shared__ uint32_t s_scan[TILE + 1];                // key lengths in sorted order -> their exclusive prefix; [TILE] = the tile's bytes
    __shared__ uint16_t s_perm[TILE];                    // sorted position -> key of the tile
    __shared__ uint8_t s_own[TILE];
    __shared__ uint32_t s_wave[THREADS / 64][MAX_WORLD]; // per-wave counts -> exclusive prefix over the waves
    __shared__ uint32_t s_first[MAX_WORLD + 1];          // sorted position of each destination's first key of the tile
    __shared__ uint32_t s_kbase[MAX_WORLD];              // output key index of that key
    __shared__ uint32_t s_brel[MAX_WORLD];               // its byte offset inside its segment ...
    __shared__ uint32_t s_babs[MAX_WORLD];               // ... and inside out_bytes
    __shared__ uint32_t s_piece[MAX_WORLD + 1];          // 16-byte output pieces: exclusive prefix over the destinations
    __shared__ uint32_t s_wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x, t0 = tile * TILE, cnt = min(TILE, n - t0);

    for (uint32_t k = threadIdx.x; k <= TILE; k += THREADS) {
        s_off[k] = key_off[t0 + min(k, cnt)];
        s_scan[k] = 0;
    }
    for (uint32_t i = threadIdx.x; i < (THREADS / 64) * MAX_WORLD; i += THREADS) (&s_wave[0][0])[i] = 0;
    // wave-striped: step j of wave k covers keys k * 128 + j * 64 + lane of the tile (key order inside a wave)
    const uint32_t kfirst = wave * (64 * PER) + lane;
    uint32_t dest[PER], rank[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t k = kfirst + j * 64;
        dest[j] = k < cnt ? w.owner[t0 + k] : 0u;
        if (k < cnt) s_own[k] = (uint8_t)dest[j];
    }
    __syncthreads();
    // ---- stable counting sort by destination: rank of every key among the tile's keys of its destination
    const int bits = world > 1 ? 32 - __clz((int)world - 1) : 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const bool valid = kfirst + j * 64 < cnt;
        const unsigned long long mm = same_owner(valid, dest[j], bits);
        rank[j] = valid ? s_wave[wave][dest[j]] + (uint32_t)__popcll(mm & lt) : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && (mm & lt) == 0ull) s_wave[wave][dest[j]] += (uint32_t)__popcll(mm);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (wave == 0) { // lane d: destination d
        const uint32_t d = lane;
        uint32_t run = 0;
        for (int k = 0; k < THREADS / 64; ++k) {
            const uint32_t c = s_wave[k][d];
            s_wave[k][d] = run;
            run += c;
        }
        uint32_t total;
        s_first[d] = wave_exclusive(run, total);
        if (d == 63) s_first[MAX_WORLD] = total;
        uint32_t kat = 0, bat = 0, kt_ = 0, bt_ = 0;
        if (d < world) {
            if (only < 0)
                for (uint32_t k = 0; k < d; ++k) {
                    kat += __hip_atomic_load(&w.totals[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    bat += __hip_atomic_load(&w.totals[world + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            kt_ = __hip_atomic_load(&w.tile_keys[(size_t)d * w.tiles + tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bt_ = __hip_atomic_load(&w.tile_bytes[(size_t)d * w.tiles + tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_kbase[d] = kat + kt_;
        s_brel[d] = bt_;
        s_babs[d] = bat + bt_;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t k = kfirst + j * 64;
        if (k < cnt) {
            const uint32_t p = s_first[dest[j]] + s_wave[wave][dest[j]] + rank[j];
            s_perm[p] = (uint16_t)k;
            s_scan[p] = s_off[k + 1] - s_off[k];
        }
    }
    __syncthreads();
    // ---- exclusive scan of the lengths in sorted order (PER consecutive ones per thread); a destination's keys are
    // consecutive there, so "reset at each destination boundary" is a subtraction of the scan at its first key
    {
        uint32_t v[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            v[j] = s_scan[threadIdx.x * PER + j];
            sum += v[j];
        }
        uint32_t wtotal;
        uint32_t excl = wave_exclusive(sum, wtotal);
        if (lane == 0) s_wsum[wave] = wtotal;
        __syncthreads();
        for (int k = 0; k < wave; ++k) excl += s_wsum[k];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            s_scan[threadIdx.x * PER + j] = excl;
            excl += v[j];
        }
        if (threadIdx.x == THREADS - 1) s_scan[TILE] = excl;
    }
    __syncthreads();
    const uint32_t in0 = s_off[0], tile_bytes = s_scan[TILE];
    const uint32_t pad = (uint32_t)((uintptr_t)(key_bytes + in0) & 15u);
    const bool staged = tile_bytes <= STAGE; // (block-uniform)
    // ---- offsets and positions, in sorted order (consecutive lanes, consecutive outputs)
    for (uint32_t p = threadIdx.x; p < cnt; p += THREADS) {
        const uint32_t k = s_perm[p], d = s_own[k];
        if (only >= 0 && d != (uint32_t)only) continue;
        const uint32_t g = s_kbase[d] + (p - s_first[d]);
        out_off[g + (only < 0 ? d : 0u)] = s_brel[d] + (s_scan[p] - s_scan[s_first[d]]);
        if (out_pos) out_pos[g] = t0 + k;
    }
    // (the entry that closes a segment: its byte total)
    if (tile == 0 && threadIdx.x < world && (only < 0 || threadIdx.x == (uint32_t)only)) {
        const uint32_t d = threadIdx.x;
        uint32_t at = only < 0 ? d : 0u;
        for (uint32_t k = only < 0 ? 0u : d; k <= d; ++k) at += __hip_atomic_load(&w.totals[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out_off[at] = __hip_atomic_load(&w.totals[world + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the tile's bytes into LDS: whole aligned 16-byte words where they lie inside the tile, single bytes at its ends
    if (staged) {
        const uint8_t* src = key_bytes + in0;
        const uint32_t head = min((16u - pad) & 15u, tile_bytes), words = (tile_bytes - head) / 16u;
        for (uint32_t i = threadIdx.x; i < words; i += THREADS)
            *reinterpret_cast<uint4*>(&s_stage[pad + head + i * 16u]) = *reinterpret_cast<const uint4*>(src + head + i * 16u);
        const uint32_t tail0 = head + words * 16u;
        for (uint32_t i = threadIdx.x; i < head + (tile_bytes - tail0); i += THREADS) {
            const uint32_t b = i < head ? i : tail0 + (i - head);
            s_stage[pad + b] = src[b];
        }
    }
    // ---- 16-byte pieces of the output per destination (aligned on the output ADDRESS)
    if (wave == 0) {
        const uint32_t d = lane;
        uint32_t pieces = 0;
        if (d < world && (only < 0 || d == (uint32_t)only)) {
            const uint32_t len = s_scan[s_first[d + 1]] - s_scan[s_first[d]];
            const uint32_t mis = (uint32_t)((uintptr_t)(out_bytes + s_babs[d]) & 15u);
            pieces = len ? (mis + len + 15u) / 16u : 0u;
        }
        uint32_t total;
        s_piece[d] = wave_exclusive(pieces, total);
        if (d == 63) s_piece[MAX_WORLD] = total;
    }
    __syncthreads();
    const uint32_t pieces = s_piece[MAX_WORLD];
    for (uint32_t c = threadIdx.x; c < pieces; c += THREADS) {
        // the destination of piece c: the last d with s_piece[d] <= c (destinations without pieces repeat their successor's value)
        uint32_t d = 0;
        for (uint32_t step = MAX_WORLD / 2; step; step >>= 1)
            if (s_piece[d + step] <= c) d += step;
        const uint32_t pf = s_first[d], pl = s_first[d + 1]; // the destination's keys in sorted order: [pf, pl)
        const uint32_t q0 = s_scan[pf], len = s_scan[pl] - q0;
        uint8_t* dst = out_bytes + s_babs[d];
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
        const uint32_t c16 = (c - s_piece[d]) * 16u;
        const uint32_t lo = c16 > mis ? c16 - mis : 0u, hi = min(c16 + 16u - mis, len); // bytes [lo, hi) of the destination's range
        // the key of byte q0 + lo: the last p in [pf, pl) whose scan is <= it and that is followed by a greater one
        uint32_t a = pf, b = pl; // invariant: scan[a] <= q, scan[b] > q
        const uint32_t q = q0 + lo;
        while (b - a > 1u) {
            const uint32_t mid = (a + b) >> 1;
            if (s_scan[mid] <= q) a = mid;
            else b = mid;
        }
        uint32_t p = a, end = s_scan[p + 1];
        uint32_t from = s_off[s_perm[p]] - in0 - s_scan[p]; // source byte of sorted byte x of this key: from + x (wraps, as intended)
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        const bool whole = hi - lo == 16u;
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint32_t x = q + i;
            if (lo + i < hi) {
                while (x >= end) { // (empty keys are stepped over)
                    ++p;
                    end = s_scan[p + 1];
                    from = s_off[s_perm[p]] - in0 - s_scan[p];
                }
                const uint32_t sb = from + x;
                const uint32_t v = staged ? s_stage[pad + sb] : key_bytes[(size_t)in0 + sb];
                if (whole) word[i >> 2] |= v << (8u * (i & 3u));
                else dst[lo + i] = (uint8_t)v;
            }
        }
        if (whole) *reinterpret_cast<uint4*>(dst + lo) = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

static __global__ __launch_bounds__(2 * MAX_WORLD) void k_publish(Work w, uint32_t world) {
    if (threadIdx.x < 2 * world) w.host_totals[threadIdx.x] = __hip_atomic_load(&w.totals[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        w.host_totals[2 * world] = w.tag;
        __threadfence_system();
    }
}
#endif // __HIPCC__

} // namespace krt
