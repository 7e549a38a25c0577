// The hot list's maker (throttlecrab_amd/csrc/hot_list.hpp: what slots.hip's hot_make runs) against a brute-force model: a
// map of the notes, a full sort, the keep-or-remake rule written out once more.  No GPU, no engine.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "hot_list.hpp"

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

using u64 = unsigned long long;
static const hl::Limits L = hl::ENGINE;

static u64 rnd_state = 88172645463325252ULL;
static u64 rnd() {
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
    return rnd_state;
}

static u64 note(uint32_t len, uint32_t slot, uint32_t tag = 0) { return ((u64)len << 44) | ((u64)(tag & 0xFFFu) << 32) | slot; }

struct Notes {
    std::vector<u64> w = std::vector<u64>(L.notes, 0ull);
    uint32_t used = 0;
    void add(uint32_t len, uint32_t slot) {
        CHECK(used < L.notes);
        w[used++] = note(len, slot, (uint32_t)rnd());
    }
    void shuffle() { // (empty words anywhere in the table, as the device's two hashed halves leave them)
        for (uint32_t i = L.notes - 1; i > 0; --i) std::swap(w[i], w[rnd() % (i + 1)]);
    }
};

// ---- the model ----
struct Model {
    std::vector<uint32_t> made;
    // the slots below `capacity` with a run of at least heavy_min, longest first, ties: the smaller slot first, cut to hot_max
    static std::vector<uint32_t> ranked(const Notes& n, uint32_t heavy_min, uint64_t capacity, std::map<uint32_t, uint32_t>* all = nullptr) {
        std::map<uint32_t, uint32_t> best;
        for (const u64 v : n.w) {
            const uint32_t len = (uint32_t)(v >> 44), slot = (uint32_t)(v & 0xFFFFFFFFull);
            if (len >= heavy_min && slot < capacity) best[slot] = std::max(best[slot], len);
        }
        std::vector<std::pair<uint32_t, uint32_t>> by; // (length, slot)
        for (const auto& kv : best) by.push_back({kv.second, kv.first});
        std::sort(by.begin(), by.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
            return a.first != b.first ? a.first > b.first : a.second < b.second;
        });
        if (by.size() > L.hot_max) by.resize(L.hot_max);
        std::vector<uint32_t> out;
        for (const auto& p : by) out.push_back(p.second);
        if (all) *all = best;
        return out;
    }
    bool look(const Notes& n, uint32_t heavy_min, uint64_t capacity) {
        std::map<uint32_t, uint32_t> all;
        const std::vector<uint32_t> now = ranked(n, heavy_min, capacity, &all);
        bool keep;
        if (made.empty()) {
            keep = now.empty();
        } else {
            const std::set<uint32_t> cur(made.begin(), made.end());
            keep = true;
            for (const uint32_t s : now) // no slot of the new list with a long run is missing from the old one
                if (all[s] >= L.long_run && !cur.count(s)) keep = false;
            size_t noted = 0;
            for (const uint32_t s : made) noted += all.count(s);
            if (noted * 10 < made.size() * 9) keep = false;               // fewer than nine in ten still noted: stale
            if (now.size() * 4 > made.size() * 5 + 128) keep = false;     // a crowd of new hot slots
        }
        if (!keep) made = now;
        return !keep;
    }
};

struct Maker {
    std::vector<u64> scratch, found;
    std::vector<uint32_t> made;
    bool look(const Notes& n, uint32_t heavy_min, uint64_t capacity) { return hl::make_list(n.w.data(), L, heavy_min, capacity, scratch, found, made); }
};

static void check_list(const std::vector<uint32_t>& list, uint64_t capacity) {
    CHECK(list.size() <= L.hot_max);
    const std::set<uint32_t> s(list.begin(), list.end());
    CHECK(s.size() == list.size()); // no duplicates
    for (const uint32_t v : list) CHECK(v < capacity);
}

// both on the same notes: same answer, same list (order included)
static bool both(Maker& mk, Model& md, const Notes& n, uint32_t heavy_min, uint64_t capacity) {
    const bool a = mk.look(n, heavy_min, capacity), b = md.look(n, heavy_min, capacity);
    CHECK(a == b);
    CHECK(mk.made == md.made);
    check_list(mk.made, capacity);
    return a;
}

static uint32_t scratch_home(uint32_t slot) { return (slot * 0x9E3779B1u) >> (32 - L.scratch_bits); }

int main() {
    const uint64_t CAP = 3000000;
    // ---- a first list from 0, 1, 511, 512, 513 and 8 192 distinct slots (+ notes that do not count) ----
    for (const uint32_t distinct : {0u, 1u, 511u, 512u, 513u, 8192u}) {
        for (int rep = 0; rep < 3; ++rep) {
            Notes n;
            std::set<uint32_t> seen;
            const uint32_t heavy_min = 32;
            while (seen.size() < distinct) {
                const uint32_t slot = (uint32_t)(rnd() % CAP);
                if (!seen.insert(slot).second) continue;
                n.add(heavy_min + (uint32_t)(rnd() % (rep == 0 ? 5000 : 7)), slot); // (rep > 0: lengths tie all over, also across the cut)
            }
            // what must be ignored: runs below heavy_min, slots at or beyond the capacity; a second, shorter note of a slot
            for (uint32_t k = 0; k < 64 && n.used < L.notes; ++k) {
                if (k % 3 == 0) n.add(heavy_min - 1 - k % 20, (uint32_t)(rnd() % CAP));
                else if (k % 3 == 1) n.add(900000, (uint32_t)(CAP + k / 3 * 1000003ull));
                else if (!seen.empty()) n.add(heavy_min, *seen.begin());
            }
            n.shuffle();
            Maker mk;
            Model md;
            CHECK(both(mk, md, n, heavy_min, CAP) == (distinct != 0));
            CHECK(mk.made.size() == std::min(distinct, L.hot_max));
            for (const uint32_t s : mk.made) CHECK(seen.count(s));
            CHECK(!both(mk, md, n, heavy_min, CAP)); // the same notes again: the list is kept
            n.shuffle();                             // ... wherever they stand in the table
            CHECK(!both(mk, md, n, heavy_min, CAP));
        }
    }
    { // ties resolve by slot: 600 runs of one length -> the 512 smallest slots, ascending
        Notes n;
        for (uint32_t i = 0; i < 600; ++i) n.add(100, 5000 + 7 * ((i * 389u) % 600u));
        n.shuffle();
        Maker mk;
        Model md;
        CHECK(both(mk, md, n, 32, CAP));
        CHECK(mk.made.size() == 512);
        for (uint32_t i = 0; i < 512; ++i) CHECK(mk.made[i] == 5000 + 7 * i);
    }
    { // every note names the same slot: one entry, and its LONGEST run is what ranks it
        Notes n;
        for (uint32_t i = 0; i + 1 < L.notes; ++i) n.add(40 + (i * 2654435761u) % 8000u, 77);
        n.add(5000, 99);
        n.shuffle();
        Maker mk;
        Model md;
        CHECK(both(mk, md, n, 32, CAP));
        CHECK((mk.made == std::vector<uint32_t>{77, 99}));
        Notes one;
        for (uint32_t i = 0; i < L.notes; ++i) one.add(50, 123);
        Maker m2;
        Model d2;
        CHECK(both(m2, d2, one, 32, CAP) && m2.made == std::vector<uint32_t>{123});
    }
    { // slots that collide in the scratch hash: 700 with one home entry near the table's end (the probe sequence wraps around),
      // among 3 000 others
        const uint64_t cap = 0xFFFFFFFFull;
        const uint32_t home = (1u << L.scratch_bits) - 3u;
        Notes n;
        std::vector<uint32_t> col;
        for (uint32_t s = 1; col.size() < 700; ++s)
            if (scratch_home(s) == home) col.push_back(s);
        for (size_t i = 0; i < col.size(); ++i) n.add(40 + (uint32_t)(i % 300), col[i]), n.add(33, col[i]);
        for (uint32_t i = 0; i < 3000; ++i) n.add(32 + (uint32_t)(rnd() % 200), (uint32_t)rnd());
        n.shuffle();
        Maker mk;
        Model md;
        CHECK(both(mk, md, n, 32, cap));
        CHECK(mk.made.size() == 512);
        CHECK(!both(mk, md, n, 32, cap));
        // a slot whose home entry is taken by ANOTHER slot must not be mistaken for noted: the list = collided slots only, the
        // notes then lose 11 % of them -- their entries' neighbours are still there
        Notes a;
        for (size_t i = 0; i < 500; ++i) a.add(100, col[i]);
        Maker m2;
        Model d2;
        CHECK(both(m2, d2, a, 32, cap) && m2.made.size() == 500);
        Notes b;
        for (size_t i = 55; i < 500; ++i) b.add(100, col[i]);
        for (size_t i = 500; i < 555; ++i) b.add(100, col[i]);
        CHECK(both(m2, d2, b, 32, cap)); // 445 of 500 still noted: stale
    }
    { // the keep-or-remake rule, edge by edge: a list of 500 slots with runs of 100 .. 599
        const uint32_t heavy_min = 32;
        auto base = [&](uint32_t keep_from, uint32_t keep_to) {
            Notes n;
            for (uint32_t i = keep_from; i < keep_to; ++i) n.add(100 + i, 1000 + i);
            return n;
        };
        Maker mk;
        Model md;
        CHECK(both(mk, md, base(0, 500), heavy_min, CAP) && mk.made.size() == 500);
        const std::vector<uint32_t> first = mk.made;
        // exactly nine in ten still noted: kept; one fewer: made afresh
        CHECK(!both(mk, md, base(50, 500), heavy_min, CAP) && mk.made == first);
        CHECK(both(mk, md, base(51, 500), heavy_min, CAP) && mk.made.size() == 449);
        // the 51 come back: every slot of the list of 449 is noted, 500 slots are no crowd beside 449, no run is long -- kept
        CHECK(!both(mk, md, base(0, 500), heavy_min, CAP) && mk.made.size() == 449);
        CHECK(both(mk, md, Notes(), heavy_min, CAP) && mk.made.empty());
        CHECK(both(mk, md, base(0, 500), heavy_min, CAP) && mk.made == first);
        // other lengths, same slots: kept (which slots are hot is all that counts)
        {
            Notes n;
            for (uint32_t i = 0; i < 500; ++i) n.add(700 - i, 1000 + i);
            CHECK(!both(mk, md, n, heavy_min, CAP) && mk.made == first);
        }
        // a new slot with a run just below long_run: kept; of long_run: made afresh, the new slot first
        {
            Notes n = base(0, 500);
            n.add(L.long_run - 1, 9);
            CHECK(!both(mk, md, n, heavy_min, CAP) && mk.made == first);
            Notes m = base(0, 500);
            m.add(L.long_run, 9);
            CHECK(both(mk, md, m, heavy_min, CAP) && mk.made.size() == 501 && mk.made[0] == 9);
            CHECK(!both(mk, md, m, heavy_min, CAP));
        }
        // a crowd of new short runs: kept up to 5/4 of the list + 32, then made afresh
        {
            Maker m3;
            Model d3;
            Notes n;
            for (uint32_t i = 0; i < 40; ++i) n.add(200, 50 + i);
            CHECK(both(m3, d3, n, heavy_min, CAP));
            for (uint32_t i = 0; i < 42; ++i) n.add(40, 500 + i); // 82 * 4 = 328 = 40 * 5 + 128
            CHECK(!both(m3, d3, n, heavy_min, CAP) && m3.made.size() == 40);
            n.add(40, 900);
            CHECK(both(m3, d3, n, heavy_min, CAP) && m3.made.size() == 83);
        }
        // the stream stops being skewed: empty notes empty the list, once
        {
            Notes none;
            CHECK(both(mk, md, none, heavy_min, CAP) && mk.made.empty());
            CHECK(!both(mk, md, none, heavy_min, CAP) && mk.made.empty());
            Maker m4;
            Model d4;
            CHECK(!both(m4, d4, none, heavy_min, CAP)); // empty notes after an empty list: no change
            Notes low; // ... and notes that do not count are empty notes
            low.add(heavy_min - 1, 5), low.add(1000, (uint32_t)CAP);
            CHECK(!both(m4, d4, low, heavy_min, CAP) && m4.made.empty());
        }
    }
    { // a stream of looks: the hot set drifts, lengths jitter, now and then a very long run turns up or most of the set goes
        for (const uint32_t heavy_min : {2u, 32u, 200u}) {
            Maker mk;
            Model md;
            std::vector<uint32_t> pool;
            for (uint32_t i = 0; i < 900; ++i) pool.push_back((uint32_t)(rnd() % CAP));
            int changed = 0, kept = 0;
            uint32_t width = 400;
            for (int look = 0; look < 400; ++look) {
                width = std::min(880u, std::max(60u, width + (uint32_t)(rnd() % 41) - 20u)); // (how many slots are hot: a slow walk)
                if (look % 37 == 36)
                    for (uint32_t i = 0; i < 300; ++i) pool[rnd() % pool.size()] = (uint32_t)(rnd() % CAP);
                else
                    for (uint32_t i = 0; i < 5; ++i) pool[rnd() % pool.size()] = (uint32_t)(rnd() % (CAP + 50)); // (some beyond the capacity)
                Notes n;
                const uint32_t hot = look % 53 == 52 ? 0u : width;
                for (uint32_t i = 0; i < hot; ++i) {
                    // (a slot's run: its own length +- 20 -- the slots around heavy_min come and go -- and sometimes a very long one)
                    const uint32_t len = (rnd() % 97 == 0) ? L.long_run + (uint32_t)(rnd() % 3000) : (pool[i] * 2654435761u) % 560u + (uint32_t)(rnd() % 40);
                    n.add(len, pool[i]);
                    if (rnd() % 4 == 0) n.add((uint32_t)(rnd() % 600), pool[i]); // the device's second table
                }
                n.shuffle();
                (both(mk, md, n, heavy_min, CAP) ? changed : kept)++;
            }
            std::printf("heavy_min %u: %d looks made a list, %d kept it\n", heavy_min, changed, kept);
            CHECK(changed > 20 && kept > 20); // (the stream exercises both answers)
        }
    }
    std::printf("all tests passed\n");
    return 0;
}
