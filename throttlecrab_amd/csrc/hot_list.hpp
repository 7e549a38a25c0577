// hot_list.hpp -- WHICH slots make the hot list (range_part.hpp): the selection of slots.hip's hot_make over plain arrays and
// vectors, so that it runs without an engine (tests/cpp/test_hot_list.cpp).  Host code only, nothing from HIP in here.
//
// The evaluations note every run of at least heavy_min requests: length << 44 | tag << 32 | slot, in a table of `notes` words
// (ev::heavy_note; a slot may be noted twice, an empty word is 0).  Three steps: one note per slot (the longest run), the
// hot_max longest of them (ties: the smaller slot first), and the keep-or-remake rule against the list as last made.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace hl {

struct Limits {
    uint32_t notes;        // words of the note table (ev::HEAVY_SLOTS)
    uint32_t scratch_bits; // the scratch hash holds 1 << scratch_bits entries: twice the notes
    uint32_t hot_max;      // slots a list holds (rp::HOT_MAX)
    uint32_t long_run;     // a run this long endangers a range: its slot must be on the list (rs::FIN_CAP / 4)
};
constexpr Limits ENGINE = {8192u, 14u, 512u, 1024u}; // (slots.hip checks these against the kernels' constants)

// -> true: the list changed (`made` is the new one, heaviest first); false: `made` still serves and is left as it was
// scratch, found: workspace that keeps its memory between calls
inline bool make_list(const volatile unsigned long long* notes, const Limits& lim, uint32_t heavy_min, uint64_t capacity,
                      std::vector<unsigned long long>& scratch, std::vector<unsigned long long>& found, std::vector<uint32_t>& made) {
    // one note per slot (the longest run), through a scratch hash: 8 192 notes at most, no sort of them all (a first version
    // sorted the notes twice and cost the pipeline 0.3 ms every 8th batch)
    const uint32_t SCR = 1u << lim.scratch_bits;
    if (scratch.size() != SCR) scratch.assign(SCR, 0ull);
    else std::fill(scratch.begin(), scratch.end(), 0ull);
    auto probe = [&](uint32_t slot) -> unsigned long long& { // entry: (slot + 1) << 32 | length
        uint32_t at = (slot * 0x9E3779B1u) >> (32 - lim.scratch_bits);
        while (scratch[at] != 0ull && (uint32_t)(scratch[at] >> 32) != slot + 1u) at = (at + 1u) & (SCR - 1u);
        return scratch[at];
    };
    // length << 32 | ~slot: descending = longest first, then by slot
    found.clear();
    for (uint32_t i = 0; i < lim.notes; ++i) {
        const unsigned long long v = notes[i];
        const uint32_t len = (uint32_t)(v >> 44), slot = (uint32_t)v;
        if (len < heavy_min || slot >= capacity) continue;
        unsigned long long& en = probe(slot);
        if ((uint32_t)en < len) en = ((unsigned long long)(slot + 1u) << 32) | len;
    }
    for (const unsigned long long en : scratch)
        if (en) found.push_back(((unsigned long long)(uint32_t)en << 32) | (0xFFFFFFFFu - ((uint32_t)(en >> 32) - 1u)));
    if (found.size() > lim.hot_max) {
        std::nth_element(found.begin(), found.begin() + lim.hot_max, found.end(), std::greater<unsigned long long>());
        found.resize(lim.hot_max);
    }
    std::sort(found.begin(), found.end(), std::greater<unsigned long long>());
    std::vector<uint32_t> now(found.size());
    for (size_t i = 0; i < found.size(); ++i) now[i] = 0xFFFFFFFFu - (uint32_t)found[i];
    // Keep the installed tables while the list still serves: nine in ten of its slots are still noted (else it is stale: made
    // afresh, so that the table does not fill with slots that stopped being hot), and no slot with a run long enough to endanger a
    // range (a quarter of what a block finishes) is missing from it.  Which slots are hot is all that counts -- the rank form
    // does not care about their order -- and the tail of a skewed stream's list changes with every look (slots around heavy_min
    // requests per batch come and go; in round 6's first version so did the boundary between the 64th and the 65th heaviest,
    // and every change cost six installs and the hints about the ranges).
    bool same = !made.empty();
    if (same) {
        std::vector<uint32_t> cur(made);
        std::sort(cur.begin(), cur.end());
        for (size_t i = 0; i < found.size() && same; ++i) {
            const uint32_t len = (uint32_t)(found[i] >> 32), sl = 0xFFFFFFFFu - (uint32_t)found[i];
            if (len < lim.long_run) break; // (sorted by length, longest first)
            same = std::binary_search(cur.begin(), cur.end(), sl);
        }
        size_t both = 0;
        for (const uint32_t sl : made) both += probe(sl) != 0ull ? 1u : 0u; // (noted at all: on the new list or just below its cut)
        same = same && both * 10u >= made.size() * 9u && now.size() * 4u <= made.size() * 5u + 128u; // (... nor has a crowd of new hot slots turned up)
    }
    if (now.empty() && made.empty()) same = true;
    if (same) return false;
    made.swap(now);
    return true;
}

} // namespace hl
