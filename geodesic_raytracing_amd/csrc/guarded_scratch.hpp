// guarded_scratch.hpp — the fenced device scratch of the file encoders (device_encoders.cpp), as arithmetic on the host: regions of 32-bit
// words in one allocation, GUARD_WORDS in front of every region and behind the last, everything filled with GUARD_PATTERN at creation.  What
// a kernel wrote outside the words its encoder counts as used shows as a word that no longer holds the pattern.  Host only (no HIP):
// tests/guarded_scratch_check.cpp includes this file alone.
#pragma once

#include <algorithm>
#include <cstddef>

namespace guarded_scratch {

const size_t GUARD_WORDS = 64;
const unsigned int GUARD_PATTERN = 0xa5c3e1f7u;
const int MAX_REGIONS = 4;

struct layout {
    int regions = 0;
    size_t at[MAX_REGIONS] = {}, words[MAX_REGIONS] = {}, total = 0;   // where a region starts, its size rounded up; the words in all
};

// `regions` regions of sizes[r] words, each rounded up to a multiple of `alignment` words (1: as it is)
inline layout lay_out(const size_t* sizes, int regions, size_t alignment) {
    layout l;
    l.regions = regions, l.total = GUARD_WORDS;
    for (int r = 0; r < regions; r++) {
        l.at[r] = l.total;
        l.words[r] = (sizes[r] + alignment - 1) / alignment * alignment;
        l.total += l.words[r] + GUARD_WORDS;
    }
    return l;
}

// The words that must still hold the pattern when the first used[r] words of region r may have been written: the first guard, then from
// behind each region's used words to the next region (or the end).  Writes regions + 1 spans [from, to) and returns that count.
struct span { size_t from, to; };
inline int unwritten_spans(const layout& l, const size_t* used, span out[MAX_REGIONS + 1]) {
    out[0] = {0, GUARD_WORDS};
    for (int r = 0; r < l.regions; r++) out[r + 1] = {l.at[r] + std::min(used[r], l.words[r]), r + 1 < l.regions ? l.at[r + 1] : l.total};
    return l.regions + 1;
}

inline bool holds_pattern(const unsigned int* words, size_t count) {
    return std::all_of(words, words + count, [](unsigned int word) { return word == GUARD_PATTERN; });
}

// the verdict on a host copy of all l.total words
inline bool intact(const layout& l, const unsigned int* words, const size_t* used) {
    span spans[MAX_REGIONS + 1];
    const int count = unwritten_spans(l, used, spans);
    return std::all_of(spans, spans + count, [&](const span& s) { return holds_pattern(words + s.from, s.to - s.from); });
}

}  // namespace guarded_scratch
