// guarded_scratch_check.cpp — csrc/guarded_scratch.hpp on its own (tests/test_guarded_scratch.py compiles this with the host compiler and
// the address and undefined-behaviour sanitizers; no HIP).  The expected layouts are the encoders' as they computed them before the header
// existed, restated here: gr_png_encoder_create (one region of the stream's capacity, no rounding, scratch = capacity + 128 words, the
// stream at word 64) and gr_jpeg_encoder_create (four regions, each rounded up to 4 words, the file's size in the last two words of
// region 2).  Prints "ok" last; any difference ends it with a message and status 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../geodesic_raytracing_amd/csrc/guarded_scratch.hpp"

namespace gs = guarded_scratch;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("line %d: %s does not hold\n", __LINE__, #cond);         \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

// the JPEG encoder's region sizes in words for a frame (jpeg_stream.hpp's arithmetic, written out)
static void jpeg_sizes(size_t width, size_t height, size_t words[4]) {
    const size_t rows = (height + 15) / 16, across = (width + 15) / 16;
    const size_t block_bits = 9 + 11 + 63 * (16 + 10), header_bytes = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14;
    const size_t row_bytes_bound = (across * 6 * block_bits + 7) / 8, slot_bytes = (row_bytes_bound + 15) / 16 * 16;
    const size_t file_bound = header_bytes + rows * (2 * row_bytes_bound + 2);
    words[0] = rows * across * 6 * 32;
    words[1] = rows * (slot_bytes / 4);
    words[2] = 2 * rows + 2;
    words[3] = (file_bound + 3) / 4;
}

// every verdict the encoders ask for, on a host copy: intact as filled; one wrong word in a guard, right behind `used` or at the tail's end
// flips it; a wrong word inside the used span does not
static void check_verdicts(const gs::layout& l, const size_t* used, int region_with_tail) {
    std::vector<unsigned int> words(l.total, gs::GUARD_PATTERN);
    EXPECT(gs::intact(l, words.data(), used));
    const size_t tail_from = l.at[region_with_tail] + used[region_with_tail], tail_to = l.at[region_with_tail] + l.words[region_with_tail];
    std::vector<size_t> guarded = {0, gs::GUARD_WORDS - 1, l.total - gs::GUARD_WORDS, l.total - 1};   // the first guard's ends, the last guard's
    for (int r = 1; r < l.regions; r++) {   // the middle guards' ends
        guarded.push_back(l.at[r] - gs::GUARD_WORDS);
        guarded.push_back(l.at[r] - 1);
    }
    if (tail_from < tail_to) {   // the first word behind "used", the last word of the tail
        guarded.push_back(tail_from);
        guarded.push_back(tail_to - 1);
    }
    for (size_t i : guarded) {
        words[i] ^= 1u;
        EXPECT(!gs::intact(l, words.data(), used));
        words[i] = gs::GUARD_PATTERN;
    }
    for (int r = 0; r < l.regions; r++) {
        if (!used[r]) continue;
        for (size_t i : {l.at[r], l.at[r] + used[r] - 1}) {
            words[i] = 0;
            EXPECT(gs::intact(l, words.data(), used));
            words[i] = gs::GUARD_PATTERN;
        }
    }
    // the spans, downloaded one by one as the device side does, give the same verdict
    gs::span spans[gs::MAX_REGIONS + 1];
    EXPECT(gs::unwritten_spans(l, used, spans) == l.regions + 1);
    words[l.total - 1] = 0;
    bool all = true;
    for (int s = 0; s <= l.regions; s++) all = all && gs::holds_pattern(words.data() + spans[s].from, spans[s].to - spans[s].from);
    EXPECT(!all);
}

int main() {
    EXPECT(gs::GUARD_WORDS == 64 && gs::GUARD_PATTERN == 0xa5c3e1f7u);
    // PNG: scratch_words = stream_capacity_words + 2 * GUARD_WORDS, the stream at scratch + GUARD_WORDS
    for (size_t capacity : {(size_t)1, (size_t)3, (size_t)4}) {
        const gs::layout l = gs::lay_out(&capacity, 1, 1);
        EXPECT(l.regions == 1 && l.at[0] == 64 && l.words[0] == capacity && l.total == capacity + 128);
        for (size_t used = 0; used <= capacity; used++) check_verdicts(l, &used, 0);
        printf("png %zu words: %zu in all\n", capacity, l.total);
    }
    // JPEG: at = GUARD_WORDS; per region: region_at = at, region_words = (words + 3) / 4 * 4, at += region_words + GUARD_WORDS; scratch_words = at
    const size_t sizes[4][2] = {{1, 1}, {16, 16}, {17, 33}, {1025, 31}};
    for (auto& size : sizes) {
        size_t words[4];
        jpeg_sizes(size[0], size[1], words);
        const gs::layout l = gs::lay_out(words, 4, 4);
        size_t at = 64;
        EXPECT(l.regions == 4);
        for (int r = 0; r < 4; r++) {
            EXPECT(l.at[r] == at && l.words[r] == (words[r] + 3) / 4 * 4 && l.at[r] % 4 == 0);
            at += (words[r] + 3) / 4 * 4 + 64;
        }
        EXPECT(l.total == at);
        EXPECT((l.at[2] + l.words[2] - 2) * 4 % 8 == 0);   // the size word's byte offset
        EXPECT(l.at[2] + l.words[2] - 2 >= l.at[2] + words[2] - 2);   // ... behind the rows' counts
        // the verdict the encoder asks for: three regions written whole, the file region up to the longest file so far (629 header bytes first)
        for (size_t file_bytes : {(size_t)629, (size_t)630, (size_t)632, words[3] * 4 - 3, words[3] * 4}) {
            const size_t used[4] = {l.words[0], l.words[1], l.words[2], (file_bytes + 3) / 4};
            check_verdicts(l, used, 3);
        }
        printf("jpeg %zux%zu: regions at %zu %zu %zu %zu, %zu words in all\n", size[0], size[1], l.at[0], l.at[1], l.at[2], l.at[3], l.total);
    }
    {   // 1 x 1 by hand: 192, 312, 4 and 780 words
        size_t words[4];
        jpeg_sizes(1, 1, words);
        EXPECT(words[0] == 192 && words[1] == 312 && words[2] == 4 && words[3] == 780);
        const gs::layout l = gs::lay_out(words, 4, 4);
        EXPECT(l.at[0] == 64 && l.at[1] == 320 && l.at[2] == 696 && l.at[3] == 764 && l.total == 1608);
    }
    printf("ok\n");
    return 0;
}
