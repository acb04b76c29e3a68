// png_stream.cpp — the PNG stream of both PNG encoders (png_stream.hpp; geodesic_hip_internal.h, "PNG frames"): table, header, sizes,
// container, and the host encoder that defines the bytes.  No HIP header.
#include "png_stream.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <queue>

#include "internal.hpp"

namespace png_stream {

// ---------------------------------------------------------------------------------------------------------------- code lengths

void limited_lengths(const uint64_t* count, int symbols, int max_length, uint8_t* length) {
    std::fill(length, length + symbols, (uint8_t)0);
    std::vector<int> leaves;
    for (int s = 0; s < symbols; s++)
        if (count[s]) leaves.push_back(s);
    for (int s = 0; s < symbols && leaves.size() < 2; s++)   // a code of one leaf has no bits to read: a second leaf that never occurs
        if (!count[s]) leaves.push_back(s);
    std::sort(leaves.begin(), leaves.end());
    const int n = (int)leaves.size();
    if (n < 2) return;   // (an alphabet of one symbol: nothing to code)
    // Huffman's tree: the two lightest nodes joined until one is left; ties go to the node made first, leaves in symbol order before all
    struct node { uint64_t weight; int id; };
    auto heavier = [](const node& a, const node& b) { return a.weight != b.weight ? a.weight > b.weight : a.id > b.id; };
    std::priority_queue<node, std::vector<node>, decltype(heavier)> heap(heavier);
    std::vector<int> parent(2 * n - 1, -1);
    for (int i = 0; i < n; i++) heap.push({count[leaves[i]], i});
    for (int made = n; made < 2 * n - 1; made++) {
        const node a = heap.top(); heap.pop();
        const node b = heap.top(); heap.pop();
        parent[a.id] = parent[b.id] = made;
        heap.push({a.weight + b.weight, made});
    }
    // leaves per depth, everything deeper than max_length moved up to it
    std::vector<int> of_length(std::max(max_length, 2 * n) + 1, 0);
    for (int i = 0; i < n; i++) {
        int depth = 0;
        for (int at = i; parent[at] >= 0; at = parent[at]) depth++;
        of_length[std::min(depth, max_length)]++;
    }
    // ... which oversubscribes the code: Kraft's sum in units of 2^-max_length, brought back to exactly 1 by taking one leaf from the
    // deepest level, and making a leaf of the deepest level above that still has one into an inner node with two leaves below it
    uint64_t total = 0;
    for (int l = 1; l <= max_length; l++) total += (uint64_t)of_length[l] << (max_length - l);
    while (total > (1ull << max_length)) {
        of_length[max_length]--;
        for (int l = max_length - 1; l >= 1; l--)
            if (of_length[l]) {
                of_length[l]--;
                of_length[l + 1] += 2;
                break;
            }
        total--;
    }
    // the shortest codes to the commonest symbols (ties: the lower symbol first)
    std::vector<int> by_count(leaves);
    std::stable_sort(by_count.begin(), by_count.end(), [&](int a, int b) { return count[a] > count[b]; });
    int at = 0;
    for (int l = 1; l <= max_length; l++)
        for (int k = 0; k < of_length[l]; k++) length[by_count[at++]] = (uint8_t)l;
}

void canonical_codes(const uint8_t* length, int symbols, uint16_t* code) {
    unsigned of_length[MAX_LENGTH + 2] = {}, next[MAX_LENGTH + 2] = {};
    for (int s = 0; s < symbols; s++) of_length[length[s]]++;
    of_length[0] = 0;
    for (int l = 1; l <= MAX_LENGTH; l++) next[l] = (next[l - 1] + of_length[l - 1]) << 1;
    for (int s = 0; s < symbols; s++) {
        code[s] = 0;
        if (!length[s]) continue;
        const unsigned forward = next[length[s]]++;
        unsigned reversed = 0;
        for (int b = 0; b < length[s]; b++) reversed |= ((forward >> b) & 1u) << (length[s] - 1 - b);
        code[s] = (uint16_t)reversed;
    }
}

namespace {
// bits from bit 0 of word 0 up
struct bit_string {
    uint32_t* words;
    int bits = 0;
    void put(uint32_t value, int count) {
        for (int b = 0; b < count; b++, bits++)
            if ((value >> b) & 1u) words[bits >> 5] |= 1u << (bits & 31);
    }
};
}   // namespace

void build_table(const uint64_t* histogram, int stream_kind, table& out) {
    const int symbols = symbols_of(stream_kind), distances = stream_kind == GR_PNG_STREAM_RUNS ? 4 : 1;
    uint64_t count[MAX_SYMBOLS];
    std::copy(histogram, histogram + symbols, count);
    if (!count[END_OF_BLOCK]) count[END_OF_BLOCK] = 1;
    out.symbols = symbols;
    std::fill(out.length, out.length + MAX_SYMBOLS, (uint8_t)0);
    std::fill(out.code, out.code + MAX_SYMBOLS, (uint16_t)0);
    limited_lengths(count, symbols, MAX_LENGTH, out.length);
    canonical_codes(out.length, symbols, out.code);
    // the code lengths as deflate sends them: the literal/length lengths and the distance lengths - literals: one, 0, no distance code at
    // all, which is what RFC 1951 3.2.7 gives a block of literals only; runs: 0 0 0 1, the one distance code of one bit that the same
    // paragraph allows, whether the frame has a match or not - run-length coded as one sequence (16: the last length 3 ... 6 more times;
    // 17, 18: 3 ... 10 and 11 ... 138 zeros)
    uint8_t sent[MAX_SYMBOLS + 4];
    const int sent_count = symbols + distances;
    std::copy(out.length, out.length + symbols, sent);
    std::fill(sent + symbols, sent + sent_count, (uint8_t)0);
    if (stream_kind == GR_PNG_STREAM_RUNS) sent[sent_count - 1] = 1;
    struct item { uint8_t symbol, extra_bits, extra; };
    std::vector<item> items;
    for (int i = 0; i < sent_count;) {
        int run = 1;
        while (i + run < sent_count && sent[i + run] == sent[i]) run++;
        const uint8_t v = sent[i];
        i += run;
        if (v == 0) {
            while (run >= 11) { const int n = std::min(run, 138); items.push_back({18, 7, (uint8_t)(n - 11)}); run -= n; }
            if (run >= 3) { items.push_back({17, 3, (uint8_t)(run - 3)}); run = 0; }
        } else {
            items.push_back({v, 0, 0});
            run--;
            while (run >= 3) { const int n = std::min(run, 6); items.push_back({16, 2, (uint8_t)(n - 3)}); run -= n; }
        }
        for (; run > 0; run--) items.push_back({v, 0, 0});
    }
    uint64_t used[19] = {};
    for (auto& it : items) used[it.symbol]++;
    uint8_t length_of[19];
    uint16_t code_of[19];
    limited_lengths(used, 19, MAX_LENGTH_OF_LENGTHS, length_of);
    canonical_codes(length_of, 19, code_of);
    static const int ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int sent_lengths = 19;
    while (sent_lengths > 4 && !length_of[ORDER[sent_lengths - 1]]) sent_lengths--;
    std::fill(out.header, out.header + HEADER_WORDS, 0u);
    bit_string h{out.header};
    h.put(0, 1);                    // BFINAL: the stream ends with a block of its own
    h.put(2, 2);                    // BTYPE: dynamic Huffman
    h.put((uint32_t)symbols - 257, 5);     // HLIT
    h.put((uint32_t)distances - 1, 5);     // HDIST
    h.put((uint32_t)sent_lengths - 4, 4);
    for (int i = 0; i < sent_lengths; i++) h.put(length_of[ORDER[i]], 3);
    for (auto& it : items) {
        h.put(code_of[it.symbol], length_of[it.symbol]);
        h.put(it.extra, it.extra_bits);
    }
    out.header_bits = h.bits;
}

// ---------------------------------------------------------------------------------------------------------------- sizes

uint64_t row_block_bits(const table& t, int row, const uint32_t* row_histogram) {
    uint64_t bits = (uint64_t)t.header_bits + t.length[filter_of_row(row)] + t.length[END_OF_BLOCK];
    for (int v = 0; v < 256; v++) bits += (uint64_t)t.length[v] * row_histogram[v];
    for (int s = FIRST_LENGTH_SYMBOL; s < t.symbols; s++) bits += (uint64_t)(t.length[s] + extra_bits_of(s) + 1) * row_histogram[s];
    return bits;
}

void tokenise_row(const uint8_t* filtered, int width, int stream_kind, int* run) {
    std::fill(run, run + width, 0);
    if (stream_kind != GR_PNG_STREAM_RUNS) return;
    for (int x = 1; x < width;) {
        if (memcmp(filtered + 4 * (size_t)x, filtered + 4 * (size_t)(x - 1), 4) != 0) { x++; continue; }
        // a maximal run of repeats that ends with its group of GROUP_PIXELS at the latest
        const int end_of_group = std::min(width, (x / GROUP_PIXELS + 1) * GROUP_PIXELS);
        int r = 1;
        while (x + r < end_of_group && memcmp(filtered + 4 * (size_t)(x + r), filtered + 4 * (size_t)(x + r - 1), 4) == 0) r++;
        run[x] = r;
        std::fill(run + x + 1, run + x + r, -1);
        x += r;
    }
}

namespace {
uint64_t idat_chunks(uint64_t stream_bytes, uint64_t max_idat) { return (stream_bytes + max_idat - 1) / max_idat; }
}   // namespace

uint64_t file_bytes(uint64_t rows_bytes, uint64_t max_idat) {
    const uint64_t stream = zlib_bytes(rows_bytes);
    return 8 + 25 + 12 * idat_chunks(stream, max_idat) + stream + 12;
}

uint64_t rows_bound(int width, int height) {
    if (width < 1 || height < 1 || 4ull * (uint64_t)width * (uint64_t)height > MAX_RAW_BYTES) return 0;
    const uint64_t block_bits = HEADER_MAX_BITS + (uint64_t)MAX_LENGTH * (4ull * (uint64_t)width + 2);
    return (uint64_t)height * row_segment_bytes(block_bits);
}

uint32_t row_adler(int row, int width, uint32_t sum, uint32_t weighted) {
    const uint64_t M = 65521, n = 4ull * (uint64_t)width + 1, f = (uint64_t)filter_of_row(row);
    const uint64_t s1 = (1 + f + sum) % M, s2 = (n % M + (n % M) * f + weighted) % M;
    return (uint32_t)((s2 << 16) | s1);
}

uint32_t join_adler(const uint32_t* row_adlers, int width, int height) {
    uLong adler = 1;
    const z_off_t n = (z_off_t)(4ll * width + 1);
    for (int r = 0; r < height; r++) adler = adler32_combine(adler, row_adlers[r], n);
    return (uint32_t)adler;
}

// ---------------------------------------------------------------------------------------------------------------- container

namespace {
void put_be32(uint8_t* at, uint32_t v) {
    at[0] = (uint8_t)(v >> 24);
    at[1] = (uint8_t)(v >> 16);
    at[2] = (uint8_t)(v >> 8);
    at[3] = (uint8_t)v;
}
uLong crc_of(uLong crc, const uint8_t* data, uint64_t bytes) {
    while (bytes) {   // (zlib counts in 32 bits)
        const uint64_t n = std::min<uint64_t>(bytes, 1u << 30);
        crc = crc32(crc, data, (uInt)n);
        data += n;
        bytes -= n;
    }
    return crc;
}
}   // namespace

void write_container(uint8_t* out, int width, int height, const uint8_t* rows, uint64_t rows_bytes, uint32_t adler, uint64_t max_idat) {
    static const uint8_t SIGNATURE[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    memcpy(out, SIGNATURE, 8);
    uint8_t* at = out + 8;
    put_be32(at, 13);
    memcpy(at + 4, "IHDR", 4);
    put_be32(at + 8, (uint32_t)width);
    put_be32(at + 12, (uint32_t)height);
    at[16] = 8;   // bit depth
    at[17] = 6;   // colour type: RGBA
    at[18] = at[19] = at[20] = 0;   // deflate, adaptive filtering, no interlace
    put_be32(at + 21, (uint32_t)crc32(0, at + 4, 17));
    at += 25;
    // the zlib stream is three pieces - two bytes, the rows' segments, six bytes - cut into IDAT chunks wherever max_idat falls
    uint8_t front[2] = {0x78, 0x01}, back[6] = {0x03, 0x00};
    put_be32(back + 2, adler);
    const uint8_t* piece[3] = {front, rows, back};
    uint64_t left[3] = {2, rows_bytes, 6};
    int current = 0;
    for (uint64_t stream = zlib_bytes(rows_bytes); stream;) {
        const uint64_t data = std::min(stream, max_idat);
        put_be32(at, (uint32_t)data);
        memcpy(at + 4, "IDAT", 4);
        uLong crc = crc32(0, at + 4, 4);
        at += 8;
        for (uint64_t need = data; need;) {
            while (!left[current]) current++;
            const uint64_t n = std::min(need, left[current]);
            memcpy(at, piece[current], n);
            crc = crc_of(crc, at, n);
            at += n;
            piece[current] += n;
            left[current] -= n;
            need -= n;
        }
        put_be32(at, (uint32_t)crc);
        at += 4;
        stream -= data;
    }
    put_be32(at, 0);
    memcpy(at + 4, "IEND", 4);
    put_be32(at + 8, (uint32_t)crc32(0, at + 4, 4));
}

std::string refusal(const void* rgba8, int width, int height, const void* out_file, size_t capacity, const void* out_bytes, bool* too_small) {
    *too_small = false;
    if (!rgba8 || !out_file || !out_bytes) return "a required pointer is NULL";
    if (width < 1 || height < 1) return "a size below 1";
    if ((uintptr_t)rgba8 % 4) return "the frame is not aligned to 4 bytes";
    if (4ull * (uint64_t)width * (uint64_t)height > MAX_RAW_BYTES) return "a frame of more than 2^31 - 1 raw bytes";
    const uint64_t need = file_bytes(rows_bound(width, height));
    if ((uint64_t)capacity < need) {
        *too_small = true;
        return "a capacity of " + std::to_string(capacity) + " bytes, " + std::to_string(need) + " needed (gr_png_encode_bound)";
    }
    return "";
}

}  // namespace png_stream

// ---------------------------------------------------------------------------------------------------------------- exports

namespace ps = png_stream;

using gr_internal::refuse;

namespace {
// the filtered pixel bytes of one row (4 * width; the filter-type byte is not among them): Sub with bpp = 4 for row 0, Up for the others
void filter_row(const unsigned char* rgba8, int width, int row, uint8_t* out) {
    const size_t n = 4 * (size_t)width;
    const unsigned char* here = rgba8 + (size_t)row * n;
    if (row == 0)
        for (size_t i = 0; i < n; i++) out[i] = (uint8_t)(here[i] - (i >= 4 ? here[i - 4] : 0));
    else
        for (size_t i = 0; i < n; i++) out[i] = (uint8_t)(here[i] - here[i - n]);
}
}   // namespace

extern "C" {

int gr_png_encode_bound(int width, int height, size_t* bytes) {
    const char* who = "gr_png_encode_bound";
    if (!bytes) return refuse(who, "a required pointer is NULL", false);
    if (width < 1 || height < 1) return refuse(who, "a size below 1", false);
    const uint64_t rows = ps::rows_bound(width, height);
    if (!rows) return refuse(who, "a frame of more than 2^31 - 1 raw bytes", false);
    *bytes = (size_t)ps::file_bytes(rows);
    return GR_OK;
}

}   // extern "C"

namespace {
int build_table_of(const char* who, const unsigned long long* histogram, int stream_kind, unsigned char* lengths, unsigned short* codes,
                   unsigned int* header_words, int* header_bits) {
    if (!histogram || !lengths || !codes || !header_words || !header_bits) return refuse(who, "a required pointer is NULL", false);
    if (!ps::known_kind(stream_kind)) return refuse(who, "an unknown stream kind " + std::to_string(stream_kind), false);
    const int symbols = ps::symbols_of(stream_kind);
    uint64_t h[ps::MAX_SYMBOLS];
    std::copy(histogram, histogram + symbols, h);
    ps::table t;
    ps::build_table(h, stream_kind, t);
    std::copy(t.length, t.length + symbols, lengths);
    std::copy(t.code, t.code + symbols, codes);
    std::copy(t.header, t.header + ps::HEADER_WORDS, header_words);
    *header_bits = t.header_bits;
    return GR_OK;
}

// the host encoder of both kinds: a row is its tokens - a pixel is four literals, the head of a match or nothing (literals stream: always
// four literals) - and everything else is shared
int encode_host(const char* who, const unsigned char* rgba8, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes,
                int stream_kind) {
    bool too_small = false;
    const std::string wrong = ps::refusal(rgba8, width, height, out_file, capacity, out_bytes, &too_small);
    if (!wrong.empty()) return refuse(who, wrong, too_small);
    if (!ps::known_kind(stream_kind)) return refuse(who, "an unknown stream kind " + std::to_string(stream_kind), false);
    const size_t n = 4 * (size_t)width, bins = (size_t)ps::row_bins_of(stream_kind);
    std::vector<uint8_t> filtered(n);
    std::vector<int> run(width);
    // first pass: the rows' histograms - the frame's is their sum plus the filter-type bytes and one end-of-block a row
    std::vector<uint32_t> row_histogram((size_t)height * bins, 0u);
    uint64_t histogram[ps::MAX_SYMBOLS] = {};
    for (int r = 0; r < height; r++) {
        filter_row(rgba8, width, r, filtered.data());
        ps::tokenise_row(filtered.data(), width, stream_kind, run.data());
        uint32_t* mine = &row_histogram[(size_t)r * bins];
        for (int x = 0; x < width; x++) {
            if (run[x] > 0) mine[ps::length_code_of(run[x]).symbol]++;
            if (run[x] == 0)
                for (int c = 0; c < 4; c++) mine[filtered[4 * (size_t)x + c]]++;
        }
        for (size_t v = 0; v < bins; v++) histogram[v] += mine[v];
        histogram[ps::filter_of_row(r)]++;
    }
    histogram[ps::END_OF_BLOCK] = (uint64_t)height;
    ps::table t;
    ps::build_table(histogram, stream_kind, t);
    // the sizes, before a bit is packed
    std::vector<uint64_t> offset((size_t)height + 1, 0);
    for (int r = 0; r < height; r++) offset[r + 1] = offset[r] + ps::row_segment_bytes(ps::row_block_bits(t, r, &row_histogram[(size_t)r * bins]));
    const uint64_t rows_bytes = offset[height];
    // second pass: the segments, each from a byte boundary, and the rows' Adler-32 values
    std::vector<uint8_t> rows(rows_bytes, 0);
    std::vector<uint32_t> adlers(height);
    for (int r = 0; r < height; r++) {
        filter_row(rgba8, width, r, filtered.data());
        ps::tokenise_row(filtered.data(), width, stream_kind, run.data());
        uint8_t* segment = rows.data() + offset[r];
        uint64_t at = 0;   // in bits
        auto put = [&](uint32_t value, int count) {
            for (int b = 0; b < count; b++, at++)
                if ((value >> b) & 1u) segment[at >> 3] |= (uint8_t)(1u << (at & 7));
        };
        for (int b = 0; b < t.header_bits; b += 32) put(t.header[b >> 5], std::min(32, t.header_bits - b));
        const int f = ps::filter_of_row(r);
        put(t.code[f], t.length[f]);
        for (int x = 0; x < width; x++) {
            if (run[x] > 0) {
                const ps::length_code l = ps::length_code_of(run[x]);
                put(t.code[l.symbol], t.length[l.symbol]);
                put((uint32_t)l.extra, l.extra_bits);
                put(0, 1);   // distance code 3, the only one: distance 4
            }
            if (run[x] == 0)
                for (int c = 0; c < 4; c++) put(t.code[filtered[4 * (size_t)x + c]], t.length[filtered[4 * (size_t)x + c]]);
        }
        put(t.code[ps::END_OF_BLOCK], t.length[ps::END_OF_BLOCK]);
        put(0, 3);                          // an empty stored block, not the last: BFINAL = 0, BTYPE = 0
        at = (at + 7) / 8 * 8;              // ... whose length field starts at a byte
        put(0xffff0000u, 32);               // LEN = 0, NLEN = 0xffff
        if (at / 8 != offset[r + 1] - offset[r]) return refuse(who, "a row's segment is not the size computed for it", false);
        const uint8_t type = (uint8_t)f;
        uLong a = adler32(1, &type, 1);
        for (size_t done = 0; done < n;) {
            const size_t piece = std::min<size_t>(n - done, 1u << 30);
            a = adler32(a, filtered.data() + done, (uInt)piece);
            done += piece;
        }
        adlers[r] = (uint32_t)a;
    }
    ps::write_container(out_file, width, height, rows.data(), rows_bytes, ps::join_adler(adlers.data(), width, height));
    *out_bytes = (size_t)ps::file_bytes(rows_bytes);
    return GR_OK;
}
}   // namespace

extern "C" {

int gr_png_build_table(const unsigned long long* histogram, unsigned char* lengths, unsigned short* codes, unsigned int* header_words, int* header_bits) {
    return build_table_of("gr_png_build_table", histogram, GR_PNG_STREAM_LITERALS, lengths, codes, header_words, header_bits);
}

int gr_png_build_table_as(const unsigned long long* histogram, int stream_kind, unsigned char* lengths, unsigned short* codes, unsigned int* header_words,
                          int* header_bits) {
    return build_table_of("gr_png_build_table_as", histogram, stream_kind, lengths, codes, header_words, header_bits);
}

int gr_png_encode_rgba8_host(const unsigned char* rgba8, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    return encode_host("gr_png_encode_rgba8_host", rgba8, width, height, out_file, capacity, out_bytes, GR_PNG_STREAM_LITERALS);
}

int gr_png_encode_rgba8_host_as(const unsigned char* rgba8, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes,
                                int stream_kind) {
    return encode_host("gr_png_encode_rgba8_host_as", rgba8, width, height, out_file, capacity, out_bytes, stream_kind);
}

}   // extern "C"
