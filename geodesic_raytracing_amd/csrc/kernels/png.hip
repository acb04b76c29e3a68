// ------------------------------------------------------------------------------------------------
// png.hip - the device half of the PNG encoder (geodesic_hip_internal.h, "PNG frames"; the host half and the definition of the bytes:
// csrc/png_stream.cpp).  Part of the set-up module (capi.cpp: compile_setup_module); integers only.  Two launches over an RGBA8 frame
// that is already on the device, one workgroup of 256 lanes (64 x 4, the shape of kernels/present.hip) per image row in both:
//
// gr_png_histogram - what the host needs to build the frame's table and place the rows.  A lane filters a pixel on the fly - one 32-bit
// load for the pixel, one for the pixel above it (row 0: the pixel to its left; Sub with bpp = 4), a byte-wise difference in one register -
// and counts its four bytes in the workgroup's 256 bins in LDS (ds_add).  At the end of the row the bins are stored as the row's own
// histogram (the host computes the row's bit count from it: sum of length x count) and added to the frame's 256 bins with vector atomics,
// bins of 0 left out.  Beside that the lane sums what the row's Adler-32 is made of: sum of b and sum of (n - i) b over its bytes (n = 4
// width + 1 bytes a row with the filter byte, i the byte's position), the weight reduced mod 65521 first so that a term fits 32 bits;
// both are reduced mod 65521 per lane, summed over the wave by shuffles and over the four waves through LDS.  The filter-type bytes and
// the end-of-block symbols are not counted here: the host adds them, it knows them without looking.
//
// gr_png_pack - the bits.  Per pass a lane owns one item of at most 60 bits: in the first pass a 32-bit word of the block header (the same
// bits for every row; the lane behind the last word owns the filter byte's code), in the passes over the row a pixel - its four literals'
// codes, looked up in a copy of the table in LDS, concatenated in a 64-bit register -, in the last pass lane 0 owns end-of-block, the three
// bits of the empty stored block, the zero bits up to the byte boundary and 00 00 FF FF.  An inclusive scan of the bit counts over the wave
// (shuffles) and the four waves' totals through LDS place every item; the lanes OR their bits into a buffer of 32-bit words in LDS
// (ds_or: up to three words an item), whole words are flushed with coalesced 32-bit stores - lane t stores words t and t + 256 - and the
// bits of the last, partial word are carried into word 0 of the next pass.
// Segment ends: segments meet at byte boundaries, so the 32-bit word that holds a segment's first byte or its last one may hold a neighbour
// row's bytes too.  CHOSEN HERE: an atomic OR into a stream that the launcher zeroes on the same stream in front of this launch - the
// workgroup's buffer starts at the word that holds the segment's first byte, with the neighbour's bits in it left 0, and a word is stored
// with atomicOr when it is the segment's first or its last word and with a plain store otherwise (a word that is neither lies inside the
// segment whole).  No store goes past stream_word_count, whatever the offsets say.
//
// Both kernels are instances of one template over the stream kind: gr_png_histogram and gr_png_pack are kind 0 (literals only),
// gr_png_histogram_runs and gr_png_pack_runs kind 1 (previous-pixel run matches; the header states the stream).  What kind 1 adds: a pass
// of 256 lanes is four waves and a wave's 64 pixels are one group of the stream (passes start at multiples of 256), so a wave tokenises
// its own group - every lane compares its filtered pixel with the lane's before it (a shuffle; lane 0 loads pixel x - 1 itself), one
// ballot gives the group's repeat mask, and from the mask a lane knows what it is: four literals (its bit is 0), the head of a run (its bit
// is 1 and the bit below is 0, or it is lane 0; the run's length is the count of 1 bits from its own up) or nothing (inside a run).  No scan
// crosses waves.  The histogram counts a head's length symbol (RFC 1951 3.2.5, computed, no table) in bins 257 ... 284 - 285 bins a row, bin
// 256 left 0 for the host's end-of-block - and nothing for a pixel inside a run, while the Adler sums still run over all filtered bytes.
// The pack's item of a head is the length symbol's code, its extra bits and the one 0 bit of the distance code, 21 bits at most; a lane
// inside a run has an item of 0 bits, which png_emit places nowhere.

#define GR_PNG_LANES 256
// 31 carried bits and 256 items of at most 60 bits are 15 391 bits, 481 words; an item's OR may name two words more
#define GR_PNG_BUFFER_WORDS 488

// the four filtered bytes of pixel x of a row, as one word: the pixel minus the pixel above it (row 0: minus the pixel to its left, 0 for x = 0), byte-wise mod 256
__device__ __forceinline__ unsigned int png_filtered_pixel(const unsigned int* __restrict__ frame, int width, int row, int x) {
    const unsigned int here = frame[(size_t)row * (size_t)width + (size_t)x];
    const unsigned int from = row ? frame[(size_t)(row - 1) * (size_t)width + (size_t)x] : (x ? frame[x - 1] : 0u);
    return ((here | 0x80808080u) - (from & 0x7f7f7f7fu)) ^ ((here ^ ~from) & 0x80808080u);
}

// what pixel x of a row is in the runs stream: PNG_LITERALS, the pixels of the run it heads (1 ... 64), or PNG_NOTHING - inside a run, or
// past the row's end.  Every lane of the wave calls it, x = a multiple of 256 + t; f: the pixel's filtered bytes (0 past the row's end)
#define PNG_LITERALS 0u
#define PNG_NOTHING 0xffffffffu
__device__ __forceinline__ unsigned int png_run_token(const unsigned int* __restrict__ frame, int width, int row, int x, unsigned int& f) {
    const int lane = x & 63;   // in the wave, and of the pixel in its group
    const bool in_row = x < width;
    f = in_row ? png_filtered_pixel(frame, width, row, x) : 0u;
    unsigned int before = (unsigned int)__shfl_up((int)f, 1, 64);
    if (lane == 0 && in_row && x > 0) before = png_filtered_pixel(frame, width, row, x - 1);   // the last pixel of the group before
    const bool repeats = in_row && x > 0 && f == before;
    const unsigned long long mask = __ballot(repeats);
    if (!in_row) return PNG_NOTHING;
    if (!repeats) return PNG_LITERALS;
    if (lane && ((mask >> (lane - 1)) & 1ull)) return PNG_NOTHING;
    const unsigned long long rest = ~(mask >> lane);   // its lowest 1 bit: the first pixel from this one up that does not repeat
    return rest ? (unsigned int)__ffsll(rest) - 1u : 64u;
}

// the length symbol of a match of `run` pixels, 4 run bytes: with m = length - 3 the symbols 257 ... 264 are m = 0 ... 7, and four symbols
// follow for every count of extra bits 1 ... 5, m = 8 ... 15, 16 ... 31 and so on
__device__ __forceinline__ unsigned int png_length_symbol(unsigned int run, unsigned int& extra_bits, unsigned int& extra) {
    const unsigned int m = 4u * run - 3u;
    extra_bits = m < 8u ? 0u : 29u - (unsigned int)__clz((int)m);
    extra = m & ((1u << extra_bits) - 1u);
    return 257u + 4u * extra_bits + (m >> extra_bits);
}

template <int KIND>
__device__ __forceinline__ void png_histogram_row(const unsigned int* __restrict__ frame, int width, int height, unsigned int* frame_histogram,
                                                  unsigned int* __restrict__ row_histogram, unsigned int* __restrict__ row_sums) {
    constexpr int BINS = KIND ? 285 : 256;
    __shared__ unsigned int bins[BINS];
    __shared__ unsigned int of_wave[2][4];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), row = (int)blockIdx.x;
    if (row >= height) return;   // (uniform)
    bins[t] = 0u;
    if constexpr (BINS > GR_PNG_LANES)
        if (t + GR_PNG_LANES < BINS) bins[t + GR_PNG_LANES] = 0u;
    __syncthreads();
    unsigned long long sum = 0ull, weighted = 0ull;
    if constexpr (KIND == 0) {
        for (int x = t; x < width; x += GR_PNG_LANES) {
            const unsigned int f = png_filtered_pixel(frame, width, row, x);
            const unsigned int weight = 4u * (unsigned int)(width - x);   // n - i of the pixel's first byte
#pragma unroll
            for (unsigned int c = 0; c < 4u; c++) {
                const unsigned int b = (f >> (8u * c)) & 255u;
                atomicAdd(&bins[b], 1u);
                sum += b;
                weighted += (unsigned long long)(((weight - c) % 65521u) * b);
            }
        }
    } else {
        for (int base = 0; base < width; base += GR_PNG_LANES) {   // (uniform: the ballot wants every lane)
            const int x = base + t;
            unsigned int f;
            const unsigned int token = png_run_token(frame, width, row, x, f);
            if (x < width) {
                const unsigned int weight = 4u * (unsigned int)(width - x);
#pragma unroll
                for (unsigned int c = 0; c < 4u; c++) {
                    const unsigned int b = (f >> (8u * c)) & 255u;
                    if (token == PNG_LITERALS) atomicAdd(&bins[b], 1u);
                    sum += b;
                    weighted += (unsigned long long)(((weight - c) % 65521u) * b);
                }
                if (token != PNG_LITERALS && token != PNG_NOTHING) {
                    unsigned int extra_bits, extra;
                    atomicAdd(&bins[png_length_symbol(token, extra_bits, extra)], 1u);
                }
            }
        }
    }
    unsigned int a = (unsigned int)(sum % 65521ull), w = (unsigned int)(weighted % 65521ull);
    for (int offset = 32; offset > 0; offset >>= 1) {   // (at most 64 x 65 520 a wave)
        a += (unsigned int)__shfl_xor((int)a, offset, 64);
        w += (unsigned int)__shfl_xor((int)w, offset, 64);
    }
    if ((t & 63) == 0) {
        of_wave[0][t >> 6] = a;
        of_wave[1][t >> 6] = w;
    }
    __syncthreads();   // (and every lane's adds to the bins are done)
    if (t == 0) {
        row_sums[2 * (size_t)row] = (of_wave[0][0] + of_wave[0][1] + of_wave[0][2] + of_wave[0][3]) % 65521u;
        row_sums[2 * (size_t)row + 1] = (of_wave[1][0] + of_wave[1][1] + of_wave[1][2] + of_wave[1][3]) % 65521u;
    }
    const unsigned int mine = bins[t];
    row_histogram[(size_t)row * BINS + (size_t)t] = mine;
    if (mine) atomicAdd(&frame_histogram[t], mine);
    if constexpr (BINS > GR_PNG_LANES) {   // (the bins behind the first 256: the length symbols)
        static_assert(BINS <= 2 * GR_PNG_LANES, "a lane stores two bins at most");
        const int u = t + GR_PNG_LANES;
        if (u < BINS) {
            const unsigned int more = bins[u];
            row_histogram[(size_t)row * BINS + (size_t)u] = more;
            if (more) atomicAdd(&frame_histogram[u], more);
        }
    }
}

// grid: height workgroups of 64 x 4.  frame_histogram: 256 words, zeroed by the launcher; row_histogram: height x 256 words;
// row_sums: height x 2 words (sum of b, sum of (n - i) b, each mod 65521, over the row's pixel bytes)
extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) gr_png_histogram(const unsigned int* __restrict__ frame, int width, int height,
                                                                            unsigned int* frame_histogram, unsigned int* __restrict__ row_histogram,
                                                                            unsigned int* __restrict__ row_sums) {
    png_histogram_row<0>(frame, width, height, frame_histogram, row_histogram, row_sums);
}

// the runs stream's: frame_histogram 285 words, row_histogram height x 285 words - a bin a symbol, [256] left 0
extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) gr_png_histogram_runs(const unsigned int* __restrict__ frame, int width, int height,
                                                                                 unsigned int* frame_histogram, unsigned int* __restrict__ row_histogram,
                                                                                 unsigned int* __restrict__ row_sums) {
    png_histogram_row<1>(frame, width, height, frame_histogram, row_histogram, row_sums);
}

// where a row's workgroup is in its segment: buffer[0] of the pass is word `word_at` of the stream and holds `fill` bits already
struct png_segment {
    unsigned int* words;
    unsigned long long word_count, first_word, last_word, word_at;
    unsigned int fill;
};

// one pass: every lane's item (`count` bits of `bits`, the bits above them 0; count 0: none) behind the items of the lanes before it
__device__ __forceinline__ void png_emit(png_segment& s, unsigned int* buffer, unsigned int* wave_bits, int t, unsigned long long bits,
                                         unsigned int count, bool last) {
    const int lane = t & 63, wave = t >> 6;
    unsigned int through = count;   // the bits of this wave's lanes up to and including this one
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int before = (unsigned int)__shfl_up((int)through, d, 64);
        if (lane >= d) through += before;
    }
    if (lane == 63) wave_bits[wave] = through;
    __syncthreads();
    unsigned int at = s.fill + through - count, total = s.fill;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned int v = wave_bits[k];
        total += v;
        if (k < wave) at += v;
    }
    if (count) {
        const unsigned int shift = at & 31u, word = at >> 5;
        const unsigned long long low = bits << shift;
        const unsigned int w0 = (unsigned int)low, w1 = (unsigned int)(low >> 32), w2 = shift ? (unsigned int)(bits >> (64u - shift)) : 0u;
        if (w0 && word < GR_PNG_BUFFER_WORDS) atomicOr(&buffer[word], w0);
        if (w1 && word + 1u < GR_PNG_BUFFER_WORDS) atomicOr(&buffer[word + 1u], w1);
        if (w2 && word + 2u < GR_PNG_BUFFER_WORDS) atomicOr(&buffer[word + 2u], w2);
    }
    __syncthreads();
    // whole words leave (with `last`: the partial word too, the segment ends in it); every word read is left 0 for the next pass
    const unsigned int whole = total >> 5, leaving = last ? (total + 31u) >> 5 : whole;
    unsigned int carried = 0u;
    for (unsigned int i = (unsigned int)t; i <= whole && i < GR_PNG_BUFFER_WORDS; i += GR_PNG_LANES) {
        const unsigned int v = buffer[i];
        buffer[i] = 0u;
        if (i < leaving) {
            const unsigned long long g = s.word_at + i;
            if (g < s.word_count) {
                if (g == s.first_word || g == s.last_word) atomicOr(&s.words[g], v);
                else s.words[g] = v;
            }
        } else {
            carried = v;   // (i == whole: the partial word)
        }
    }
    __syncthreads();
    if (carried) atomicOr(&buffer[0], carried);   // one lane at most; joins the next pass's ORs, which the next pass's barrier covers
    s.word_at += whole;
    s.fill = last ? 0u : (total & 31u);
}

template <int KIND>
__device__ __forceinline__ void png_pack_row(const unsigned int* __restrict__ frame, int width, int height, const unsigned int* __restrict__ table,
                                             const unsigned int* __restrict__ header, int header_bits, const unsigned long long* __restrict__ row_offset,
                                             unsigned int* stream_words, unsigned long long stream_word_count) {
    constexpr int SYMBOLS = KIND ? 285 : 257;
    __shared__ unsigned int codes[SYMBOLS];
    __shared__ unsigned int buffer[GR_PNG_BUFFER_WORDS];
    __shared__ unsigned int wave_bits[4];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), row = (int)blockIdx.x;
    if (row >= height) return;   // (uniform)
    for (int i = t; i < SYMBOLS; i += GR_PNG_LANES) codes[i] = table[i];
    for (int i = t; i < GR_PNG_BUFFER_WORDS; i += GR_PNG_LANES) buffer[i] = 0u;
    const unsigned long long begin = row_offset[row], end = row_offset[row + 1];
    png_segment s;
    s.words = stream_words;
    s.word_count = stream_word_count;
    s.first_word = begin >> 2;
    s.last_word = (end - 1ull) >> 2;
    s.word_at = begin >> 2;
    s.fill = (unsigned int)(begin & 3ull) * 8u;   // the neighbour's bytes of the first word: left 0, the OR keeps them
    __syncthreads();
    {
        // the block header, a word a lane, and the filter-type byte
        const int header_words = (header_bits + 31) >> 5;
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if (t < header_words) {
            bits = header[t];
            count = (unsigned int)min(32, header_bits - 32 * t);
        } else if (t == header_words) {
            const unsigned int e = codes[row ? 2 : 1];
            bits = e & 0xffffu;
            count = e >> 16;
        }
        png_emit(s, buffer, wave_bits, t, bits, count, false);
    }
    for (int base = 0; base < width; base += GR_PNG_LANES) {
        const int x = base + t;
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if constexpr (KIND == 0) {
            if (x < width) {
                const unsigned int f = png_filtered_pixel(frame, width, row, x);
#pragma unroll
                for (unsigned int c = 0; c < 4u; c++) {
                    const unsigned int e = codes[(f >> (8u * c)) & 255u];
                    bits |= (unsigned long long)(e & 0xffffu) << count;
                    count += e >> 16;
                }
            }
        } else {
            unsigned int f;
            const unsigned int token = png_run_token(frame, width, row, x, f);
            if (token == PNG_LITERALS) {
#pragma unroll
                for (unsigned int c = 0; c < 4u; c++) {
                    const unsigned int e = codes[(f >> (8u * c)) & 255u];
                    bits |= (unsigned long long)(e & 0xffffu) << count;
                    count += e >> 16;
                }
            } else if (token != PNG_NOTHING) {
                // a match: the length symbol's code, its extra bits, the distance code's one bit (0)
                unsigned int extra_bits, extra;
                const unsigned int e = codes[png_length_symbol(token, extra_bits, extra)];
                bits = (unsigned long long)(e & 0xffffu) | ((unsigned long long)extra << (e >> 16));
                count = (e >> 16) + extra_bits + 1u;
            }
        }
        png_emit(s, buffer, wave_bits, t, bits, count, false);
    }
    {
        // end-of-block, then the empty stored block: 3 bits, 0 bits up to the byte boundary, LEN = 0, NLEN = 0xffff
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if (t == 0) {
            const unsigned int e = codes[256];
            bits = e & 0xffffu;
            count = (e >> 16) + 3u;
            count += (8u - ((s.fill + count) & 7u)) & 7u;
            bits |= 0xffff0000ull << count;
            count += 32u;
        }
        png_emit(s, buffer, wave_bits, t, bits, count, true);
    }
}

// grid: height workgroups of 64 x 4.  table: 257 words, code | length << 16, the code bit-reversed; header: the block header's bits from
// bit 0 of word 0 up, the bits past header_bits 0; row_offset: height + 1 byte offsets of the segments in the stream (the last: its size);
// stream_words: zeroed by the launcher on this stream, stream_word_count words
extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) gr_png_pack(const unsigned int* __restrict__ frame, int width, int height,
                                                                       const unsigned int* __restrict__ table, const unsigned int* __restrict__ header,
                                                                       int header_bits, const unsigned long long* __restrict__ row_offset,
                                                                       unsigned int* stream_words, unsigned long long stream_word_count) {
    png_pack_row<0>(frame, width, height, table, header, header_bits, row_offset, stream_words, stream_word_count);
}

// the runs stream's: table 285 words
extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) gr_png_pack_runs(const unsigned int* __restrict__ frame, int width, int height,
                                                                            const unsigned int* __restrict__ table, const unsigned int* __restrict__ header,
                                                                            int header_bits, const unsigned long long* __restrict__ row_offset,
                                                                            unsigned int* stream_words, unsigned long long stream_word_count) {
    png_pack_row<1>(frame, width, height, table, header, header_bits, row_offset, stream_words, stream_word_count);
}
