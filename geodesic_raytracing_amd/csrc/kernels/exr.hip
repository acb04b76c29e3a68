// ------------------------------------------------------------------------------------------------
// exr.hip - the device half of the EXR encoder (geodesic_hip_internal.h, "EXR frames"; the host half and the definition of the bytes:
// csrc/exr_stream.cpp).  Part of the set-up module, behind png.hip, whose bit-packer (png_segment, png_emit) it uses as it stands; integers
// and bit arithmetic only - a float of the frame is loaded as its 32 bits and never computed with.  Two launches over a float4 frame that
// is already on the device, one workgroup of 256 lanes (64 x 4) per image row in both:
//
// gr_exr_histogram - what the host needs to build the frame's table, to size the rows' zlib streams and to decide which rows are stored
// raw.  A lane takes a pixel: one 128-bit load for it and one for the pixel to its left, the halfs of b, g, r of both (exr_half_bits, the
// host's lines), and from them the pixel's six predicted bytes - the low and the high byte of each plane, each minus the same byte of the
// pixel before plus 128.  The stream's order is low bytes of B, G, R over all x, then the high bytes, and the predictor runs through it
// without a stop, so pixel 0 closes the five seams of a row with pixel width - 1: its G bytes follow B's last, its R bytes G's, its high
// B byte follows the LOW byte of R's last, and its low B byte, the stream's first, is not predicted at all.  The bytes are counted in 256
// bins in LDS, stored as the row's histogram and added to the frame's; the Adler-32's two sums are reduced as png.hip reduces them, the
// weight of a byte being n minus its position in the REORDERED row (n = 6 width; plane p, pixel x: p width + x, high bytes 3 width more).
//
// gr_exr_pack - the chunks, headers included: chunk r is bytes chunk_offset[r] ... chunk_offset[r + 1] of the stream, 8 bytes of header
// (y, size) and `size` bytes of data, and what the data is the host has decided (row_words[2 r + 1]: 1 = raw).
// A compressed row is emitted in stream order through png_emit, an item of at most 60 bits a lane and pass: in the first pass lane 0 owns
// y, lane 1 the size, lane 2 the bytes 78 01 and the lanes behind a 32-bit word of the block header each; in the passes over the row a lane
// owns GR_EXR_ITEM_BYTES = 4 consecutive positions of the reordered row - a pass is 1 024 of them, NOT 256 pixels: consecutive positions
// are consecutive pixels of one plane, so a lane loads the one component it needs of five pixels (the first for the predictor only); in
// the last pass lane 0 owns end-of-block, the 0 bits up to the byte boundary and the Adler-32 the host made of the row's sums
// (row_words[2 r]), high byte first.
// A raw row is not a bit stream: a lane takes a 32-bit word of the stream and gathers its four bytes - header bytes, or the low or high
// byte of a half in plane order - and stores it with a plain vector store.
// Segment ends: chunks meet at byte boundaries, any of the four.  As in png.hip the launcher zeroes the stream on the same stream in front
// of this launch and a chunk's first and last word are stored with an atomic OR, whichever kind the chunk and its neighbours are; no
// store goes past stream_word_count, whatever the offsets say.

#define GR_EXR_LANES 256
#define GR_EXR_ITEM_BYTES 4
#define GR_EXR_PASS_BYTES (GR_EXR_LANES * GR_EXR_ITEM_BYTES)

// csrc/exr_stream.hpp half_bits, line for line
__device__ __forceinline__ unsigned int exr_half_bits(unsigned int f) {
    const unsigned int sign = (f >> 16) & 0x8000u;
    unsigned int a = f & 0x7fffffffu;
    if (a > 0x7f800000u) return 0u;
    if (a > 0x477fe000u) a = 0x477fe000u;
    if (a >= 0x38800000u) {
        const unsigned int r = a - 0x38000000u;
        return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
    }
    const unsigned int e = a >> 23;
    if (e < 102u) return sign;
    const unsigned int m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;
    unsigned int h = m >> shift;
    const unsigned int rest = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    if (rest > tie || (rest == tie && (h & 1u))) h++;
    return sign | h;
}

// half j of a row's raw bytes, 0 <= j < 3 width: plane j / width (B, G, R: components 2, 1, 0), pixel j % width
__device__ __forceinline__ unsigned int exr_half_at(const unsigned int* __restrict__ row_words, unsigned int width, unsigned int j) {
    const unsigned int plane = (j >= 2u * width) ? 2u : (j >= width) ? 1u : 0u;
    return exr_half_bits(row_words[4 * (size_t)(j - plane * width) + (2u - plane)]);
}

// byte i of the reordered row before the predictor, 0 <= i < 6 width: the low bytes of the halfs, then the high bytes
__device__ __forceinline__ unsigned int exr_reordered_byte(const unsigned int* __restrict__ row_words, unsigned int width, unsigned int i) {
    const unsigned int halfs = 3u * width;
    return i >= halfs ? exr_half_at(row_words, width, i - halfs) >> 8 : exr_half_at(row_words, width, i) & 255u;
}

// grid: height workgroups of 64 x 4.  frame: float4 pixels, 16-byte aligned; frame_histogram: 256 words, zeroed by the launcher;
// row_histogram: height x 256 words; row_sums: height x 2 words (sum of b, sum of (n - i) b, each mod 65521, over the row's predicted bytes)
extern "C" __global__ void __launch_bounds__(GR_EXR_LANES) gr_exr_histogram(const uint4* __restrict__ frame, int width, int height,
                                                                            unsigned int* frame_histogram, unsigned int* __restrict__ row_histogram,
                                                                            unsigned int* __restrict__ row_sums) {
    __shared__ unsigned int bins[256];
    __shared__ unsigned int of_wave[2][4];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), row = (int)blockIdx.x;
    if (row >= height) return;   // (uniform)
    bins[t] = 0u;
    __syncthreads();
    const uint4* pixels = frame + (size_t)row * (size_t)width;
    const unsigned int w = (unsigned int)width, n = 6u * w;
    unsigned long long sum = 0ull, weighted = 0ull;
    for (int x = t; x < width; x += GR_EXR_LANES) {
        const uint4 here = pixels[x], left = pixels[x ? x - 1 : width - 1];
        const unsigned int mine[3] = {exr_half_bits(here.z), exr_half_bits(here.y), exr_half_bits(here.x)};   // B, G, R
        unsigned int low_from[3], high_from[3];   // what the predictor subtracts: the byte before in the stream
        if (x) {
            for (int p = 0; p < 3; p++) {
                const unsigned int before = exr_half_bits(p == 0 ? left.z : p == 1 ? left.y : left.x);
                low_from[p] = before & 255u;
                high_from[p] = before >> 8;
            }
        } else {
            // the seams: `left` is the row's last pixel, and a plane follows the plane before it
            const unsigned int last_b = exr_half_bits(left.z), last_g = exr_half_bits(left.y), last_r = exr_half_bits(left.x);
            low_from[0] = 128u;             // the stream's first byte stands as it is: b - 128 + 128
            low_from[1] = last_b & 255u;
            low_from[2] = last_g & 255u;
            high_from[0] = last_r & 255u;   // the first high byte follows the last LOW byte
            high_from[1] = last_b >> 8;
            high_from[2] = last_g >> 8;
        }
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const unsigned int low = ((mine[p] & 255u) - low_from[p] + 128u) & 255u, high = ((mine[p] >> 8) - high_from[p] + 128u) & 255u;
            const unsigned int at = (unsigned int)p * w + (unsigned int)x;   // of the low byte; the high byte's: 3 w more
            atomicAdd(&bins[low], 1u);
            atomicAdd(&bins[high], 1u);
            sum += low + high;
            weighted += (unsigned long long)(((n - at) % 65521u) * low) + (unsigned long long)(((n - at - 3u * w) % 65521u) * high);
        }
    }
    unsigned int a = (unsigned int)(sum % 65521ull), wsum = (unsigned int)(weighted % 65521ull);
    for (int offset = 32; offset > 0; offset >>= 1) {   // (at most 64 x 65 520 a wave)
        a += (unsigned int)__shfl_xor((int)a, offset, 64);
        wsum += (unsigned int)__shfl_xor((int)wsum, offset, 64);
    }
    if ((t & 63) == 0) {
        of_wave[0][t >> 6] = a;
        of_wave[1][t >> 6] = wsum;
    }
    __syncthreads();   // (and every lane's adds to the bins are done)
    if (t == 0) {
        row_sums[2 * (size_t)row] = (of_wave[0][0] + of_wave[0][1] + of_wave[0][2] + of_wave[0][3]) % 65521u;
        row_sums[2 * (size_t)row + 1] = (of_wave[1][0] + of_wave[1][1] + of_wave[1][2] + of_wave[1][3]) % 65521u;
    }
    const unsigned int counted = bins[t];
    row_histogram[(size_t)row * 256 + (size_t)t] = counted;
    if (counted) atomicAdd(&frame_histogram[t], counted);
}

// grid: height workgroups of 64 x 4.  table: 257 words, code | length << 16, the code bit-reversed; header: the block header's bits from
// bit 0 of word 0 up (BFINAL = 1), the bits past header_bits 0, at most 253 words; chunk_offset: height + 1 byte offsets of the chunks in
// the stream (the last: its size); row_words: height x 2 - the row's Adler-32, and 1 where the row is stored raw; stream_words: zeroed
// by the launcher on this stream, stream_word_count words
extern "C" __global__ void __launch_bounds__(GR_EXR_LANES) gr_exr_pack(const uint4* __restrict__ frame, int width, int height,
                                                                       const unsigned int* __restrict__ table, const unsigned int* __restrict__ header,
                                                                       int header_bits, const unsigned long long* __restrict__ chunk_offset,
                                                                       const unsigned int* __restrict__ row_words, unsigned int* stream_words,
                                                                       unsigned long long stream_word_count) {
    __shared__ unsigned int codes[257];
    __shared__ unsigned int buffer[GR_PNG_BUFFER_WORDS];
    __shared__ unsigned int wave_bits[4];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), row = (int)blockIdx.x;
    if (row >= height) return;   // (uniform)
    const unsigned int* row_pixels = (const unsigned int*)(frame + (size_t)row * (size_t)width);
    const unsigned int w = (unsigned int)width, n = 6u * w;
    const unsigned long long begin = chunk_offset[row], end = chunk_offset[row + 1];
    if (end <= begin) return;   // (uniform; no chunk is empty - offsets that say so are not a frame's)
    const unsigned long long first_word = begin >> 2, last_word = (end - 1ull) >> 2;
    const unsigned int size = (unsigned int)(end - begin - 8ull);
    if (row_words[2 * (size_t)row + 1]) {   // (uniform) raw: a word of the stream a lane
        for (unsigned long long g = first_word + (unsigned long long)t; g <= last_word && g < stream_word_count; g += GR_EXR_LANES) {
            unsigned int word = 0u;
#pragma unroll
            for (unsigned int k = 0; k < 4u; k++) {
                const unsigned long long in_stream = 4ull * g + k;
                if (in_stream < begin || in_stream >= end) continue;   // a neighbour's byte: left 0, the OR keeps it
                const unsigned long long q = in_stream - begin;
                unsigned int b;
                if (q < 4ull) b = ((unsigned int)row >> (8u * (unsigned int)q)) & 255u;
                else if (q < 8ull) b = (size >> (8u * (unsigned int)(q - 4ull))) & 255u;
                else {
                    const unsigned int i = (unsigned int)(q - 8ull);
                    if (i >= n) continue;   // (a size that is no raw row's)
                    const unsigned int h = exr_half_at(row_pixels, w, i >> 1);
                    b = (i & 1u) ? h >> 8 : h & 255u;
                }
                word |= b << (8u * k);
            }
            if (g == first_word || g == last_word) atomicOr(&stream_words[g], word);
            else stream_words[g] = word;
        }
        return;
    }
    for (int i = t; i < 257; i += GR_EXR_LANES) codes[i] = table[i];
    for (int i = t; i < GR_PNG_BUFFER_WORDS; i += GR_EXR_LANES) buffer[i] = 0u;
    png_segment s;
    s.words = stream_words;
    s.word_count = stream_word_count;
    s.first_word = first_word;
    s.last_word = last_word;
    s.word_at = first_word;
    s.fill = (unsigned int)(begin & 3ull) * 8u;   // the neighbour's bytes of the first word: left 0, the OR keeps them
    __syncthreads();
    {
        // the chunk's header, the zlib header, the block header a word a lane
        const int header_words = min((header_bits + 31) >> 5, GR_EXR_LANES - 3);
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if (t == 0) bits = (unsigned int)row, count = 32u;
        else if (t == 1) bits = size, count = 32u;
        else if (t == 2) bits = 0x0178ull, count = 16u;
        else if (t - 3 < header_words) {
            bits = header[t - 3];
            count = (unsigned int)min(32, header_bits - 32 * (t - 3));
        }
        png_emit(s, buffer, wave_bits, t, bits, count, false);
    }
    for (unsigned int base = 0u; base < n; base += GR_EXR_PASS_BYTES) {   // (n <= 2^31 - 1: base does not wrap)
        const unsigned int i0 = base + GR_EXR_ITEM_BYTES * (unsigned int)t;
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if (i0 < n) {
            unsigned int before = i0 ? exr_reordered_byte(row_pixels, w, i0 - 1u) : 128u;   // (position 0 stands as it is)
#pragma unroll
            for (unsigned int k = 0; k < GR_EXR_ITEM_BYTES; k++) {
                if (i0 + k < n) {
                    const unsigned int here = exr_reordered_byte(row_pixels, w, i0 + k);
                    const unsigned int e = codes[(here - before + 128u) & 255u];
                    bits |= (unsigned long long)(e & 0xffffu) << count;
                    count += e >> 16;
                    before = here;
                }
            }
        }
        png_emit(s, buffer, wave_bits, t, bits, count, false);
    }
    {
        // end-of-block, 0 bits up to the byte boundary, the Adler-32 with its high byte first
        unsigned long long bits = 0ull;
        unsigned int count = 0u;
        if (t == 0) {
            const unsigned int e = codes[256], adler = row_words[2 * (size_t)row];
            bits = e & 0xffffu;
            count = e >> 16;
            count += (8u - ((s.fill + count) & 7u)) & 7u;
            bits |= (unsigned long long)__builtin_bswap32(adler) << count;
            count += 32u;
        }
        png_emit(s, buffer, wave_bits, t, bits, count, true);
    }
}
