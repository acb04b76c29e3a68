// ------------------------------------------------------------------------------------------------
// jpeg.hip - the device half of the JPEG encoder (geodesic_hip_internal.h, "JPEG frames"; the host half and the definition of the bytes:
// csrc/jpeg_stream.cpp).  Part of the set-up module (capi.cpp: compile_setup_module); integers only.  Three launches over an RGBA8 frame
// that is already on the device; no table depends on the frame, so nothing goes through the host between them.
//
// gr_jpeg_blocks - a workgroup of 256 lanes (64 x 4) on GR_JPEG_BLOCKS_MCUS = 4 MCUs side by side, 64 x 16 pixels.  The pixels come in with
// 32-bit loads, a wave on 256 consecutive bytes of an image row (a pixel past the right or bottom edge is the edge's), and are staged in
// LDS; from there a lane converts four pixels to Y' - 128 and one 2 x 2 group to Cb - 128 and Cr - 128 (the rounded mean of R, G, B,
// converted once) into the 24 blocks' samples.  Lanes 0 ... 191 then own a row of a block (eight sums of eight products with the 2^14
// constants, rounded to 6 fraction bits) and, behind a barrier, a column (the same, rounded to 4 fraction bits), quantise the eight
// coefficients - the division by 16 step is a multiplication by ceil(2^32 / (16 step)), exact for these operands (jpeg_stream.cpp:
// device_tables) - and leave them in LDS in zig-zag order; the workgroup's 3 072 bytes go out with coalesced 32-bit stores.
// Every product's operands fit 24 bits (a constant is below 2^13 + 2^12, a sample 8 bits, a row sum 16), so __mul24 is exact.
//
// gr_jpeg_pack - a workgroup of 384 lanes (64 x 6) per MCU row; per pass a lane owns one block of GR_JPEG_PACK_MCUS = 64 MCUs.  It walks
// its 64 coefficients (eight 16-byte loads) once to count its bits - the DC difference against its component's previous block in scan order,
// 0 at the row's start; run/size symbols with ZRL and EOB - an inclusive scan of the counts over the wave (shuffles) and the six waves'
// totals through LDS place it, and it walks them again to OR code and value bits, most significant bit first, into a window of
// GR_JPEG_WINDOW_WORDS 32-bit words in LDS.  A pass of 384 worst-case blocks is 636 672 bits, five windows; a rendered frame's fits one.
// Whole words are flushed byte-swapped (the stream is big-endian) with coalesced stores into the row's own slot of the scratch, the
// partial word is carried into the next pass, the last pass pads with 1-bits to a byte.  Slots are 16-byte aligned: no atomics on
// global memory.  The row's byte count and its count of FF bytes are stored beside.
//
// gr_jpeg_gather - a workgroup of 256 lanes per MCU row.  It sums the stuffed sizes of the rows in front of it (at most 4 096: every
// workgroup redoes the sum), then moves its row 4 096 bytes a pass: a lane loads 16 bytes, counts its FF bytes, a scan places it, and it
// stores its bytes one by one with a 00 behind each FF.  RSTm (m = row mod 8) follows, EOI behind the last row, whose workgroup stores the
// file's size.  No store goes past the capacities the launcher hands in, whatever the sizes in the scratch say.

#define GR_JPEG_BLOCKS_MCUS 4
#define GR_JPEG_PACK_MCUS 64
#define GR_JPEG_PACK_LANES (6 * GR_JPEG_PACK_MCUS)
#define GR_JPEG_WINDOW_WORDS 4096u
// 31 carried bits, 384 blocks of at most 1 658 bits, 7 bits of padding: 636 710 bits in windows of 131 072
#define GR_JPEG_MAX_WINDOWS 5u
// jpeg_stream.hpp: TABLE_DC, TABLE_AC, TABLE_RECIPROCAL, TABLE_HALF
#define GR_JPEG_TABLE_DC 0
#define GR_JPEG_TABLE_AC 32
#define GR_JPEG_TABLE_RECIPROCAL 544
#define GR_JPEG_TABLE_HALF 672

// round(2^14 c[u][x]), c the orthonormal DCT-II matrix (jpeg_stream.cpp: DCT)
__device__ const int gr_jpeg_dct[64] = {5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793,     8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035,
                                        7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568, 6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811,
                                        5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793, 4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551,
                                        3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135, 1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598};
// the zig-zag position of natural index i (the inverse of jpeg_stream.cpp: ZIGZAG)
__device__ const unsigned char gr_jpeg_zigzag_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                                        10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// jpeg_stream.cpp: convert() - component 0 gives Y' - 128, 1 Cb - 128, 2 Cr - 128
__device__ __forceinline__ int jpeg_convert(int component, int r, int g, int b) {
    const int sum = component == 0 ? 19595 * r + 38470 * g + 7471 * b : component == 1 ? -11059 * r - 21709 * g + 32768 * b : 32768 * r - 27439 * g - 5329 * b;
    const int centred = ((sum + 32768) >> 16) - (component == 0 ? 128 : 0);
    return min(max(centred, -128), 127);
}

// grid: ceil(MCUs across / 4) x MCU rows workgroups of 64 x 4.  coefficients: per MCU in scan order six blocks of 64 int16 in zig-zag order
extern "C" __global__ void __launch_bounds__(256) gr_jpeg_blocks(const unsigned int* __restrict__ frame, int width, int height,
                                                                 const unsigned int* __restrict__ tables, unsigned int* __restrict__ coefficients) {
    __shared__ unsigned int pixels[16][16 * GR_JPEG_BLOCKS_MCUS];
    __shared__ int work[6 * GR_JPEG_BLOCKS_MCUS][64];
    __shared__ short quantised[6 * GR_JPEG_BLOCKS_MCUS][64];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x);
    const int across = (width + 15) >> 4, first_mcu = (int)blockIdx.x * GR_JPEG_BLOCKS_MCUS, mcu_row = (int)blockIdx.y;
    if (first_mcu >= across || mcu_row * 16 >= height) return;   // (uniform)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int at = t + 256 * i, y = at >> 6, x = at & 63;
        const int px = min(first_mcu * 16 + x, width - 1), py = min(mcu_row * 16 + y, height - 1);
        pixels[y][x] = frame[(size_t)py * (size_t)width + (size_t)px];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int at = t + 256 * i, y = at >> 6, x = at & 63;
        const unsigned int p = pixels[y][x];
        work[(x >> 4) * 6 + ((y >> 3) << 1 | ((x >> 3) & 1))][(y & 7) * 8 + (x & 7)] = jpeg_convert(0, (int)(p & 255u), (int)((p >> 8) & 255u), (int)((p >> 16) & 255u));
    }
    {
        const int cy = t >> 5, cx = t & 31;
        int r = 2, g = 2, b = 2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned int p = pixels[2 * cy + (k >> 1)][2 * cx + (k & 1)];
            r += (int)(p & 255u);
            g += (int)((p >> 8) & 255u);
            b += (int)((p >> 16) & 255u);
        }
        work[(cx >> 3) * 6 + 4][cy * 8 + (cx & 7)] = jpeg_convert(1, r >> 2, g >> 2, b >> 2);
        work[(cx >> 3) * 6 + 5][cy * 8 + (cx & 7)] = jpeg_convert(2, r >> 2, g >> 2, b >> 2);
    }
    __syncthreads();
    const int block = t >> 3, line = t & 7;   // lanes 0 ... 191: a row of a block, then a column
    if (block < 6 * GR_JPEG_BLOCKS_MCUS) {
        int s[8], out[8];
#pragma unroll
        for (int x = 0; x < 8; x++) s[x] = work[block][8 * line + x];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int sum = 0;
#pragma unroll
            for (int x = 0; x < 8; x++) sum += __mul24(gr_jpeg_dct[8 * u + x], s[x]);
            out[u] = (sum + 128) >> 8;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) work[block][8 * line + u] = out[u];
    }
    __syncthreads();
    if (block < 6 * GR_JPEG_BLOCKS_MCUS) {
        const int cls = block % 6 >= 4 ? 1 : 0;
        int s[8];
#pragma unroll
        for (int y = 0; y < 8; y++) s[y] = work[block][8 * y + line];
#pragma unroll
        for (int v = 0; v < 8; v++) {
            int sum = 0;
#pragma unroll
            for (int y = 0; y < 8; y++) sum += __mul24(gr_jpeg_dct[8 * v + y], s[y]);
            const int coefficient = (sum + 32768) >> 16, natural = 8 * v + line;
            const unsigned int n = (unsigned int)abs(coefficient) + tables[GR_JPEG_TABLE_HALF + 64 * cls + natural];
            const int q = (int)__umulhi(n, tables[GR_JPEG_TABLE_RECIPROCAL + 64 * cls + natural]);
            quantised[block][gr_jpeg_zigzag_of[natural]] = (short)(coefficient < 0 ? -q : q);
        }
    }
    __syncthreads();
    const int mcus = min(GR_JPEG_BLOCKS_MCUS, across - first_mcu);
    unsigned int* to = coefficients + ((size_t)mcu_row * (size_t)across + (size_t)first_mcu) * (6 * 32);
    const unsigned int* from = (const unsigned int*)&quantised[0][0];
    for (int i = t; i < mcus * 6 * 32; i += 256) to[i] = from[i];
}

// `count` bits (1 ... 26) of `value` at bit `at` of the pass's bit string, bit 31 of a word first; only the words inside the window, which
// starts at word first_word of the string, are touched
__device__ __forceinline__ void jpeg_put(unsigned int* window, unsigned int first_word, unsigned int at, unsigned int value, unsigned int count) {
    const unsigned long long bits = (unsigned long long)value << (64u - count - (at & 31u));
    const unsigned int high = (unsigned int)(bits >> 32), low = (unsigned int)bits, word = (at >> 5) - first_word;   // (in front of the window: wraps)
    if (high && word < GR_JPEG_WINDOW_WORDS) atomicOr(&window[word], high);
    if (low && word + 1u < GR_JPEG_WINDOW_WORDS) atomicOr(&window[word + 1u], low);
}

// the bits of one block: counted, and with EMIT also written at bit `at`.  block: 64 coefficients in zig-zag order, 16-byte aligned
template <bool EMIT>
__device__ __forceinline__ unsigned int jpeg_code_block(const short* block, int predictor, const unsigned int* dc, const unsigned int* ac,
                                                        unsigned int* window, unsigned int first_word, unsigned int at) {
    unsigned int bits = 0u, run = 0u;
    for (int j = 0; j < 8; j++) {
        const uint4 loaded = ((const uint4*)block)[j];
        const unsigned int pair[4] = {loaded.x, loaded.y, loaded.z, loaded.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            int v = (int)(short)(pair[i >> 1] >> (16 * (i & 1)));
            const bool is_dc = j == 0 && i == 0;
            if (is_dc) v -= predictor;
            if (!is_dc && v == 0) {
                run++;
                continue;
            }
            for (; run >= 16u; run -= 16u) {   // ZRL
                const unsigned int e = ac[0xf0];
                if (EMIT) jpeg_put(window, first_word, at + bits, e & 0xffffu, e >> 16);
                bits += e >> 16;
            }
            const unsigned int size = 32u - (unsigned int)__clz(abs(v));
            const unsigned int e = is_dc ? dc[size] : ac[run << 4 | size], length = (e >> 16) + size;
            if (EMIT) jpeg_put(window, first_word, at + bits, (e & 0xffffu) << size | ((unsigned int)(v < 0 ? v - 1 : v) & ((1u << size) - 1u)), length);
            bits += length;
            run = 0u;
        }
    }
    if (run) {   // EOB
        const unsigned int e = ac[0x00];
        if (EMIT) jpeg_put(window, first_word, at + bits, e & 0xffffu, e >> 16);
        bits += e >> 16;
    }
    return bits;
}

__device__ __forceinline__ unsigned int jpeg_ff_bytes(unsigned int word) {
    return ((word & 0xffu) == 0xffu) + ((word & 0xff00u) == 0xff00u) + ((word & 0xff0000u) == 0xff0000u) + ((word & 0xff000000u) == 0xff000000u);
}

// grid: MCU rows workgroups of 64 x 6.  rows: slot_words words per MCU row, the row's entropy-coded bytes before stuffing from its first
// byte on; row_bytes, row_ff: one word per MCU row each
extern "C" __global__ void __launch_bounds__(GR_JPEG_PACK_LANES) gr_jpeg_pack(const short* __restrict__ coefficients, int width, int height,
                                                                              const unsigned int* __restrict__ tables, unsigned int* __restrict__ rows,
                                                                              unsigned int slot_words, unsigned int* __restrict__ row_bytes,
                                                                              unsigned int* __restrict__ row_ff) {
    __shared__ unsigned int dc[32], ac[512];
    __shared__ unsigned int window[GR_JPEG_WINDOW_WORDS];
    __shared__ unsigned int of_wave[6];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), lane = t & 63, wave = t >> 6, row = (int)blockIdx.x;
    const int across = (width + 15) >> 4, blocks_of_row = across * 6;
    if (row * 16 >= height) return;   // (uniform)
    for (int i = t; i < 32; i += GR_JPEG_PACK_LANES) dc[i] = tables[GR_JPEG_TABLE_DC + i];
    for (int i = t; i < 512; i += GR_JPEG_PACK_LANES) ac[i] = tables[GR_JPEG_TABLE_AC + i];
    for (unsigned int i = (unsigned int)t; i < GR_JPEG_WINDOW_WORDS; i += GR_JPEG_PACK_LANES) window[i] = 0u;
    const short* of_row = coefficients + (size_t)row * (size_t)blocks_of_row * 64;
    unsigned int* slot = rows + (size_t)row * (size_t)slot_words;
    __syncthreads();
    unsigned int word_at = 0u, fill = 0u, ff = 0u;   // words of the slot written, bits carried in window[0], FF bytes this lane stored
    for (int base = 0; base < blocks_of_row; base += GR_JPEG_PACK_LANES) {
        const int b = base + t, component = b % 6;
        const bool mine = b < blocks_of_row, last = base + GR_JPEG_PACK_LANES >= blocks_of_row;
        const short* block = of_row + (size_t)b * 64;
        const int cls = component >= 4 ? 1 : 0;
        int predictor = 0;   // the DC of the component's previous block in scan order: Y00 follows the MCU before's Y11
        if (mine && component >= 1 && component <= 3) predictor = block[-64];
        else if (mine && b >= 6) predictor = block[component == 0 ? -3 * 64 : -6 * 64];
        const unsigned int count = mine ? jpeg_code_block<false>(block, predictor, dc + 16 * cls, ac + 256 * cls, window, 0u, 0u) : 0u;
        unsigned int through = count;   // the bits of this wave's lanes up to and including this one
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int before = (unsigned int)__shfl_up((int)through, d, 64);
            if (lane >= d) through += before;
        }
        __syncthreads();   // (the pass before has read of_wave, and carried its partial word into window[0])
        if (lane == 63) of_wave[wave] = through;
        __syncthreads();
        unsigned int at = fill + through - count, total = fill;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const unsigned int v = of_wave[k];
            total += v;
            if (k < wave) at += v;
        }
        const unsigned int padding = last ? (8u - (total & 7u)) & 7u : 0u, end = total + padding;
        for (unsigned int w = 0u; w < GR_JPEG_MAX_WINDOWS; w++) {
            const unsigned int first_word = w * GR_JPEG_WINDOW_WORDS, first_bit = first_word * 32u;
            if (first_bit >= end) break;   // (uniform)
            if (mine && at < first_bit + GR_JPEG_WINDOW_WORDS * 32u && at + count > first_bit)
                jpeg_code_block<true>(block, predictor, dc + 16 * cls, ac + 256 * cls, window, first_word, at);
            if (t == 0 && padding) jpeg_put(window, first_word, total, (1u << padding) - 1u, padding);
            __syncthreads();
            // whole words leave; the partial word at the end of the pass is carried, or leaves too where the row ends (its padding made it whole bytes)
            const unsigned int left = end - first_bit;
            const unsigned int whole = min(GR_JPEG_WINDOW_WORDS, left >> 5), partial = (left >> 5) < GR_JPEG_WINDOW_WORDS && (left & 31u) ? 1u : 0u;
            unsigned int carried = 0u;
            for (unsigned int i = (unsigned int)t; i < whole + partial; i += GR_JPEG_PACK_LANES) {
                const unsigned int v = window[i];
                window[i] = 0u;
                if (i < whole || last) {
                    const unsigned int to = word_at + first_word + i;
                    if (to < slot_words) slot[to] = __builtin_bswap32(v);
                    ff += jpeg_ff_bytes(v);
                } else {
                    carried = v;
                }
            }
            __syncthreads();
            if (carried) window[0] = carried;   // (one lane at most, and the last window of the pass)
        }
        word_at += end >> 5;
        fill = end & 31u;
    }
    for (int offset = 32; offset > 0; offset >>= 1) ff += (unsigned int)__shfl_xor((int)ff, offset, 64);
    __syncthreads();
    if (lane == 0) of_wave[wave] = ff;
    __syncthreads();
    if (t == 0) {
        row_bytes[row] = word_at * 4u + (fill >> 3);
        row_ff[row] = of_wave[0] + of_wave[1] + of_wave[2] + of_wave[3] + of_wave[4] + of_wave[5];
    }
}

// grid: MCU rows workgroups of 64 x 4.  rows, row_bytes, row_ff: as gr_jpeg_pack left them; file: the headers (header_bytes of them, in
// place already) and behind them the entropy-coded data, capacity bytes in all; file_bytes: the file's size, stored by the last row
extern "C" __global__ void __launch_bounds__(256) gr_jpeg_gather(const unsigned int* __restrict__ rows, unsigned int slot_words,
                                                                 const unsigned int* __restrict__ row_bytes, const unsigned int* __restrict__ row_ff,
                                                                 int mcu_rows, unsigned char* __restrict__ file, unsigned int header_bytes,
                                                                 unsigned long long capacity, unsigned long long* __restrict__ file_bytes) {
    __shared__ unsigned long long sums[4];
    __shared__ unsigned int of_wave[4];
    const int t = (int)(threadIdx.y * 64 + threadIdx.x), lane = t & 63, wave = t >> 6, row = (int)blockIdx.x;
    if (row >= mcu_rows) return;   // (uniform)
    const unsigned int slot_bytes = slot_words * 4u;
    unsigned long long before = 0ull;   // the stuffed bytes and the markers of the rows in front of this one
    for (int r = t; r < row; r += 256) before += (unsigned long long)min(row_bytes[r], slot_bytes) + row_ff[r] + 2ull;
    for (int offset = 32; offset > 0; offset >>= 1) before += (unsigned long long)__shfl_xor((long long)before, offset, 64);
    if (lane == 0) sums[wave] = before;
    __syncthreads();
    unsigned long long at = (unsigned long long)header_bytes + sums[0] + sums[1] + sums[2] + sums[3];
    const unsigned int bytes = min(row_bytes[row], slot_bytes);
    const uint4* slot = (const uint4*)(rows + (size_t)row * (size_t)slot_words);
    for (unsigned int base = 0u; base < slot_bytes; base += 256u * 16u) {
        if (base >= bytes) break;   // (uniform)
        const unsigned int from = base + 16u * (unsigned int)t, have = from < bytes ? min(16u, bytes - from) : 0u;
        uint4 loaded = make_uint4(0u, 0u, 0u, 0u);
        if (have) loaded = slot[from >> 4];
        const unsigned int word[4] = {loaded.x, loaded.y, loaded.z, loaded.w};
        unsigned int count = have;
#pragma unroll
        for (unsigned int i = 0u; i < 16u; i++)
            if (i < have && ((word[i >> 2] >> (8u * (i & 3u))) & 255u) == 255u) count++;
        unsigned int through = count;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int v = (unsigned int)__shfl_up((int)through, d, 64);
            if (lane >= d) through += v;
        }
        __syncthreads();   // (the pass before has read of_wave)
        if (lane == 63) of_wave[wave] = through;
        __syncthreads();
        unsigned long long to = at + through - count;
        unsigned int total = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned int v = of_wave[k];
            total += v;
            if (k < wave) to += v;
        }
#pragma unroll
        for (unsigned int i = 0u; i < 16u; i++) {
            if (i >= have) continue;
            const unsigned int byte = (word[i >> 2] >> (8u * (i & 3u))) & 255u;
            if (to < capacity) file[to] = (unsigned char)byte;
            to++;
            if (byte == 255u) {
                if (to < capacity) file[to] = 0u;
                to++;
            }
        }
        at += total;
    }
    if (t == 0) {
        if (at < capacity) file[at] = 0xffu;
        if (at + 1ull < capacity) file[at + 1ull] = row + 1 < mcu_rows ? (unsigned char)(0xd0 + row % 8) : (unsigned char)0xd9;
        if (row + 1 == mcu_rows) *file_bytes = at + 2ull;
    }
}
