// ------------------------------------------------------------------------------------------------
// present.hip - the last step of the reference's presentation chain: 8-bit sRGB pixels.  The reference presents through an sRGB texture and
// its screenshot path (main.cpp:2791-2796) turns every value into a byte with clamp -> lin_to_srgb -> clamp -> * 255 truncated; the host
// states that in csrc/imageio.cpp (gr_frame_to_rgba8).  gr_present_rgba8 does it on the device, fused with the box filter of a
// supersampled frame: box_average<F> of resolve.hip - the same function in the same compilation, so the value encoded is
// gr_resolve_supersampled's to the bit - and then the encode of all four channels, alpha included.  Part of the set-up module only.
//
// The encode evaluates no power.  The host encode is monotone on [0, 1], so it is a step function with at most 255 steps, and the host
// finds them by bisection with its own function (gr_srgb8_thresholds): T[k] = the smallest float whose byte is >= k, +infinity where no
// float's is.  byte(c) = the number of k in 1 ... 255 with T[k] <= c: the device agrees with the library's host powf by construction.
// GR_SRGB8_TREE_BITS (written in front of this module's source when it is assembled, capi.cpp: compile_setup_module) holds T[1 ... 255] as
// bit patterns in the breadth-first order of the perfect search tree over them: node i has children 2i and 2i + 1, entry 0 is unused.
// A search is  i = 1;  8 x  i = 2 i + (tree[i] <= c);  byte = i - 256  - no branch, 8 LDS reads.  Why that order and not the sorted table:
// a ds_read_b32 is banked by (address / 4) % 32 within 32 lanes, and a bisection of the sorted table probes T[128], then T[64] / T[192],
// then four entries 64 apart ... - for its first five steps every address a wave asks for is on one or two banks, 2-, 4-, 8-way
// conflicts by design.  Level l of the tree is 2^l consecutive entries: no two of them share a bank down to level 5, and levels 6 and
// 7 conflict only as far as the picture's values scatter (lanes that ask for the same entry are served by one broadcast).
//
// A NaN compares false with every entry: its byte is 0 (the host's cast of a NaN is undefined).  Negative values and -0.0 likewise give
// 0; values above 1, +infinity included, are clamped to 1 first, so that the +infinity entries of unreachable bytes are never counted.
//
// Shape: resolve.hip's.  A workgroup is 64 x 4, one lane per output pixel, a wave on 64 consecutive pixels of one row: it reads whole
// lines of each of its f source rows in 16-byte loads and writes 256 contiguous bytes.  Each workgroup copies the 1 KiB table to LDS,
// one entry per lane, and meets at one barrier BEFORE any lane leaves for being out of range.  One pixel per lane is the form to start
// from and the form kept; no claim about its speed is made here.  tools/present_probe.py times the launch against a device copy of its
// traffic, and DESIGN.md ("8-bit frames") records what that gave, or that it has not been run: four pixels per lane (one 16-byte store)
// is worth trying only if that number is short of the copy's.
// Rows are dealt to devices exactly as in gr_resolve_supersampled.

__device__ __forceinline__ unsigned int srgb8_of(const float* tree, float v) {
    const float c = v > 1.0f ? 1.0f : v;   // (not fminf: a NaN stays a NaN)
    unsigned int i = 1;
#pragma unroll
    for (int level = 0; level < 8; level++) i = 2u * i + (tree[i] <= c ? 1u : 0u);
    return i - 256u;
}

extern "C" __global__ void __launch_bounds__(256) gr_present_rgba8(const float4* __restrict__ source, unsigned int* __restrict__ out, int width,
                                                                   int height, int factor, int block_rows, int strip_rank, int strip_count,
                                                                   int compact_out, int local_rows) {
    __shared__ float tree[256];
    const unsigned int lane = threadIdx.y * 64u + threadIdx.x;   // the launcher's workgroup is 64 x 4: one entry per lane
    tree[lane] = __uint_as_float(GR_SRGB8_TREE_BITS[lane]);
    __syncthreads();
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int lr = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || lr >= local_rows) return;
    const int lb = lr / block_rows;
    const int row = (lb * strip_count + strip_rank) * block_rows + (lr - lb * block_rows);
    if (row >= height) return;
    const int at = compact_out ? lr : row;
    const size_t source_width = (size_t)width * factor;
    const float4* block = source + (size_t)at * factor * source_width + (size_t)x * factor;
    float4 pixel;
    switch (factor) {
        case 1: pixel = box_average<1>(block, source_width); break;
        case 2: pixel = box_average<2>(block, source_width); break;
        case 3: pixel = box_average<3>(block, source_width); break;
        case 4: pixel = box_average<4>(block, source_width); break;
        default: return;
    }
    // bytes R, G, B, A in memory order
    out[(size_t)at * width + x] = srgb8_of(tree, pixel.x) | (srgb8_of(tree, pixel.y) << 8) | (srgb8_of(tree, pixel.z) << 16) | (srgb8_of(tree, pixel.w) << 24);
}

// ------------------------------------------------------------------------------------------------
// gr_present_yuv420 - the same chain in a third format: resolve -> sRGB bytes -> 8-bit BT.709 Y'CbCr, limited range, chroma subsampled
// 2 x 2 (centre sited: the average of the four ENCODED pixels), as csrc/imageio.cpp states it on the host (gr_rgba8_to_yuv420; the
// formulas and the layouts are in include/geodesic_hip.h).  The R, G, B bytes are gr_present_rgba8's: box_average<F> and srgb8_of above,
// over the same table; alpha is not encoded.  The matrix is 32-bit integer arithmetic with arithmetic shifts - no float after the bytes -
// so the launch can be held to the host function byte for byte.  Whole frames only (no strips: 1.5 bytes a pixel in planes do not fit the
// exchange of a split frame).
//
// Shape: a lane owns 2 rows x 4 columns, so each of its two chroma samples is formed in registers - no second pass, no LDS exchange, no
// atomics.  A workgroup is 64 x 4 as above: lane x of 64 on columns 4 x ... 4 x + 3, a wave along one row PAIR - 256 columns, and a
// workgroup on 256 columns x 8 rows.  Per source row a lane reads 4 f consecutive float4 and a wave 4 KiB f contiguously; a wave writes
// 256 contiguous bytes to each of its two luma rows and 128 to each chroma plane (256 to NV12's one).  Where width % 4 == 0 (every
// video size; dst is aligned to 4 bytes, the launcher refuses anything else) every group of a lane is one store: 4 bytes a luma row,
// 2 bytes a chroma plane or 4 bytes of NV12 - the alignment follows from width % 4 == 0 for every plane offset.  Any other width
// stores byte by byte.  A pixel past the right or bottom edge is the edge pixel itself (x and y are clamped BEFORE the read: nothing is
// read outside the source), which is the definition's rule for an odd width or height; what lies past the edge is not stored.
// The table is copied and the barrier met before any lane leaves, as in gr_present_rgba8.  No claim about its speed is made here:
// tools/present_yuv_probe.py times it against gr_present_rgba8 on the same source, and DESIGN.md ("Video frames") says what that gave.

#define GR_YUV420_I420 0
#define GR_YUV420_NV12 1

template <int F>
__device__ __forceinline__ void present_yuv420_lane(const float* tree, const float4* __restrict__ source, unsigned char* __restrict__ out,
                                                    int width, int height, int layout, int x0, int y0) {
    const size_t source_width = (size_t)width * F;
    unsigned int luma[2][4];
    int sum_r[2] = {0, 0}, sum_g[2] = {0, 0}, sum_b[2] = {0, 0};   // of the 2 x 2 block behind chroma sample 0 and 1 of this lane
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int y = min(y0 + j, height - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = min(x0 + i, width - 1);
            const float4 pixel = box_average<F>(source + (size_t)y * F * source_width + (size_t)x * F, source_width);
            const int r = (int)srgb8_of(tree, pixel.x), g = (int)srgb8_of(tree, pixel.y), b = (int)srgb8_of(tree, pixel.z);
            luma[j][i] = (unsigned int)(16 + ((11966 * r + 40254 * g + 4064 * b + 32768) >> 16));
            sum_r[i / 2] += r;
            sum_g[i / 2] += g;
            sum_b[i / 2] += b;
        }
    }
    unsigned int cb[2], cr[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        cb[k] = (unsigned int)(128 + ((-6596 * sum_r[k] - 22188 * sum_g[k] + 28784 * sum_b[k] + 131072) >> 18));
        cr[k] = (unsigned int)(128 + ((28784 * sum_r[k] - 26145 * sum_g[k] - 2639 * sum_b[k] + 131072) >> 18));
    }
    const size_t chroma_width = (size_t)((width + 1) / 2), chroma_height = (size_t)((height + 1) / 2);
    unsigned char* chroma = out + (size_t)width * height;   // both layouts: the chroma follows the luma plane
    const size_t cx = (size_t)(x0 / 2), cy = (size_t)(y0 / 2);
    if ((width & 3) == 0) {   // (uniform) x0 + 3 < width, every plane offset below is a multiple of its store's size
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (y0 + j < height)
                *(unsigned int*)(out + (size_t)(y0 + j) * width + x0) = luma[j][0] | (luma[j][1] << 8) | (luma[j][2] << 16) | (luma[j][3] << 24);
        if (layout == GR_YUV420_NV12) {
            *(unsigned int*)(chroma + cy * 2 * chroma_width + 2 * cx) = cb[0] | (cr[0] << 8) | (cb[1] << 16) | (cr[1] << 24);
        } else {
            *(unsigned short*)(chroma + cy * chroma_width + cx) = (unsigned short)(cb[0] | (cb[1] << 8));
            *(unsigned short*)(chroma + chroma_width * chroma_height + cy * chroma_width + cx) = (unsigned short)(cr[0] | (cr[1] << 8));
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (y0 + j < height && x0 + i < width) out[(size_t)(y0 + j) * width + x0 + i] = (unsigned char)luma[j][i];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (x0 + 2 * k >= width) continue;
        if (layout == GR_YUV420_NV12) {
            chroma[cy * 2 * chroma_width + 2 * (cx + k)] = (unsigned char)cb[k];
            chroma[cy * 2 * chroma_width + 2 * (cx + k) + 1] = (unsigned char)cr[k];
        } else {
            chroma[cy * chroma_width + cx + k] = (unsigned char)cb[k];
            chroma[chroma_width * chroma_height + cy * chroma_width + cx + k] = (unsigned char)cr[k];
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) gr_present_yuv420(const float4* __restrict__ source, unsigned char* __restrict__ out, int width,
                                                                    int height, int factor, int layout) {
    __shared__ float tree[256];
    const unsigned int lane = threadIdx.y * 64u + threadIdx.x;   // the launcher's workgroup is 64 x 4: one entry per lane
    tree[lane] = __uint_as_float(GR_SRGB8_TREE_BITS[lane]);
    __syncthreads();
    const long long column = 4ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x), row = 2ll * ((long long)blockIdx.y * blockDim.y + threadIdx.y);
    if (column >= width || row >= height) return;
    const int x0 = (int)column, y0 = (int)row;
    switch (factor) {
        case 1: present_yuv420_lane<1>(tree, source, out, width, height, layout, x0, y0); break;
        case 2: present_yuv420_lane<2>(tree, source, out, width, height, layout, x0, y0); break;
        case 3: present_yuv420_lane<3>(tree, source, out, width, height, layout, x0, y0); break;
        case 4: present_yuv420_lane<4>(tree, source, out, width, height, layout, x0, y0); break;
        default: return;
    }
}

// ------------------------------------------------------------------------------------------------
// gr_present_yuv420p10 - gr_present_yuv420 with ten bits a sample: resolve -> 10-bit sRGB codes -> BT.709 Y'CbCr, limited range
// (Y' 64 ... 940, Cb and Cr 64 ... 960), chroma sited and subsampled as above, every sample a 16-bit word.  The host states it in
// csrc/imageio.cpp (gr_frame_to_rgb10, gr_rgb10_to_yuv420p10); the formulas and layouts are in include/geodesic_hip_internal.h
// ("10-bit video frames").  GR_YUV420_I420 is yuv420p10le - planes Y, Cb, Cr, the code in the low ten bits of its word; GR_YUV420_NV12 is
// P010 - the Y plane, then rows of (Cb, Cr) pairs, the code in the HIGH ten bits (code << 6).
//
// The code of a value is found as its byte is above, in a table of the same kind: GR_SRGB10_TREE_BITS (written in front of this
// module's source next to the 8-bit one) holds gr_srgb10_thresholds' T[1 ... 1023] in the breadth-first order of the perfect search
// tree, entry 0 unused.  A search is  i = 1;  10 x  i = 2 i + (tree[i] <= c);  code = i - 1024  - no branch, 10 LDS reads, a NaN gives 0.
// Levels 0 to 5 are as conflict-free as the 8-bit tree's; levels 6 to 9 (64 to 512 consecutive entries) conflict as far as the
// picture's values scatter.  The table is 4 KiB of LDS: every lane of the 64 x 4 workgroup copies four entries, 256 apart, so that
// each of the four copies reads and writes 1 KiB contiguously, and all lanes meet at one barrier BEFORE any of them leaves.
//
// Shape and edges: gr_present_yuv420's - a lane owns 2 rows x 4 columns and forms its two chroma samples in registers, x and y are
// clamped BEFORE the read, what lies past the edge is not stored.  Where width % 4 == 0 (dst is aligned to 8 bytes, the launcher
// refuses anything else) a lane's stores are 8 bytes a luma row, 4 bytes a chroma plane or 8 bytes of P010's pairs.  Their alignment
// follows from width % 4 == 0 for every plane offset: x0 is a multiple of 4 words, a luma row of 4 words, the luma plane (width * height
// words) therefore too; the chroma width is even, so x0 / 2 and a chroma row are multiples of 2 words and so is the Cb plane; a P010
// chroma row is width words and 2 (x0 / 2) a multiple of 4.  Any other width stores word by word (dst aligned to 2 bytes).
// No claim about its speed is made here: tools/present_yuv_probe.py times it against gr_present_yuv420 on the same source.

__device__ __forceinline__ int srgb10_of(const float* tree, float v) {
    const float c = v > 1.0f ? 1.0f : v;   // (not fminf: a NaN stays a NaN)
    unsigned int i = 1;
#pragma unroll
    for (int level = 0; level < 10; level++) i = 2u * i + (tree[i] <= c ? 1u : 0u);
    return (int)(i - 1024u);
}

template <int F>
__device__ __forceinline__ void present_yuv420p10_lane(const float* tree, const float4* __restrict__ source, unsigned short* __restrict__ out,
                                                       int width, int height, int layout, int x0, int y0) {
    const size_t source_width = (size_t)width * F;
    const int shift = layout == GR_YUV420_NV12 ? 6 : 0;   // P010 keeps a code in the high ten bits of its word
    unsigned int luma[2][4];
    int sum_r[2] = {0, 0}, sum_g[2] = {0, 0}, sum_b[2] = {0, 0};   // of the 2 x 2 block behind chroma sample 0 and 1 of this lane
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int y = min(y0 + j, height - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = min(x0 + i, width - 1);
            const float4 pixel = box_average<F>(source + (size_t)y * F * source_width + (size_t)x * F, source_width);
            const int r = srgb10_of(tree, pixel.x), g = srgb10_of(tree, pixel.y), b = srgb10_of(tree, pixel.z);
            luma[j][i] = (unsigned int)(64 + ((11931 * r + 40136 * g + 4052 * b + 32768) >> 16)) << shift;
            sum_r[i / 2] += r;
            sum_g[i / 2] += g;
            sum_b[i / 2] += b;
        }
    }
    unsigned int cb[2], cr[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        cb[k] = (unsigned int)(512 + ((-6576 * sum_r[k] - 22124 * sum_g[k] + 28700 * sum_b[k] + 131072) >> 18)) << shift;
        cr[k] = (unsigned int)(512 + ((28700 * sum_r[k] - 26068 * sum_g[k] - 2632 * sum_b[k] + 131072) >> 18)) << shift;
    }
    const size_t chroma_width = (size_t)((width + 1) / 2), chroma_height = (size_t)((height + 1) / 2);
    unsigned short* chroma = out + (size_t)width * height;   // both layouts: the chroma follows the luma plane
    const size_t cx = (size_t)(x0 / 2), cy = (size_t)(y0 / 2);
    if ((width & 3) == 0) {   // (uniform) x0 + 3 < width, every plane offset below is a multiple of its store's size
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (y0 + j < height)
                *(uint2*)(out + (size_t)(y0 + j) * width + x0) = make_uint2(luma[j][0] | (luma[j][1] << 16), luma[j][2] | (luma[j][3] << 16));
        if (layout == GR_YUV420_NV12) {
            *(uint2*)(chroma + cy * 2 * chroma_width + 2 * cx) = make_uint2(cb[0] | (cr[0] << 16), cb[1] | (cr[1] << 16));
        } else {
            *(unsigned int*)(chroma + cy * chroma_width + cx) = cb[0] | (cb[1] << 16);
            *(unsigned int*)(chroma + chroma_width * chroma_height + cy * chroma_width + cx) = cr[0] | (cr[1] << 16);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (y0 + j < height && x0 + i < width) out[(size_t)(y0 + j) * width + x0 + i] = (unsigned short)luma[j][i];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (x0 + 2 * k >= width) continue;
        if (layout == GR_YUV420_NV12) {
            chroma[cy * 2 * chroma_width + 2 * (cx + k)] = (unsigned short)cb[k];
            chroma[cy * 2 * chroma_width + 2 * (cx + k) + 1] = (unsigned short)cr[k];
        } else {
            chroma[cy * chroma_width + cx + k] = (unsigned short)cb[k];
            chroma[chroma_width * chroma_height + cy * chroma_width + cx + k] = (unsigned short)cr[k];
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) gr_present_yuv420p10(const float4* __restrict__ source, unsigned short* __restrict__ out, int width,
                                                                       int height, int factor, int layout) {
    __shared__ float tree[1024];
    const unsigned int lane = threadIdx.y * 64u + threadIdx.x;   // the launcher's workgroup is 64 x 4: four entries per lane
#pragma unroll
    for (unsigned int k = 0; k < 4u; k++) tree[lane + 256u * k] = __uint_as_float(GR_SRGB10_TREE_BITS[lane + 256u * k]);
    __syncthreads();
    const long long column = 4ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x), row = 2ll * ((long long)blockIdx.y * blockDim.y + threadIdx.y);
    if (column >= width || row >= height) return;
    const int x0 = (int)column, y0 = (int)row;
    switch (factor) {
        case 1: present_yuv420p10_lane<1>(tree, source, out, width, height, layout, x0, y0); break;
        case 2: present_yuv420p10_lane<2>(tree, source, out, width, height, layout, x0, y0); break;
        case 3: present_yuv420p10_lane<3>(tree, source, out, width, height, layout, x0, y0); break;
        case 4: present_yuv420p10_lane<4>(tree, source, out, width, height, layout, x0, y0); break;
        default: return;
    }
}
