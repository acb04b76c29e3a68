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
