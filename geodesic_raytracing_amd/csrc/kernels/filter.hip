// ------------------------------------------------------------------------------------------------
// filter.hip - separable reconstruction filters behind a supersampled frame: gr_resolve_filtered replaces the one-pixel box of
// resolve.hip by a table of n taps per axis (tent, Gaussian, Mitchell-Netravali: csrc/imageio.cpp's gr_filter_taps; any table of 1 to 16
// taps with n = f mod 2), centred on the output pixel.  The definition is host code, gr_filter_frame (csrc/imageio.cpp;
// include/geodesic_hip_internal.h, "Filtered frames", states it in full), and this kernel is held to it bit for bit: the rows pass
//     h(y, X)   = taps[0] * s(y, cx(X,0)) + taps[1] * s(y, cx(X,1)) + ...      summed in that order, every traced row y
// then the columns pass
//     out(Y, X) = taps[0] * h(cy(Y,0), X) + taps[1] * h(cy(Y,1), X) + ...
// with cx(X,t) = clamp(X f + (f - n)/2 + t, 0, W f - 1) and cy alike, every product and every sum one rounded fp32 operation, h rounded
// to fp32 in between.  Part of the set-up module only (program_build.cpp: PARTS), which is built with -ffp-contract=off: the products and
// sums below stay v_mul_f32 / v_add_f32 (packed or not).  The first term is taps[0] * s and not 0 + ...: a single tap of 1 hands every
// value through, the sign of a zero included, as box_average does at factor 1.
//
// Shape.  A radius-2 filter at factor 4 reads 16 x 16 traced samples a pixel, each shared by 16 pixels, so unlike resolve.hip's stream
// this launch keeps something in LDS.  A workgroup of 256 lanes owns a tile of GR_FILTER_TX x GR_FILTER_TY = 32 x 8 output pixels.
//   phase 1, the rows pass over the (rows of the tile - 1) f + n traced rows the tile's pixels look at (44 at f = 4, n = 16: 1.375 x the 32
//     it owns): one item is one h(y, X); the items are dealt to the lanes row by row, consecutive lanes on consecutive X, so a wave
//     covers two traced rows and in each a run of 31 f + n samples, which its lanes read with n float4 loads each at a stride of f
//     samples - every byte of the run is used, by n / f lanes; that overlap is served by the vector L1, not staged.  The n loads of an
//     item are independent and issued together (n is a template argument: the loop is unrolled and the taps are named by constant
//     indices into the argument block, so they are scalar operands and nothing is indexed at run time).  h goes to LDS as [row][32] float4,
//     a contiguous 1 KiB per wave and store.
//   one barrier.
//   phase 2, the columns pass: lane = (Y, X) of the tile, X fastest; tap t reads LDS row (Y - Y0) f + t.  The two half-waves of a
//     ds_read_b128 read 512 contiguous bytes each, a multiple of 512 B apart: every 16-lane group of the instruction covers all 64 banks
//     once (MI355X: 4 groups of 16 lanes, bank = (address / 4) mod 64), so the reads are conflict-free without padding.  One float4 store
//     a lane, 512 contiguous bytes a half-wave.
// LDS: 44 x 32 x 16 B = 22 KiB a workgroup.  Coordinates are clamped BEFORE the read - a sample past an edge is the edge sample - so lanes of
// a tile that overhangs the frame read inside it; they compute nothing (no lane leaves before the barrier) and store nothing.  Every
// index into the frames is 64-bit.  Whole frames only.  No claim about its speed is made here: tools/filter_probe.py times it against
// gr_resolve_supersampled on the same source and a device copy of the algorithmic traffic, and DESIGN.md ("Filtered frames") says what
// that gave, which other shapes were tried, or that it has not been run.

#define GR_FILTER_TX 32
#define GR_FILTER_TY 8
#define GR_FILTER_MAX_TAPS 16
#define GR_FILTER_LDS_ROWS ((GR_FILTER_TY - 1) * 4 + GR_FILTER_MAX_TAPS)

struct gr_filter_table {   // passed by value: the taps live in the kernel's argument block
    float tap[GR_FILTER_MAX_TAPS];
};

template <int N>
__device__ __forceinline__ void filter_tile(const float4* __restrict__ source, float4* __restrict__ out, int width, int height, int factor,
                                            const gr_filter_table& taps, float4* __restrict__ h) {
    const int lane = threadIdx.x;
    const int tile_x = blockIdx.x * GR_FILTER_TX, tile_y = blockIdx.y * GR_FILTER_TY;
    const int source_width = width * factor, source_height = height * factor;
    const int first = (factor - N) / 2;   // (factor - N is even: exact, negative for a filter wider than a pixel)
    const int tile_rows = min(GR_FILTER_TY, height - tile_y);
    const int rows = (tile_rows - 1) * factor + N;   // at most GR_FILTER_LDS_ROWS
    const int row0 = tile_y * factor + first;

    for (int item = lane; item < rows * GR_FILTER_TX; item += GR_FILTER_TX * GR_FILTER_TY) {
        const int r = item / GR_FILTER_TX, X = tile_x + item % GR_FILTER_TX;
        if (X >= width) continue;
        const int y = min(max(row0 + r, 0), source_height - 1);
        const float4* __restrict__ row = source + (size_t)y * (size_t)source_width;
        const int x0 = X * factor + first;
        float4 s[N];
#pragma unroll
        for (int t = 0; t < N; t++) s[t] = row[(size_t)min(max(x0 + t, 0), source_width - 1)];
        float4 acc = make_float4(taps.tap[0] * s[0].x, taps.tap[0] * s[0].y, taps.tap[0] * s[0].z, taps.tap[0] * s[0].w);
#pragma unroll
        for (int t = 1; t < N; t++) {
            const float4 product = make_float4(taps.tap[t] * s[t].x, taps.tap[t] * s[t].y, taps.tap[t] * s[t].z, taps.tap[t] * s[t].w);
            acc = make_float4(acc.x + product.x, acc.y + product.y, acc.z + product.z, acc.w + product.w);
        }
        h[item] = acc;
    }
    __syncthreads();

    const int lx = lane % GR_FILTER_TX, ly = lane / GR_FILTER_TX;
    const int X = tile_x + lx, Y = tile_y + ly;
    if (X >= width || Y >= height) return;
    const float4* __restrict__ column = h + (ly * factor) * GR_FILTER_TX + lx;
    const float4 v0 = column[0];
    float4 acc = make_float4(taps.tap[0] * v0.x, taps.tap[0] * v0.y, taps.tap[0] * v0.z, taps.tap[0] * v0.w);
#pragma unroll
    for (int t = 1; t < N; t++) {
        const float4 v = column[t * GR_FILTER_TX];
        const float4 product = make_float4(taps.tap[t] * v.x, taps.tap[t] * v.y, taps.tap[t] * v.z, taps.tap[t] * v.w);
        acc = make_float4(acc.x + product.x, acc.y + product.y, acc.z + product.z, acc.w + product.w);
    }
    out[(size_t)Y * (size_t)width + (size_t)X] = acc;
}

extern "C" __global__ void __launch_bounds__(GR_FILTER_TX * GR_FILTER_TY) gr_resolve_filtered(const float4* __restrict__ source, float4* __restrict__ out,
                                                                                                int width, int height, int factor, int count,
                                                                                                gr_filter_table taps) {
    __shared__ float4 h[GR_FILTER_LDS_ROWS * GR_FILTER_TX];
    if (factor < 1 || factor > 4) return;   // (the rows of h are counted for these; uniform, so no lane waits at the barrier)
    switch (count) {   // (wave-uniform; the launcher refuses every other count)
        case 1: filter_tile<1>(source, out, width, height, factor, taps, h); break;
        case 2: filter_tile<2>(source, out, width, height, factor, taps, h); break;
        case 3: filter_tile<3>(source, out, width, height, factor, taps, h); break;
        case 4: filter_tile<4>(source, out, width, height, factor, taps, h); break;
        case 5: filter_tile<5>(source, out, width, height, factor, taps, h); break;
        case 6: filter_tile<6>(source, out, width, height, factor, taps, h); break;
        case 7: filter_tile<7>(source, out, width, height, factor, taps, h); break;
        case 8: filter_tile<8>(source, out, width, height, factor, taps, h); break;
        case 9: filter_tile<9>(source, out, width, height, factor, taps, h); break;
        case 10: filter_tile<10>(source, out, width, height, factor, taps, h); break;
        case 11: filter_tile<11>(source, out, width, height, factor, taps, h); break;
        case 12: filter_tile<12>(source, out, width, height, factor, taps, h); break;
        case 13: filter_tile<13>(source, out, width, height, factor, taps, h); break;
        case 14: filter_tile<14>(source, out, width, height, factor, taps, h); break;
        case 15: filter_tile<15>(source, out, width, height, factor, taps, h); break;
        case 16: filter_tile<16>(source, out, width, height, factor, taps, h); break;
        default: break;
    }
}
