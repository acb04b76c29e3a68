// ------------------------------------------------------------------------------------------------
// resolve.hip - the box filter behind a supersampled frame (graphics_settings.hpp:23-24, main.cpp:1760-1791: with `supersample` on the
// reference allocates its frame buffers at supersample_factor x the window size per axis, traces at that size and minifies when it
// presents).  gr_resolve_supersampled averages the f x f block of traced float4 pixels behind every output pixel.  Part of the set-up
// module (capi.cpp: compile_setup_module): IEEE arithmetic, no contraction, no re-association - the sum below is taken in the order it
// is written - and none of this shares a compilation with the ray kernels.
//
// One work item per output pixel, consecutive lanes on consecutive pixels of a row: a wave reads 64 * f * 16 contiguous bytes of each of
// its f source rows (f loads of 16 bytes per lane and row, which between them use every byte of the lines they touch) and writes 1 KiB
// contiguously.  The launch is a stream - every source byte is read once, every output byte written once - so there is nothing to keep
// in LDS.  A workgroup is 64 x 4: four waves, each on 64 pixels of one of four consecutive local output rows of the device.
//
// Rows are dealt to devices as gr_render deals them (shading.hip): local row lr is row lr % block_rows of local block lr / block_rows,
// global block = local block * strip_count + strip_rank.  A traced block is exactly f * block_rows rows, so with compact_out - source and
// destination both hold the device's blocks back to back - the f source rows of local output row lr are the local rows f * lr ...
// f * lr + f - 1; without it both are indexed by global row.

template <int F>
__device__ __forceinline__ float4 box_average(const float4* __restrict__ block, size_t source_width) {
    float4 sum = block[0];   // (not 0 + block[0]: a factor of 1 hands every value through as it is, the sign of a zero included)
#pragma unroll
    for (int j = 0; j < F; j++) {
#pragma unroll
        for (int i = 0; i < F; i++) {
            if (i == 0 && j == 0) continue;
            const float4 v = block[(size_t)j * source_width + i];
            sum.x += v.x;
            sum.y += v.y;
            sum.z += v.z;
            sum.w += v.w;
        }
    }
    const float weight = 1.0f / (float)(F * F);
    return make_float4(sum.x * weight, sum.y * weight, sum.z * weight, sum.w * weight);
}

extern "C" __global__ void gr_resolve_supersampled(const float4* __restrict__ source, float4* __restrict__ out, int width, int height,
                                                   int factor, int block_rows, int strip_rank, int strip_count, int compact_out,
                                                   int local_rows) {
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
    out[(size_t)at * width + x] = pixel;
}
