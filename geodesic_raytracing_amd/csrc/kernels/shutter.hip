// ------------------------------------------------------------------------------------------------
// shutter.hip - the shutter of a motion-blurred frame: a delivered frame is the weighted sum of T sub-frames rendered at T poses inside the
// frame's shutter interval, summed in linear light on the device.  gr_shutter_accumulate adds ONE sub-frame: per output pixel
//     accum = [accum +] weight * box_average<F>(the pixel's block of the traced sub-frame)
// as csrc/imageio.cpp states it on the host (gr_accumulate_frame: one fp32 multiply and one fp32 add, each rounded).  box_average<F> is
// resolve.hip's - the same function in the same compilation, so the value weighted is gr_resolve_supersampled's to the bit.  Part of the
// set-up module only (capi.cpp: compile_setup_module): it is built with -ffp-contract=off, so the multiply and the add below stay two
// instructions (v_mul_f32, v_add_f32; tests/test_shutter_abi.py reads the module's disassembly for an fma in this kernel).
//
// With `first` the accumulation frame is written and NOT read: the first sub-frame of a shutter needs no memset launch in front of it and
// saves 16 bytes of traffic a pixel; what the buffer held before - a NaN included - does not matter.  It is weight * value and not
// 0 + weight * value: a weight of 1 hands every value through as it is, the sign of a zero included, as box_average does at factor 1.
// The weights are the caller's: nothing here normalises them.
//
// Shape: resolve.hip's.  One lane per output pixel, a workgroup of 64 x 4, consecutive lanes on consecutive pixels of a row: a wave reads
// 64 * f * 16 contiguous bytes of each of its f source rows, reads (unless `first`) and writes 1 KiB of the accumulation frame contiguously.
// The launch is a stream - every byte is touched once - so there is nothing to keep in LDS.  Whole frames only (no strips: a share of a
// split frame has its own exchange rules).  Every index is 64-bit.  No claim about its speed is made here: tools/shutter_probe.py times it
// against gr_resolve_supersampled on the same source and against a device copy of its traffic, and DESIGN.md ("Motion-blurred frames")
// says what that gave, or that it has not been run.

extern "C" __global__ void __launch_bounds__(256) gr_shutter_accumulate(const float4* __restrict__ source, float4* __restrict__ accum, int width,
                                                                        int height, int factor, float weight, int first) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t source_width = (size_t)width * factor;
    const float4* block = source + (size_t)y * factor * source_width + (size_t)x * factor;
    float4 pixel;
    switch (factor) {
        case 1: pixel = box_average<1>(block, source_width); break;
        case 2: pixel = box_average<2>(block, source_width); break;
        case 3: pixel = box_average<3>(block, source_width); break;
        case 4: pixel = box_average<4>(block, source_width); break;
        default: return;
    }
    const size_t at = (size_t)y * width + x;
    float4 sum = make_float4(pixel.x * weight, pixel.y * weight, pixel.z * weight, pixel.w * weight);
    if (!first) {
        const float4 before = accum[at];
        sum = make_float4(before.x + sum.x, before.y + sum.y, before.z + sum.z, before.w + sum.w);
    }
    accum[at] = sum;
}
