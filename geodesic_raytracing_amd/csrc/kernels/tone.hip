// ------------------------------------------------------------------------------------------------
// tone.hip - the meter and the tone curve of a delivered frame (include/geodesic_hip_internal.h, "Metering and tone curve", states all of
// it; the host statements are gr_meter_histogram_frame, gr_meter_solve_host and gr_tone_frame in csrc/imageio.cpp, and these kernels are
// held to them exactly: the counts as integers, the solve and the curve bit for bit).  Part of the set-up module only (program_build.cpp:
// PARTS), which is built without contraction and with IEEE division: every product, sum and quotient below is one rounded operation.
//
//   gr_meter_histogram   one read of the float4 frame -> 385 counters: per pixel Y = ((0.2126f r) + (0.7152f g)) + (0.0722f b); a pixel
//     whose Y > 0 is false is counted in [384] ("black"), every other in [clamp((bits(Y) >> 20) - 824, 0, 383)] - eight bins an octave
//     from 2^-24, no logarithm.  The launcher zeroes the 385 words on the stream first.
//   gr_meter_solve       one wave, lane 0: the counts and the tone's scalars -> the adaptation state, q and the gain, in double, 385 trips.
//   gr_tone_apply        elementwise: gain x colour through the curve; alpha passes; src == dst is allowed.
//
// gr_meter_histogram's shape.  A workgroup of 256 lanes (four waves) walks tiles of 1024 consecutive pixels with the grid's stride; in a
// tile lane l reads pixels l, l + 256, l + 512, l + 768 - four 16-byte loads in flight a lane, each 1 KiB contiguous a wave.  Every wave
// owns a sub-histogram of 385 counters in LDS (4 x 385 x 4 B = 6160 B a workgroup), so waves never meet on a counter.  Inside a wave the
// lanes would: a star frame puts nearly every pixel into `black` or into the one bin of the sky's floor, and 64 LDS atomics on one
// address are served one after another.  So a wave first takes `black` out - a ballot counts the lanes that hold it and one of them
// adds the count in one LDS atomic - and then peels two more values: the first live lane's bin is broadcast, the lanes that hold it are
// counted by a ballot and the leader adds that count; twice.  After that a star frame's wave - black, the sky's floor, a star - is mostly
// done with three LDS atomics for 64 pixels.  What is left - a frame whose bins are spread - goes lane by lane with one LDS atomic each,
// where lanes mostly differ and conflicts are few.  Measured, a 4K star frame still takes 1.4 times a spread one, with `black` first
// (0.052 ms) as without (0.053 ms): the wave's two common values are not where that time goes, and where it does go - the lane-by-lane
// tail into 185 occupied counters, or the merge's five times as many global atomics - is not established.  Two peels and not a loop until empty: on a
// spread frame a full peel costs up to 64 serial rounds a wave, more than the atomics it replaces.  Other schemes (a sort inside the wave,
// a match over all lanes, counters in registers for the run of a lane) were not tried.  At the end the four sub-histograms are summed
// and every non-zero counter goes to global memory with one vector atomic add (no return value): at most 385 a workgroup, at most
// 1024 workgroups.  Lanes past the end of the frame carry the bin -1, which is no counter; the trip count of the stride loop is the
// workgroup's, so every lane reaches both barriers.  Every frame index is 64-bit.  No claim about its speed is made here:
// tools/tone_probe.py times it against a factor-1 gr_resolve_supersampled launch of the same frame, and DESIGN.md ("Metering and tone
// curve") says what that gave, or that it has not been run.

#define GR_METER_BINS 384          // [384] is `black`
#define GR_METER_COUNTERS 385
#define GR_METER_LANES 256
#define GR_METER_WAVES 4
#define GR_METER_PER_LANE 4
#define GR_METER_TILE 1024         // GR_METER_LANES * GR_METER_PER_LANE pixels a workgroup and trip
#define GR_TONE_LANES 256

__device__ __forceinline__ int meter_bin(const float4 s) {
    const float yr = 0.2126f * s.x, yg = 0.7152f * s.y, yb = 0.0722f * s.z;
    const float yrg = yr + yg;
    const float y = yrg + yb;
    if (!(y > 0.f)) return GR_METER_BINS;
    const int e = (int)(__float_as_uint(y) >> 20) - 824;
    return min(max(e, 0), GR_METER_BINS - 1);
}

// all 64 lanes of the wave call this together; bin < 0: nothing to count
__device__ __forceinline__ void meter_count(unsigned* counters, int bin, int lane_in_wave) {
    unsigned long long todo = __ballot(bin >= 0);
    // `black` first, whoever holds it: one atomic of its lane count
    const unsigned long long dark = __ballot(bin == GR_METER_BINS);
    if (dark) {   // (wave-uniform)
        if (lane_in_wave == __ffsll((long long)dark) - 1) atomicAdd(&counters[GR_METER_BINS], (unsigned)__popcll(dark));
        todo &= ~dark;
    }
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (todo == 0) return;   // (wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int value = __builtin_amdgcn_readlane(bin, leader);
        const unsigned long long same = __ballot(bin == value) & todo;
        if (lane_in_wave == leader) atomicAdd(&counters[value], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane_in_wave) & 1ull) atomicAdd(&counters[bin], 1u);
}

extern "C" __global__ void __launch_bounds__(GR_METER_LANES) gr_meter_histogram(const float4* __restrict__ source, unsigned long long pixels,
                                                                                unsigned* __restrict__ hist) {
    __shared__ unsigned sub[GR_METER_WAVES][GR_METER_COUNTERS];
    const int lane = threadIdx.x;
    const int wave = lane / 64, lane_in_wave = lane % 64;
    for (int i = lane; i < GR_METER_WAVES * GR_METER_COUNTERS; i += GR_METER_LANES) (&sub[0][0])[i] = 0u;
    __syncthreads();
    for (unsigned long long base = (unsigned long long)blockIdx.x * GR_METER_TILE; base < pixels; base += (unsigned long long)gridDim.x * GR_METER_TILE) {
        int bin[GR_METER_PER_LANE];
#pragma unroll
        for (int j = 0; j < GR_METER_PER_LANE; j++) {
            const unsigned long long at = base + (unsigned long long)(j * GR_METER_LANES + lane);
            bin[j] = at < pixels ? meter_bin(source[at]) : -1;
        }
#pragma unroll
        for (int j = 0; j < GR_METER_PER_LANE; j++) meter_count(sub[wave], bin[j], lane_in_wave);
    }
    __syncthreads();
    for (int b = lane; b < GR_METER_COUNTERS; b += GR_METER_LANES) {
        const unsigned total = ((sub[0][b] + sub[1][b]) + sub[2][b]) + sub[3][b];
        if (total) atomicAdd(&hist[b], total);
    }
}

// struct gr_tone_state of the header: what the solve keeps in device memory from frame to frame, and what it hands to gr_tone_apply
struct gr_tone_state_words {
    double adapted;
    int primed;
    int q;
    float gain;
    int reserved;
};

// T[i] = (float)exp2(i / 16.0): the header's GR_TONE_SIXTEENTHS, literal for literal (tests/test_tone_abi.py compares the two texts)
__device__ const float gr_tone_sixteenths[16] = {0x1.000000p+0f, 0x1.0b5586p+0f, 0x1.172b84p+0f, 0x1.2387a6p+0f, 0x1.306fe0p+0f, 0x1.3dea64p+0f, 0x1.4bfdaep+0f, 0x1.5ab07ep+0f,
                                                 0x1.6a09e6p+0f, 0x1.7a1148p+0f, 0x1.8ace54p+0f, 0x1.9c4918p+0f, 0x1.ae89fap+0f, 0x1.c199bep+0f, 0x1.d5818ep+0f, 0x1.ea4afap+0f};

// (no NaN reaches these: a < b ? a : b and a > b ? a : b, as the host writes them)
__device__ __forceinline__ double tone_lesser(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double tone_greater(double a, double b) { return a > b ? a : b; }

// gr_meter_solve_host's arithmetic, operation for operation, on lane 0 (the sums are serial by definition).  mode 1 is auto; in manual
// mode the launcher does not come here.
extern "C" __global__ void __launch_bounds__(64) gr_meter_solve(const unsigned* __restrict__ hist, gr_tone_state_words* __restrict__ state, float key_stops,
                                                                float low, float high, float min_stops, float max_stops, float rate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long total = 0;
    for (int b = 0; b < GR_METER_BINS; b++) total += hist[b];
    double adapted = state->adapted;
    int primed = state->primed;
    if (total != 0) {
        const double n = (double)total;
        const double lo = (double)low * n, hi = (double)high * n;
        double sum_w = 0.0, sum_m = 0.0;
        unsigned long long below = 0;
        for (int b = 0; b < GR_METER_BINS; b++) {
            const double c = (double)below;
            below += hist[b];
            const double upper = tone_lesser((double)below, hi), lower = tone_greater(c, lo);
            const double w = tone_greater(0.0, upper - lower);
            const double centre = (double)b + 0.5;
            const double m = w * centre;
            sum_w = sum_w + w;
            sum_m = sum_m + m;
        }
        const double mean = sum_m / sum_w;
        const double octaves = mean / 8.0;
        const double level = octaves - 24.0;
        const double wanted = (double)key_stops - level;
        const double target = tone_lesser(tone_greater(wanted, (double)min_stops), (double)max_stops);
        if (!primed) {
            adapted = target;
            primed = 1;
        } else {
            const double step = target - adapted;
            const double move = (double)rate * step;
            adapted = adapted + move;
        }
    } else if (!primed) {
        adapted = 0.0;
    }
    const double sixteenths = adapted * 16.0;
    const int q = (int)rint(sixteenths);
    const int index = ((q % 16) + 16) % 16;
    const int whole = (q - index) / 16;
    state->adapted = adapted;
    state->primed = primed;
    state->q = q;
    state->gain = ldexpf(gr_tone_sixteenths[index], whole);
}

__device__ __forceinline__ float tone_curve(float c, float gain, int curve, float iw2) {
    const float v = gain * c;
    const float x = v > 0.f ? (v < 16777216.f ? v : 16777216.f) : 0.f;
    if (curve == 1) {   // GR_TONE_REINHARD
        const float a = x * iw2;
        const float one_a = 1.f + a;
        const float n = x * one_a;
        const float d = 1.f + x;
        return n / d;
    }
    if (curve == 2) {   // GR_TONE_FILMIC
        const float n1 = 2.51f * x;
        const float n2 = n1 + 0.03f;
        const float n = x * n2;
        const float d1 = 2.43f * x;
        const float d2 = d1 + 0.59f;
        const float d3 = x * d2;
        const float d = d3 + 0.14f;
        const float y = n / d;
        return y < 1.f ? y : 1.f;
    }
    return x;           // GR_TONE_LINEAR
}

// device_gain: the word gr_meter_solve wrote, or NULL: host_gain, from the argument block.  source and out may be one frame: each pixel is
// read and then written by its own lane, so neither is __restrict__.
extern "C" __global__ void __launch_bounds__(GR_TONE_LANES) gr_tone_apply(const float4* source, float4* out, unsigned long long pixels, int curve, float iw2,
                                                                          const float* device_gain, float host_gain) {
    const float gain = device_gain ? *device_gain : host_gain;
    for (unsigned long long i = (unsigned long long)blockIdx.x * GR_TONE_LANES + threadIdx.x; i < pixels; i += (unsigned long long)gridDim.x * GR_TONE_LANES) {
        const float4 s = source[i];
        out[i] = make_float4(tone_curve(s.x, gain, curve, iw2), tone_curve(s.y, gain, curve, iw2), tone_curve(s.z, gain, curve, iw2), s.w);
    }
}
