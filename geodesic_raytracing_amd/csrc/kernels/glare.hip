// ------------------------------------------------------------------------------------------------
// glare.hip - a point-spread function and an exposure applied to the resolved frame in linear light, before any encode: gr_apply_glare
// (capi.cpp) convolves a float4 frame of W x H with a core plus up to four separable components of 1 to 129 taps each.  The definition is
// host code, gr_glare_frame (csrc/imageio.cpp; include/geodesic_hip_internal.h, "Glare", states it in full), and these kernels are held to
// it bit for bit, for r, g and b: per component k, the rows pass
//     h_k(y, X) = tap[0] * s(y, cx(X,0)) + tap[1] * s(y, cx(X,1)) + ...          summed in that order, every row y
// then the columns pass
//     g_k(Y, X) = tap[0] * h_k(cy(Y,0), X) + tap[1] * h_k(cy(Y,1), X) + ...
// with cx(X,t) = clamp(X - R + t, 0, W - 1), cy alike, R = (n - 1) / 2, and the combine
//     out(Y, X) = core * s(Y, X) + weight[0] * g_0(Y, X) + weight[1] * g_1(Y, X) + ...     in that order; out.w = s.w, bit for bit
// every product and every sum one rounded fp32 operation, h_k and g_k rounded to fp32.  Part of the set-up module only (program_build.cpp:
// PARTS), which is built with -ffp-contract=off: the products and sums below stay v_mul_f32 / v_add_f32 (packed or not).  The sum over t
// is a dependent chain by definition and is not reassociated.  The first terms are tap[0] * s and core * s, not 0 + ...: core 1 with no
// component hands every value through, the sign of a zero included.
//
// Launches.  No component: gr_glare_scale, one elementwise launch.  Otherwise two a component, 2 K in all: gr_glare_rows reads the source and
// writes h_k to a scratch frame; gr_glare_columns reads h_k and does the component's step of the combine in place in the destination - the
// first reads core * s from the source, every later one the running sum it finds in the destination, each pixel read and written by the
// one lane that owns it.  The round trip of h_k through memory is 2 x 133 MB for a 4K frame, tens of microseconds: the passes are not fused.
// The one table a launch applies travels in its argument block (516 bytes); t is wave-uniform, so a tap is a scalar operand.
//
// Shape.  With up to 129 taps a lane's neighbours come from LDS, staged once a tile with 16-byte accesses, the apron included.
//   gr_glare_rows     a workgroup of 256 lanes owns 256 consecutive pixels of one row.  LDS: the 256 + 2 R samples around them,
//     (256 + 128) x 16 B = 6 KiB; at R = 64 a sample is loaded 1.5 times.  Lane l reads line[l + t]: the 64 lanes of a read cover
//     1 KiB contiguous.
//   gr_glare_columns  a workgroup of 256 lanes owns 16 columns x 64 rows, four pixels a lane (rows ly, ly + 16, ly + 32, ly + 48: four
//     independent chains in flight).  LDS: (64 + 2 R) rows x 16 pixels, at most 192 x 16 x 16 B = 48 KiB (three workgroups a CU); at R = 64 a
//     sample is loaded 3 times, at R = 30 1.9 times - the tile is tall and narrow because the apron is rows.  A row of the tile is 256
//     contiguous bytes of the frame.  Lane (ly, lx) reads tile[(ly + 16 j + t) * 16 + lx]: again 1 KiB contiguous a wave.
//   Banks.  Alpha is not convolved, so the compiler narrows a lane's read to the 12 bytes it uses: ds_read_b96, which MI355X serves in 8
//     groups of 8 lanes - {0-3, 20-23}, {4-7, 16-19}, {8-11, 28-31}, {12-15, 24-27} and the same plus 32 - with bank = (address / 4) mod 32.
//     With lane l on the bytes at base + 16 l, the three banks of a lane are 4 (l mod 8) + 0 ... 2, and each group holds every residue mod 8
//     once: both passes read conflict-free without padding (a 16-byte read, 4 groups of 16 lanes over 64 banks, would be too, by l mod 16).
//     The staging stores are ds_write_b128 of consecutive lanes to consecutive 16 bytes.  A 12-byte read costs 8 LDS cycles a wave against
//     4 for 16 bytes, and every tap of every pixel is a read of its own: a lane that kept a sliding window of a column in registers would
//     read each sample once for its four pixels.  That is not done here; DESIGN.md ("Glare") says what is known of the cost.
// Coordinates are clamped BEFORE the read - a sample past an edge is the edge sample - so lanes of a tile that overhangs the frame read
// inside it; they compute on what LDS holds and store nothing, and no lane leaves before a barrier.  Every index into the frames is 64-bit,
// and a workgroup walks the tiles with a stride of the grid, so no frame of up to 2^31 - 1 pixels is too tall or too wide for the grid.
// Whole frames only.  No claim about its speed is made here: tools/glare_probe.py times it against as many factor-1
// gr_resolve_supersampled launches, and DESIGN.md ("Glare") says what that gave, or that it has not been run.

#define GR_GLARE_MAX_TAPS 129
#define GR_GLARE_MAX_RADIUS 64
#define GR_GLARE_LANES 256
#define GR_GLARE_ROW_TILE 256   // gr_glare_rows: pixels of one row a workgroup owns
#define GR_GLARE_COLUMN_TX 16   // gr_glare_columns: the tile
#define GR_GLARE_COLUMN_TY 64

struct gr_glare_table {   // passed by value: the taps live in the kernel's argument block
    float tap[GR_GLARE_MAX_TAPS];
};

__device__ __forceinline__ bool glare_count_is_valid(int count) { return count >= 1 && count <= GR_GLARE_MAX_TAPS && (count & 1); }

extern "C" __global__ void __launch_bounds__(GR_GLARE_LANES) gr_glare_rows(const float4* __restrict__ source, float4* __restrict__ out, int width, int height,
                                                                             int count, gr_glare_table taps) {
    __shared__ float4 line[GR_GLARE_ROW_TILE + 2 * GR_GLARE_MAX_RADIUS];
    if (!glare_count_is_valid(count) || width < 1 || height < 1) return;   // (the launcher refuses these; uniform, so no lane waits at a barrier)
    const int lane = threadIdx.x;
    const int radius = (count - 1) / 2;
    const unsigned long long tiles_x = ((unsigned long long)width + GR_GLARE_ROW_TILE - 1) / GR_GLARE_ROW_TILE;
    const unsigned long long tiles = tiles_x * (unsigned long long)height;
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long y = (long long)(tile / tiles_x), x0 = (long long)(tile % tiles_x) * GR_GLARE_ROW_TILE;
        const float4* __restrict__ row = source + (size_t)y * (size_t)width;
        const int staged = (int)min((long long)GR_GLARE_ROW_TILE, (long long)width - x0) + 2 * radius;   // at most 384
        for (int i = lane; i < staged; i += GR_GLARE_LANES) line[i] = row[(size_t)min(max(x0 - radius + i, 0ll), (long long)width - 1)];
        __syncthreads();
        if (x0 + lane < width) {
            float4 s = line[lane];
            float ax = taps.tap[0] * s.x, ay = taps.tap[0] * s.y, az = taps.tap[0] * s.z;
            for (int t = 1; t < count; t++) {
                s = line[lane + t];
                const float px = taps.tap[t] * s.x, py = taps.tap[t] * s.y, pz = taps.tap[t] * s.z;
                ax = ax + px;
                ay = ay + py;
                az = az + pz;
            }
            out[(size_t)y * (size_t)width + (size_t)(x0 + lane)] = make_float4(ax, ay, az, 0.f);   // (alpha is not convolved: the columns pass never reads it)
        }
        __syncthreads();   // the next tile's staging writes the line
    }
}

// previous: the source with first != 0 (the combine starts at scale * s, scale = the core), else the destination itself (the running sum);
// it may be `out`, each pixel read and then written by its own lane, so neither is __restrict__
extern "C" __global__ void __launch_bounds__(GR_GLARE_LANES) gr_glare_columns(const float4* __restrict__ rows, const float4* previous, float4* out, int width,
                                                                                int height, int count, float scale, float weight, int first,
                                                                                gr_glare_table taps) {
    __shared__ float4 tile[(GR_GLARE_COLUMN_TY + 2 * GR_GLARE_MAX_RADIUS) * GR_GLARE_COLUMN_TX];
    if (!glare_count_is_valid(count) || width < 1 || height < 1) return;   // (as above)
    const int lane = threadIdx.x;
    const int lx = lane % GR_GLARE_COLUMN_TX, ly = lane / GR_GLARE_COLUMN_TX;   // ly: 0 ... 15
    const int radius = (count - 1) / 2;
    const unsigned long long tiles_x = ((unsigned long long)width + GR_GLARE_COLUMN_TX - 1) / GR_GLARE_COLUMN_TX;
    const unsigned long long tiles_y = ((unsigned long long)height + GR_GLARE_COLUMN_TY - 1) / GR_GLARE_COLUMN_TY;
    const unsigned long long tiles = tiles_x * tiles_y;
    for (unsigned long long index = blockIdx.x; index < tiles; index += gridDim.x) {
        const long long x0 = (long long)(index % tiles_x) * GR_GLARE_COLUMN_TX, y0 = (long long)(index / tiles_x) * GR_GLARE_COLUMN_TY;
        const int staged_rows = (int)min((long long)GR_GLARE_COLUMN_TY, (long long)height - y0) + 2 * radius;   // at most 192
        for (int i = lane; i < staged_rows * GR_GLARE_COLUMN_TX; i += GR_GLARE_LANES) {
            const long long x = min(x0 + i % GR_GLARE_COLUMN_TX, (long long)width - 1);
            const long long y = min(max(y0 - radius + i / GR_GLARE_COLUMN_TX, 0ll), (long long)height - 1);
            tile[i] = rows[(size_t)y * (size_t)width + (size_t)x];
        }
        __syncthreads();
        // pixel j of the lane is row ly + 16 j of the tile; tap t reads tile row ly + 16 j + t <= 63 + 128.  Rows past staged_rows hold what an
        // earlier tile left: only lanes whose pixel is outside the frame read them, and they store nothing.
        const float4* __restrict__ column = tile + ly * GR_GLARE_COLUMN_TX + lx;
        float ax[4], ay[4], az[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float4 v = column[j * 16 * GR_GLARE_COLUMN_TX];
            ax[j] = taps.tap[0] * v.x;
            ay[j] = taps.tap[0] * v.y;
            az[j] = taps.tap[0] * v.z;
        }
        for (int t = 1; t < count; t++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float4 v = column[(j * 16 + t) * GR_GLARE_COLUMN_TX];
                const float px = taps.tap[t] * v.x, py = taps.tap[t] * v.y, pz = taps.tap[t] * v.z;
                ax[j] = ax[j] + px;
                ay[j] = ay[j] + py;
                az[j] = az[j] + pz;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long X = x0 + lx, Y = y0 + ly + 16 * j;
            if (X < width && Y < height) {
                const size_t at = (size_t)Y * (size_t)width + (size_t)X;
                const float4 p = previous[at];
                float bx = p.x, by = p.y, bz = p.z;
                if (first) {   // (wave-uniform)
                    bx = scale * p.x;
                    by = scale * p.y;
                    bz = scale * p.z;
                }
                const float wx = weight * ax[j], wy = weight * ay[j], wz = weight * az[j];
                bx = bx + wx;
                by = by + wy;
                bz = bz + wz;
                out[at] = make_float4(bx, by, bz, p.w);
            }
        }
        __syncthreads();   // the next tile's staging writes the tile
    }
}

// no component: out = (scale * s.rgb, s.w), a gain
extern "C" __global__ void __launch_bounds__(GR_GLARE_LANES) gr_glare_scale(const float4* __restrict__ source, float4* __restrict__ out, unsigned long long pixels,
                                                                              float scale) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * GR_GLARE_LANES + threadIdx.x; i < pixels; i += (unsigned long long)gridDim.x * GR_GLARE_LANES) {
        const float4 s = source[i];
        out[i] = make_float4(scale * s.x, scale * s.y, scale * s.z, s.w);
    }
}
