// ------------------------------------------------------------------------------------------------
// background.hip - the sky's mip slices, made on the device.  The reference hands its sky to the GL driver, which makes the mip chain on the
// GPU (graphics_settings.cpp:152-243); the host states it in capi.cpp (gr_pack_mipped_background: `levels` full-size slices, slice l the
// l-th level of a 2 x 2 box chain, edge-replicated).  The two kernels here write the same bytes from an RGBA8 image that is already on the
// device.  Part of the set-up module (capi.cpp: compile_setup_module): IEEE divide, no contraction, no re-association - every sum below is
// taken in the order it is written, which is the host's.
//
// What the host function computes, restated (tests/test_background_abi.py checks this restatement against the host function on the CPU):
//   levels = min(floor(log2(min(w, h))) + 1, 10);  level 0 = byte / 255.f;  level l is (w >> l) x (h >> l) and its texel (x, y) is
//   0.25f * (((c00 + c01) + c10) + c11) of the texels (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1) of level l - 1, in float,
//   never re-quantised;  slice l, texel (x, y) = level l at (min(x, cw - 1), min(y, ch - 1)), clamped to [0, 1], (unsigned char)(v * 255).
// Two things the host writes differently and why they are the same:
//   * its size max(cw / 2, 1): l <= levels - 1 <= floor(log2(min(w, h))), so min(w, h) >> l >= 1 for every level made - a dimension never
//     halves below 1, the max never binds, and level l is (w >> l) x (h >> l) because floor(floor(n / 2) / 2) = floor(n / 4);
//   * its clamps min(2x + 1, cw - 1): x < nw = floor(cw / 2) gives 2x + 1 <= 2 floor(cw / 2) - 1 <= cw - 1, so they never bind either.  An
//     odd last column or row of a level is simply never read, and texel (x, y) of level l is the tree reduction of the base block
//     [x 2^l, (x + 1) 2^l) x [y 2^l, (y + 1) 2^l) - a workgroup that holds a 32 x 32 block of level l therefore holds everything its
//     16 x 16, 8 x 8 ... 1 x 1 texels of the next five levels are made of.  A texel of level l + k exists when its index is below
//     (w >> (l + k), h >> (l + k)), and if it does its four children do (2X + 1 <= cw - 1 again): a validity test per level, no neighbour's data.
//   * slice 0: (unsigned char)((k / 255.f) * 255) == k for all 256 k (checked in the test on the CPU and on the device), so it is the image.
//
// gr_background_reduce - the float levels.  One workgroup of 16 x 16 lanes per 32 x 32 texels of the source level (level 0: the image's
// bytes; later: float4 of the pyramid): a lane reads its 2 x 2 block, writes one texel of the next level and leaves it in LDS, where the
// workgroup goes on to 8 x 8, 4 x 4, 2 x 2 and 1 x 1 - up to five levels a launch, so a ten-level chain is two launches (0 -> 1 ... 5,
// 5 -> 6 ... 9) instead of nine.  Levels >= 1 are kept as float4 in a pyramid the caller supplies (level 1 first, levels back to back):
// they cannot be bytes, the host never re-quantises.  The byte becomes a float by the IEEE divide the module is built with, the host's
// own operation; a table of 256 bit patterns would save ~10 instructions a channel in a launch that is bound by its 16-byte stores.
// This launch moves little: it reads w h 4 bytes and writes about a third more than that in float4; the slice writer moves `levels` times
// the image.  So it is kept plain: two 4-byte loads per lane and source row (an odd width leaves a row only 4-byte aligned; a wave's
// 16 lanes of a row still cover 128 contiguous bytes), float4 in LDS read at a stride of two (bank conflicts in a step that touches
// 4 KiB a workgroup).  Lanes without a texel carry zeros through LDS and store nothing; nobody leaves before the last barrier.
//
// gr_background_slices - the bytes.  One launch over all levels * h * w texels as ONE flat array: a lane makes four consecutive texels
// and writes them with one 16-byte store.  Per row that would break on an odd width (rows, and slices, then start at any multiple of 4
// bytes); the flat array keeps the store aligned whatever the size, and a lane decodes (level, y, x) once - the level by at most nine
// compares, one 32-bit divide for the row - and steps from texel to texel by carry.  Slice 0 copies the image (or, built in place -
// the image was uploaded into slice 0 - is not touched: such texels are not stored, not even with their own value).  Slices >= 1 read the
// pyramid: a wave reads 4 KiB contiguously where the level has texels of its own, and the same few texels - one line, broadcast - in
// the replicated region, which is three quarters of slice 1 and nearly all of the later ones.  Only the last lane of the array and a
// lane that straddles slice 0's end in an in-place build store texel by texel.  All indices are 64-bit: a 16384 x 8192 sky packs to 5.4 GB.

__device__ __forceinline__ float4 background_quarter_sum(const float4 c00, const float4 c01, const float4 c10, const float4 c11) {
    return make_float4(0.25f * (((c00.x + c01.x) + c10.x) + c11.x), 0.25f * (((c00.y + c01.y) + c10.y) + c11.y),
                       0.25f * (((c00.z + c01.z) + c10.z) + c11.z), 0.25f * (((c00.w + c01.w) + c10.w) + c11.w));
}

// bytes R, G, B, A in memory order
__device__ __forceinline__ float4 background_texel_of_bytes(unsigned int rgba) {
    return make_float4((float)(rgba & 255u) / 255.f, (float)((rgba >> 8) & 255u) / 255.f, (float)((rgba >> 16) & 255u) / 255.f, (float)(rgba >> 24) / 255.f);
}

__device__ __forceinline__ unsigned int background_byte_of(float v) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return (unsigned int)(v * 255.f);
}

// where level `level` (>= 1) starts in the pyramid, in texels
__device__ __forceinline__ size_t background_level_start(int width, int height, int level) {
    size_t at = 0;
    for (int k = 1; k < level; k++) at += (size_t)(width >> k) * (size_t)(height >> k);
    return at;
}

// levels source_level + 1 ... source_level + count (1 <= count <= 5) from level source_level; grid: 32 x 32 tiles of the source level that
// hold a texel of level source_level + 1, workgroup 16 x 16
extern "C" __global__ void __launch_bounds__(256) gr_background_reduce(const unsigned int* __restrict__ image, float4* pyramid, int width,
                                                                       int height, int source_level, int count) {
    __shared__ float4 tile[2][256];
    const int tx = threadIdx.x, ty = threadIdx.y, id = ty * 16 + tx;
    const int cw = width >> source_level, ch = height >> source_level;
    int nw = cw >> 1, nh = ch >> 1;
    size_t out_at = background_level_start(width, height, source_level + 1);
    {
        const int x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x < nw && y < nh) {
            const size_t upper = (size_t)(2 * y) * cw + 2 * x, lower = upper + cw;
            if (source_level == 0) {
                v = background_quarter_sum(background_texel_of_bytes(image[upper]), background_texel_of_bytes(image[upper + 1]),
                                           background_texel_of_bytes(image[lower]), background_texel_of_bytes(image[lower + 1]));
            } else {
                const float4* source = pyramid + background_level_start(width, height, source_level);
                v = background_quarter_sum(source[upper], source[upper + 1], source[lower], source[lower + 1]);
            }
            pyramid[out_at + (size_t)y * nw + x] = v;
        }
        tile[0][id] = v;
    }
    int side = 16, from = 0;
    for (int k = 2; k <= count; k++) {
        __syncthreads();   // the level below is in tile[from]; every read of tile[from ^ 1] was made before the barrier of the step before
        out_at += (size_t)nw * nh;
        nw >>= 1;
        nh >>= 1;
        const int half = side >> 1;
        if (id < half * half) {
            const int lx = id % half, ly = id / half;
            const float4* below = &tile[from][(2 * ly) * side + 2 * lx];
            const float4 v = background_quarter_sum(below[0], below[1], below[side], below[side + 1]);
            const int x = blockIdx.x * half + lx, y = blockIdx.y * half + ly;
            if (x < nw && y < nh) pyramid[out_at + (size_t)y * nw + x] = v;
            tile[from ^ 1][id] = v;   // (id = ly * half + lx)
        }
        side = half;
        from ^= 1;
    }
}

// packed: levels slices of width x height texels, one uint32 a texel; grid: ceil(levels * width * height / 4 / 256) workgroups of 256
extern "C" __global__ void __launch_bounds__(256) gr_background_slices(const unsigned int* image, const float4* __restrict__ pyramid,
                                                                       unsigned int* packed, int width, int height, int levels, int in_place) {
    const unsigned long long slice = (unsigned long long)width * (unsigned long long)height;   // < 2^31 (the launcher's check)
    const unsigned long long total = slice * (unsigned long long)levels;
    const unsigned long long first = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    if (first >= total) return;
    int level = 0;
    unsigned long long slice_start = 0;
    while (first - slice_start >= slice) {
        slice_start += slice;
        level++;
    }
    size_t level_at = level >= 1 ? background_level_start(width, height, level) : 0;
    const unsigned int within = (unsigned int)(first - slice_start);
    unsigned int y = within / (unsigned int)width, x = within - y * (unsigned int)width;
    unsigned int texel[4] = {0u, 0u, 0u, 0u};
    unsigned int stored = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (first + j >= total) break;
        if (level == 0) {
            if (!in_place) {
                texel[j] = image[(size_t)y * width + x];
                stored |= 1u << j;
            }
        } else {
            const unsigned int cw = (unsigned int)(width >> level), ch = (unsigned int)(height >> level);
            const unsigned int lx = x < cw ? x : cw - 1u, ly = y < ch ? y : ch - 1u;
            const float4 v = pyramid[level_at + (size_t)ly * cw + lx];
            texel[j] = background_byte_of(v.x) | (background_byte_of(v.y) << 8) | (background_byte_of(v.z) << 16) | (background_byte_of(v.w) << 24);
            stored |= 1u << j;
        }
        if (++x == (unsigned int)width) {
            x = 0;
            if (++y == (unsigned int)height) {
                y = 0;
                if (level >= 1) level_at += (size_t)(width >> level) * (size_t)(height >> level);
                level++;
            }
        }
    }
    if (stored == 15u) {
        *reinterpret_cast<uint4*>(packed + first) = make_uint4(texel[0], texel[1], texel[2], texel[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (stored & (1u << j)) packed[first + j] = texel[j];
    }
}
