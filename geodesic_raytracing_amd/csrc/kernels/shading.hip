// ------------------------------------------------------------------------------------------------
// Shading: what a pixel's ray sees of the sky (the reference: render, cl.cl:5453-5846, with read_mipmap 5421-5449, the colour
// helpers 326-350 and 5366-5413, circular_diff 3598-3610).  The pixel's footprint on the sky texture is an ellipse (from the
// texture-coordinate differences to the neighbouring pixels); it is integrated by a few Gaussian-weighted trilinear probes along
// its long axis (an EWA approximation), each at the mip level of its short axis.  Written here as three pieces - the sky sampler,
// the footprint, the probe integration - around the arithmetic the golden pixels pin (tests/test_gpu_parity.py::test_render_pixels).

// The sky as the reference stores it (graphics_settings.cpp:152-212): `levels` RGBA8 slices of the full size, slice L holding mip L
// in its top-left 2^-L corner with the edge texels replicated, so that a lookup at coordinates scaled by 2^-L never leaves the mip.
// Sampling is what OpenCL's NORMALIZED | REPEAT | LINEAR sampler does on a 2D array (OpenCL 1.2, 8.2 and 8.4): wrap, texel
// centres at +0.5, the slice picked by rounding.
struct sky_sampler {
    const uchar4* __restrict__ texels;   // [levels][height][width]
    int width, height, levels;

    __device__ __forceinline__ float4 texel(int x, int y, int slice) const {
        const uchar4 t = texels[((size_t)slice * height + y) * width + x];
        const float unorm = 1.f / 255.f;
        return f4(t.x * unorm, t.y * unorm, t.z * unorm, t.w * unorm);
    }
    __device__ float4 bilinear(float u, float v, float slice_f) const {
        int slice = (int)rintf(slice_f);
        slice = slice < 0 ? 0 : (slice > levels - 1 ? levels - 1 : slice);
        const float x = (u - floorf(u)) * width - 0.5f, y = (v - floorf(v)) * height - 0.5f;
        const float x_floor = floorf(x), y_floor = floorf(y);
        int x0 = (int)x_floor, y0 = (int)y_floor, x1 = x0 + 1, y1 = y0 + 1;
        if (x0 < 0) x0 += width;
        if (x1 > width - 1) x1 -= width;
        if (y0 < 0) y0 += height;
        if (y1 > height - 1) y1 -= height;
        const float wx = x - x_floor, wy = y - y_floor;
        return ((1 - wx) * (1 - wy)) * texel(x0, y0, slice) + (wx * (1 - wy)) * texel(x1, y0, slice) +
               ((1 - wx) * wy) * texel(x0, y1, slice) + (wx * wy) * texel(x1, y1, slice);
    }
    // between the two mips around `lod`
    __device__ float4 trilinear(float2 uv, float lod) const {
        lod = __builtin_fmaxf(lod, 0.f);
        // fmod(x, 1) is x - trunc(x), and a quotient by 2^n a product with 2^-n: the same values as the reference's fmod / exp2 /
        // divide without the library routines (two probes a pixel at the least, eight at the most, each through here)
        uv.x = uv.x - __builtin_truncf(uv.x);
        uv.y = uv.y - __builtin_truncf(uv.y);
        const float fine = floorf(lod), coarse = ceilf(lod);
        const float fine_scale = __builtin_ldexpf(1.f, -(int)fine), coarse_scale = __builtin_ldexpf(1.f, -(int)coarse);
        const float4 a = bilinear(uv.x * fine_scale, uv.y * fine_scale, fine);
        const float4 b = bilinear(uv.x * coarse_scale, uv.y * coarse_scale, coarse);
        return a + (b - a) * (lod - fine);
    }
};

// Footprint of a pixel in texels: the ellipse  A u^2 + B u v + C v^2 = 1  spanned by the texture-space images of the pixel's two
// edges, each padded by one texel (the "+ 1" that keeps a vanishing footprint from collapsing), reduced to its axes.
struct sky_footprint {
    float long_radius, short_radius;
    float cos_angle, sin_angle;   // of the reference's angle = atan2(b, (a - c) / 2): the direction the probes are spaced along
};
__device__ __forceinline__ sky_footprint pixel_footprint(float2 along_x, float2 along_y) {
    const float raw_a = along_x.y * along_x.y + along_y.y * along_y.y + 1;
    const float raw_b = -2 * (along_x.x * along_x.y + along_y.x * along_y.y);
    const float raw_c = along_x.x * along_x.x + along_y.x * along_y.x + 1;
    const float norm = raw_a * raw_c - raw_b * raw_b / 4;
    const float a = raw_a / norm, b = raw_b / norm, c = raw_c / norm;
    const float spread = __builtin_sqrtf((a - c) * (a - c) + b * b);
    sky_footprint f;
    f.long_radius = 1.f / __builtin_sqrtf((a + c - spread) / 2);
    f.short_radius = 1.f / __builtin_sqrtf((a + c + spread) / 2);
    {   // cos and sin of atan2(y, x) are x / hypot and y / hypot: no angle is ever needed (atan2f + cosf + sinf were a tenth of the pass)
        const float x = (a - c) / 2, y = b;
        const float hyp = __builtin_sqrtf(x * x + y * y);
        f.cos_angle = hyp > 0.f ? x / hyp : 1.f;   // atan2(0, 0) = 0
        f.sin_angle = hyp > 0.f ? y / hyp : 0.f;
    }
    f.long_radius = __builtin_fmaxf(f.long_radius, 1.f);
    f.short_radius = __builtin_fmaxf(f.short_radius, 1.f);
    f.long_radius = __builtin_fmaxf(f.long_radius, f.short_radius);
    return f;
}

// The footprint integrated over the sky: 2 (long / short) - 1 probes, capped at `most_probes` (the short axis then grows to keep
// the long one covered), spaced along the long axis, Gaussian weights exp(-2 d^2) in units of the long radius, each probe a
// trilinear lookup at the mip level of the short axis.
__device__ float4 integrate_footprint(const sky_sampler& sky, float2 centre, sky_footprint f, int most_probes) {
    const float wanted = 2 * (f.long_radius / f.short_radius) - 1;
    int probes = (int)floorf(wanted + 0.5f);
    probes = probes < most_probes ? probes : most_probes;
    if (probes < wanted) f.short_radius = 2 * f.long_radius / (probes + 1);
    float lod = __builtin_amdgcn_logf(f.short_radius);   // v_log_f32 is log2; short_radius >= 1
    const int coarsest = sky.levels - 1;
    if (lod > coarsest) { lod = coarsest; probes = 1; }
    if (probes <= 1) {
        if (probes < 1) lod = coarsest;
        return sky.trilinear(centre, lod);
    }
    const float span = 2 * (f.long_radius - f.short_radius);
    const float step_u = f.cos_angle * span / (probes - 1), step_v = f.sin_angle * span / (probes - 1);
    const float step_u_norm = step_u / sky.width, step_v_norm = step_v / sky.height;
    const float step2 = (step_u * step_u + step_v * step_v) / (f.long_radius * f.long_radius);
    // probe k sits at (2k - (probes - 1)) half steps from the centre; an even count starts one half step further out on the
    // low side (the reference's startN, cl.cl:5641-5650)
    int half_steps = (probes % 2) == 1 ? -2 * ((probes - 1) / 2) : -2 * (probes / 2) - 1;
    float4 sum = f4(0, 0, 0, 0);
    float weight_sum = 0;
    for (int k = 0; k < probes; k++, half_steps += 2) {
        const float weight = __builtin_amdgcn_exp2f(-2.88539008177792681472f * ((half_steps * half_steps / 4.f) * step2));   // exp(-2 d^2) on v_exp_f32
        const float offset = half_steps / 2.f;
        sum = sum + weight * sky.trilinear(make_float2(centre.x + offset * step_u_norm, centre.y + offset * step_v_norm), lod);
        weight_sum += weight;
    }
    return sum / weight_sum;
}

// colour (cl.cl:326-350, 5366-5413)
// x^y for x > 0 on v_log_f32 / v_exp_f32: the colour curves take powers of values in (0, 1] with |log2 x| < 9.  The exponent
// t = y log2 x carries the rounding of the logarithm and of the product, so the error is about (2 |t| ln 2 + 2) 2^-24 of the result:
// 2e-7 for |t| < 1, 1.9e-6 at |t| = 21.6 (x = 2^-9, y = 2.4; measured 1.4e-6 with correctly rounded log2 / exp2,
// tests/test_shading_model.py).  The curves below call it above their linear toes only, |t| < 8.5: 8e-7 of a result that is small
// where |t| is large, a few 1e-7 of the frame's unit in absolute terms (the library's pow: ~100 instructions, three to six of them a pixel)
__device__ __forceinline__ float colour_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float srgb_to_linear(float v) { return v < 0.04045f ? v / 12.92f : colour_pow((v + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float linear_to_srgb(float v) { return v <= 0.0031308f ? v * 12.92f : 1.055f * colour_pow(v, 1.0f / 2.4f) - 0.055f; }
__device__ __forceinline__ float3 srgb_to_linear(float3 c) { return f3(srgb_to_linear(c.x), srgb_to_linear(c.y), srgb_to_linear(c.z)); }
__device__ __forceinline__ float3 linear_to_srgb(float3 c) { return f3(linear_to_srgb(c.x), linear_to_srgb(c.y), linear_to_srgb(c.z)); }
__device__ __forceinline__ float luminous_energy(float3 v) { return v.x * 0.2125f + v.y * 0.7154f + v.z * 0.0721f; }
__device__ __forceinline__ float3 saturate3(float3 v) { return f3(clampf(v.x, 0.f, 1.f), clampf(v.y, 0.f, 1.f), clampf(v.z, 0.f, 1.f)); }
__device__ __forceinline__ float3 blend3(float3 a, float3 b, float t) { return a + (b - a) * t; }

// A linear colour seen at redshift z: its luminance scaled as the cube of the wavelength ratio (555 nm reference), then tinted
// towards red (z > 0) or blue (z < 0) by tanh of the shift; what a blue shift pushes out of gamut is handed to red and green.
__device__ float3 apply_redshift(float3 linear, float z, dfg_t dfg) {
    const float light_speed = 299792458;
    const float reference_wavelength = 555 / light_speed;
    const float seen_wavelength = reference_wavelength / (z + 1);
    const float luminance = 0.2126f * linear.x + 0.7152f * linear.y + 0.0722f * linear.z;
    // (seen / reference)^3 as the reference writes it, pow(seen, 3) * luminance / pow(reference, 3), with the cubes multiplied out
    const float shifted_luminance = clampf((seen_wavelength * seen_wavelength * seen_wavelength) * luminance /
                                           (reference_wavelength * reference_wavelength * reference_wavelength), 0.f, 1.f);
    if ((double)luminance > 0.00001) linear = saturate3((shifted_luminance / luminance) * linear);
    const float energy = luminous_energy(linear);
    const float3 pure_red = f3(1 / 0.2125f, 0.f, 0.f), pure_green = f3(0, (float)(1 / 0.7154), 0.f), pure_blue = f3(0.f, 0.f, (float)(1 / 0.0721));
    float3 tinted;
    if (z > 0) {
        tinted = blend3(linear, energy * pure_red, tanhf(z));
    } else {
        tinted = blend3(linear, energy * pure_blue, tanhf((1 / (1 + z)) - 1));
        if (!GET_FEATURE(use_old_redshift, dfg)) {
            const float lost = luminous_energy(tinted) - luminous_energy(saturate3(tinted));
            tinted.x += lost * (pure_red.x + pure_green.x);
            tinted.y += lost * (pure_red.y + pure_green.y);
        }
    }
    return saturate3(saturate3(tinted));
}

// b - a for texture coordinates that wrap with period 1, through the angle they stand for (mixed double / float as the
// reference evaluates it, cl.cl:3598-3604)
__device__ __forceinline__ float wrapped_difference(float a, float b) {
    const float angle_a = (float)((double)a * (2 * GR_PI / (double)1.f));
    const float angle_b = (float)((double)b * (2 * GR_PI / (double)1.f));
    const float d = angle_b - angle_a;
    // atan2(sin d, cos d) is d brought into (-pi, pi]: for the differences between neighbouring pixels that is d itself, across the
    // texture's seam one turn is taken off.  (The library's sin, cos and atan2 here - four differences a pixel - were 400 of the
    // pass's ~1 000 vector instructions per pixel.)
    // One value takes neither road: |d| = float(pi) exactly - a record in the equatorial plane (v = 0.5) next to a black one (0, 0), i.e.
    // the shadow's edge on the middle row of a frame with an even number of rows.  float(pi) lies 8.7e-8 beyond pi, so sin d has the
    // sign opposite to d's and atan2(sin d, cos d) is the float below pi with the OTHER sign: the footprint's long axis is mirrored
    // (found by the round-5 fixture kerr_max_probes_16, one pixel off by 2e-2; invisible with up to 8 probes on the odd-rowed fixtures).
    const float two_pi = 6.283185307179586f, pi_f = 3.14159274101257324f, below_pi = 3.14159250259399414f;
    float wrapped = __builtin_fabsf(d) <= pi_f ? d : d - two_pi * __builtin_rintf(d / two_pi);
    if (__builtin_fabsf(d) == pi_f) wrapped = d > 0 ? -below_pi : below_pi;
    return (float)((double)(1.f * wrapped) / (2 * GR_PI));
}

// The colour tail every sky ends in, for a colour in linear light: the redshift where the feature is on, then the frame's coding
// (sRGB unless LINEAR_FRAMEBUFFER)
__device__ __forceinline__ float3 finish_linear_colour(float3 linear, float z_shift, dfg_t dfg) {
    if (GET_FEATURE(redshift, dfg)) linear = apply_redshift(linear, z_shift, dfg);
#ifndef LINEAR_FRAMEBUFFER
    linear = linear_to_srgb(linear);
#endif
    return linear;
}
// ... and for an sRGB-coded colour (a texel, a colour of the C ABI): decoded for the tail, or passed through untouched where neither
// the redshift nor the frame wants linear light
__device__ __forceinline__ float3 finish_srgb_colour(float3 srgb, float z_shift, dfg_t dfg) {
    if (GET_FEATURE(redshift, dfg)) return finish_linear_colour(srgb_to_linear(srgb), z_shift, dfg);
#ifdef LINEAR_FRAMEBUFFER
    return srgb_to_linear(srgb);
#else
    return srgb;
#endif
}

// Half the footprint's size along u and v (x, y of the result) for the skies that integrate over a box: the mean size of the
// differences to the two neighbours, no smaller than `floor`.  Only sizes enter, so a previous neighbour (last column / row) needs no sign.
__device__ __forceinline__ float2 footprint_half_sizes(const render_data& self, float2 beside, float2 below, float floor) {
    const float u = self.tex_coord.x, v = self.tex_coord.y;
    return make_float2(__builtin_fmaxf(0.5f * (__builtin_fabsf(wrapped_difference(u, beside.x)) + __builtin_fabsf(wrapped_difference(u, below.x))), floor),
                       __builtin_fmaxf(0.5f * (__builtin_fabsf(wrapped_difference(v, beside.y)) + __builtin_fabsf(wrapped_difference(v, below.y))), floor));
}

// One pixel: `self` is its record, `beside` / `below` the texture coordinates of its horizontal / vertical neighbour - the next
// pixel, or the previous one at the last column / row (`beside_is_previous`, `below_is_previous`), cl.cl:5509-5546.
__device__ float4 shade_pixel(const render_data& self, float2 beside, bool beside_is_previous, float2 below, bool below_is_previous,
                              const sky_sampler& near_sky, const sky_sampler& far_sky, int most_probes, dfg_t dfg) {
    if (self.terminated != 1) return f4(0, 0, 0, 1);
    const sky_sampler& sky = self.side >= 1 ? near_sky : far_sky;   // which side of a wormhole the ray ended on
    const float shrink = 1.3f;   // the reference's filter bias
    float2 along_x = make_float2(wrapped_difference(self.tex_coord.x, beside.x) / shrink, wrapped_difference(self.tex_coord.y, beside.y) / shrink);
    float2 along_y = make_float2(wrapped_difference(self.tex_coord.x, below.x) / shrink, wrapped_difference(self.tex_coord.y, below.y) / shrink);
    if (beside_is_previous) { along_x.x = -along_x.x; along_x.y = -along_x.y; }
    if (below_is_previous) { along_y.x = -along_y.x; along_y.y = -along_y.y; }
    along_x.x *= sky.width; along_y.x *= sky.width;
    along_x.y *= sky.height; along_y.y *= sky.height;
    float4 colour = integrate_footprint(sky, self.tex_coord, pixel_footprint(along_x, along_y), most_probes);
    const float3 rgb = finish_srgb_colour(f3(colour.x, colour.y, colour.z), self.z_shift, dfg);
    return f4(rgb.x, rgb.y, rgb.z, colour.w);
}

__device__ __attribute__((noinline)) float4 shade_pixel_in_tile(const render_data& self, float2 beside, float2 below, const trace_shading& shading, dfg_t dfg) {
    const sky_sampler near_sky{shading.bg1_texels, shading.bg_width, shading.bg_height, shading.bg_levels},
                      far_sky{shading.bg2_texels, shading.bg_width, shading.bg_height, shading.bg_levels};
    return shade_pixel(self, beside, false, below, false, near_sky, far_sky, shading.most_probes, dfg);
}

#if GR_FRAME_KERNELS
// What a work item of a shading launch shades: the launch contract of gr_render, gr_render_analytic and gr_render_stars alike.
// The launch of the reference (num_pixels = block_pixels = width * height, strip_rank 0, strip_count 1, compact_out 0) shades the
// whole image; the extension shades one device's row blocks of a split image: work item gid is pixel `off` of local block `lb`,
// the global block being lb * strip_count + strip_rank, and with compact_out the device's blocks are written back to back.
// An item with work ends in shade(self, out_index, beside, below, last_column, last_row), the neighbours as shade_pixel takes them.
// (The shader is handed in, not a flag handed back: a flag tested after the call stays a lane mask in the compiled kernels, which grow.)
// A kernel without seams passes a literal 0 for seams_only and that branch folds away.
template <class Shade>
__device__ __forceinline__ void shading_work_item(int num_pixels, int block_pixels, int strip_rank, int strip_count, int compact_out, int seams_only,
                                                  const render_data* __restrict__ rdata, const int* __restrict__ rdata_count, int width, int height,
                                                  Shade shade) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= num_pixels) return;
    int lb, off;
    if (seams_only) {
        // the pixels a fused trace launch left (trace_shading): last column and last row of every 8x8 tile, 15 work items per tile,
        // tiles numbered block by block as the trace numbers them.  Records are indexed by pixel; width is a multiple of 8.
        const int tiles_x = width / GR_TILE, tiles_per_block = tiles_x * (block_pixels / width / GR_TILE);
        const int tile = gid / 15, k = gid - tile * 15;
        lb = tile / tiles_per_block;
        const int within = tile - lb * tiles_per_block;
        const int x = (within % tiles_x) * GR_TILE + (k < GR_TILE ? GR_TILE - 1 : k - GR_TILE);
        const int y = (within / tiles_x) * GR_TILE + (k < GR_TILE ? k : GR_TILE - 1);
        off = y * width + x;
    } else {
        lb = gid / block_pixels;
        off = gid - lb * block_pixels;
    }
    const int id = (lb * strip_count + strip_rank) * block_pixels + off;
    if (id >= *rdata_count || id >= width * height) return;
    const render_data self = rdata[id];
    const int px = self.sx, py = self.sy;
    const int out_index = compact_out ? lb * block_pixels + off : py * width + px;
    const bool last_column = px == width - 1, last_row = py == height - 1;
    float2 beside = make_float2(0, 0), below = make_float2(0, 0);
    if (self.terminated == 1) {
        // a frame one pixel wide (high) has no horizontal (vertical) neighbour: the pixel stands in for it, the difference is zero
        // and the footprint is the one-texel padding (the reference reads the record before the buffer there)
        beside = rdata[py * width + px + (last_column ? (width > 1 ? -1 : 0) : 1)].tex_coord;
        below = rdata[(py + (last_row ? (height > 1 ? -1 : 0) : 1)) * width + px].tex_coord;
    }
    shade(self, out_index, beside, below, last_column, last_row);
}

extern "C" __global__ void gr_render(const render_data* __restrict__ rdata, const int* __restrict__ rdata_count, float4* __restrict__ out,
                                     const uchar4* __restrict__ bg1_texels, const uchar4* __restrict__ bg2_texels,
                                     int bg_width, int bg_height, int bg_levels,
                                     int width, int height, int most_probes, cfg_t cfg, dfg_t dfg,
                                     int num_pixels, int block_pixels, int strip_rank, int strip_count, int compact_out, int seams_only) {
    shading_work_item(num_pixels, block_pixels, strip_rank, strip_count, compact_out, seams_only, rdata, rdata_count, width, height,
                      [&](const render_data& self, int out_index, float2 beside, float2 below, bool last_column, bool last_row) __attribute__((always_inline)) {
        const sky_sampler near_sky{bg1_texels, bg_width, bg_height, bg_levels}, far_sky{bg2_texels, bg_width, bg_height, bg_levels};
        out[out_index] = shade_pixel(self, beside, last_column, below, last_row, near_sky, far_sky, most_probes, dfg);
    });
    (void)cfg;
}

// ------------------------------------------------------------------------------------------------
// The analytic sky (no reference counterpart; defined in include/geodesic_hip_internal.h, "Analytic sky"): a coloured celestial sphere
// with a latitude / longitude grid, integrated in closed form over a box the size of the pixel's footprint - no texels, no mips.
// gr_analytic_sky of the C ABI, field for field; it travels in the kernel's argument block, and every index into it below is a
// constant (a colour of the side a ray ended on is a select between two scalars, never an indexed copy in scratch).
struct analytic_sky {
    int meridians, parallels;
    float line_width;
    float quadrant[2][4][3];
    float line[2][3];
};

// The share of [x - h, x + h] that the lines of a pulse train cover: n cells to the unit, a line of width w (in cells) centred on
// every cell boundary.  Only the fraction of t = x n matters, and it comes from the exact product: in double, which holds it whole
// and which the build's contraction and reassociation cannot hurt (they fold the fp32 pair x n, fma(x, n, -(x n)) into one rounding
// and its low part counted twice); one rounding to fp32, the same value the pair gives under IEEE rules.  The integer parts of the
// two ends are differenced before they meet w: the error is a few ulps of a cell, not of n cells.
__device__ __forceinline__ float line_coverage(float x, float h, int n, float w) {
    const float cells = (float)n;
    const double t_exact = (double)x * (double)n;
    const float t = (float)(t_exact - __builtin_floor(t_exact));
    const float a = h * cells, half_line = 0.5f * w;
    const float s_upper = t + (a + half_line), s_lower = t - (a - half_line);
    const float k_upper = __builtin_floorf(s_upper), k_lower = __builtin_floorf(s_lower);
    const float covered = (k_upper - k_lower) * w + (__builtin_fminf(s_upper - k_upper, w) - __builtin_fminf(s_lower - k_lower, w));
    return covered / (2.f * a);
}

// ... and the share that lies in the upper half of a unit: of every unit for u (the sphere closes), of the one unit for v
__device__ __forceinline__ float upper_half_share(float x, float h, bool periodic) {
    const float upper = x + h, lower = x - h;
    const float k_upper = periodic ? __builtin_floorf(upper) : 0.f, k_lower = periodic ? __builtin_floorf(lower) : 0.f;
    const float inside = 0.5f * (k_upper - k_lower) + (__builtin_fmaxf((upper - k_upper) - 0.5f, 0.f) - __builtin_fmaxf((lower - k_lower) - 0.5f, 0.f));
    return inside / (2.f * h);
}

// One pixel: `self`, `beside` and `below` as shade_pixel takes them
__device__ __forceinline__ float4 shade_pixel_analytic(const render_data& self, float2 beside, float2 below, const analytic_sky& sky, dfg_t dfg) {
    if (self.terminated != 1) return f4(0, 0, 0, 1);
    const float floor_h = 6.103515625e-05f;   // 2^-14: keeps the result a continuous function of the record
    const float2 half = footprint_half_sizes(self, beside, below, floor_h);
    const float hu = half.x, hv = half.y;
    const float u = self.tex_coord.x, v = self.tex_coord.y;
    const float cu = line_coverage(u, hu, sky.meridians, sky.line_width), cv = line_coverage(v, hv, sky.parallels, sky.line_width);
    const float grid = 1.f - (1.f - cu) * (1.f - cv);
    const float fu = upper_half_share(u, hu, true), fv = upper_half_share(v, hv, false);
    const float w0 = (1.f - fu) * (1.f - fv), w1 = fu * (1.f - fv), w2 = (1.f - fu) * fv, w3 = fu * fv;
    const bool near_side = self.side >= 1;   // which side of a wormhole the ray ended on, as shade_pixel picks bg1 / bg2
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float q0 = near_side ? sky.quadrant[1][0][k] : sky.quadrant[0][0][k], q1 = near_side ? sky.quadrant[1][1][k] : sky.quadrant[0][1][k];
        const float q2 = near_side ? sky.quadrant[1][2][k] : sky.quadrant[0][2][k], q3 = near_side ? sky.quadrant[1][3][k] : sky.quadrant[0][3][k];
        const float line = near_side ? sky.line[1][k] : sky.line[0][k];
        const float base = w0 * q0 + w1 * q1 + w2 * q2 + w3 * q3;
        c[k] = base + (line - base) * grid;
    }
    const float3 rgb = finish_srgb_colour(f3(c[0], c[1], c[2]), self.z_shift, dfg);
    return f4(rgb.x, rgb.y, rgb.z, 1.f);
}

// shading_work_item's launch with the sky's description in place of the textures (and no seams_only: a frame with an analytic sky
// is never shaded inside the trace)
extern "C" __global__ void gr_render_analytic(const render_data* __restrict__ rdata, const int* __restrict__ rdata_count, float4* __restrict__ out,
                                              analytic_sky sky, int width, int height, cfg_t cfg, dfg_t dfg,
                                              int num_pixels, int block_pixels, int strip_rank, int strip_count, int compact_out) {
    shading_work_item(num_pixels, block_pixels, strip_rank, strip_count, compact_out, 0, rdata, rdata_count, width, height,
                      [&](const render_data& self, int out_index, float2 beside, float2 below, bool last_column, bool last_row) __attribute__((always_inline)) {
        out[out_index] = shade_pixel_analytic(self, beside, below, sky, dfg);
    });
    (void)cfg;
}

// ------------------------------------------------------------------------------------------------
// The star sky (no reference counterpart; defined in include/geodesic_hip_internal.h, "Star sky"): point stars gathered from a catalogue
// that kernels/stars.hip built - cell_start[cells + 1], the stars' records cell by cell (two float4 a star: u, v, r, g | b), and a
// float64 summed-area table of the cells' flux.  A pixel whose footprint spans at most 4 x 4 cells (NEAR) sums tents over the stars
// themselves; a wider one (FAR) takes the box integral of the table.  gr_star_sky and a view of each side's catalogue travel in the
// kernel's argument block (a NULL catalogue: n = 0 and no pointers).
struct star_sky {
    float min_footprint;
    float background[2][3];
};
struct star_catalogue_view {
    const int* cell_start;
    const float4* stars;
    const double* table;
    int n, cells_u, cells_v;
};

// NEAR, step 3: the sum of flux x tent x tent, not yet divided by the footprint's area.  The cells i0 ... i1 of a row are one run of
// consecutive cells, or two where the run crosses the seam of u (cells are taken modulo cells_u, a power of two), and the stars of a
// run of cells are one run of records: cell_start of its first cell to cell_start behind its last - four loads a row, issued together
// ahead of the stars.  A run `turn` turns away from the pixel has its stars at u_s + turn: the difference is formed as (u_s - a) - b
// with (a, b) = (0, u), (1, u) for turn -1 (u_s - 1 is exact for a star in front of the seam) or (0, u - 1) for turn +1 (u - 1 is
// exact for a pixel there), and the pragma keeps the two subtractions apart: folded into u_s - (a + b) they would round a position
// against the turn, 2^-24 of a tent that may be 2^-19 wide.  Per star: those two, v_s - v, two tents and three multiply-adds.
__device__ __forceinline__ float3 star_sum_near(const star_catalogue_view& cat, float u, float v, float hu, float hv, int i0, int i1, int j0, int j1) {
#pragma clang fp reassociate(off)
    const float inverse_u = 1.f / (2.f * hu), inverse_v = 1.f / (2.f * hv);
    const int shift = 31 - __builtin_clz(cat.cells_u), mask = cat.cells_u - 1;
    const int seam = ((i0 >> shift) + 1) << shift;        // the first cell of the next turn
    const int last = min(i1, seam - 1);
    const bool two_runs = i1 >= seam;
    const int turn = i0 >> shift;                          // of the first run: -1, 0 (or 1 for u = 1); the second run is one further
    const float a0 = turn < 0 ? 1.f : 0.f, b0 = turn > 0 ? u - 1.f : u;
    const float a1 = turn + 1 < 0 ? 1.f : 0.f, b1 = turn + 1 > 0 ? u - 1.f : u;
    float r = 0.f, g = 0.f, b = 0.f;
    for (int j = max(j0, 0); j <= min(j1, cat.cells_v - 1); j++) {
        const int* row = cat.cell_start + j * cat.cells_u;
        const int begin0 = row[i0 & mask], end0 = row[(last & mask) + 1];
        const int begin1 = two_runs ? row[0] : 0, end1 = two_runs ? row[(i1 & mask) + 1] : 0;
#pragma unroll
        for (int run = 0; run < 2; run++) {
            const int begin = run ? begin1 : begin0, end = min(run ? end1 : end0, cat.n);
            const float a = run ? a1 : a0, from = run ? b1 : b0;
            for (int s = max(begin, 0); s < end; s++) {
                const float4 first = cat.stars[2 * s], second = cat.stars[2 * s + 1];
                const float du = (first.x - a) - from, dv = first.y - v;
                const float tent_u = __builtin_fmaxf(1.f - __builtin_fabsf(du) * inverse_u, 0.f), tent_v = __builtin_fmaxf(1.f - __builtin_fabsf(dv) * inverse_v, 0.f);
                const float weight = tent_u * tent_v;
                r += first.z * weight;
                g += first.w * weight;
                b += second.x * weight;
            }
        }
    }
    return f3(r, g, b);
}

// I(x, y) of step 4 for one channel's plane, x in [-1, 2], y in [0, 1]
__device__ __forceinline__ double star_table_at(const double* plane, int cells_u, int cells_v, double x, double y) {
    const double turns = __builtin_floor(x);
    const double X = (x - turns) * cells_u, Y = y * cells_v;
    const int i = min(max((int)X, 0), cells_u - 1), j = min(max((int)Y, 0), cells_v - 1);
    const double a = X - i, b = Y - j;
    const double* lower = plane + (size_t)j * (cells_u + 1);
    const double* upper = lower + (cells_u + 1);
    const double inside = (1 - a) * (1 - b) * lower[i] + a * (1 - b) * lower[i + 1] + (1 - a) * b * upper[i] + a * b * upper[i + 1];
    return inside + turns * ((1 - b) * lower[cells_u] + b * upper[cells_u]);
}

// FAR, step 4: the stars as a glow, in double (the four terms cancel), already divided by the footprint's area.  Few pixels come
// here.  A channel at a time, so that sixteen doubles are in flight and not forty-eight.  Inlined on purpose: as a noinline function
// the kernel took the callee's registers anyway (120 VGPRs against 108) and 84 bytes of scratch for what it keeps across the call.
__device__ __forceinline__ float3 star_glow_far(const double* table, int cells_u, int cells_v, float u, float v, float hu, float hv) {
    const double left = (double)u - (double)hu, right = (double)u + (double)hu;
    const double v0 = __builtin_fmax((double)v - (double)hv, 0.0), v1 = __builtin_fmin((double)v + (double)hv, 1.0);
    const double area = 4.0 * (double)hu * (double)hv;
    const size_t plane = (size_t)(cells_v + 1) * (size_t)(cells_u + 1);
    float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll 1   // a channel at a time: sixteen doubles in flight, not forty-eight
    for (int k = 0; k < 3; k++) {
        const double* t = table + k * plane;
        const double sum = star_table_at(t, cells_u, cells_v, right, v1) - star_table_at(t, cells_u, cells_v, left, v1) -
                           star_table_at(t, cells_u, cells_v, right, v0) + star_table_at(t, cells_u, cells_v, left, v0);
        const float value = (float)(sum / area);
        r = k == 0 ? value : r;
        g = k == 1 ? value : g;
        b = k == 2 ? value : b;
    }
    return f3(r, g, b);
}

// One pixel: `self`, `beside` and `below` as shade_pixel_analytic takes them
__device__ __forceinline__ float4 shade_pixel_stars(const render_data& self, float2 beside, float2 below, const star_sky& sky, const star_catalogue_view& near_stars,
                                                    const star_catalogue_view& far_stars, dfg_t dfg) {
    if (self.terminated != 1) return f4(0, 0, 0, 1);
    const float u = self.tex_coord.x, v = self.tex_coord.y;
    const float2 half = footprint_half_sizes(self, beside, below, sky.min_footprint);
    const float hu = half.x, hv = half.y;
    const bool near_side = self.side >= 1;   // which side of a wormhole the ray ended on, as shade_pixel picks bg1 / bg2
    const star_catalogue_view cat = near_side ? near_stars : far_stars;
    float3 stars = f3(0.f, 0.f, 0.f);
    if (cat.n > 0) {
        // step 2: single IEEE operations and multiplications by powers of two - what contraction makes of them is the same value.  The
        // clamp only keeps a coordinate that is no coordinate (not finite) from overflowing the conversion.
        const float margin = 2.384185791015625e-07f;   // 2^-22
        const float reach_u = 2.f * hu + margin, reach_v = 2.f * hv + margin;
        const float cells_u = (float)cat.cells_u, cells_v = (float)cat.cells_v, most = 16777216.f;
        const int i0 = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf((u - reach_u) * cells_u), -most), most);
        const int i1 = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf((u + reach_u) * cells_u), -most), most);
        const int j0 = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf((v - reach_v) * cells_v), -most), most);
        const int j1 = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf((v + reach_v) * cells_v), -most), most);
        if (i1 - i0 <= 3 && j1 - j0 <= 3) {
            const float3 sum = star_sum_near(cat, u, v, hu, hv, i0, i1, j0, j1);
            const float per_area = 1.f / (4.f * hu * hv);
            stars = f3(sum.x * per_area, sum.y * per_area, sum.z * per_area);
        } else {
            stars = star_glow_far(cat.table, cat.cells_u, cat.cells_v, u, v, hu, hv);
        }
    }
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = srgb_to_linear(near_side ? sky.background[1][k] : sky.background[0][k]);
    const float3 rgb = finish_linear_colour(f3(c[0] + stars.x, c[1] + stars.y, c[2] + stars.z), self.z_shift, dfg);   // (the sum is in linear light already)
    return f4(rgb.x, rgb.y, rgb.z, 1.f);
}

// gr_render_analytic's launch with the star sky and the two catalogues in place of the analytic sky
extern "C" __global__ void gr_render_stars(const render_data* __restrict__ rdata, const int* __restrict__ rdata_count, float4* __restrict__ out,
                                           star_sky sky, star_catalogue_view near_stars, star_catalogue_view far_stars, int width, int height,
                                           cfg_t cfg, dfg_t dfg, int num_pixels, int block_pixels, int strip_rank, int strip_count, int compact_out) {
    shading_work_item(num_pixels, block_pixels, strip_rank, strip_count, compact_out, 0, rdata, rdata_count, width, height,
                      [&](const render_data& self, int out_index, float2 beside, float2 below, bool last_column, bool last_row) __attribute__((always_inline)) {
        out[out_index] = shade_pixel_stars(self, beside, below, sky, near_stars, far_stars, dfg);
    });
    (void)cfg;
}
#endif  // GR_FRAME_KERNELS

