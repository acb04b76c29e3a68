// shading.cpp — the host half of kernels/shading.hip: the launchers of its three kernels on one geometry and one launch, and the analytic
// sky's default, check and host rasteriser (geodesic_hip_internal.h, "Analytic sky").  The star sky's catalogue and check: star_catalogue.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "internal.hpp"

using gr_internal::blocks, gr_internal::launch, gr_internal::refuse;

namespace {

// What a shading launch hands shading_work_item of kernels/shading.hip (the launch contract is stated there): `num` work items, 256 to a workgroup
struct shading_geometry {
    int num, block_pixels, rank, count, compact, seams_only;
    const void* rdata_count;
};

// the whole frame, as the reference launches it: one block of all the pixels
shading_geometry whole_frame(int num_pixels, const void* rdata_count) { return {num_pixels, num_pixels > 0 ? num_pixels : 1, 0, 1, 0, 0, rdata_count}; }

// strip mode: this device's row blocks, block-cyclic; render_data is indexed by pixel (no count: the program's INT_MAX; a NULL program: launch() refuses it)
int strips_of_frame(const char* who, const gr_program* p, int width, int height, int block_rows, int rank, int count, int compact, shading_geometry& g) {
    if (block_rows <= 0 || count <= 0 || rank < 0 || rank >= count) return refuse(who, "bad strip parameters");
    const int block_pixels = block_rows * width;
    g = {gr_strip_local_blocks(height, block_rows, rank, count) * block_pixels, block_pixels, rank, count, compact, 0, p ? gr_internal::no_count_of(p) : nullptr};
    return GR_OK;
}

// the pixels gr_trace_fused_launch's in-tile shading leaves: last column and last row of every 8x8 tile of this device's blocks, 15 work items a tile
int seams_of_frame(const char* who, const gr_program* p, int width, int height, int block_rows, int rank, int count, int compact, shading_geometry& g) {
    if (count <= 1) { count = 1; rank = 0; block_rows = ((height + 7) / 8) * 8; }
    if (block_rows <= 0 || block_rows % 8 != 0 || rank < 0 || rank >= count || width <= 0 || width % 8 != 0)
        return refuse(who, "width and block_rows must be multiples of 8");
    const long long items = (long long)gr_strip_local_blocks(height, block_rows, rank, count) * (width / 8) * (block_rows / 8) * 15;
    if (items > 0x7fffffff) return refuse(who, "image too large");
    g = {(int)items, block_rows * width, rank, count, compact, 1, p ? gr_internal::no_count_of(p) : nullptr};
    return GR_OK;
}

// One launch of shading kernel k: the argument block in the kernel's order - records, count, frame; `sky`, what this kernel takes in
// place of the others' sky; the frame's size (gr_render: and its probe cap); cfg, dfg; the geometry (gr_render: and seams_only).
int launch_shading(int k, gr_program* p, void* stream, const void* rdata, void* out, std::initializer_list<void*> sky, int width, int height,
                   int max_probes, const void* cfg, const void* dfg, shading_geometry g) {
    void* args[24];
    int n = 0;
    for (void* a : {(void*)&rdata, (void*)&g.rdata_count, (void*)&out}) args[n++] = a;
    for (void* a : sky) args[n++] = a;
    args[n++] = &width, args[n++] = &height;
    if (k == K_RENDER) args[n++] = &max_probes;
    for (void* a : {(void*)&cfg, (void*)&dfg, (void*)&g.num, (void*)&g.block_pixels, (void*)&g.rank, (void*)&g.count, (void*)&g.compact}) args[n++] = a;
    if (k == K_RENDER) args[n++] = &g.seams_only;
    return launch(p, k, stream, blocks(g.num, 256), 1, 256, 1, args);
}

// gr_render_stars': the full check of the sky (with the program: its device is the catalogues'), the sky and a view of each catalogue by value
int launch_stars(const char* who, gr_program* p, void* stream, const void* rdata, void* out, const gr_star_sky* sky, const gr_star_catalogue* near,
                 const gr_star_catalogue* far, int width, int height, const void* cfg, const void* dfg, const shading_geometry& g) {
    GR_CHECK(gr_internal_check_star_sky(who, sky, near, far, p));
    gr_star_sky by_value = *sky;
    gr_internal::catalogue_view near_view = gr_internal::view_of(near), far_view = gr_internal::view_of(far);
    return launch_shading(K_RENDER_STARS, p, stream, rdata, out, {&by_value, &near_view, &far_view}, width, height, 0, cfg, dfg, g);
}

// the analytic sky's rasteriser: steps 2 and 3 of the definition, in double
double sky_line_coverage(double x, double h, int n, double w) {
    const double t = x * n, a = h * n;
    auto covered_below = [&](double at) { const double s = at + w / 2, k = std::floor(s); return k * w + std::min(s - k, w); };
    return (covered_below(t + a) - covered_below(t - a)) / (2 * a);
}
double sky_upper_half_share(double x, double h, bool periodic) {
    auto below = [&](double at) { const double k = periodic ? std::floor(at) : 0.0; return k / 2 + std::max(at - k - 0.5, 0.0); };
    return (below(x + h) - below(x - h)) / (2 * h);
}

}   // namespace

// ---- the texture sky ------------------------------------------------------------------------------------------------------------------
int gr_render(gr_program* p, void* stream, const void* rdata, const void* rdata_count, int num_pixels, void* out,
              const void* bg1, const void* bg2, int bg_width, int bg_height, int bg_levels, int width, int height,
              int max_probes, const void* cfg, const void* dfg) {
    GR_NEED("gr_render", rdata, rdata_count, out, bg1, bg2);
    if (bg_width <= 0 || bg_height <= 0 || bg_levels <= 0) return refuse("gr_render", "the background's width, height and levels");
    return launch_shading(K_RENDER, p, stream, rdata, out, {&bg1, &bg2, &bg_width, &bg_height, &bg_levels}, width, height, max_probes, cfg, dfg,
                          whole_frame(num_pixels, rdata_count));
}

int gr_render_strips(gr_program* p, void* stream, const void* rdata, void* out, const void* bg1, const void* bg2, int bg_width,
                     int bg_height, int bg_levels, int width, int height, int block_rows, int strip_rank, int strip_count,
                     int compact_out, int max_probes, const void* cfg, const void* dfg) {
    GR_NEED("gr_render_strips", rdata, out, bg1, bg2);
    shading_geometry g{};
    GR_CHECK(strips_of_frame("gr_render_strips", p, width, height, block_rows, strip_rank, strip_count, compact_out, g));
    return launch_shading(K_RENDER, p, stream, rdata, out, {&bg1, &bg2, &bg_width, &bg_height, &bg_levels}, width, height, max_probes, cfg, dfg, g);
}

int gr_render_seams(gr_program* p, void* stream, const void* rdata, void* out, const void* bg1, const void* bg2, int bg_width,
                    int bg_height, int bg_levels, int width, int height, int block_rows, int strip_rank, int strip_count,
                    int compact_out, int max_probes, const void* cfg, const void* dfg) {
    GR_NEED("gr_render_seams", rdata, out, bg1, bg2);
    shading_geometry g{};
    GR_CHECK(seams_of_frame("gr_render_seams", p, width, height, block_rows, strip_rank, strip_count, compact_out, g));
    return launch_shading(K_RENDER, p, stream, rdata, out, {&bg1, &bg2, &bg_width, &bg_height, &bg_levels}, width, height, max_probes, cfg, dfg, g);
}

// ---- the analytic sky (geodesic_hip_internal.h, "Analytic sky") ------------------------------------------------------------------------
int gr_analytic_sky_default(gr_analytic_sky* out) {
    if (!out) return refuse("gr_analytic_sky_default", "null argument");
    static const float quadrants[2][4][3] = {{{0.16f, 0.30f, 0.62f}, {0.66f, 0.26f, 0.20f}, {0.20f, 0.52f, 0.32f}, {0.72f, 0.60f, 0.22f}},
                                             {{0.52f, 0.24f, 0.58f}, {0.22f, 0.56f, 0.60f}, {0.76f, 0.46f, 0.18f}, {0.40f, 0.62f, 0.24f}}};
    out->meridians = 36;
    out->parallels = 18;
    out->line_width = 0.08f;
    memcpy(out->quadrant, quadrants, sizeof(quadrants));
    for (int side = 0; side < 2; side++)
        for (int c = 0; c < 3; c++) out->line[side][c] = 0.02f;
    return GR_OK;
}

// what every entry point that takes a sky refuses of it, under its own name
extern "C" int gr_internal_check_analytic_sky(const char* who, const gr_analytic_sky* sky) {
    const std::string w = who;
    if (!sky) return refuse(w, "null sky");
    if (sky->meridians < 2 || sky->meridians > 360) return refuse(w, "meridians " + std::to_string(sky->meridians) + " (2 to 360)");
    if (sky->parallels < 1 || sky->parallels > 180) return refuse(w, "parallels " + std::to_string(sky->parallels) + " (1 to 180)");
    if (!(sky->line_width >= 0.f && sky->line_width <= 0.5f)) return refuse(w, "line_width " + std::to_string(sky->line_width) + " (0 to 0.5)");
    for (int side = 0; side < 2; side++) {
        for (int q = 0; q < 4; q++)
            for (int c = 0; c < 3; c++)
                if (!(sky->quadrant[side][q][c] >= 0.f && sky->quadrant[side][q][c] <= 1.f))
                    return refuse(w, "quadrant[" + std::to_string(side) + "][" + std::to_string(q) + "][" + std::to_string(c) + "] is not in [0, 1]");
        for (int c = 0; c < 3; c++)
            if (!(sky->line[side][c] >= 0.f && sky->line[side][c] <= 1.f))
                return refuse(w, "line[" + std::to_string(side) + "][" + std::to_string(c) + "] is not in [0, 1]");
    }
    return GR_OK;
}

int gr_render_analytic(gr_program* p, void* stream, const void* rdata, const void* rdata_count, int num_pixels, void* out, const gr_analytic_sky* sky,
                       int width, int height, const void* cfg, const void* dfg) {
    GR_NEED("gr_render_analytic", rdata, rdata_count, out);
    GR_CHECK(gr_internal_check_analytic_sky("gr_render_analytic", sky));
    gr_analytic_sky by_value = *sky;
    return launch_shading(K_RENDER_ANALYTIC, p, stream, rdata, out, {&by_value}, width, height, 0, cfg, dfg, whole_frame(num_pixels, rdata_count));
}

int gr_render_analytic_strips(gr_program* p, void* stream, const void* rdata, void* out, const gr_analytic_sky* sky, int width, int height,
                              int block_rows, int strip_rank, int strip_count, int compact_out, const void* cfg, const void* dfg) {
    GR_NEED("gr_render_analytic_strips", rdata, out);
    GR_CHECK(gr_internal_check_analytic_sky("gr_render_analytic_strips", sky));
    shading_geometry g{};
    GR_CHECK(strips_of_frame("gr_render_analytic_strips", p, width, height, block_rows, strip_rank, strip_count, compact_out, g));
    gr_analytic_sky by_value = *sky;
    return launch_shading(K_RENDER_ANALYTIC, p, stream, rdata, out, {&by_value}, width, height, 0, cfg, dfg, g);
}

int gr_analytic_sky_image(const gr_analytic_sky* sky, int side, int width, int height, unsigned char* out_rgba8) {
    GR_CHECK(gr_internal_check_analytic_sky("gr_analytic_sky_image", sky));
    if (!out_rgba8) return refuse("gr_analytic_sky_image", "null out_rgba8");
    if (side != 0 && side != 1) return refuse("gr_analytic_sky_image", "side " + std::to_string(side) + " (0 or 1)");
    if (width < 1 || height < 1) return refuse("gr_analytic_sky_image", "width and height");
    const double floor_h = std::ldexp(1.0, -14);
    const double hu = std::max(0.5 / width, floor_h), hv = std::max(0.5 / height, floor_h);
    std::vector<double> cu(width), fu(width);
    for (int x = 0; x < width; x++) {
        const double u = (x + 0.5) / width;
        cu[x] = sky_line_coverage(u, hu, sky->meridians, sky->line_width);
        fu[x] = sky_upper_half_share(u, hu, true);
    }
    for (int y = 0; y < height; y++) {
        const double v = (y + 0.5) / height;
        const double cv = sky_line_coverage(v, hv, sky->parallels, sky->line_width), fv = sky_upper_half_share(v, hv, false);
        for (int x = 0; x < width; x++) {
            const double g = 1 - (1 - cu[x]) * (1 - cv);
            const double weight[4] = {(1 - fu[x]) * (1 - fv), fu[x] * (1 - fv), (1 - fu[x]) * fv, fu[x] * fv};
            unsigned char* px = out_rgba8 + ((size_t)y * width + x) * 4;
            for (int c = 0; c < 3; c++) {
                double base = 0;
                for (int q = 0; q < 4; q++) base += weight[q] * sky->quadrant[side][q][c];
                const double value = base + (sky->line[side][c] - base) * g;
                px[c] = (unsigned char)std::lround(std::min(std::max(value, 0.0), 1.0) * 255.0);
            }
            px[3] = 255;
        }
    }
    return GR_OK;
}

// ---- the star sky (geodesic_hip_internal.h, "Star sky") ---------------------------------------------------------------------------------
int gr_render_stars(gr_program* p, void* stream, const void* rdata, const void* rdata_count, int num_pixels, void* out, const gr_star_sky* sky,
                    const gr_star_catalogue* near, const gr_star_catalogue* far, int width, int height, const void* cfg, const void* dfg) {
    GR_NEED("gr_render_stars", rdata, rdata_count, out);
    return launch_stars("gr_render_stars", p, stream, rdata, out, sky, near, far, width, height, cfg, dfg, whole_frame(num_pixels, rdata_count));
}

int gr_render_stars_strips(gr_program* p, void* stream, const void* rdata, void* out, const gr_star_sky* sky, const gr_star_catalogue* near,
                           const gr_star_catalogue* far, int width, int height, int block_rows, int strip_rank, int strip_count, int compact_out,
                           const void* cfg, const void* dfg) {
    // (the refusals first, in gr_render_analytic_strips' order: the program is not looked into before them)
    GR_NEED("gr_render_stars_strips", rdata, out);
    GR_CHECK(gr_internal_check_star_sky("gr_render_stars_strips", sky, nullptr, nullptr, nullptr));
    shading_geometry g{};
    GR_CHECK(strips_of_frame("gr_render_stars_strips", p, width, height, block_rows, strip_rank, strip_count, compact_out, g));
    if (!p) return refuse("gr_render_stars_strips", "null program");
    return launch_stars("gr_render_stars_strips", p, stream, rdata, out, sky, near, far, width, height, cfg, dfg, g);
}
