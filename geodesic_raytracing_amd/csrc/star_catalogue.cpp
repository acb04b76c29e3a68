// star_catalogue.cpp — the star sky's host half (geodesic_hip_internal.h, "Star sky"): gr_star_catalogue, built on the device by the
// kernels of kernels/stars.hip through a borrowed program, as the file encoders of device_encoders.cpp are; the random field; and the view of
// a catalogue that the launchers of gr_render_stars (shading.cpp) hand the kernel by value.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "internal.hpp"

using gr_internal::blocks, gr_internal::launch;

namespace {

int fail(const std::string& msg) { return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, msg.c_str()); }

const int LANES = 256, CHUNK = 2048;   // GR_STARS_LANES, GR_STARS_CHUNK of kernels/stars.hip
const int MOST_STARS = 1 << 24;

bool cell_count_allowed(int cells) { return cells >= 16 && cells <= 4096 && (cells & (cells - 1)) == 0; }

}   // namespace

struct gr_star_catalogue {
    int device = 0, n = 0, cells_u = 0, cells_v = 0;
    int* cell_start = nullptr;   // [cells + 1]
    int* order = nullptr;        // [n]: catalogue indices, cell by cell, ascending within a cell
    void* stars = nullptr;       // [n] records of two float4, (u, v, r, g | b, 0, 0, 0), in that order
    double* table = nullptr;     // [3][cells_v + 1][cells_u + 1]
    std::vector<void*> on_device;

    ~gr_star_catalogue() {
        if (!on_device.empty()) (void)hipSetDevice(device);
        for (void* memory : on_device) (void)hipFree(memory);
    }
    template <class T> int allocate(T** out, size_t bytes) {
        HIP_CHECK(hipMalloc((void**)out, bytes));
        on_device.push_back(*out);
        return GR_OK;
    }
    size_t cells() const { return (size_t)cells_u * (size_t)cells_v; }
    size_t table_entries() const { return 3 * (size_t)(cells_v + 1) * (size_t)(cells_u + 1); }
};

int gr_star_sky_default(gr_star_sky* out) {
    if (!out) return fail("gr_star_sky_default: null argument");
    out->min_footprint = std::ldexp(1.f, -16);
    memset(out->background, 0, sizeof(out->background));
    return GR_OK;
}

extern "C" int gr_internal_check_star_sky(const char* who, const gr_star_sky* sky, const gr_star_catalogue* near, const gr_star_catalogue* far,
                                          const gr_program* p) {
    const std::string w = who;
    if (!sky) return fail(w + ": null sky");
    int exponent = 0;
    const bool power_of_two = std::isfinite(sky->min_footprint) && sky->min_footprint > 0 && std::frexp(sky->min_footprint, &exponent) == 0.5f;
    if (!power_of_two || exponent - 1 < -20 || exponent - 1 > -8)
        return fail(w + ": min_footprint " + std::to_string(sky->min_footprint) + " (a power of two, 2^-20 to 2^-8)");
    for (int side = 0; side < 2; side++)
        for (int c = 0; c < 3; c++)
            if (!(sky->background[side][c] >= 0.f && sky->background[side][c] <= 1.f))
                return fail(w + ": background[" + std::to_string(side) + "][" + std::to_string(c) + "] is not in [0, 1]");
    if (p && near && near->device != gr_internal::device_of(p)) return fail(w + ": the near catalogue lives on another device than the program");
    if (p && far && far->device != gr_internal::device_of(p)) return fail(w + ": the far catalogue lives on another device than the program");
    return GR_OK;
}

int gr_star_catalogue_create(gr_program* p, int n, const float* uv, const float* flux, int cells_u, int cells_v, gr_star_catalogue** out) {
    const std::string who = "gr_star_catalogue_create: ";
    if (!p) return fail(who + "null program");
    if (!uv) return fail(who + "null uv");
    if (!flux) return fail(who + "null flux");
    if (!out) return fail(who + "null out");
    if (n < 1 || n > MOST_STARS) return fail(who + "n " + std::to_string(n) + " (1 to 2^24)");
    if (cells_u == 0) cells_u = 1024;
    if (cells_v == 0) cells_v = 512;
    if (!cell_count_allowed(cells_u)) return fail(who + "cells_u " + std::to_string(cells_u) + " (a power of two, 16 to 4096)");
    if (!cell_count_allowed(cells_v)) return fail(who + "cells_v " + std::to_string(cells_v) + " (a power of two, 16 to 4096)");
    for (int s = 0; s < n; s++) {
        if (!(uv[2 * (size_t)s] >= 0.f && uv[2 * (size_t)s] < 1.f)) return fail(who + "uv: u of star " + std::to_string(s) + " is not in [0, 1)");
        if (!(uv[2 * (size_t)s + 1] >= 0.f && uv[2 * (size_t)s + 1] <= 1.f)) return fail(who + "uv: v of star " + std::to_string(s) + " is not in [0, 1]");
        for (int c = 0; c < 3; c++)
            if (!(flux[3 * (size_t)s + c] >= 0.f && std::isfinite(flux[3 * (size_t)s + c])))
                return fail(who + "flux: star " + std::to_string(s) + " has a flux that is negative or not finite");
    }
    auto c = std::make_unique<gr_star_catalogue>();
    c->device = gr_internal::device_of(p), c->n = n, c->cells_u = cells_u, c->cells_v = cells_v;
    HIP_CHECK(hipSetDevice(c->device));
    int cells = (int)c->cells(), sum_count = (cells + CHUNK - 1) / CHUNK;
    GR_CHECK(c->allocate(&c->cell_start, (c->cells() + 1) * sizeof(int)));
    GR_CHECK(c->allocate(&c->order, (size_t)n * sizeof(int)));
    GR_CHECK(c->allocate(&c->stars, (size_t)n * 32));
    GR_CHECK(c->allocate(&c->table, c->table_entries() * sizeof(double)));
    // what only the build needs: the upload, the histogram (then the scatter's cursors) and the scan's sums
    gr_star_catalogue scratch;
    scratch.device = c->device;
    float *device_uv = nullptr, *device_flux = nullptr;
    unsigned int *counts = nullptr, *sums = nullptr;
    GR_CHECK(scratch.allocate(&device_uv, (size_t)n * 8));
    GR_CHECK(scratch.allocate(&device_flux, (size_t)n * 12));
    GR_CHECK(scratch.allocate(&counts, c->cells() * 4));
    GR_CHECK(scratch.allocate(&sums, (size_t)sum_count * 4));
    hipStream_t on = nullptr;
    void* stream = nullptr;
    HIP_CHECK(hipMemcpyAsync(device_uv, uv, (size_t)n * 8, hipMemcpyHostToDevice, on));
    HIP_CHECK(hipMemcpyAsync(device_flux, flux, (size_t)n * 12, hipMemcpyHostToDevice, on));
    HIP_CHECK(hipMemsetAsync(counts, 0, c->cells() * 4, on));
    HIP_CHECK(hipMemsetAsync(c->table, 0, c->table_entries() * sizeof(double), on));
    int* cell_start = c->cell_start;
    int* order = c->order;
    void* stars = c->stars;
    double* table = c->table;
    void* count_args[] = {&device_uv, &n, &cells_u, &cells_v, &counts};
    GR_CHECK(launch(p, K_STARS_COUNT, stream, blocks(n, LANES), 1, LANES, 1, count_args));
    for (int phase = 0; phase < 3; phase++) {
        void* scan_args[] = {&counts, &cells, &sums, &sum_count, &cell_start, &phase};
        GR_CHECK(launch(p, K_STARS_SCAN, stream, phase == 1 ? 1u : (unsigned)sum_count, 1, LANES, 1, scan_args));
    }
    HIP_CHECK(hipMemsetAsync(counts, 0, c->cells() * 4, on));
    void* scatter_args[] = {&device_uv, &n, &cells_u, &cells_v, &cell_start, &counts, &order};
    GR_CHECK(launch(p, K_STARS_SCATTER, stream, blocks(n, LANES), 1, LANES, 1, scatter_args));
    void* order_args[] = {&cell_start, &cells, &n, &order};
    GR_CHECK(launch(p, K_STARS_ORDER, stream, (unsigned)std::min(cells, 1 << 16), 1, LANES, 1, order_args));
    void* gather_args[] = {&device_uv, &device_flux, &n, &order, &stars};
    GR_CHECK(launch(p, K_STARS_GATHER, stream, blocks(n, LANES), 1, LANES, 1, gather_args));
    void* sums_args[] = {&cell_start, &stars, &n, &cells_u, &cells_v, &table};
    GR_CHECK(launch(p, K_STARS_SUMS, stream, blocks(cells, LANES), 1, LANES, 1, sums_args));
    for (int along = 0; along < 2; along++) {
        void* prefix_args[] = {&table, &cells_u, &cells_v, &along};
        GR_CHECK(launch(p, K_STARS_PREFIX, stream, blocks(3 * (along == 0 ? cells_v : cells_u), LANES), 1, LANES, 1, prefix_args));
    }
    HIP_CHECK(hipStreamSynchronize(on));
    *out = c.release();
    return GR_OK;
}

void gr_star_catalogue_destroy(gr_star_catalogue* c) { delete c; }

gr_internal::catalogue_view gr_internal::view_of(const gr_star_catalogue* c) {
    return c ? catalogue_view{c->cell_start, c->stars, c->table, c->n, c->cells_u, c->cells_v} : catalogue_view{};
}

int gr_star_catalogue_info(const gr_star_catalogue* c, int* n, int* cells_u, int* cells_v) {
    if (!c) return fail("gr_star_catalogue_info: null catalogue");
    if (n) *n = c->n;
    if (cells_u) *cells_u = c->cells_u;
    if (cells_v) *cells_v = c->cells_v;
    return GR_OK;
}

int gr_star_catalogue_download(const gr_star_catalogue* c, int* cell_start, int* order, double* table) {
    if (!c) return fail("gr_star_catalogue_download: null catalogue");
    HIP_CHECK(hipSetDevice(c->device));
    if (cell_start) HIP_CHECK(hipMemcpy(cell_start, c->cell_start, (c->cells() + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (order) HIP_CHECK(hipMemcpy(order, c->order, (size_t)c->n * sizeof(int), hipMemcpyDeviceToHost));
    if (table) HIP_CHECK(hipMemcpy(table, c->table, c->table_entries() * sizeof(double), hipMemcpyDeviceToHost));
    return GR_OK;
}

int gr_star_field_random(unsigned long long seed, int n, float* out_uv, float* out_flux) {
    if (!out_uv) return fail("gr_star_field_random: null out_uv");
    if (!out_flux) return fail("gr_star_field_random: null out_flux");
    if (n < 1 || n > MOST_STARS) return fail("gr_star_field_random: n " + std::to_string(n) + " (1 to 2^24)");
    static const double colour[7][3] = {{0.61, 0.71, 1.0}, {0.68, 0.77, 1.0}, {0.80, 0.85, 1.0}, {0.97, 0.96, 1.0},
                                        {1.0, 0.92, 0.82}, {1.0, 0.78, 0.56}, {1.0, 0.58, 0.33}};
    const double pi = 3.14159265358979323846, faintest = 2e-9;
    uint64_t state = seed;
    auto next = [&state] {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * 0x1p-53;
    };
    for (int s = 0; s < n; s++) {
        const double x1 = next(), x2 = next(), x3 = next(), x4 = next();
        const float u = (float)x1;
        const double v = std::acos(1 - 2 * x2) / pi;
        out_uv[2 * (size_t)s] = u >= 1.f ? 0.f : u;
        out_uv[2 * (size_t)s + 1] = (float)v;
        const double brightness = faintest * std::min(std::pow(1 - x3, -2.0 / 3.0), 1e4);
        const int k = std::min((int)std::floor(7 * x4), 6);
        const double area = 2 * pi * pi * std::max(std::sin(pi * v), 1e-3);
        for (int c = 0; c < 3; c++) out_flux[3 * (size_t)s + c] = (float)(brightness * colour[k][c] / area);
    }
    return GR_OK;
}
