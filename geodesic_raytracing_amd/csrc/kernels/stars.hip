// ------------------------------------------------------------------------------------------------
// stars.hip - a star catalogue built on the device (geodesic_hip_internal.h, "Star sky"; the host object: csrc/star_catalogue.cpp; the
// kernel that gathers from it: gr_render_stars in shading.hip).  Part of the set-up module (capi.cpp: compile_setup_module): IEEE
// arithmetic, no contraction, no re-association - every sum below is taken in the order it is written.  Vector stores and ordinary
// atomics only.
//
// The host uploads uv[2 n] and flux[3 n]; the launches, in order (star_catalogue.cpp):
//   gr_stars_count    a lane a star: its cell, one atomic add into counts[cell]
//   gr_stars_scan     the exclusive scan of counts into cell_start[cells + 1], in three phases of one kernel (up to 2^24 cells): a
//                     workgroup sums its 2048 counts; one workgroup scans the up to 8192 sums; a workgroup scans its 2048 counts from its sum
//   gr_stars_scatter  a lane a star: order[cell_start[cell] + (an atomic add into cursor[cell])] = s.  Which star of a cell gets which slot
//                     is the hardware's business, so
//   gr_stars_order    a workgroup a cell sorts the cell's slots in place, ascending: the result is a function of the inputs alone.  A
//                     bitonic network with every exchange ascending (the first step of a merge flips its partner, i ^ (k - 1)), which
//                     sorts any length: a partner behind the end is skipped, as if +infinity stood there.  The slots are in global
//                     memory - a cell may hold every star - and a workgroup's barrier orders its own stores and loads.
//   gr_stars_gather   a lane a slot: the star's record (u, v, r, g | b, 0, 0, 0), two float4, in cell order - what gr_render_stars reads
//   gr_stars_sums     a lane a cell: the cell's flux summed in double in ascending catalogue index, into table[c][j + 1][i + 1]; the
//                     table's first row and column are zeroed by the host's memset
//   gr_stars_prefix   along = 0: a lane a (channel, row), running sums along u; along = 1: a lane a (channel, column), along v

#define GR_STARS_LANES 256
#define GR_STARS_CHUNK 2048   // counts a workgroup of gr_stars_scan: 8 a lane

__device__ __forceinline__ int star_cell(float u, float v, int cells_u, int cells_v) {
    const int i = min((int)__builtin_floorf(u * (float)cells_u), cells_u - 1), j = min((int)__builtin_floorf(v * (float)cells_v), cells_v - 1);
    return j * cells_u + i;
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_count(const float2* __restrict__ uv, int n, int cells_u, int cells_v,
                                                                            unsigned int* __restrict__ counts) {
    const int s = blockIdx.x * GR_STARS_LANES + threadIdx.x;
    if (s >= n) return;
    const float2 at = uv[s];
    atomicAdd(&counts[star_cell(at.x, at.y, cells_u, cells_v)], 1u);
}

// the workgroup's exclusive scan of one value a lane -> the lane's offset; *total: the sum of all (the same in every lane)
__device__ __forceinline__ unsigned int stars_scan_lanes(unsigned int mine, unsigned int* shared, unsigned int* total) {
    const int t = threadIdx.x;
    shared[t] = mine;
    __syncthreads();
    for (int step = 1; step < GR_STARS_LANES; step <<= 1) {
        const unsigned int before = t >= step ? shared[t - step] : 0u;
        __syncthreads();
        shared[t] += before;
        __syncthreads();
    }
    const unsigned int inclusive = shared[t];
    *total = shared[GR_STARS_LANES - 1];
    __syncthreads();
    return inclusive - mine;
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_scan(const unsigned int* __restrict__ counts, int cells, unsigned int* __restrict__ sums,
                                                                           int sum_count, int* __restrict__ cell_start, int phase) {
    __shared__ unsigned int shared[GR_STARS_LANES];
    const int t = threadIdx.x;
    unsigned int total;
    if (phase == 1) {
        // one workgroup: sums[] becomes its own exclusive scan, a lane takes `each` consecutive sums
        const int each = (sum_count + GR_STARS_LANES - 1) / GR_STARS_LANES, first = t * each;
        unsigned int mine = 0;
        for (int k = first; k < first + each && k < sum_count; k++) mine += sums[k];
        unsigned int running = stars_scan_lanes(mine, shared, &total);
        for (int k = first; k < first + each && k < sum_count; k++) {
            const unsigned int value = sums[k];
            sums[k] = running;
            running += value;
        }
        if (t == 0) cell_start[cells] = (int)total;
        return;
    }
    const int first = blockIdx.x * GR_STARS_CHUNK + t * (GR_STARS_CHUNK / GR_STARS_LANES);
    unsigned int value[GR_STARS_CHUNK / GR_STARS_LANES], mine = 0;
#pragma unroll
    for (int k = 0; k < GR_STARS_CHUNK / GR_STARS_LANES; k++) {
        value[k] = first + k < cells ? counts[first + k] : 0u;
        mine += value[k];
    }
    unsigned int running = stars_scan_lanes(mine, shared, &total);
    if (phase == 0) {
        if (t == 0) sums[blockIdx.x] = total;
        return;
    }
    running += sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < GR_STARS_CHUNK / GR_STARS_LANES; k++) {
        if (first + k < cells) cell_start[first + k] = (int)running;
        running += value[k];
    }
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_scatter(const float2* __restrict__ uv, int n, int cells_u, int cells_v,
                                                                              const int* __restrict__ cell_start, unsigned int* __restrict__ cursor,
                                                                              int* __restrict__ order) {
    const int s = blockIdx.x * GR_STARS_LANES + threadIdx.x;
    if (s >= n) return;
    const float2 at = uv[s];
    const int cell = star_cell(at.x, at.y, cells_u, cells_v);
    const int slot = cell_start[cell] + (int)atomicAdd(&cursor[cell], 1u);
    if (slot < n) order[slot] = s;   // (always: the cursors count what the histogram counted)
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_order(const int* __restrict__ cell_start, int cells, int n, int* order) {
    for (int cell = blockIdx.x; cell < cells; cell += gridDim.x) {   // (the trip counts are the workgroup's: every lane meets every barrier)
        const int begin = cell_start[cell], m = min(cell_start[cell + 1], n) - begin;
        if (m < 2) continue;
        int* slots = order + begin;
        for (int k = 2; (k >> 1) < m; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int flip = j == (k >> 1) ? k - 1 : j;
                for (int i = threadIdx.x; i < m; i += GR_STARS_LANES) {
                    const int partner = i ^ flip;
                    if (partner > i && partner < m) {
                        const int a = slots[i], b = slots[partner];
                        if (a > b) {
                            slots[i] = b;
                            slots[partner] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_gather(const float2* __restrict__ uv, const float* __restrict__ flux, int n,
                                                                             const int* __restrict__ order, float4* __restrict__ stars) {
    const int slot = blockIdx.x * GR_STARS_LANES + threadIdx.x;
    if (slot >= n) return;
    const int s = order[slot];
    if (s < 0 || s >= n) return;
    const float2 at = uv[s];
    stars[2 * (size_t)slot] = make_float4(at.x, at.y, flux[3 * (size_t)s], flux[3 * (size_t)s + 1]);
    stars[2 * (size_t)slot + 1] = make_float4(flux[3 * (size_t)s + 2], 0.f, 0.f, 0.f);
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_sums(const int* __restrict__ cell_start, const float4* __restrict__ stars, int n,
                                                                           int cells_u, int cells_v, double* __restrict__ table) {
    const int cell = blockIdx.x * GR_STARS_LANES + threadIdx.x;
    if (cell >= cells_u * cells_v) return;
    const int j = cell / cells_u, i = cell - j * cells_u;
    double r = 0, g = 0, b = 0;
    for (int slot = cell_start[cell], end = min(cell_start[cell + 1], n); slot < end; slot++) {
        const float4 first = stars[2 * (size_t)slot], second = stars[2 * (size_t)slot + 1];
        r += (double)first.z;
        g += (double)first.w;
        b += (double)second.x;
    }
    const size_t plane = (size_t)(cells_v + 1) * (size_t)(cells_u + 1), at = (size_t)(j + 1) * (size_t)(cells_u + 1) + (size_t)(i + 1);
    table[at] = r;
    table[plane + at] = g;
    table[2 * plane + at] = b;
}

extern "C" __global__ void __launch_bounds__(GR_STARS_LANES) gr_stars_prefix(double* table, int cells_u, int cells_v, int along) {
    const int line = blockIdx.x * GR_STARS_LANES + threadIdx.x;
    const int lines = along == 0 ? cells_v : cells_u;
    if (line >= 3 * lines) return;
    const int channel = line / lines, within = line - channel * lines;
    const size_t row = (size_t)(cells_u + 1);
    double* plane = table + (size_t)channel * (size_t)(cells_v + 1) * row;
    double running = 0;
    if (along == 0) {
        double* at = plane + (size_t)(within + 1) * row;
        for (int i = 1; i <= cells_u; i++) {
            running += at[i];
            at[i] = running;
        }
    } else {
        double* at = plane + (size_t)(within + 1);
        for (int j = 1; j <= cells_v; j++) {
            running += at[(size_t)j * row];
            at[(size_t)j * row] = running;
        }
    }
}
