// trace_launch.cpp — the launchers of the trace stage: the prepass, the tile order, gr_trace_fused and its kin, the two launches of
// adaptive sampling with their refine step, the scheduled reference trace and the compacting one.  What a launch decides is in
// trace_plan.cpp (no HIP, host-tested); here are the argument arrays in the kernels' order, the resets and the launches.
#include <hip/hip_runtime_api.h>

#include "internal.hpp"
#include "trace_plan.hpp"

using gr_internal::blocks, gr_internal::launch, gr_internal::facts_of, gr_internal::draw_ticket, gr_internal::resident_groups_per_cu;
using namespace trace_plan;

namespace {

int fail(const char* msg) { return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, msg); }

// tiles (one wave each) a device traces; 0 when the description is invalid (trace_launch says why)
long long device_tile_count(int width, int height, int block_rows, int strip_rank, int strip_count) {
    const strip_share share = strips(height, block_rows, strip_rank, strip_count, HEIGHT_ROUNDED_UP_TO_8);
    return share.bad || share.block_rows % 8 != 0 ? 0 : device_tiles(width, height, share);
}

int order_tiles_launch(gr_program* p, void* stream, const void* term, const void* cell_attempts, int prepass_width, int prepass_height, int width,
                       int height, int block_rows, int strip_rank, int strip_count, void* tile_order, const void* tile_history, int shift_x, int shift_y) {
    const strip_share share = strips(height, block_rows, strip_rank, strip_count, HEIGHT_ROUNDED_UP_TO_8);
    const long long tiles = share.bad || share.block_rows % 8 != 0 ? 0 : device_tiles(width, height, share);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail("gr_order_tiles: bad image or strip description");
    block_rows = share.block_rows; strip_rank = share.strip_rank; strip_count = share.strip_count;
    int total = (int)tiles;
    HIP_CHECK(hipSetDevice(gr_internal::device_of(p)));
    HIP_CHECK(hipMemsetAsync(tile_order, 0, 128, (hipStream_t)stream));
    int history_reach = switches::tile_history_reach();
    for (int phase = 0; phase < 2; phase++) {
        void* args[] = {&term, &cell_attempts, &prepass_width, &prepass_height, &width, &height, &block_rows, &strip_rank, &strip_count,
                        &total, &tile_order, &phase, &tile_history, &history_reach, &shift_x, &shift_y};
        GR_CHECK(launch(p, K_ORDER_TILES, stream, blocks(total, 1024), 1, 1024, 1, args));
    }
    return GR_OK;
}

// gr_trace_fused (rays_per_lane 1) and gr_trace_pair (2): same tiles, same arguments; a pair wave takes two tile-waves.  Plan, refuse,
// reset, launch: a refused call and an empty share make no HIP call at all.
int trace_launch(gr_program* p, void* stream, int rays_per_lane, const gr_trace_fused_args& a) {
    if (!p) return fail("null program");
    trace_input in;
    in.args = a;
    in.rays_per_lane = rays_per_lane;
    in.program = facts_of(p);
    in.resident_per_cu = [p](int kernel, int wg, int* per_cu) { return resident_groups_per_cu(p, kernel, wg, per_cu); };
    trace_plan::trace_plan plan = plan_trace(in);
    if (plan.refused.code != GR_OK) return plan.refused.message ? gr_internal_fail(plan.refused.code, plan.refused.message) : plan.refused.code;
    if (plan.nothing) return GR_OK;
    unsigned int* tickets = nullptr;
    if (plan.ticket) GR_CHECK(draw_ticket(p, stream, &tickets));
    if (plan.termination_bytes || plan.tile_cost_bytes || plan.lot_words_bytes) HIP_CHECK(hipSetDevice(gr_internal::device_of(p)));
    if (plan.termination_bytes) HIP_CHECK(hipMemsetAsync(const_cast<void*>(a.termination_buffer), 0xff, plan.termination_bytes, (hipStream_t)stream));
    if (plan.tile_cost_bytes) HIP_CHECK(hipMemsetAsync(a.tile_cost, 0, plan.tile_cost_bytes, (hipStream_t)stream));
    if (plan.lot_words_bytes) HIP_CHECK(hipMemsetAsync(plan.lot.words, 0, plan.lot_words_bytes, (hipStream_t)stream));
    gr_trace_fused_args k = a;   // (addressable copies of what the kernel takes as the caller gave it)
    // the last eleven: gr_trace_fused only (gr_trace_pair's parameter list ends before them), the lot gr_trace_fused_parking and
    // (unused) gr_trace_fused_lattice, the very last gr_trace_fused_lattice only
    void* args[] = {&k.camera_generic, &k.camera_quat, &k.render_data, &k.width, &k.height, &plan.block_rows, &plan.strip_rank, &plan.strip_count,
                    &k.termination_buffer, &k.prepass_width, &k.prepass_height, &k.e0, &k.e1, &k.e2, &k.e3, &k.cfg, &k.dfg, &k.attempt_counter, &tickets,
                    &plan.total_waves, &k.lattice, &k.pending_only, &k.tile_order, &plan.shading, &plan.prepass_tickets, &plan.ticket_tiles, &k.tile_cost,
                    &plan.last_class_is_skipped, &k.lattice_rays, &plan.lot, &k.guessed};
    return launch(p, plan.kernel, stream, plan.grid, 1, plan.wg, 1, args);
}

// the arguments gr_trace_fused and gr_trace_pair share, and gr_trace_fused_adaptive's first seventeen
gr_trace_fused_args plain_args(const void* camera_generic, const void* camera_quat, void* rdata, int width, int height, int block_rows, int strip_rank,
                               int strip_count, const void* term, int prepass_width, int prepass_height, const void* e0, const void* e1, const void* e2,
                               const void* e3, const void* cfg, const void* dfg, void* attempt_counter) {
    gr_trace_fused_args a = {};
    a.camera_generic = camera_generic; a.camera_quat = camera_quat; a.render_data = rdata;
    a.width = width; a.height = height; a.block_rows = block_rows; a.strip_rank = strip_rank; a.strip_count = strip_count;
    a.termination_buffer = term; a.prepass_width = prepass_width; a.prepass_height = prepass_height;
    a.e0 = e0; a.e1 = e1; a.e2 = e2; a.e3 = e3; a.cfg = cfg; a.dfg = dfg; a.attempt_counter = attempt_counter;
    a.lattice = 1;
    return a;
}

// one launch of gr_adaptive_refine's kernel: phase 0 decides (and, with a list, marks and counts by cost class), phase 1 deals every marked pixel its place
int refine_launch(gr_program* p, void* stream, void* rdata, void* pending_count, int width, int height, const void* dfg, const strip_share& share,
                  const void* lattice_rays, const void* cfg, void* pending_list, int phase, const void* block_cost_before) {
    int block_rows = share.block_rows, strip_rank = share.strip_rank, strip_count = share.strip_count;
    void* args[] = {&rdata, &pending_count, &width, &height, &dfg, &block_rows, &strip_rank, &strip_count, &lattice_rays, &cfg, &pending_list, &phase,
                    &block_cost_before};
    return launch(p, K_ADAPTIVE_REFINE, stream, (unsigned)((width / 2 + 15) / 16), (unsigned)((height / 2 + 15) / 16), 16, 16, args);
}

}   // namespace

extern "C" {

int gr_prepass_fused_strips(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* term,
                            int prepass_width, int prepass_height, const void* e0, const void* e1, const void* e2, const void* e3,
                            const void* cfg, const void* dfg, int image_height, int block_rows, int strip_rank, int strip_count,
                            void* cell_attempts, int row_margin) {
    const strip_share share = strips(image_height, block_rows, strip_rank, strip_count, EIGHT_ROWS);
    if (share.bad || image_height <= 0) return fail("bad strip description");
    block_rows = share.block_rows; strip_rank = share.strip_rank; strip_count = share.strip_count;
    void* args[] = {&camera_generic, &camera_quat, &term, &prepass_width, &prepass_height, &e0, &e1, &e2, &e3, &cfg, &dfg,
                    &image_height, &block_rows, &strip_rank, &strip_count, &cell_attempts, &row_margin};
    if (row_margin < 0) return fail("negative row margin");
    return launch(p, K_PREPASS_FUSED, stream, blocks((long long)prepass_width * prepass_height, 64), 1, 64, 1, args);   // (a NULL program is launch()'s to refuse)
}

int gr_camera_prepass(gr_program* p, void* stream, const void* position_cart, float flip, const float basis_speed[3], void* position_generic_out,
                      void* e0_out, void* e1_out, void* e2_out, void* e3_out, const void* camera_quat, void* term, int prepass_width,
                      int prepass_height, const void* cfg, const void* dfg, int image_height, int block_rows, int strip_rank, int strip_count,
                      void* cell_attempts, int row_margin) {
    if (!basis_speed) return fail("null basis speed");
    if (prepass_width < 0 || prepass_height < 0) return fail("negative prepass size");
    const strip_share share = strips(image_height, block_rows, strip_rank, strip_count, EIGHT_ROWS);
    if (share.bad) return fail("bad strip description");
    block_rows = share.block_rows; strip_rank = share.strip_rank; strip_count = share.strip_count;
    if (image_height <= 0) image_height = prepass_height > 0 ? prepass_height * 16 : 16;
    float sx = basis_speed[0], sy = basis_speed[1], sz = basis_speed[2];
    if (row_margin < 0) return fail("negative row margin");
    // the camera's coordinates and tetrad: one lane of the set-up module (IEEE arithmetic, kernels/camera.hip) ...
    void* setup_args[] = {&position_cart, &flip, &sx, &sy, &sz, &position_generic_out, &e0_out, &e1_out, &e2_out, &e3_out, &cfg};
    GR_CHECK(launch(p, K_CAMERA_SETUP, stream, 1, 1, 64, 1, setup_args));
    // ... then the prepass grid reads them back (same stream)
    const long long cells = (long long)prepass_width * prepass_height;
    if (cells <= 0) return GR_OK;
    const void* camera_generic = position_generic_out;
    const void *e0 = e0_out, *e1 = e1_out, *e2 = e2_out, *e3 = e3_out;
    void* args[] = {&camera_generic, &camera_quat, &term, &prepass_width, &prepass_height, &e0, &e1, &e2, &e3, &cfg, &dfg,
                    &image_height, &block_rows, &strip_rank, &strip_count, &cell_attempts, &row_margin};
    return launch(p, K_PREPASS_FUSED, stream, blocks(cells, 64), 1, 64, 1, args);
}

int gr_prepass_fused(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* term,
                     int prepass_width, int prepass_height, const void* e0, const void* e1, const void* e2, const void* e3,
                     const void* cfg, const void* dfg) {
    return gr_prepass_fused_strips(p, stream, camera_generic, camera_quat, term, prepass_width, prepass_height, e0, e1, e2, e3, cfg, dfg,
                                   prepass_height * 16, 8, 0, 1, nullptr, 0);
}

long long gr_tile_order_bytes(int width, int height, int block_rows, int strip_rank, int strip_count) {
    return (32 + 2 * device_tile_count(width, height, block_rows, strip_rank, strip_count)) * 4;   // header (2 x 16 classes), list, classes
}

int gr_order_tiles(gr_program* p, void* stream, const void* term, const void* cell_attempts, int prepass_width, int prepass_height,
                   int width, int height, int block_rows, int strip_rank, int strip_count, void* tile_order) {
    if (!p || !term || !cell_attempts || !tile_order || prepass_width <= 0 || prepass_height <= 0)
        return fail("gr_order_tiles: null argument or no prepass");
    return order_tiles_launch(p, stream, term, cell_attempts, prepass_width, prepass_height, width, height, block_rows, strip_rank, strip_count,
                              tile_order, nullptr, 0, 0);
}

int gr_order_tiles_by_history(gr_program* p, void* stream, const void* tile_history, int width, int height, int block_rows, int strip_rank,
                              int strip_count, void* tile_order, int shift_x, int shift_y) {
    if (!p || !tile_history || !tile_order) return fail("gr_order_tiles_by_history: null argument");
    return order_tiles_launch(p, stream, nullptr, nullptr, 0, 0, width, height, block_rows, strip_rank, strip_count, tile_order, tile_history,
                              shift_x, shift_y);
}

size_t gr_parking_lot_bytes(int slots, int groups, size_t* words_bytes) {
    if (words_bytes) *words_bytes = (16 + (size_t)(groups > 0 ? groups : 0)) * sizeof(unsigned int);
    return (size_t)(slots > 0 ? slots : 0) * 6 * 16;
}

long long gr_trace_fused_wave_slots(gr_program* p) {
    int per_cu = 0;
    if (!p || resident_groups_per_cu(p, K_TRACE_FUSED, 256, &per_cu) != GR_OK) return 0;
    return (long long)facts_of(p).compute_units * per_cu * 4;
}

int gr_trace_fused(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rdata, int width,
                   int height, int block_rows, int strip_rank, int strip_count, const void* term, int prepass_width,
                   int prepass_height, const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg,
                   const void* dfg, void* attempt_counter) {
    return trace_launch(p, stream, 1, plain_args(camera_generic, camera_quat, rdata, width, height, block_rows, strip_rank, strip_count, term, prepass_width,
                                                 prepass_height, e0, e1, e2, e3, cfg, dfg, attempt_counter));
}

int gr_trace_pair(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rdata, int width,
                  int height, int block_rows, int strip_rank, int strip_count, const void* term, int prepass_width,
                  int prepass_height, const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg,
                  const void* dfg, void* attempt_counter) {
    return trace_launch(p, stream, 2, plain_args(camera_generic, camera_quat, rdata, width, height, block_rows, strip_rank, strip_count, term, prepass_width,
                                                 prepass_height, e0, e1, e2, e3, cfg, dfg, attempt_counter));
}

int gr_trace_fused_adaptive(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rdata, int width,
                            int height, const void* term, int prepass_width, int prepass_height, const void* e0, const void* e1,
                            const void* e2, const void* e3, const void* cfg, const void* dfg, void* attempt_counter, int lattice,
                            int pending_only, void* lattice_rays) {
    gr_trace_fused_args a = plain_args(camera_generic, camera_quat, rdata, width, height, 0, 0, 1, term, prepass_width, prepass_height, e0, e1, e2, e3, cfg,
                                       dfg, attempt_counter);
    a.lattice = lattice;
    a.pending_only = pending_only;
    a.lattice_rays = lattice == 2 ? lattice_rays : nullptr;
    return trace_launch(p, stream, 1, a);
}

int gr_trace_fused_launch(gr_program* p, void* stream, const gr_trace_fused_args* args) {
    if (!args) return fail("null argument");
    gr_trace_fused_args a = *args;
    a.lattice = a.lattice == 2 ? 2 : 1;
    a.pending_only = a.pending_only ? 1 : 0;
    a.inline_prepass = a.inline_prepass ? 1 : 0;
    a.tile_order_by_history = a.tile_order_by_history ? 1 : 0;
    if (a.lattice != 2) a.lattice_rays = a.guessed = nullptr;
    return trace_launch(p, stream, 1, a);
}

int gr_adaptive_refine_strips(gr_program* p, void* stream, void* rdata, void* pending_count, int width, int height, const void* dfg,
                              int block_rows, int strip_rank, int strip_count, const void* lattice_rays, const void* cfg) {
    const strip_share share = strips(height, block_rows, strip_rank, strip_count, HEIGHT_ROUNDED_UP_TO_8);
    if (share.bad || share.block_rows % 8 != 0) return fail("bad strip description");
    if (lattice_rays && !cfg) return fail("gr_adaptive_refine: lattice_rays needs the metric's cfg");
    return refine_launch(p, stream, rdata, pending_count, width, height, dfg, share, lattice_rays, cfg, nullptr, 0, nullptr);
}

int gr_adaptive_refine(gr_program* p, void* stream, void* rdata, void* pending_count, int width, int height, const void* dfg,
                       const void* lattice_rays, const void* cfg) {
    return gr_adaptive_refine_strips(p, stream, rdata, pending_count, width, height, dfg, 0, 0, 1, lattice_rays, cfg);
}

size_t gr_pending_list_bytes(int width, int height) {
    if (width < 2 || height < 2) return 0;
    return (128 + 3 * (size_t)(width / 2) * (height / 2)) * sizeof(unsigned int);   // 64 class counts, 64 cursors, the pixels
}

size_t gr_lattice_rays_bytes(int width, int height) {
    if (width < 2 || height < 2) return 0;
    return (size_t)(width / 2) * (height / 2) * (3 * 16 + 4);   // three float4 of end state + the ray's attempts per lattice pixel
}

int gr_adaptive_refine_list(gr_program* p, void* stream, void* rdata, void* pending_count, int width, int height, const void* dfg, int block_rows,
                            int strip_rank, int strip_count, const void* lattice_rays, const void* cfg, void* pending_list,
                            const void* block_cost_before) {
    if (!p || !rdata || !pending_list) return fail("gr_adaptive_refine_list: null argument");
    const strip_share share = strips(height, block_rows, strip_rank, strip_count, HEIGHT_ROUNDED_UP_TO_8);
    if (share.bad || share.block_rows % 8 != 0) return fail("bad strip description");
    if (lattice_rays && !cfg) return fail("gr_adaptive_refine_list: lattice_rays needs the metric's cfg");
    HIP_CHECK(hipSetDevice(gr_internal::device_of(p)));
    HIP_CHECK(hipMemsetAsync(pending_list, 0, 128 * sizeof(unsigned int), (hipStream_t)stream));
    for (int phase = 0; phase < 2; phase++)
        GR_CHECK(refine_launch(p, stream, rdata, pending_count, width, height, dfg, share, lattice_rays, cfg, pending_list, phase, block_cost_before));
    return GR_OK;
}

int gr_trace_pending(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rdata, int width, int height,
                     const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg, const void* dfg, void* attempt_counter,
                     const void* pending_list, int waves_per_simd, void* block_cost, void* guessed_next) {
    if (!p || !rdata || !pending_list) return fail("gr_trace_pending: null argument");
    if (width < 2 || height < 2) return GR_OK;
    int per_cu = 0;
    GR_CHECK(resident_groups_per_cu(p, K_TRACE_PENDING, 256, &per_cu));
    const long long groups = pending_groups(facts_of(p).compute_units, per_cu, waves_per_simd, width, height);
    unsigned int* tickets = nullptr;
    GR_CHECK(draw_ticket(p, stream, &tickets));
    void* args[] = {&camera_generic, &camera_quat, &rdata, &width, &height, &e0, &e1, &e2, &e3, &cfg, &dfg, &attempt_counter, &tickets, &pending_list,
                    &block_cost, &guessed_next};
    return launch(p, K_TRACE_PENDING, stream, (unsigned)groups, 1, 256, 1, args);
}

size_t gr_guessed_bytes(void) { return (8 + (size_t)65536 * (1 + 1 + 8)) * sizeof(unsigned int); }   // program.hip: GR_GUESSED_HEADER, GR_GUESSED_CAPACITY pixels, attempts, records

int gr_apply_guessed(gr_program* p, void* stream, void* rdata, int width, const void* guessed, void* guessed_next, void* block_cost, void* attempt_counter) {
    if (!p || !rdata || !guessed || width < 2) return fail("gr_apply_guessed: null argument");
    void* args[] = {&rdata, &width, &guessed, &guessed_next, &block_cost, &attempt_counter};
    return launch(p, K_APPLY_GUESSED, stream, 65536 / 256, 1, 256, 1, args);
}

// gr_do_generic_rays over ray records in 8x8-tile slot order with the fused trace's scheduling (kernels/trace.hip): the device filled
// once, tiles drawn from a ticket counter in `tile_order`'s order (NULL: slot order), each tile's cost left in `tile_cost` (NULL: not).
int gr_do_generic_rays_scheduled(gr_program* p, void* stream, void* rays, const void* ray_count, int tile_count, const void* cfg, const void* dfg,
                                 void* attempt_counter, const void* tile_order, void* tile_cost) {
    if (!p || !rays || !ray_count) return fail("gr_do_generic_rays_scheduled: null argument");
    if (tile_count < 1) return GR_OK;
    int per_cu = 0;
    GR_CHECK(resident_groups_per_cu(p, K_DO_RAYS_SCHEDULED, 64, &per_cu));
    const long long groups = scheduled_groups(facts_of(p).compute_units, per_cu, tile_count);
    unsigned int* tickets = nullptr;
    GR_CHECK(draw_ticket(p, stream, &tickets));
    void* args[] = {&rays, &ray_count, &cfg, &dfg, &attempt_counter, &tickets, &tile_count, &tile_order, &tile_cost};
    return launch(p, K_DO_RAYS_SCHEDULED, stream, (unsigned)groups, 1, 64, 1, args);
}

int gr_sort_tiles_by_cost(gr_program* p, void* stream, const void* tile_cost, int tiles_x, int tiles_y, void* tile_order, void* work) {
    if (!p || !tile_cost || !tile_order || !work) return fail("gr_sort_tiles_by_cost: null argument");
    const int tile_count = tiles_x * tiles_y;
    if (tile_count < 1) return GR_OK;
    HIP_CHECK(hipSetDevice(gr_internal::device_of(p)));
    HIP_CHECK(hipMemsetAsync(work, 0, 128 * sizeof(unsigned int), (hipStream_t)stream));
    void* count_args[] = {&tile_cost, &tiles_x, &tiles_y, &work};
    GR_CHECK(launch(p, K_SORT_TILES_COUNT, stream, blocks(tile_count, 256), 1, 256, 1, count_args));
    int n = tile_count;
    void* place_args[] = {&n, &work, &tile_order};
    return launch(p, K_SORT_TILES_PLACE, stream, blocks(tile_count, 256), 1, 256, 1, place_args);
}

int gr_trace_compact(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rdata, int width,
                     int height, int block_rows, int strip_rank, int strip_count, const void* term, int prepass_width,
                     int prepass_height, const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg,
                     const void* dfg, void* attempt_counter, int keep_lanes) {
    if (keep_lanes < 1 || keep_lanes > 64) return fail("keep_lanes must be 1..64");
    const strip_share share = strips(height, block_rows, strip_rank, strip_count, HEIGHT_ROUNDED_UP_TO_8);
    if (share.bad || share.block_rows % 8 != 0) return fail("block_rows must be a positive multiple of 8 and 0 <= strip_rank < strip_count");
    if (share.strip_count > 1 && height > 1 && (height - 1) % share.block_rows == 0)
        return fail("the last image row must not start a block (its filter reads the row above)");
    block_rows = share.block_rows; strip_rank = share.strip_rank; strip_count = share.strip_count;
    const long long waves = device_tiles(width, height, share);
    if (waves <= 0) return GR_OK;
    if (waves * 64 > 0x7fffffffLL) return fail("too many ray slots");
    unsigned int total_slots = (unsigned int)(waves * 64);
    const long long groups = compact_groups(facts_of(p).compute_units, waves);
    unsigned int* tickets = nullptr;
    GR_CHECK(draw_ticket(p, stream, &tickets));
    void* args[] = {&camera_generic, &camera_quat, &rdata, &width, &height, &block_rows, &strip_rank, &strip_count, &term,
                    &prepass_width, &prepass_height, &e0, &e1, &e2, &e3, &cfg, &dfg, &attempt_counter, &tickets, &total_slots, &keep_lanes};
    return launch(p, K_TRACE_COMPACT, stream, (unsigned)groups, 1, 256, 1, args);
}

}  // extern "C"
