/* geodesic_hip_internal.h - the rest of libgeodesic_hip.so's exports: the launchers of the fused MI355X path (no reference counterpart),
 * its schedules (tile orders, tickets, the pending list of adaptive sampling), the knobs gr_render_frame picks them with
 * (gr_frame_tuning) and every measurement hook (stage timers, attempt / clock counters, build keys).  Tests, bench.py and tools/ use
 * them; the contract a maintainer binds is geodesic_hip.h.  Same conventions: 0 on success, device pointers owned by the caller. */
#ifndef GEODESIC_HIP_INTERNAL_H
#define GEODESIC_HIP_INTERNAL_H

#include "geodesic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- what gr_render_frame chooses among (gr_frame_options.tuning; NULL = these defaults) ------------------------------------- */
struct gr_frame_tuning {
    int ray_compaction;    /* fused mode: 0 = gr_trace_fused (one tile per wave at a time), 1..64 = gr_trace_compact with this
                            * keep_lanes; -1 = library default (off: the benchmark workloads keep > 95 % of their lanes busy) */
    int rays_per_lane;     /* fused mode without compaction: 1 = gr_trace_fused, 2 = gr_trace_pair (error if the program lacks it),
                            * 0 = library default: 2 where the program has the pair kernel, else 1 (GR_TRACE_RAYS_PER_LANE=1|2 overrides) */
    int fused_shading;     /* fused mode: 1 = the trace launch shades the 49 of every 64 pixels whose filter neighbours are in the same
                            * tile and gr_render_seams the rest (needs a program built with -DGR_TILE_SHADING, width and height
                            * multiples of 8, one ray per lane, no compaction, no adaptive sampling; an error otherwise);
                            * 0 or -1 (library default) = gr_render shades every pixel (measured faster: EXPERIMENTS.md C.2) */
    int inline_prepass;    /* fused mode, a frame whose prepass was not computed ahead (next_camera): trace the prepass grid inside
                            * the trace launch (gr_trace_fused_args.inline_prepass).  -1 (default): on whole frames that do not order
                            * their tiles; 1: also on a device's share of a split frame; 0: the prepass as a launch of its own in front */
    int trace_waves_per_simd;   /* fused mode: persistent waves per SIMD a trace launch takes, 1..8; 0 = as many as fit (best for
                            * one frame at a time).  With three or more frames in flight on streams of their own, 4 measured 2-3 % faster */
    int tile_history;      /* fused mode, one ray per lane: 1 = hand the tiles of this frame out dearest first by what they cost in this
                            * render state's previous frame (gr_order_tiles_by_history, shifted by how far the camera has moved the
                            * picture since); 0 = no; -1 = library default: whole frames of at most 32 tiles per wave slot that find no
                            * frame of ANOTHER stream still running on the device when they are submitted.  Scheduling only. */
    int park_lanes;        /* fused mode, one ray per lane, every pixel: 2..64 = gr_trace_fused_parking - a tile's wave with fewer than this many
                            * rays left after park_trips trips of the Verlet loop hands them over (gr_parking_lot); 0 = no; -1 = library
                            * default (GR_PARK="lanes,trips" in the environment, else off).  Scheduling only.  The program must have been
                            * built with -DGR_PARKING appended to its argument string (gr_program_has_parking): an error if asked for
                            * explicitly without it, ignored when it only comes from the environment. */
    int park_trips;        /* ... trips (two attempts each); <= 0 = library default (512) */
    /* -- what rides with the look-ahead cameras of gr_frame_options (next_camera, next_camera2) -- */
    int next_strip_rank;   /* strip_rank of the next_camera / next_camera2 frames when a device's share rotates from frame to frame; */
    int next_strip_rank2;  /*   -1 (default) = the same as this frame's.  gr_render_frame_tiled fills both in (gr_tiled_look_ahead). */
    float next_geodesic_time, next_geodesic_time2;   /* current_geodesic_time of the look-ahead frames (gr_frame_options.geodesic) */
    /* -- measurement -- */
    int count_attempts;    /* 1: accumulate the Verlet step attempts of this frame (gr_render_state_attempts) */
    /* -- an interactive caller that does not know the next camera (round 6) -- */
    int guess_still_camera;   /* fused mode, whole frames with a prepass, no next_camera given: 1 = when this frame repeats the previous frame of
                            * this render state (as below), take "the same again" as the NEXT frame's camera - its camera set-up and prepass
                            * then run on the side stream while this frame traces, exactly as for an announced next_camera, and are used only
                            * if the next frame's key matches bit for bit.  The prepass is still computed every frame (a measurement that must
                            * not skip it uses this with reuse_still_camera = 0); it has to find wave slots beside a trace launch that fills
                            * the device, and a long one (Kerr a = 0.9: 8 ms) that loses that race ends up in front of the next frame -
                            * profiles/r06_still_camera.txt.  0 = never; -1 = library default (off: reuse_still_camera supersedes it). */
    int reuse_still_camera;   /* fused mode, whole frames with a prepass and a Cartesian camera: 1 = a frame whose camera, parameters, features
                            * and program equal, bit for bit, those of the previous frame of this render state on the same stream takes that
                            * frame's camera set-up and prepass verdicts as they stand - both are functions of exactly those inputs and
                            * still sit in the state's buffers (a pointer to them handed out by gr_render_state_buffer ends that) - and
                            * launches neither.  A viewer whose user has stopped moving renders the same camera again and again; the
                            * reference pays the prepass's single-ray latency on each of those frames (main.cpp:2384-2437).  0 = never;
                            * -1 = library default (on).  gr_render_state_prepass_reused counts the frames that did. */
    int speculative_classes;  /* a whole frame that traces its prepass inside its trace launch and hands its tiles out by the frame before's
                            * costs (tile_history): gr_trace_fused_args.speculative_classes of its launch - n classes, 0 = none, -1 = library default */
};
void gr_frame_tuning_default(gr_frame_tuning* out);

/* ---- buffers of the frame driver's objects, the background build a program manager runs (tests and tools) ---- */
enum { GR_GEOBUF_PATH = 0, GR_GEOBUF_VELOCITY = 1, GR_GEOBUF_DS = 2, GR_GEOBUF_COUNT = 3, GR_GEOBUF_TRANSPORTED0 = 4,
       GR_GEOBUF_TRANSPORTED1 = 5, GR_GEOBUF_TRANSPORTED2 = 6, GR_GEOBUF_TRANSPORTED3 = 7 };
void* gr_geodesic_camera_buffer(gr_geodesic_camera* g, int which);

enum { GR_BUF_RAYS_IN = 0, GR_BUF_RAYS_COUNT = 1, GR_BUF_RENDER_DATA = 2, GR_BUF_TERMINATION = 3, GR_BUF_CAMERA_GENERIC = 4,
       GR_BUF_TETRAD0 = 5, GR_BUF_TETRAD1 = 6, GR_BUF_TETRAD2 = 7, GR_BUF_TETRAD3 = 8, GR_BUF_RAYS_ADAPTIVE = 9,
       GR_BUF_RAYS_ADAPTIVE_COUNT = 10, GR_BUF_CFG = 11, GR_BUF_DFG = 12, GR_BUF_CAMERA_QUAT = 13 };
/* device pointer of one of the state's buffers (NULL if not allocated).  Asking for the camera set, the prepass verdicts or the parameters
 * (anything but the ray and render-data records) tells the state that they may be written from outside: the next frame then does its own
 * camera set-up and prepass whatever gr_frame_tuning.reuse_still_camera says.  That holds for the NEXT frame only - a caller that keeps such
 * a pointer and writes through it in later frames renders those with reuse_still_camera = 0. */
void* gr_render_state_buffer(gr_render_state* s, int which);
/* A state made by gr_render_state_create_supersampled works at the TRACED size throughout - prepass, adaptive sampling, look-ahead, tile
 * history, both modes - and gr_render_state_buffer hands out its traced-size buffers (records of traced_width x traced_height pixels).
 * _supersample: the factor (1 for gr_render_state_create) and that size; any output may be NULL.  _resolve_ms: elapsed milliseconds of
 * the resolve launch of the last frame rendered with time_kernels = 1 (0 when it launched none); it has an event pair of its own
 * beside the GR_STAGE_* ones, whose GR_STAGE_RENDER covers the shading of the traced frame. */
int gr_render_state_supersample(const gr_render_state* s, int* factor, int* traced_width, int* traced_height);
int gr_render_state_resolve_ms(gr_render_state* s, float* ms);

/* counters of a program manager: out[0] parameter changes taken (gr_program_manager_update), [1] substituted programs swapped in, [2] substituted
 * builds started - never more than one of them is running -, [3] 1 while a build is running whose result nobody wants any more */
void gr_program_manager_counters(const gr_program_manager* pm, unsigned long long out[4]);

/* Background build of the "substituted" program (metric_manager.hpp:153-166, swapped in by check_substitution :172-219): create_async
 * returns at once; poll returns 1 and a loaded program when it is ready, 0 while pending, < 0 on a build error. */
typedef struct gr_program_future gr_program_future;
int gr_program_create_async(const char* argument_string, int device, gr_program_future** out);
/* compile only (no device): what gr_program_create_async's worker builds before the program can be swapped in - the code object of the
 * kernels a fused frame launches and the set-up module, side by side on two threads; fills the cache (bench.py: startup.program_build_s) */
int gr_program_precompile_frame_path(const char* argument_string);
int gr_program_future_poll(gr_program_future* f, gr_program** out);
void gr_program_future_destroy(gr_program_future* f);


/* gr_metric_info's operation counts for the substituted program of these parameter values (NULL = defaults): parameters that
 * make parts of a metric vanish - real rod lengths in the complex-valued double-Kerr family - shrink the DAG a good deal. */
int gr_metric_substituted_op_counts(const gr_metric* m, const float* cfg_values, int num_cfg_values, int* accel_ops,
                                    int* accel_transcendentals, int* coord_ops);


/* registers / scratch of a kernel as recorded in the code object (0 if unknown) */
int gr_program_kernel_info(const gr_program* p, const char* kernel_name, int* vgprs, int* sgprs, int* scratch_bytes);

/* render restricted to this device's row blocks (block-cyclic rows, see gr_trace_fused); render_data must be
 * pixel-indexed.  compact_out = 1 writes the device's blocks back to back (block i of this device at
 * out + i*block_rows*width float4), which is the layout the multi-GPU gather ships. */
int gr_render_strips(gr_program* p, void* stream, const void* render_data, void* out_rgba_f32,
                     const void* background1, const void* background2, int bg_width, int bg_height, int bg_levels,
                     int width, int height, int block_rows, int strip_rank, int strip_count, int compact_out,
                     int max_probes, const void* cfg, const void* dfg);
/* number of row blocks device `strip_rank` owns */
int gr_strip_local_blocks(int height, int block_rows, int strip_rank, int strip_count);
/* The box filter of a supersampled frame (kernels/resolve.hip, built into the set-up module: IEEE arithmetic): every float4 of dst
 * (width x height) is the sum of the factor x factor block of src (width*factor x height*factor) behind it, times 1.0f / factor^2, in
 * fp32; factor 1..4, 1 copies.  Rows as in gr_render_strips (strip_count <= 1: the whole image): with compact_out BOTH src and dst hold
 * the device's blocks back to back (a traced block is factor * block_rows rows), without it both are indexed by global row and only
 * this device's rows are read and written. */
int gr_resolve_supersampled(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int block_rows,
                            int strip_rank, int strip_count, int compact_out);
/* gr_resolve_supersampled fused with the 8-bit sRGB encode (kernels/present.hip, set-up module): dst_rgba8 holds one uint32 a pixel
 * (width x height; bytes R, G, B, A in memory order), each byte gr_frame_to_rgba8's of the value gr_resolve_supersampled would have
 * written - identical for every input but a NaN, whose byte is 0 here and undefined there.  Same arguments, same checks (all before
 * any device call), same row dealing; factor 1 encodes src as it is. */
int gr_present_rgba8(gr_program* p, void* stream, const void* src, void* dst_rgba8, int width, int height, int factor, int block_rows,
                     int strip_rank, int strip_count, int compact_out);
/* gr_present_rgba8's resolve and encode followed by gr_rgba8_to_yuv420's integer matrix (geodesic_hip.h), in one launch of the same
 * module: dst (device, gr_yuv420_bytes(width, height) bytes, layout GR_YUV420_I420 or GR_YUV420_NV12) holds exactly
 * gr_rgba8_to_yuv420(gr_present_rgba8(src)); no RGBA8 frame is written.  src: float4, width*factor x height*factor; factor 1..4.  Whole
 * frames only, every width and height >= 1 (width % 4 == 0 stores 4 bytes at a time, any other width single bytes).  Refused before any
 * device call: a NULL (the program included), a factor outside 1..4, a size below 1 or with more than 2^31 - 1 source pixels or more
 * than 524 280 rows, an unknown layout, dst not aligned to 4 bytes. */
int gr_present_yuv420(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int layout);
/* The bytes of a width x height frame in 8-bit Y'CbCr 4:2:0, either layout: width*height + 2 * ((width+1)/2) * ((height+1)/2), as geodesic_hip.h
 * ("video frames") gives it; 0 for a size below 1.  (Here and not there only because the contract header keeps to 80 names: the formula is public.) */
size_t gr_yuv420_bytes(int width, int height);
/* What defines that encode: out[k] = the smallest float of [0, 1] whose byte under gr_frame_to_rgba8 is >= k (out[0] = 0; +infinity for a
 * k no input reaches), found by bisection with the host function itself.  byte(c) = the largest k with out[k] <= c; the device searches
 * this table, so it agrees with the host's powf by construction.  NaN: the host conversion is undefined, the device writes 0. */
int gr_srgb8_thresholds(float out[256]);
/* Pinned host memory and an asynchronous download into it, for Python and tools (a C caller owns its streams and copies for itself):
 * a frame of gr_render_frame_rgba8 is fetched with _download_async on the frame's stream and a gr_stream_synchronize. */
int gr_host_alloc(size_t bytes, void** out);
int gr_host_free(void* ptr);
int gr_device_download_async(void* stream, void* host_dst, const void* device_src, size_t bytes);

/* ---- 10-bit video frames ------------------------------------------------------------------------------------------------------
 * The video frames of geodesic_hip.h with ten bits a sample: BT.709 Y'CbCr 4:2:0, limited range, every sample a 16-bit little-endian word.
 *
 * The 10-bit sRGB code of one linear value is the 8-bit chain of gr_frame_to_rgba8 with 1 023 for 255:
 *   code10(v) = (int)(clamp01(lin_to_srgb(clamp01(v))) * 1023.f), truncated, in float arithmetic with the library's own powf.
 * A NaN's code is undefined on the host and 0 on the device, as for bytes; values above 1, +infinity included, are clamped to 1 first;
 * negative values and -0 give 0.
 *
 * Matrix (int32 arithmetic on the codes R, G, B in 0 ... 1023, >> arithmetic): Y' = 64 + 876 E'y, Cb = 512 + 896 E'pb, Cr = 512 + 896 E'pr as
 *   per pixel:        Y  =  64 + (( 11931*R  + 40136*G  +  4052*B  +  32768) >> 16)
 *   per 2 x 2 block:  Cb = 512 + (( -6576*SR - 22124*SG + 28700*SB + 131072) >> 18)
 *                     Cr = 512 + (( 28700*SR - 26068*SG -  2632*SB + 131072) >> 18)      SR, SG, SB: the sums of its four pixels' codes
 * The coefficients are 876/1023 * 2^16 and 896/1023 * 2^16 times BT.709's weights, rounded; the luma row sums to 56 119 = round(876/1023 *
 * 2^16), each chroma row to 0.  So Y is in 64 ... 940 (black 64, white 940), Cb and Cr in 64 ... 960, a grey gives Cb = Cr = 512 exactly, and
 * every sample is within 0.51 of a code of the real-valued formula; the largest intermediate is about 1.2e8.
 *
 * Chroma siting and edges are the 8-bit rules: cw = (width+1)/2, ch = (height+1)/2; a sample is the mean of its four ENCODED pixels
 * (C420jpeg siting); an odd width or height counts the edge column or row twice.
 *
 * Layouts: a frame is gr_yuv420p10_bytes(width, height) = 2 * gr_yuv420_bytes(width, height) bytes, no padding.  GR_YUV420_I420 is
 * yuv420p10le: planes Y, Cb, Cr, the code in the LOW ten bits of each word.  GR_YUV420_NV12 is P010: the Y plane, then ch rows of cw
 * (Cb, Cr) word pairs, the code in the HIGH ten bits (code << 6, the low six bits zero).
 *
 * File: .y4m with the header "YUV4MPEG2 W<w> H<h> F<n>:<d> Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n"; per frame "FRAME\n" and the
 * GR_YUV420_I420 planes.
 *
 * Every function below refuses, before it writes anything, with GR_ERROR_INVALID_ARGUMENT and a message that names it: a NULL, a size
 * below 1, an unknown layout or depth, a code above 1 023 in rgb10. */
/* out[0] = 0; out[k] = the smallest float of [0, 1] whose code is >= k, found by bisection over the bit patterns 0 ... 0x3f800000 with
 * code10 itself; +infinity for every k above code10(1.0f), which need not be 1 023.  code10(c) = the number of k in 1 ... 1023 with
 * out[k] <= c: the device searches this table, so it agrees with the host's powf by construction. */
int gr_srgb10_thresholds(float out[1024]);
/* out_rgb: [height][width][3] codes of the frame's R, G, B; alpha is not encoded */
int gr_frame_to_rgb10(const float* frame_rgba_f32, int width, int height, unsigned short* out_rgb);
/* rgb10: [height][width][3] codes; out: gr_yuv420p10_bytes(width, height) bytes in `layout` - the definition above */
int gr_rgb10_to_yuv420p10(const unsigned short* rgb10, int width, int height, int layout, unsigned short* out);
/* 2 * gr_yuv420_bytes(width, height); 0 for a size below 1 */
size_t gr_yuv420p10_bytes(int width, int height);
/* gr_y4m_open with a depth: bit_depth 8 is gr_y4m_open byte for byte, 10 writes the C420p10 header and takes frames of
 * gr_yuv420p10_bytes in GR_YUV420_I420 order.  gr_y4m_write_frame and gr_y4m_close serve both (the handle knows its frame's size), with
 * the same rules for a short write. */
int gr_y4m_open_depth(const char* path, int width, int height, int fps_num, int fps_den, int bit_depth, gr_y4m** out);
/* gr_present_yuv420 with ten bits a sample (kernels/present.hip, set-up module): dst (device, gr_yuv420p10_bytes(width, height) bytes) holds
 * exactly gr_rgb10_to_yuv420p10(gr_frame_to_rgb10(the frame gr_resolve_supersampled would have written)) but for a NaN, whose code is 0.
 * Refused before any device call: what gr_present_yuv420 refuses, with dst aligned to 8 bytes where width % 4 == 0 (8-byte stores) and to
 * 2 bytes at any other width (stores of one word). */
int gr_present_yuv420p10(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int layout);
/* gr_render_frame_yuv420 with gr_present_yuv420p10 as its one launch after the frame.  Whole frames only: strip_count > 1 is refused before
 * anything is rendered, as a NULL, an unknown layout or a misaligned out_yuv420p10 (gr_present_yuv420p10's rule at the state's width) is. */
int gr_render_frame_yuv420p10(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera,
                              const gr_features* features, const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2,
                              int bg_width, int bg_height, int bg_levels, void* out_yuv420p10, int layout, const gr_frame_options* options);

/* ---- Motion-blurred frames --------------------------------------------------------------------------------------------------------
 * A shutter: a delivered frame is the weighted sum of T sub-frames rendered at T poses inside the frame's shutter interval, summed in linear
 * light (float4, before any encode) on the device; only the finished frame leaves it, in one of the four formats a plain frame leaves in.
 * (Declared here and not in geodesic_hip.h only because the contract header keeps to 80 names and 350 lines; all of this is public.)
 *
 * Definition, per float of the frame (all four channels, alpha included), with w the sub-frame's weight and r its resolved value - the
 * value gr_render_frame would have delivered for that pose, box average of a supersampled state included:
 *   the first sub-frame:   accum = w * r                one fp32 multiply, rounded to nearest even
 *   every later one:       accum = accum + (w * r)      that multiply, rounded, then one fp32 add, rounded - NEVER a fused multiply-add
 * in the order the sub-frames are submitted.  The first is not 0 + w * r: with w == 1.0f every value passes bit for bit, the sign of a zero
 * included.  NaN and infinity propagate as IEEE arithmetic has them (0 * inf is a NaN).  The library does NOT normalise weights: the caller's
 * weights are expected to sum to 1 (box weights: w = 1.0f / (float)T for every sub-frame; the sum of T of them need not be exactly 1).
 * The delivered frame is the encode of the final accum by the format's own definition: the float4 itself, gr_frame_to_rgba8,
 * gr_rgba8_to_yuv420(gr_frame_to_rgba8), or gr_rgb10_to_yuv420p10(gr_frame_to_rgb10) - a NaN's byte or code is 0 on the device. */
/* The host statement of one accumulation step over count_floats floats: with first != 0 accum[i] = weight * frame[i] (accum is not read),
 * otherwise accum[i] = accum[i] + weight * frame[i], as defined above; compiled so that the product and the sum are not contracted.
 * Refuses, with GR_ERROR_INVALID_ARGUMENT and a message that names it, a NULL accum or frame and a weight that is NaN or infinite;
 * count_floats == 0 does nothing.  accum and frame may be the same array. */
int gr_accumulate_frame(float* accum, const float* frame, size_t count_floats, float weight, int first);
/* The formats of gr_deliver_accumulated that GR_FRAME_F32 = 0 and GR_FRAME_RGBA8 = 1 (geodesic_hip.h) do not name; gr_render_frame_tiled_as
 * takes neither. */
enum { GR_FRAME_YUV420 = 2, GR_FRAME_YUV420P10 = 3 };
/* One accumulation step on the device (kernels/shutter.hip, set-up module: IEEE arithmetic, no contraction): src is a traced sub-frame,
 * float4 of width*factor x height*factor; accum is float4 of width x height; per pixel r = the value gr_resolve_supersampled would write
 * (the same function in the same compilation; factor 1..4, 1 takes src as it is) and accum = [accum +] weight * r as defined above.
 * With first != 0 accum is written and not read: no memset in front of a shutter, and whatever accum held - a NaN included - is gone.
 * Whole frames only.  Refused before any device call: a NULL (the program included), src == accum, a factor outside 1..4, a size below 1
 * or with more than 2^31 - 1 source pixels or more than 262 140 rows, a weight that is not finite. */
int gr_shutter_accumulate(gr_program* p, void* stream, const void* src, void* accum, int width, int height, int factor, float weight, int first);
/* One sub-frame of a shutter: renders the frame gr_render_frame would render for these arguments (same options: geodesic / geodesic_time,
 * next_camera ..., tuning - consecutive sub-frames are consecutive frames of the state, and a caller may announce the next sub-frame's camera)
 * into the state's traced frame and adds it with ONE gr_shutter_accumulate launch to an accumulation frame the state owns (float4, the
 * state's output size; allocated with the first sub-frame that is not refused, freed with the state).  first != 0 starts a new accumulation.
 * With time_kernels = 1 the accumulate launch is what gr_render_state_resolve_ms reports, beside the GR_STAGE_* times of the sub-frame.
 * Refused with GR_ERROR_INVALID_ARGUMENT and a message that names it - these three before any device call and before any object is looked
 * at: a NULL state, program, metric, camera or background; a weight that is not finite; options->strip_count > 1 (whole frames only) - and:
 * first == 0 on a state that holds no accumulation (none was started, or the last one's first sub-frame failed); what gr_render_frame
 * refuses.  Without a device: GR_ERROR_DEVICE. */
int gr_render_subframe(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera, const gr_features* features,
                       const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height, int bg_levels,
                       float weight, int first, const gr_frame_options* options);
/* The state's accumulation frame in `format`, by ONE launch of the format's existing kernel at factor 1 (gr_resolve_supersampled,
 * gr_present_rgba8, gr_present_yuv420, gr_present_yuv420p10): out (device) holds width x height float4 (GR_FRAME_F32), RGBA8 pixels
 * (GR_FRAME_RGBA8), gr_yuv420_bytes (GR_FRAME_YUV420) or gr_yuv420p10_bytes (GR_FRAME_YUV420P10) in `layout`, which the first two formats
 * ignore.  The accumulation stays as it is: it may be delivered again in another format, or added to.  Refused, with a message that names
 * it: a NULL; an unknown format; for the video formats an unknown layout, out not aligned to 4 bytes (8-bit) or to 8 bytes where the
 * state's width is a multiple of 4 and 2 bytes otherwise (10-bit); a state that holds no accumulation. */
int gr_deliver_accumulated(gr_render_state* s, gr_program* p, void* stream, int format, int layout, void* out);

/* ---- Filtered frames ----------------------------------------------------------------------------------------------------------------
 * Separable reconstruction filters behind a supersampled frame.  gr_resolve_supersampled is the mean of the f x f traced samples that lie
 * exactly behind a pixel - a box one pixel wide, the weakest filter there is.  A filtered frame weights the samples around the pixel's
 * centre with a table of n fp32 taps per axis instead (tent, Gaussian, Mitchell-Netravali, or the caller's own), on the device, before
 * any encode.  (Declared here and not in geodesic_hip.h only because the contract header keeps to 80 names and 350 lines; all of this is
 * public.)
 *
 * Definition.  The traced frame s is float4, W f x H f, f = 1 ... 4; the output is W x H.  A table has n taps, 1 <= n <= 16 and
 * n = f (mod 2), and is centred on the output pixel: tap t multiplies the traced sample at offset (f - n)/2 + t from the first sample of
 * the pixel's own block, at distance d_t = (t + 0.5 - n/2) / f output pixels from the pixel's centre.  The same table serves every pixel
 * and both axes.  The rows pass comes first, the columns pass second; per channel (all four, alpha included):
 *   h(y, X)   = acc after: acc = taps[0] * s(y, cx(X,0));  for t = 1 ... n-1: acc = acc + (taps[t] * s(y, cx(X,t)))     every traced row y
 *   out(Y, X) = acc after: acc = taps[0] * h(cy(Y,0), X);  for t = 1 ... n-1: acc = acc + (taps[t] * h(cy(Y,t), X))
 *   cx(X,t) = clamp(X f + (f - n)/2 + t, 0, W f - 1)        cy(Y,t) = clamp(Y f + (f - n)/2 + t, 0, H f - 1)
 * Every product and every sum is one fp32 operation rounded to nearest even - NEVER a fused multiply-add - in ascending t, and h is
 * rounded to fp32 between the passes: the two-pass form with a rounded intermediate is part of the definition.  The first term is
 * taps[0] * s and not 0 + ...: a single tap of 1.0f passes every value bit for bit, the sign of a zero included.  A sample past an edge
 * is the edge sample.  Taps of weight 0 are not skipped; NaN and infinity propagate as IEEE arithmetic has them. */
#define GR_FILTER_MAX_TAPS 16
/* The named filters.  GR_FILTER_BOX is gr_resolve_supersampled's path and has no table. */
enum { GR_FILTER_BOX = 0, GR_FILTER_TENT = 1, GR_FILTER_GAUSSIAN = 2, GR_FILTER_MITCHELL = 3 };
/* The taps of a named filter at factor 1 ... 4: tent (radius R = 1), Gaussian (R = 2) or Mitchell-Netravali with B = C = 1/3 (R = 2).
 * *count = n = 2 R f for an even f, 2 R f - 1 for an odd one: the taps with |d_t| < R.  k(d), in double from |d|: tent 1 - |d|; Gaussian
 * exp(-2 d^2) - exp(-8); Mitchell ((12 - 9B - 6C)|d|^3 + (-18 + 12B + 6C)|d|^2 + (6 - 2B)) / 6 below 1 and
 * ((-B - 6C)|d|^3 + (6B + 30C)|d|^2 + (-12B - 48C)|d| + (8B + 24C)) / 6 from 1 to 2.  taps[t] = (float)(k(d_t) / sum of k(d_t) over
 * ascending t, in double).  The library does NOT renormalise after rounding: the fp32 taps need not sum to exactly 1 (they are within
 * n 2^-24 of it).  Tent at factor 1 is {1.0f}; at factor 2 it is {0.125, 0.375, 0.375, 0.125} exactly.  Refused, with
 * GR_ERROR_INVALID_ARGUMENT and a message that names it: a NULL, a factor outside 1 ... 4, an unknown filter, and GR_FILTER_BOX, which has
 * no table - its frame is gr_resolve_supersampled's. */
int gr_filter_taps(int filter, int factor, float taps[GR_FILTER_MAX_TAPS], int* count);
/* The host statement of the definition above: src is float[4 * width*factor * height*factor], dst float[4 * width * height]; compiled so
 * that no product and sum are contracted.  Refused before anything is written, with GR_ERROR_INVALID_ARGUMENT and a message that names
 * it: a NULL; a size below 1; a factor outside 1 ... 4; count outside 1 ... 16 or of the wrong parity; a tap that is not finite;
 * src == dst. */
int gr_filter_frame(const float* src, int width, int height, int factor, const float* taps, int count, float* dst);
/* The same on the device by ONE launch (kernels/filter.hip, set-up module: IEEE arithmetic, no contraction), bit for bit: src and dst
 * are device memory, taps is HOST memory (the table travels in the kernel's argument block).  Whole frames only.  Refused before any
 * device call: what gr_filter_frame refuses, a NULL program, more than 2^31 - 1 source pixels, more than 524 280 rows. */
int gr_resolve_filtered(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, const float* taps, int count);
/* The filter of a state's frames: GR_FILTER_BOX (the default: every entry point is as it was, launch for launch) or a named filter, at
 * any factor, 1 included (Mitchell and Gaussian are a mild post-filter there, tent is the identity).  With a filter set,
 * gr_render_frame, gr_render_frame_rgba8, gr_render_frame_yuv420 and gr_render_frame_yuv420p10 deliver gr_filter_frame of the traced
 * frame with gr_filter_taps' table: gr_resolve_filtered from the traced frame into a frame the state owns (float4 at the output size,
 * allocated with the first frame that is not refused, freed with the state; a float4 delivery goes straight into `out`), then the
 * format's own kernel at factor 1 from it; both launches are what gr_render_state_resolve_ms reports.  gr_render_subframe accumulates the
 * filtered frame.  A filtered state renders whole frames only: strip_count > 1 and gr_render_frame_tiled / _tiled_as are refused before
 * anything is rendered (a filter wider than a pixel reads across strip borders).  gr_render_state_set_filter refuses a NULL and an unknown
 * filter; it may be called between frames. */
int gr_render_state_set_filter(gr_render_state* s, int filter);
int gr_render_state_filter(const gr_render_state* s, int* filter);

/* ---- Analytic sky -----------------------------------------------------------------------------------------------------------------------
 * A coloured celestial sphere with a latitude / longitude grid, shaded on the device from the pixel's footprint in closed form: a second
 * shading kernel beside gr_render (kernels/shading.hip: gr_render_analytic) that reads the same records and writes the same float4 frame,
 * with no sky image, no mip pyramid and no gathers.  The grid is antialiased exactly at any magnification.  (Declared here and not in
 * geodesic_hip.h only because the contract header keeps to 80 names and 350 lines; all of this is public.)
 *
 * Definition.  A pixel has the record `self` with sky coordinates (u, v) = render_data.tex_coord and the records of its neighbours
 * `beside` and `below`, chosen exactly as gr_render chooses them: the next pixel of the row / column, the previous one at the last column
 * / row, the pixel itself in a frame one pixel wide / high.
 *   1. footprint   du_x, dv_x are the wrapped differences (b - a brought into half a turn either way, as gr_render forms them, without its
 *                  shrink by 1.3) from self to beside, du_y, dv_y those from self to below.  hu = max((|du_x| + |du_y|) / 2, 2^-14),
 *                  hv = max((|dv_x| + |dv_y|) / 2, 2^-14).  The floor makes the result a continuous function of the record.
 *   2. lines       a pulse train filtered by a box of the footprint's size.  For n cells and a width w: t = x n, a = h n, s(t) = t + w/2,
 *                  k = floor(s), f = s - k, L(t) = k w + min(f, w); the coverage is c = (L(t + a) - L(t - a)) / (2 a).  c_u takes
 *                  (u, hu, meridians), c_v takes (v, hv, parallels); the pattern continues periodically past the poles.
 *                  g = 1 - (1 - c_u)(1 - c_v).  (An fp32 evaluation differences the integer parts k before it multiplies them by w, and
 *                  takes the fraction of t from the EXACT product x n, rounded once - by any means that is exact: the pair x n and
 *                  fma(x, n, -(x n)) under IEEE rules, or the product in double, which the device kernel uses because its build
 *                  contracts and reassociates fp32 - so that the error is a few ulps of a cell and not of n cells.)
 *   3. quadrants   the same box.  H(x) = floor(x) / 2 + max(x - floor(x) - 1/2, 0), f_u = (H(u + hu) - H(u - hu)) / (2 hu);
 *                  G(y) = max(y - 1/2, 0), f_v = (G(v + hv) - G(v - hv)) / (2 hv).  base = the mix of the side's four quadrant colours
 *                  with the weights (1 - f_u)(1 - f_v), f_u (1 - f_v), (1 - f_u) f_v, f_u f_v for q = 0, 1, 2, 3.
 *   4. colour      rgb = base + (line - base) g, alpha 1; from there gr_render's colour tail unchanged: with the redshift feature the
 *                  colour is linearised, shifted by self.z_shift and, unless the program has a linear framebuffer, brought back to sRGB;
 *                  without it the colour is linearised only under a linear framebuffer.
 *   5. black       a record with terminated != 1 gives exactly (0, 0, 0, 1). */
struct gr_analytic_sky {
    int meridians;              /* lines of constant u per turn, 2 ... 360 */
    int parallels;              /* cells between the poles, 1 ... 180 */
    float line_width;           /* full width of a line as a fraction of its cell, 0 (no lines) ... 0.5 */
    float quadrant[2][4][3];    /* [side][q][rgb], stored values in [0, 1] as a sky image's texels are (sRGB); q = (u >= 0.5) + 2 (v >= 0.5);
                                 * side 0 = the far sky (render_data.side < 1, gr_render's background2), side 1 = the near sky (side >= 1,
                                 * background1) */
    float line[2][3];           /* the lines' colour per side */
};
/* 36 x 18 cells (10 degrees), line_width 0.08, four distinct quadrant colours per side - another palette on side 1 - and near-black lines */
int gr_analytic_sky_default(struct gr_analytic_sky* out);
/* gr_render with the sky's description in place of the textures: one launch of gr_render_analytic over num_pixels records, out as there.
 * Everything below that takes a sky refuses, before any device call, with GR_ERROR_INVALID_ARGUMENT and a message that names the function
 * and the field: a NULL; meridians, parallels or line_width out of range or not finite; a colour outside [0, 1] or not finite; and the
 * launchers what gr_render / gr_render_strips refuse (a NULL buffer, bad strip parameters). */
int gr_render_analytic(gr_program* p, void* stream, const void* render_data, const void* render_data_count, int num_pixels, void* out_rgba_f32,
                       const struct gr_analytic_sky* sky, int width, int height, const void* cfg, const void* dfg);
/* ... restricted to a device's row blocks: gr_render_strips' arguments, rows and compact_out */
int gr_render_analytic_strips(gr_program* p, void* stream, const void* render_data, void* out_rgba_f32, const struct gr_analytic_sky* sky,
                              int width, int height, int block_rows, int strip_rank, int strip_count, int compact_out, const void* cfg,
                              const void* dfg);
/* The host rasteriser of the same definition, in double, at the footprint of one texel: texel (x, y) of a width x height image has
 * u = (x + 0.5) / width, v = (y + 0.5) / height, hu = 0.5 / width, hv = 0.5 / height (differences along the axes; the 2^-14 floor applies),
 * the colour of steps 2 to 4 up to rgb = base + (line - base) g as it is stored (sRGB, no redshift), each channel rounded to the nearest of
 * 255 steps, alpha 255.  side: 0 or 1.  out_rgba8: width * height * 4 bytes.  The same sky can so be sent down the texture path. */
int gr_analytic_sky_image(const struct gr_analytic_sky* sky, int side, int width, int height, unsigned char* out_rgba8);
/* The sky of a state's frames.  NULL (the default): every entry point is as it was, launch for launch.  With a sky set, every frame of the
 * state - gr_render_frame and its three encoded forms, gr_render_subframe, gr_render_frame_tiled(_as), both modes, split and supersampled
 * frames - is shaded by gr_render_analytic in place of gr_render / gr_render_strips; tile shading inside the trace
 * (gr_frame_tuning.fused_shading) is not taken for such a frame; background1, background2 and their sizes are ignored and may be NULL / 0.
 * May be called between frames; the traced records do not depend on it, so nothing of the still-camera reuse is invalidated.
 * gr_render_state_sky: *is_set = 1 and the sky in *out, or 0 and *out untouched. */
int gr_render_state_set_sky(gr_render_state* s, const struct gr_analytic_sky* sky_or_null);
int gr_render_state_sky(const gr_render_state* s, struct gr_analytic_sky* out, int* is_set);

/* ---- Star sky -------------------------------------------------------------------------------------------------------------------------
 * Point stars lensed on the device.  A star is unresolved: its brightness in a pixel goes as the inverse of the solid angle the pixel's rays
 * cover on the sky, which no sky image can carry.  A third shading kernel beside gr_render and gr_render_analytic (kernels/shading.hip:
 * gr_render_stars) reads the same records and writes the same float4 frame, and gathers from a star catalogue that is built on the device
 * (kernels/stars.hip, csrc/star_catalogue.cpp).  (Declared here for the reason "Analytic sky" gives; all of this is public.)
 *
 * A catalogue is n stars, 1 <= n <= 2^24.  Star s has a position (u_s, v_s) in the sky coordinates of render_data.tex_coord - u periodic in
 * [0, 1), v in [0, 1] - and flux_s[3] >= 0: linear-light RGB per unit of (u, v) area.  Whoever makes the catalogue divides a star's flux per
 * steradian by 2 pi^2 sin(pi v) once, on the host.  A catalogue has cells_u x cells_v cells, both powers of two from 16 to 4096 (0: the
 * defaults, 1024 x 512).  Star s lies in cell (min(floor(u_s cells_u), cells_u - 1), min(floor(v_s cells_v), cells_v - 1)) - exact in fp32,
 * the cell counts being powers of two; cell (i, j) has the number j cells_u + i.
 *
 * Definition.  A pixel has `self` with (u, v) = tex_coord (finite, in [0, 1]), `beside` and `below`, chosen exactly as gr_render and
 * gr_render_analytic choose them.
 *   1. footprint   hu = max((|du_x| + |du_y|) / 2, min_footprint), hv alike from dv_x, dv_y: the wrapped differences of "Analytic sky"
 *                  step 1.  min_footprint is a field of the star sky, a power of two from 2^-20 to 2^-8, default 2^-16: the angular size
 *                  below which a star is no longer a point - the cap on magnification and the knob against twinkling.  (The analytic sky's
 *                  fixed 2^-14 is above an ordinary 4K pixel's half-size and would smear every star.)
 *   2. regime      in fp32, every operation a single IEEE operation or a multiplication by a power of two, so that no contraction or
 *                  reassociation changes it and a model repeats the decision bit for bit:
 *                      r_u = 2 hu + 2^-22,  i0 = floor((u - r_u) cells_u),  i1 = floor((u + r_u) cells_u),
 *                      r_v = 2 hv + 2^-22,  j0 = floor((v - r_v) cells_v),  j1 = floor((v + r_v) cells_v).
 *                  NEAR if i1 - i0 <= 3 and j1 - j0 <= 3, otherwise FAR.
 *   3. near        the stars themselves.  S = sum_s flux_s T(d_u / (2 hu)) T(d_v / (2 hv)) / (4 hu hv), T(x) = max(1 - |x|, 0);
 *                  d_v = v_s - v, d_u = the difference u_s - u brought into half a turn either way, d - rint(d) (an fp32 evaluation forms
 *                  it without rounding a position against the turn: (u_s - 1) - u for a star in front of the seam seen from behind it,
 *                  u_s - (u - 1) the other way round).  The sum runs over the stars of the cells i0 ... i1 (taken modulo cells_u: the
 *                  sphere closes in u) x max(j0, 0) ... min(j1, cells_v - 1) (clipped: nothing is mirrored across a pole), rows in
 *                  ascending j, within a row cells in the order i0 ... i1, within a cell stars in ascending catalogue index.  The tent's
 *                  half-width is the spacing of the neighbours: on a regular lattice of pixels the weights of a star add up to one, so
 *                  no star falls between pixels.  The margin of 2^-22 makes the cells visited a superset of the tent's support whatever
 *                  the rounding.
 *   4. far         the stars as a glow.  S = (I(u + hu, v1) - I(u - hu, v1) - I(u + hu, v0) + I(u - hu, v0)) / (4 hu hv),
 *                  v0 = max(v - hv, 0), v1 = min(v + hv, 1).  I is the bilinear interpolation of the catalogue's summed-area table: per
 *                  channel, float64, (cells_v + 1) x (cells_u + 1), a zero first row and column, entry [j][i] the summed flux of the cells
 *                  below i and j.  A cell's sum is taken in ascending catalogue index, the prefixes run along u, then along v.  For
 *                  0 <= x <= 1: X = x cells_u, i = min(floor(X), cells_u - 1), a = X - i, likewise j, b from y and cells_v,
 *                  I(x, y) = (1 - a)(1 - b) t[j][i] + a (1 - b) t[j][i + 1] + (1 - a) b t[j + 1][i] + a b t[j + 1][i + 1];
 *                  I continues periodically in u: I(x + k, y) = I(x, y) + k I(1, y) for x in [0, 1) and whole k.  Evaluated in double on the
 *                  device: few pixels are far, and the four terms cancel (over an empty stretch of sky they leave a residue of either
 *                  sign, some 2^-53 of the table's total over the footprint's area).
 *   5. colour      L = srgb_to_linear(background[side]) + S, alpha 1.  With the redshift feature apply_redshift(L, z_shift), then
 *                  linear_to_srgb unless the program has a linear framebuffer; without it L under a linear framebuffer, linear_to_srgb(L)
 *                  otherwise (gr_render's colour tail, entered in linear light).  Values above 1 stay in the float4 frame; the 8-bit and
 *                  video sinks clamp, as they do for any frame.
 *   6. side        self.side >= 1 takes the near catalogue and background[1], otherwise the far one and background[0] (background1 and
 *                  background2 of gr_render).  A NULL catalogue on a side means S = 0 there.
 *   7. black       a record with terminated != 1 gives exactly (0, 0, 0, 1). */
typedef struct gr_star_catalogue gr_star_catalogue;
struct gr_star_sky {
    float min_footprint;       /* step 1: a power of two, 2^-20 ... 2^-8 */
    float background[2][3];    /* [side][rgb], stored (sRGB) values in [0, 1] behind the stars; side as in gr_analytic_sky */
};
/* min_footprint 2^-16, both backgrounds black */
int gr_star_sky_default(struct gr_star_sky* out);
/* Uploads the 20 bytes a star (uv[2 n], flux[3 n]) to the program's device and builds everything else there: a cell histogram, an
 * exclusive scan (cell_start[cells + 1]), a scatter, a per-cell ordering that leaves every cell's stars in ascending catalogue index, the
 * stars' records in that order, the per-cell float64 sums and the two prefix passes.  The result is a function of the inputs alone: two
 * builds give the same bytes.  The catalogue borrows the program (its set-up module holds the kernels) for the length of this call only,
 * and lives on the program's device.  The ordering is a sorting network a cell: its cost grows as m log^2 m with the m stars of the
 * fullest cell.  Refused before any device call, with GR_ERROR_INVALID_ARGUMENT and a message that names the function and the field: a
 * NULL; n, cells_u or cells_v out of range or no power of two; a uv outside its range or not finite; a flux that is negative or not finite. */
int gr_star_catalogue_create(gr_program* p, int n, const float* uv, const float* flux, int cells_u, int cells_v, gr_star_catalogue** out);
void gr_star_catalogue_destroy(gr_star_catalogue* c);
int gr_star_catalogue_info(const gr_star_catalogue* c, int* n, int* cells_u, int* cells_v);
/* for tests: cell_start[cells_u cells_v + 1], order[n] (the catalogue indices as the device holds the stars, cell by cell) and
 * table[3][cells_v + 1][cells_u + 1]; any of the three may be NULL */
int gr_star_catalogue_download(const gr_star_catalogue* c, int* cell_start, int* order, double* table);
/* A random field, on the host and in double: n stars uniform on the sphere from one splitmix64 stream.
 *   next():  state += 0x9E3779B97F4A7C15 (state starts as seed); z = state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31; x = (z >> 11) * 2^-53.
 *   star s draws x1, x2, x3, x4 in that order (draws 4 s + 1 ... 4 s + 4 of the stream).
 *   u = x1, stored as float (a float of 1 is stored as 0);  V = acos(1 - 2 x2) / pi, stored as float.
 *   brightness: a power law of slope -5/2 above f0 = 2e-9 per steradian (the Euclidean counts N(> f) ~ f^-3/2), cut at 10^4 f0:
 *            f = f0 min((1 - x3)^(-2/3), 1e4).
 *   colour:  class k = min(floor(7 x4), 6) of O B A F G K M, linear RGB (0.61, 0.71, 1), (0.68, 0.77, 1), (0.80, 0.85, 1), (0.97, 0.96, 1),
 *            (1, 0.92, 0.82), (1, 0.78, 0.56), (1, 0.58, 0.33).
 *   flux[c] = f colour[k][c] / (2 pi^2 max(sin(pi V), 1e-3)), stored as float.
 * out_uv[2 n], out_flux[3 n]; 1 <= n <= 2^24. */
int gr_star_field_random(unsigned long long seed, int n, float* out_uv, float* out_flux);
/* gr_render_analytic with the star sky in place of the analytic one: one launch of gr_render_stars over num_pixels records.  near / far:
 * the catalogues of side 1 / side 0, either may be NULL (step 6), both must live on the program's device.  The launchers and the state's
 * setter refuse, before any device call and by the function's and the field's name: a NULL sky, min_footprint out of range or no power
 * of two, a background outside [0, 1] or not finite, a catalogue of another device, and what gr_render / gr_render_strips refuse. */
int gr_render_stars(gr_program* p, void* stream, const void* render_data, const void* render_data_count, int num_pixels, void* out_rgba_f32,
                    const struct gr_star_sky* sky, const gr_star_catalogue* near_or_null, const gr_star_catalogue* far_or_null, int width,
                    int height, const void* cfg, const void* dfg);
int gr_render_stars_strips(gr_program* p, void* stream, const void* render_data, void* out_rgba_f32, const struct gr_star_sky* sky,
                           const gr_star_catalogue* near_or_null, const gr_star_catalogue* far_or_null, int width, int height, int block_rows,
                           int strip_rank, int strip_count, int compact_out, const void* cfg, const void* dfg);
/* The stars of a state's frames.  sky NULL (the default): every entry point is as it was, launch for launch.  With stars set, every frame
 * of the state - on every path gr_render_state_set_sky lists - is shaded by gr_render_stars; it never shades inside the trace and reads
 * no background image (background1, background2 may be NULL).  The catalogues are borrowed: they must outlive the state's frames.  A state
 * that has an analytic sky refuses stars, and a state with stars refuses an analytic sky: composing the two is not defined.
 * gr_render_state_stars: *is_set = 1 and the three in *out, *near, *far, or 0 and those untouched. */
int gr_render_state_set_stars(gr_render_state* s, const struct gr_star_sky* sky_or_null, const gr_star_catalogue* near_or_null,
                              const gr_star_catalogue* far_or_null);
int gr_render_state_stars(const gr_render_state* s, struct gr_star_sky* out, const gr_star_catalogue** near, const gr_star_catalogue** far, int* is_set);

/* ---- Glare ------------------------------------------------------------------------------------------------------------------------------
 * A point-spread function and an exposure, applied to the resolved frame on the device in linear light, between the resolve (box or
 * filter) and the sink.  A lensed point star reaches hundreds (Star sky, step 5) and the 8-bit and video sinks clamp at 1: without this
 * stage a star of brightness 1 and one of 400 are the same white pixel in every file.  A camera, an eye or a telescope shows a bright
 * point as a sharp core inside a halo - the frame convolved with a PSF - and that is how a bright star reads as bright in 8 bits.  The
 * PSF is a core plus up to four separable components; a plain gain is the PSF with no components.  (Declared here and not in
 * geodesic_hip.h only because the contract header keeps to 80 names and 350 lines, so that header gains nothing; all of this is public.)
 *
 * Definition.  s is the source, float4, W x H.  For the channels r, g and b, for every component k in ascending order, with n_k taps and
 * R_k = (n_k - 1) / 2:
 *   h_k(y, X) = acc after: acc = tap_k[0] * s(y, cx(X,0));    for t = 1 ... n_k-1: acc = acc + (tap_k[t] * s(y, cx(X,t)))     every row y
 *   g_k(Y, X) = acc after: acc = tap_k[0] * h_k(cy(Y,0), X);  for t = 1 ... n_k-1: acc = acc + (tap_k[t] * h_k(cy(Y,t), X))
 *   cx(X,t) = clamp(X - R_k + t, 0, W - 1)      cy(Y,t) = clamp(Y - R_k + t, 0, H - 1)
 * then
 *   out(Y, X) = acc after: acc = core * s(Y, X);  for k = 0 ... K-1: acc = acc + (weight[k] * g_k(Y, X))
 * Every product and every sum is one fp32 operation rounded to nearest even - NEVER a fused multiply-add - in the order written, and h_k
 * and g_k are rounded to fp32.  Tap t multiplies the sample at offset t - R_k: the correlation form, as in "Filtered frames", so a single
 * bright pixel comes out as the table reversed.  A sample past an edge is the edge sample, so a uniform frame stays uniform.  Alpha is
 * not convolved: out.w is s.w, bit for bit.  The first term is core * s and not 0 + ...: with core 1.0f and K = 0 every r, g and b value
 * passes unchanged, the sign of a zero included.  Taps and weights of 0 are not skipped.  NaN and infinity propagate as IEEE arithmetic has
 * them: a NaN pixel spreads over the whole footprint of the PSF (a cross of 2 R_k + 1 rows and columns becomes a square of NaN), and an
 * infinity next to a tap of 0 is a NaN. */
#define GR_GLARE_MAX_COMPONENTS 4
#define GR_GLARE_MAX_TAPS 129
struct gr_glare {
    float core;                                   /* finite */
    int components;                               /* K, 0 ... 4 */
    float weight[GR_GLARE_MAX_COMPONENTS];        /* finite */
    int taps[GR_GLARE_MAX_COMPONENTS];            /* n_k: odd, 1 ... 129; R_k = (n_k - 1) / 2 */
    float tap[GR_GLARE_MAX_COMPONENTS][GR_GLARE_MAX_TAPS];   /* finite; the first n_k of a row are read */
};
/* Every function below refuses, before any device call and before it writes anything, with GR_ERROR_INVALID_ARGUMENT and a message that
 * names the function and the field.  Of a struct gr_glare only core, components and the first `components` weights, counts and rows are
 * looked at. */
/* The named PSF: `count` Gaussians, 0 ... 4.  Component k has R_k = min(ceil(3 sigma_k), 64) and the taps (float)(exp(-d^2 / (2 sigma_k^2)) /
 * sum), d = t - R_k, evaluated in double, the sum taken in ascending t; core = (float)(1 - the sum of the weights, in double).  The taps
 * are NOT renormalised after rounding (they sum to 1 within n_k 2^-24).  Everything of *out that the PSF does not use is zero.  Refused: a
 * NULL; a count outside 0 ... 4; a sigma not in (0, 64] or not finite; a weight outside [0, 1] or not finite; weights that sum to more
 * than 1. */
int gr_glare_gaussians(const float* sigma, const float* weight, int count, struct gr_glare* out);
/* Exposure: core and all four weights times (float)exp2((double)stops), each one fp32 product.  Refused: a NULL, stops that are not
 * finite or lie outside -32 ... 32. */
int gr_glare_exposure(struct gr_glare* g, float stops);
/* The host statement of the definition: src and dst are float[4 * width * height]; compiled so that nothing is contracted.  Refused before
 * anything is written: a NULL; a size below 1; src == dst; a field of *g out of its range. */
int gr_glare_frame(const float* src, int width, int height, const struct gr_glare* g, float* dst);
/* The same on the device, bit for bit (kernels/glare.hip, set-up module: IEEE arithmetic, no contraction), asynchronous on `stream`: src,
 * dst and scratch are device memory, *g is HOST memory (the one table a launch applies travels in its argument block).  K = 0 is one
 * elementwise launch; otherwise a rows launch into scratch and a columns launch that adds the component into dst, 2 K in all.  Whole
 * frames only.  gr_glare_scratch_bytes: what scratch must hold for a frame of that size - one float4 frame.  Refused: what gr_glare_frame
 * refuses; a NULL program; scratch that is NULL, shorter than that or not aligned to 16 bytes; any overlap of src, dst and scratch; more
 * than 2^31 - 1 pixels. */
int gr_glare_scratch_bytes(int width, int height, size_t* bytes);
int gr_apply_glare(gr_program* p, void* stream, const void* src, void* dst, void* scratch, size_t scratch_bytes, int width, int height,
                   const struct gr_glare* g);
/* The glare of a state's frames.  NULL (the default): every entry point is as it was, launch for launch.  With a glare set,
 * gr_render_frame, gr_render_frame_rgba8, gr_render_frame_yuv420 and gr_render_frame_yuv420p10 deliver gr_glare_frame of the frame they
 * would have delivered as float4: the frame is resolved into a frame the state owns (gr_resolve_supersampled or gr_resolve_filtered; a
 * factor-1 box state's traced frame is the source as it is - it no longer renders straight into `out`, but for out == NULL), then
 * gr_apply_glare into a second frame of the state - a float4 delivery goes straight into `out` -, then the format's own kernel at factor 1.
 * The state's frames and scratch are allocated with the first frame that is not refused and freed with the state; all these launches lie
 * between the events of gr_render_state_resolve_ms.  gr_render_subframe accumulates the frame WITHOUT the glare and
 * gr_deliver_accumulated applies it to the accumulation, into the state's own frame, before the encode: the glare is linear, so that is
 * one application a frame, it is the definition, and the accumulation stays as it is.  A state with a glare renders whole frames only:
 * strip_count > 1 and gr_render_frame_tiled / _tiled_as are refused before anything is rendered (the PSF reads across strip borders).
 * gr_render_state_set_glare refuses a NULL state and a field out of range; it may be called between frames.  gr_render_state_glare:
 * *is_set = 1 and the glare in *out, or 0 and *out untouched. */
int gr_render_state_set_glare(gr_render_state* s, const struct gr_glare* glare_or_null);
int gr_render_state_glare(const gr_render_state* s, struct gr_glare* out, int* is_set);

/* ---- Metering and tone curve ----------------------------------------------------------------------------------------------------------
 * The gain that puts a frame into the range the sinks keep, chosen on the device from the frame itself, and a curve that rolls highlights
 * off instead of clipping them.  Both sit after the glare and before the encode, and nothing on the frame path waits for the host: the
 * meter reduces the finished frame to a luminance histogram, one wave solves it to an exposure and adapts it from frame to frame, and the
 * curve reads the gain from the device word the solve wrote.  (Declared here for the reason "Glare" gives: the contract header gains
 * nothing.)
 *
 * 1. The histogram - exact integers.  s is the source, float4, W x H.  Per pixel
 *      Y = ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b)          five fp32 operations, each rounded once, NEVER fused
 *    black: Y > 0 is false (a zero of either sign, a negative value, NaN): counted in hist[384].  Otherwise e = bits(Y) >> 20 (the exponent
 *    and the top three bits of the mantissa: 8 bins an octave) and bin = clamp((int)e - 824, 0, 383); 824 = (127 - 24) * 8, so bin 0 starts
 *    at 2^-24 and bin 383 ends below 2^24; everything smaller, subnormals included, lands in bin 0, everything larger, +infinity included,
 *    in bin 383.  The pixel is counted in hist[bin].  hist is 385 uint32 counters; a frame has at most 2^31 - 1 pixels, so none overflows.
 *    No logarithm is taken, the counts are a function of the frame alone, and host and device agree exactly.
 * 2. The solve - double, a handful of operations, every one a single IEEE double operation, none contracted, host and device the same bits.
 *      N = hist[0] + ... + hist[383] (an integer)      lo = (double)low * N      hi = (double)high * N      c_b = the count below bin b
 *      w_b = max(0, min(c_b + hist[b], hi) - max(c_b, lo))        min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b
 *      W = the sum of w_b, M = the sum of (w_b * (b + 0.5)), both in ascending b        level = M / W / 8 - 24
 *      auto = min(max(key_stops - level, min_stops), max_stops)
 *    The adaptation state is a double `adapted` and a flag `primed`.  Not primed: adapted = auto, and the state becomes primed.  Primed:
 *    adapted = adapted + rate * (auto - adapted).  A frame with N == 0 changes nothing: it uses adapted if primed, else 0 stops.  Manual
 *    mode: adapted = stops, and the state is neither read nor written.  The gain:
 *      q = nearbyint(adapted * 16), ties to even        gain = ldexpf(T[q mod 16], floor(q / 16))        T[i] = (float)exp2(i / 16.0)
 *    with q mod 16 in 0 ... 15.  T is GR_TONE_SIXTEENTHS below, 16 hex float literals that host and kernel share; neither evaluates exp2.
 *    So the exposure moves in sixteenths of a stop and is reproducible to the bit.
 * 3. The curve.  Per r, g and b, every step a single fp32 IEEE operation in the order written, NEVER fused, the division IEEE's:
 *      v = gain * c        x = v > 0 ? (v < 16777216.f ? v : 16777216.f) : 0.f        (NaN, negatives and -0 become +0; infinity 2^24)
 *      GR_TONE_LINEAR     y = x
 *      GR_TONE_REINHARD   a = x * iw2;  n = x * (1 + a);  y = n / (1 + x)        iw2 = (float)(1.0 / ((double)white * white)), on the host
 *      GR_TONE_FILMIC     n = x * ((2.51f * x) + 0.03f);  d = (x * ((2.43f * x) + 0.59f)) + 0.14f;  y = n / d;  y = y < 1 ? y : 1
 *    Alpha passes bit for bit.  The output is still linear-light float4: the sinks' own transfer curves stay as they are. */
#define GR_TONE_MANUAL 0
#define GR_TONE_AUTO 1
#define GR_TONE_LINEAR 0
#define GR_TONE_REINHARD 1
#define GR_TONE_FILMIC 2
#define GR_METER_BINS 384
#define GR_METER_COUNTERS 385   /* [384]: black */
#define GR_TONE_SIXTEENTHS {0x1.000000p+0f, 0x1.0b5586p+0f, 0x1.172b84p+0f, 0x1.2387a6p+0f, 0x1.306fe0p+0f, 0x1.3dea64p+0f, 0x1.4bfdaep+0f, 0x1.5ab07ep+0f, \
                            0x1.6a09e6p+0f, 0x1.7a1148p+0f, 0x1.8ace54p+0f, 0x1.9c4918p+0f, 0x1.ae89fap+0f, 0x1.c199bep+0f, 0x1.d5818ep+0f, 0x1.ea4afap+0f}
struct gr_tone {
    int mode;               /* GR_TONE_MANUAL, GR_TONE_AUTO */
    float stops;            /* manual: -32 ... 32 */
    float key_stops;        /* auto: where the metered level goes, -32 ... 32; default (float)log2(0.18) = -0x1.3ca9c6p+1f */
    float low, high;        /* the metered window, fractions of the non-black pixels: 0 <= low < high <= 1; default 0.5, 0.98 */
    float min_stops, max_stops;   /* -32 <= min_stops <= max_stops <= 32; default -32, 32 */
    float rate;             /* (0, 1]; default 1: no memory */
    int curve;              /* GR_TONE_LINEAR, _REINHARD, _FILMIC; default linear */
    float white;            /* Reinhard's white point: finite, (0, 4096]; default 4 */
};
/* what the solve keeps in DEVICE memory from frame to frame (adapted, primed: the 16 bytes of adaptation state) and what it writes for
 * the curve and for gr_render_state_exposure (q, gain); 24 bytes, aligned to 8.  All zero: not primed. */
struct gr_tone_state {
    double adapted;
    int primed;
    int q;
    float gain;
    int reserved;
};
/* Every function below refuses, before any device call and before it writes anything, with GR_ERROR_INVALID_ARGUMENT and a message that
 * names the function and the field: a NULL; a size below 1; more than 2^31 - 1 pixels; a field of *tone out of its range or not finite -
 * all fields are checked in both modes -, low >= high, min_stops > max_stops, an unknown mode or curve; a gain that is not finite or is
 * negative; the launchers also a NULL program and a device pointer that is not aligned (frames to 16 bytes, the state to 8, counters to 4). */
int gr_tone_default(struct gr_tone* out);   /* manual, 0 stops, and the defaults above */
/* The host statements of 1, 2 and 3, compiled so that nothing is contracted.  src, dst: float[4 * width * height]; hist: 385 counters,
 * written (not added to).  gr_meter_solve_host reads and writes *adapted and *primed as 2 says (manual mode: neither), and writes *gain
 * and *q.  gr_tone_frame takes the gain as a value; src == dst is allowed. */
int gr_meter_histogram_frame(const float* src, int width, int height, unsigned* hist);
int gr_meter_solve_host(const unsigned* hist, const struct gr_tone* tone, double* adapted, int* primed, float* gain, int* q);
int gr_tone_frame(const float* src, int width, int height, const struct gr_tone* tone, float gain, float* dst);
/* The same on the device (kernels/tone.hip, set-up module: IEEE arithmetic, no contraction), asynchronous on `stream`; *tone is HOST
 * memory and travels in the argument block.  gr_meter_frame zeroes device_hist (385 words) on the stream and launches gr_meter_histogram
 * - a one-dimensional grid of at most 1024 workgroups that walk tiles of 1024 pixels.  gr_meter_solve_device (auto mode only: a manual
 * gain is the host's) launches gr_meter_solve, one wave, which reads device_hist and *device_state and writes *device_state.
 * gr_apply_tone launches gr_tone_apply: the gain is the float at device_gain (&state->gain), or host_gain where that is NULL; the mode
 * of *tone is not looked at; src == dst is allowed, any other overlap is not. */
int gr_meter_frame(gr_program* p, void* stream, const void* src, int width, int height, void* device_hist);
int gr_meter_solve_device(gr_program* p, void* stream, const void* device_hist, const struct gr_tone* tone, void* device_state);
int gr_apply_tone(gr_program* p, void* stream, const void* src, void* dst, int width, int height, const struct gr_tone* tone,
                  const void* device_gain_or_null, float host_gain);
/* The tone of a state's frames.  NULL (the default): every entry point is as it was, launch for launch.  With a tone set the order of a
 * delivery (gr_render_frame and its three encoded kin, gr_deliver_accumulated) is: resolve, glare if one is set, meter and solve in auto
 * mode, tone, sink at factor 1 - all four formats; a float4 delivery is toned straight into `out`, and a factor-1 box state no longer
 * renders straight into `out`, as with a glare.  What is delivered is gr_tone_frame of the frame the state delivers without a tone,
 * with the gain of gr_meter_solve_host of gr_meter_histogram_frame of that frame.  The traced frame and the accumulation stay as they
 * are: gr_render_subframe accumulates untoned and the delivery meters and tones the accumulation once, after its glare.  All launches
 * lie between the events of gr_render_state_resolve_ms, and no call on the frame path synchronises.  The adaptation state lives in the
 * state's device memory, advances once per delivered frame, is reset by gr_render_state_set_tone (on the stream of the next delivery)
 * and is freed with the state.  gr_render_state_exposure synchronises `stream` and downloads the last delivered frame's values: *stops =
 * q / 16 and *gain (before any delivery: 0 and 1); it serves tests and the CLI's printout.  Whole frames only: strip_count > 1 and
 * gr_render_frame_tiled / _tiled_as are refused before anything is rendered, because a histogram of a strip is not the frame's.
 * gr_render_state_tone: *is_set = 1 and the tone in *out, or 0 and *out untouched. */
int gr_render_state_set_tone(gr_render_state* s, const struct gr_tone* tone_or_null);
int gr_render_state_tone(const gr_render_state* s, struct gr_tone* out, int* is_set);
int gr_render_state_exposure(gr_render_state* s, void* stream, float* stops, float* gain);

/* ---- PNG frames -----------------------------------------------------------------------------------------------------------------------
 * A PNG encoder behind an RGBA8 frame that is already in device memory (gr_render_frame_rgba8, gr_deliver_accumulated(GR_FRAME_RGBA8),
 * participant 0's frame of gr_render_frame_tiled_as): filtering, histogram and bit-packing run on the device (kernels/png.hip, set-up
 * module), only the compressed bytes come back.  A sink, not a fifth GR_FRAME_* format: a compressed size is no function of width and height.
 * gr_write_png_rgba8 (geodesic_hip.h) stays as it is.  (Declared here and not in geodesic_hip.h only because the contract header keeps to 80
 * names and 350 lines; all of this is public.)
 *
 * The stream is fixed, so that host and device write the same bytes:
 *   container   8 bit, colour type 6 (RGBA), no interlace; one IDAT where the zlib stream is below 2^31 - 1 bytes, otherwise several
 *   row filters row 0 is filter type 1 (Sub, bpp = 4), every other row type 2 (Up): a filtered byte depends on one other byte of the frame
 *   zlib        78 01, one deflate segment per row, then 03 00 (a final empty fixed block) and the big-endian Adler-32
 *   segment     one non-final dynamic-Huffman block - the frame's block header (the same bits for every row), the codes of the filter byte
 *               and the row's 4 * width filtered bytes, end-of-block - then an empty stored block: three 0 bits, 0 bits up to a byte
 *               boundary, 00 00 FF FF.  Segments therefore meet at byte boundaries and concatenate byte-wise.  Literals only, no matches.
 *   table       one literal/length code per frame, from the frame's histogram of filtered bytes (filter bytes included) plus one
 *               end-of-block a row: Huffman's lengths (ties: the node made first, leaves in symbol order), lengths above 15 moved to 15
 *               and the code made complete again (one leaf of the deepest level dropped a level at a time), the shortest lengths dealt to
 *               the commonest symbols (ties: the lower symbol); canonical codes.  A histogram with fewer than two symbols gets the
 *               lowest-numbered others as leaves that never occur (two leaves of one bit).  HLIT = 257, HDIST = 1 with the one distance
 *               length 0 (RFC 1951 3.2.7: no distance codes, literals only); the 258 lengths run-length coded (16, 17, 18) and coded
 *               with lengths limited to 7 in the same way.
 *   checksums   the Adler-32 is joined from the rows' (adler32_combine), the chunk CRCs are taken on the host over the finished bytes.
 *
 * A second stream kind, opt-in, beside that one (GR_PNG_STREAM_LITERALS, the default of everything that takes no kind): GR_PNG_STREAM_RUNS
 * adds the one LZ77 match a rendered frame is full of and a wave finds without a search - "this pixel's four filtered bytes are the
 * previous pixel's".  Container, row filters, zlib framing, one dynamic block a row with the frame's header repeated, the empty stored
 * block and the checksums are the ones above; what differs:
 *   repeats     q[x] is the four filtered bytes of pixel x of a row as one 32-bit word; repeat[x] = x >= 1 and q[x] == q[x - 1].  Pixel 0
 *               never repeats: nothing refers across the filter byte or into the row before.
 *   tokens      pixels are taken in groups of 64 by position (x / 64).  Inside a group every maximal run of consecutive pixels with repeat
 *               set is one match of distance 4 and length 4 * run, 4 ... 256 bytes (the minimum run is 1 pixel, a constant of the stream);
 *               the first pixel of a group may repeat the last pixel of the group before, and a run ends with its group whatever follows:
 *               no match crosses a group boundary, so a run of repeats over a boundary is two matches.  Every other pixel is four
 *               literals.  In the block: the filter byte's literal, the tokens in pixel order - a match is its length symbol's code, the
 *               symbol's extra bits, and the one bit 0 of the distance code -, end-of-block.
 *   alphabets   literal/length symbols 0 ... 284, HLIT = 285: lengths 4 ... 256 by RFC 1951 3.2.5 (symbol 258 = 4 ... 264 = 10 without extra
 *               bits, then four symbols each with 1 ... 5 extra bits; 256 is symbol 284 with extra 29).  HDIST = 4 with the distance lengths
 *               0 0 0 1: distance code 3 is distance 4 and has no extra bits; the single one-bit distance code is what RFC 1951 3.2.7
 *               allows and zlib accepts.  These four lengths are always sent, also for a frame without a match.
 *   table       one per frame from the frame's histogram over literals (filter bytes included), one end-of-block a row and the matches'
 *               length symbols, by the rules above (tie-breaks, the limit of 15, Kraft's sum restored); the 285 + 4 lengths run-length
 *               coded as one sequence and coded with lengths limited to 7.
 *   bit count   of a row's block, from the row's histogram alone: the header, the filter byte's and end-of-block's codes, and the sum over
 *               the symbols of count x (code length + the symbol's extra bits), plus one bit for every match.
 *   bound       gr_png_encode_bound holds for both kinds.  It counts 15 bits for every filtered byte and 4 096 bits of header a row.  A
 *               match stands for 4 bytes or more and costs 15 + 5 + 1 bits at most, less than the 60 counted for its bytes.  The header
 *               is 17 bits of counts, 19 x 3 bits and the code-length symbols of 289 lengths: 7 bits at most for a symbol that stands for
 *               one length, 7 + 7 for one with extra bits, which stands for three lengths or more - 7 bits a length at most,
 *               74 + 289 x 7 = 2 097 bits. */
enum { GR_PNG_STREAM_LITERALS = 0, GR_PNG_STREAM_RUNS = 1 };
typedef struct gr_png_encoder gr_png_encoder;
/* What a file of this size never exceeds, of either stream kind (every literal 15 bits, a block header of 512 bytes a row): the capacity both
 * encoders ask for. */
int gr_png_encode_bound(int width, int height, size_t* bytes);
/* The host encoder: the definition of the bytes above.  rgba8: [height][width][4] bytes, R, G, B, A; *out_bytes: the file's size.  Both
 * encoders refuse, before anything is written or any device call is made, with a message that names the entry point: a NULL; a size below 1; a
 * frame pointer not aligned to 4 bytes; a frame of more than 2^31 - 1 raw bytes (4 a pixel); a capacity below gr_png_encode_bound
 * (GR_ERROR_BUFFER_TOO_SMALL; everything else GR_ERROR_INVALID_ARGUMENT).  out_file needs no alignment. */
int gr_png_encode_rgba8_host(const unsigned char* rgba8, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* The host encoder of a stream kind, the definition of that kind's bytes: GR_PNG_STREAM_LITERALS gives gr_png_encode_rgba8_host's file.
 * Refuses what that one refuses and an unknown kind (GR_ERROR_INVALID_ARGUMENT). */
int gr_png_encode_rgba8_host_as(const unsigned char* rgba8, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes, int stream_kind);
/* The table builder on its own: histogram[257] (literals, then end-of-block; a 0 there is taken as 1) to lengths[257], codes[257] (bit-reversed:
 * written from bit 0 up), the block header as bits from bit 0 of header_words[0] up (128 words) and its bit count. */
int gr_png_build_table(const unsigned long long* histogram, unsigned char* lengths, unsigned short* codes, unsigned int* header_words, int* header_bits);
/* ... of a stream kind: GR_PNG_STREAM_LITERALS is gr_png_build_table; GR_PNG_STREAM_RUNS takes histogram[285] (literals, end-of-block, the
 * length symbols 257 ... 284) and gives lengths[285], codes[285] and the header with HLIT = 285 and the four distance lengths 0 0 0 1. */
int gr_png_build_table_as(const unsigned long long* histogram, int stream_kind, unsigned char* lengths, unsigned short* codes, unsigned int* header_words, int* header_bits);
/* A device encoder for frames of one size on the program's device: owns the device scratch (the rows' histograms and Adler sums, the table,
 * the rows' offsets, the stream) and a pinned staging buffer of gr_png_encode_bound bytes.  The program is borrowed and must outlive it. */
int gr_png_encoder_create(gr_program* p, int width, int height, gr_png_encoder** out);
/* ... for a stream kind (gr_png_encoder_create: GR_PNG_STREAM_LITERALS); an unknown kind is refused before any device call.  Everything
 * below serves whichever kind the encoder was made with: gr_png_encode_rgba8 then launches gr_png_histogram_runs and gr_png_pack_runs, its
 * file is gr_png_encode_rgba8_host_as's of that kind byte for byte, and its first download is 1 140 bytes + 1 148 bytes a row (285 bins a
 * row and the two Adler sums). */
int gr_png_encoder_create_as(gr_program* p, int width, int height, int stream_kind, gr_png_encoder** out);
void gr_png_encoder_destroy(gr_png_encoder* e);
/* Encodes device_rgba8 (device memory, width x height pixels) into out_file (host memory): enqueues on `stream` - gr_png_histogram, one
 * download of the rows' histograms and Adler sums (1 KiB + 1 032 bytes a row), the table and the rows' offsets built on the host and
 * uploaded, the stream zeroed, gr_png_pack, the download of the compressed bytes - and returns after the file's bytes are in out_file: it
 * SYNCHRONISES that stream, twice.  The file is gr_png_encode_rgba8_host's of the same pixels, byte for byte. */
int gr_png_encode_rgba8(gr_png_encoder* e, void* stream, const void* device_rgba8, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* Measurement and tests.  _time_launches: with on != 0 every later encode brackets its two launches with events; _launch_ms: the last such
 * encode's gr_png_histogram and gr_png_pack in milliseconds.  _scratch_intact: *intact = 1 when every word of the stream scratch outside the
 * longest stream this encoder has made - the guard words in front of it and everything behind it - still holds what gr_png_encoder_create
 * wrote there. */
int gr_png_encoder_time_launches(gr_png_encoder* e, int on);
int gr_png_encoder_launch_ms(gr_png_encoder* e, float ms[2]);
int gr_png_encoder_scratch_intact(gr_png_encoder* e, int* intact);

/* ---- EXR frames -----------------------------------------------------------------------------------------------------------------------
 * An OpenEXR encoder behind a float4 frame that is already in device memory (gr_render_frame, gr_deliver_accumulated(GR_FRAME_F32)): the one
 * sink that keeps what the renderer computed - scene-linear half floats, values far above 1 included - at 6 bytes a pixel or less.  Half
 * conversion, plane separation, byte split, predictor, histogram and bit-packing run on the device (kernels/exr.hip, set-up module), only
 * the file's chunks come back.  A sink like PNG, not a fifth GR_FRAME_* format.  (Declared here and not in geodesic_hip.h only because the
 * contract header keeps to 80 names and 350 lines; all of this is public.)
 *
 * The file is fixed, so that host and device write the same bytes:
 *   container   76 2F 31 01, version 02 00 00 00: one part, scan lines, short names.  The attributes, in this order: channels (chlist: B, G,
 *               R, each HALF, pLinear 0, sampling 1 x 1), compression = 2 (ZIPS: zlib, one scan line a chunk), dataWindow and displayWindow
 *               = (0, 0, width - 1, height - 1), lineOrder = 0, pixelAspectRatio = 1, screenWindowCenter = (0, 0), screenWindowWidth = 1 -
 *               313 bytes with the closing 0.  No alpha (the frame's carries nothing), no chromaticities (the default, Rec. 709, is right).
 *               Then the offset table, height x uint64 from the file's start, then the chunks in increasing y: int32 y, int32 size, data.
 *   halfs       of a pixel's r, g, b: a NaN is +0; everything else is clamped to [-65504, 65504] - no infinity is written - and rounded to
 *               nearest even with half subnormals kept (2^-25 is a tie and goes to 0).  Stated in integer arithmetic on the float's bits, the
 *               same lines on host and device: no compiler's _Float16 and no build flag has a say.
 *   raw row     three planes, B then G then R, each `width` little-endian halfs: 6 * width bytes.
 *   zip order   of a raw row: its even-indexed bytes followed by its odd-indexed ones - the low bytes of B, G, R over all x, then the high
 *               bytes - and then t[i] = t[i] - t[i - 1] + 128 mod 256 for i >= 1 over the reordered values.  The predictor does not stop at a
 *               plane's end or between low and high bytes.
 *   zlib        a row's stream: 78 01, ONE dynamic-Huffman block with BFINAL = 1 - the frame's block header, the codes of the row's 6 * width
 *               predicted bytes, end-of-block; literals only -, 0 bits up to the byte boundary, the big-endian Adler-32 of the predicted bytes.
 *   table       one per frame, "PNG frames"' construction as it stands (gr_png_build_table; only BFINAL differs in the header): from the
 *               histogram of ALL rows' predicted bytes plus one end-of-block a row.  Rows that end up stored raw are counted too: the table is
 *               a function of the pixels alone.
 *   raw rows    the format's own fallback: a reader tells a raw chunk from a compressed one by its size.  With c the bytes of a row's zlib
 *               stream, the chunk holds the stream when c < 6 * width and otherwise the 6 * width raw bytes, neither reordered nor
 *               predicted.  c follows from the row's histogram before a bit is packed (width 1: always raw).
 *   bound       gr_exr_encode_bound = 313 + 8 * height + height * (8 + 6 * width): every row raw.  Exact, not an estimate.
 * The launches (one workgroup of 256 lanes a row in both): gr_exr_histogram - a pixel a lane: the six predicted bytes of its b, g, r counted
 * in LDS, the row's histogram stored and added to the frame's, the Adler-32's sums reduced mod 65521 - and gr_exr_pack, which writes every
 * chunk with its header at the byte offset the host gives it: a compressed row as bits in stream order, four consecutive bytes of the
 * reordered row a lane, through the PNG encoder's bit-packer; a raw row as 32-bit words of halfs. */
typedef struct gr_exr_encoder gr_exr_encoder;
/* What no file of this size exceeds - the size of the file whose every row is stored raw: the capacity both encoders ask for. */
int gr_exr_encode_bound(int width, int height, size_t* bytes);
/* The half conversion on its own: out[i] = the bits of the half of values[i] as defined above. */
int gr_exr_half_bits(const float* values, size_t count, unsigned short* out);
/* The host encoder: the definition of the bytes above.  frame_rgba_f32: [height][width][4] floats, r, g, b, a; *out_bytes: the file's size.
 * Both encoders refuse, before anything is written or any device call is made, with a message that names the entry point and the field: a
 * NULL; a size below 1; a row of more than 2^31 - 1 raw bytes (6 a pixel); a capacity below gr_exr_encode_bound
 * (GR_ERROR_BUFFER_TOO_SMALL; everything else GR_ERROR_INVALID_ARGUMENT); a frame pointer not aligned to 16 bytes.  out_file needs no
 * alignment. */
int gr_exr_encode_f32_host(const float* frame_rgba_f32, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* gr_exr_encode_f32_host's file written to `path` (gr_write_frame_png's counterpart; the frame needs no alignment here). */
int gr_write_frame_exr(const char* path, const float* frame_rgba_f32, int width, int height);
/* A device encoder for frames of one size on the program's device: owns the device scratch (the rows' histograms and Adler sums, the table,
 * the chunks' offsets, the chunk area) and a pinned staging buffer.  The program is borrowed and must outlive it. */
int gr_exr_encoder_create(gr_program* p, int width, int height, gr_exr_encoder** out);
void gr_exr_encoder_destroy(gr_exr_encoder* e);
/* Encodes device_rgba_f32 (device memory, width x height float4 pixels, 16-byte aligned) into out_file (host memory): enqueues on `stream` -
 * gr_exr_histogram, one download of the rows' histograms and Adler sums (1 KiB + 1 032 bytes a row), the table, the raw-or-compressed
 * decisions and the chunks' offsets made on the host and uploaded, the chunk area zeroed, gr_exr_pack, the download of the chunks - and
 * returns after the file's bytes are in out_file: it SYNCHRONISES that stream, twice.  Header and offset table are written by the host.
 * The file is gr_exr_encode_f32_host's of the same pixels, byte for byte. */
int gr_exr_encode_f32(gr_exr_encoder* e, void* stream, const void* device_rgba_f32, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* Measurement and tests, as the PNG encoder's: _launch_ms gives the last timed encode's gr_exr_histogram and gr_exr_pack in milliseconds;
 * _scratch_intact: *intact = 1 when every word of the chunk scratch outside the longest chunk area this encoder has made - the guard words in
 * front of it and everything behind it - still holds what gr_exr_encoder_create wrote there. */
int gr_exr_encoder_time_launches(gr_exr_encoder* e, int on);
int gr_exr_encoder_launch_ms(gr_exr_encoder* e, float ms[2]);
int gr_exr_encoder_scratch_intact(gr_exr_encoder* e, int* intact);

/* ---- JPEG frames ----------------------------------------------------------------------------------------------------------------------
 * A baseline JPEG encoder behind an RGBA8 frame that is already in device memory - the three sources the PNG encoder takes - and a
 * Motion-JPEG AVI writer for a sequence of such files: colour conversion, DCT, quantiser, Huffman coding and byte stuffing run on the device
 * (kernels/jpeg.hip, set-up module), only the file's bytes come back.  A sink like PNG, not a fifth GR_FRAME_* format.  (Declared here and not
 * in geodesic_hip.h only because the contract header keeps to 80 names and 350 lines; all of this is public.)
 *
 * The stream is fixed, so that host and device write the same bytes:
 *   container   JFIF: SOI, APP0 "JFIF" 1.01 (density 1:1 without units, no thumbnail), DQT luminance, DQT chrominance, SOF0, DHT DC and AC
 *               luminance, DHT DC and AC chrominance, DRI, SOS, the entropy-coded data, EOI - 629 bytes in front of the data.  SOF0: baseline,
 *               8 bit, components 1, 2, 3 sampled 2x2, 1x1, 1x1: an MCU is 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr.  Width and height
 *               1 ... 65 535.  Alpha is ignored.
 *   colour      JFIF's full-range BT.601 Y'CbCr of the 8-bit sRGB codes as they stand - NOT the limited-range BT.709 of gr_present_yuv420:
 *               a JFIF decoder assumes 601 full range and would show anything else with wrong colours.  Integers:
 *                 Y' = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *                 Cb = ((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128       Cr = ((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128
 *               (arithmetic shifts: rounded to nearest, halves up), clamped to 0 ... 255.  CHROMA: the mean of the 2 x 2 pixels' R, of their
 *               G and of their B, each (sum + 2) >> 2, converted once.  A pixel past the right or bottom edge is the last of its row or column.
 *   DCT         of sample - 128, separable, with K[u][x] = round(2^14 c[u][x]), c the orthonormal DCT-II matrix (c[0][x] = 1 / (2 sqrt 2),
 *               c[u][x] = cos((2x + 1) u pi / 16) / 2; the eight magnitudes 5793 8035 7568 6811 5793 4551 3135 1598):
 *                 rows     t[y][u] = (sum over x of K[u][x] s[y][x] + 128) >> 8             6 fraction bits
 *                 columns  F[v][u] = (sum over y of K[v][y] t[y][u] + 32768) >> 16          4 fraction bits: F is 16 x the coefficient
 *               Every sum fits 32 bits (|t| <= 23 175, sum over y of |K| = 46 344: below 1.08 x 10^9) and every product's operands 24.
 *               ERROR BOUND of F / 16 against the exact DCT: 0.19.  With e = 0.00019 >= the largest row sum of |K / 2^14 - c| and A = 2 sqrt 2
 *               = the largest row sum of |c|: a row value is off by at most e1 = 128 e + 2^-7 < 0.0317, a coefficient by at most
 *               A e1 + e (128 A + e1) + 2^-5 < 0.0896 + 0.0689 + 0.0313 = 0.19 - below 0.5, half the smallest quantiser step.
 *   quantiser   the Annex K.1 tables scaled by the quality q = 1 ... 100: s = 5000 / q below 50, else 200 - 2 q; step = (table s + 50) / 100
 *               clamped to 1 ... 255 (integer divisions).  Quantised = sign(F) ((|F| + 8 step) / (16 step)): rounded half away from zero.  An AC
 *               value stays within +-1 020.2, the DC within -1 024 ... 1 016: sizes 10 and 11 are never exceeded.  Zig-zag order.
 *   entropy     the four Annex K.3 Huffman tables, as DHT holds them.  Tables optimised per frame are OUT OF SCOPE: they would cost a pass over
 *               the frame and a round trip through the host, for some 5 to 10 % of the file.  DC: the difference to the component's previous
 *               block, 0 at the start of a restart interval; AC: run/size with ZRL (F0) and EOB (00).
 *   restarts    DRI = the MCUs of one MCU row.  Every MCU row is a segment of its own: its bits, 1-bits up to a byte boundary, FF 00 for every
 *               FF byte, then RSTm with m = row mod 8 - EOI behind the last row.  Rows are therefore coded independently.
 *   AVI         plain AVI 1.0: RIFF 'AVI ', LIST 'hdrl' with 'avih' and one LIST 'strl' of 'strh' ('vids' / 'MJPG', dwScale = fps_den, dwRate =
 *               fps_num) and 'strf' (BITMAPINFOHEADER, 24 bit, 'MJPG'); LIST 'movi' with one '00dc' chunk a frame, padded to even length;
 *               'idx1' with one key-frame entry a frame, offsets from the 'movi' tag.  Sizes and counts are patched at close.  OpenDML (files
 *               of 2 GiB and more) is out of scope. */
typedef struct gr_jpeg_encoder gr_jpeg_encoder;
typedef struct gr_avi gr_avi;
/* What no file of this size exceeds - the capacity both encoders ask for: 629 bytes of headers and, per MCU row, twice (every byte an FF, stuffed)
 * the row's largest segment - ceil(MCUs x 6 blocks x 1 658 bits / 8) bytes, a block being at most a DC code of 9 bits with 11 value bits and 63
 * AC codes of 16 bits with 10 value bits - and 2 bytes of marker.  Refused: a NULL, a width or height outside 1 ... 65 535. */
int gr_jpeg_encode_bound(int width, int height, size_t* bytes);
/* The quantiser's steps at a quality, in natural (row-major) order.  Refused: a NULL, a quality outside 1 ... 100. */
int gr_jpeg_quant_tables(int quality, unsigned char luma[64], unsigned char chroma[64]);
/* The host encoder: the definition of the bytes above.  rgba8: [height][width][4] bytes, R, G, B, A; *out_bytes: the file's size.  Both
 * encoders refuse, before anything is written or any device call is made, with a message that names the entry point: a NULL; a width or height
 * outside 1 ... 65 535; a quality outside 1 ... 100; a frame pointer not aligned to 4 bytes; a capacity below gr_jpeg_encode_bound
 * (GR_ERROR_BUFFER_TOO_SMALL; everything else GR_ERROR_INVALID_ARGUMENT).  out_file needs no alignment. */
int gr_jpeg_encode_rgba8_host(const unsigned char* rgba8, int width, int height, int quality, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* The quantised coefficients alone: per MCU in scan order (rows of MCUs, left to right) six blocks of 64 values in zig-zag order;
 * out holds ceil(width / 16) x ceil(height / 16) x 384 values. */
int gr_jpeg_blocks_host(const unsigned char* rgba8, int width, int height, int quality, short* out);
/* The DCT alone (tests hold its error bound to it): samples[64] in natural order, each -128 ... 127 (anything else is refused), to F as
 * defined above - 16 x the coefficient - in natural order. */
int gr_jpeg_fdct_host(const short* samples, int* coefficients_x16);
/* A device encoder for frames of one size and quality on the program's device: owns the device scratch (3 bytes a pixel of coefficients, the
 * MCU rows' segments, the file; the headers are made here, by the host encoder's own function, and uploaded once) and a pinned staging buffer
 * of gr_jpeg_encode_bound bytes.  The program is borrowed and must outlive it. */
int gr_jpeg_encoder_create(gr_program* p, int width, int height, int quality, gr_jpeg_encoder** out);
void gr_jpeg_encoder_destroy(gr_jpeg_encoder* e);
/* Encodes device_rgba8 (device memory, width x height pixels) into out_file (host memory): enqueues on `stream` gr_jpeg_blocks, gr_jpeg_pack and
 * gr_jpeg_gather with nothing between them, downloads the file's size and then exactly that many bytes, and returns after they are in
 * out_file: it SYNCHRONISES that stream, twice.  The file is gr_jpeg_encode_rgba8_host's of the same pixels, byte for byte. */
int gr_jpeg_encode_rgba8(gr_jpeg_encoder* e, void* stream, const void* device_rgba8, unsigned char* out_file, size_t capacity, size_t* out_bytes);
/* Measurement and tests.  _time_launches: with on != 0 every later encode brackets its three launches with events; _launch_ms: the last such
 * encode's gr_jpeg_blocks, gr_jpeg_pack and gr_jpeg_gather in milliseconds.  _scratch_intact: *intact = 1 when the guard words around each
 * region of the scratch and every word of the file region behind the longest file this encoder has made still hold what
 * gr_jpeg_encoder_create wrote there. */
int gr_jpeg_encoder_time_launches(gr_jpeg_encoder* e, int on);
int gr_jpeg_encoder_launch_ms(gr_jpeg_encoder* e, float ms[3]);
int gr_jpeg_encoder_scratch_intact(gr_jpeg_encoder* e, int* intact);
/* The Motion-JPEG writer, shaped like gr_y4m_*: _open writes the headers (refused: a NULL, a size outside 1 ... 65 535, a rate part below 1, a
 * path that cannot be written), _write_frame appends one finished JPEG file of `bytes` bytes as a chunk, _close writes the index, patches the
 * sizes and counts and frees the handle.  A frame with which the finished file would pass 2^31 - 1 bytes is refused with a message that says
 * so, nothing of it is written, and the file still closes valid.  After a short write the handle only waits for gr_avi_close, which then
 * reports the file incomplete. */
int gr_avi_open(const char* path, int width, int height, int fps_num, int fps_den, gr_avi** out);
int gr_avi_write_frame(gr_avi* a, const unsigned char* jpeg, size_t bytes);
int gr_avi_close(gr_avi* a);
/* For tests: a lower limit than 2^31 - 1 for the finished file of this handle (a limit above that is refused). */
int gr_avi_set_size_limit(gr_avi* a, unsigned long long bytes);

/* ---- fused MI355X path (no reference counterpart) ------------------------------------------- */

/* Prepass termination flags from one fused trace at prepass resolution (replaces the sequence
 * clear_termination_buffer / init_rays_generic / do_generic_rays / calculate_singularities,
 * main.cpp:2387-2436). */
int gr_prepass_fused(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat,
                     void* termination_buffer, int prepass_width, int prepass_height,
                     const void* e0, const void* e1, const void* e2, const void* e3,
                     const void* cfg, const void* dfg);
/* the same for a device that owns only the row blocks strip_rank, strip_rank + strip_count, ... of an image of
 * image_height rows (see gr_trace_fused): cells none of its rows can look at are not traced and keep their old value.
 * cell_attempts (unsigned[prepass_width * prepass_height], may be NULL): the step attempts each cell's ray took, the cost
 * estimate gr_order_tiles works from.  row_margin: how many pixel rows beyond its blocks and their halo rows the device also
 * traces from (0; adaptive sampling on a split frame: 2) */
int gr_prepass_fused_strips(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat,
                            void* termination_buffer, int prepass_width, int prepass_height,
                            const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg, const void* dfg,
                            int image_height, int block_rows, int strip_rank, int strip_count, void* cell_attempts, int row_margin);

/* gr_cart_to_generic + gr_init_basis_vectors + gr_prepass_fused_strips in one launch: the camera's metric coordinates and tetrad
 * are computed from the Cartesian camera inside the launch (and stored to position_generic_out / e*_out for gr_trace_fused), then
 * the prepass cells are traced.  prepass_width * prepass_height may be 0: camera set-up only.  Removes two single-lane launches
 * from every frame's chain. */
int gr_camera_prepass(gr_program* p, void* stream, const void* position_cart, float flip, const float basis_speed[3],
                      void* position_generic_out, void* e0_out, void* e1_out, void* e2_out, void* e3_out, const void* camera_quat,
                      void* termination_buffer, int prepass_width, int prepass_height, const void* cfg, const void* dfg,
                      int image_height, int block_rows, int strip_rank, int strip_count, void* cell_attempts, int row_margin);

/* The order in which a persistent gr_trace_fused launch hands out its tiles: longest first, as estimated from what the prepass
 * rays around each tile cost (cell_attempts of gr_prepass_fused_strips / gr_camera_prepass), tiles on the shadow's edge before
 * everything, tiles no pixel of which needs a ray last (gr_trace_fused_launch then writes their records without looking anything up).  A launch lasts as long as its slowest wave, and a long tile drawn late is what
 * makes a wave slow; which wave traces a tile has no influence on the tile's pixels.  tile_order: gr_tile_order_bytes(...) bytes,
 * written by two small launches on `stream`; pass it to gr_trace_fused_ordered with the same image and strip description. */
long long gr_tile_order_bytes(int width, int height, int block_rows, int strip_rank, int strip_count);
int gr_order_tiles(gr_program* p, void* stream, const void* termination_buffer, const void* cell_attempts, int prepass_width,
                   int prepass_height, int width, int height, int block_rows, int strip_rank, int strip_count, void* tile_order);
/* The reference-shaped trace with the fused trace's scheduling (round 5; what gr_render_frame's reference mode launches for ray records in
 * 8x8-tile slot order): persistent waves draw tiles - 64 consecutive records - from a ticket counter, in tile_order's order (unsigned per
 * tile; NULL = slot order), and leave each tile's cost (attempts of its longest ray) in tile_cost (unsigned per tile; NULL = not).  The
 * records are gr_do_generic_rays'.  gr_sort_tiles_by_cost: the tiles dearest first by such costs (largest among a tile and its neighbours);
 * work: (128 + tiles) unsigned words of scratch. */
int gr_do_generic_rays_scheduled(gr_program* p, void* stream, void* rays, const void* ray_count, int tile_count, const void* cfg, const void* dfg,
                                 void* attempt_counter, const void* tile_order, void* tile_cost);
int gr_sort_tiles_by_cost(gr_program* p, void* stream, const void* tile_cost, int tiles_x, int tiles_y, void* tile_order, void* work);

/* The same list from what the tiles cost in an earlier frame of the same size and strip description (tile_history: the tile_cost a
 * gr_trace_fused_launch left): exact where the prepass rays sample - the long rays near the photon orbits are filaments a pixel or
 * two wide - as long as the camera moves little between the two frames (a tile takes the largest cost among itself and its eight
 * neighbours).  Needs no prepass, so it combines with inline_prepass.  Pass the list with tile_order_by_history = 1.
 * shift_x, shift_y: how far the picture has moved since, in tiles of 8 pixels (0, 0 if unknown): a tile takes the costs of the
 * tiles that far back.  gr_render_frame estimates it from where the two cameras see the coordinate origin. */
int gr_order_tiles_by_history(gr_program* p, void* stream, const void* tile_history, int width, int height, int block_rows,
                              int strip_rank, int strip_count, void* tile_order, int shift_x, int shift_y);

/* Counter block of the fused trace launchers (their `attempt_counter`; NULL = count nothing): GR_COUNTER_WORDS uint64 words on
 * the device, zeroed by the caller.  [0] attempts of the pair / compaction kernels, [1] summed wave lifetimes in shader cycles,
 * [2] the same in ticks of the 100 MHz reference clock, [3] waves, [8..255] probe builds only, [256..511] gr_trace_fused's attempts
 * spread over 256 words by workgroup (one same-address atomic per tile would serialise a frame of many short tiles).  The total
 * is [0] + sum [256..511]; gr_render_state_attempts does that for a frame's own block. */
#define GR_COUNTER_WORDS 512

/* init -> integrate -> render-data in one launch; writes only render_data[sy*width+sx] (32 B per pixel).
 * Rows are dealt to devices block-cyclically: global block b (block_rows rows, multiple of 8) belongs to device
 * b % strip_count; each block additionally traces the one row below it (texture-filter halo).  strip_count <= 1
 * traces the whole image.  termination_buffer may be NULL (no prepass). */
int gr_trace_fused(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat,
                   void* render_data, int width, int height, int block_rows, int strip_rank, int strip_count,
                   const void* termination_buffer, int prepass_width, int prepass_height,
                   const void* e0, const void* e1, const void* e2, const void* e3,
                   const void* cfg, const void* dfg, void* attempt_counter);
/* gr_trace_fused with everything that only schedules it or rides along, by name:
 *   tile_order      gr_order_tiles' list (NULL: image order)
 *   waves_per_simd  1..8: at most that many persistent waves per SIMD (0: as many as the kernel's registers allow)
 *   lattice, pending_only   the two launches of adaptive sampling (gr_trace_fused_adaptive), also on a split frame
 *   shading.out     not NULL: the launch also SHADES the pixels whose two filter neighbours lie in the same 8x8 tile - 49 of every
 *                   64 - from the registers their records were built in (the neighbours' sky coordinates come over by
 *                   ds_bpermute) and writes them to shading.out as gr_render would (compact_out as in gr_render_strips);
 *                   gr_render_seams then shades the last column and row of every tile from the records.  Width and height
 *                   must be multiples of 8, and the program must have been built with -DGR_TILE_SHADING appended to its argument
 *                   string (gr_program_has_tile_shading).  The records are written either way. */
typedef struct gr_trace_shading {
    void* out;                       /* float4 per pixel; NULL = no shading in the trace launch */
    const void* background1;
    const void* background2;
    int bg_width, bg_height, bg_levels, max_probes, compact_out;
} gr_trace_shading;
/* Parking (kernels/trace.hip, gr_trace_fused_parking): a tile's wave that has fewer than `lanes` rays left after `trips` trips of the
 * Verlet loop (two attempts each) writes their state to the lot and draws its next tile; parked rays are picked up 64 to a wave by
 * whichever wave draws next.  Scheduling only: the records are those of the unparked launch bit for bit.  lanes = 0 (or a NULL
 * lot): the plain kernel.  records: gr_parking_lot_bytes(slots, groups, &words_bytes) bytes, words: words_bytes; a lot that runs
 * out of room is not an error (the wave goes on with its rays itself; words[4] counts the times). */
typedef struct gr_parking_lot {
    void* records;
    void* words;
    int lanes, trips;
    int slots, groups;   /* capacity: parked rays (<= 2^24), and groups of rays parked together (each parking event is one) */
} gr_parking_lot;
size_t gr_parking_lot_bytes(int slots, int groups, size_t* words_bytes);
/* 1 when the program's argument string (or GR_EXTRA_FLAGS) carried -DGR_PARKING: it has the gr_trace_fused_parking kernel.  A build option,
 * like -DGR_TILE_SHADING: measured on MI355X the kernel does not pay (EXPERIMENTS.md C.2), and every program would carry its compile time. */
int gr_program_has_parking(const gr_program* p);
typedef struct gr_trace_fused_args {
    const void* camera_generic;
    const void* camera_quat;
    void* render_data;
    int width, height, block_rows, strip_rank, strip_count;
    const void* termination_buffer;
    int prepass_width, prepass_height;
    const void *e0, *e1, *e2, *e3, *cfg, *dfg;
    void* attempt_counter;
    const void* tile_order;
    int waves_per_simd;
    gr_trace_shading shading;
    int lattice;        /* 0 or 1: every pixel; 2: the pixels (2x, 2y) only (first launch of adaptive sampling) */
    int pending_only;   /* 1: only the pixels gr_adaptive_refine marked (second launch of adaptive sampling) */
    int inline_prepass; /* 1: the launch traces the prepass grid itself - its cells are the first tickets of the persistent launch, 64
                         * to a wave, and a tile waits for the cells its pixels look at (device-scope flags in termination_buffer,
                         * which must be writable and is reset by the call).  Image order only (no tile_order), lattice 1; a device's
                         * share of a split frame traces the cells its rows look at and leaves the others unknown.  Camera and tetrad must be on the device already (gr_camera_prepass with a 0 x 0
                         * grid).  Records and flags are those of the two-launch sequence.  With tile_order_by_history the tiles
                         * behind the cell waves follow tile_order. */
    void* tile_cost;    /* not NULL: unsigned[number of the device's tiles = (gr_tile_order_bytes - 128) / 8]; the launch leaves what
                         * each tile cost there (the attempts of its longest ray) for gr_order_tiles_by_history.  Every pixel, one ray per lane. */
    int tile_order_by_history;   /* 1: tile_order is gr_order_tiles_by_history's list (its last class is looked up like any tile) */
    void* lattice_rays;          /* lattice = 2: where the launch leaves its rays' end states for gr_adaptive_refine (see there); may be NULL */
    gr_parking_lot parking;      /* lanes > 0: gr_trace_fused_parking (every pixel, one ray per lane, no in-tile shading) */
    int speculative_classes;     /* inline_prepass with tile_order_by_history: the tiles of the list's first n classes (octaves of a tile's
                                  * longest ray in the frame before, 16 384 attempts = class 0) do not wait for the prepass cells their pixels
                                  * look at: they trace every pixel from the start and take the verdicts when their rays have ended - the
                                  * launch's critical path is otherwise the longest cell ray followed by the longest tile, which reads that
                                  * cell.  Records are the same.  0 = library default (5: tiles that had a ray of 1 024 attempts or more), -1 = none */
    void* guessed;               /* lattice = 2 (persistent launch): gr_guessed_bytes of device memory whose first word says how many pixels of
                                  * its list the launch is to trace ahead, beside the lattice - the pixels the frame before traced in its second
                                  * launch and found dear (gr_trace_pending leaves them) - each record into the same buffer for
                                  * gr_apply_guessed; NULL or a count of 0: none */
} gr_trace_fused_args;
int gr_trace_fused_launch(gr_program* p, void* stream, const gr_trace_fused_args* args);
/* waves of gr_trace_fused the program's device holds at once (what a persistent launch fills it with): a frame of many more tiles than
 * that has a short tail whatever the order of its tiles */
long long gr_trace_fused_wave_slots(gr_program* p);
/* the pixels such a launch leaves to shade: same arguments as gr_render_strips (strip_count <= 1: the whole image) */
int gr_render_seams(gr_program* p, void* stream, const void* render_data, void* out_rgba_f32,
                    const void* background1, const void* background2, int bg_width, int bg_height, int bg_levels,
                    int width, int height, int block_rows, int strip_rank, int strip_count, int compact_out,
                    int max_probes, const void* cfg, const void* dfg);

/* Adaptive sampling on the fused path (the reference: init_rays_generic's packing cl.cl:3234-3250 + handle_adaptive_sampling
 * cl.cl:5223-5345 + a second do_generic_rays / calculate_render_data).  gr_trace_fused_adaptive is gr_trace_fused on a whole image
 * with lattice = 2: only the pixels (2x, 2y) are traced; or with pending_only = 1: only the pixels whose record says terminated ==
 * -1 are traced, every other record is left alone.  gr_adaptive_refine decides per 2x2 block from the lattice records (boundary
 * blocks and blocks whose termination flags differ always refine, otherwise the angular error across the block against the
 * per-pixel angle times adaptive_sampling_threshold): a block to refine gets its three other records marked -1, any other block
 * gets them interpolated; pending_count (device int, may be NULL) accumulates 3 per refined block. */
int gr_trace_fused_adaptive(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* render_data,
                            int width, int height, const void* termination_buffer, int prepass_width, int prepass_height,
                            const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg, const void* dfg,
                            void* attempt_counter, int lattice, int pending_only, void* lattice_rays);
int gr_adaptive_refine(gr_program* p, void* stream, void* render_data, void* pending_count, int width, int height, const void* dfg,
                       const void* lattice_rays, const void* cfg);
/* The second launch as a list (what gr_render_frame does): gr_adaptive_refine_list decides and marks as gr_adaptive_refine_strips does
 * and leaves the marked pixels in pending_list (gr_pending_list_bytes), ordered by what their rays are expected to cost - the dearest of
 * the four lattice rays around the block, a quarter of an octave of attempts per class, dearest first; gr_trace_pending traces the list 64
 * entries to a wave (waves_per_simd as in gr_trace_fused_args; 0 = as many as fit).  Every lane of every wave has a ray, the rays of a wave
 * are neighbours of one cost class, and the longest rays of the frame start first.  Records equal those of the pending_only launch to
 * rounding (another kernel around the same device functions).  block_cost (unsigned per 2x2 block, (width / 2) * (height / 2), zeroed by the
 * caller; may be NULL): gr_trace_pending leaves what the dearest ray of each block cost; given to the NEXT frame's gr_adaptive_refine_list
 * as block_cost_before (while the picture has moved little) it orders that list by the blocks' own rays - the lattice rays either side of
 * a filament of long rays say nothing about it. */
size_t gr_pending_list_bytes(int width, int height);
size_t gr_lattice_rays_bytes(int width, int height);
int gr_adaptive_refine_list(gr_program* p, void* stream, void* render_data, void* pending_count, int width, int height, const void* dfg,
                            int block_rows, int strip_rank, int strip_count, const void* lattice_rays, const void* cfg, void* pending_list,
                            const void* block_cost_before);
int gr_trace_pending(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* render_data, int width, int height,
                     const void* e0, const void* e1, const void* e2, const void* e3, const void* cfg, const void* dfg, void* attempt_counter,
                     const void* pending_list, int waves_per_simd, void* block_cost, void* guessed_next);
/* Tracing ahead what the second launch will ask for (round 6).  An adaptively sampled frame is two dependent launches, and where single rays
 * run to the step cap (an extremal hole at 1080p) each lasts as long as its longest ray: 2 x 14 ms.  gr_trace_pending leaves the pixels that
 * cost 4 096 attempts or more in guessed_next (gr_guessed_bytes; its first word zeroed by the caller; NULL: nothing kept, nothing passed
 * over); the next frame's lattice launch traces them beside its tiles (gr_trace_fused_args.guessed), gr_apply_guessed - after
 * gr_adaptive_refine_list, before gr_trace_pending - hands a guessed pixel that IS marked its record, attempts and cost (and keeps it
 * guessed for the frame after), and gr_trace_pending passes over what is no longer marked.  Records are those of a frame that guesses nothing. */
size_t gr_guessed_bytes(void);
int gr_apply_guessed(gr_program* p, void* stream, void* render_data, int width, const void* guessed, void* guessed_next, void* block_cost,
                     void* attempt_counter);
/* lattice_rays: gr_lattice_rays_bytes(width, height) bytes - 3 x float4 per lattice pixel, and behind those one unsigned per lattice
 * pixel: the attempts its ray took (the cost estimate of gr_adaptive_refine_list) - written by the lattice launch (lattice = 2) and
 * read by gr_adaptive_refine: where every lattice ray ended (position, velocity, the quaternion of its rotated frame) - what the
 * reference's decision reads off its ray records through get_intersection_position, also for rays whose render-data record is black
 * (they ended inside r = 1; their texture coordinates are 0, 0; cl.cl:5260-5268).  NULL on both: the decision falls back on the
 * records' texture coordinates, which differs from the reference's around black features.  cfg: the metric's dynamic variables
 * (needed with lattice_rays). */
/* the same on a device's share of a split frame: only the 2x2 pixel blocks whose rows the device shades or reads as a halo row are
 * decided.  The lattice launch before it (gr_trace_fused_launch with lattice = 2 and the strip description) traces the lattice
 * rows those decisions read - two rows of halo either side of a block - and the launch after it (pending_only = 1, same strip
 * description) the marked pixels of the device's rows; the rows equal those of the whole frame sampled adaptively. */
int gr_adaptive_refine_strips(gr_program* p, void* stream, void* render_data, void* pending_count, int width, int height,
                              const void* dfg, int block_rows, int strip_rank, int strip_count, const void* lattice_rays, const void* cfg);

/* gr_trace_fused with two rays per lane: a wave takes two neighbouring 8x8 tiles and every lane integrates one pixel of each,
 * all per-ray arithmetic in packed fp32 (v_pk_fma/mul/add_f32: one instruction, two rays).  Same arguments, same records;
 * each ray's arithmetic is that of gr_trace_fused (results agree to what the compiler contracts differently).  A program has
 * the kernel when its Verlet-loop expressions instantiate on float pairs (no comparison/select forms, moderate size) and it
 * steps without the adaptive controller - there it is 1.3-1.5x faster; with the controller it is slower and only built on
 * request (GR_TRACE_PAIR_BUILD=1).  gr_program_has_trace_pair tells; GR_ERROR_INVALID_ARGUMENT when it is missing. */
int gr_trace_pair(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat,
                  void* render_data, int width, int height, int block_rows, int strip_rank, int strip_count,
                  const void* termination_buffer, int prepass_width, int prepass_height,
                  const void* e0, const void* e1, const void* e2, const void* e3,
                  const void* cfg, const void* dfg, void* attempt_counter);
int gr_program_has_trace_pair(const gr_program* p);   /* 1 / 0 */
/* 1 when the program's argument string (or GR_EXTRA_FLAGS) carried -DGR_TILE_SHADING: its gr_trace_fused can shade (gr_trace_shading) */
int gr_program_has_tile_shading(const gr_program* p);
/* Process-unique identity of a program object (never reused, unlike its address); 0 for NULL. */
unsigned long long gr_program_serial(const gr_program* p);
/* What the program's code object was built from - kernel source, every compile option, hiprtc version, the setting of the pass
 * over the compiled code - as 16 hex digits (the name of its cache file), followed by what came out: "-v<VGPRs>s<scratch bytes>"
 * of gr_trace_fused as loaded (the build-time occupancy rule can go either way for one set of inputs).  Measurements that belong
 * to one build (hardware counters under profiles/) carry it, so that a reader can tell whether they still describe the kernel
 * that runs. */
const char* gr_program_build_key(const gr_program* p);

/* gr_trace_fused with ray compaction (north_star: "wave-level ballots for step-acceptance and ray compaction"): persistent
 * waves hold one ray per lane; whenever fewer than keep_lanes (1..64) of a wave's rays are still integrating, the finished
 * ones are written out and the idle lanes draw new pixels from a device-side counter.  Every ray is integrated exactly as
 * in gr_trace_fused (results agree to rounding); it can only pay when neighbouring rays need very different numbers of
 * steps - not the case for the BASELINE workloads, where 8x8 tiles keep >= 94 % of the lanes busy (EXPERIMENTS.md C.2). */
int gr_trace_compact(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat,
                     void* render_data, int width, int height, int block_rows, int strip_rank, int strip_count,
                     const void* termination_buffer, int prepass_width, int prepass_height,
                     const void* e0, const void* e1, const void* e2, const void* e3,
                     const void* cfg, const void* dfg, void* attempt_counter, int keep_lanes);


/* What tile_history did with this render state's frames so far: how many recorded their tiles' costs, how many of those followed
 * the costs of the frame before, and the shift (in tiles) the last one that did applied.  Any pointer may be NULL. */
int gr_render_state_tile_history(gr_render_state* s, unsigned long long* frames_recorded, unsigned long long* frames_followed,
                                 int last_shift[2]);
/* Do the expressions a program's Verlet loop evaluates (its GEO_ACCEL* / GR_DEVICE_ACCEL* macros and their temporaries) call sin / cos?  1 yes,
 * 0 no, -1 no string.  A program whose accelerations call neither is built with -DGR_ACCEL_WITHOUT_TRIG: its loop has no range-limited
 * polynomial whose NaN it would have to tell from the metric's own (kernels/integrator.hip). */
int gr_argument_string_accelerations_call_trig(const char* argument_string);
/* Is a program built from this string built with -DGR_RADIUS_EXITS_ORDERED (kernels/integrator.hip: a wave whose live rays are all inside the
 * precision radius skips the outer boundary test)?  1 when the string is a substituted program's, its distance function is the polar radius
 * (DISTANCE_FUNC is v2; GR_DISTANCE_OF_GENERIC absent, or it and TO_COORD2 the bare v2) and SINGULAR_TERMINATOR < max_precision_radius < universe_size; 0 otherwise; -1 no string. */
int gr_argument_string_radius_exits_ordered(const char* argument_string);
/* How many frames of this render state took the previous frame's camera set-up and prepass (gr_frame_tuning.reuse_still_camera). */
int gr_render_state_prepass_reused(gr_render_state* s, unsigned long long* frames);
/* The two estimates tile_history works with (host arithmetic, no device).  gr_camera_origin_on_screen: the pixel at which the
 * camera sees the coordinate origin as if space were flat - the inverse of the kernels' pixel -> direction map (cl.cl:2015-2059) -
 * 1 and pixel_out[0..1] = (x, y), or 0 when the origin is behind the camera or the camera sits on it.  gr_picture_motion: an upper
 * estimate of how many pixels the picture moves between two cameras (angle between the orientations + parallax of the origin, at the
 * focal length); 1e9 when flip or observer speed differ. */
int gr_camera_origin_on_screen(const gr_camera* camera, float field_of_view, int width, int height, float pixel_out[2]);
float gr_picture_motion(const gr_camera* from, const gr_camera* to, float field_of_view, int width);


/* what the prepass policy (gr_frame_options.use_prepass = -2) has done with this state's frames so far, and the fraction of
 * the prepass grid the last inspected prepass made skippable (-1: none inspected yet); any output may be NULL */
int gr_render_state_prepass_policy(gr_render_state* s, unsigned long long* frames_with_prepass, unsigned long long* frames_without,
                                   float* last_marked_fraction);

/* sum of the durations and number of the trace launches (gr_trace_fused / gr_do_generic_rays) logged with time_kernels = 2
 * since the last reset; waits for the logged launches to finish */
int gr_render_state_trace_log(gr_render_state* s, float* total_ms, int* launches, int reset);
/* total Verlet step attempts of the last frame rendered with count_attempts (synchronises the device) */
int gr_render_state_attempts(gr_render_state* s, unsigned long long* attempts);
/* average shader clock (MHz) the fused trace kernel of that frame ran at: wave lifetimes in shader cycles (s_memtime) over the
 * same lifetimes in ticks of the constant 100 MHz reference clock (s_memrealtime); 0 when the frame was not traced by
 * gr_trace_fused with count_attempts (synchronises the device) */
int gr_render_state_shader_clock(gr_render_state* s, double* mhz);
/* of the same launch: the summed lifetime of its waves in milliseconds and how many waves ran.  Over (wave slots the launch
 * held) x (launch duration) this is the share of the slots that was occupied - the rest is the launch's ramp and tail */
int gr_render_state_wave_time(gr_render_state* s, double* wave_ms, unsigned long long* waves);
/* the first count (<= 256) words of that frame's counter block as the kernels left them: [0] attempts, [1] shader cycles,
 * [2] reference-clock ticks, [3] waves, [8..255] only written by probe builds of the kernels (tools/README.md) */
int gr_render_state_counters(gr_render_state* s, unsigned long long* words, int count);

/* the transfer step of gr_render_frame_tiled on its own: `staging` = this participant's compact rows (blocks back to back,
 * gr_tiled_staging_bytes; unused on participant 0), frame_on_root as there */
int gr_tiled_exchange(gr_tiled* t, const void* staging, void* frame_on_root, int rotation, void* stream);
/* the same for a frame of either format (gr_render_frame_tiled_as; gr_tiled_exchange is its GR_FRAME_F32 case): rows of a GR_FRAME_RGBA8
 * frame are width * 4 bytes, in frame_on_root and in the staged blocks alike - block i of this participant at i * block_rows * width * 4,
 * so a byte frame fills the first quarter of gr_tiled_staging_bytes - and a gr_transport is handed width * rows words per block */
int gr_tiled_exchange_as(gr_tiled* t, const void* staging, void* frame_on_root, int rotation, void* stream, int format);
size_t gr_tiled_staging_bytes(const gr_tiled* t);
/* rows [row_begin, row_end) of the local_block-th block of a share; returns 1, 0 for a padding block past the image, -1 on bad
 * arguments.  Pure arithmetic: global block = local_block * world + share. */
int gr_tiled_block_rows(int height, int block_rows, int world, int share, int local_block, int* row_begin, int* row_end);
int gr_tiled_block_rows_of(const gr_tiled* t, int share, int local_block, int* row_begin, int* row_end);

#ifdef __cplusplus
}
#endif
#endif
