// delivery_plan.hpp — what a frame's delivery DECIDES, apart from what it launches: for a state (supersampling factor, filter, glare,
// tone) and a call (a frame in a format, a sub-frame of a shutter, the delivery of the accumulation) which stages run behind the trace,
// in what order, from and into which buffer, which of the state's buffers the call needs, and what it refuses.  Plain C++, no HIP
// header: every decision here can be checked without a GPU (tests/delivery_plan_check.cpp).  frame.cpp gathers the facts and carries the
// plan out; the stages' launchers are in frame_launch.cpp.
//
// The chain, once: a traced frame is float4 at factor x the output size.  A filter other than the box resolves it (FILTER); the box is
// part of the sink's own kernel (ENCODE and ACCUMULATE read at the factor) unless a glare or a tone stands in between, which want the
// resolved frame (BOX).  Then the glare (GLARE), then in auto mode the meter and the solve of the gain (ZERO_TONE_STATE first where the
// adaptation starts again), then the tone curve (TONE).  The last of these writes the caller's memory where that is float4; else each
// writes a frame of the state's, and the format's kernel encodes the last at factor 1 (ENCODE).  A sub-frame is resolved as far as the
// filter and accumulated; glare and tone wait for the delivery of the sum, which is the same chain from ACCUMULATION.
#pragma once

#include "internal.hpp"

namespace delivery_plan __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

enum call_kind { DELIVER, ACCUMULATE_SUBFRAME, DELIVER_ACCUMULATED };   // gr_render_frame*, gr_render_subframe, gr_deliver_accumulated
enum tone_kind { TONE_NONE, TONE_MANUAL, TONE_AUTO };

struct facts {
    int factor = 1;
    bool filtered = false;      // the state's filter is not GR_FILTER_BOX
    bool glare_set = false;
    tone_kind tone = TONE_NONE;
    bool tone_reset = false;    // the adaptation state is to be zeroed (set by gr_render_state_set_tone, or the words are not allocated yet)
    int format = GR_FRAME_F32;
    call_kind call = DELIVER;
    bool out_is_null = false;
    int strip_count = 1;
    bool mode_is_fused = true;
    int block_rows = 0;         // in output rows; the frame behind them is traced in blocks of factor x as many
};

// Names, not pointers.  The first seven are buffers of the state, in the order they are allocated in; RESOLVED is its filtered_frame.
enum buffer { TRACED, ACCUMULATION, RESOLVED, GLARE_FRAME, GLARE_SCRATCH, TONE_FRAME, TONE_WORDS, STATE_BUFFERS, OUT = STATE_BUFFERS, NONE };
enum stage_kind { FILTER, BOX, GLARE, ZERO_TONE_STATE, METER, SOLVE, TONE, ACCUMULATE, ENCODE };

struct stage {
    stage_kind kind;
    buffer source, destination;   // NONE: the stage reads / writes no frame (the tone state's words are METER's, SOLVE's and ZERO_TONE_STATE's)
    int factor;                   // the source is factor x the output size per axis
    bool with_strips;             // ENCODE: the call's strip description goes to the launcher (else: the whole frame)
};

struct plan {
    const char* refused = nullptr;   // GR_ERROR_INVALID_ARGUMENT with this text behind the entry point's name and ": "
    bool direct = false;             // the frame is traced straight into the caller's memory and nothing follows
    int count = 0;
    stage stages[8] = {};            // (at most FILTER, GLARE, ZERO_TONE_STATE, METER, SOLVE, TONE, ENCODE)
    unsigned needs = 0;              // bit b: the call needs the state's buffer b; what is missing is allocated before anything is rendered
};

plan plan_delivery(const facts& f);

}   // namespace delivery_plan
