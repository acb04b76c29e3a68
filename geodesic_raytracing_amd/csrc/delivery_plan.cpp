// delivery_plan.cpp — the decisions of a frame's delivery (delivery_plan.hpp).  No HIP call, no state written: facts in, plan out.
#include "delivery_plan.hpp"

namespace delivery_plan {

namespace {
plan refuse(const char* text) {
    plan p;
    p.refused = text;
    return p;
}

// one more stage; what it writes, if that is a buffer of the state's, the call needs
buffer add(plan& p, stage_kind kind, buffer source, buffer destination, int factor, bool with_strips = false) {
    p.stages[p.count++] = {kind, source, destination, factor, with_strips};
    if (destination < STATE_BUFFERS) p.needs |= 1u << destination;
    return destination;
}
}   // namespace

plan plan_delivery(const facts& f) {
    // a factor-1 box state's float4 frame has no chain, and a frame without `out` stops after its records: nothing was shaded
    if (f.call == DELIVER && f.format == GR_FRAME_F32 && ((f.factor == 1 && !f.filtered && !f.glare_set && f.tone == TONE_NONE) || f.out_is_null)) {
        plan p;
        p.direct = true;
        return p;
    }
    if (f.block_rows > 0x7fffffff / f.factor) return refuse("block_rows");
    // filter, glare and tone read beyond a strip's rows; the state's setting counts, whichever call would set it to work
    if (f.strip_count > 1) {
        if (f.filtered) return refuse("a state with a filter renders whole frames only (strip_count > 1): a filter wider than a pixel reads across strip borders");
        if (f.glare_set) return refuse("a state with a glare renders whole frames only (strip_count > 1): the PSF reads across strip borders");
        if (f.tone != TONE_NONE) return refuse("a state with a tone renders whole frames only (strip_count > 1): a histogram of a strip is not the frame's");
    }
    const bool traces = f.call != DELIVER_ACCUMULATED, accumulates = f.call == ACCUMULATE_SUBFRAME;
    // a sub-frame is accumulated without glare and tone: the delivery applies them to the sum, once
    const bool glared = f.glare_set && !accumulates, toned = f.tone != TONE_NONE && !accumulates;
    // The float4 stages (FILTER or BOX, GLARE, TONE) write a frame of the state's each - but the last of them the caller's memory, if
    // that is float4.
    const bool float_out = !accumulates && f.format == GR_FRAME_F32;
    const auto into = [&](bool last, buffer own) { return last && float_out ? OUT : own; };
    plan p;
    buffer at = traces ? TRACED : ACCUMULATION;   // where the frame is, at `factor` x the output size
    int factor = traces ? f.factor : 1;
    if (traces) p.needs |= 1u << TRACED;
    if (traces && (f.filtered || ((glared || toned) && factor > 1))) {
        at = add(p, f.filtered ? FILTER : BOX, at, into(!glared && !toned, RESOLVED), factor);
        p.needs |= 1u << RESOLVED;   // (kept: allocated even where the filter writes the caller's memory)
        factor = 1;
    }
    if (glared) {
        at = add(p, GLARE, at, into(!toned, GLARE_FRAME), 1);
        p.needs |= 1u << GLARE_FRAME | 1u << GLARE_SCRATCH;   // (kept: the glare frame likewise)
    }
    if (toned) {
        if (f.tone == TONE_AUTO) {
            if (f.tone_reset) add(p, ZERO_TONE_STATE, NONE, NONE, 1);
            add(p, METER, at, NONE, 1);
            add(p, SOLVE, NONE, NONE, 1);
            p.needs |= 1u << TONE_WORDS;
        }
        at = add(p, TONE, at, into(true, TONE_FRAME), 1);
    }
    if (accumulates) add(p, ACCUMULATE, at, ACCUMULATION, factor);
    else if (at != OUT) add(p, ENCODE, at, OUT, factor, f.mode_is_fused && f.strip_count > 1);
    return p;
}

}   // namespace delivery_plan
