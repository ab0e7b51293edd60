// The sequenced row body of the envelope programs: one voice's render cut into spans at the frames where its current segment completes
// (include/oalsfx_hip.h, "envelope programs"), each span rendered by voice_row (voice_rows_body.hpp) as a call of that many frames, the
// head of the voice's queue taken as the current segment in between.  Two kernels compile it: k_program_rows (program.hip) and
// k_program_biquad_rows (biquad.hip).
//
// Records between spans.  voice_row lets lane 0 write the records behind a call, and no lane reads them afterwards; here span k + 1
// needs what span k left in every lane.  So every lane carries what a render changes -- the sampler's position, step and flags, the
// envelope's counters and sub, the queue's head and count: a dozen words -- in registers of its own, and voice_row<..., CARRIED>
// advances them in every lane: integer arithmetic on values that are the same in every lane.  What a render does not change (the
// asset's description, the gains, a segment's lengths and flags) is read where it lies: in the voice's two records, or, once the head
// of the queue has been taken, in the queue's entry, which no render writes.  Global memory is written once, behind the last span, by
// lane 0: the sampler's three fields, the envelope's four, and, where a switch took place, the segment taken last copied whole into the
// voice's envelope record, with the queue's head and count.  No lane reads from global memory what a lane stored earlier in the same
// kernel -- the voice's envelope record is not read again once it has been left for a queue entry --, so nothing has to order the
// lanes against each other; that is also why the host build, where a wavefront's lanes run one after the other with lane 0 last
// (tests/cpp/program_rows_host.cpp), computes what the device computes.
//
// Lane ownership under AddSink.  Frame f of the instance's row belongs to lane (f mod 64) from the zero fill to the last voice.  A span
// that starts at row offset t is rendered into out + t * C with frames counted from 0 again, so it is given the lane number turned back
// by t -- span frame f' = f - t is then lane (f mod 64)'s once more -- and voice_row turns it back further by the segment's delay.
// With StoreSink every frame of [t, t + s) is written exactly once, by whichever lane, and the spans tile [0, F).
//
// stream_rows_body.hpp holds this body's twin, stream_row, with a second reason to end a span (a one-shot's end while the voice's ring
// holds an entry): what changes here in the queue's walk, the span's cut, the lane's rotation or the write-back changes there too.
//
// The including file sets `#pragma clang fp contract(off)` in front of the include.
#ifndef OALSFX_HIP_PROGRAM_ROWS_BODY_HPP
#define OALSFX_HIP_PROGRAM_ROWS_BODY_HPP

#include "program.hpp"
#include "voice_rows_body.hpp"

namespace oalsfx_hip {

namespace {

// "complete": nothing of the segment is left to run
__device__ __forceinline__ bool segment_complete(const oalsfx_envelope& e)
{
    return (e.flags & OALSFX_ENV_ACTIVE) != 0 && e.delay == 0U && e.ramp_done == e.ramp_frames;
}

// A carried word as it is loaded, behind the row's stores, by a vector load: with SCALAR it is said to be the same in every lane and
// lives in a scalar register from span to span, without it where the compiler puts it.  The bits do not depend on it, the registers do:
// the kernel with the filter stage stays within 128 VGPRs at seven channels with it, the one without a filter stage without it.
template <bool SCALAR>
__device__ __forceinline__ uint32_t same(uint32_t v)
{
    if constexpr (SCALAR) return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
    else return v;
}
template <bool SCALAR>
__device__ __forceinline__ uint64_t same(uint64_t v)
{
    return static_cast<uint64_t>(same<SCALAR>(static_cast<uint32_t>(v >> 32))) << 32 | same<SCALAR>(static_cast<uint32_t>(v));
}

// One voice's `frames` frames into the row `out`, [frames][C], its two records advanced and its queue shortened, by one wavefront: `lane`
// is the caller's lane; *rec, *env, *prog and `table` are the same in every lane.  With an empty queue this is voice_row's one call.
template <int C, int V, class Sink, bool SCALAR>
__device__ __forceinline__ void program_row(oalsfx_sampler* rec, oalsfx_envelope* env, EnvProgram* prog, int table, const FirTables& tables, float* out,
                                            unsigned frames, unsigned lane)
{
    Carried now;
    now.position = same<SCALAR>(static_cast<uint64_t>(rec->position));
    now.step = same<SCALAR>(rec->step);
    now.flags = same<SCALAR>(rec->flags);
    const uint32_t flags0 = now.flags;
    const oalsfx_envelope* segment = env; // the current one: the voice's record, or the queue's entry taken last
    const auto take = [&now](const oalsfx_envelope* from) {
        now.delay = same<SCALAR>(from->delay);
        now.ramp_done = same<SCALAR>(from->ramp_done);
        now.glide_done = same<SCALAR>(from->glide_done);
        now.sub = same<SCALAR>(from->sub);
    };
    take(segment);
    const uint32_t head0 = same<SCALAR>(prog->head);
    uint32_t head = head0, count = same<SCALAR>(prog->count);
    unsigned t = 0;
    for (;;) {
        const uint32_t eflags = segment->flags;
        // (also at t == frames: a segment that completes on the render's last frame is replaced in this render)
        if (count != 0U && (eflags & OALSFX_ENV_ACTIVE) != 0 && now.delay == 0U && now.ramp_done == segment->ramp_frames) {
            segment = &prog->queue[head];
            take(segment);
            ++head;
            --count;
            continue;
        }
        if (t == frames) break;
        unsigned span = frames - t;
        if (count != 0U && (eflags & OALSFX_ENV_ACTIVE) != 0) {
            // not complete: at least one frame is left (ramp_done <= ramp_frames: refused otherwise)
            const uint64_t left = static_cast<uint64_t>(now.delay) + (segment->ramp_frames - now.ramp_done);
            if (left < span) span = static_cast<unsigned>(left);
        }
        // (the lane number made opaque once per span: what the render computes from it alone would otherwise be held across the spans)
        unsigned mine = Sink::kAdds ? (lane + kWave - t % kWave) % kWave : lane;
#ifndef OALSFX_FIR_HOST_SHIM
        asm volatile("" : "+v"(mine));
#endif
        voice_row<C, V, Sink, true, true>(rec, const_cast<oalsfx_envelope*>(segment), table, tables, out + static_cast<size_t>(t) * C, span, mine, &now);
        t += span;
    }
    // (a voice that neither plays nor has an active envelope -- one busy through its filter alone -- has changed nothing: no store, as in
    // voice_row; a voice with a queue has an ACTIVE envelope)
    if (lane != 0 || (!(flags0 & OALSFX_SAMPLER_PLAYING) && !(env->flags & OALSFX_ENV_ACTIVE))) return;
    // what the spans changed in the sampler's record ...
    rec->position = now.position;
    rec->step = now.step;
    rec->flags = now.flags;
    // ... and the current segment: where the queue's head was taken, that record whole, then the counters as the spans left them
    if (head != head0) {
        *env = *segment;
        prog->head = head;
        prog->count = count;
    }
    env->delay = now.delay;
    env->ramp_done = now.ramp_done;
    env->glide_done = now.glide_done;
    env->sub = now.sub;
}

} // namespace

} // namespace oalsfx_hip

#endif
