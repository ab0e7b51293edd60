// The sequenced row body of the sampler streams: program_row (program_rows_body.hpp) with a second reason to end a span.  One voice's
// render is cut where its current envelope segment completes, as there, and where its current one-shot ends while its ring holds an
// entry (include/oalsfx_hip.h, "sampler streams"); each span is rendered by voice_row as a call of that many frames; in between the head
// of the envelope queue is taken as the current segment, and the head of the ring as the current sampler record, at the entry's position
// plus the excess by which the span's last step ran past the end.  k_stream_rows (stream.hip) compiles it.
//
// Records between spans are carried as in program_row, in every lane; the carried words gain the taken count and the excess.  What a
// render does not change in a sampler's record -- the asset's description, the loop, the gains -- is read where it lies: in the voice's
// record, or, once the ring's head has been taken, in the ring's entry, which no render writes.  Global memory is written once, behind
// the last span, by lane 0: where an entry was taken, the entry taken last copied whole into the voice's sampler record and the taken
// count; then position, step and flags; then the envelope as program_row leaves it.  No lane reads from global memory what a lane stored
// earlier in the same kernel, so nothing orders the lanes against each other, and the host build, where the lanes run one after the
// other with lane 0 last, computes what the device computes.
//
// Where the end lies.  A streaming voice's envelope does not GLIDE (refused on the host), so its step is constant and sub takes no part
// in a frame's 12-bit position: frame j of the sampler reads at q_j = P + j * step exactly.  The first j with q_j >= E is n = ceil((E - P)
// / step), n >= 1 because P < E; that frame lies delay + n frames ahead, and its excess is P + n * step - E, below step and so below
// 2^32.  A span cut there leaves the record at E with PLAYING cleared (voice_row's own ending) exactly when the sampler ran over all n
// frames; a STOP that completes first leaves it short of E, not PLAYING, and nothing is taken.
//
// The including file sets `#pragma clang fp contract(off)` in front of the include.
#ifndef OALSFX_HIP_STREAM_ROWS_BODY_HPP
#define OALSFX_HIP_STREAM_ROWS_BODY_HPP

#include "stream.hpp"
#include "program_rows_body.hpp"

namespace oalsfx_hip {

namespace {

// One voice's `frames` frames into the row `out`, [frames][C], its two records advanced, its envelope queue and its ring shortened, by
// one wavefront: `lane` is the caller's lane; everything else is the same in every lane.  prog may be null (no queue table: an empty
// queue).  With an empty queue and an empty ring this is voice_row's one call.
template <int C, int V, class Sink, bool SCALAR>
__device__ __forceinline__ void stream_row(oalsfx_sampler* rec, oalsfx_envelope* env, EnvProgram* prog, const StreamRing* ring, uint32_t* taken_at, int table,
                                           const FirTables& tables, float* out, unsigned frames, unsigned lane)
{
    Carried now;
    now.position = same<SCALAR>(static_cast<uint64_t>(rec->position));
    now.step = same<SCALAR>(rec->step);
    now.flags = same<SCALAR>(rec->flags);
    const uint32_t flags0 = now.flags;
    const oalsfx_sampler* entry = rec;    // the current one: the voice's record, or the ring's entry taken last
    const oalsfx_envelope* segment = env; // ... and the same for the envelope
    const auto take = [&now](const oalsfx_envelope* from) {
        now.delay = same<SCALAR>(from->delay);
        now.ramp_done = same<SCALAR>(from->ramp_done);
        now.glide_done = same<SCALAR>(from->glide_done);
        now.sub = same<SCALAR>(from->sub);
    };
    take(segment);
    const uint32_t head0 = prog ? same<SCALAR>(prog->head) : 0U;
    uint32_t head = head0, count = prog ? same<SCALAR>(prog->count) : 0U;
    // (the queued count is read once, here: what is appended behind the render's start waits for the next render)
    // (never more than the ring holds: the host keeps queued - taken within it, and a walk that trusted a broken pair would not end)
    // The words this body carries beyond program_row's -- the two counts and the excess -- are said to be the same in every lane
    // whatever SCALAR says of the others: they live in scalar registers across the spans, and the kernel keeps program_row's VGPRs.
    const uint32_t taken0 = same<true>(*taken_at), waiting0 = same<true>(ring->queued) - taken0;
    uint32_t taken = taken0, waiting = waiting0 <= OALSFX_STREAM_QUEUE ? waiting0 : 0U;
    // by how much the span before ran past the end; 0 for a record that was at its end when the render began.  One word: an excess is
    // below the step that made it, and an entry that hands it on takes its own frames off it
    uint32_t over = 0;
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
        const uint64_t E = static_cast<uint64_t>(entry->frames) << kFrac;
        // (also at t == frames, and in a row: an entry whose start lies at or past its own end hands the rest of the excess on)
        if (waiting != 0U && !(now.flags & OALSFX_SAMPLER_LOOP) && now.position >= E) {
            entry = &ring->entry[taken % OALSFX_STREAM_QUEUE];
            ++taken;
            --waiting;
            uint64_t q = entry->position + over;
            uint32_t flags = entry->flags;
            over = 0;
            if (flags & OALSFX_SAMPLER_LOOP) {
                const uint64_t L0 = static_cast<uint64_t>(entry->loop_start) << kFrac, L1 = static_cast<uint64_t>(entry->loop_end) << kFrac;
                if (q >= L1) q = wrap_past(q, L0, L1, L1 - L0);
            } else {
                const uint64_t end = static_cast<uint64_t>(entry->frames) << kFrac;
                if (q >= end) {
                    // the samplers' ending, should the ring be empty now
                    over = same<true>(static_cast<uint32_t>(q - end));
                    q = end;
                    flags &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
                }
            }
            now.position = same<SCALAR>(q);
            now.step = same<SCALAR>(entry->step);
            now.flags = same<SCALAR>(flags);
            continue;
        }
        if (t == frames) break;
        unsigned span = frames - t;
        const bool active = (eflags & OALSFX_ENV_ACTIVE) != 0;
        if (count != 0U && active) {
            // not complete: at least one frame is left (ramp_done <= ramp_frames: refused otherwise)
            const uint64_t left = static_cast<uint64_t>(now.delay) + (segment->ramp_frames - now.ramp_done);
            if (left < span) span = static_cast<unsigned>(left);
        }
        over = 0;
        if (waiting != 0U && (now.flags & (OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP)) == OALSFX_SAMPLER_PLAYING && now.step != 0U) {
            // position < E: the record would have been replaced above
            const uint64_t n = (E - now.position + (now.step - 1U)) / now.step;
            const uint64_t left = (active ? now.delay : 0U) + n;
            if (left < span) span = static_cast<unsigned>(left);
            over = same<true>(static_cast<uint32_t>(now.position + n * now.step - E));
        }
        // (the lane number made opaque once per span: what the render computes from it alone would otherwise be held across the spans)
        unsigned mine = Sink::kAdds ? (lane + kWave - t % kWave) % kWave : lane;
#ifndef OALSFX_FIR_HOST_SHIM
        asm volatile("" : "+v"(mine));
#endif
        voice_row<C, V, Sink, true, true>(const_cast<oalsfx_sampler*>(entry), const_cast<oalsfx_envelope*>(segment), table, tables, out + static_cast<size_t>(t) * C,
                                          span, mine, &now);
        t += span;
        // (the excess counts only where the span reached the end: it was cut there, so it ran over the n frames `over` was formed for;
        // a span that did not left the record short of its end, and nothing is taken behind it)
        if (now.position != static_cast<uint64_t>(entry->frames) << kFrac) over = 0;
    }
    // (a voice that neither plays nor has an active envelope and took nothing has changed nothing: no store, as in voice_row)
    if (lane != 0 || (!(flags0 & OALSFX_SAMPLER_PLAYING) && !(env->flags & OALSFX_ENV_ACTIVE) && taken == taken0)) return;
    // the entry taken last, whole ...
    if (taken != taken0) {
        *rec = *entry;
        *taken_at = taken;
    }
    // ... what the spans changed in the sampler's record ...
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
