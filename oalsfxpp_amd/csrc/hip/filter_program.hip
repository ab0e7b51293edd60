// Filter programs: a voice filter's queued sweeps take their turn inside a render, at the exact frame (include/oalsfx_hip.h, "filter
// programs").  A voice's sweep record is the current segment; its row of the queues' table holds up to seven more.  A render of F frames
// is cut at the frames where the current segment completes: each span is filtered as "voice filter sweeps" filters a render of that many
// frames, and in between the head of the queue is copied over the current segment.
//
// The kernels are k_sweep_rows and k_sweep_program_rows (biquad.hip's row body: one wavefront per instance, four to a workgroup, the
// filtered voice rendered into the instance's scratch row first, wavefront-scope syncs only and NO workgroup barrier; C + 2 LDS rows per
// wavefront) with one more table beside the others.  A filtered voice's stage looks at the count of the voice's queue first, one word
// that is the same in every lane.  With an empty queue it is sweep.hip's stage, sweep_row or filter_row, on the same bits.  Otherwise it
// runs filter_program_row, which is sweep_row with one change in the lane = frame phase: unlike an envelope program's, a frame's
// coefficients depend only on the frame's index and the program, so there is no span loop around the recurrence and nothing is carried
// but the histories.  Per tile of 64 frames the wavefront walks the segments that overlap the tile -- a loop that is the same in every
// lane, the segment's from, step and to the same in every lane as well -- and a lane forms its five coefficients in the iteration
// whose range holds its frame: from[k] + ((float)n * step[k]) with n the frame's index inside the segment.  Phases 2 and 3 are
// sweep_row's.  Behind the last tile the lanes c < C write the histories and lane 0 writes, once, what is the same in every lane: the
// segment the render ended in (copied whole where the queue was walked) with its `done`, or the spent last one without ACTIVE; the
// queue's head and count; and, where a segment completed, the filter record's coefficients, `to` of the last one that did.  No lane reads
// what a lane stored in the same kernel.
//
// stream.hip includes this file with OALSFX_FILTER_PROGRAM_BODY_ONLY set, for the stages and the row body around them without the kernels.
//
// The file also compiles for the host, each phase run over the 64 lanes in turn (tests/cpp/filter_program_rows_host.cpp).
#include "filter_program.hpp"

#pragma clang fp contract(off)

// (the sweeps' stages and the row body around them, without their kernels)
#define OALSFX_SWEEP_BODY_ONLY 1
#include "sweep.hip"

namespace oalsfx_hip {

namespace {

static_assert(offsetof(FilterProgram, queue) == 16 && sizeof(FilterProgram) == 16 + 7 * sizeof(oalsfx_filter_sweep), "the layout the programmed stage reads and writes");

// (a word that is the same in every lane, said so: it lives in a scalar register, and what is decided by it is a scalar branch)
__device__ __forceinline__ uint32_t in_every_lane(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

// The segment a walk stands in, the same in every lane: where its record is, its three counters, and `start`, the frame of the render
// that has the index `done`.  Under way: ACTIVE with done < length; only the last segment of a program (the queue empty behind it) may
// be anything else.  from, step and to stay in memory: a lane loads them where it forms its coefficients, and holds nothing of them
// across the phases (fifteen registers on top of sweep_row's 125 at seven channels would not fit).
struct FilterWalk {
    const oalsfx_filter_sweep* at;
    uint32_t flags, length, done;
    unsigned start;
};

__device__ __forceinline__ void take_segment(FilterWalk& g, const oalsfx_filter_sweep* from, unsigned start)
{
    g.at = from;
    g.flags = in_every_lane(from->flags);
    g.length = in_every_lane(from->frames);
    g.done = in_every_lane(from->done);
    g.start = start;
}

__device__ __forceinline__ bool under_way(const FilterWalk& g) { return (g.flags & OALSFX_SWEEP_ACTIVE) != 0 && g.done < g.length; }

// ---- phase 1b of a programmed voice, lane = frame `at` of the render, once per segment that overlaps the tile, in the program's order:
// a frame at or behind the segment's first takes its coefficients from it -- the ramp's at the index done + (at - start), `to` behind the
// ramp's end, plain[0 .. 4] (the filter record's, or `to` of the segment before) where the segment is not under way.  A later segment's
// call replaces what an earlier one's left for the frames behind its end ----
__device__ __forceinline__ void segment_coefficients(float (&k)[5], unsigned at, const FilterWalk& g, const float* plain)
{
    if (at < g.start) return;
    const bool under = under_way(g);
    const unsigned since = at - g.start;
    if (under && since < g.length - g.done) {
        const float n = static_cast<float>(g.done + since); // below R <= 2^24: exact
#pragma unroll
        for (int j = 0; j < 5; ++j) k[j] = g.at->from[j] + (n * g.at->step[j]);
    } else {
        const float* const held_at = under ? g.at->to : plain;
#pragma unroll
        for (int j = 0; j < 5; ++j) k[j] = held_at[j];
    }
}

// ---- ... then, once per tile: u into row c with the lane's own k[0 .. 2], its k[3] and k[4] (a1, a2) into rows C, C + 1: the second half
// of sweep.hip's swept_feed_phase (written again here: taken out of that function as one of its own, it changed the order of the
// instructions of k_sweep_rows from four channels on) ----
template <int C>
__device__ __forceinline__ void own_feed_phase(const FilterLanes<C>& s, unsigned l, const float (&k)[5], const float (&xh1)[C], const float (&xh2)[C], float* rows)
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float up1 = below(s, c, l, 1U), up2 = below(s, c, l, 2U);
        const float x1 = l >= 1U ? up1 : xh1[c];
        const float x2 = l >= 2U ? up2 : l == 1U ? xh1[c] : xh2[c];
        rows[c * kFilterRow + 4 + l] = ((k[0] * s.x[held(l)][c]) + (k[1] * x1)) + (k[2] * x2);
    }
    rows[C * kFilterRow + 4 + l] = k[3];
    rows[(C + 1) * kFilterRow + 4 + l] = k[4];
}

// sweep_row for a voice whose queue holds a segment: *queue has count >= 1, the same in every lane; rows: the wavefront's C + 2 LDS rows.
// Afterwards the histories in *rec are those of the render's last two frames, *sweep is the segment the render ended in, *queue is
// shorter by the segments taken, and where a segment completed *rec holds `to` of the last one that did.
template <int C, int V>
__device__ __forceinline__ void filter_program_row(FilterProgram* queue, oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* in, float* out,
                                                   unsigned frames, unsigned lane, bool add, float* rows)
{
    static_assert(offsetof(oalsfx_voice_filter, a2) == offsetof(oalsfx_voice_filter, b0) + 16, "b0, b1, b2, a1, a2 in a row, as from, step and to have them");
    uint32_t head = in_every_lane(queue->head), count = in_every_lane(queue->count);
    FilterWalk g;
    take_segment(g, sweep, 0U);
    const float* plain = &rec->b0; // the coefficients of a frame behind the last segment that completed: the record's, until one has
    bool taken = false;            // a segment came from the queue
    float xh1[C], xh2[C]; // the inputs of the two frames in front of the tile: the same in every lane
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xh1[c] = rec->x[c][0];
        xh2[c] = rec->x[c][1];
    }
    FilterLanes<C> s;
    OALSFX_EACH_LANE(l, lane) {
        s.y1[held(l)] = 0.0F;
        s.y2[held(l)] = 0.0F;
        if (l < C) {
            s.y1[held(l)] = rec->y[l][0];
            s.y2[held(l)] = rec->y[l][1];
        }
    }
    for (unsigned base = 0; base < frames; base += kWave) {
        const unsigned L = frames - base < kWave ? frames - base : kWave;
        OALSFX_EACH_LANE(l, lane) load_phase<C, V>(s, l, in, base, L);
        float k[kHeld][5];
        OALSFX_EACH_LANE(l, lane) {
#pragma unroll
            for (int j = 0; j < 5; ++j) k[held(l)][j] = 0.0F; // (g.start <= base: the first segment's call below writes every lane's)
        }
        // the segments that overlap the tile, a loop that is the same in every lane; behind the last tile base + L == frames, and a
        // segment that completes on the render's last frame is replaced here
        for (;;) {
            if (count != 0U && !under_way(g)) {
                take_segment(g, &queue->queue[head], g.start);
                ++head;
                --count;
                taken = true;
                continue;
            }
            OALSFX_EACH_LANE(l, lane) segment_coefficients(k[held(l)], base + l, g, plain);
            if (count == 0U) break; // the last segment: to the render's end, as a sweep runs
            const unsigned left = g.length - g.done;
            if (left > base + L - g.start) break; // goes on behind the tile
            plain = g.at->to;
            g.start += left;
            g.done = g.length;
        }
        OALSFX_EACH_LANE(l, lane) own_feed_phase<C>(s, l, k[held(l)], xh1, xh2, rows);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float last = of_lane(s, c, L - 1U), before = of_lane(s, c, L >= 2U ? L - 2U : 0U);
            xh2[c] = L >= 2U ? before : xh1[c];
            xh1[c] = last;
        }
        wave_sync();
        OALSFX_EACH_LANE(l, lane) swept_recur_phase<C>(s, l, L, rows);
        wave_sync();
        OALSFX_EACH_LANE(l, lane) out_phase<C, V>(l, base, L, rows, out, add);
        wave_sync(); // the rows are free for the next tile, the scratch row behind the last one for the next voice
    }
    OALSFX_EACH_LANE(l, lane) {
        float mine1 = 0.0F, mine2 = 0.0F;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (l == static_cast<unsigned>(c)) {
                mine1 = xh1[c];
                mine2 = xh2[c];
            }
        }
        if (l < C) {
            rec->x[l][0] = mine1;
            rec->x[l][1] = mine2;
            rec->y[l][0] = s.y1[held(l)];
            rec->y[l][1] = s.y2[held(l)];
        }
    }
    // what is the same in every lane, written once: g is the segment the render ended in, frames - g.start of its frames run here
    if (lane == 0U) {
        const bool under = under_way(g);
        const unsigned ran = frames - g.start, left = g.length - g.done;
        const bool completes = under && ran >= left; // (the last segment: one with a queue behind it was replaced above)
        if (completes) plain = g.at->to;
        float coefficients[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) coefficients[j] = plain[j];
        if (taken) {
            // (g.at is a row of the queue, which no lane writes)
            sweep->frames = g.length;
            sweep->reserved = 0U;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                sweep->from[j] = g.at->from[j];
                sweep->step[j] = g.at->step[j];
                sweep->to[j] = g.at->to[j];
            }
            sweep->reserved1 = 0.0F;
            queue->head = head;
            queue->count = count;
        }
        if (under) {
            sweep->done = completes ? g.length : g.done + ran;
            sweep->flags = completes ? g.flags & ~static_cast<uint32_t>(OALSFX_SWEEP_ACTIVE) : g.flags;
        } else if (taken) {
            sweep->done = g.done;
            sweep->flags = g.flags;
        }
        if (plain != &rec->b0) {
            rec->b0 = coefficients[0];
            rec->b1 = coefficients[1];
            rec->b2 = coefficients[2];
            rec->a1 = coefficients[3];
            rec->a2 = coefficients[4];
        }
    }
}

template <int C, int V>
__device__ __forceinline__ void queued_or_sweep_row(FilterProgram* queue, oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* from, float* out,
                                                    unsigned frames, unsigned lane, bool add, float* rows)
{
    // (the same in every lane: the whole wavefront goes one way)
    if (queue->count != 0U) filter_program_row<C, V>(queue, sweep, rec, from, out, frames, lane, add, rows);
    else sweep_or_filter_row<C, V>(sweep, rec, from, out, frames, lane, add, rows);
}

} // namespace

#ifndef OALSFX_FILTER_PROGRAM_BODY_ONLY
// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_filter_program_resources.py)
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_filter_program_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                       oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps, FilterProgram* queues,
                                                                       const FirTables tables, float* dst, float* scratch, int instances, int lanes, unsigned frames)
{
    biquad_rows<C, V, false, true, true>(records, envelopes, resamplers, filters, nullptr, sweeps, tables, dst, scratch, instances, lanes, frames, queues);
}

// k_filter_program_rows while a voice's envelope program may hold a segment (include/oalsfx_hip.h, "envelope programs")
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_filter_program_env_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                           oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps, FilterProgram* queues,
                                                                           EnvProgram* programs, const FirTables tables, float* dst, float* scratch, int instances,
                                                                           int lanes, unsigned frames)
{
    biquad_rows<C, V, true, true, true>(records, envelopes, resamplers, filters, programs, sweeps, tables, dst, scratch, instances, lanes, frames, queues);
}

// The rows oalsfx_batch_set_filter_programs has written since the last render (and those a plain set has emptied), put in place in front
// of it: a thread per 16-byte piece.
__global__ __launch_bounds__(256) void k_filter_program_upload(FilterProgram* queues, const int* __restrict__ index, const FilterProgram* __restrict__ changed, int count)
{
    constexpr unsigned kPieces = sizeof(FilterProgram) / 16;
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned k = g / kPieces, piece = g % kPieces;
    if (k >= static_cast<unsigned>(count)) return;
    const uint32_t* const from = reinterpret_cast<const uint32_t*>(changed + k) + piece * 4U;
    uint32_t* const to = reinterpret_cast<uint32_t*>(queues + index[k]) + piece * 4U;
#pragma unroll
    for (int i = 0; i < 4; ++i) to[i] = from[i];
}

bool launch_filter_program(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                           FilterProgram* queues, const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch,
                           hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_filter_program_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters, sweeps,
                           queues, tables, dst, scratch, instances, lanes, frames);
    });
}

bool launch_filter_program_env(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                               FilterProgram* queues, EnvProgram* programs, const FirTables& tables, int instances, int lanes, unsigned frames, int channels,
                               float* dst, float* scratch, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_filter_program_env_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters,
                           sweeps, queues, programs, tables, dst, scratch, instances, lanes, frames);
    });
}

void launch_filter_program_upload(FilterProgram* queues, const int* index, const FilterProgram* changed, int count, hipStream_t stream)
{
    constexpr unsigned kPieces = sizeof(FilterProgram) / 16;
    const unsigned threads = static_cast<unsigned>(count) * kPieces;
    hipLaunchKernelGGL(k_filter_program_upload, dim3((threads + 255U) / 256U), dim3(256), 0, stream, queues, index, changed, count);
}
#endif // OALSFX_FILTER_PROGRAM_BODY_ONLY

} // namespace oalsfx_hip
