// Voice filter sweeps: a voice filter whose five coefficients ramp per frame (include/oalsfx_hip.h, "voice filter sweeps").  For a voice
// whose filter is ACTIVE and whose sweep is ACTIVE with done < R, frame f of the render has the index n = done + f and the coefficients
// from[k] + ((float)n * step[k]) for n < R, to[k] from there on -- the product and the sum each rounded by themselves, no running sum --
// and y_f = ((((b0_f * x_f) + (b1_f * x_(f-1))) + (b2_f * x_(f-2))) - (a1_f * y_(f-1))) - (a2_f * y_(f-2)).
//
// The kernels are k_biquad_rows and k_program_biquad_rows (biquad.hip's row body: one wavefront per instance, four to a workgroup, the
// filtered voice rendered into the instance's scratch row first, wavefront-scope syncs only and NO workgroup barrier) with one more
// table beside the others and two more LDS rows per wavefront.  A filtered voice's stage looks at the voice's sweep record first, three
// words that are the same in every lane.  Without a sweep under way it runs filter_row, the stage of the other kernels, on the same bits.
// With one it runs sweep_row, the same three phases per tile of 64 frames:
//   1. lane = frame: the lane forms its frame's five coefficients from n = done + base + lane, writes u = ((b0 x) + (b1 x1)) + (b2 x2)
//      into row c of the wavefront's LDS block with its OWN b0, b1, b2, and its a1 and a2 into rows C and C + 1;
//   2. lane = channel, c < C: the recurrence y_i = (u_i - a1[i] y1) - a2[i] y2 over its row (filter_recurrence.hpp,
//      filter_recurrence_swept), a1[i] and a2[i] from the two rows, which all channel lanes read at the same address;
//   3. lane = frame: the outputs stored or added, as in filter_row.
// Behind the last tile the lanes c < C write the histories, and lane 0 writes what is the same in every lane: the sweep's `done`, and
// in the render in which it reaches R the filter record's five coefficients (`to`) and the sweep's flags without ACTIVE.  A sweep that
// completes in mid-render needs no second pass: the lanes at and behind its end take `to`, which is what a plain filter would compute.
//
// The file also compiles for the host, each phase run over the 64 lanes in turn (tests/cpp/sweep_rows_host.cpp).
// filter_program.hip includes it with OALSFX_SWEEP_BODY_ONLY set, for the stages without the kernels.
#include "sweep.hpp"

#pragma clang fp contract(off)

// (the voice filters' stage and row body, without their kernels)
#define OALSFX_BIQUAD_BODY_ONLY 1
#include "biquad.hip"

namespace oalsfx_hip {

namespace {

static_assert(sizeof(oalsfx_filter_sweep) == 80 && offsetof(oalsfx_filter_sweep, from) == 16 && offsetof(oalsfx_filter_sweep, step) == 36 &&
              offsetof(oalsfx_filter_sweep, to) == 56, "the layout the sweep's stage reads and writes");

// ---- phase 1b of a swept voice, lane = frame `at` of the render: the frame's coefficients; u into row c, a1 and a2 into rows C, C + 1.
// `left` = R - done in front of the render: the frames that still ramp ----
template <int C>
__device__ __forceinline__ void swept_feed_phase(const FilterLanes<C>& s, unsigned l, unsigned at, unsigned done, unsigned left, const float (&from)[5],
                                                 const float (&step)[5], const float (&to)[5], const float (&xh1)[C], const float (&xh2)[C], float* rows)
{
    const bool ramps = at < left;
    const float n = static_cast<float>(ramps ? done + at : 0U); // below R <= 2^24: exact
    float k[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float on_ramp = from[j] + (n * step[j]);
        k[j] = ramps ? on_ramp : to[j];
    }
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

// ---- phase 2 of a swept voice, lane = channel ----
template <int C>
__device__ __forceinline__ void swept_recur_phase(FilterLanes<C>& s, unsigned l, unsigned L, float* rows)
{
    if (l < C)
        filter_recurrence_swept(rows + l * kFilterRow, rows + C * kFilterRow + 4, rows + (C + 1) * kFilterRow + 4, static_cast<int>(L), s.y1[held(l)], s.y2[held(l)]);
}

// filter_row for a voice whose sweep is under way: *sweep is ACTIVE with done < frames, the same in every lane; rows: the wavefront's
// C + 2 LDS rows.  Afterwards the histories in *rec are those of the render's last two frames, sweep->done has moved on by the render's
// frames, and where it has reached the sweep's length *rec holds `to` and *sweep is no longer ACTIVE.
template <int C, int V>
__device__ __forceinline__ void sweep_row(oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* in, float* out, unsigned frames, unsigned lane, bool add,
                                          float* rows)
{
    const uint32_t flags = sweep->flags, length = sweep->frames, done = sweep->done;
    const unsigned left = length - done;
    float from[5], step[5], to[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        from[j] = sweep->from[j];
        step[j] = sweep->step[j];
        to[j] = sweep->to[j];
    }
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
        OALSFX_EACH_LANE(l, lane) swept_feed_phase<C>(s, l, base + l, done, left, from, step, to, xh1, xh2, rows);
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
    // what is the same in every lane, written once
    if (lane == 0U) {
        const bool completes = frames >= left;
        sweep->done = completes ? length : done + frames;
        if (completes) {
            rec->b0 = to[0];
            rec->b1 = to[1];
            rec->b2 = to[2];
            rec->a1 = to[3];
            rec->a2 = to[4];
            sweep->flags = flags & ~static_cast<uint32_t>(OALSFX_SWEEP_ACTIVE);
        }
    }
}

template <int C, int V>
__device__ __forceinline__ void sweep_or_filter_row(oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* from, float* out, unsigned frames, unsigned lane,
                                                    bool add, float* rows)
{
    // (the same in every lane: the whole wavefront goes one way)
    if ((sweep->flags & OALSFX_SWEEP_ACTIVE) != 0 && sweep->done < sweep->frames) sweep_row<C, V>(sweep, rec, from, out, frames, lane, add, rows);
    else filter_row<C, V>(rec, from, out, frames, lane, add, rows);
}

} // namespace

#ifndef OALSFX_SWEEP_BODY_ONLY
// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_sweep_resources.py)
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_sweep_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                              oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps, const FirTables tables, float* dst,
                                                              float* scratch, int instances, int lanes, unsigned frames)
{
    biquad_rows<C, V, false, true>(records, envelopes, resamplers, filters, nullptr, sweeps, tables, dst, scratch, instances, lanes, frames);
}

// k_sweep_rows while a voice's queue may hold a segment (include/oalsfx_hip.h, "envelope programs")
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_sweep_program_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                      oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps, EnvProgram* programs,
                                                                      const FirTables tables, float* dst, float* scratch, int instances, int lanes, unsigned frames)
{
    biquad_rows<C, V, true, true>(records, envelopes, resamplers, filters, programs, sweeps, tables, dst, scratch, instances, lanes, frames);
}

// The rows oalsfx_batch_set_sweeps has written since the last render (and those a filter set has cancelled), put in place in front of
// it: a thread per 16-byte piece.
__global__ __launch_bounds__(256) void k_sweep_upload(oalsfx_filter_sweep* sweeps, const int* __restrict__ index, const oalsfx_filter_sweep* __restrict__ changed,
                                                      int count)
{
    constexpr unsigned kPieces = sizeof(oalsfx_filter_sweep) / 16;
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned k = g / kPieces, piece = g % kPieces;
    if (k >= static_cast<unsigned>(count)) return;
    const uint32_t* const from = reinterpret_cast<const uint32_t*>(changed + k) + piece * 4U;
    uint32_t* const to = reinterpret_cast<uint32_t*>(sweeps + index[k]) + piece * 4U;
#pragma unroll
    for (int i = 0; i < 4; ++i) to[i] = from[i];
}

bool launch_sweep(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                  const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_sweep_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters, sweeps, tables,
                           dst, scratch, instances, lanes, frames);
    });
}

bool launch_program_sweep(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                          EnvProgram* programs, const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch,
                          hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_sweep_program_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters,
                           sweeps, programs, tables, dst, scratch, instances, lanes, frames);
    });
}

void launch_sweep_upload(oalsfx_filter_sweep* sweeps, const int* index, const oalsfx_filter_sweep* changed, int count, hipStream_t stream)
{
    constexpr unsigned kPieces = sizeof(oalsfx_filter_sweep) / 16;
    const unsigned threads = static_cast<unsigned>(count) * kPieces;
    hipLaunchKernelGGL(k_sweep_upload, dim3((threads + 255U) / 256U), dim3(256), 0, stream, sweeps, index, changed, count);
}
#endif // OALSFX_SWEEP_BODY_ONLY

} // namespace oalsfx_hip
