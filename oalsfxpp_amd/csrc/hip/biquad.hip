// Voice filters: a biquad per voice, run before the voices of an instance are summed (include/oalsfx_hip.h, "voice filters").  For a
// voice whose filter is ACTIVE, y_f = ((((b0 * x_f) + (b1 * x_(f-1))) + (b2 * x_(f-2))) - (a1 * y_(f-1))) - (a2 * y_(f-2)) over every
// frame of the render, x_f what the voice renders by itself, every operation rounded by itself; y_f stands where the voice's own value
// stood: stored at one lane, added in ascending lanes at two or more.
//
// The shape is k_mix_rows': one wavefront per INSTANCE, the instance number in a scalar register, four instances to a workgroup, the
// three flag words of every voice read in front of the first store.  A busy voice without an ACTIVE filter runs the row body k_mix_rows
// runs (AddSink; at one lane StoreSink, k_fir_rows' bits).  A voice with one is rendered with StoreSink, untouched row body and all, into
// the instance's own scratch row -- [frames][C] of a buffer the batch owns -- and then filtered from there in tiles of 64 frames:
//   1. lane = frame: the lane loads its frame, takes x_(f-1) and x_(f-2) from its neighbours with a cross-lane move (lanes 0 and 1:
//      from the history carried from the tile before, the same in every lane), and writes u = ((b0 x) + (b1 x1)) + (b2 x2) into row c of
//      the wavefront's LDS block, C rows of 4 + 64 floats;
//   2. lane = channel, c < C: the recurrence y = (u - a1 y1) - a2 y2 over its row, in 16-sample register blocks
//      (filter_recurrence.hpp, which k_send_filters runs as well); y1 and y2 stay in the lane's registers from the first tile to the last;
//   3. lane = frame: the lane reads its C outputs and stores them, or adds them to the row with add_frame.  It is lane (f mod 64), the
//      owner of that frame from the zero fill to the last voice, so k_mix_rows' ownership rule still carries the sum.
// Behind the last tile the lanes c < C write their channel's four history floats.
//
// Ordering is wavefront-scope only: a release fence, a wave barrier and an acquire fence (k_send_filters' wave_sync) between the render
// and the first read of the scratch row (a delayed voice's frames are stored by other lanes than read them), between the phases of a
// tile, and between the last read of the scratch row and the next voice's render into it.  There is NO workgroup barrier anywhere, and
// there must not be: the four wavefronts of a workgroup run different instances with different voices.
// sweep.hip includes this file with OALSFX_BIQUAD_BODY_ONLY set, for the stage and the render around it without the kernels: its swept
// voices run a stage of their own (sweep_row) where the others run filter_row.  filter_program.hip includes sweep.hip in the same way:
// a voice whose filter program's queue holds a segment runs filter_program_row.
#include "biquad.hpp"
#include "filter_program.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "program_rows_body.hpp"
#include "stream_rows_body.hpp"
#include "filter_recurrence.hpp"

namespace oalsfx_hip {

namespace {

// The filter stage is written as per-lane phase functions between the wavefront's syncs.  On the device a thread is a lane, runs every
// phase once, and what a lane holds across phases is a register.  Compiled for the host (tests/cpp/biquad_rows_host.cpp) the kernel
// runs once per wavefront, OALSFX_EACH_LANE runs a phase -- or a whole stretch of zero fill and renders -- over the 64 lanes one after
// the other, lane 0 last (it writes the records back), and what a lane holds is its entry of an array; a value of another lane, which
// the device moves across lanes, is read there.
#ifdef OALSFX_FIR_HOST_SHIM
constexpr int kHeld = kWave;
#define OALSFX_EACH_LANE(l, mine) for (unsigned l = kWave; l-- > 0;)
inline unsigned held(unsigned l) { return l; }
inline void wave_sync() {}
#else
constexpr int kHeld = 1;
#define OALSFX_EACH_LANE(l, mine) for (unsigned l = (mine), once_ = 1U; once_ != 0U; once_ = 0U)
__device__ __forceinline__ unsigned held(unsigned) { return 0U; }
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

// what the lanes hold from one phase of the filter stage to the next
template <int C>
struct FilterLanes {
    float x[kHeld][C];         // lane = frame: the tile's frame
    float y1[kHeld], y2[kHeld]; // lane = channel, c < C: the outputs of channel c in front of the tile
};

// channel c of the frame `delta` lanes below lane l (lanes below delta: not looked at)
template <int C>
__device__ __forceinline__ float below(const FilterLanes<C>& s, int c, unsigned l, unsigned delta)
{
#ifdef OALSFX_FIR_HOST_SHIM
    return l >= delta ? s.x[l - delta][c] : 0.0F;
#else
    return __shfl_up(s.x[0][c], delta);
#endif
}

// channel c of lane `from`'s frame, the same in every lane (`from` is)
template <int C>
__device__ __forceinline__ float of_lane(const FilterLanes<C>& s, int c, unsigned from)
{
#ifdef OALSFX_FIR_HOST_SHIM
    return s.x[from][c];
#else
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.x[0][c]), static_cast<int>(from)));
#endif
}

// the frame at `at`, in the pieces store_frame writes it in
template <int C, int V>
__device__ __forceinline__ void load_frame(const float* at, float (&x)[C])
{
#ifndef OALSFX_FIR_HOST_SHIM
    typedef typename Vec<V>::type vec;
#pragma unroll
    for (int j = 0; j < C / V; ++j) {
        const vec v = reinterpret_cast<const vec*>(at)[j];
        if constexpr (V == 1) x[j] = v;
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) x[j * V + i] = v[i];
        }
    }
#else
    for (int c = 0; c < C; ++c) x[c] = at[c];
#endif
}

// ---- phase 1a, lane = frame: the lane's frame of the tile at `base`, L frames long (+0.0f beyond it) ----
template <int C, int V>
__device__ __forceinline__ void load_phase(FilterLanes<C>& s, unsigned l, const float* from, unsigned base, unsigned L)
{
#pragma unroll
    for (int c = 0; c < C; ++c) s.x[held(l)][c] = 0.0F;
    if (l < L) load_frame<C, V>(from + static_cast<size_t>(base + l) * C, s.x[held(l)]);
}

// ---- phase 1b, lane = frame: u = ((b0 x) + (b1 x1)) + (b2 x2) into row c; lanes 0 and 1 take x1, x2 from the carried history ----
template <int C>
__device__ __forceinline__ void feed_phase(const FilterLanes<C>& s, unsigned l, float b0, float b1, float b2, const float (&xh1)[C], const float (&xh2)[C], float* rows)
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float up1 = below(s, c, l, 1U), up2 = below(s, c, l, 2U);
        const float x1 = l >= 1U ? up1 : xh1[c];
        const float x2 = l >= 2U ? up2 : l == 1U ? xh1[c] : xh2[c];
        rows[c * kFilterRow + 4 + l] = ((b0 * s.x[held(l)][c]) + (b1 * x1)) + (b2 * x2);
    }
}

// ---- phase 2, lane = channel: the recurrence over the lane's row ----
template <int C>
__device__ __forceinline__ void recur_phase(FilterLanes<C>& s, unsigned l, unsigned L, float a1, float a2, float* rows)
{
    if (l < C) filter_recurrence(rows + l * kFilterRow, static_cast<int>(L), a1, a2, s.y1[held(l)], s.y2[held(l)]);
}

// ---- phase 3, lane = frame: the lane's C outputs stored, or added to the row ----
template <int C, int V>
__device__ __forceinline__ void out_phase(unsigned l, unsigned base, unsigned L, const float* rows, float* out, bool add)
{
    if (l >= L) return;
    float y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = rows[c * kFilterRow + 4 + l];
    float* const at = out + static_cast<size_t>(base + l) * C;
    if (add) add_frame<C, V>(at, y);
    else store_frame<C, V>(at, y);
}

// The voice's `frames` frames in `from`, [frames][C], through its filter into the row `out`: stored, or with `add` added.  *rec is the
// same in every lane; rows: the wavefront's C LDS rows.  The histories in *rec afterwards are those of the render's last two frames.
template <int C, int V>
__device__ __forceinline__ void filter_row(oalsfx_voice_filter* rec, const float* from, float* out, unsigned frames, unsigned lane, bool add, float* rows)
{
    const float b0 = rec->b0, b1 = rec->b1, b2 = rec->b2, a1 = rec->a1, a2 = rec->a2;
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
        OALSFX_EACH_LANE(l, lane) load_phase<C, V>(s, l, from, base, L);
        OALSFX_EACH_LANE(l, lane) feed_phase<C>(s, l, b0, b1, b2, xh1, xh2, rows);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float last = of_lane(s, c, L - 1U), before = of_lane(s, c, L >= 2U ? L - 2U : 0U);
            xh2[c] = L >= 2U ? before : xh1[c];
            xh1[c] = last;
        }
        wave_sync();
        OALSFX_EACH_LANE(l, lane) recur_phase<C>(s, l, L, a1, a2, rows);
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
}

static_assert(sizeof(oalsfx_voice_filter) == 160 && offsetof(oalsfx_voice_filter, b0) == 8 && offsetof(oalsfx_voice_filter, x) == 32 &&
              offsetof(oalsfx_voice_filter, y) == 96, "the layout the filter stage reads and writes");

// The filter stage of a voice in a launch that looks at the sweeps (sweep.hip): sweep_row while the voice's sweep is under way,
// filter_row otherwise.  rows: the wavefront's C + 2 LDS rows.
template <int C, int V>
__device__ __forceinline__ void sweep_or_filter_row(oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* from, float* out, unsigned frames, unsigned lane,
                                                    bool add, float* rows);

// The filter stage of a voice in a launch that looks at the filter programs' queues as well (filter_program.hip): filter_program_row while
// the voice's queue holds a segment, sweep_or_filter_row otherwise.
template <int C, int V>
__device__ __forceinline__ void queued_or_sweep_row(FilterProgram* queue, oalsfx_filter_sweep* sweep, oalsfx_voice_filter* rec, const float* from, float* out,
                                                    unsigned frames, unsigned lane, bool add, float* rows);

// Workgroup g, wavefront w: instance g * kRows + w.  C channels, V floats per access (C % V == 0, dst and scratch aligned to V floats).
// PROGRAM: a voice's render is program_row's, which walks the voice's queue in `programs` (program_rows_body.hpp), not voice_row's; the
// filter stage behind it sees the voice's whole row either way.  Not PROGRAM: `programs` is not looked at.  SWEEP: a filtered voice's
// stage looks at the voice's row of `sweeps` first, and the wavefront has two more LDS rows; not SWEEP: `sweeps` is not looked at.
// QUEUED (with SWEEP): the stage looks at the voice's row of `queues`, its filter program's queue, in front of that; not QUEUED: `queues`
// is not looked at.  STREAM (with PROGRAM, SWEEP and QUEUED: stream.hip's k_stream_filter_rows): a voice's render is stream_row's, which
// walks the voice's ring in `rings` with its count in `taken` beside the queue in `programs` (stream_rows_body.hpp), a voice whose ring
// holds an entry is rendered whatever its record says, and `programs` and `queues` may be null: a table that was never made counts
// as empty queues.
template <int C, int V, bool PROGRAM, bool SWEEP, bool QUEUED = false, bool STREAM = false>
__device__ __forceinline__ void biquad_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers, oalsfx_voice_filter* filters,
                                            EnvProgram* programs, oalsfx_filter_sweep* sweeps, const FirTables& tables, float* dst, float* scratch, int instances,
                                            int lanes, unsigned frames, FilterProgram* queues = nullptr, const StreamRing* rings = nullptr, uint32_t* taken = nullptr)
{
    static_assert(SWEEP || !QUEUED, "the queues hold sweeps");
    static_assert(!STREAM || (PROGRAM && QUEUED), "the streams' render is the most general one");
    constexpr int kLdsRows = SWEEP ? C + 2 : C;
#ifdef OALSFX_FIR_HOST_SHIM
    if (threadIdx.x % kWave != 0) return; // (the host runs a wavefront in one call)
    static float filter_rows[kRows][kLdsRows * kFilterRow] __attribute__((aligned(16)));
#else
    __shared__ __attribute__((aligned(16))) float filter_rows[kRows][kLdsRows * kFilterRow];
#endif
    const int wave = static_cast<int>(threadIdx.x) / kWave;
    const int instance = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + wave);
    if (instance >= instances) return; // whole wavefronts leave; no workgroup barrier in this kernel
    const unsigned lane = threadIdx.x % kWave;
    float* const out = dst + static_cast<size_t>(instance) * frames * C;
    float* const own = scratch + static_cast<size_t>(instance) * frames * C;
    float* const rows = filter_rows[__builtin_amdgcn_readfirstlane(wave)];
    // the three flag words of every lane, read in front of the kernel's first store: scalar loads, all in flight together
    uint32_t busy = 0, filtered = 0;
#pragma unroll
    for (int k = 0; k < OALSFX_MAX_POLYPHONY; ++k) {
        if (k < lanes) {
            const size_t row = static_cast<size_t>(k) * instances + instance;
            const uint32_t flags = records[row].flags & OALSFX_SAMPLER_PLAYING, eflags = envelopes[row].flags & OALSFX_ENV_ACTIVE;
            const uint32_t fflags = filters[row].flags & OALSFX_VF_ACTIVE;
            if constexpr (STREAM) busy |= rings[row].queued != taken[row] ? 1U << k : 0U;
            busy |= (flags | eflags | fflags) != 0 ? 1U << k : 0U;
            filtered |= fflags != 0 ? 1U << k : 0U;
        }
    }
    const bool add = lanes >= 2;
    // The voices in stretches that end behind the render of a filtered voice: a lane runs a whole stretch -- the zero fill in front of
    // the first, the renders and sums of its voices -- by itself, and the lanes meet only for the filter stage behind it.
    for (int first = 0; first < lanes;) {
        int stop = first; // the stretch's last voice: the next filtered one, or the last lane
        while (stop < lanes - 1 && !(filtered >> stop & 1U)) ++stop;
        OALSFX_EACH_LANE(l, lane) {
            // (at one lane a voice's frames are stored: by its render, by its filter, or, where it is idle, here)
            if (first == 0 && (add || busy == 0)) {
                unsigned filler = l; // (opaque for the reason given below: 125 VGPRs at seven channels instead of 129)
#ifndef OALSFX_FIR_HOST_SHIM
                asm volatile("" : "+v"(filler));
#endif
                store_zeros<C, V>(out, 0U, frames, filler);
            }
            for (int k = first; k <= stop; ++k) {
                if (!(busy >> k & 1U)) continue;
                const size_t row = static_cast<size_t>(k) * instances + instance;
                const bool through = (filtered >> k & 1U) != 0;
                // (the lane number made opaque once per voice: what the render and the filter compute from it alone -- addresses, masks --
                // would otherwise be taken out of this loop and held in registers across the whole row body: 141 VGPRs at seven channels
                // instead of 125)
                unsigned mine = l;
#ifndef OALSFX_FIR_HOST_SHIM
                asm volatile("" : "+v"(mine));
#endif
                if constexpr (STREAM) {
                    EnvProgram* const prog = programs ? programs + row : nullptr;
                    if (through || !add) stream_row<C, V, StoreSink, true>(records + row, envelopes + row, prog, rings + row, taken + row, resamplers[row], tables, through ? own : out, frames, mine);
                    else stream_row<C, V, AddSink, true>(records + row, envelopes + row, prog, rings + row, taken + row, resamplers[row], tables, out, frames, mine);
                } else if constexpr (PROGRAM) {
                    if (through || !add) program_row<C, V, StoreSink, true>(records + row, envelopes + row, programs + row, resamplers[row], tables, through ? own : out, frames, mine);
                    else program_row<C, V, AddSink, true>(records + row, envelopes + row, programs + row, resamplers[row], tables, out, frames, mine);
                } else {
                    if (through || !add) voice_row<C, V, StoreSink>(records + row, envelopes + row, resamplers[row], tables, through ? own : out, frames, mine);
                    else voice_row<C, V, AddSink>(records + row, envelopes + row, resamplers[row], tables, out, frames, mine);
                }
            }
        }
        if (filtered >> stop & 1U) {
            wave_sync(); // the scratch row is written
            unsigned mine = lane;
#ifndef OALSFX_FIR_HOST_SHIM
            asm volatile("" : "+v"(mine));
#endif
            const size_t row = static_cast<size_t>(stop) * instances + instance;
            if constexpr (STREAM) {
                // (the same in every lane: the whole wavefront goes one way)
                if (queues) queued_or_sweep_row<C, V>(queues + row, sweeps + row, filters + row, own, out, frames, mine, add, rows);
                else sweep_or_filter_row<C, V>(sweeps + row, filters + row, own, out, frames, mine, add, rows);
            } else if constexpr (QUEUED) queued_or_sweep_row<C, V>(queues + row, sweeps + row, filters + row, own, out, frames, mine, add, rows);
            else if constexpr (SWEEP) sweep_or_filter_row<C, V>(sweeps + row, filters + row, own, out, frames, mine, add, rows);
            else filter_row<C, V>(filters + row, own, out, frames, mine, add, rows);
        }
        first = stop + 1;
    }
}

} // namespace

#ifndef OALSFX_BIQUAD_BODY_ONLY
// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_biquad_resources.py,
// tests/test_program_resources.py)
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_biquad_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                               oalsfx_voice_filter* filters, const FirTables tables, float* dst, float* scratch, int instances,
                                                               int lanes, unsigned frames)
{
    biquad_rows<C, V, false, false>(records, envelopes, resamplers, filters, nullptr, nullptr, tables, dst, scratch, instances, lanes, frames);
}

// k_biquad_rows while a voice's queue may hold a segment (include/oalsfx_hip.h, "envelope programs")
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_program_biquad_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                       oalsfx_voice_filter* filters, EnvProgram* programs, const FirTables tables, float* dst,
                                                                       float* scratch, int instances, int lanes, unsigned frames)
{
    biquad_rows<C, V, true, false>(records, envelopes, resamplers, filters, programs, nullptr, tables, dst, scratch, instances, lanes, frames);
}

// The rows oalsfx_batch_set_filters has written since the last render, put in place in front of it: flags and coefficients always, the
// histories where the row says LOAD, which the device's copy never shows.
__global__ __launch_bounds__(256) void k_biquad_upload(oalsfx_voice_filter* filters, const int* __restrict__ index, const oalsfx_voice_filter* __restrict__ changed,
                                                       int count)
{
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= count) return;
    const oalsfx_voice_filter& from = changed[k];
    oalsfx_voice_filter& to = filters[index[k]];
    const uint32_t flags = from.flags;
    to.flags = flags & ~static_cast<uint32_t>(OALSFX_VF_LOAD);
    to.reserved0 = 0U;
    to.b0 = from.b0;
    to.b1 = from.b1;
    to.b2 = from.b2;
    to.a1 = from.a1;
    to.a2 = from.a2;
    to.reserved1 = 0.0F;
    if (!(flags & OALSFX_VF_LOAD)) return;
#pragma unroll
    for (int c = 0; c < OALSFX_MAX_CHANNELS; ++c) {
        to.x[c][0] = from.x[c][0];
        to.x[c][1] = from.x[c][1];
        to.y[c][0] = from.y[c][0];
        to.y[c][1] = from.y[c][1];
    }
}

bool launch_biquad(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, const FirTables& tables,
                   int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_biquad_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters, tables, dst,
                           scratch, instances, lanes, frames);
    });
}

bool launch_program_biquad(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, EnvProgram* programs,
                           const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_program_biquad_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters,
                           programs, tables, dst, scratch, instances, lanes, frames);
    });
}

void launch_biquad_upload(oalsfx_voice_filter* filters, const int* index, const oalsfx_voice_filter* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_biquad_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, filters, index, changed, count);
}
#endif // OALSFX_BIQUAD_BODY_ONLY

} // namespace oalsfx_hip
