// The row body of the voices' renders: one voice -- a sampler's record, an envelope and, where the kernel has them, a table index --
// rendered by one wavefront, in the arithmetic include/oalsfx_hip.h states ("samplers", "voice envelopes", "resamplers"), bit for bit.
// This is the only place that arithmetic is written down.  Three files compile it: voice.hip (k_voice_rows: no tables, TABLED off, so
// that no table is looked up and the FIR bodies are not instantiated), resample.hip (k_fir_rows: a voice per instance, its frames
// stored) and polyphony.hip (k_mix_rows: several voices per instance, their frames added into the instance's row); the last two differ
// in the sink alone, a template parameter.  A row without a table gets the same bits from all three.
//
// The shape: the row's fields are the same in every lane (the caller forms the row number through readfirstlane, so both records, the
// table index and the table's descriptor are scalar loads and every branch on them is wave-uniform); lane l owns the frames l, l + 64,
// ...; the tile's base is wrapped once per tile; a frame's channels go out as one access where the address allows.  A lane issues the
// asset loads of up to 16 taps (32 values) before the first conversion: several frames where a frame's taps are few, one frame's taps
// in two runs of ascending k where a wide asset at 8 taps would be 64 values.  A tap outside the asset or behind a one-shot's end is
// never loaded: it is steered to element 0 and its value replaced by +0.0f, which the sum absorbs (finite coefficients: +0.0f + c *
// +0.0f is +0.0f whatever c's sign).  A lane's coefficient row is 4 or 8 contiguous floats, 16- or 32-byte aligned.  No LDS, no
// cross-lane operation, no atomics, no barrier: the body also compiles for the host, the lanes run one after the other
// (tests/cpp/fir_rows_host.cpp, tests/cpp/mix_rows_host.cpp).  What the samplers' kernel needs as well -- the stores, the conversions,
// the wrap, the launch -- is row_kernels.hpp.
//
// The including file sets `#pragma clang fp contract(off)` in front of the include.
#ifndef OALSFX_HIP_VOICE_ROWS_BODY_HPP
#define OALSFX_HIP_VOICE_ROWS_BODY_HPP

#include "resample.hpp"
#include "row_kernels.hpp"

#include <cstddef>
#include <cstdint>

namespace oalsfx_hip {

namespace {

constexpr int kFrac = OALSFX_SAMPLER_FRAC_BITS;
constexpr int kSub = OALSFX_ENV_SUB_BITS;
constexpr int kFine = kFrac + kSub;        // fractional bits of PHI

// at[c] = at[c] + x[c], each sum rounded by itself: the frame is read and written back in the pieces store_frame writes it in
template <int C, int V>
__device__ __forceinline__ void add_frame(float* at, const float (&x)[C])
{
#ifndef OALSFX_FIR_HOST_SHIM
    typedef typename Vec<V>::type vec;
    vec held[C / V];
#pragma unroll
    for (int j = 0; j < C / V; ++j) held[j] = reinterpret_cast<const vec*>(at)[j];
#pragma unroll
    for (int j = 0; j < C / V; ++j) {
        vec v = held[j];
        if constexpr (V == 1) v = v + x[j];
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = v[i] + x[j * V + i];
        }
        reinterpret_cast<vec*>(at)[j] = v;
    }
#else
    for (int c = 0; c < C; ++c) at[c] = at[c] + x[c];
#endif
}

// Where a voice's frames go.  StoreSink: the row is the voice's own, every frame of the call is written, silent ones as +0.0f.
// AddSink: the row holds the sum of the voices in front of this one (+0.0f in front of the first) and a frame is added to it; a silent
// frame is left out, which gives the same bits (the sum is never -0.0f, and x + +0.0f is x for every other x).  A frame is read and
// written by the lane that owns it and by no other, so a lane's program order is all the ordering the sum needs.
struct StoreSink {
    static constexpr bool kAdds = false;
    template <int C, int V> static __device__ __forceinline__ void put(float* at, const float (&x)[C]) { store_frame<C, V>(at, x); }
};
struct AddSink {
    static constexpr bool kAdds = true;
    template <int C, int V> static __device__ __forceinline__ void put(float* at, const float (&x)[C]) { add_frame<C, V>(at, x); }
};

// frames of one lane whose loads are issued together, for rows without a table: 8 up to stereo, 4 from quad up, and 3 at eight channels
// in a kernel that has tables (TABLED), where the table's descriptor and the FIR bodies beside this one would take the kernel past 128
// VGPRs with 4 -- the bits do not depend on it
template <int C, bool TABLED> struct Ahead { static constexpr int value = C <= 2 ? 8 : C < 8 || !TABLED ? 4 : 3; };
// ... rows with one: at most 16 taps and 32 values in flight.  K asset channels, TAPS taps: `ahead` frames at once, a frame's taps in runs
// of `run`
template <int TAPS, int K, class Sink> struct Fan {
    static constexpr int taps_in_flight = K <= 2 ? 16 : K <= 4 ? 8 : 4;
    static constexpr int ahead = taps_in_flight / TAPS >= 1 ? taps_in_flight / TAPS : 1;
    static constexpr int run = TAPS < taps_in_flight ? TAPS : taps_in_flight;
    static_assert(TAPS % run == 0, "whole runs");
};

// One row, the same in every lane.  Positions are PHI: kFine fractional bits.
struct Voice {
    uint64_t phi;                   // of the first frame rendered
    uint64_t E, L0, L1;             // asset end, loop region
    uint64_t sigma, sigma_to;       // step << 16; step_to << 16 (without a glide: step << 16 as well)
    int64_t slope;
    uint32_t g, G;                  // glide index of the first frame rendered, glide length (without a glide: 0, 0)
    uint32_t n, R;                  // ramp index of the first frame rendered, ramp length
    uint32_t frames, loop_start, loop_end;
    bool loop, linear, env;
};

// What a render changes in a voice's two records: the sampler's position, step and flags, the envelope's counters and sub.
struct Carried {
    uint64_t position;
    uint32_t step, flags;
    uint32_t delay, ramp_done, glide_done, sub;
};

// PHI's advance over the m frames from glide index g on, m no more than a tile: sum of S_(g + j), j < m.  Modular in 64 bits (a negative
// slope is its two's complement); the sum itself is below 2^58.
__device__ __forceinline__ uint64_t advance(const Voice& v, uint32_t g, uint32_t m)
{
    const uint32_t left = v.G - g; // g <= G
    const uint32_t in = m < left ? m : left;
    const uint32_t pairs = in * (in - 1U) / 2U;
    const uint64_t sg = v.sigma + g * static_cast<uint64_t>(v.slope);
    return in * sg + pairs * static_cast<uint64_t>(v.slope) + (m - in) * v.sigma_to;
}

// The tile's base behind its m frames: wrapped into the loop, or held at a one-shot's end once it has got there.
__device__ __forceinline__ uint64_t next_base(const Voice& r, uint64_t base, uint32_t g, uint32_t m, uint64_t len)
{
    base += advance(r, g, m);
    if (r.loop) {
        if (base >= r.L1) base = wrap_past(base, r.L0, r.L1, len);
    } else if (base > r.E) {
        base = r.E; // ended: every later frame is past the end as well
    }
    return base;
}

// out = (v * gain) * e: the sampler's product first, then the envelope's factor at ramp index n + f.
template <int C, bool MONO>
__device__ __forceinline__ void finish(const Voice& r, const float (&v)[MONO ? 1 : C], unsigned f, const float (&gain)[C], const float (&from)[C],
                                       const float (&step)[C], const float (&to)[C], float (&o)[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = v[MONO ? 0 : c] * gain[c];
    if (r.env) {
        const uint32_t n = r.n + f;
        const float nf = static_cast<float>(n); // exact: used only where n < R <= 2^24
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = o[c] * (n < r.R ? from[c] + (nf * step[c]) : to[c]);
    }
}

// The frames [0, F) of one playing row without a table, F >= 1.  Returns PHI behind them, wrapped (a one-shot's: E once it has ended).
// T: the asset's element; MONO: one asset channel for every output channel, else C.  `lane`: which frames are this lane's -- lane,
// lane + 64, ...
template <int C, int V, typename T, bool MONO, class Sink, bool TABLED>
__device__ __forceinline__ uint64_t render_plain(const T* __restrict__ data, const Voice& r, const float (&gain)[C], const float (&from)[C],
                                                 const float (&step)[C], const float (&to)[C], float* __restrict__ out, unsigned F, unsigned lane)
{
    constexpr int K = MONO ? 1 : C;
    constexpr int kAhead = Ahead<C, TABLED>::value;
    constexpr unsigned kTile = kWave * kAhead;
    const uint64_t len = r.L1 - r.L0;
    uint64_t base = r.phi; // of the tile's first frame, wrapped: the same in every lane
    uint32_t g = r.g;
    if (r.loop && base >= r.L1) base = wrap_past(base, r.L0, r.L1, len);
    for (unsigned f0 = 0; f0 < F; f0 += kTile) {
        T a[kAhead][K], b[kAhead][K];
        unsigned mu_bits[kAhead];
        bool live[kAhead], b_silent[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned in_tile = lane + k * kWave;
            uint64_t q = base + advance(r, g, in_tile);
            if (r.loop && q >= r.L1) q = wrap_past(q, r.L0, r.L1, len);
            mu_bits[k] = static_cast<unsigned>(q >> kSub) & ((1U << kFrac) - 1U);
            // (a frame beyond the call's or past the asset's end reads element 0 and takes no part)
            live[k] = f0 + in_tile < F && (r.loop || q < r.E);
            const uint32_t i = live[k] ? static_cast<uint32_t>(q >> kFine) : 0U;
            uint32_t j = i + 1U;
            b_silent[k] = false;
            if (r.loop) {
                if (j == r.loop_end) j = r.loop_start;
            } else if (j == r.frames) {
                j = i;
                b_silent[k] = true; // a one-shot interpolates into silence
            }
#pragma unroll
            for (int c = 0; c < K; ++c) a[k][c] = data[static_cast<size_t>(i) * K + c];
            if (r.linear) {
#pragma unroll
                for (int c = 0; c < K; ++c) b[k][c] = data[static_cast<size_t>(j) * K + c];
            } else {
#pragma unroll
                for (int c = 0; c < K; ++c) b[k][c] = a[k][c];
            }
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned f = f0 + lane + k * kWave;
            if (f >= F) continue;
            float o[C];
            if (live[k]) {
                const float mu = static_cast<float>(mu_bits[k]) * (1.0F / static_cast<float>(1 << kFrac));
                float v[K];
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const float av = to_float(a[k][c]);
                    const float bv = b_silent[k] ? 0.0F : to_float(b[k][c]);
                    v[c] = r.linear ? av + ((bv - av) * mu) : av; // the reference's Math::lerp (src/oalsfxpp.cpp:180-186)
                }
                finish<C, MONO>(r, v, f, gain, from, step, to, o);
            } else {
                if constexpr (Sink::kAdds) continue;
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = 0.0F;
            }
            Sink::template put<C, V>(out + static_cast<size_t>(f) * C, o);
        }
        const uint32_t m = F - f0 < kTile ? F - f0 : kTile;
        base = next_base(r, base, g, m, len);
        g = r.G - g < m ? r.G : g + m;
    }
    return base;
}

// Which frame tap `offset` frames from frame i reads, i a live frame's: false where the tap lies in front of the asset or behind a
// one-shot's end (`at` is then 0: element 0 is loaded and discarded); a looping voice's tap at or past loop_end goes round the loop, as
// often as a loop shorter than the filter's half needs.
__device__ __forceinline__ bool tap_frame(const Voice& r, bool live, uint32_t i, int offset, uint32_t& at)
{
    const int64_t j = static_cast<int64_t>(i) + offset;
    at = 0U;
    if (!live || j < 0) return false;
    if (r.loop) {
        if (j >= static_cast<int64_t>(r.loop_end)) {
            const uint32_t len = r.loop_end - r.loop_start;
            uint32_t past = static_cast<uint32_t>(j - static_cast<int64_t>(r.loop_end)); // at most TAPS / 2
            if (past >= len) past %= len;
            at = r.loop_start + past;
        } else {
            at = static_cast<uint32_t>(j);
        }
        return true;
    }
    if (j >= static_cast<int64_t>(r.frames)) return false;
    at = static_cast<uint32_t>(j);
    return true;
}

// The frames [0, F) of one playing row with a table of TAPS taps, coef[phase][TAPS], phase = a position's 12 fractional bits >> shift.
template <int C, int V, typename T, bool MONO, int TAPS, class Sink>
__device__ __forceinline__ uint64_t render_fir(const T* __restrict__ data, const Voice& r, const float* __restrict__ coef, int shift, const float (&gain)[C],
                                               const float (&from)[C], const float (&step)[C], const float (&to)[C], float* __restrict__ out, unsigned F,
                                               unsigned lane)
{
    constexpr int K = MONO ? 1 : C;
    constexpr int H = TAPS / 2;
    constexpr int kAhead = Fan<TAPS, K, Sink>::ahead;
    constexpr int kRun = Fan<TAPS, K, Sink>::run;
    constexpr unsigned kTile = kWave * kAhead;
    const uint64_t len = r.L1 - r.L0;
    uint64_t base = r.phi; // of the tile's first frame, wrapped: the same in every lane
    uint32_t g = r.g;
    if (r.loop && base >= r.L1) base = wrap_past(base, r.L0, r.L1, len);
    for (unsigned f0 = 0; f0 < F; f0 += kTile) {
        float cf[kAhead][TAPS], v[kAhead][K];
        uint32_t first[kAhead];
        bool live[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned in_tile = lane + k * kWave;
            uint64_t q = base + advance(r, g, in_tile);
            if (r.loop && q >= r.L1) q = wrap_past(q, r.L0, r.L1, len);
            // (a frame beyond the call's or past the asset's end loads element 0, TAPS times, and takes no part)
            live[k] = f0 + in_tile < F && (r.loop || q < r.E);
            first[k] = live[k] ? static_cast<uint32_t>(q >> kFine) : 0U;
            const unsigned phase = (static_cast<unsigned>(q >> kSub) & ((1U << kFrac) - 1U)) >> shift; // below the table's phase count
            const float* const row = static_cast<const float*>(__builtin_assume_aligned(coef + static_cast<size_t>(phase) * TAPS, 16));
#pragma unroll
            for (int t = 0; t < TAPS; ++t) cf[k][t] = row[t];
#pragma unroll
            for (int c = 0; c < K; ++c) v[k][c] = 0.0F;
        }
#pragma unroll
        for (int t0 = 0; t0 < TAPS; t0 += kRun) {
            T x[kAhead][kRun][K];
            bool in_range[kAhead][kRun];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
#pragma unroll
                for (int t = 0; t < kRun; ++t) {
                    uint32_t at;
                    in_range[k][t] = tap_frame(r, live[k], first[k], t0 + t - (H - 1), at);
#pragma unroll
                    for (int c = 0; c < K; ++c) x[k][t][c] = data[static_cast<size_t>(at) * K + c];
                }
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
#pragma unroll
                for (int t = 0; t < kRun; ++t) {
#pragma unroll
                    for (int c = 0; c < K; ++c) v[k][c] = v[k][c] + (cf[k][t0 + t] * (in_range[k][t] ? to_float(x[k][t][c]) : 0.0F));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned f = f0 + lane + k * kWave;
            if (f >= F) continue;
            float o[C];
            if (live[k]) {
                finish<C, MONO>(r, v[k], f, gain, from, step, to, o);
            } else {
                if constexpr (Sink::kAdds) continue;
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = 0.0F;
            }
            Sink::template put<C, V>(out + static_cast<size_t>(f) * C, o);
        }
        const uint32_t m = F - f0 < kTile ? F - f0 : kTile;
        base = next_base(r, base, g, m, len);
        g = r.G - g < m ? r.G : g + m;
    }
    return base;
}

// Where a render leaves what it has changed: in the voice's two records, or in a caller's Carried.
struct IntoRecords {
    oalsfx_sampler* rec;
    oalsfx_envelope* env;
    __device__ __forceinline__ void position(uint64_t v) const { rec->position = v; }
    __device__ __forceinline__ void step(uint32_t v) const { rec->step = v; }
    __device__ __forceinline__ void flags(uint32_t v) const { rec->flags = v; }
    __device__ __forceinline__ void sub(uint32_t v) const { env->sub = v; }
    __device__ __forceinline__ void delay(uint32_t v) const { env->delay = v; }
    __device__ __forceinline__ void ramp_done(uint32_t v) const { env->ramp_done = v; }
    __device__ __forceinline__ void glide_done(uint32_t v) const { env->glide_done = v; }
};
struct IntoCarried {
    Carried* to;
    __device__ __forceinline__ void position(uint64_t v) const { to->position = v; }
    __device__ __forceinline__ void step(uint32_t v) const { to->step = v; }
    __device__ __forceinline__ void flags(uint32_t v) const { to->flags = v; }
    __device__ __forceinline__ void sub(uint32_t v) const { to->sub = v; }
    __device__ __forceinline__ void delay(uint32_t v) const { to->delay = v; }
    __device__ __forceinline__ void ramp_done(uint32_t v) const { to->ramp_done = v; }
    __device__ __forceinline__ void glide_done(uint32_t v) const { to->glide_done = v; }
};

// The records behind a call (voice_row's names): phi is PHI behind the frames advanced.
template <class To>
__device__ __forceinline__ void leave(To to, const oalsfx_sampler* rec, uint32_t flags, bool playing, bool active, bool stop, bool glide, uint32_t advanced, uint32_t shown,
                                      uint64_t phi, uint32_t delay, uint32_t D, uint32_t R, uint32_t n0, uint32_t G, uint32_t g0, uint32_t step_to)
{
    uint32_t flags_after = flags;
    if (playing && advanced != 0) {
        // after the call: PHI behind the frames advanced; a one-shot that has reached its end stops there
        if (!(flags & OALSFX_SAMPLER_LOOP) && phi >= static_cast<uint64_t>(rec->frames) << kFine) {
            phi = static_cast<uint64_t>(rec->frames) << kFine;
            flags_after &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
        }
        to.position(phi >> kSub);
        if (active) to.sub(static_cast<uint32_t>(phi) & ((1U << kSub) - 1U));
    }
    if (active) {
        // the counters run on the frames rendered, playing or not
        const uint32_t ramp_done = R - n0 < shown ? R : n0 + shown;
        to.delay(delay - D);
        to.ramp_done(ramp_done);
        if (stop && ramp_done == R) flags_after &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
        if (glide) {
            const uint32_t glide_done = G - g0 < advanced ? G : g0 + advanced;
            to.glide_done(glide_done);
            if (glide_done == G) to.step(step_to);
        }
    }
    to.flags(flags_after);
}

// taps: 0 without a table, else 4 or 8 -- the same in every lane (not TABLED: 0)
template <int C, int V, typename T, bool MONO, class Sink, bool TABLED>
__device__ __forceinline__ uint64_t render_taps(const T* __restrict__ data, const Voice& r, const float* __restrict__ coef, int taps, int shift,
                                                const float (&gain)[C], const float (&from)[C], const float (&step)[C], const float (&to)[C],
                                                float* __restrict__ out, unsigned F, unsigned lane)
{
    if constexpr (TABLED) {
        if (taps == 4) return render_fir<C, V, T, MONO, 4, Sink>(data, r, coef, shift, gain, from, step, to, out, F, lane);
        if (taps == 8) return render_fir<C, V, T, MONO, 8, Sink>(data, r, coef, shift, gain, from, step, to, out, F, lane);
    }
    return render_plain<C, V, T, MONO, Sink, TABLED>(data, r, gain, from, step, to, out, F, lane);
}

template <int C, int V, typename T, class Sink, bool TABLED>
__device__ __forceinline__ uint64_t render_layout(const void* data, bool mono, const Voice& r, const float* coef, int taps, int shift, const float (&gain)[C],
                                                  const float (&from)[C], const float (&step)[C], const float (&to)[C], float* __restrict__ out, unsigned F,
                                                  unsigned lane)
{
    if constexpr (C == 1) return render_taps<C, V, T, true, Sink, TABLED>(static_cast<const T*>(data), r, coef, taps, shift, gain, from, step, to, out, F, lane);
    else if (mono) return render_taps<C, V, T, true, Sink, TABLED>(static_cast<const T*>(data), r, coef, taps, shift, gain, from, step, to, out, F, lane);
    else return render_taps<C, V, T, false, Sink, TABLED>(static_cast<const T*>(data), r, coef, taps, shift, gain, from, step, to, out, F, lane);
}

// One voice's `frames` frames into the row `out`, [frames][C], and both of its records advanced, by one wavefront: `lane` is the
// caller's lane, and *rec, *env and `table` (a table index or OALSFX_RESAMPLER_NONE) are the same in every lane.  C channels, V floats
// per access (C % V == 0, out aligned to V floats).  Lane 0 writes the records back; no lane reads them afterwards.  Not TABLED: the
// kernel has no tables, `table` and `tables` are not looked at and every row is rendered as one that names none.  CARRIED: what a render
// changes in the two records is read from *carried and left there by every lane, in registers, and neither record is written -- for a
// caller that renders a row in several spans (program_rows_body.hpp); otherwise `carried` is not looked at.
//
// With StoreSink lane l writes the frames l, l + 64, ... of the whole call, the voice's and the silent ones around them.  With AddSink
// nothing but the voice's own live frames is touched, and they too belong to the lane (f mod 64) whatever the envelope's delay D: the
// render, whose frames count from D on, is given the lane number turned back by D, so that its frame f' = f - D is again lane
// (f mod 64)'s.
template <int C, int V, class Sink, bool TABLED = true, bool CARRIED = false>
__device__ __forceinline__ void voice_row(oalsfx_sampler* rec, oalsfx_envelope* env, int table, const FirTables& tables, float* out, unsigned frames, unsigned lane,
                                          Carried* carried = nullptr)
{
    const bool tabled = TABLED && table >= 0 && table < OALSFX_FIR_TABLES;
    const float* const coef = tabled ? tables.coef[table] : nullptr;
    const int taps = tabled ? tables.taps[table] : 0;
    const int shift = tabled ? tables.shift[table] : 0;
    const uint32_t flags = CARRIED ? carried->flags : rec->flags, eflags = env->flags;
    const bool playing = (flags & OALSFX_SAMPLER_PLAYING) != 0, active = (eflags & OALSFX_ENV_ACTIVE) != 0;
    const bool stop = active && (eflags & OALSFX_ENV_STOP) != 0, glide = active && (eflags & OALSFX_ENV_GLIDE) != 0;
    // D frames of delay, then F' = shown - D frames of the voice, of which the sampler runs over the first F'' = advanced
    const uint32_t delay = active ? (CARRIED ? carried->delay : env->delay) : 0U;
    const uint32_t D = delay < frames ? delay : frames;
    const uint32_t shown = frames - D;
    const uint32_t R = active ? env->ramp_frames : 0U, n0 = active ? (CARRIED ? carried->ramp_done : env->ramp_done) : 0U;
    const uint32_t advanced = stop && R - n0 < shown ? R - n0 : shown;
    const uint32_t step_now = CARRIED ? carried->step : rec->step;
    const uint32_t G = glide ? env->glide_frames : 0U, g0 = glide ? (CARRIED ? carried->glide_done : env->glide_done) : 0U;
    const uint32_t step_to = glide ? env->step_to : step_now;
    uint64_t phi = 0;
    if (!playing || advanced == 0) {
        // the cheapest path: zeros, no asset read
        if constexpr (!Sink::kAdds) store_zeros<C, V>(out, 0U, frames, lane);
    } else {
        if constexpr (!Sink::kAdds) {
            store_zeros<C, V>(out, 0U, D, lane);
            store_zeros<C, V>(out, D + advanced, frames, lane);
        }
        Voice r;
        r.phi = ((CARRIED ? carried->position : rec->position) << kSub) | (active ? (CARRIED ? carried->sub : env->sub) : 0U);
        r.E = static_cast<uint64_t>(rec->frames) << kFine;
        r.L0 = static_cast<uint64_t>(rec->loop_start) << kFine;
        r.L1 = static_cast<uint64_t>(rec->loop_end) << kFine;
        r.sigma = static_cast<uint64_t>(step_now) << kSub;
        r.sigma_to = static_cast<uint64_t>(step_to) << kSub;
        r.slope = glide ? static_cast<int64_t>(env->glide_slope) : 0;
        r.g = g0;
        r.G = G;
        r.n = n0;
        r.R = R;
        r.frames = rec->frames;
        r.loop_start = rec->loop_start;
        r.loop_end = rec->loop_end;
        r.loop = (flags & OALSFX_SAMPLER_LOOP) != 0;
        r.linear = (flags & OALSFX_SAMPLER_LINEAR) != 0;
        r.env = active;
        const void* const data = reinterpret_cast<const void*>(rec->data);
        const bool mono = rec->channels == 1;
        const uint32_t format = rec->format;
        float gain[C], from[C], step[C], to[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            gain[c] = rec->gain[c];
            from[c] = active ? env->gain_from[c] : 1.0F;
            step[c] = active ? env->gain_step[c] : 0.0F;
            to[c] = active ? env->gain_to[c] : 1.0F;
        }
        float* const at = out + static_cast<size_t>(D) * C;
        const unsigned owner = Sink::kAdds ? (lane + kWave - D % kWave) % kWave : lane;
        if (format == OALSFX_PCM_S16) phi = render_layout<C, V, int16_t, Sink, TABLED>(data, mono, r, coef, taps, shift, gain, from, step, to, at, advanced, owner);
        else if (format == OALSFX_PCM_F32) phi = render_layout<C, V, float, Sink, TABLED>(data, mono, r, coef, taps, shift, gain, from, step, to, at, advanced, owner);
        else phi = render_layout<C, V, uint8_t, Sink, TABLED>(data, mono, r, coef, taps, shift, gain, from, step, to, at, advanced, owner);
    }
    if constexpr (CARRIED) {
        // on values that are the same in every lane, in every lane
        if (!playing && !active) return;
        leave(IntoCarried{carried}, rec, flags, playing, active, stop, glide, advanced, shown, phi, delay, D, R, n0, G, g0, step_to);
    } else {
        if (lane != 0 || (!playing && !active)) return;
        leave(IntoRecords{rec, env}, rec, flags, playing, active, stop, glide, advanced, shown, phi, delay, D, R, n0, G, g0, step_to);
    }
}

static_assert(sizeof(oalsfx_sampler) == 80 && sizeof(oalsfx_envelope) == 144 && offsetof(oalsfx_envelope, gain_from) == 16 &&
              offsetof(oalsfx_envelope, glide_frames) == 112 && offsetof(oalsfx_envelope, sub) == 128, "the layout the row body reads and writes");

} // namespace

} // namespace oalsfx_hip

#endif
