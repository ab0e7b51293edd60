// Voice envelopes: the samplers' render (sampler.hip) with a second record per row, which starts the voice after a delay, ramps a gain per
// output channel, stops the voice when a fade completes and glides its pitch; in the arithmetic that include/oalsfx_hip.h states ("voice
// envelopes"), bit for bit.  A row whose envelope is not ACTIVE gets the samplers' bits.
//
// The shape is k_sampler_rows': one wavefront per row, lane l owns the frames l, l + 64, ..., a frame's channels go out as one store where
// the address allows, a lane issues the loads of several of its frames before the first conversion.  Positions carry 16 more fractional
// bits (PHI = position << 16 | sub), so that a glide's fine step S_g = (step << 16) + g * slope adds up exactly: a frame's offset from its
// tile's base is the closed form m * S_g + slope * m (m - 1) / 2 + (t - m) * (step_to << 16), m the frames of the t in front of it that
// lie inside the glide -- a select per lane, no loop --; without a glide m is 0 and the offset is the samplers' t * step, 16 bits up.
// The tile's base is wrapped into the loop once per tile, wave-uniformly (a one-shot's stays at its end once it has got there), a lane
// takes a 64-bit remainder only where its own offset carries it more than one loop length past the loop's end, and what the base is
// after the last tile is the position the row leaves behind.  Frames of delay and frames behind a completed STOP are zeros written apart
// from the tiles: they take no part in the asset loads.  Lane 0 writes both records back.  Rows are independent: no atomics, no LDS.
#include "voice.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

namespace oalsfx_hip {

namespace {

constexpr int kWave = 64;
constexpr int kRows = 4;                   // rows (wavefronts) per workgroup
constexpr int kFrac = OALSFX_SAMPLER_FRAC_BITS;
constexpr int kSub = OALSFX_ENV_SUB_BITS;
constexpr int kFine = kFrac + kSub;        // fractional bits of PHI

template <int V> struct Vec { typedef float type __attribute__((ext_vector_type(V))); };
template <> struct Vec<1> { typedef float type; };

// frames of one lane whose loads are issued together
template <int C> struct Ahead { static constexpr int value = C <= 2 ? 8 : 4; };

template <int C, int V>
__device__ __forceinline__ void store_frame(float* __restrict__ at, const float (&x)[C])
{
    typedef typename Vec<V>::type vec;
#pragma unroll
    for (int j = 0; j < C / V; ++j) {
        vec v;
        if constexpr (V == 1) v = x[j];
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = x[j * V + i];
        }
        reinterpret_cast<vec*>(at)[j] = v;
    }
}

template <int C, int V>
__device__ __forceinline__ void store_zeros(float* __restrict__ out, unsigned from, unsigned to, unsigned lane)
{
    float zero[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zero[c] = 0.0F;
    for (unsigned f = from + lane; f < to; f += kWave) store_frame<C, V>(out + static_cast<size_t>(f) * C, zero);
}

// the conversions of the reference's demo program (src/oalsfxpp_test.cpp:713-735)
__device__ __forceinline__ float to_float(uint8_t v) { return static_cast<float>(static_cast<int>(v) - 128) / 128.0F; }
__device__ __forceinline__ float to_float(int16_t v) { return static_cast<float>(v) / 32768.0F; }
__device__ __forceinline__ float to_float(float v) { return v; }

// q, at or past the loop's end L1, taken back into [L0, L1):  L0 + (q - L0) mod len  ==  L0 + (q - L1) mod len
__device__ __forceinline__ uint64_t wrap_past(uint64_t q, uint64_t L0, uint64_t L1, uint64_t len)
{
    uint64_t r = q - L1;
    if (r >= len) r %= len;
    return L0 + r;
}

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

// The frames [0, F) of one playing row, F >= 1; returns PHI behind them, wrapped (a one-shot's: E once it has ended).
// T: the asset's element; MONO: one asset channel for every output channel, else C.
template <int C, int V, typename T, bool MONO>
__device__ __forceinline__ uint64_t render(const T* __restrict__ data, const Voice& r, const float (&gain)[C], const float (&from)[C], const float (&step)[C],
                                           const float (&to)[C], float* __restrict__ out, unsigned F, unsigned lane)
{
    constexpr int K = MONO ? 1 : C;
    constexpr int kAhead = Ahead<C>::value;
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
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = v[MONO ? 0 : c] * gain[c];
                if (r.env) {
                    const uint32_t n = r.n + f;
                    const float nf = static_cast<float>(n); // exact: used only where n < R <= 2^24
#pragma unroll
                    for (int c = 0; c < C; ++c) o[c] = o[c] * (n < r.R ? from[c] + (nf * step[c]) : to[c]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = 0.0F;
            }
            store_frame<C, V>(out + static_cast<size_t>(f) * C, o);
        }
        const uint32_t m = F - f0 < kTile ? F - f0 : kTile;
        base += advance(r, g, m);
        g = r.G - g < m ? r.G : g + m;
        if (r.loop) {
            if (base >= r.L1) base = wrap_past(base, r.L0, r.L1, len);
        } else if (base > r.E) {
            base = r.E; // ended: every later frame is past the end as well
        }
    }
    return base;
}

template <int C, int V, typename T>
__device__ __forceinline__ uint64_t render_layout(const void* data, bool mono, const Voice& r, const float (&gain)[C], const float (&from)[C],
                                                  const float (&step)[C], const float (&to)[C], float* __restrict__ out, unsigned F, unsigned lane)
{
    if constexpr (C == 1) return render<C, V, T, true>(static_cast<const T*>(data), r, gain, from, step, to, out, F, lane);
    else if (mono) return render<C, V, T, true>(static_cast<const T*>(data), r, gain, from, step, to, out, F, lane);
    else return render<C, V, T, false>(static_cast<const T*>(data), r, gain, from, step, to, out, F, lane);
}

} // namespace

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_voice_resources.py)
// Workgroup g, wavefront w: row g * kRows + w.  C channels, V floats per store (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_voice_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, float* __restrict__ dst, int rows,
                                                              unsigned frames)
{
    // (the row number in a scalar register: the fields of both records are the same in every lane)
    const int row = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (row >= rows) return;
    const unsigned lane = threadIdx.x % kWave;
    oalsfx_sampler* const rec = records + row;
    oalsfx_envelope* const env = envelopes + row;
    float* const out = dst + static_cast<size_t>(row) * frames * C;
    const uint32_t flags = rec->flags, eflags = env->flags;
    const bool playing = (flags & OALSFX_SAMPLER_PLAYING) != 0, active = (eflags & OALSFX_ENV_ACTIVE) != 0;
    const bool stop = active && (eflags & OALSFX_ENV_STOP) != 0, glide = active && (eflags & OALSFX_ENV_GLIDE) != 0;
    // D frames of delay, then F' = shown - D frames of the voice, of which the sampler runs over the first F'' = advanced
    const uint32_t delay = active ? env->delay : 0U;
    const uint32_t D = delay < frames ? delay : frames;
    const uint32_t shown = frames - D;
    const uint32_t R = active ? env->ramp_frames : 0U, n0 = active ? env->ramp_done : 0U;
    const uint32_t advanced = stop && R - n0 < shown ? R - n0 : shown;
    const uint32_t step_now = rec->step;
    const uint32_t G = glide ? env->glide_frames : 0U, g0 = glide ? env->glide_done : 0U;
    const uint32_t step_to = glide ? env->step_to : step_now;
    uint64_t phi = 0;
    if (!playing || advanced == 0) {
        // the cheapest path: zeros, no asset read
        store_zeros<C, V>(out, 0U, frames, lane);
    } else {
        store_zeros<C, V>(out, 0U, D, lane);
        store_zeros<C, V>(out, D + advanced, frames, lane);
        Voice r;
        r.phi = (rec->position << kSub) | (active ? env->sub : 0U);
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
        if (format == OALSFX_PCM_S16) phi = render_layout<C, V, int16_t>(data, mono, r, gain, from, step, to, at, advanced, lane);
        else if (format == OALSFX_PCM_F32) phi = render_layout<C, V, float>(data, mono, r, gain, from, step, to, at, advanced, lane);
        else phi = render_layout<C, V, uint8_t>(data, mono, r, gain, from, step, to, at, advanced, lane);
    }
    if (lane != 0 || (!playing && !active)) return;
    uint32_t flags_after = flags;
    if (playing && advanced != 0) {
        // after the call: PHI behind the frames advanced; a one-shot that has reached its end stops there
        if (!(flags & OALSFX_SAMPLER_LOOP) && phi >= static_cast<uint64_t>(rec->frames) << kFine) {
            phi = static_cast<uint64_t>(rec->frames) << kFine;
            flags_after &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
        }
        rec->position = phi >> kSub;
        if (active) env->sub = static_cast<uint32_t>(phi) & ((1U << kSub) - 1U);
    }
    if (active) {
        // the counters run on the frames rendered, playing or not
        const uint32_t ramp_done = R - n0 < shown ? R : n0 + shown;
        env->delay = delay - D;
        env->ramp_done = ramp_done;
        if (stop && ramp_done == R) flags_after &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
        if (glide) {
            const uint32_t glide_done = G - g0 < advanced ? G : g0 + advanced;
            env->glide_done = glide_done;
            if (glide_done == G) rec->step = step_to;
        }
    }
    rec->flags = flags_after;
}

// envelopes[index[k]] = changed[k]: the records oalsfx_batch_set_envelopes has written since the last render, put in place in front of it.
__global__ __launch_bounds__(256) void k_voice_upload(oalsfx_envelope* envelopes, const int* __restrict__ index, const oalsfx_envelope* __restrict__ changed,
                                                      int count)
{
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < count) envelopes[index[k]] = changed[k];
}

namespace {

static_assert(sizeof(oalsfx_envelope) == 144 && offsetof(oalsfx_envelope, gain_from) == 16 && offsetof(oalsfx_envelope, glide_frames) == 112 &&
              offsetof(oalsfx_envelope, sub) == 128, "the layout the kernel reads and writes");

template <int C, int V>
void launch(oalsfx_sampler* records, oalsfx_envelope* envelopes, int rows, unsigned frames, float* dst, hipStream_t stream)
{
    hipLaunchKernelGGL((k_voice_rows<C, V>), dim3(static_cast<unsigned>((rows + kRows - 1) / kRows)), dim3(kWave * kRows), 0, stream, records, envelopes, dst,
                       rows, frames);
}

template <int C>
void launch_width(int vector, oalsfx_sampler* records, oalsfx_envelope* envelopes, int rows, unsigned frames, float* dst, hipStream_t stream)
{
    if constexpr (C % 4 == 0)
        if (vector >= 4) return launch<C, 4>(records, envelopes, rows, frames, dst, stream);
    if constexpr (C % 2 == 0)
        if (vector >= 2) return launch<C, 2>(records, envelopes, rows, frames, dst, stream);
    launch<C, 1>(records, envelopes, rows, frames, dst, stream);
}

} // namespace

bool launch_voice(oalsfx_sampler* records, oalsfx_envelope* envelopes, int rows, unsigned frames, int channels, float* dst, hipStream_t stream)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | (static_cast<uintptr_t>(channels) * sizeof(float));
    const int vector = bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1; // sampler_vector's rule
    switch (channels) {
    case 1: launch_width<1>(vector, records, envelopes, rows, frames, dst, stream); return true;
    case 2: launch_width<2>(vector, records, envelopes, rows, frames, dst, stream); return true;
    case 4: launch_width<4>(vector, records, envelopes, rows, frames, dst, stream); return true;
    case 6: launch_width<6>(vector, records, envelopes, rows, frames, dst, stream); return true;
    case 7: launch_width<7>(vector, records, envelopes, rows, frames, dst, stream); return true;
    case 8: launch_width<8>(vector, records, envelopes, rows, frames, dst, stream); return true;
    default: return false; // (no channel format has 3 or 5 channels: oalsfx_host_channel_count)
    }
}

void launch_voice_upload(oalsfx_envelope* envelopes, const int* index, const oalsfx_envelope* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_voice_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, envelopes, index, changed, count);
}

} // namespace oalsfx_hip
