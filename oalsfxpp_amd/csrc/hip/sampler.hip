// Samplers: every instance renders its row of [instance][frame][channel] from an asset resident in device memory -- 8-bit, 16-bit or
// fp32 PCM, mono or with the batch's channel count --, read at a fixed-point position that advances by a fixed-point step per frame,
// looping or not, nearest or linearly interpolated, times a gain per output channel; in the arithmetic that include/oalsfx_hip.h
// states ("samplers"), bit for bit.
//
// A streaming write of every row; the asset reads mostly hit the cache (a few hundred assets serve thousands of voices).  One wavefront
// per row; lane l owns the frames f = l, l + 64, ... and stores a frame's channels as one access where the address allows, so that the
// 64 lanes together write 64 * channels contiguous floats, and with a step near 4096 read contiguous asset elements too.  A lane issues
// the loads of several of its frames, both neighbours, before the first conversion.  Positions are exact 64-bit integers: the row's base
// is wrapped into the loop once per tile, wave-uniformly, and a lane takes a 64-bit remainder only where its own offset carries it more
// than one loop length past the loop's end.  Lane 0 writes the advanced position and flags.  Rows are independent: no atomics, no LDS.
#include "sampler.hpp"

#include <climits>
#include <cstdint>

#include "row_kernels.hpp"

#pragma clang fp contract(off)

namespace oalsfx_hip {

namespace {

constexpr int kFrac = OALSFX_SAMPLER_FRAC_BITS;

// frames of one lane whose loads are issued together
template <int C> struct Ahead { static constexpr int value = C <= 2 ? 8 : 4; };

struct Row {
    uint64_t position;
    uint32_t frames, loop_start, loop_end, step;
    bool loop, linear;
};

// One playing row.  T: the asset's element; MONO: one asset channel for every output channel, else C.
template <int C, int V, typename T, bool MONO>
__device__ __forceinline__ void render(const T* __restrict__ data, const Row& r, const float (&gain)[C], float* __restrict__ out, unsigned F, unsigned lane)
{
    constexpr int K = MONO ? 1 : C;
    constexpr int kAhead = Ahead<C>::value;
    constexpr unsigned kTile = kWave * kAhead;
    const uint64_t E = static_cast<uint64_t>(r.frames) << kFrac;
    const uint64_t L0 = static_cast<uint64_t>(r.loop_start) << kFrac, L1 = static_cast<uint64_t>(r.loop_end) << kFrac, len = L1 - L0;
    const uint64_t tile_step = static_cast<uint64_t>(r.step) * kTile;
    uint64_t base = r.position; // of the tile's first frame, wrapped: the same in every lane
    if (r.loop && base >= L1) base = wrap_past(base, L0, L1, len);
    for (unsigned f0 = 0; f0 < F; f0 += kTile) {
        T a[kAhead][K], b[kAhead][K];
        unsigned mu_bits[kAhead];
        bool live[kAhead], b_silent[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned in_tile = lane + k * kWave;
            uint64_t q = base + static_cast<uint64_t>(in_tile) * r.step;
            if (r.loop && q >= L1) q = wrap_past(q, L0, L1, len);
            mu_bits[k] = static_cast<unsigned>(q) & ((1U << kFrac) - 1U);
            // (a frame beyond the call's or past the asset's end reads element 0 and takes no part)
            live[k] = f0 + in_tile < F && (r.loop || q < E);
            const uint32_t i = live[k] ? static_cast<uint32_t>(q >> kFrac) : 0U;
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
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = 0.0F;
            }
            store_frame<C, V>(out + static_cast<size_t>(f) * C, o);
        }
        base += tile_step;
        if (r.loop && base >= L1) base = wrap_past(base, L0, L1, len);
    }
}

template <int C, int V, typename T>
__device__ __forceinline__ void render_layout(const void* data, bool mono, const Row& r, const float (&gain)[C], float* __restrict__ out, unsigned F, unsigned lane)
{
    if constexpr (C == 1) render<C, V, T, true>(static_cast<const T*>(data), r, gain, out, F, lane);
    else if (mono) render<C, V, T, true>(static_cast<const T*>(data), r, gain, out, F, lane);
    else render<C, V, T, false>(static_cast<const T*>(data), r, gain, out, F, lane);
}

} // namespace

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_sampler_abi.py)
// Workgroup g, wavefront w: row g * kRows + w.  C channels, V floats per store (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_sampler_rows(oalsfx_sampler* records, float* __restrict__ dst, int rows, unsigned frames)
{
    // (the row number in a scalar register: the record's fields are the same in every lane)
    const int row = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (row >= rows) return;
    const unsigned lane = threadIdx.x % kWave;
    oalsfx_sampler* const rec = records + row;
    float* const out = dst + static_cast<size_t>(row) * frames * C;
    const uint32_t flags = rec->flags;
    if (!(flags & OALSFX_SAMPLER_PLAYING)) {
        // the cheapest path: zeros, no asset read, the record as it is
        store_zeros<C, V>(out, 0U, frames, lane);
        return;
    }
    Row r;
    r.position = rec->position;
    r.frames = rec->frames;
    r.loop_start = rec->loop_start;
    r.loop_end = rec->loop_end;
    r.step = rec->step;
    r.loop = (flags & OALSFX_SAMPLER_LOOP) != 0;
    r.linear = (flags & OALSFX_SAMPLER_LINEAR) != 0;
    const void* const data = reinterpret_cast<const void*>(rec->data);
    const bool mono = rec->channels == 1;
    const uint32_t format = rec->format;
    float gain[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gain[c] = rec->gain[c];
    if (format == OALSFX_PCM_S16) render_layout<C, V, int16_t>(data, mono, r, gain, out, frames, lane);
    else if (format == OALSFX_PCM_F32) render_layout<C, V, float>(data, mono, r, gain, out, frames, lane);
    else render_layout<C, V, uint8_t>(data, mono, r, gain, out, frames, lane);
    if (lane != 0) return;
    // after the call: position = wrap(P + F * step); a one-shot that has reached its end stops there
    uint64_t end = r.position + static_cast<uint64_t>(frames) * r.step;
    uint32_t flags_after = flags;
    if (r.loop) {
        const uint64_t L0 = static_cast<uint64_t>(r.loop_start) << kFrac, L1 = static_cast<uint64_t>(r.loop_end) << kFrac;
        if (end >= L1) end = wrap_past(end, L0, L1, L1 - L0);
    } else if (end >= static_cast<uint64_t>(r.frames) << kFrac) {
        end = static_cast<uint64_t>(r.frames) << kFrac;
        flags_after &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
    }
    rec->position = end;
    rec->flags = flags_after;
}

// records[index[k]] = changed[k]: the records oalsfx_batch_set_samplers has written since the last render, put in place in front of it.
__global__ __launch_bounds__(256) void k_sampler_upload(oalsfx_sampler* records, const int* __restrict__ index, const oalsfx_sampler* __restrict__ changed,
                                                        int count)
{
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < count) records[index[k]] = changed[k];
}

namespace {

static_assert(sizeof(oalsfx_sampler) == 80 && offsetof(oalsfx_sampler, position) == 8 && offsetof(oalsfx_sampler, flags) == 40 &&
              offsetof(oalsfx_sampler, gain) == 48, "the layout the kernel reads and writes");

} // namespace

int sampler_vector(const void* dst, int channels)
{
    return row_vector(dst, channels);
}

bool sampler_fits(int rows)
{
    // (the runtime refuses a grid of 2^32 work-items or more)
    return (static_cast<unsigned long long>(rows) + kRows - 1) / kRows * (kWave * kRows) <= UINT_MAX;
}

bool launch_sampler(oalsfx_sampler* records, int rows, unsigned frames, int channels, float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, rows, [=](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_sampler_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, dst, rows, frames);
    });
}

void launch_sampler_upload(oalsfx_sampler* records, const int* index, const oalsfx_sampler* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_sampler_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, records, index, changed, count);
}

} // namespace oalsfx_hip
