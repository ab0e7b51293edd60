// Bus sends: level 1 of the bus downmix where some member's gain ramps (include/oalsfx_hip.h, "bus sends").  The kernel of downmix.hip
// with one difference: a member's gain is no value but a row (from, step, to, frames, done), and the gain of an element is formed from
// the element's frame.  With `since` frames downmixed since the table was built, frame f of this call is n = done + since + f of the
// ramp, and e = n < frames ? from + ((float)n * step) : to -- product and sum rounded separately, no running sum, so that any split of a
// stretch of frames into calls gives the same bits.  A member without a ramp has frames == 0 and e == to on every frame.
//
// Still a streaming read of every routed row: one wavefront per (chunk, span of the row), the loads of its members' rows issued before
// the first addition -- of as many rows as the registers of the plain kernel's occupancy hold, the rest following as rows are added --,
// no LDS, no atomics, no cross-lane traffic.  The rows of the ramp table are the same for a whole wavefront
// (scalar loads); what is per lane is the frame of each of its V elements, worked out once, and per member and element a conversion, a
// product, a sum and a select in front of the product and the sum the plain kernel has.  Level 2 is downmix.hip's.
#include "downmix.hpp"

#include <cstdint>

#pragma clang fp contract(off)

namespace oalsfx_hip {

namespace {

// (downmix.hip's kChunk, kWave and kSumBatch under names of their own: the host build of the tests compiles both files as one)
constexpr int kMembers = OALSFX_DOWNMIX_CHUNK;
constexpr int kLanes = 64; // one wavefront per workgroup: the two level-1 kernels share the grid
constexpr int kBatch = 8;  // loads in flight per lane in a short chunk
// Wavefronts a SIMD holds, as many as of k_downmix_chunks<V> (46, 68 and 66 VGPRs): the pass lives on loads in flight across wavefronts,
// and with a whole chunk's rows held at once (260 VGPRs at V = 4) a SIMD would hold one.  So a full chunk keeps kRowsInFlight rows in
// registers -- what the compiler makes of the plain kernel too, which starts adding at V = 4 with fourteen rows loaded.  (Ten rows at
// V = 4: 66 VGPRs; twelve spill.)
template <int V> constexpr int kWavesPerSimd = V == 1 ? 8 : 7;
template <int V> constexpr int kRowsInFlight = V == 4 ? 10 : V == 2 ? 24 : 32;

// V floats at `at`, which is V * 4 bytes aligned, in one load; on the host (tests/cpp/bus_sends_host.cpp) float by float.
template <int V>
__device__ __forceinline__ void load_floats(const float* __restrict__ at, float (&x)[V])
{
#ifndef OALSFX_FIR_HOST_SHIM
    typedef float vec __attribute__((ext_vector_type(V)));
    const vec v = *reinterpret_cast<const vec*>(at);
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = v[j];
#else
    for (int j = 0; j < V; ++j) x[j] = at[j];
#endif
}

template <>
__device__ __forceinline__ void load_floats<1>(const float* __restrict__ at, float (&x)[1])
{
    x[0] = at[0];
}

template <int V>
__device__ __forceinline__ void store_floats(float* __restrict__ at, const float (&x)[V])
{
#ifndef OALSFX_FIR_HOST_SHIM
    typedef float vec __attribute__((ext_vector_type(V)));
    vec v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = x[j];
    *reinterpret_cast<vec*>(at) = v;
#else
    for (int j = 0; j < V; ++j) at[j] = x[j];
#endif
}

template <>
__device__ __forceinline__ void store_floats<1>(float* __restrict__ at, const float (&x)[1])
{
    at[0] = x[0];
}

// What is left of a member's ramp when the call begins: frame f of the call ramps while f < left, at n = at + f.
struct RampWindow {
    unsigned left, at;
};

__device__ __forceinline__ RampWindow window(const DownmixRamp& r, unsigned long long since)
{
    const unsigned ahead = r.frames - r.done; // (done <= frames <= 2^24)
    if (since >= ahead) return {0U, 0U};
    return {ahead - static_cast<unsigned>(since), r.done + static_cast<unsigned>(since)}; // at + f < frames wherever f < left
}

// p = p + (x * e), element by element, e from the element's frame
template <int V>
__device__ __forceinline__ void add_member(float (&p)[V], const float (&x)[V], const unsigned (&frame)[V], const DownmixRamp& r, const RampWindow w)
{
#pragma unroll
    for (int j = 0; j < V; ++j) {
        // (tied to the loaded value: e does not depend on x, and left alone the compiler forms the e of all 32 members ahead of the
        // loads' return -- 128 more VGPRs at V = 4)
        unsigned f = frame[j];
#ifndef OALSFX_FIR_HOST_SHIM
        asm volatile("" : "+v"(f) : "v"(x[j]));
#endif
        // (past the window the sum may wrap: its value is not used there)
        float ramped = r.from + static_cast<float>(w.at + f) * r.step;
#ifndef OALSFX_FIR_HOST_SHIM
        asm volatile("" : "+v"(ramped)); // (a value, so that what follows is a select and no branch around the three operations above)
#endif
        const float e = f < w.left ? ramped : r.to;
        p[j] = p[j] + x[j] * e;
    }
}

} // namespace

// Workgroup g: chunk g / spans, span g % spans of the row; lane l owns elements (span * 64 + l) * V .. + V (k_downmix_chunks' layout).
template <int V>
__global__ __launch_bounds__(kLanes, kWavesPerSimd<V>) void k_downmix_ramp_chunks(const DownmixChunk* __restrict__ chunks, const int* __restrict__ members,
                                                               const DownmixRamp* __restrict__ ramps, const float* __restrict__ src,
                                                               float* __restrict__ dst, float* __restrict__ partials, unsigned elements, unsigned spans,
                                                               unsigned channels, unsigned long long since)
{
    const DownmixChunk c = chunks[blockIdx.x / spans];
    const size_t e = (static_cast<size_t>(blockIdx.x % spans) * kLanes + threadIdx.x) * V;
    if (e >= elements) return;
    const int* const m = members + c.first;
    const DownmixRamp* const r = ramps + c.first;
    const float* const col = src + e;
    // the frames of this lane's V elements: element / channels, one division and then steps
    unsigned frame[V];
    {
        unsigned f = static_cast<unsigned>(e) / channels, ch = static_cast<unsigned>(e) - f * channels;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            frame[j] = f;
            if (++ch == channels) {
                ch = 0;
                ++f;
            }
        }
    }
    float p[V];
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = 0.0F;
    if (c.count == kMembers) {
        // kDepth rows in flight: the first kDepth loads go out before the first addition, and every row added gives its registers to the
        // load of the row kDepth behind it
        constexpr int kDepth = kRowsInFlight<V>;
        float x[kDepth][V];
#pragma unroll
        for (int k = 0; k < kDepth; ++k) load_floats<V>(col + static_cast<size_t>(m[k]) * elements, x[k]);
#pragma unroll
        for (int k = 0; k < kMembers; ++k) {
            add_member<V>(p, x[k % kDepth], frame, r[k], window(r[k], since));
            if (k + kDepth < kMembers) {
                // (the address tied to the sum so far: the load stays behind the addition that frees its registers, where the compiler
                // would otherwise move it up and then spill to scratch memory what does not fit)
                const float* next = col;
#ifndef OALSFX_FIR_HOST_SHIM
#pragma unroll
                for (int j = 0; j < V; ++j) asm volatile("" : "+v"(next) : "v"(p[j]));
#endif
                load_floats<V>(next + static_cast<size_t>(m[k + kDepth]) * elements, x[k % kDepth]);
            }
        }
    } else {
        // (a bus's last chunk, or all of a small bus: the rows beyond the chunk's end are read again as its last row and not added)
        for (int base = 0; base < c.count; base += kBatch) {
            float x[kBatch][V];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int at = base + k < c.count ? base + k : c.count - 1;
                load_floats<V>(col + static_cast<size_t>(m[at]) * elements, x[k]);
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k)
                if (base + k < c.count) add_member<V>(p, x[k], frame, r[base + k], window(r[base + k], since));
        }
    }
    if (c.row < 0) {
        // (the bus has this chunk only: out = +0.0f + p, what level 2 would have made of it)
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = 0.0F + p[j];
        store_floats<V>(dst + static_cast<size_t>(c.bus) * elements + e, p);
    } else {
        store_floats<V>(partials + static_cast<size_t>(c.row) * elements + e, p);
    }
}

namespace {

template <int V>
void launch(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int channels, unsigned long long since, hipStream_t stream)
{
    const unsigned spans = static_cast<unsigned>((elements + kLanes * V - 1) / (kLanes * V));
    hipLaunchKernelGGL(k_downmix_ramp_chunks<V>, dim3(static_cast<unsigned>(t.n_chunks) * spans), dim3(kLanes), 0, stream, t.chunks, t.members, t.ramps, src, dst,
                       partials, static_cast<unsigned>(elements), spans, static_cast<unsigned>(channels), since);
}

} // namespace

void launch_ramp_chunks(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int channels, unsigned long long since,
                        int vector, hipStream_t stream)
{
    if (!t.n_chunks) return;
    if (vector >= 4) launch<4>(t, src, dst, partials, elements, channels, since, stream);
    else if (vector >= 2) launch<2>(t, src, dst, partials, elements, channels, since, stream);
    else launch<1>(t, src, dst, partials, elements, channels, since, stream);
}

} // namespace oalsfx_hip
