// Level meters: per row of [row][frame][channel] -- an instance's output or a bus -- the peak and the sum of squares per channel, the
// count of non-finite elements and the trailing run of quiet frames, in the order that include/oalsfx_hip.h states ("level meters"), bit
// for bit.
//
// A streaming read of every row with an 80-byte result: the loads in flight decide the time, not the arithmetic.  One wavefront per row;
// lane l owns the frames f = l, l + 64, ... and loads a frame's channels as one access where the address allows, so that the 64 lanes
// together read 64 * channels contiguous floats.  A lane issues the loads of several of its frames before the first addition and keeps
// its sums, maxima, last loud frame and non-finite count in registers; the stated tree over the lanes finishes the sums, and the maxima,
// the last loud frame and the count go the same way.  Lane 0 writes the record.  Rows are independent: no atomics, no LDS, one launch.
#include "meter.hpp"

#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace oalsfx_hip {

namespace {

constexpr int kWave = OALSFX_METER_LANES;  // the lanes of the stated order are the lanes of a wavefront
constexpr int kRows = 4;                   // rows (wavefronts) per workgroup
static_assert(kWave == 64, "the stated order is that of a 64-lane wavefront");

template <int V> struct Vec { typedef float type __attribute__((ext_vector_type(V))); };
template <> struct Vec<1> { typedef float type; };

// frames of one lane whose loads are issued together
template <int C> struct Ahead { static constexpr int value = C <= 2 ? 8 : 4; };

template <int C, int V>
__device__ __forceinline__ void load_frame(const float* __restrict__ at, float (&x)[C])
{
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
}

} // namespace

// (a name outside the anonymous namespace so that the code object's notes list the kernel: tests/test_meter_abi.py)
// Workgroup g, wavefront w: row g * kRows + w.  C channels, V floats per load (C % V == 0, src aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_meter_rows(const float* __restrict__ src, oalsfx_meter* meters, int rows, unsigned frames,
                                                             float threshold, int carry)
{
    const int row = static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave;
    if (row >= rows) return; // (a whole wavefront: the lanes of a row stay together for the tree)
    const unsigned lane = threadIdx.x % kWave;
    const float* const x0 = src + static_cast<size_t>(row) * frames * C;
    constexpr int kAhead = Ahead<C>::value;
    float q[C], p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = p[c] = 0.0F;
    int last = -1;      // the lane's last loud frame
    unsigned bad = 0;   // its non-finite elements
    for (unsigned base = lane; base < frames; base += kWave * kAhead) {
        float x[kAhead][C];
        // (frames beyond the row's end are read again as the lane's first frame of the batch and take no part)
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned f = base + k * kWave;
            load_frame<C, V>(x0 + static_cast<size_t>(f < frames ? f : base) * C, x[k]);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const unsigned f = base + k * kWave;
            if (f >= frames) continue;
            bool loud = false;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = x[k][c], a = fabsf(v);
                q[c] = q[c] + v * v;
                p[c] = fmaxf(p[c], a);
                bad += !(a < INFINITY);
                loud |= !(a <= threshold);
            }
            if (loud) last = static_cast<int>(f);
        }
    }
    // the stated tree: lane l takes lane l + s.  (Lanes from s on compute values nobody reads.)
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = q[c] + __shfl_down(q[c], s);
            p[c] = fmaxf(p[c], __shfl_down(p[c], s));
        }
        const int other = __shfl_down(last, s);
        last = other > last ? other : last;
        bad += __shfl_down(bad, s);
    }
    if (lane != 0) return;
    oalsfx_meter* const m = meters + row;
    float hold = p[0];
#pragma unroll
    for (int c = 1; c < C; ++c) hold = fmaxf(hold, p[c]);
    const unsigned quiet = frames - 1U - static_cast<unsigned>(last); // (no loud frame: last == -1, and this is `frames`)
    unsigned run = quiet;
    if (carry) {
        const float old_hold = m->peak_hold;
        const unsigned old_run = m->quiet_run;
        hold = fmaxf(old_hold, hold);
        if (quiet == frames) run = old_run + frames < old_run ? UINT_MAX : old_run + frames;
    }
    typedef Vec<4>::type vec4;
    float w[2 * OALSFX_MAX_CHANNELS];
#pragma unroll
    for (int c = 0; c < OALSFX_MAX_CHANNELS; ++c) {
        w[c] = c < C ? p[c] : 0.0F;
        w[OALSFX_MAX_CHANNELS + c] = c < C ? q[c] : 0.0F;
    }
    vec4* const out = reinterpret_cast<vec4*>(m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vec4 v = {w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
        out[j] = v;
    }
    vec4 tail = {hold, __uint_as_float(run), __uint_as_float(bad), __uint_as_float(frames)};
    out[4] = tail;
}

namespace {

static_assert(sizeof(oalsfx_meter) == 80 && sizeof(oalsfx_meter) % 16 == 0, "a record is five 16-byte stores");
static_assert(offsetof(oalsfx_meter, sumsq) == 32 && offsetof(oalsfx_meter, peak_hold) == 64 && offsetof(oalsfx_meter, quiet_run) == 68 &&
              offsetof(oalsfx_meter, nonfinite) == 72 && offsetof(oalsfx_meter, frames) == 76, "the layout the kernel writes");

template <int C, int V>
void launch(const float* src, int rows, unsigned frames, float threshold, bool carry, oalsfx_meter* meters, hipStream_t stream)
{
    hipLaunchKernelGGL((k_meter_rows<C, V>), dim3(static_cast<unsigned>((rows + kRows - 1) / kRows)), dim3(kWave * kRows), 0, stream, src, meters, rows,
                       frames, threshold, carry ? 1 : 0);
}

template <int C>
void launch_width(int vector, const float* src, int rows, unsigned frames, float threshold, bool carry, oalsfx_meter* meters, hipStream_t stream)
{
    if constexpr (C % 4 == 0)
        if (vector >= 4) return launch<C, 4>(src, rows, frames, threshold, carry, meters, stream);
    if constexpr (C % 2 == 0)
        if (vector >= 2) return launch<C, 2>(src, rows, frames, threshold, carry, meters, stream);
    launch<C, 1>(src, rows, frames, threshold, carry, meters, stream);
}

} // namespace

int meter_vector(const void* src, int channels)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src) | (static_cast<uintptr_t>(channels) * sizeof(float));
    return bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1;
}

bool meter_fits(int rows)
{
    // (the runtime refuses a grid of 2^32 work-items or more)
    return (static_cast<unsigned long long>(rows) + kRows - 1) / kRows * (kWave * kRows) <= UINT_MAX;
}

bool launch_meter(const float* src, int rows, unsigned frames, int channels, float threshold, bool carry, oalsfx_meter* meters, hipStream_t stream)
{
    const int vector = meter_vector(src, channels);
    switch (channels) {
    case 1: launch_width<1>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    case 2: launch_width<2>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    case 4: launch_width<4>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    case 6: launch_width<6>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    case 7: launch_width<7>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    case 8: launch_width<8>(vector, src, rows, frames, threshold, carry, meters, stream); return true;
    default: return false; // (no channel format has 3 or 5 channels: oalsfx_host_channel_count)
    }
}

} // namespace oalsfx_hip
