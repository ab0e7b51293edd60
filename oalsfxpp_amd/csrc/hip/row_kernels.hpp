// What the four row kernels share -- k_sampler_rows (sampler.hip), k_voice_rows (voice.hip), k_fir_rows (resample.hip) and k_mix_rows
// (polyphony.hip), one wavefront per row, lane l owning the frames l, l + 64, ... --: the workgroup's shape, a frame's stores, the asset
// conversions, the wrap into a loop, and the one way from a channel count and a destination to a kernel's instantiation and grid.
// Everything here also compiles for the host behind the shim of tests/cpp/fir_rows_host.cpp.
#ifndef OALSFX_HIP_ROW_KERNELS_HPP
#define OALSFX_HIP_ROW_KERNELS_HPP

#ifndef OALSFX_FIR_HOST_SHIM
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "oalsfx_hip.h"

namespace oalsfx_hip {

namespace {

constexpr int kWave = 64;
constexpr int kRows = 4;                   // rows (wavefronts) per workgroup

#ifndef OALSFX_FIR_HOST_SHIM
template <int V> struct Vec { typedef float type __attribute__((ext_vector_type(V))); };
template <> struct Vec<1> { typedef float type; };
#endif

template <int C, int V>
__device__ __forceinline__ void store_frame(float* __restrict__ at, const float (&x)[C])
{
#ifndef OALSFX_FIR_HOST_SHIM
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
#else
    for (int c = 0; c < C; ++c) at[c] = x[c];
#endif
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

// Floats one lane stores at once (4, 2 or 1): as wide as the channel count and the destination's address allow (sampler_vector).
inline int row_vector(const void* dst, int channels)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | (static_cast<uintptr_t>(channels) * sizeof(float));
    return bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1;
}

template <int C, class Launch>
void launch_rows_width(int vector, int rows, Launch& launch)
{
    const dim3 grid(static_cast<unsigned>((rows + kRows - 1) / kRows)), block(kWave * kRows);
    if constexpr (C % 4 == 0)
        if (vector >= 4) return launch(std::integral_constant<int, C>(), std::integral_constant<int, 4>(), grid, block);
    if constexpr (C % 2 == 0)
        if (vector >= 2) return launch(std::integral_constant<int, C>(), std::integral_constant<int, 2>(), grid, block);
    launch(std::integral_constant<int, C>(), std::integral_constant<int, 1>(), grid, block);
}

// The launch of a row kernel k<C, V> over `rows` rows of `channels` channels at dst: calls launch(integral_constant<int, C>,
// integral_constant<int, V>, grid, block) with C the channel count, V the widest store that divides C and that dst is aligned to, and
// one wavefront per row, kRows to a workgroup (`launch` is a generic lambda around the caller's hipLaunchKernelGGL: a kernel template
// cannot be an argument itself).  False, with nothing called, for a channel count no format has.
template <class Launch>
bool launch_rows(int channels, const void* dst, int rows, Launch launch)
{
    const int vector = row_vector(dst, channels);
    switch (channels) {
    case 1: launch_rows_width<1>(vector, rows, launch); return true;
    case 2: launch_rows_width<2>(vector, rows, launch); return true;
    case 4: launch_rows_width<4>(vector, rows, launch); return true;
    case 6: launch_rows_width<6>(vector, rows, launch); return true;
    case 7: launch_rows_width<7>(vector, rows, launch); return true;
    case 8: launch_rows_width<8>(vector, rows, launch); return true;
    default: return false; // (no channel format has 3 or 5 channels: oalsfx_host_channel_count)
    }
}

} // namespace

} // namespace oalsfx_hip

#endif
