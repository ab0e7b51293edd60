// Voice envelopes: the samplers' render (sampler.hip) with a second record per row, which starts the voice after a delay, ramps a gain per
// output channel, stops the voice when a fade completes and glides its pitch; in the arithmetic that include/oalsfx_hip.h states ("voice
// envelopes"), bit for bit.  A row whose envelope is not ACTIVE gets the samplers' bits.
//
// The render itself is voice_rows_body.hpp, the row body that resample.hip and polyphony.hip compile as well; this file compiles it
// without tables (TABLED off: no table is looked up, the FIR bodies are not instantiated, and at eight channels a lane keeps four frames
// in flight, not three) and adds the kernel's row number, the envelopes' upload and the launchers.  The shape is k_sampler_rows': one
// wavefront per row, lane l owns the frames l, l + 64, ..., a frame's channels go out as one store where the address allows, a lane
// issues the loads of several of its frames before the first conversion.  Positions carry 16 more fractional bits (PHI = position << 16 |
// sub), so that a glide's fine step S_g = (step << 16) + g * slope adds up exactly: a frame's offset from its tile's base is the closed
// form m * S_g + slope * m (m - 1) / 2 + (t - m) * (step_to << 16), m the frames of the t in front of it that lie inside the glide -- a
// select per lane, no loop --; without a glide m is 0 and the offset is the samplers' t * step, 16 bits up.  The tile's base is wrapped
// into the loop once per tile, wave-uniformly (a one-shot's stays at its end once it has got there), a lane takes a 64-bit remainder
// only where its own offset carries it more than one loop length past the loop's end, and what the base is after the last tile is the
// position the row leaves behind.  Frames of delay and frames behind a completed STOP are zeros written apart from the tiles: they take
// no part in the asset loads.  Lane 0 writes both records back.  Rows are independent: no atomics, no LDS, no cross-lane operation: the
// file also compiles for the host, the lanes run one after the other (tests/cpp/fir_rows_host.cpp).
#include "voice.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "voice_rows_body.hpp"

namespace oalsfx_hip {

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
    voice_row<C, V, StoreSink, false>(records + row, envelopes + row, OALSFX_RESAMPLER_NONE, FirTables{}, dst + static_cast<size_t>(row) * frames * C, frames,
                                      lane);
}

// envelopes[index[k]] = changed[k]: the records oalsfx_batch_set_envelopes has written since the last render, put in place in front of it.
__global__ __launch_bounds__(256) void k_voice_upload(oalsfx_envelope* envelopes, const int* __restrict__ index, const oalsfx_envelope* __restrict__ changed,
                                                      int count)
{
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < count) envelopes[index[k]] = changed[k];
}

bool launch_voice(oalsfx_sampler* records, oalsfx_envelope* envelopes, int rows, unsigned frames, int channels, float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, rows, [=](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_voice_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, dst, rows, frames);
    });
}

void launch_voice_upload(oalsfx_envelope* envelopes, const int* index, const oalsfx_envelope* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_voice_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, envelopes, index, changed, count);
}

} // namespace oalsfx_hip
