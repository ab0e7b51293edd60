// Resamplers: the voices' render (voice.hip) with a table index per row.  A row that names a table takes the value of a frame from a 4- or
// 8-tap FIR over the frames around its position, the coefficients selected by the position's fraction, in the arithmetic that
// include/oalsfx_hip.h states ("resamplers"), bit for bit; positions, wrapping, envelopes and both records afterwards are voice.hip's.  A
// row that names none takes voice.hip's arithmetic exactly (and with an envelope that is not ACTIVE therefore sampler.hip's).
//
// The shape is k_voice_rows': one wavefront per row, the row number in a scalar register so that both records, the table index and the
// table's descriptor are scalar loads and every branch on them is wave-uniform.  The row's body is voice_rows_body.hpp, which
// polyphony.hip compiles as well; here a voice's frames are stored (StoreSink).  No LDS, no cross-lane operation, no atomics: the file
// also compiles for the host, the lanes run one after the other (tests/cpp/fir_rows_host.cpp).
#include "resample.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "voice_rows_body.hpp"

namespace oalsfx_hip {

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_resample_resources.py)
// Workgroup g, wavefront w: row g * kRows + w.  C channels, V floats per store (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_fir_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                            const FirTables tables, float* __restrict__ dst, int rows, unsigned frames)
{
    // (the row number in a scalar register: the fields of both records and the table's descriptor are the same in every lane)
    const int row = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (row >= rows) return;
    const unsigned lane = threadIdx.x % kWave;
    voice_row<C, V, StoreSink>(records + row, envelopes + row, resamplers[row], tables, dst + static_cast<size_t>(row) * frames * C, frames, lane);
}

// resamplers[index[k]] = changed[k]: the indices oalsfx_batch_set_resamplers has written since the last render, put in place in front of it.
__global__ __launch_bounds__(256) void k_fir_upload(int* resamplers, const int* __restrict__ index, const int* __restrict__ changed, int count)
{
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < count) resamplers[index[k]] = changed[k];
}

namespace {

template <int C, int V>
void launch(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int rows, unsigned frames, float* dst,
            hipStream_t stream)
{
    hipLaunchKernelGGL((k_fir_rows<C, V>), dim3(static_cast<unsigned>((rows + kRows - 1) / kRows)), dim3(kWave * kRows), 0, stream, records, envelopes,
                       resamplers, tables, dst, rows, frames);
}

template <int C>
void launch_width(int vector, oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int rows, unsigned frames,
                  float* dst, hipStream_t stream)
{
    if constexpr (C % 4 == 0)
        if (vector >= 4) return launch<C, 4>(records, envelopes, resamplers, tables, rows, frames, dst, stream);
    if constexpr (C % 2 == 0)
        if (vector >= 2) return launch<C, 2>(records, envelopes, resamplers, tables, rows, frames, dst, stream);
    launch<C, 1>(records, envelopes, resamplers, tables, rows, frames, dst, stream);
}

} // namespace

bool launch_fir(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int rows, unsigned frames, int channels,
                float* dst, hipStream_t stream)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | (static_cast<uintptr_t>(channels) * sizeof(float));
    const int vector = bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1; // sampler_vector's rule
    switch (channels) {
    case 1: launch_width<1>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    case 2: launch_width<2>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    case 4: launch_width<4>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    case 6: launch_width<6>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    case 7: launch_width<7>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    case 8: launch_width<8>(vector, records, envelopes, resamplers, tables, rows, frames, dst, stream); return true;
    default: return false; // (no channel format has 3 or 5 channels: oalsfx_host_channel_count)
    }
}

void launch_fir_upload(int* resamplers, const int* index, const int* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_fir_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, resamplers, index, changed, count);
}

} // namespace oalsfx_hip
