// Resamplers: the voices' render with a table index per row.  A row that names a table takes the value of a frame from a 4- or 8-tap FIR
// over the frames around its position, the coefficients selected by the position's fraction, in the arithmetic that
// include/oalsfx_hip.h states ("resamplers"), bit for bit; positions, wrapping, envelopes and both records afterwards are those of every
// voice.  A row that names none runs the code k_voice_rows runs (and with an envelope that is not ACTIVE therefore gets sampler.hip's
// bits).
//
// The shape is k_voice_rows': one wavefront per row, the row number in a scalar register so that both records, the table index and the
// table's descriptor are scalar loads and every branch on them is wave-uniform.  The row's body is voice_rows_body.hpp, which voice.hip
// (without tables) and polyphony.hip compile as well; here the tables are looked up (TABLED) and a voice's frames are stored
// (StoreSink).  No LDS, no cross-lane operation, no atomics: the file also compiles for the host, the lanes run one after the other
// (tests/cpp/fir_rows_host.cpp).
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

bool launch_fir(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int rows, unsigned frames, int channels,
                float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, rows, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_fir_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, tables, dst, rows,
                           frames);
    });
}

void launch_fir_upload(int* resamplers, const int* index, const int* changed, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(k_fir_upload, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, resamplers, index, changed, count);
}

} // namespace oalsfx_hip
