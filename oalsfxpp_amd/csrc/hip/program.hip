// Envelope programs: a voice's queued envelope segments take their turn inside one render, at the exact frame, on the device
// (include/oalsfx_hip.h, "envelope programs").  For every voice the render of F frames is the concatenation of spans, each what the
// samplers', envelopes' and resamplers' contracts give a call of that many frames; the polyphony sums the voices' concatenated outputs.
//
// The shape is k_mix_rows': one wavefront per INSTANCE, the instance number in a scalar register, both flag words of every voice read in
// front of the first store, the row filled with +0.0f, the voices added lane by lane in ascending order.  Where k_mix_rows calls
// voice_row, this kernel calls program_row (program_rows_body.hpp), which walks the voice's queue; a voice with an empty queue costs the
// two words that say so.  At one lane a voice's frames are stored, not added, as k_fir_rows stores them: a lone voice's -0.0f reaches
// the input as -0.0f, which a sum that starts at +0.0f would lose.
//
// No LDS, no cross-lane operation, no atomics, no barrier: every element of the row is written and read by one lane only (lane f mod 64
// under AddSink; under StoreSink nothing is read), and every lane carries the records from span to span in copies of its own.  The
// file also compiles for the host, the lanes of a wavefront run one after the other (tests/cpp/program_rows_host.cpp).
#include "program.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "program_rows_body.hpp"

namespace oalsfx_hip {

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_program_resources.py)
// Workgroup g, wavefront w: instance g * kRows + w.  C channels, V floats per access (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_program_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                EnvProgram* programs, const FirTables tables, float* dst, int instances, int lanes,
                                                                unsigned frames)
{
    const int instance = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (instance >= instances) return;
    const unsigned lane = threadIdx.x % kWave;
    float* const out = dst + static_cast<size_t>(instance) * frames * C;
    // (a voice with a queue has an ACTIVE envelope: both calls that fill a queue refuse any other)
    uint32_t busy = 0;
#pragma unroll
    for (int k = 0; k < OALSFX_MAX_POLYPHONY; ++k) {
        if (k < lanes) {
            const size_t row = static_cast<size_t>(k) * instances + instance;
            const uint32_t flags = records[row].flags & OALSFX_SAMPLER_PLAYING, eflags = envelopes[row].flags & OALSFX_ENV_ACTIVE;
            busy |= (flags | eflags) != 0 ? 1U << k : 0U;
        }
    }
    const bool add = lanes >= 2;
    // (at one lane the voice's spans store every frame of the row themselves; an idle voice's row is filled here)
    if (add || busy == 0) store_zeros<C, V>(out, 0U, frames, lane);
    for (int k = 0; k < lanes; ++k) {
        if (!(busy >> k & 1U)) continue;
        const size_t row = static_cast<size_t>(k) * instances + instance;
        if (add) program_row<C, V, AddSink, false>(records + row, envelopes + row, programs + row, resamplers[row], tables, out, frames, lane);
        else program_row<C, V, StoreSink, false>(records + row, envelopes + row, programs + row, resamplers[row], tables, out, frames, lane);
    }
}

// The queues oalsfx_batch_set_env_programs has written since the last render, put in place in front of it: a thread per 16-byte piece.
__global__ __launch_bounds__(256) void k_program_upload(EnvProgram* programs, const int* __restrict__ index, const EnvProgram* __restrict__ changed, int count)
{
    constexpr unsigned kPieces = sizeof(EnvProgram) / 16;
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned k = g / kPieces, piece = g % kPieces;
    if (k >= static_cast<unsigned>(count)) return;
    const uint32_t* const from = reinterpret_cast<const uint32_t*>(changed + k) + piece * 4U;
    uint32_t* const to = reinterpret_cast<uint32_t*>(programs + index[k]) + piece * 4U;
#pragma unroll
    for (int i = 0; i < 4; ++i) to[i] = from[i];
}

bool launch_program(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, EnvProgram* programs, const FirTables& tables, int instances,
                    int lanes, unsigned frames, int channels, float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_program_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, programs, tables,
                           dst, instances, lanes, frames);
    });
}

void launch_program_upload(EnvProgram* programs, const int* index, const EnvProgram* changed, int count, hipStream_t stream)
{
    constexpr unsigned kPieces = sizeof(EnvProgram) / 16;
    const unsigned threads = static_cast<unsigned>(count) * kPieces;
    hipLaunchKernelGGL(k_program_upload, dim3((threads + 255U) / 256U), dim3(256), 0, stream, programs, index, changed, count);
}

} // namespace oalsfx_hip
