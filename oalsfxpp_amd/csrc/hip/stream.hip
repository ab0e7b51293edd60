// Sampler streams: a voice's queued sampler records take their turn inside one render, at the exact frame, on the device
// (include/oalsfx_hip.h, "sampler streams").  For every voice the render of F frames is the concatenation of spans, each what the
// samplers', envelopes' and resamplers' contracts give a call of that many frames; the polyphony sums the voices' concatenated outputs.
//
// The shape is k_program_rows': one wavefront per INSTANCE, the instance number in a scalar register, the flag words of every voice read
// in front of the first store, the row filled with +0.0f, the voices added lane by lane in ascending order.  Where k_program_rows calls
// program_row, this kernel calls stream_row (stream_rows_body.hpp), which walks the voice's envelope queue and its ring; a voice whose
// ring is empty costs the two words that say so.  A voice whose ring holds an entry is rendered whatever its record says: an idle voice
// that is appended to starts.  At one lane a voice's frames are stored, not added: a lone voice's -0.0f reaches the input as -0.0f.
//
// No LDS, no cross-lane operation, no atomics, no barrier: every element of the row is written and read by one lane only, and every
// lane carries the records from span to span in copies of its own.  The file also compiles for the host, the lanes of a wavefront run
// one after the other.
#include "stream.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

// (the filter stages at their most general -- filters, sweeps, filter programs -- and the row body around them, without their kernels)
#define OALSFX_FILTER_PROGRAM_BODY_ONLY 1
#include "filter_program.hip"
#include "stream_rows_body.hpp"

namespace oalsfx_hip {

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_stream_resources.py)
// Workgroup g, wavefront w: instance g * kRows + w.  C channels, V floats per access (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_stream_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                               EnvProgram* programs, const StreamRing* __restrict__ rings, uint32_t* taken, const FirTables tables,
                                                               float* dst, int instances, int lanes, unsigned frames)
{
    const int instance = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (instance >= instances) return;
    const unsigned lane = threadIdx.x % kWave;
    float* const out = dst + static_cast<size_t>(instance) * frames * C;
    uint32_t busy = 0;
#pragma unroll
    for (int k = 0; k < OALSFX_MAX_POLYPHONY; ++k) {
        if (k < lanes) {
            const size_t row = static_cast<size_t>(k) * instances + instance;
            const uint32_t flags = records[row].flags & OALSFX_SAMPLER_PLAYING, eflags = envelopes[row].flags & OALSFX_ENV_ACTIVE;
            const uint32_t waiting = rings[row].queued - taken[row];
            busy |= (flags | eflags | waiting) != 0 ? 1U << k : 0U;
        }
    }
    const bool add = lanes >= 2;
    // (at one lane the voice's spans store every frame of the row themselves; an idle voice's row is filled here)
    if (add || busy == 0) store_zeros<C, V>(out, 0U, frames, lane);
    for (int k = 0; k < lanes; ++k) {
        if (!(busy >> k & 1U)) continue;
        const size_t row = static_cast<size_t>(k) * instances + instance;
        EnvProgram* const prog = programs ? programs + row : nullptr;
        if (add) stream_row<C, V, AddSink, false>(records + row, envelopes + row, prog, rings + row, taken + row, resamplers[row], tables, out, frames, lane);
        else stream_row<C, V, StoreSink, false>(records + row, envelopes + row, prog, rings + row, taken + row, resamplers[row], tables, out, frames, lane);
    }
}

// k_stream_rows in front of the filter stage at its most general, while any voice filter is ACTIVE: biquad.hip's row body (one wavefront
// per instance, a filtered voice rendered into its instance's scratch row first, C + 2 LDS rows per wavefront, wavefront-scope syncs
// only) with stream_row as the voice's render.  `programs` and `queues` may be null.
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_stream_filter_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                                      oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps, FilterProgram* queues,
                                                                      EnvProgram* programs, const StreamRing* rings, uint32_t* taken, const FirTables tables, float* dst,
                                                                      float* scratch, int instances, int lanes, unsigned frames)
{
    biquad_rows<C, V, true, true, true, true>(records, envelopes, resamplers, filters, programs, sweeps, tables, dst, scratch, instances, lanes, frames, queues, rings,
                                              taken);
}

// The rings oalsfx_batch_set_streams and _append_streams have written since the last render, put in place in front of it: a thread per
// 16-byte piece.  The thread of a row's first piece also looks at `reset`: a row that comes from a set call starts its taken count at 0.
__global__ __launch_bounds__(256) void k_stream_upload(StreamRing* rings, uint32_t* taken, const int* __restrict__ index, const StreamRing* __restrict__ changed,
                                                       int count)
{
    constexpr unsigned kPieces = sizeof(StreamRing) / 16;
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned k = g / kPieces, piece = g % kPieces;
    if (k >= static_cast<unsigned>(count)) return;
    const uint32_t* const from = reinterpret_cast<const uint32_t*>(changed + k) + piece * 4U;
    uint32_t* const to = reinterpret_cast<uint32_t*>(rings + index[k]) + piece * 4U;
#pragma unroll
    for (int i = 0; i < 4; ++i) to[i] = piece == 0U && i == 1 ? 0U : from[i];
    if (piece == 0U && from[1] != 0U) taken[index[k]] = 0U;
}

bool launch_stream(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, EnvProgram* programs, const StreamRing* rings, uint32_t* taken,
                   const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_stream_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, programs, rings, taken,
                           tables, dst, instances, lanes, frames);
    });
}

bool launch_stream_filter(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                          FilterProgram* queues, EnvProgram* programs, const StreamRing* rings, uint32_t* taken, const FirTables& tables, int instances, int lanes,
                          unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_stream_filter_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, filters, sweeps,
                           queues, programs, rings, taken, tables, dst, scratch, instances, lanes, frames);
    });
}

void launch_stream_upload(StreamRing* rings, uint32_t* taken, const int* index, const StreamRing* changed, int count, hipStream_t stream)
{
    constexpr unsigned kPieces = sizeof(StreamRing) / 16;
    const unsigned threads = static_cast<unsigned>(count) * kPieces;
    hipLaunchKernelGGL(k_stream_upload, dim3((threads + 255U) / 256U), dim3(256), 0, stream, rings, taken, index, changed, count);
}

} // namespace oalsfx_hip
