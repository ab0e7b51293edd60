// Polyphony: several voices per instance, summed into the instance's input.  For instance i, frame f, channel c the row gets
// (((+0.0f + o_0) + o_1) + ...) + o_(K-1), o_k what the voice (lane k, instance i) renders by itself (include/oalsfx_hip.h, "polyphony"):
// lanes ascending, every addition rounded by itself, a voice's last product not fused into it.
//
// The shape is k_fir_rows': one wavefront per INSTANCE, the instance number in a scalar register, so that every voice's two records, its
// table index and the table's descriptor are the same in every lane and every branch on them is wave-uniform (the flag words in front
// of the first store and the table's index and descriptor are scalar loads; the records of a voice that plays are read behind the
// row's stores, where the compiler takes a uniform vector load and readfirstlane instead).  The wavefront fills its row with +0.0f,
// then walks the lanes k = 0 ... K - 1 at the rows k * instances + i; each voice runs the row body k_fir_rows runs
// (voice_rows_body.hpp) with AddSink: a frame is added to the row, not stored.  A voice that neither plays nor has an active envelope
// costs two scalar loads and a bit test; one that plays nothing in this call moves its counters and touches neither the row nor an
// asset.
//
// The sum needs no barrier, fence, atomic or LDS, because every element of the row is written and read by one lane only, lane
// (f mod 64) of the instance's wavefront, from the zero fill to the last voice: store_zeros owns the frames that way, and voice_row
// turns the lane number it gives the render back by the envelope's delay, so that a delayed voice's frames keep their owners.  A
// lane's program order is then all the ordering there is.  There is NO workgroup barrier anywhere in the lane loop, and there must
// not be: the four wavefronts of a workgroup run different instances with different playing lanes.  The file also compiles for the
// host, the lanes of a wavefront run one after the other (tests/cpp/mix_rows_host.cpp) -- which only gives the device's sums if no
// lane reads what another wrote.
#include "polyphony.hpp"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "voice_rows_body.hpp"

namespace oalsfx_hip {

// (names outside the anonymous namespace so that the code object's notes list the kernels: tests/test_polyphony_resources.py)
// Workgroup g, wavefront w: instance g * kRows + w.  C channels, V floats per access (C % V == 0, dst aligned to V floats).
template <int C, int V>
__global__ __launch_bounds__(kWave * kRows) void k_mix_rows(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* __restrict__ resamplers,
                                                            const FirTables tables, float* dst, int instances, int lanes, unsigned frames)
{
    // (the instance number in a scalar register: the fields of every voice's records and the tables' descriptors are the same in every lane)
    const int instance = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kRows + static_cast<int>(threadIdx.x) / kWave);
    if (instance >= instances) return;
    const unsigned lane = threadIdx.x % kWave;
    float* const out = dst + static_cast<size_t>(instance) * frames * C;
    // Which voices have anything to render or a counter to move: both flag words of every lane, read in front of the kernel's first store
    // -- scalar loads, all in flight together -- so that an idle voice costs the loop below a bit test.  (A voice's records are written
    // by its own turn of the loop alone.)
    uint32_t busy = 0;
#pragma unroll
    for (int k = 0; k < OALSFX_MAX_POLYPHONY; ++k) {
        if (k < lanes) {
            const size_t row = static_cast<size_t>(k) * instances + instance;
            const uint32_t flags = records[row].flags & OALSFX_SAMPLER_PLAYING, eflags = envelopes[row].flags & OALSFX_ENV_ACTIVE;
            busy |= (flags | eflags) != 0 ? 1U << k : 0U;
        }
    }
    store_zeros<C, V>(out, 0U, frames, lane);
    for (int k = 0; k < lanes; ++k) {
        if (!(busy >> k & 1U)) continue;
        const size_t row = static_cast<size_t>(k) * instances + instance;
        voice_row<C, V, AddSink>(records + row, envelopes + row, resamplers[row], tables, out, frames, lane);
    }
}

bool launch_mix(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int instances, int lanes, unsigned frames,
                int channels, float* dst, hipStream_t stream)
{
    return launch_rows(channels, dst, instances, [=, &tables](auto c, auto v, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_mix_rows<decltype(c)::value, decltype(v)::value>), grid, block, 0, stream, records, envelopes, resamplers, tables, dst,
                           instances, lanes, frames);
    });
}

} // namespace oalsfx_hip
