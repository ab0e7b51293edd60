// Resamplers (batch.cpp: sampler_queue): the launchers of resample.hip.  The arithmetic is the contract of include/oalsfx_hip.h
// ("resamplers"): per instance a table index beside the sampler's record and the envelope; a row that names a table takes the value of a
// frame from a 4- or 8-tap FIR whose coefficients the frame's phase selects; a row that names none is rendered as k_voice_rows renders it:
// both kernels compile the one row body, voice_rows_body.hpp.
#ifndef OALSFX_HIP_RESAMPLE_HPP
#define OALSFX_HIP_RESAMPLE_HPP

// (resample.hip is also compiled for the host, behind a shim that stands in for the runtime: tests/cpp/fir_rows_host.cpp)
#ifndef OALSFX_FIR_HOST_SHIM
#include <hip/hip_runtime.h>
#endif

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// The tables of one batch as the kernel gets them, by value in its arguments: coef[t] is [1 << (12 - shift[t])][taps[t]] floats in device
// memory, 32-byte aligned; taps[t] is 4 or 8, or 0 for an empty slot, which no row names.
struct FirTables {
    const float* coef[OALSFX_FIR_TABLES];
    int taps[OALSFX_FIR_TABLES];
    int shift[OALSFX_FIR_TABLES]; // 12 - phase_bits
};

// k_voice_rows' launch with the resamplers beside the records and envelopes: resamplers[r] is a table index or OALSFX_RESAMPLER_NONE.  A
// row without a table gets k_voice_rows' bits.  Store width and grid as sampler_vector and sampler_fits (sampler.hpp) have them.
// frames >= 1.  False, with nothing launched, for a channel count no format has.
bool launch_fir(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int rows, unsigned frames, int channels,
                float* dst, hipStream_t stream);
// resamplers[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_fir_upload(int* resamplers, const int* index, const int* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
