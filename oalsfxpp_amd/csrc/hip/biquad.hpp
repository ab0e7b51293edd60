// Voice filters (batch.cpp: sampler_queue, while any voice's filter is ACTIVE): the launchers of biquad.hip.  The arithmetic is the
// contract of include/oalsfx_hip.h ("voice filters"): a voice with an ACTIVE filter is rendered by itself, run through its biquad over
// every frame of the render, and stands with the filter's output where it stood with its own in the instance's input.
#ifndef OALSFX_HIP_BIQUAD_HPP
#define OALSFX_HIP_BIQUAD_HPP

#include "resample.hpp"

namespace oalsfx_hip {

// k_mix_rows' launch with the filters beside the three other tables (instances * lanes rows each, lane-major), at any lanes >= 1.
// scratch: [instances][frames][channels] floats the launch may overwrite, 16-byte aligned, apart from dst.  frames >= 1.  False, with
// nothing launched, for a channel count no format has.
bool launch_biquad(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, const FirTables& tables,
                   int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream);
// filters[index[k]] takes flags (without LOAD) and coefficients of changed[k], and its histories where changed[k] has LOAD, for k < count
// (index and changed: device-visible memory); count >= 1.
void launch_biquad_upload(oalsfx_voice_filter* filters, const int* index, const oalsfx_voice_filter* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
