// Voice filter sweeps (batch.cpp: sampler_queue, while a sweep may be under way and a voice's filter is ACTIVE): the launchers of
// sweep.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("voice filter sweeps"): a swept voice's five coefficients are formed
// per frame, from[k] + ((float)n * step[k]) below the sweep's length and to[k] from there on, and the sweep that completes leaves `to` in
// the voice's filter record.
#ifndef OALSFX_HIP_SWEEP_HPP
#define OALSFX_HIP_SWEEP_HPP

#include "program.hpp"

namespace oalsfx_hip {

// launch_biquad with the sweeps beside the four other tables (instances * lanes rows each, lane-major).
bool launch_sweep(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                  const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream);
// ... and launch_program_biquad.
bool launch_program_sweep(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                          EnvProgram* programs, const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch,
                          hipStream_t stream);
// sweeps[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_sweep_upload(oalsfx_filter_sweep* sweeps, const int* index, const oalsfx_filter_sweep* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
