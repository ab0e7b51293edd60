// Polyphony (batch.cpp: sampler_queue, while the batch has two lanes or more): the launcher of polyphony.hip.  The arithmetic is the
// contract of include/oalsfx_hip.h ("polyphony"): every instance has `lanes` voices, each a sampler's record, an envelope and a table
// index of its own, and a render writes their sum, lanes ascending from +0.0f, every addition rounded by itself.
#ifndef OALSFX_HIP_POLYPHONY_HPP
#define OALSFX_HIP_POLYPHONY_HPP

#include "resample.hpp"

namespace oalsfx_hip {

// k_fir_rows' launch over `lanes` voices per instance: the three tables have instances * lanes rows, lane-major (voice row = lane *
// instances + instance), and dst[i], [frames][channels], becomes the sum of instance i's voices.  One wavefront per instance: store
// width and grid as sampler_vector and sampler_fits (sampler.hpp) have them for `instances` rows.  frames >= 1, lanes >= 1.  False,
// with nothing launched, for a channel count no format has.
bool launch_mix(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, const FirTables& tables, int instances, int lanes, unsigned frames,
                int channels, float* dst, hipStream_t stream);

} // namespace oalsfx_hip

#endif
