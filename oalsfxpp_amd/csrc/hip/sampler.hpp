// Samplers (batch.cpp: oalsfx_batch_sample_device, oalsfx_batch_play_downmix_meter): the launchers of sampler.hip.  The arithmetic is the
// contract of include/oalsfx_hip.h ("samplers"): per instance a record that names an asset in device memory, a fixed-point position and
// step, a loop region, a format and per-channel gains; a render writes [instance][frame][channel] and advances the records.
#ifndef OALSFX_HIP_SAMPLER_HPP
#define OALSFX_HIP_SAMPLER_HPP

#include <hip/hip_runtime.h>

#include <cstddef>

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// Floats one lane stores at once (4, 2 or 1): as wide as the channel count and the destination's address allow.  Every width writes the
// same bits (a lane owns whole frames).
int sampler_vector(const void* dst, int channels);
// Whether `rows` rows fit one launch.
bool sampler_fits(int rows);
// One wavefront per row: dst[r], [frames][channels], is rendered from records[r], which the first lane of the row's wavefront advances.
// frames >= 1.  False, with nothing launched, for a channel count no format has.
bool launch_sampler(oalsfx_sampler* records, int rows, unsigned frames, int channels, float* dst, hipStream_t stream);
// records[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_sampler_upload(oalsfx_sampler* records, const int* index, const oalsfx_sampler* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
