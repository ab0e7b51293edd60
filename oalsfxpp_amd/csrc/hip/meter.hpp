// Level meters (batch.cpp: oalsfx_batch_meter_device, oalsfx_batch_mix_downmix_meter): the launcher of meter.hip.  The arithmetic is the
// contract of include/oalsfx_hip.h ("level meters"): per row and channel the largest |x|, the sum of x * x -- lane l of
// OALSFX_METER_LANES adds its frames f = l, l + 64, ... in ascending order from +0.0f, then the tree s = 32 .. 1 adds lane l + s into lane
// l --, the count of non-finite elements and the trailing run of quiet frames; fp32, product and sum rounded separately.
#ifndef OALSFX_HIP_METER_HPP
#define OALSFX_HIP_METER_HPP

#include <hip/hip_runtime.h>

#include <cstddef>

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// Floats one lane loads at once (4, 2 or 1): as wide as the channel count and the source's address allow.  Every width computes the
// same bits (a lane owns whole frames).
int meter_vector(const void* src, int channels);
// Whether `rows` rows fit one launch.
bool meter_fits(int rows);
// One wavefront per row of src, [rows][frames][channels]; meters[r] is written by the first lane of row r's wavefront, and read first
// where `carry` is set.  frames >= 1.  False, with nothing launched, for a channel count no format has.
bool launch_meter(const float* src, int rows, unsigned frames, int channels, float threshold, bool carry, oalsfx_meter* meters, hipStream_t stream);

} // namespace oalsfx_hip

#endif
