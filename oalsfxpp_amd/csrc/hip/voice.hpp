// Voice envelopes (batch.cpp: sampler_queue): the launchers of voice.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("voice
// envelopes"): per instance a second record beside the sampler's -- a delay in frames, a gain ramp per output channel, a fade that stops
// the voice, a pitch glide at positions of 16 more fractional bits --; a render writes [instance][frame][channel] and advances both records.
// The render's arithmetic is the row body voice_rows_body.hpp, which voice.hip compiles without tables.
#ifndef OALSFX_HIP_VOICE_HPP
#define OALSFX_HIP_VOICE_HPP

// (voice.hip is also compiled for the host, behind a shim that stands in for the runtime: tests/cpp/fir_rows_host.cpp)
#ifndef OALSFX_FIR_HOST_SHIM
#include <hip/hip_runtime.h>
#endif

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// k_sampler_rows' launch with the envelopes beside the records: a row whose envelope is not ACTIVE gets k_sampler_rows' bits.  Store
// width and grid as sampler_vector and sampler_fits (sampler.hpp) have them.  1 <= frames <= 2^24.  False, with nothing launched, for a
// channel count no format has.
bool launch_voice(oalsfx_sampler* records, oalsfx_envelope* envelopes, int rows, unsigned frames, int channels, float* dst, hipStream_t stream);
// envelopes[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_voice_upload(oalsfx_envelope* envelopes, const int* index, const oalsfx_envelope* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
