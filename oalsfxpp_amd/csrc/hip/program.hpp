// Envelope programs (batch.cpp: sampler_queue, while a voice's queue may hold a segment): the queue's row and the launchers of
// program.hip and, for the render with voice filters, biquad.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("envelope
// programs"): a voice's render is cut into spans at the frames where its current segment completes, each span rendered as a call of
// that many frames, the head of the queue taken as the current segment in between.
#ifndef OALSFX_HIP_PROGRAM_HPP
#define OALSFX_HIP_PROGRAM_HPP

#include "resample.hpp"

namespace oalsfx_hip {

// A voice's queue: the segments behind the current one (which is the voice's row of the envelopes' table), queue[head] the next to take
// its place, `count` of them left.  A program is set whole, so head + count never passes the array's end.
struct EnvProgram {
    uint32_t head, count;
    uint32_t reserved[2];
    oalsfx_envelope queue[OALSFX_ENV_PROGRAM_MAX - 1];
};
static_assert(sizeof(EnvProgram) == 1024, "a queue row is 64 16-byte pieces (k_program_upload)");

// k_mix_rows' launch with the queues beside the three other tables (instances * lanes rows each, lane-major), at any lanes >= 1; at one
// lane a voice's frames are stored, as k_fir_rows stores them.  frames >= 1.  False, with nothing launched, for a channel count no format
// has.
bool launch_program(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, EnvProgram* programs, const FirTables& tables, int instances,
                    int lanes, unsigned frames, int channels, float* dst, hipStream_t stream);
// ... and k_biquad_rows' (biquad.hip).
bool launch_program_biquad(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, EnvProgram* programs,
                           const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream);
// programs[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_program_upload(EnvProgram* programs, const int* index, const EnvProgram* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
