// Filter programs (batch.cpp: sampler_queue, while a voice's filter program may hold a queued segment and a voice's filter is ACTIVE): the
// queue's row and the launchers of filter_program.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("filter programs"): a
// voice's filter stage is cut into spans at the frames where its current sweep completes, each span filtered as a render of that many
// frames under "voice filter sweeps", the head of the queue taken as the current sweep in between.
#ifndef OALSFX_HIP_FILTER_PROGRAM_HPP
#define OALSFX_HIP_FILTER_PROGRAM_HPP

#include "sweep.hpp"

namespace oalsfx_hip {

// A voice's queue: the sweeps behind the current one (which is the voice's row of the sweeps' table), queue[head] the next to take its
// place, `count` of them left.  A program is set whole, so head + count never passes the array's end.
struct FilterProgram {
    uint32_t head, count;
    uint32_t reserved[2];
    oalsfx_filter_sweep queue[OALSFX_FILTER_PROGRAM_MAX - 1];
};
static_assert(sizeof(FilterProgram) == 576, "a queue row is 36 16-byte pieces (k_filter_program_upload)");

// launch_sweep with the queues beside the five other tables (instances * lanes rows each, lane-major).
bool launch_filter_program(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                           FilterProgram* queues, const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, float* scratch,
                           hipStream_t stream);
// ... and launch_program_sweep: the envelope programs' queues walked as well.
bool launch_filter_program_env(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                               FilterProgram* queues, EnvProgram* programs, const FirTables& tables, int instances, int lanes, unsigned frames, int channels,
                               float* dst, float* scratch, hipStream_t stream);
// queues[index[k]] = changed[k] for k < count (index and changed: device-visible memory); count >= 1.
void launch_filter_program_upload(FilterProgram* queues, const int* index, const FilterProgram* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
