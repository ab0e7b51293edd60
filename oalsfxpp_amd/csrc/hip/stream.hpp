// Sampler streams (batch.cpp: sampler_queue, while a voice's ring may hold an entry): the ring's row, the voices' taken counts and the
// launchers of stream.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("sampler streams"): a voice's render is cut into spans
// at the frames where its current one-shot ends (and, as for the envelope programs, where its current envelope segment completes), each
// span rendered as a call of that many frames, the ring's head taken as the voice's sampler record in between, its position advanced by
// the excess the span ran past the end.
#ifndef OALSFX_HIP_STREAM_HPP
#define OALSFX_HIP_STREAM_HPP

#include "filter_program.hpp"
#include "program.hpp"

namespace oalsfx_hip {

// A voice's ring: the records behind the current one (which is the voice's row of the samplers' table).  The host owns the row and no
// render writes it.  `queued` counts the entries put in since the stream was last set and the device's `taken` (an array of its own, a
// word per voice) those taken since then: entry[taken % OALSFX_STREAM_QUEUE] is the next to be taken, queued - taken of them wait.
// Both run on modulo 2^32, of which the ring's length is a divisor, so that a counter that wraps needs no case of its own.  `reset` is
// looked at by k_stream_upload alone: the row comes from a set call, and the voice's taken count starts at 0 again.
struct StreamRing {
    uint32_t queued;
    uint32_t reset;
    uint32_t reserved[2];
    oalsfx_sampler entry[OALSFX_STREAM_QUEUE];
};
static_assert(sizeof(StreamRing) == 656 && sizeof(StreamRing) % 16 == 0, "a ring row is 41 16-byte pieces (k_stream_upload)");
static_assert((1ULL << 32) % OALSFX_STREAM_QUEUE == 0, "the counters wrap on a multiple of the ring's length");

// k_program_rows' launch with the rings and the taken counts beside the other tables (instances * lanes rows each, lane-major), at any
// lanes >= 1.  `programs` may be null: a table that was never made counts as empty queues.  frames >= 1.  False, with nothing launched,
// for a channel count no format has.
bool launch_stream(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, EnvProgram* programs, const StreamRing* rings, uint32_t* taken,
                   const FirTables& tables, int instances, int lanes, unsigned frames, int channels, float* dst, hipStream_t stream);
// ... and k_filter_program_env_rows' (its filter stage: filters, sweeps, filter programs; scratch: [instances][frames][channels]), while any
// voice filter is ACTIVE.  `programs` and `queues` may be null.
bool launch_stream_filter(oalsfx_sampler* records, oalsfx_envelope* envelopes, const int* resamplers, oalsfx_voice_filter* filters, oalsfx_filter_sweep* sweeps,
                          FilterProgram* queues, EnvProgram* programs, const StreamRing* rings, uint32_t* taken, const FirTables& tables, int instances, int lanes,
                          unsigned frames, int channels, float* dst, float* scratch, hipStream_t stream);
// rings[index[k]] = changed[k] for k < count (index and changed: device-visible memory), and taken[index[k]] = 0 where changed[k].reset is
// set (the device's row keeps reset == 0); count >= 1.
void launch_stream_upload(StreamRing* rings, uint32_t* taken, const int* index, const StreamRing* changed, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
