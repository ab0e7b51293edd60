// Launchers of state_io.hip and the tables they read (built per call by batch.cpp, in device memory).
#ifndef OALSFX_HIP_STATE_IO_HPP
#define OALSFX_HIP_STATE_IO_HPP

#include <hip/hip_runtime.h>

namespace oalsfx_hip {

// One piece of work of k_state_copy: 64 KiB of one segment.
constexpr unsigned long long kStatePieceBytes = 64 * 1024;

// `bytes` from `src` to `dst`; src == nullptr: zeros.  Addresses and byte counts are multiples of 16.  first_piece: the sum of
// ceil(bytes / kStatePieceBytes) over the segments before this one (the table is in that order).
struct StateSegment {
    const void* src;
    void* dst;
    unsigned long long bytes;
    unsigned long long first_piece;
};

// *dst_seen = (blob_seen && *blob_seen == old_seq) ? new_seq : new_seq - 1
struct StateSeenFix {
    unsigned* dst_seen;
    const unsigned* blob_seen;
    unsigned old_seq;
    unsigned new_seq;
};

// One launch for every segment of the table (`pieces`: the pieces of all of them; piece_seg[g]: the segment piece g belongs to).
void launch_state_copy(const StateSegment* segs, const unsigned* piece_seg, unsigned long long pieces, bool nontemporal, hipStream_t stream);
void launch_state_seen_fix(const StateSeenFix* fixes, int count, hipStream_t stream);

} // namespace oalsfx_hip

#endif
