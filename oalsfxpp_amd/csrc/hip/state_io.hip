// Instance state snapshot / restore (batch.cpp: oalsfx_batch_snapshot, oalsfx_batch_restore, oalsfx_batch_reset): one segmented copy
// kernel that moves a set of instances' records and delay lines between their scattered places in the batch and one contiguous blob, and
// the small fix-up of the restored states' update stamps behind it.
#include "common.hpp"
#include "state_io.hpp"

namespace oalsfx_hip {

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4; // loads in flight per lane before the first store of a round

// Workgroup g copies piece g: bytes [(g - first_piece) * kStatePieceBytes, ... + kStatePieceBytes) of segment piece_seg[g], found with one
// load (a binary search over the segments would take 14 dependent loads for a 4096-instance snapshot, about as long as the copy of a
// piece).  16 bytes per lane and access; a round issues all its loads before its first store.  A null source fills with zeros.
// `nontemporal`: the stores bypass the caches' normal allocation (the blob of a snapshot is not read again by this launch or the ones
// behind it).  Both memory kinds of the batch (ordinary and uncached) and
// page-locked host memory are addressed the same way.
__global__ __launch_bounds__(kCopyThreads) void k_state_copy(const StateSegment* __restrict__ segs, const unsigned* __restrict__ piece_seg, int nontemporal)
{
    const unsigned long long piece = blockIdx.x;
    const StateSegment s = segs[piece_seg[piece]];
    const unsigned long long off = (piece - s.first_piece) * kStatePieceBytes;
    if (off >= s.bytes) return;
    const unsigned long long left = s.bytes - off;
    const int n16 = static_cast<int>((left < kStatePieceBytes ? left : kStatePieceBytes) >> 4);
    const v4u* src = s.src ? reinterpret_cast<const v4u*>(static_cast<const char*>(s.src) + off) : nullptr;
    v4u* dst = reinterpret_cast<v4u*>(static_cast<char*>(s.dst) + off);
    const int t = threadIdx.x;
    for (int base = 0; base < n16; base += kCopyThreads * kCopyUnroll) {
        v4u v[kCopyUnroll];
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j) {
            const int i = base + j * kCopyThreads + t;
            v[j] = (src && i < n16) ? src[i] : v4u{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j) {
            const int i = base + j * kCopyThreads + t;
            if (i < n16) {
                if (nontemporal) __builtin_nontemporal_store(v[j], dst + i);
                else dst[i] = v[j];
            }
        }
    }
}

// One thread per restored slot: the state's seen_seq becomes the slot's new update_seq where the state had folded in the parameters it
// was snapshotted with (its stamp equals their old update_seq), else one less -- the next launch then folds them in, as the source's would.
__global__ __launch_bounds__(256) void k_state_seen_fix(const StateSeenFix* __restrict__ fixes, int count)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const StateSeenFix f = fixes[k];
    const bool seen = f.blob_seen != nullptr && *f.blob_seen == f.old_seq;
    *f.dst_seen = seen ? f.new_seq : f.new_seq - 1u;
}

} // namespace

void launch_state_copy(const StateSegment* segs, const unsigned* piece_seg, unsigned long long pieces, bool nontemporal, hipStream_t stream)
{
    if (pieces == 0) return;
    hipLaunchKernelGGL(k_state_copy, dim3(static_cast<unsigned>(pieces)), dim3(kCopyThreads), 0, stream, segs, piece_seg, nontemporal ? 1 : 0);
}

void launch_state_seen_fix(const StateSeenFix* fixes, int count, hipStream_t stream)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_state_seen_fix, dim3((count + 255) / 256), dim3(256), 0, stream, fixes, count);
}

} // namespace oalsfx_hip
