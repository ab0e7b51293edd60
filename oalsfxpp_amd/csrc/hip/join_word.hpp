// The join word ("calls that join a queued launch"): how a mix_device call that arrives while a chained launch still sits
// behind its gate becomes one more buffer of that launch, with neither side ever waiting for the other.
//
// One JoinSlot per queued launch, in page-locked host memory the device can address.  The slot's 64-bit word is its whole state:
//
//     0                      never used
//     kJoinOpen | count      the host has published `count` buffers (src[k], dst[k], k < count) and may publish more
//     kJoinClosed | count    the gate has taken `count` buffers: nothing joins any more; it is still copying the entries
//     kJoinDone | count      ... and has copied them: the host may use the slot for another launch
//
// The host appends with one compare-and-swap (open, c) -> (open, c + 1), release order: the entry it wrote before is visible to whoever
// reads the count.  The gate closes with one exchange, acquire order, and learns the final count from what it replaced.  The two are
// atomic operations on one word, so every buffer is either counted by the close or told by the failed compare-and-swap to queue a launch
// of its own: never both, never neither.  Nobody spins: an append that fails is final, and a close always succeeds.
//
// Plain C++ and the compilers' __atomic builtins only (system scope in device code), no HIP types: tests/test_join_word.py drives both
// sides from two host threads.
#ifndef OALSFX_JOIN_WORD_HPP
#define OALSFX_JOIN_WORD_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define OALSFX_JOIN_FN __host__ __device__ inline
#else
#define OALSFX_JOIN_FN inline
#endif

namespace oalsfx_join {

constexpr int kMaxBuffers = 32; // (oalsfx_hip::kMaxPassBuffers)
constexpr uint64_t kJoinOpen = 1ull << 63, kJoinClosed = 1ull << 62, kJoinDone = 1ull << 61, kJoinCountMask = 0xFFFFFFFFull;

// What the grid behind the gate reads: the layout of oalsfx_hip::BufferTable (common.hpp asserts it).
struct JoinTable {
    const float* src[kMaxBuffers];
    float* dst[kMaxBuffers];
    int frames;  // per buffer
    int buffers;
};

struct JoinSlot {
    uint64_t word;
    int frames; // per buffer: set when the launch is queued, the same for every buffer that joins
    int pad;
    const float* src[kMaxBuffers];
    float* dst[kMaxBuffers];
};

// ---- the host's side ----
// May the slot take another launch?  (Its last gate has copied what it took, or it never had one.)
OALSFX_JOIN_FN bool join_reusable(const JoinSlot* s)
{
    const uint64_t w = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    return w == 0 || (w & kJoinDone) != 0;
}

// A launch is queued with its own call as buffer 0: before its gate is.
OALSFX_JOIN_FN void join_start(JoinSlot* s, int frames, const float* src, float* dst)
{
    s->frames = frames;
    s->src[0] = src;
    s->dst[0] = dst;
    __atomic_store_n(&s->word, kJoinOpen | 1u, __ATOMIC_RELEASE);
}

// Buffer `count` (the number published so far: only the host appends, so it knows).  False: the launch has closed, this call queues its own.
OALSFX_JOIN_FN bool join_append(JoinSlot* s, unsigned count, const float* src, float* dst)
{
    if (count >= static_cast<unsigned>(kMaxBuffers)) return false;
    s->src[count] = src;
    s->dst[count] = dst;
    uint64_t expected = kJoinOpen | count;
    return __atomic_compare_exchange_n(&s->word, &expected, kJoinOpen | (count + 1u), false, __ATOMIC_RELEASE, __ATOMIC_RELAXED);
}

// ---- the gate's side ----
// Closes the launch, once, and returns how many buffers it has (0: the word was not open -- a launch is never queued that way).
OALSFX_JOIN_FN unsigned join_close(JoinSlot* s)
{
    const uint64_t old = __atomic_exchange_n(&s->word, kJoinClosed, __ATOMIC_ACQUIRE);
    return (old & kJoinOpen) ? static_cast<unsigned>(old & kJoinCountMask) : 0u;
}

// Entry k of the closed launch into the table its grid reads (any order, any number of lanes: k < what join_close returned).
OALSFX_JOIN_FN void join_copy_entry(const JoinSlot* s, JoinTable* t, unsigned k)
{
    t->src[k] = s->src[k];
    t->dst[k] = s->dst[k];
}

OALSFX_JOIN_FN void join_copy_sizes(const JoinSlot* s, JoinTable* t, unsigned count)
{
    t->frames = s->frames;
    t->buffers = static_cast<int>(count);
}

// The entries are copied: the slot is the host's again.
OALSFX_JOIN_FN void join_done(JoinSlot* s, unsigned count)
{
    __atomic_store_n(&s->word, kJoinDone | count, __ATOMIC_RELEASE);
}

} // namespace oalsfx_join

#endif // OALSFX_JOIN_WORD_HPP
