// Both sides of the join word (oalsfxpp_amd/csrc/hip/join_word.hpp) on two host threads: one appends buffers as mix_device does, one closes
// at a random moment as the gate does.  Over many rounds every buffer must be counted exactly once -- by the close, or by the append's
// "failed, launch my own" -- and the entries the closer copies must be the ones that were published.  Built by tests/test_join_word.py,
// with -fsanitize=thread where the toolchain has it.  Prints "ok <rounds> <joined> <refused>", or what went wrong, and exits 0 / 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>

#include "join_word.hpp"

using namespace oalsfx_join;

namespace {

// Entry k of round r: addresses nobody dereferences, different for every (round, buffer), so that a stale or torn entry shows.
const float* src_of(unsigned r, unsigned k) { return reinterpret_cast<const float*>(static_cast<uintptr_t>(0x100000000ull + (static_cast<uintptr_t>(r) << 12) + k * 16)); }
float* dst_of(unsigned r, unsigned k) { return reinterpret_cast<float*>(static_cast<uintptr_t>(0x900000000ull + (static_cast<uintptr_t>(r) << 12) + k * 16)); }

struct Round {
    std::atomic<int> go{0};     // the appender has started the slot: the closer may close whenever it likes
    std::atomic<int> closed{0}; // the closer is through
    unsigned taken = 0;         // what the close counted
    bool entries_ok = true;
};

} // namespace

int main(int argc, char** argv)
{
    const unsigned rounds = argc > 1 ? static_cast<unsigned>(std::atoi(argv[1])) : 20000u;
    constexpr int kSlots = 3; // used in turn, as the batch does
    static JoinSlot slots[kSlots];
    static JoinTable tables[kSlots];
    std::memset(slots, 0, sizeof(slots));
    static Round* round = new Round[rounds];
    long long joined_total = 0, refused_total = 0;
    bool failed = false;

    std::thread closer([&] {
        std::mt19937 rng(12345);
        for (unsigned r = 0; r < rounds; ++r) {
            JoinSlot* s = &slots[r % kSlots];
            JoinTable* t = &tables[r % kSlots];
            while (round[r].go.load(std::memory_order_acquire) == 0) std::this_thread::yield();
            // a random moment: at once, after a few spins, or after the appender has had time to fill the table
            const unsigned wait = rng() % 4 == 0 ? 0 : rng() % 2000;
            for (volatile unsigned i = 0; i < wait; ++i) {}
            const unsigned count = join_close(s);
            for (unsigned k = 0; k < count && k < static_cast<unsigned>(kMaxBuffers); ++k) join_copy_entry(s, t, k);
            join_copy_sizes(s, t, count);
            join_done(s, count);
            bool ok = t->buffers == static_cast<int>(count) && t->frames == 256;
            for (unsigned k = 0; k < count && k < static_cast<unsigned>(kMaxBuffers); ++k) ok = ok && t->src[k] == src_of(r, k) && t->dst[k] == dst_of(r, k);
            round[r].taken = count;
            round[r].entries_ok = ok;
            round[r].closed.store(1, std::memory_order_release);
        }
    });

    std::mt19937 rng(54321);
    for (unsigned r = 0; r < rounds && !failed; ++r) {
        JoinSlot* s = &slots[r % kSlots];
        // (the slot's last user -- three rounds ago -- is through: the batch would queue an ordinary launch otherwise, here every round joins)
        if (!join_reusable(s)) { std::printf("round %u: slot not handed back\n", r); failed = true; break; }
        join_start(s, 256, src_of(r, 0), dst_of(r, 0));
        round[r].go.store(1, std::memory_order_release);
        unsigned count = 1, refused = 0;
        const unsigned want = 1 + rng() % kMaxBuffers; // buffers this round offers in all (up to a full table)
        for (unsigned k = 1; k < want; ++k) {
            if (refused == 0 && join_append(s, count, src_of(r, count), dst_of(r, count))) ++count;
            else ++refused; // (closed: this one and every later one queue launches of their own)
        }
        while (round[r].closed.load(std::memory_order_acquire) == 0) std::this_thread::yield();
        // every buffer counted once: the appender's successes are exactly what the close took
        if (round[r].taken != count || !round[r].entries_ok || count + refused != want) {
            std::printf("round %u: appended %u, refused %u of %u, the close took %u, entries %s\n", r, count, refused, want, round[r].taken,
                        round[r].entries_ok ? "ok" : "WRONG");
            failed = true;
        }
        // a closed launch stays closed
        if (join_append(s, count, src_of(r, count), dst_of(r, count))) { std::printf("round %u: an append after the close succeeded\n", r); failed = true; }
        joined_total += count - 1;
        refused_total += refused;
    }
    if (failed) {
        // (the closer may be waiting for a round that never starts)
        for (unsigned r = 0; r < rounds; ++r) round[r].go.store(1, std::memory_order_release);
    }
    closer.join();
    if (failed) return 1;
    std::printf("ok %u %lld %lld\n", rounds, joined_total, refused_total);
    return 0;
}
