// The record table (oalsfxpp_amd/csrc/hip/record_table.hpp) against a naive model: a plain array stands for the device's rows, a plain
// array and a flag per row for what the host should know.  Random sequences of set / drain and scatter / render / merge over tables of
// 1, 2, 63, 64, 65 and 200 rows, with an int and an 80-byte struct as the record; the staging arrays are heap blocks of exactly the size
// the header's rule gives and live on from drain to drain as the runtime's buffer does, so that under AddressSanitizer a drain that
// writes past them ends the run.  Built by tests/test_record_table.py.  Prints "ok <sequences> <drains> <drains with nothing pending>
// <merges>", or what went wrong, and exits 0 / 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "record_table.hpp"

namespace {

struct Wide { // the size of a sampler's record
    uint64_t word[10];
    bool operator==(const Wide& o) const
    {
        for (int k = 0; k < 10; ++k)
            if (word[k] != o.word[k]) return false;
        return true;
    }
    bool operator!=(const Wide& o) const { return !(*this == o); }
};
static_assert(sizeof(Wide) == 80, "an 80-byte record");

void make(std::mt19937_64& rng, int& v) { v = static_cast<int>(rng()); }
void make(std::mt19937_64& rng, Wide& v)
{
    for (uint64_t& w : v.word) w = rng();
}

long long g_drains = 0, g_empty_drains = 0, g_merges = 0;

#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("failed: %s (n = %d, sequence %d): ", #cond, n, seq);   \
            std::printf(__VA_ARGS__);                                           \
            std::printf("\n");                                                  \
            return false;                                                       \
        }                                                                       \
    } while (0)

template <class T>
bool sequence(int n, int seq, std::mt19937_64& rng)
{
    const auto below = [&](int m) { return static_cast<int>(rng() % static_cast<uint64_t>(m)); };
    T init;
    make(rng, init);
    oalsfx_records::RecordTable<T> table;
    table.assign(n, init);
    std::vector<T> device(n, init), host(n, init); // the model: the device's rows, and what the host should hold
    std::vector<char> marked(n, 0);                // ... and which rows were set since the last drain
    size_t capacity = 0;
    std::unique_ptr<T[]> changed;
    std::unique_ptr<int[]> index;
    CHECK(table.pending() == 0 && table.host.size() == static_cast<size_t>(n), "a new table");
    const int ops = 8 + below(40);
    for (int op = 0; op < ops; ++op) {
        const int what = below(10);
        if (what < 5) {
            // set: a few rows, one of them twice in a row now and then; or every row
            const int rows = below(8) == 0 ? n : 1 + below(std::min(n, 6));
            for (int k = 0; k < rows; ++k) {
                const int i = rows == n ? k : below(n);
                for (int again = below(4) == 0 ? 2 : 1; again > 0; --again) {
                    T v;
                    make(rng, v);
                    table.set(i, v);
                    host[i] = v;
                    marked[i] = 1;
                }
            }
        } else if (what < 8) {
            // drain, and scatter as the upload kernel does
            size_t count = 0;
            for (int i = 0; i < n; ++i) count += marked[i];
            CHECK(table.pending() == count, "%zu rows pending, %zu distinct rows set", table.pending(), count);
            const size_t wanted = table.staging_capacity(capacity);
            CHECK(wanted >= count && wanted <= static_cast<size_t>(n), "capacity %zu for %zu rows", wanted, count);
            CHECK(count > capacity || wanted == capacity, "a buffer of %zu that holds %zu rows is replaced by one of %zu", capacity, count, wanted);
            CHECK(count <= capacity || wanted == std::min<size_t>(n, std::max<size_t>(2 * count, 64)), "capacity %zu for %zu rows", wanted, count);
            if (wanted != capacity) {
                changed.reset(new T[wanted]);
                index.reset(new int[wanted]);
                capacity = wanted;
            }
            T mark;
            make(rng, mark);
            for (size_t k = 0; k < capacity; ++k) { changed[k] = mark; index[k] = -7; }
            table.drain(changed.get(), index.get());
            ++g_drains;
            if (count == 0) ++g_empty_drains;
            CHECK(table.pending() == 0, "rows pending after a drain");
            std::vector<char> seen(n, 0);
            for (size_t k = 0; k < count; ++k) {
                const int i = index[k];
                CHECK(i >= 0 && i < n && marked[i], "entry %zu names row %d, which was not set", k, i);
                CHECK(!seen[i], "row %d is listed twice", i);
                seen[i] = 1;
                device[i] = changed[k];
            }
            // (with nothing pending that is every entry: the drain has written nothing)
            for (size_t k = count; k < capacity; ++k) CHECK(index[k] == -7 && changed[k] == mark, "entry %zu behind the %zu drained was written", k, count);
            for (int i = 0; i < n; ++i) {
                CHECK(!marked[i] || (device[i] == host[i] && table.host[i] == host[i]), "row %d on the device is not the host's after the scatter", i);
                marked[i] = 0;
            }
        } else if (what < 9) {
            // a render: the device advances some of its rows
            for (int k = 1 + below(n); k > 0; --k) make(rng, device[below(n)]);
        } else {
            const std::vector<T> before = table.host;
            table.merge(device.data());
            ++g_merges;
            for (int i = 0; i < n; ++i) {
                if (marked[i]) CHECK(table.host[i] == before[i] && before[i] == host[i], "row %d was set since the drain and did not keep the host's value", i);
                else {
                    CHECK(table.host[i] == device[i], "row %d is not the device's after the merge", i);
                    host[i] = device[i];
                }
            }
        }
        for (int i = 0; i < n; ++i) CHECK(table.host[i] == host[i], "row %d differs from the model after operation %d", i, op);
    }
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937_64 rng(20240611);
    int total = 0;
    for (int n : {1, 2, 63, 64, 65, 200})
        for (int seq = 0; seq < sequences; ++seq) {
            if (!sequence<int>(n, seq, rng) || !sequence<Wide>(n, seq, rng)) return 1;
            total += 2;
        }
    std::printf("ok %d %lld %lld %lld\n", total, g_drains, g_empty_drains, g_merges);
    return 0;
}
