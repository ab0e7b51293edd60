// k_downmix_ramp_chunks and DownmixTable::build on the host: oalsfxpp_amd/csrc/hip/bus_sends.hip and the table builder of downmix.hip
// compiled by a host compiler behind the shim below (the one of mix_rows_host.cpp), the lanes of a wavefront run one after the other.  The
// kernel has no LDS, no cross-lane operation and no barrier, and a lane owns its elements from load to store: then a lane's values are
// what the device's lane computes.  A host build under AddressSanitizer sees every address the kernel forms: the source, the buses, the
// partials and the four arrays of the table are heap blocks of exactly their size.  Level 2 -- downmix.hip's kernel, which this change
// leaves alone and which needs the device compiler's vector types -- is restated here in three lines from the table's sums.
// (tests/test_sends_host.py writes the job, runs this program and compares what it leaves with tests/sends_ref.py.)
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define OALSFX_FIR_HOST_SHIM 1
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
static dim3 threadIdx, blockIdx, blockDim;
#define hipLaunchKernelGGL(kernel, grid, block, shared, stream, ...)                          \
    do {                                                                                      \
        const dim3 grid_ = (grid), block_ = (block);                                          \
        blockDim = block_;                                                                    \
        for (unsigned b_ = 0; b_ < grid_.x; ++b_)                                             \
            for (unsigned t_ = block_.x; t_-- > 0;) {                                         \
                blockIdx.x = b_;                                                              \
                threadIdx.x = t_;                                                             \
                kernel(__VA_ARGS__);                                                          \
            }                                                                                 \
    } while (0)

#include "downmix.hip"
#include "bus_sends.hip"

namespace {

bool read_all(std::FILE* f, void* to, size_t bytes) { return bytes == 0 || std::fread(to, 1, bytes, f) == bytes; }

// A heap block of exactly the vector's bytes (never null: an empty array is a block of one byte nobody may read).
template <typename T>
T* exact_copy(const std::vector<T>& v)
{
    T* block = static_cast<T*>(std::malloc(v.empty() ? 1 : v.size() * sizeof(T)));
    if (block && !v.empty()) std::memcpy(block, v.data(), v.size() * sizeof(T));
    return block;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

} // namespace

// bus_sends_host <job> <result>.  The job, little-endian: int32 instances, buses, channels, calls, max_vector, offset in floats; int32
// frames[calls]; then [sends][instances] each: int32 bus, float gain, DownmixRamp (frames == 0: the send does not ramp); then for every
// call the source [instances][frames][channels].  The table is built once; call k runs with `since` = the frames of the calls before it.
// The result: for every call the buses [buses][frames][channels].
int main(int argc, char** argv)
{
    using oalsfx_hip::DownmixRamp;
    CHECK(argc == 3, "usage: bus_sends_host <job> <result>");
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in, "cannot open %s", argv[1]);
    int32_t head[6];
    CHECK(read_all(in, head, sizeof(head)), "short job");
    const int n = head[0], buses = head[1], channels = head[2], calls = head[3], max_vector = head[4], offset = head[5];
    CHECK(n >= 1 && buses >= 1 && channels >= 1 && calls >= 1 && offset >= 0 && offset < 4, "bad job");
    std::vector<int32_t> frames(calls);
    CHECK(read_all(in, frames.data(), calls * sizeof(int32_t)), "short job");
    const size_t all = static_cast<size_t>(OALSFX_BUS_SENDS) * n;
    std::vector<int> bus(all);
    std::vector<float> gain(all);
    std::vector<DownmixRamp> ramp(all);
    static_assert(sizeof(DownmixRamp) == 20, "the job's rows are five words");
    CHECK(read_all(in, bus.data(), all * sizeof(int)) && read_all(in, gain.data(), all * sizeof(float)) && read_all(in, ramp.data(), all * sizeof(DownmixRamp)),
          "short job");
    const int* bus_of[OALSFX_BUS_SENDS];
    const float* gain_of[OALSFX_BUS_SENDS];
    const DownmixRamp* ramp_of[OALSFX_BUS_SENDS];
    for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
        bus_of[s] = bus.data() + static_cast<size_t>(s) * n;
        gain_of[s] = gain.data() + static_cast<size_t>(s) * n;
        ramp_of[s] = ramp.data() + static_cast<size_t>(s) * n;
        for (int i = 0; i < n; ++i) CHECK(bus_of[s][i] >= -1 && bus_of[s][i] < buses && ramp_of[s][i].done <= ramp_of[s][i].frames, "bad send");
    }
    oalsfx_hip::DownmixTable table, plain;
    table.build(bus_of, gain_of, ramp_of, n, buses);
    plain.build(bus_of, gain_of, nullptr, n, buses);
    // with and without ramp rows: the same members in the same chunks
    CHECK(plain.ramps.empty() && table.ramps.size() == table.members.size() && plain.members == table.members && plain.chunks.size() == table.chunks.size() &&
          plain.sums.size() == table.sums.size() && plain.partial_rows == table.partial_rows, "the two tables differ");
    for (size_t k = 0; k < table.chunks.size(); ++k)
        CHECK(std::memcmp(&table.chunks[k], &plain.chunks[k], sizeof(table.chunks[k])) == 0 && table.chunks[k].count >= 1 &&
              table.chunks[k].count <= OALSFX_DOWNMIX_CHUNK, "chunk %zu", k);
    size_t at[5];
    std::vector<char> packed(table.packed_bytes(at) + 1);
    table.pack(packed.data());
    CHECK(at[4] % 16 == 0 && (table.ramps.empty() || std::memcmp(packed.data() + at[4], table.ramps.data(), table.ramps.size() * sizeof(DownmixRamp)) == 0), "pack");

    oalsfx_hip::DownmixChunk* const chunks = exact_copy(table.chunks);
    int* const members = exact_copy(table.members);
    DownmixRamp* const ramps = exact_copy(table.ramps);
    CHECK(chunks && members && ramps, "malloc");
    oalsfx_hip::DownmixDevice dev;
    dev.chunks = chunks;
    dev.members = members;
    dev.ramps = ramps;
    dev.n_chunks = static_cast<int>(table.chunks.size());
    dev.n_sums = static_cast<int>(table.sums.size());

    std::FILE* out = std::fopen(argv[2], "wb");
    CHECK(out, "cannot open %s", argv[2]);
    unsigned long long since = 0;
    for (int k = 0; k < calls; ++k) {
        const size_t elements = static_cast<size_t>(frames[k]) * channels;
        // (blocks of exactly the arrays' sizes, `offset` floats off a 16-byte boundary: the width the runtime would take is taken)
        float* const src_block = static_cast<float*>(std::malloc((n * elements + offset) * sizeof(float)));
        float* const dst_block = static_cast<float*>(std::malloc((buses * elements + offset) * sizeof(float)));
        float* const partials = static_cast<float*>(std::malloc(table.partial_rows ? table.partial_rows * elements * sizeof(float) : 1));
        CHECK(src_block && dst_block && partials, "malloc");
        float* const src = src_block + offset;
        float* const dst = dst_block + offset;
        CHECK(read_all(in, src, n * elements * sizeof(float)), "short job");
        for (size_t e = 0; e < buses * elements; ++e) dst[e] = -7.0F;
        for (size_t e = 0; e < table.partial_rows * elements; ++e) partials[e] = -7.0F;
        const int vector = oalsfx_hip::downmix_vector(src, dst, elements, max_vector);
        CHECK(oalsfx_hip::downmix_fits(dev, elements, vector), "too large");
        oalsfx_hip::launch_ramp_chunks(dev, src, dst, partials, elements, channels, since, vector, nullptr);
        // level 2: a bus of no or several chunks is the sum of its partial rows in order, from +0.0f
        for (const oalsfx_hip::DownmixSum& s : table.sums)
            for (size_t e = 0; e < elements; ++e) {
                float total = 0.0F;
                for (int r = 0; r < s.rows; ++r) total = total + partials[static_cast<size_t>(s.first_row + r) * elements + e];
                dst[static_cast<size_t>(s.bus) * elements + e] = total;
            }
        CHECK(std::fwrite(&vector, sizeof(int), 1, out) == 1 && std::fwrite(dst, sizeof(float), buses * elements, out) == buses * elements, "short write");
        since += static_cast<unsigned long long>(frames[k]);
        std::free(src_block);
        std::free(dst_block);
        std::free(partials);
    }
    std::fclose(in);
    std::fclose(out);
    std::free(chunks);
    std::free(members);
    std::free(ramps);
    std::printf("ok\n");
    return 0;
}
