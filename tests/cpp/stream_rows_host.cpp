// k_stream_rows on the host: oalsfxpp_amd/csrc/hip/stream.hip compiled by a host compiler behind the shim below (the one of
// program_rows_host.cpp).  The kernel runs its lanes one after the other, each through all of its instance's voices and all of their
// spans, lane 0 last.  That stands in for the device because of how the sequenced row body keeps the records between spans
// (stream_rows_body.hpp): every lane carries what the spans change in registers of its own -- the taken count and the excess among
// them --, reads from memory only what no lane writes before the voice's last span is done -- the records as the kernel found them, the
// ring's and the queue's entries, the taken count as it was --, and lane 0 alone writes, once, behind its own last span.  A body in which a
// lane read back what lane 0 had stored would see here, in the lanes 63 .. 1, records no span has advanced yet: wrong bits, which the
// comparison with the restatement shows.  A host build under AddressSanitizer sees every address the kernel forms: every record's PCM --
// every chunk by itself --, the output, the records, the rings, the queues and the taken counts are heap blocks of exactly their size, so
// a frame read past a chunk's end or in front of its start is an error and not the neighbouring chunk.  (tests/test_stream_host.py
// writes the job, runs this program and compares what it leaves with the restatement.)
//
// The shim: __global__ and __device__ mean nothing, threadIdx / blockIdx / blockDim are globals the launch macro sets, readfirstlane is
// the identity, and a launch calls the kernel for every thread, blocks ascending, a block's threads in DESCENDING order.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define OALSFX_FIR_HOST_SHIM 1
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(threads)
#define __builtin_amdgcn_readfirstlane(x) (x)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
struct alignas(16) float4 { float x, y, z, w; };
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

#include "stream.hip"

namespace {

bool read_all(std::FILE* f, void* to, size_t bytes) { return bytes == 0 || std::fread(to, 1, bytes, f) == bytes; }

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

} // namespace

// stream_rows_host <job> <result>.  The job, little-endian: int32 instances, lanes, channels, calls, PCM blocks, dst offset in floats, and
// whether there is a queue table (0: the kernel is handed a null pointer); int32 frames[calls]; for each of the 8 tables int32 taps,
// phase_bits and the coefficients; for each PCM block int64 bytes and the bytes; then for the instances * lanes voices, lane-major: int32
// block of every voice's record (-1: none), the records, the envelopes, the resamplers, the queues, int32 block of every ring entry
// [voices][8], the rings; then behind every call int32 appends and for each int32 voice, int32 count and count times (int32 block, the
// record), which go into the ring as oalsfx_batch_append_streams puts them.  The result: for every call the output
// [instances][frames][channels], the records, the envelopes, the queues, the rings and the taken counts behind it (a record's data is
// this process's address of its block).
int main(int argc, char** argv)
{
    CHECK(argc == 3, "usage: stream_rows_host <job> <result>");
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in, "cannot open %s", argv[1]);
    int32_t head[7];
    CHECK(read_all(in, head, sizeof(head)), "short job");
    const int instances = head[0], lanes = head[1], channels = head[2], calls = head[3], n_blocks = head[4], offset = head[5];
    const bool queued = head[6] != 0;
    CHECK(instances >= 1 && lanes >= 1 && lanes <= OALSFX_MAX_POLYPHONY && calls >= 1 && n_blocks >= 0 && offset >= 0, "bad job");
    const int rows = instances * lanes;
    std::vector<int32_t> frames(calls);
    CHECK(read_all(in, frames.data(), calls * sizeof(int32_t)), "short job");
    oalsfx_hip::FirTables tables = {};
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) {
        int32_t shape[2];
        CHECK(read_all(in, shape, sizeof(shape)), "short job");
        if (!shape[0]) continue;
        CHECK((shape[0] == 4 || shape[0] == 8) && shape[1] >= 0 && shape[1] <= OALSFX_SAMPLER_FRAC_BITS, "table %d: bad shape", t);
        const size_t bytes = (size_t{1} << shape[1]) * shape[0] * sizeof(float);
        float* coef = static_cast<float*>(std::aligned_alloc(16, bytes)); // (exactly its size: a phase past the table is an error too)
        CHECK(coef && read_all(in, coef, bytes), "short job");
        tables.coef[t] = coef;
        tables.taps[t] = shape[0];
        tables.shift[t] = OALSFX_SAMPLER_FRAC_BITS - shape[1];
    }
    std::vector<void*> blocks(n_blocks, nullptr);
    for (int a = 0; a < n_blocks; ++a) {
        int64_t bytes = 0;
        CHECK(read_all(in, &bytes, sizeof(bytes)) && bytes > 0, "short job");
        blocks[a] = std::malloc(static_cast<size_t>(bytes));
        CHECK(blocks[a] && read_all(in, blocks[a], static_cast<size_t>(bytes)), "short job");
    }
    const auto placed = [&](oalsfx_sampler& r, int32_t block) {
        if (block < -1 || block >= n_blocks) return false;
        r.data = block < 0 ? 0 : reinterpret_cast<uint64_t>(blocks[block]);
        return true;
    };
    std::vector<int32_t> block_of(rows), resamplers(rows), ring_block(static_cast<size_t>(rows) * OALSFX_STREAM_QUEUE);
    std::vector<oalsfx_sampler> records(rows);
    std::vector<oalsfx_envelope> envelopes(rows);
    std::vector<oalsfx_hip::EnvProgram> programs(rows);
    std::vector<oalsfx_hip::StreamRing> rings(rows);
    std::vector<uint32_t> taken(rows, 0U);
    CHECK(read_all(in, block_of.data(), rows * sizeof(int32_t)) && read_all(in, records.data(), rows * sizeof(oalsfx_sampler)) &&
          read_all(in, envelopes.data(), rows * sizeof(oalsfx_envelope)) && read_all(in, resamplers.data(), rows * sizeof(int32_t)) &&
          read_all(in, programs.data(), rows * sizeof(oalsfx_hip::EnvProgram)) && read_all(in, ring_block.data(), ring_block.size() * sizeof(int32_t)) &&
          read_all(in, rings.data(), rows * sizeof(oalsfx_hip::StreamRing)), "short job");
    for (int r = 0; r < rows; ++r) {
        CHECK(placed(records[r], block_of[r]), "bad block number");
        CHECK(rings[r].queued <= OALSFX_STREAM_QUEUE, "bad ring");
        for (int j = 0; j < OALSFX_STREAM_QUEUE; ++j) CHECK(placed(rings[r].entry[j], ring_block[static_cast<size_t>(r) * OALSFX_STREAM_QUEUE + j]), "bad block number");
        CHECK(resamplers[r] >= -1 && resamplers[r] < OALSFX_FIR_TABLES && (resamplers[r] < 0 || tables.taps[resamplers[r]]), "bad resampler");
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    CHECK(out, "cannot open %s", argv[2]);
    for (int k = 0; k < calls; ++k) {
        const size_t floats = static_cast<size_t>(instances) * frames[k] * channels;
        // (a block of exactly the output's size, `offset` floats off an allocation 16-byte aligned: every store width's launch is taken)
        float* block = static_cast<float*>(std::malloc((floats + offset) * sizeof(float)));
        CHECK(block, "malloc");
        float* dst = block + offset;
        for (size_t i = 0; i < floats; ++i) dst[i] = -7.0F;
        CHECK(oalsfx_hip::launch_stream(records.data(), envelopes.data(), resamplers.data(), queued ? programs.data() : nullptr, rings.data(), taken.data(), tables,
                                        instances, lanes, static_cast<unsigned>(frames[k]), channels, dst, nullptr),
              "no kernel for %d channels", channels);
        CHECK(std::fwrite(dst, sizeof(float), floats, out) == floats && std::fwrite(records.data(), sizeof(oalsfx_sampler), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(envelopes.data(), sizeof(oalsfx_envelope), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(programs.data(), sizeof(oalsfx_hip::EnvProgram), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(rings.data(), sizeof(oalsfx_hip::StreamRing), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(taken.data(), sizeof(uint32_t), rows, out) == static_cast<size_t>(rows), "short write");
        std::free(block);
        int32_t appends = 0;
        CHECK(read_all(in, &appends, sizeof(appends)) && appends >= 0, "short job");
        for (int a = 0; a < appends; ++a) {
            int32_t to[2];
            CHECK(read_all(in, to, sizeof(to)) && to[0] >= 0 && to[0] < rows && to[1] >= 1, "bad append");
            oalsfx_hip::StreamRing& ring = rings[to[0]];
            CHECK(ring.queued - taken[to[0]] + static_cast<uint32_t>(to[1]) <= OALSFX_STREAM_QUEUE, "an append without room");
            for (int j = 0; j < to[1]; ++j) {
                int32_t block_number = 0;
                oalsfx_sampler& entry = ring.entry[ring.queued % OALSFX_STREAM_QUEUE];
                CHECK(read_all(in, &block_number, sizeof(block_number)) && read_all(in, &entry, sizeof(entry)) && placed(entry, block_number), "bad append");
                ++ring.queued;
            }
        }
    }
    std::fclose(in);
    std::fclose(out);
    for (void* a : blocks) std::free(a);
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) std::free(const_cast<float*>(tables.coef[t]));
    std::printf("ok\n");
    return 0;
}
