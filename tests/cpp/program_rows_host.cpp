// k_program_rows and k_program_biquad_rows on the host: oalsfxpp_amd/csrc/hip/program.hip and biquad.hip compiled by a host compiler
// behind the shim below (the one of biquad_rows_host.cpp).  k_program_rows runs its lanes one after the other, each through all of its
// instance's voices and all of their spans; k_program_biquad_rows runs once per wavefront and walks the lanes itself, a whole stretch of
// zero fill and sequenced renders per lane between two filter stages (OALSFX_EACH_LANE in biquad.hip).  Either way a lane's turn ends
// before the next lane's begins, lane 0 last.  That stands in for the device because of how the sequenced row body keeps the records
// between spans (program_rows_body.hpp): every lane carries what the spans change in registers of its own, reads from memory only what no
// lane writes before the voice's last span is done -- the records as the kernel found them, the queue's entries -- and lane 0 alone
// writes, once, behind its own last span.  A body in which a lane read back what lane 0 had stored after a span would see here, in the
// lanes 63 .. 1, records no span has advanced yet, and render every span from the first segment: wrong bits, which the comparison with
// the restatement shows.  And as in mix_rows_host.cpp, a lane that read a frame another lane owns would sum over zeros not yet filled in
// or over voices already added.  A host build under AddressSanitizer sees every address the kernels form: the assets, the output, the
// scratch rows and the queues are heap blocks of exactly their size.  (tests/test_program_host.py writes the job, runs this program
// and compares what it leaves with the restatement.)
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

#include "program.hip"
#include "biquad.hip"

namespace {

bool read_all(std::FILE* f, void* to, size_t bytes) { return bytes == 0 || std::fread(to, 1, bytes, f) == bytes; }

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

} // namespace

// program_rows_host <job> <result>.  The job, little-endian: int32 instances, lanes, channels, calls, assets, dst offset in floats, and
// whether the filters take part (k_program_biquad_rows) or not (k_program_rows); int32 frames[calls]; for each of the 8 tables int32 taps,
// phase_bits and the coefficients; for each asset int64 bytes and the bytes; then for the instances * lanes voices, lane-major: int32
// asset of every voice (-1: none), the records, the envelopes, the resamplers, the filters, the queues.  The result: for every call the
// output [instances][frames][channels], the records, the envelopes, the filters and the queues behind it (a record's data is this
// process's address of its asset).
int main(int argc, char** argv)
{
    CHECK(argc == 3, "usage: program_rows_host <job> <result>");
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in, "cannot open %s", argv[1]);
    int32_t head[7];
    CHECK(read_all(in, head, sizeof(head)), "short job");
    const int instances = head[0], lanes = head[1], channels = head[2], calls = head[3], n_assets = head[4], offset = head[5];
    const bool filtered = head[6] != 0;
    CHECK(instances >= 1 && lanes >= 1 && lanes <= OALSFX_MAX_POLYPHONY && calls >= 1 && n_assets >= 0 && offset >= 0, "bad job");
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
    std::vector<void*> assets(n_assets, nullptr);
    for (int a = 0; a < n_assets; ++a) {
        int64_t bytes = 0;
        CHECK(read_all(in, &bytes, sizeof(bytes)) && bytes > 0, "short job");
        assets[a] = std::malloc(static_cast<size_t>(bytes));
        CHECK(assets[a] && read_all(in, assets[a], static_cast<size_t>(bytes)), "short job");
    }
    std::vector<int32_t> asset_of(rows), resamplers(rows);
    std::vector<oalsfx_sampler> records(rows);
    std::vector<oalsfx_envelope> envelopes(rows);
    std::vector<oalsfx_voice_filter> filters(rows);
    std::vector<oalsfx_hip::EnvProgram> programs(rows);
    CHECK(read_all(in, asset_of.data(), rows * sizeof(int32_t)) && read_all(in, records.data(), rows * sizeof(oalsfx_sampler)) &&
          read_all(in, envelopes.data(), rows * sizeof(oalsfx_envelope)) && read_all(in, resamplers.data(), rows * sizeof(int32_t)) &&
          read_all(in, filters.data(), rows * sizeof(oalsfx_voice_filter)) && read_all(in, programs.data(), rows * sizeof(oalsfx_hip::EnvProgram)), "short job");
    std::fclose(in);
    for (int r = 0; r < rows; ++r) {
        CHECK(asset_of[r] >= -1 && asset_of[r] < n_assets, "bad asset number");
        records[r].data = asset_of[r] < 0 ? 0 : reinterpret_cast<uint64_t>(assets[asset_of[r]]);
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
        // (the scratch rows: exactly [instances][frames][channels], 16-byte aligned as the batch's buffer is)
        float* scratch = static_cast<float*>(std::aligned_alloc(16, (floats * sizeof(float) + 15) / 16 * 16));
        CHECK(scratch, "aligned_alloc");
        for (size_t i = 0; i < floats; ++i) scratch[i] = -9.0F;
        if (filtered)
            CHECK(oalsfx_hip::launch_program_biquad(records.data(), envelopes.data(), resamplers.data(), filters.data(), programs.data(), tables, instances, lanes,
                                                    static_cast<unsigned>(frames[k]), channels, dst, scratch, nullptr),
                  "no kernel for %d channels", channels);
        else
            CHECK(oalsfx_hip::launch_program(records.data(), envelopes.data(), resamplers.data(), programs.data(), tables, instances, lanes,
                                             static_cast<unsigned>(frames[k]), channels, dst, nullptr),
                  "no kernel for %d channels", channels);
        std::free(scratch);
        CHECK(std::fwrite(dst, sizeof(float), floats, out) == floats && std::fwrite(records.data(), sizeof(oalsfx_sampler), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(envelopes.data(), sizeof(oalsfx_envelope), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(filters.data(), sizeof(oalsfx_voice_filter), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(programs.data(), sizeof(oalsfx_hip::EnvProgram), rows, out) == static_cast<size_t>(rows), "short write");
        std::free(block);
    }
    std::fclose(out);
    for (void* a : assets) std::free(a);
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) std::free(const_cast<float*>(tables.coef[t]));
    std::printf("ok\n");
    return 0;
}
