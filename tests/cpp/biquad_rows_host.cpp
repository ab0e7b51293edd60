// k_biquad_rows on the host: oalsfxpp_amd/csrc/hip/biquad.hip compiled by a host compiler behind the shim below (the one of
// fir_rows_host.cpp and mix_rows_host.cpp, with a float4 for the recurrence).  The filter stage exchanges values between lanes, so the
// lanes cannot simply run one after the other: the kernel is written as per-lane phase functions between its wavefront syncs, and
// compiled for the host it runs once per wavefront and runs each phase over all 64 lanes before the next (OALSFX_EACH_LANE in
// biquad.hip).  The zero fill and the renders and sums of the voices between two filter stages still run lane by lane, each lane
// through the whole stretch, so k_mix_rows' ownership rule is still proven: a kernel in which one lane read what another wrote
// outside the filter stage would sum over zeros not yet filled in, or over voices already added.  A host build under AddressSanitizer
// sees every address the kernel forms: the assets, the output and the scratch rows are heap blocks of exactly their size.
// (tests/test_biquad_host.py writes the job, runs this program and compares what it leaves with the restatement.)
//
// The shim: __global__ and __device__ mean nothing, threadIdx / blockIdx / blockDim are globals the launch macro sets, readfirstlane is
// the identity, and a launch calls the kernel for every thread, blocks ascending; the kernel itself leaves at once in all threads but a
// wavefront's first and walks the lanes in DESCENDING order -- lane 0 writes the records back that the other lanes read, so it comes last.
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

#include "biquad.hip"

namespace {

bool read_all(std::FILE* f, void* to, size_t bytes) { return bytes == 0 || std::fread(to, 1, bytes, f) == bytes; }

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

} // namespace

// biquad_rows_host <job> <result>.  The job, little-endian: int32 instances, lanes, channels, calls, assets, dst offset in floats; int32
// frames[calls]; for each of the 8 tables int32 taps, phase_bits and the coefficients; for each asset int64 bytes and the bytes; then for
// the instances * lanes voices, lane-major: int32 asset of every voice (-1: none), the records, the envelopes, the resamplers, the filters.
// The result: for every call the output [instances][frames][channels], the records, the envelopes and the filters behind it (a
// record's data is this process's address of its asset).
int main(int argc, char** argv)
{
    CHECK(argc == 3, "usage: biquad_rows_host <job> <result>");
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in, "cannot open %s", argv[1]);
    int32_t head[6];
    CHECK(read_all(in, head, sizeof(head)), "short job");
    const int instances = head[0], lanes = head[1], channels = head[2], calls = head[3], n_assets = head[4], offset = head[5];
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
    CHECK(read_all(in, asset_of.data(), rows * sizeof(int32_t)) && read_all(in, records.data(), rows * sizeof(oalsfx_sampler)) &&
          read_all(in, envelopes.data(), rows * sizeof(oalsfx_envelope)) && read_all(in, resamplers.data(), rows * sizeof(int32_t)) &&
          read_all(in, filters.data(), rows * sizeof(oalsfx_voice_filter)), "short job");
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
        CHECK(oalsfx_hip::launch_biquad(records.data(), envelopes.data(), resamplers.data(), filters.data(), tables, instances, lanes,
                                        static_cast<unsigned>(frames[k]), channels, dst, scratch, nullptr),
              "no kernel for %d channels", channels);
        std::free(scratch);
        CHECK(std::fwrite(dst, sizeof(float), floats, out) == floats && std::fwrite(records.data(), sizeof(oalsfx_sampler), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(envelopes.data(), sizeof(oalsfx_envelope), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(filters.data(), sizeof(oalsfx_voice_filter), rows, out) == static_cast<size_t>(rows), "short write");
        std::free(block);
    }
    std::fclose(out);
    for (void* a : assets) std::free(a);
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) std::free(const_cast<float*>(tables.coef[t]));
    std::printf("ok\n");
    return 0;
}
