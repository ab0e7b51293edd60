// k_fir_rows and k_voice_rows on the host: oalsfxpp_amd/csrc/hip/resample.hip and voice.hip compiled by a host compiler behind the shim
// below, the lanes of a wavefront run one after the other.  The kernels' row body has no LDS and no cross-lane operation, so a lane's
// frames are what the device's lane writes, and a host build under AddressSanitizer sees every address the kernel forms: the assets
// are heap blocks of exactly their size, so a tap read one element outside one is an error here and not a silent wrong value.
// (tests/test_resample_host.py writes the job, runs this program and compares what it leaves with the restatement.)
//
// The shim: __global__ and __device__ mean nothing, threadIdx / blockIdx / blockDim are globals the launch macro sets, readfirstlane is
// the identity (every lane of a wavefront computes the same row number), and a launch runs the blocks in ascending and a block's threads
// in DESCENDING order -- lane 0 of a wavefront writes the records back that the other lanes read, so it must come last.
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

#include "resample.hip"
#include "voice.hip"

namespace {

bool read_all(std::FILE* f, void* to, size_t bytes) { return bytes == 0 || std::fread(to, 1, bytes, f) == bytes; }

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

} // namespace

// fir_rows_host <job> <result> [voice].  With `voice` the job names no table and is rendered through launch_voice (k_voice_rows), else
// through launch_fir (k_fir_rows).  The job, little-endian: int32 rows, channels, calls, assets, dst offset in floats; int32 frames[calls];
// for each of the 8 tables int32 taps, phase_bits and the coefficients; for each asset int64 bytes and the bytes; int32 asset of every row
// (-1: none); the records, the envelopes, the resamplers.  The result: for every call the output [rows][frames][channels], the records
// and the envelopes behind it (a record's data is this process's address of its asset).
int main(int argc, char** argv)
{
    CHECK(argc == 3 || (argc == 4 && std::string(argv[3]) == "voice"), "usage: fir_rows_host <job> <result> [voice]");
    const bool voice = argc == 4;
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in, "cannot open %s", argv[1]);
    int32_t head[5];
    CHECK(read_all(in, head, sizeof(head)), "short job");
    const int rows = head[0], channels = head[1], calls = head[2], n_assets = head[3], offset = head[4];
    CHECK(rows >= 1 && calls >= 1 && n_assets >= 0 && offset >= 0, "bad job");
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
    CHECK(read_all(in, asset_of.data(), rows * sizeof(int32_t)) && read_all(in, records.data(), rows * sizeof(oalsfx_sampler)) &&
          read_all(in, envelopes.data(), rows * sizeof(oalsfx_envelope)) && read_all(in, resamplers.data(), rows * sizeof(int32_t)), "short job");
    std::fclose(in);
    for (int r = 0; r < rows; ++r) {
        CHECK(asset_of[r] >= -1 && asset_of[r] < n_assets, "bad asset number");
        records[r].data = asset_of[r] < 0 ? 0 : reinterpret_cast<uint64_t>(assets[asset_of[r]]);
        CHECK(resamplers[r] >= -1 && resamplers[r] < OALSFX_FIR_TABLES && (resamplers[r] < 0 || tables.taps[resamplers[r]]), "bad resampler");
        CHECK(!voice || resamplers[r] < 0, "k_voice_rows has no tables");
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    CHECK(out, "cannot open %s", argv[2]);
    for (int k = 0; k < calls; ++k) {
        const size_t floats = static_cast<size_t>(rows) * frames[k] * channels;
        // (a block of exactly the output's size, `offset` floats off an allocation 16-byte aligned: every store width's launch is taken)
        float* block = static_cast<float*>(std::malloc((floats + offset) * sizeof(float)));
        CHECK(block, "malloc");
        float* dst = block + offset;
        for (size_t i = 0; i < floats; ++i) dst[i] = -7.0F;
        const bool launched = voice ? oalsfx_hip::launch_voice(records.data(), envelopes.data(), rows, static_cast<unsigned>(frames[k]), channels, dst, nullptr)
                                    : oalsfx_hip::launch_fir(records.data(), envelopes.data(), resamplers.data(), tables, rows, static_cast<unsigned>(frames[k]), channels, dst, nullptr);
        CHECK(launched, "no kernel for %d channels", channels);
        CHECK(std::fwrite(dst, sizeof(float), floats, out) == floats && std::fwrite(records.data(), sizeof(oalsfx_sampler), rows, out) == static_cast<size_t>(rows) &&
              std::fwrite(envelopes.data(), sizeof(oalsfx_envelope), rows, out) == static_cast<size_t>(rows), "short write");
        std::free(block);
    }
    std::fclose(out);
    for (void* a : assets) std::free(a);
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) std::free(const_cast<float*>(tables.coef[t]));
    std::printf("ok\n");
    return 0;
}
