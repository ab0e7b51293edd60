// oalsfxpp::ApiArray::set_fir_table / set_resampler / get_resampler: one round trip.  Three stereo voices without effects loop a short
// fp32 asset resident in device memory at two thirds of its rate; voice 0 interpolates it through a 4-tap Catmull-Rom table of four
// phases, voice 1 through an 8-tap table of one phase, voice 2 names no table.  The bus must be the one a second array gives when fed
// the render this program computes itself in the order the C header states ("resamplers").
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "oalsfx_hip.h"
#include "oalsfxpp_array.h"

using namespace oalsfxpp;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 3, frames = 40, asset_frames = 6;
    const uint32_t step = 2731;
    ApiArray arr, plain;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    const float pcm[asset_frames] = {0.5F, -0.25F, 0.75F, 1.0F, -0.625F, 0.125F};
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(pcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, pcm, sizeof(pcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    for (int i = 0; i < n; ++i) {
        oalsfx_sampler s;
        std::memset(&s, 0, sizeof(s));
        s.data = reinterpret_cast<uint64_t>(dev);
        s.frames = asset_frames;
        s.loop_start = 1;
        s.loop_end = 5;
        s.step = step;
        s.format = OALSFX_PCM_F32;
        s.channels = 1;
        s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP;
        s.gain[0] = 0.5F;
        s.gain[1] = 0.25F;
        CHECK(arr.set_sampler(i, s), "set_sampler: %s", arr.get_error_message());
        CHECK(arr.set_routing(i, 0, 0.5F) && plain.set_routing(i, 0, 0.5F), "set_routing");
    }
    float cubic[4 * 4];
    oalsfx_host_fir_cubic(2, cubic);
    const float wide[8] = {-0.03125F, 0.125F, -0.25F, 0.625F, 0.5F, -0.125F, 0.09375F, -0.015625F};
    int table = 7;
    CHECK(arr.get_resampler(0, table) && table == OALSFX_RESAMPLER_NONE, "a fresh array's resampler: %d", table);
    CHECK(!arr.set_resampler(0, 2) && std::strstr(arr.get_error_message(), "has not been set"), "a table that was not set: %s", arr.get_error_message());
    CHECK(arr.set_fir_table(2, 4, 2, cubic) && arr.set_fir_table(5, 8, 0, wide), "set_fir_table: %s", arr.get_error_message());
    CHECK(arr.set_resampler(0, 2) && arr.set_resampler(1, 5), "set_resampler: %s", arr.get_error_message());
    CHECK(arr.get_resampler(1, table) && table == 5 && arr.get_resampler(2, table) && table == OALSFX_RESAMPLER_NONE, "get_resampler");
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    // what the three voices render, computed here in the stated order; a second array without samplers is fed it
    std::vector<float> src(static_cast<size_t>(n) * frames * 2, 0.0F), bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    for (int i = 0; i < n; ++i)
        for (int f = 0; f < frames; ++f) {
            uint64_t q = static_cast<uint64_t>(f) * step;
            const uint64_t l0 = uint64_t{1} << 12, l1 = uint64_t{5} << 12;
            if (q >= l1) q = l0 + (q - l0) % (l1 - l0);
            const int at = static_cast<int>(q >> 12);
            volatile float v = 0.0F; // (volatile: every operation rounded to fp32 on its own)
            if (i == 2) {
                v = pcm[at];
            } else {
                const int taps = i == 0 ? 4 : 8, half = taps / 2;
                const float* c = i == 0 ? cubic + 4 * ((q & 4095) >> 10) : wide;
                for (int k = 0; k < taps; ++k) {
                    const int j = at - (half - 1) + k;
                    if (j < 0) continue; // (+0.0f: an out-of-range tap may be left out)
                    const float x = pcm[j >= 5 ? 1 + (j - 5) % 4 : j];
                    volatile float product = c[k] * x;
                    v = v + product;
                }
            }
            for (int c = 0; c < 2; ++c) {
                volatile float o = v * (c ? 0.25F : 0.5F);
                src[(static_cast<size_t>(i) * frames + f) * 2 + c] = o;
            }
        }
    CHECK(plain.mix_to_buses_metered(frames, src.data(), 1, want.data(), 0.0F, false, nullptr, nullptr), "mix_to_buses_metered: %s", plain.get_error_message());
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "the bus differs from the one of the render computed here");
    float loudest = 0.0F;
    for (float v : bus) loudest = v > loudest ? v : (-v > loudest ? -v : loudest);
    CHECK(loudest > 0.1F, "the bus is silent");
    // refusals come back as false with the library's message
    CHECK(!arr.set_fir_table(2, 0, 0, nullptr) && std::strstr(arr.get_error_message(), "still named"), "clearing a named table: %s", arr.get_error_message());
    CHECK(!arr.set_fir_table(8, 4, 2, cubic) && !arr.set_fir_table(3, 5, 2, cubic) && !arr.set_resampler(0, 8), "a table, a tap count and a resampler out of range");
    CHECK(!arr.set_resampler(n, 2) && !arr.get_resampler(-1, table), "an index outside the array");
    CHECK(arr.set_resampler(0, OALSFX_RESAMPLER_NONE) && arr.set_fir_table(2, 0, 0, nullptr), "clearing: %s", arr.get_error_message());
    arr.uninitialize();
    plain.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
