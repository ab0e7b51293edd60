// oalsfxpp::ApiArray::set_polyphony and the (index, lane) overloads of set_/get_sampler, _envelope and _resampler: one round trip.  Two
// stereo instances without effects, three lanes each: lane 0 (set through the signatures without a lane) and lane 1 loop a short fp32
// asset resident in device memory at different rates and gains, lane 2 of instance 1 plays it through a one-phase 4-tap table behind an
// envelope with a delay of 5 frames; lane 2 of instance 0 stays idle.  The bus must be the one a second array gives when fed the sum this
// program computes itself in the order the C header states ("polyphony"): lanes ascending from +0.0f, every addition rounded by itself.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "oalsfx_hip.h"
#include "oalsfxpp_array.h"

using namespace oalsfxpp;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

namespace {

const int kAssetFrames = 6;
const float kPcm[kAssetFrames] = {0.5F, -0.25F, 0.75F, 1.0F, -0.625F, 0.125F};
const float kTaps[4] = {-0.125F, 0.625F, 0.5F, 0.0625F};
const uint32_t kStep[3] = {2731, 4096, 1500};
const float kGain[3][2] = {{0.5F, 0.25F}, {-0.75F, 0.375F}, {0.3F, -0.9F}};
const float kEnvTo[2] = {0.5F, 2.0F};
const int kDelay = 5;

// the wrapped 12-bit position of the voice's frame f: a loop over frames 1 .. 4, started at 0
uint64_t position(uint32_t step, int f)
{
    uint64_t q = static_cast<uint64_t>(f) * step;
    const uint64_t l0 = uint64_t{1} << 12, l1 = uint64_t{5} << 12;
    if (q >= l1) q = l0 + (q - l0) % (l1 - l0);
    return q;
}

} // namespace

int main()
{
    const int n = 2, lanes = 3, frames = 40;
    ApiArray arr, plain;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(kPcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, kPcm, sizeof(kPcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    oalsfx_sampler s, got;
    std::memset(&s, 0, sizeof(s));
    s.data = reinterpret_cast<uint64_t>(dev);
    s.frames = kAssetFrames;
    s.loop_start = 1;
    s.loop_end = 5;
    s.format = OALSFX_PCM_F32;
    s.channels = 1;
    s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP;
    CHECK(arr.get_polyphony() == 1, "a fresh array's polyphony: %d", arr.get_polyphony());
    CHECK(!arr.set_sampler(0, 1, s) && std::strstr(arr.get_error_message(), "Lane out of range."), "lane 1 of one: %s", arr.get_error_message());
    CHECK(!arr.set_polyphony(0) && !arr.set_polyphony(OALSFX_MAX_POLYPHONY + 1) && std::strstr(arr.get_error_message(), "Polyphony out of range."), "set_polyphony(17): %s",
          arr.get_error_message());
    CHECK(arr.set_polyphony(lanes) && arr.get_polyphony() == lanes, "set_polyphony: %s", arr.get_error_message());
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < lanes; ++k) {
            if (k == 2 && i == 0) continue;
            s.step = kStep[k];
            s.gain[0] = kGain[k][0];
            s.gain[1] = kGain[k][1];
            // (lane 0 through the signature that means it)
            CHECK(k == 0 ? arr.set_sampler(i, s) : arr.set_sampler(i, k, s), "set_sampler: %s", arr.get_error_message());
            CHECK(arr.get_sampler(i, k, got) && std::memcmp(&got, &s, sizeof(s)) == 0, "get_sampler(%d, %d)", i, k);
        }
        CHECK(arr.get_sampler(i, got) && got.step == kStep[0], "get_sampler without a lane is lane 0");
        CHECK(arr.set_routing(i, 0, 0.5F) && plain.set_routing(i, 0, 0.5F), "set_routing");
    }
    oalsfx_envelope e, e_got;
    std::memset(&e, 0, sizeof(e));
    e.flags = OALSFX_ENV_ACTIVE;
    e.delay = kDelay;
    e.gain_from[0] = e.gain_to[0] = kEnvTo[0];
    e.gain_from[1] = e.gain_to[1] = kEnvTo[1];
    CHECK(arr.set_envelope(1, 2, e) && arr.get_envelope(1, 2, e_got) && std::memcmp(&e_got, &e, sizeof(e)) == 0, "set_envelope: %s", arr.get_error_message());
    CHECK(arr.get_envelope(1, e_got) && e_got.flags == 0 && arr.get_envelope(0, 2, e_got) && e_got.flags == 0, "the other voices have no envelope");
    int table = 7;
    CHECK(arr.set_fir_table(3, 4, 0, kTaps), "set_fir_table: %s", arr.get_error_message());
    CHECK(arr.set_resampler(1, 2, 3) && arr.get_resampler(1, 2, table) && table == 3, "set_resampler: %s", arr.get_error_message());
    CHECK(arr.get_resampler(1, table) && table == OALSFX_RESAMPLER_NONE && arr.get_resampler(0, 2, table) && table == OALSFX_RESAMPLER_NONE, "the other voices name no table");
    CHECK(!arr.set_resampler(1, lanes, 3) && !arr.get_envelope(0, -1, e_got) && std::strstr(arr.get_error_message(), "Lane out of range."), "a lane outside the array's: %s",
          arr.get_error_message());
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    // what the instances' voices sum to, computed here in the stated order; a second array without samplers is fed it
    std::vector<float> src(static_cast<size_t>(n) * frames * 2, 0.0F), bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    for (int i = 0; i < n; ++i)
        for (int f = 0; f < frames; ++f)
            for (int c = 0; c < 2; ++c) {
                volatile float acc = 0.0F; // (volatile: every operation rounded to fp32 on its own)
                for (int k = 0; k < lanes; ++k) {
                    if (k == 2 && (i == 0 || f < kDelay)) continue; // (+0.0f: a silent frame may be left out)
                    volatile float o;
                    if (k < 2) {
                        o = kPcm[position(kStep[k], f) >> 12] * kGain[k][c];
                    } else {
                        const int at = static_cast<int>(position(kStep[k], f - kDelay) >> 12);
                        volatile float v = 0.0F;
                        for (int t = 0; t < 4; ++t) {
                            const int j = at - 1 + t;
                            if (j < 0) continue;
                            volatile float product = kTaps[t] * kPcm[j >= 5 ? 1 + (j - 5) % 4 : j];
                            v = v + product;
                        }
                        o = v * kGain[k][c];
                        o = o * kEnvTo[c];
                    }
                    acc = acc + o;
                }
                src[(static_cast<size_t>(i) * frames + f) * 2 + c] = acc;
            }
    CHECK(plain.mix_to_buses_metered(frames, src.data(), 1, want.data(), 0.0F, false, nullptr, nullptr), "mix_to_buses_metered: %s", plain.get_error_message());
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "the bus differs from the one of the sum computed here");
    float loudest = 0.0F;
    for (float v : bus) loudest = v > loudest ? v : (-v > loudest ? -v : loudest);
    CHECK(loudest > 0.1F, "the bus is silent");
    // every voice has advanced by its own contract
    CHECK(arr.get_sampler(1, 1, got) && got.position == position(kStep[1], frames), "lane 1's position: %llu", static_cast<unsigned long long>(got.position));
    CHECK(arr.get_sampler(1, 2, got) && got.position == position(kStep[2], frames - kDelay), "lane 2's position: %llu", static_cast<unsigned long long>(got.position));
    CHECK(arr.get_envelope(1, 2, e_got) && e_got.delay == 0, "lane 2's delay: %u", e_got.delay);
    // a lane in use is not dropped
    CHECK(!arr.set_polyphony(1) && std::strstr(arr.get_error_message(), "still in use") && arr.get_polyphony() == lanes, "dropping playing lanes: %s", arr.get_error_message());
    std::memset(&s, 0, sizeof(s));
    s.channels = 1;
    std::memset(&e, 0, sizeof(e));
    for (int i = 0; i < n; ++i)
        for (int k = 1; k < lanes; ++k)
            CHECK(arr.set_sampler(i, k, s) && arr.set_envelope(i, k, e) && arr.set_resampler(i, k, OALSFX_RESAMPLER_NONE), "clearing (%d, %d): %s", i, k, arr.get_error_message());
    CHECK(arr.set_polyphony(1) && arr.get_polyphony() == 1, "set_polyphony(1): %s", arr.get_error_message());
    CHECK(arr.get_sampler(1, got) && got.position == position(kStep[0], frames), "lane 0 keeps its record");
    arr.uninitialize();
    plain.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
