// oalsfxpp::ApiArray::set_voice_filter / get_voice_filter: one round trip through a render.  Two stereo instances without effects, two
// lanes each: every voice holds one sample of a short fp32 asset (step 0), so its input is a constant per channel; lane 1 of instance 1
// (set through the signature with a lane) and lane 0 of instance 0 (through the one without) run through a biquad whose histories are
// loaded.  The bus must be the one a second array gives when fed the sum this program computes itself in the order the C header states
// ("voice filters"), and the histories read back must be the last two frames'.
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
    const int n = 2, lanes = 2, frames = 70;
    const float pcm[2] = {0.75F, -0.5F};
    const float gain[2][2] = {{0.5F, 0.25F}, {-0.75F, 0.375F}};
    ApiArray arr, plain;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(pcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, pcm, sizeof(pcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    CHECK(arr.set_polyphony(lanes), "set_polyphony: %s", arr.get_error_message());
    oalsfx_sampler s;
    std::memset(&s, 0, sizeof(s));
    s.data = reinterpret_cast<uint64_t>(dev);
    s.frames = 2;
    s.loop_end = 2;
    s.format = OALSFX_PCM_F32;
    s.channels = 1;
    s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < lanes; ++k) {
            s.position = static_cast<uint64_t>(k) << OALSFX_SAMPLER_FRAC_BITS; // lane k holds sample k
            s.gain[0] = gain[k][0];
            s.gain[1] = gain[k][1];
            CHECK(arr.set_sampler(i, k, s), "set_sampler: %s", arr.get_error_message());
        }
        CHECK(arr.set_routing(i, 0, 0.5F) && plain.set_routing(i, 0, 0.5F), "set_routing");
    }
    oalsfx_voice_filter f, got;
    std::memset(&f, 0, sizeof(f));
    CHECK(oalsfx_host_voice_filter(OALSFX_VF_LOW_PASS, 1.0F, 0.05F, 1.0F, &f) && f.b0 > 0.0F && f.a2 > 0.0F, "oalsfx_host_voice_filter");
    f.flags = OALSFX_VF_ACTIVE | OALSFX_VF_LOAD;
    for (int c = 0; c < 2; ++c) {
        f.x[c][0] = 0.25F; f.x[c][1] = -0.125F; f.y[c][0] = 0.5F; f.y[c][1] = 0.0625F;
    }
    CHECK(arr.set_voice_filter(1, 1, f) && arr.set_voice_filter(0, f), "set_voice_filter: %s", arr.get_error_message());
    CHECK(arr.get_voice_filter(1, 1, got) && got.flags == OALSFX_VF_ACTIVE && got.b0 == f.b0 && got.y[1][1] == 0.0625F, "get_voice_filter shows the row without LOAD");
    CHECK(arr.get_voice_filter(1, got) && got.flags == 0 && arr.get_voice_filter(0, 1, got) && got.flags == 0, "the other voices have no filter");
    CHECK(!arr.set_voice_filter(0, lanes, f) && std::strstr(arr.get_error_message(), "Lane out of range."), "a lane outside the array's: %s", arr.get_error_message());
    f.flags = 8;
    CHECK(!arr.set_voice_filter(0, 0, f) && std::strstr(arr.get_error_message(), "Unknown voice filter flags."), "unknown flags: %s", arr.get_error_message());
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    // the instances' inputs, computed here in the stated order
    std::vector<float> src(static_cast<size_t>(n) * frames * 2, 0.0F), bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    float last_x[2][2], last_y[2][2]; // of the voice (1, 1): [channel][0 the last, 1 the one before]
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 2; ++c) {
            volatile float x1 = 0.25F, x2 = -0.125F, y1 = 0.5F, y2 = 0.0625F; // (volatile: every operation rounded to fp32 on its own)
            const int through = i == 0 ? 0 : 1;
            for (int fr = 0; fr < frames; ++fr) {
                volatile float acc = 0.0F;
                for (int k = 0; k < lanes; ++k) {
                    volatile float o = pcm[k] * gain[k][c];
                    if (k == through) {
                        volatile float p0 = f.b0 * o, p1 = f.b1 * x1, p2 = f.b2 * x2, q1 = f.a1 * y1, q2 = f.a2 * y2;
                        volatile float u = p0 + p1;
                        u = u + p2;
                        volatile float y = u - q1;
                        y = y - q2;
                        x2 = x1; x1 = o; y2 = y1; y1 = y;
                        o = y;
                    }
                    acc = acc + o;
                }
                src[(static_cast<size_t>(i) * frames + fr) * 2 + c] = acc;
            }
            if (i == 1) { last_x[c][0] = x1; last_x[c][1] = x2; last_y[c][0] = y1; last_y[c][1] = y2; }
        }
    CHECK(plain.mix_to_buses_metered(frames, src.data(), 1, want.data(), 0.0F, false, nullptr, nullptr), "mix_to_buses_metered: %s", plain.get_error_message());
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "the bus differs from the one of the sum computed here");
    CHECK(arr.get_voice_filter(1, 1, got), "get_voice_filter: %s", arr.get_error_message());
    for (int c = 0; c < 2; ++c)
        CHECK(got.x[c][0] == last_x[c][0] && got.x[c][1] == last_x[c][1] && got.y[c][0] == last_y[c][0] && got.y[c][1] == last_y[c][1], "the histories of channel %d", c);
    CHECK(got.x[2][0] == 0.0F && got.y[7][1] == 0.0F && got.flags == OALSFX_VF_ACTIVE, "channels above the array's are untouched");
    // a lane with an ACTIVE filter is not dropped
    std::memset(&s, 0, sizeof(s));
    s.channels = 1;
    for (int i = 0; i < n; ++i) CHECK(arr.set_sampler(i, 1, s), "clearing: %s", arr.get_error_message());
    CHECK(!arr.set_polyphony(1) && std::strstr(arr.get_error_message(), "still in use"), "dropping a filtered lane: %s", arr.get_error_message());
    got.flags = 0;
    CHECK(arr.set_voice_filter(1, 1, got) && arr.set_polyphony(1) && arr.get_polyphony() == 1, "set_polyphony(1): %s", arr.get_error_message());
    arr.uninitialize();
    plain.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
