// oalsfxpp::ApiArray::set_envelope / get_envelope: one round trip.  Four stereo voices without effects loop a short fp32 asset resident in
// device memory; voice 1 fades out over six frames and stops, voice 2 starts after a delay of three frames.  The envelopes and the
// samplers' records read back after a call of eight frames must be the ones the C header's arithmetic ("voice envelopes") leaves, and
// the bus must be the one a second array gives when fed the render this program computes itself in the stated order.
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
    const int n = 4, frames = 8;
    ApiArray arr, plain;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    const float pcm[4] = {0.5F, -0.25F, 0.75F, 1.0F};
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(pcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, pcm, sizeof(pcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    for (int i = 0; i < n; ++i) {
        oalsfx_sampler s;
        std::memset(&s, 0, sizeof(s));
        s.data = reinterpret_cast<uint64_t>(dev);
        s.frames = 4;
        s.loop_end = 4;
        s.step = 4096;
        s.format = OALSFX_PCM_F32;
        s.channels = 1;
        s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP;
        s.gain[0] = 0.5F;
        s.gain[1] = 0.25F;
        CHECK(arr.set_sampler(i, s), "set_sampler: %s", arr.get_error_message());
        CHECK(arr.set_routing(i, i == 3 ? -1 : 0, 0.5F) && plain.set_routing(i, i == 3 ? -1 : 0, 0.5F), "set_routing");
    }
    oalsfx_envelope fade, late, got;
    std::memset(&fade, 0, sizeof(fade));
    const float one[2] = {1.0F, 1.0F}, none[2] = {0.0F, 0.0F};
    oalsfx_host_envelope_ramp(one, none, 2, 6, &fade);
    fade.flags = OALSFX_ENV_ACTIVE | OALSFX_ENV_STOP;
    std::memset(&late, 0, sizeof(late));
    oalsfx_host_envelope_ramp(one, one, 2, 0, &late);
    late.flags = OALSFX_ENV_ACTIVE;
    late.delay = 3;
    CHECK(arr.set_envelope(1, fade) && arr.set_envelope(2, late), "set_envelope: %s", arr.get_error_message());
    CHECK(arr.get_envelope(1, got) && std::memcmp(&got, &fade, sizeof(got)) == 0, "get_envelope before a render");
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    // what the four voices render, computed here in the stated order: voice 1's fade over six frames, then silence; voice 2 from frame 3
    // on; a second array without samplers is fed it and must give the same bus
    std::vector<float> src(static_cast<size_t>(n) * frames * 2, 0.0F), bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    for (int i = 0; i < n; ++i)
        for (int f = 0; f < frames; ++f)
            for (int c = 0; c < 2; ++c) {
                const float gain = c ? 0.25F : 0.5F;
                volatile float o = 0.0F; // (volatile: every operation rounded to fp32 on its own)
                if (i == 1) {
                    if (f < 6) {
                        volatile float product = static_cast<float>(f) * fade.gain_step[c];
                        volatile float e = fade.gain_from[c] + product;
                        volatile float v = pcm[f % 4] * gain;
                        o = v * e;
                    }
                } else if (i == 2) {
                    if (f >= 3) {
                        volatile float v = pcm[(f - 3) % 4] * gain;
                        o = v * late.gain_to[c];
                    }
                } else {
                    o = pcm[f % 4] * gain;
                }
                src[(static_cast<size_t>(i) * frames + f) * 2 + c] = o;
            }
    CHECK(plain.mix_to_buses_metered(frames, src.data(), 1, want.data(), 0.0F, false, nullptr, nullptr), "mix_to_buses_metered: %s", plain.get_error_message());
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "the bus differs from the one of the render computed here");
    float loudest = 0.0F;
    for (float v : bus) loudest = v > loudest ? v : (-v > loudest ? -v : loudest);
    CHECK(loudest > 0.1F, "the bus is silent");
    oalsfx_sampler s;
    CHECK(arr.get_envelope(1, got) && got.ramp_done == 6 && got.delay == 0 && got.flags == fade.flags, "the fade read back: ramp_done %u", got.ramp_done);
    CHECK(arr.get_sampler(1, s) && !(s.flags & OALSFX_SAMPLER_PLAYING) && s.position == (2u << 12), "the faded voice: flags %u, position %llu", s.flags,
          static_cast<unsigned long long>(s.position));
    CHECK(arr.get_envelope(2, got) && got.delay == 0 && got.ramp_done == 0 && got.sub == 0, "the delayed envelope read back");
    CHECK(arr.get_sampler(2, s) && (s.flags & OALSFX_SAMPLER_PLAYING) && s.position == (1u << 12), "the delayed voice: position %llu",
          static_cast<unsigned long long>(s.position));
    CHECK(arr.get_envelope(0, got) && got.flags == 0, "a voice without an envelope");
    // refusals come back as false with the library's message
    fade.reserved[1] = 1;
    CHECK(!arr.set_envelope(1, fade) && std::strstr(arr.get_error_message(), "reserved"), "a reserved field: %s", arr.get_error_message());
    CHECK(!arr.set_envelope(n, late) && !arr.get_envelope(-1, got), "an index outside the array");
    arr.uninitialize();
    plain.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
