// oalsfxpp::ApiArray::set_send / ramp_send / get_send: twelve voices with an echo each go dry to a master bus and, through sends 1 and 2,
// to two more buses with levels of their own; four of the levels ramp.  The buses must equal, bit for bit, the sums this program computes
// itself in the order the C header states (members by instance and send, chunks of OALSFX_DOWNMIX_CHUNK, the ramp's gain per frame as
// from + (float)n * step, product and sum rounded separately) from the outputs of twelve separate oalsfxpp::Api objects given the same
// calls, and get_send must follow the ramps call by call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "oalsfx_hip.h"
#include "oalsfxpp_array.h"

using namespace oalsfxpp;

static void synth(uint32_t instance, uint32_t buffer_index, int count, float* out)
{
    uint32_t x = 0x9E3779B9u ^ (instance * 2654435761u) ^ buffer_index;
    if (x == 0) x = 1;
    for (int i = 0; i < count; ++i) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        out[i] = static_cast<float>(x >> 8) * (1.0F / 8388608.0F) - 1.0F;
    }
}

struct Send {
    int bus = -1;
    float gain = 1.0F, from = 0.0F, step = 0.0F, to = 0.0F;
    uint32_t frames = 0, done = 0;
    float at(uint32_t f) const
    {
        if (!frames) return gain;
        const uint32_t n = done + f;
        if (n >= frames) return to;
        volatile float product = static_cast<float>(n) * step; // (volatile: product and sum rounded to fp32 each on its own)
        volatile float sum = from + product;
        return sum;
    }
    void advance(uint32_t count)
    {
        if (!frames) return;
        done = done + count < frames ? done + count : frames;
        if (done == frames) { gain = to; frames = done = 0; }
    }
};

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 12, ch = 2, buses = 3;
    ApiArray arr;
    std::vector<Api> voice(n);
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    Send sends[n][OALSFX_BUS_SENDS];
    Effect echo;
    echo.set_type_and_defaults(EffectType::echo);
    for (int i = 0; i < n; ++i) {
        arr.set_effect(i, 0, echo);
        CHECK(voice[i].initialize(ChannelFormat::stereo, 48000, 1), "Api::initialize: %s", voice[i].get_error_message());
        voice[i].set_effect(0, echo);
        CHECK(voice[i].apply_changes(), "Api::apply_changes");
        sends[i][0].bus = 0;
        sends[i][0].gain = 0.5F + 0.03125F * static_cast<float>(i);
        CHECK(arr.set_routing(i, 0, sends[i][0].gain), "set_routing: %s", arr.get_error_message());
        sends[i][1].bus = 1;
        sends[i][1].gain = 0.25F - 0.0625F * static_cast<float>(i % 5);
        CHECK(arr.set_send(i, 1, 1, sends[i][1].gain), "set_send: %s", arr.get_error_message());
        sends[i][2].bus = i % 3 == 0 ? 0 : 2; // every third voice is in the master twice
        sends[i][2].gain = 0.125F;
        CHECK(arr.set_send(i, 2, sends[i][2].bus, sends[i][2].gain), "set_send: %s", arr.get_error_message());
    }
    CHECK(arr.apply_changes(), "apply_changes");
    CHECK(!arr.set_send(n, 1, 0, 1.0F) && !arr.set_send(0, OALSFX_BUS_SENDS, 0, 1.0F) && !arr.set_send(0, 1, -2, 1.0F) && !arr.ramp_send(0, -1, 1.0F, 16) &&
          !arr.ramp_send(0, 1, 1.0F, (1U << 24) + 1), "bad arguments were accepted");
    CHECK(std::strstr(arr.get_error_message(), "Ramp length out of range."), "message: %s", arr.get_error_message());
    const struct { int voice, send; float to; uint32_t frames; } ramps[] = {{0, 0, 0.0F, 300}, {3, 1, 1.0F, 64}, {6, 2, -0.5F, 100}, {7, 1, 0.7F, 1}};
    for (const auto& r : ramps) {
        Send& s = sends[r.voice][r.send];
        s.from = s.gain;
        s.to = r.to;
        volatile float span = r.to - s.from;
        s.step = span / static_cast<float>(r.frames);
        s.frames = r.frames;
        s.done = 0;
        CHECK(arr.ramp_send(r.voice, r.send, r.to, r.frames), "ramp_send: %s", arr.get_error_message());
    }
    const int sizes[] = {100, 256, 37};
    for (int k = 0; k < 3; ++k) {
        const int frames = sizes[k];
        const size_t per = static_cast<size_t>(frames) * ch;
        std::vector<float> src(per * n), out(per * n), got(per * buses, -1.0F), want(per * buses);
        for (int i = 0; i < n; ++i) {
            synth(900 + i, k, static_cast<int>(per), src.data() + per * i);
            CHECK(voice[i].mix(frames, src.data() + per * i, out.data() + per * i), "Api::mix");
        }
        CHECK(arr.mix_to_buses(frames, src.data(), buses, got.data()), "mix_to_buses: %s", arr.get_error_message());
        for (int b = 0; b < buses; ++b)
            for (size_t e = 0; e < per; ++e) {
                volatile float total = 0.0F, p = 0.0F;
                int in_chunk = 0;
                for (int i = 0; i < n; ++i)
                    for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
                        if (sends[i][s].bus != b) continue;
                        volatile float product = out[per * i + e] * sends[i][s].at(static_cast<uint32_t>(e / ch));
                        p = p + product;
                        if (++in_chunk == OALSFX_DOWNMIX_CHUNK) { total = total + p; p = 0.0F; in_chunk = 0; }
                    }
                if (in_chunk) total = total + p;
                want[per * b + e] = total;
            }
        CHECK(std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "call %d (%d frames): the buses differ from the stated sums", k, frames);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
                Send& mine = sends[i][s];
                mine.advance(static_cast<uint32_t>(frames));
                int bus = 7;
                float gain = -7.0F, to = -7.0F;
                uint32_t left = 7;
                CHECK(arr.get_send(i, s, bus, gain, to, left), "get_send: %s", arr.get_error_message());
                const float now = mine.at(0), end = mine.frames ? mine.to : now;
                CHECK(bus == mine.bus && left == mine.frames - mine.done && std::memcmp(&gain, &now, 4) == 0 && std::memcmp(&to, &end, 4) == 0,
                      "call %d: get_send(%d, %d) says bus %d, gain %g to %g, %u frames left", k, i, s, bus, gain, to, left);
            }
    }
    float dummy[4];
    CHECK(!arr.mix_to_buses(1, dummy, 2, dummy) && std::strstr(arr.get_error_message(), ", send 2 is routed to bus 2; the call has 2."), "bus count: %s",
          arr.get_error_message());
    std::printf("ok\n");
    return 0;
}
