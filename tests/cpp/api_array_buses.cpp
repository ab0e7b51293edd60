// oalsfxpp::ApiArray::set_routing / mix_to_buses: forty voices with effects of several kinds go to three buses (and two voices nowhere)
// with gains of their own.  The buses must equal, bit for bit, the sums this program computes itself in the order the C header states
// (members ascending, chunks of OALSFX_DOWNMIX_CHUNK, product and sum rounded separately) from the outputs of forty separate
// oalsfxpp::Api objects given the same calls -- once from one interleaved source, once from one source buffer per voice.
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

static Effect effect_of(EffectType t)
{
    Effect e;
    e.set_type_and_defaults(t);
    return e;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 40, ch = 2, buses = 3;
    const EffectType kinds[] = {EffectType::eax_reverb, EffectType::chorus, EffectType::echo, EffectType::reverb, EffectType::null};
    ApiArray arr;
    std::vector<Api> voice(n);
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    int bus[n];
    float gain[n];
    for (int i = 0; i < n; ++i) {
        const Effect e = effect_of(kinds[i % 5]);
        arr.set_effect(i, 0, e);
        CHECK(voice[i].initialize(ChannelFormat::stereo, 48000, 1), "Api::initialize: %s", voice[i].get_error_message());
        voice[i].set_effect(0, e);
        CHECK(voice[i].apply_changes(), "Api::apply_changes");
        // bus 0 gets 35 voices (a second chunk), bus 1 two, bus 2 one, voices 7 and 23 go nowhere
        bus[i] = (i == 7 || i == 23) ? -1 : i == 11 || i == 30 ? 1 : i == 39 ? 2 : 0;
        gain[i] = 0.25F + 0.03125F * static_cast<float>(i % 9) - (i % 4 == 3 ? 1.0F : 0.0F);
        CHECK(arr.set_routing(i, bus[i], gain[i]), "set_routing: %s", arr.get_error_message());
    }
    CHECK(arr.apply_changes(), "apply_changes");
    CHECK(!arr.set_routing(n, 0, 1.0F) && !arr.set_routing(0, -2, 1.0F), "set_routing accepted bad arguments");
    int b0 = 0;
    float g0 = 0.0F;
    CHECK(oalsfx_batch_get_routing(arr.batch(), 11, &b0, &g0) && b0 == 1 && g0 == gain[11], "get_routing");
    const int sizes[] = {256, 100, 2100, 256};
    for (int k = 0; k < 4; ++k) {
        const int frames = sizes[k];
        const size_t per = static_cast<size_t>(frames) * ch;
        std::vector<float> src(per * n), out(per * n), got(per * buses, -1.0F), want(per * buses);
        std::vector<const float*> rows(n);
        for (int i = 0; i < n; ++i) {
            synth(500 + i, k, static_cast<int>(per), src.data() + per * i);
            rows[i] = src.data() + per * i;
            CHECK(voice[i].mix(frames, src.data() + per * i, out.data() + per * i), "Api::mix");
        }
        const bool ok = (k & 1) ? arr.mix_to_buses(frames, rows.data(), buses, got.data()) : arr.mix_to_buses(frames, src.data(), buses, got.data());
        CHECK(ok, "mix_to_buses: %s", arr.get_error_message());
        for (int b = 0; b < buses; ++b)
            for (size_t e = 0; e < per; ++e) {
                volatile float total = 0.0F, p = 0.0F; // (volatile: every product and sum rounded to fp32 on its own)
                int in_chunk = 0;
                for (int i = 0; i < n; ++i) {
                    if (bus[i] != b) continue;
                    volatile float t = out[per * i + e] * gain[i];
                    p = p + t;
                    if (++in_chunk == OALSFX_DOWNMIX_CHUNK) { total = total + p; p = 0.0F; in_chunk = 0; }
                }
                if (in_chunk) total = total + p;
                want[per * b + e] = total;
            }
        CHECK(std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "call %d (%d frames): the buses differ from the stated sums", k, frames);
    }
    float dummy[4];
    CHECK(!arr.mix_to_buses(1, dummy, 2, dummy) && std::strstr(arr.get_error_message(), "is routed to bus 2; the call has 2."), "bus count: %s", arr.get_error_message());
    std::printf("ok\n");
    return 0;
}
