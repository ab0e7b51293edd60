// oalsfxpp::ApiArray::reset(index): Api::initialize for one voice.  Six voices play reverbs, an echo and a chorus for a while; voices 2 and
// 4 are reset and given new effects.  Each must then mix bit-identically to a fresh oalsfxpp::Api given the same calls, and every other
// voice like a twin array that was never reset.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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
    const int n = 6, slots = 2, ch = 2;
    const EffectType first[] = {EffectType::eax_reverb, EffectType::reverb, EffectType::echo, EffectType::chorus, EffectType::eax_reverb, EffectType::flanger};
    ApiArray arr, twin;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, slots) && twin.initialize(n, ChannelFormat::stereo, 48000, slots), "initialize: %s", arr.get_error_message());
    for (ApiArray* a : {&arr, &twin}) {
        for (int i = 0; i < n; ++i) {
            a->set_effect(i, 0, effect_of(first[i]));
            a->set_effect(i, 1, effect_of(EffectType::echo));
            const SendProps sp{0.8F, 0.6F, 1.0F};
            CHECK(a->set_send_props(i, -1, sp), "set_send_props");
        }
        CHECK(a->apply_changes(), "apply_changes");
    }
    CHECK(!arr.reset(n) && std::strcmp(arr.get_error_message(), "Instance index is out of range.") == 0, "reset range: %s", arr.get_error_message());
    Api fresh[2];
    const int reset_ids[2] = {2, 4};
    const int sizes[] = {256, 256, 441, 256, 100, 256, 256, 2100, 256};
    for (int k = 0; k < static_cast<int>(sizeof(sizes) / sizeof(sizes[0])); ++k) {
        const int frames = sizes[k];
        if (k == 4) {
            for (int r = 0; r < 2; ++r) {
                const int i = reset_ids[r];
                CHECK(arr.reset(i), "reset(%d): %s", i, arr.get_error_message());
                Effect e;
                CHECK(arr.get_effect(i, 0, e) && e.type_ == EffectType::null && arr.get_deferred_effect(i, 1, e) && e.type_ == EffectType::null, "reset voice %d holds effects", i);
                CHECK(fresh[r].initialize(ChannelFormat::stereo, 48000, slots), "Api::initialize: %s", fresh[r].get_error_message());
                Effect next = effect_of(r == 0 ? EffectType::chorus : EffectType::eax_reverb);
                if (r == 1) next.props_.reverb_ = ReverbPresets::Default::cave;
                arr.set_effect(i, 1, next);
                fresh[r].set_effect(1, next);
                CHECK(arr.apply_changes(i) && fresh[r].apply_changes(), "apply_changes after reset");
            }
        }
        std::vector<float> src(static_cast<size_t>(n) * frames * ch), got(src.size()), want(src.size());
        for (int i = 0; i < n; ++i) synth(300 + i, k, frames * ch, src.data() + static_cast<size_t>(i) * frames * ch);
        CHECK(arr.mix(frames, src.data(), got.data()) && twin.mix(frames, src.data(), want.data()), "mix: %s", arr.get_error_message());
        for (int i = 0; i < n; ++i) {
            const size_t at = static_cast<size_t>(i) * frames * ch;
            if (k >= 4 && (i == 2 || i == 4)) {
                std::vector<float> one(static_cast<size_t>(frames) * ch);
                CHECK(fresh[i == 2 ? 0 : 1].mix(frames, src.data() + at, one.data()), "Api::mix");
                CHECK(std::memcmp(one.data(), got.data() + at, one.size() * sizeof(float)) == 0, "call %d: reset voice %d differs from a fresh Api", k, i);
            } else {
                CHECK(std::memcmp(want.data() + at, got.data() + at, static_cast<size_t>(frames) * ch * sizeof(float)) == 0, "call %d: voice %d differs from the twin", k, i);
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
