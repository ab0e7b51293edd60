// An auxiliary send set back to exactly (1, 1, 1) while its slot's properties change, through the two public C++ surfaces:
// oalsfxpp::Api (include/oalsfxpp.h) and oalsfxpp::ApiArray (include/oalsfxpp_array.h).  The reference re-derives the sends
// from the active aux props whenever a slot changed (update_context_sources, src/oalsfxpp.cpp:3397-3412) and mixes at send
// gain 1 from then on.  Writes the outputs of the Api and of the three ApiArray instances as raw floats, one stream after the
// other; the pytest wrapper compares them with the CPU model.
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

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const int frames = 256, ch = 2, n = 3;
    const SendProps half{0.5F, 0.5F, 0.5F}, unity{1.0F, 1.0F, 1.0F};
    Effect preset;
    preset.set_type_and_defaults(EffectType::eax_reverb);
    preset.props_.reverb_ = ReverbPresets::Misc::small_water_room;

    // [stream][buffer][frames * ch]: stream 0 the Api, streams 1..3 the ApiArray instances
    std::vector<std::vector<float>> out(1 + n);

    Api api;
    CHECK(api.initialize(ChannelFormat::stereo, 48000, 1), "Api::initialize: %s", api.get_error_message());
    CHECK(api.set_effect_type(0, EffectType::eax_reverb) && api.set_send_props(0, half) && api.apply_changes(), "Api setup: %s", api.get_error_message());

    ApiArray arr;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "ApiArray::initialize: %s", arr.get_error_message());
    CHECK(arr.set_effect_type_all(0, EffectType::eax_reverb), "set_effect_type_all: %s", arr.get_error_message());
    for (int i = 0; i < n; ++i) CHECK(arr.set_send_props(i, 0, half), "set_send_props: %s", arr.get_error_message());
    CHECK(arr.apply_changes(), "apply_changes: %s", arr.get_error_message());

    for (int k = 0; k < 7; ++k) {
        if (k == 3) {
            SendProps back{};
            CHECK(api.set_send_props(0, unity) && api.get_send_props(0, back) && back.gain_ == 1.0F, "Api: send back to unity");
            CHECK(api.set_effect_props(0, preset.props_) && api.apply_changes(), "Api change: %s", api.get_error_message());
            CHECK(arr.set_send_props(0, 0, unity) && arr.set_effect_props(0, 0, preset.props_) && arr.apply_changes(0), "ApiArray[0]: %s", arr.get_error_message());
            CHECK(arr.set_send_props(1, 0, unity) && !arr.set_effect(1, 0, preset) && arr.apply_changes(1), "ApiArray[1]: %s", arr.get_error_message());
            CHECK(arr.apply_changes(), "ApiArray apply: %s", arr.get_error_message()); // instance 2 keeps its 0.5 send
        }
        std::vector<std::vector<float>> src(1 + n, std::vector<float>(static_cast<size_t>(frames) * ch));
        std::vector<std::vector<float>> dst(src);
        for (int s = 0; s <= n; ++s) synth(300 + s, k, frames * ch, src[s].data());
        CHECK(api.mix(frames, src[0].data(), dst[0].data()), "Api::mix: %s", api.get_error_message());
        std::vector<const float*> sp;
        std::vector<float*> dp;
        for (int i = 0; i < n; ++i) { sp.push_back(src[1 + i].data()); dp.push_back(dst[1 + i].data()); }
        CHECK(arr.mix(frames, sp.data(), dp.data()), "ApiArray::mix: %s", arr.get_error_message());
        for (int s = 0; s <= n; ++s) out[s].insert(out[s].end(), dst[s].begin(), dst[s].end());
    }

    std::FILE* f = std::fopen(argv[1], "wb");
    CHECK(f != nullptr, "cannot open %s", argv[1]);
    for (const auto& o : out) std::fwrite(o.data(), sizeof(float), o.size(), f);
    std::fclose(f);
    std::puts("ok");
    return 0;
}
