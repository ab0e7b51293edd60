// oalsfxpp::ApiArray::mix_to_buses_metered: forty voices with effects of several kinds go to three buses.  The voices' records must
// equal, bit for bit, the ones this program computes itself in the order the C header states ("level meters": lane l of
// OALSFX_METER_LANES adds its frames' squares in ascending order, then the tree s = 32 .. 1) from the outputs of forty separate
// oalsfxpp::Api objects given the same calls, the buses' records the same over the buses the call returned, and the buses themselves
// those of mix_to_buses on a second array -- once from one interleaved source, once from one source buffer per voice, with carry.
#include <cmath>
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

// One row's record in the stated order, continued from `m` (a call with carry).
static void meter_row(const float* x, int frames, int ch, float threshold, oalsfx_meter* m)
{
    const oalsfx_meter old = *m;
    std::memset(m, 0, sizeof(*m));
    long last = -1;
    for (int c = 0; c < ch; ++c) {
        volatile float q[OALSFX_METER_LANES]; // (volatile: every product and sum rounded to fp32 on its own)
        for (int l = 0; l < OALSFX_METER_LANES; ++l) q[l] = 0.0F;
        float p = 0.0F;
        for (int f = 0; f < frames; ++f) {
            const float v = x[static_cast<size_t>(f) * ch + c];
            volatile float sq = v * v;
            q[f % OALSFX_METER_LANES] = q[f % OALSFX_METER_LANES] + sq;
            p = std::fmax(p, std::fabs(v));
            if (!(std::fabs(v) < INFINITY)) ++m->nonfinite;
            if (!(std::fabs(v) <= threshold) && f > last) last = f;
        }
        for (int s = OALSFX_METER_LANES / 2; s >= 1; s /= 2)
            for (int l = 0; l < s; ++l) q[l] = q[l] + q[l + s];
        m->sumsq[c] = q[0];
        m->peak[c] = p;
        m->peak_hold = std::fmax(m->peak_hold, p);
    }
    const uint32_t quiet = static_cast<uint32_t>(frames - 1 - last);
    const uint64_t carried = static_cast<uint64_t>(old.quiet_run) + static_cast<uint64_t>(frames);
    m->quiet_run = quiet == static_cast<uint32_t>(frames) ? static_cast<uint32_t>(carried > UINT32_MAX ? UINT32_MAX : carried) : quiet;
    m->peak_hold = std::fmax(old.peak_hold, m->peak_hold);
    m->frames = static_cast<uint32_t>(frames);
}

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 40, ch = 2, buses = 3;
    const float threshold = 0.25F;
    const EffectType kinds[] = {EffectType::eax_reverb, EffectType::chorus, EffectType::echo, EffectType::reverb, EffectType::null};
    ApiArray arr, plain;
    std::vector<Api> voice(n);
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    for (int i = 0; i < n; ++i) {
        const Effect e = effect_of(kinds[i % 5]);
        arr.set_effect(i, 0, e);
        plain.set_effect(i, 0, e);
        CHECK(voice[i].initialize(ChannelFormat::stereo, 48000, 1), "Api::initialize: %s", voice[i].get_error_message());
        voice[i].set_effect(0, e);
        CHECK(voice[i].apply_changes(), "Api::apply_changes");
        const int bus = i == 7 ? -1 : i % 3;
        const float gain = 0.25F + 0.03125F * static_cast<float>(i % 9);
        CHECK(arr.set_routing(i, bus, gain) && plain.set_routing(i, bus, gain), "set_routing");
    }
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    std::vector<oalsfx_meter> vm(n), bm(buses), want_v(n), want_b(buses);
    std::memset(vm.data(), 0, n * sizeof(oalsfx_meter));
    std::memset(bm.data(), 0, buses * sizeof(oalsfx_meter));
    std::memset(want_v.data(), 0, n * sizeof(oalsfx_meter));
    std::memset(want_b.data(), 0, buses * sizeof(oalsfx_meter));
    const int sizes[] = {256, 100, 2100, 256, 256};
    for (int k = 0; k < 5; ++k) {
        const int frames = sizes[k];
        const size_t per = static_cast<size_t>(frames) * ch;
        std::vector<float> src(per * n), out(per * n), got(per * buses, -1.0F), want(per * buses);
        std::vector<const float*> rows(n);
        for (int i = 0; i < n; ++i) {
            // (the last two calls are silence, and voice 3 is nearly silent throughout: quiet runs that carry over)
            if (k < 3) synth(500 + i, k, static_cast<int>(per), src.data() + per * i);
            if (i == 3)
                for (size_t e = 0; e < per; ++e) src[per * i + e] *= 0.001F;
            rows[i] = src.data() + per * i;
            CHECK(voice[i].mix(frames, src.data() + per * i, out.data() + per * i), "Api::mix");
            meter_row(out.data() + per * i, frames, ch, threshold, &want_v[i]);
        }
        const bool ok = (k & 1) ? arr.mix_to_buses_metered(frames, rows.data(), buses, got.data(), threshold, true, vm.data(), bm.data())
                                : arr.mix_to_buses_metered(frames, src.data(), buses, got.data(), threshold, true, vm.data(), bm.data());
        CHECK(ok, "mix_to_buses_metered: %s", arr.get_error_message());
        CHECK(plain.mix_to_buses(frames, src.data(), buses, want.data()), "mix_to_buses: %s", plain.get_error_message());
        CHECK(std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "call %d: the buses differ from mix_to_buses'", k);
        for (int b = 0; b < buses; ++b) meter_row(got.data() + per * b, frames, ch, threshold, &want_b[b]);
        CHECK(std::memcmp(vm.data(), want_v.data(), n * sizeof(oalsfx_meter)) == 0, "call %d (%d frames): the voices' records differ", k, frames);
        CHECK(std::memcmp(bm.data(), want_b.data(), buses * sizeof(oalsfx_meter)) == 0, "call %d (%d frames): the buses' records differ", k, frames);
    }
    CHECK(vm[4].quiet_run >= 256 && vm[3].quiet_run >= 256 + 100 + 2100 + 256 + 256, "quiet runs: %u %u", vm[4].quiet_run, vm[3].quiet_run);
    float dummy[4] = {0.0F, 0.0F, 0.0F, 0.0F};
    CHECK(!arr.mix_to_buses_metered(1, dummy, buses, dummy, -1.0F, false, vm.data(), nullptr) && std::strstr(arr.get_error_message(), "threshold"),
          "a negative threshold: %s", arr.get_error_message());
    std::printf("ok\n");
    return 0;
}
