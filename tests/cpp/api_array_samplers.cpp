// oalsfxpp::ApiArray::set_sampler / get_sampler / play_to_buses_metered: forty voices with effects of several kinds play three assets
// resident in device memory -- 16-bit mono, looped and one-shot, interpolated --, into three buses.  Buses and records must equal, bit for
// bit, those of mix_to_buses_metered on a second array fed the render this program computes itself in the order the C header states
// ("samplers"), and the records read back must be the ones that arithmetic leaves.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "oalsfx_hip.h"
#include "oalsfxpp_array.h"

using namespace oalsfxpp;

static Effect effect_of(EffectType t)
{
    Effect e;
    e.set_type_and_defaults(t);
    return e;
}

static uint64_t wrap(uint64_t q, const oalsfx_sampler& s)
{
    if (!(s.flags & OALSFX_SAMPLER_LOOP)) return q;
    const uint64_t l0 = static_cast<uint64_t>(s.loop_start) << 12, l1 = static_cast<uint64_t>(s.loop_end) << 12;
    return q < l1 ? q : l0 + (q - l0) % (l1 - l0);
}

// One stereo row from a mono S16 asset in the stated order; advances the record.
static void render_row(oalsfx_sampler* s, const int16_t* pcm, int frames, float* out)
{
    std::memset(out, 0, static_cast<size_t>(frames) * 2 * sizeof(float));
    if (!(s->flags & OALSFX_SAMPLER_PLAYING)) return;
    const bool loop = (s->flags & OALSFX_SAMPLER_LOOP) != 0, linear = (s->flags & OALSFX_SAMPLER_LINEAR) != 0;
    const uint64_t end = static_cast<uint64_t>(s->frames) << 12;
    for (int f = 0; f < frames; ++f) {
        const uint64_t q = wrap(s->position + static_cast<uint64_t>(f) * s->step, *s);
        if (!loop && q >= end) continue;
        const uint32_t i = static_cast<uint32_t>(q >> 12), m = static_cast<uint32_t>(q & 4095);
        uint32_t j = i + 1;
        if (loop && j == s->loop_end) j = s->loop_start;
        volatile float a = static_cast<float>(pcm[i]) / 32768.0F; // (volatile: every operation rounded to fp32 on its own)
        volatile float b = (!loop && j == s->frames) ? 0.0F : static_cast<float>(pcm[j]) / 32768.0F;
        volatile float mu = static_cast<float>(m) * (1.0F / 4096.0F);
        volatile float d = b - a;
        volatile float p = d * mu;
        volatile float v = linear ? a + p : a;
        for (int c = 0; c < 2; ++c) {
            volatile float o = v * s->gain[c];
            out[static_cast<size_t>(f) * 2 + c] = o;
        }
    }
    uint64_t after = wrap(s->position + static_cast<uint64_t>(frames) * s->step, *s);
    if (!loop && after >= end) {
        after = end;
        s->flags &= ~static_cast<uint32_t>(OALSFX_SAMPLER_PLAYING);
    }
    s->position = after;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 40, ch = 2, buses = 3, n_assets = 3;
    const float threshold = 0.05F;
    const EffectType kinds[] = {EffectType::eax_reverb, EffectType::chorus, EffectType::echo, EffectType::reverb, EffectType::null};
    ApiArray arr, plain;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(plain.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", plain.get_error_message());
    // the assets: xorshift noise, 3000, 5000 and 7000 frames, one device allocation each
    std::vector<std::vector<int16_t>> pcm(n_assets);
    int16_t* dev[n_assets];
    for (int a = 0; a < n_assets; ++a) {
        pcm[a].resize(3000 + 2000 * a);
        uint32_t x = 0x9E3779B9u + static_cast<uint32_t>(a);
        for (auto& v : pcm[a]) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            v = static_cast<int16_t>(x >> 16);
        }
        CHECK(hipMalloc(reinterpret_cast<void**>(&dev[a]), pcm[a].size() * sizeof(int16_t)) == hipSuccess, "hipMalloc");
        CHECK(hipMemcpy(dev[a], pcm[a].data(), pcm[a].size() * sizeof(int16_t), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    }
    std::vector<oalsfx_sampler> want(n);
    for (int i = 0; i < n; ++i) {
        const Effect e = effect_of(kinds[i % 5]);
        arr.set_effect(i, 0, e);
        plain.set_effect(i, 0, e);
        const int bus = i == 7 ? -1 : i % 3;
        const float gain = 0.25F + 0.03125F * static_cast<float>(i % 9);
        CHECK(arr.set_routing(i, bus, gain) && plain.set_routing(i, bus, gain), "set_routing");
        oalsfx_sampler s;
        std::memset(&s, 0, sizeof(s));
        const int a = i % n_assets;
        s.data = reinterpret_cast<uint64_t>(dev[a]);
        s.frames = static_cast<uint32_t>(pcm[a].size());
        s.position = (static_cast<uint64_t>(17 * i) << 12) + static_cast<uint64_t>(i * 97 % 4096);
        s.step = 4096u - 300u + 37u * static_cast<uint32_t>(i);
        s.format = OALSFX_PCM_S16;
        s.channels = 1;
        s.flags = OALSFX_SAMPLER_PLAYING | (i % 4 ? OALSFX_SAMPLER_LINEAR : 0) | (i % 2 ? OALSFX_SAMPLER_LOOP : 0);
        s.loop_start = 100u + static_cast<uint32_t>(i);
        s.loop_end = 1000u + 40u * static_cast<uint32_t>(i);
        s.gain[0] = 0.125F * static_cast<float>(1 + i % 5);
        s.gain[1] = 0.6F - 0.01F * static_cast<float>(i);
        if (i == 11) s.flags = 0; // a voice that does not play
        want[i] = s;
        CHECK(arr.set_sampler(i, s), "set_sampler: %s", arr.get_error_message());
    }
    CHECK(arr.apply_changes() && plain.apply_changes(), "apply_changes");
    std::vector<oalsfx_meter> vm(n), bm(buses), want_v(n), want_b(buses);
    std::memset(vm.data(), 0, n * sizeof(oalsfx_meter));
    std::memset(bm.data(), 0, buses * sizeof(oalsfx_meter));
    std::memset(want_v.data(), 0, n * sizeof(oalsfx_meter));
    std::memset(want_b.data(), 0, buses * sizeof(oalsfx_meter));
    const int sizes[] = {256, 100, 2100, 256, 4000, 256};
    for (int k = 0; k < 6; ++k) {
        const int frames = sizes[k];
        const size_t per = static_cast<size_t>(frames) * ch;
        std::vector<float> src(per * n), got(per * buses, -1.0F), expect(per * buses);
        for (int i = 0; i < n; ++i) render_row(&want[i], pcm[i % n_assets].data(), frames, src.data() + per * i);
        CHECK(arr.play_to_buses_metered(frames, buses, got.data(), threshold, true, vm.data(), k == 3 ? nullptr : bm.data()), "play_to_buses_metered: %s",
              arr.get_error_message());
        CHECK(plain.mix_to_buses_metered(frames, src.data(), buses, expect.data(), threshold, true, want_v.data(), k == 3 ? nullptr : want_b.data()),
              "mix_to_buses_metered: %s", plain.get_error_message());
        CHECK(std::memcmp(got.data(), expect.data(), expect.size() * sizeof(float)) == 0, "call %d (%d frames): the buses differ", k, frames);
        CHECK(std::memcmp(vm.data(), want_v.data(), n * sizeof(oalsfx_meter)) == 0, "call %d (%d frames): the voices' records differ", k, frames);
        CHECK(std::memcmp(bm.data(), want_b.data(), buses * sizeof(oalsfx_meter)) == 0, "call %d (%d frames): the buses' records differ", k, frames);
        for (int i = 0; i < n; ++i) {
            oalsfx_sampler s;
            CHECK(arr.get_sampler(i, s), "get_sampler: %s", arr.get_error_message());
            CHECK(std::memcmp(&s, &want[i], sizeof(s)) == 0, "call %d: the record of voice %d differs (position %llu, expected %llu; flags %u, expected %u)", k, i,
                  static_cast<unsigned long long>(s.position), static_cast<unsigned long long>(want[i].position), s.flags, want[i].flags);
        }
    }
    int finished = 0;
    for (int i = 0; i < n; ++i) finished += !(want[i].flags & OALSFX_SAMPLER_PLAYING) && i != 11;
    CHECK(finished >= 1 && finished < n / 2, "%d one-shots finished", finished); // (voice 0: 6968 frames at a step of 0.93 outlast its 3000; voice 2 has 7000)
    // an asset one frame longer than the allocation it lies in, as the runtime has it
    oalsfx_sampler bad = want[1];
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    CHECK(hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(dev[1])) == hipSuccess, "hipMemGetAddressRange");
    bad.frames = static_cast<uint32_t>((reinterpret_cast<uint64_t>(base) + size - bad.data) / sizeof(int16_t));
    CHECK(bad.frames >= want[1].frames && arr.set_sampler(1, bad), "an asset that ends with its allocation: %s", arr.get_error_message());
    CHECK(arr.set_sampler(1, want[1]), "set_sampler: %s", arr.get_error_message());
    bad.frames += 1;
    CHECK(!arr.set_sampler(1, bad) && std::strstr(arr.get_error_message(), "one allocation"), "an asset longer than its buffer: %s", arr.get_error_message());
    CHECK(!arr.set_sampler(n, want[0]) && !arr.get_sampler(-1, bad), "an index outside the array");
    arr.uninitialize();
    for (int a = 0; a < n_assets; ++a) (void)hipFree(dev[a]);
    std::printf("ok\n");
    return 0;
}
