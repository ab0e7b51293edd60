// oalsfxpp::ApiArray::sweep_voice_filter / get_voice_filter_sweep against the batch calls.  Two arrays of two stereo instances without
// effects, one lane: every voice holds one sample of a short fp32 asset (step 0), so its input is a constant per channel, and runs
// through a low-pass.  On the first array the filter of instance 1 is swept to another low-pass over 100 frames with
// sweep_voice_filter; on the second the same record, built here with oalsfx_host_filter_sweep, is set with oalsfx_batch_set_sweeps on the
// array's batch.  Two renders of 70 frames, the sweep completing in the second: the buses, the sweep records and the filter records of
// the two must be the same bytes, the record behind the first render must say 70 frames done, and behind the second the filter holds `to`.
// Then what is refused, a second sweep set in mid-sweep, and the cancel by set_voice_filter.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "oalsfx_hip.h"
#include "oalsfx_hip_debug.h"
#include "oalsfxpp_array.h"

using namespace oalsfxpp;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main()
{
    const int n = 2, frames = 70;
    const uint32_t length = 100;
    const float pcm[2] = {0.75F, -0.5F};
    ApiArray arr, twin;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(twin.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", twin.get_error_message());
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(pcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, pcm, sizeof(pcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    oalsfx_sampler s;
    std::memset(&s, 0, sizeof(s));
    s.data = reinterpret_cast<uint64_t>(dev);
    s.frames = 2;
    s.loop_end = 2;
    s.format = OALSFX_PCM_F32;
    s.channels = 1;
    s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP;
    s.gain[0] = 0.5F;
    s.gain[1] = -0.25F;
    oalsfx_voice_filter from, to, got, got_twin;
    std::memset(&from, 0, sizeof(from));
    std::memset(&to, 0, sizeof(to));
    CHECK(oalsfx_host_voice_filter(OALSFX_VF_LOW_PASS, 1.0F, 0.01F, 1.0F, &from) && oalsfx_host_voice_filter(OALSFX_VF_LOW_PASS, 1.0F, 0.2F, 0.7F, &to),
          "oalsfx_host_voice_filter");
    from.flags = OALSFX_VF_ACTIVE | OALSFX_VF_LOAD;
    oalsfx_filter_sweep sweep, shown, shown_twin;
    for (ApiArray* a : {&arr, &twin}) {
        for (int i = 0; i < n; ++i) {
            s.position = static_cast<uint64_t>(i) << OALSFX_SAMPLER_FRAC_BITS; // instance i holds sample i
            CHECK(a->set_sampler(i, s) && a->set_routing(i, 0, 0.5F) && a->set_voice_filter(i, from), "set-up: %s", a->get_error_message());
        }
        CHECK(a->apply_changes(), "apply_changes");
    }
    // what is refused: no filter under the sweep, a length out of range, an index outside the array
    oalsfx_voice_filter off = from;
    off.flags = 0;
    CHECK(arr.set_voice_filter(0, off) && !arr.sweep_voice_filter(0, to, length) && std::strstr(arr.get_error_message(), "filter is not active"),
          "no filter under the sweep: %s", arr.get_error_message());
    CHECK(arr.set_voice_filter(0, from), "set_voice_filter: %s", arr.get_error_message());
    CHECK(!arr.sweep_voice_filter(1, to, 0) && std::strstr(arr.get_error_message(), "frame count is out of range"), "0 frames: %s", arr.get_error_message());
    CHECK(!arr.sweep_voice_filter(n, to, length), "an index outside the array");
    CHECK(arr.get_voice_filter_sweep(1, shown) && shown.flags == 0 && shown.frames == 0, "no sweep yet");
    CHECK(arr.sweep_voice_filter(1, to, length), "sweep_voice_filter: %s", arr.get_error_message());
    from.flags = OALSFX_VF_ACTIVE;
    CHECK(oalsfx_host_filter_sweep(&from, &to, length, &sweep) && sweep.flags == OALSFX_SWEEP_ACTIVE && sweep.frames == length && sweep.done == 0,
          "oalsfx_host_filter_sweep");
    CHECK(sweep.step[0] == (to.b0 - from.b0) / static_cast<float>(length) && sweep.from[3] == from.a1 && sweep.to[4] == to.a2, "the helper's arithmetic");
    const int one = 1;
    CHECK(oalsfx_batch_set_sweeps(twin.batch(), &one, 1, &sweep), "oalsfx_batch_set_sweeps: %s", oalsfx_batch_error(twin.batch()));
    CHECK(arr.get_voice_filter_sweep(1, 0, shown) && std::memcmp(&shown, &sweep, sizeof(sweep)) == 0, "the record sweep_voice_filter set is the helper's");
    std::vector<float> bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    for (int call = 0; call < 2; ++call) {
        CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
        CHECK(twin.play_to_buses_metered(frames, 1, want.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", twin.get_error_message());
        CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "call %d: the buses differ", call);
        CHECK(std::strcmp(oalsfx_debug_last_render_kernel(arr.batch()), "k_sweep_rows") == 0, "call %d ran %s", call, oalsfx_debug_last_render_kernel(arr.batch()));
        CHECK(arr.get_voice_filter_sweep(1, shown) && oalsfx_batch_get_sweeps(twin.batch(), &one, 1, &shown_twin) && std::memcmp(&shown, &shown_twin, sizeof(shown)) == 0,
              "call %d: the sweep records differ", call);
        CHECK(arr.get_voice_filter(1, got) && twin.get_voice_filter(1, got_twin) && std::memcmp(&got, &got_twin, sizeof(got)) == 0, "call %d: the filters differ", call);
        if (call == 0) CHECK(shown.done == 70 && shown.flags == OALSFX_SWEEP_ACTIVE && got.b0 == from.b0, "behind 70 frames: done %u", shown.done);
        else CHECK(shown.done == length && shown.flags == 0 && got.b0 == to.b0 && got.a2 == to.a2 && got.flags == OALSFX_VF_ACTIVE, "behind 140 frames: done %u", shown.done);
    }
    bool moved = false;
    for (float v : bus) moved = moved || v != 0.0F;
    CHECK(moved, "the bus is silent");
    // a voice swept again in mid-sweep goes on from the frame its sweep has reached, not from the old start
    CHECK(arr.sweep_voice_filter(0, to, length) && arr.get_voice_filter_sweep(0, sweep), "sweep_voice_filter: %s", arr.get_error_message());
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    CHECK(arr.sweep_voice_filter(0, from, 50) && arr.get_voice_filter_sweep(0, shown) && shown.done == 0 && shown.frames == 50, "the second sweep: %s", arr.get_error_message());
    for (int k = 0; k < 5; ++k) {
        volatile float product = static_cast<float>(frames) * sweep.step[k]; // (volatile: rounded to fp32 on its own)
        volatile float at = sweep.from[k] + product;
        CHECK(shown.from[k] == at && shown.from[k] != sweep.from[k], "coefficient %d of the second sweep's start", k);
    }
    // set_voice_filter cancels a sweep under way
    CHECK(arr.sweep_voice_filter(0, to, length) && arr.set_voice_filter(0, from) && arr.get_voice_filter_sweep(0, shown) && shown.flags == 0 && shown.frames == 0,
          "set_voice_filter cancels: %s", arr.get_error_message());
    arr.uninitialize();
    twin.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
