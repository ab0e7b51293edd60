// oalsfxpp::ApiArray::program_voice_filter / get_voice_filter_program against the batch calls.  Two arrays of two stereo instances without
// effects, one lane: every voice holds one sample of a short fp32 asset (step 0), so its input is a constant per channel, and runs
// through a low-pass.  On the first array the filter of instance 1 gets a program of three segments (40, 50 and 30 frames, built with
// oalsfx_host_filter_program) through program_voice_filter; on the second the same program is set with oalsfx_batch_set_filter_programs on
// the array's batch.  Two renders of 70 frames: the buses, the programs and the filter records of the two must be the same bytes, the
// program behind the first render must stand 30 frames into its second segment with one segment queued and the first one's `to` in the
// filter, and behind the second the program is done and the filter holds the last `to`.  Then what is refused, and the queue emptied by
// sweep_voice_filter and set_voice_filter.
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
    // four nodes: up, further up, and back down
    oalsfx_voice_filter nodes[4], got, got_twin;
    std::memset(nodes, 0, sizeof(nodes));
    const float freq[4] = {0.01F, 0.05F, 0.2F, 0.02F};
    for (int k = 0; k < 4; ++k) CHECK(oalsfx_host_voice_filter(OALSFX_VF_LOW_PASS, 1.0F, freq[k], 1.0F, &nodes[k]), "oalsfx_host_voice_filter");
    oalsfx_voice_filter from = nodes[0];
    from.flags = OALSFX_VF_ACTIVE | OALSFX_VF_LOAD;
    for (ApiArray* a : {&arr, &twin}) {
        for (int i = 0; i < n; ++i) {
            s.position = static_cast<uint64_t>(i) << OALSFX_SAMPLER_FRAC_BITS; // instance i holds sample i
            CHECK(a->set_sampler(i, s) && a->set_routing(i, 0, 0.5F) && a->set_voice_filter(i, from), "set-up: %s", a->get_error_message());
        }
        CHECK(a->apply_changes(), "apply_changes");
    }
    const uint32_t lengths[3] = {40, 50, 30};
    oalsfx_filter_sweep program[OALSFX_FILTER_PROGRAM_MAX], shown[OALSFX_FILTER_PROGRAM_MAX], shown_twin[OALSFX_FILTER_PROGRAM_MAX], one_sweep;
    std::memset(program, 0, sizeof(program));
    CHECK(oalsfx_host_filter_program(nodes, lengths, 3, program), "oalsfx_host_filter_program");
    for (int k = 0; k < 3; ++k) {
        CHECK(oalsfx_host_filter_sweep(&nodes[k], &nodes[k + 1], lengths[k], &one_sweep) && std::memcmp(&one_sweep, &program[k], sizeof(one_sweep)) == 0,
              "segment %d is not oalsfx_host_filter_sweep's", k);
        if (k < 2) CHECK(std::memcmp(program[k].to, program[k + 1].from, sizeof(program[k].to)) == 0, "segment %d does not end where the next starts", k);
    }
    // what is refused: no filter under the program, a length out of range, a queued segment that is not active, an index outside the array
    oalsfx_voice_filter off = from;
    off.flags = 0;
    CHECK(arr.set_voice_filter(0, off) && !arr.program_voice_filter(0, program, 3) && std::strstr(arr.get_error_message(), "filter is not active"),
          "no filter under the program: %s", arr.get_error_message());
    CHECK(arr.set_voice_filter(0, from), "set_voice_filter: %s", arr.get_error_message());
    CHECK(!arr.program_voice_filter(1, program, 0) && std::strstr(arr.get_error_message(), "Filter program length out of range"), "length 0: %s", arr.get_error_message());
    CHECK(!arr.program_voice_filter(1, program, 9) && std::strstr(arr.get_error_message(), "Filter program length out of range"), "length 9: %s", arr.get_error_message());
    oalsfx_filter_sweep idle[2] = {program[0], program[1]};
    idle[1].flags = 0;
    CHECK(!arr.program_voice_filter(1, idle, 2) && std::strstr(arr.get_error_message(), "segment is not active"), "an idle segment: %s", arr.get_error_message());
    CHECK(!arr.program_voice_filter(n, program, 3), "an index outside the array");
    int length = -1, length_twin = -1;
    CHECK(arr.get_voice_filter_program(1, shown, length) && length == 1 && shown[0].flags == 0, "no program yet");
    CHECK(arr.program_voice_filter(1, program, 3), "program_voice_filter: %s", arr.get_error_message());
    const int one = 1, three = 3;
    CHECK(oalsfx_batch_set_filter_programs(twin.batch(), &one, 1, &three, program), "oalsfx_batch_set_filter_programs: %s", oalsfx_batch_error(twin.batch()));
    CHECK(arr.get_voice_filter_program(1, 0, shown, length) && length == 3 && std::memcmp(shown, program, 3 * sizeof(program[0])) == 0, "the program as set");
    std::vector<float> bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    for (int call = 0; call < 2; ++call) {
        CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
        CHECK(twin.play_to_buses_metered(frames, 1, want.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", twin.get_error_message());
        CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "call %d: the buses differ", call);
        CHECK(std::strcmp(oalsfx_debug_last_render_kernel(arr.batch()), "k_filter_program_rows") == 0, "call %d ran %s", call, oalsfx_debug_last_render_kernel(arr.batch()));
        CHECK(arr.get_voice_filter_program(1, shown, length) && oalsfx_batch_get_filter_programs(twin.batch(), &one, 1, &length_twin, shown_twin) &&
                  length == length_twin && std::memcmp(shown, shown_twin, length * sizeof(shown[0])) == 0,
              "call %d: the programs differ", call);
        CHECK(arr.get_voice_filter(1, got) && twin.get_voice_filter(1, got_twin) && std::memcmp(&got, &got_twin, sizeof(got)) == 0, "call %d: the filters differ", call);
        if (call == 0)
            CHECK(length == 2 && shown[0].frames == 50 && shown[0].done == 30 && shown[0].flags == OALSFX_SWEEP_ACTIVE && shown[1].frames == 30 && shown[1].done == 0 &&
                      got.b0 == nodes[1].b0 && got.a2 == nodes[1].a2,
                  "behind 70 frames: %d segments, done %u", length, shown[0].done);
        else
            CHECK(length == 1 && shown[0].frames == 30 && shown[0].done == 30 && shown[0].flags == 0 && got.b0 == nodes[3].b0 && got.a2 == nodes[3].a2 &&
                      got.flags == OALSFX_VF_ACTIVE,
                  "behind 140 frames: %d segments, done %u", length, shown[0].done);
    }
    bool moved = false;
    for (float v : bus) moved = moved || v != 0.0F;
    CHECK(moved, "the bus is silent");
    CHECK(oalsfx_debug_filter_program_uploads(arr.batch()) == 1, "%lld queue uploads", oalsfx_debug_filter_program_uploads(arr.batch()));
    // sweep_voice_filter and set_voice_filter empty the queue
    CHECK(arr.program_voice_filter(0, program, 3) && arr.sweep_voice_filter(0, nodes[2], 25) && arr.get_voice_filter_program(0, shown, length) && length == 1 &&
              shown[0].frames == 25,
          "sweep_voice_filter empties the queue: %s", arr.get_error_message());
    CHECK(arr.program_voice_filter(0, program, 3) && arr.set_voice_filter(0, from) && arr.get_voice_filter_program(0, shown, length) && length == 1 &&
              shown[0].flags == 0 && shown[0].frames == 0,
          "set_voice_filter empties the queue: %s", arr.get_error_message());
    arr.uninitialize();
    twin.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
