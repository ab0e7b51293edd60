// oalsfxpp::ApiArray::set_envelope_program / get_envelope_program.  Four stereo voices without effects loop a short fp32 asset resident
// in device memory.  In one array voice 1 gets a program of three segments -- a fade-in over five frames, three frames held, a fade that
// stops the voice over four -- and one render of sixteen frames; in its twin the same voice gets the segments one by one through
// set_envelope, with the render split at the frames 5 and 8 where they take over.  The buses and the records read back must be the same
// bytes: that is the envelope programs' contract (include/oalsfx_hip.h), and no arithmetic is restated here.  Then the get round trip,
// a plain set_envelope that empties the queue, the lanes, and the refusals with the library's messages.
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
    const int n = 4, frames = 16;
    ApiArray arr, twin;
    CHECK(arr.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", arr.get_error_message());
    CHECK(twin.initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", twin.get_error_message());
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
        s.step = 4096 / 3;
        s.format = OALSFX_PCM_F32;
        s.channels = 1;
        s.flags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP | OALSFX_SAMPLER_LINEAR;
        s.gain[0] = 0.5F;
        s.gain[1] = 0.25F;
        CHECK(arr.set_sampler(i, s) && twin.set_sampler(i, s), "set_sampler: %s", arr.get_error_message());
        CHECK(arr.set_routing(i, 0, 0.5F) && twin.set_routing(i, 0, 0.5F), "set_routing");
    }
    const float one[2] = {1.0F, 0.75F}, none[2] = {0.0F, 0.0F};
    oalsfx_envelope program[3], got[OALSFX_ENV_PROGRAM_MAX];
    std::memset(program, 0, sizeof(program));
    oalsfx_host_envelope_ramp(none, one, 2, 5, &program[0]);
    oalsfx_host_envelope_ramp(one, one, 2, 3, &program[1]);
    oalsfx_host_envelope_ramp(one, none, 2, 4, &program[2]);
    program[0].flags = program[1].flags = OALSFX_ENV_ACTIVE;
    program[2].flags = OALSFX_ENV_ACTIVE | OALSFX_ENV_STOP;
    CHECK(arr.set_envelope_program(1, 0, program, 3), "set_envelope_program: %s", arr.get_error_message());
    int length = 0;
    CHECK(arr.get_envelope_program(1, 0, got, length) && length == 3 && std::memcmp(got, program, sizeof(program)) == 0, "get_envelope_program before a render");
    CHECK(arr.get_envelope_program(0, 0, got, length) && length == 1 && got[0].flags == 0, "a voice without a program");
    CHECK(arr.apply_changes() && twin.apply_changes(), "apply_changes");
    std::vector<float> bus(frames * 2, -1.0F), want(frames * 2, -2.0F);
    CHECK(arr.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s", arr.get_error_message());
    // the twin: the same segments set one by one, the render split where they take over
    const int cuts[4] = {0, 5, 8, frames};
    for (int k = 0; k < 3; ++k) {
        CHECK(twin.set_envelope(1, program[k]), "set_envelope: %s", twin.get_error_message());
        CHECK(twin.play_to_buses_metered(cuts[k + 1] - cuts[k], 1, want.data() + cuts[k] * 2, 0.0F, false, nullptr, nullptr), "play_to_buses_metered: %s",
              twin.get_error_message());
    }
    CHECK(std::memcmp(bus.data(), want.data(), want.size() * sizeof(float)) == 0, "the bus differs from the one of the split renders");
    float loudest = 0.0F;
    for (float v : bus) loudest = v > loudest ? v : (-v > loudest ? -v : loudest);
    CHECK(loudest > 0.1F, "the bus is silent");
    oalsfx_envelope mine, theirs;
    oalsfx_sampler s, t;
    CHECK(arr.get_envelope_program(1, 0, got, length) && length == 1 && got[0].ramp_done == 4 && got[0].flags == program[2].flags, "the program read back: %d segments",
          length);
    CHECK(arr.get_envelope(1, mine) && twin.get_envelope(1, theirs) && std::memcmp(&mine, &theirs, sizeof(mine)) == 0 && std::memcmp(&mine, &got[0], sizeof(mine)) == 0,
          "the current segment differs from the twin's envelope");
    CHECK(arr.get_sampler(1, s) && twin.get_sampler(1, t) && std::memcmp(&s, &t, sizeof(s)) == 0 && !(s.flags & OALSFX_SAMPLER_PLAYING), "the stopped voice's record");
    // a plain set_envelope empties a queue
    CHECK(arr.set_envelope_program(2, 0, program, 3) && arr.set_envelope(2, program[1]), "set: %s", arr.get_error_message());
    CHECK(arr.get_envelope_program(2, 0, got, length) && length == 1 && std::memcmp(&got[0], &program[1], sizeof(got[0])) == 0, "set_envelope left a queue: %d", length);
    // the voice (index, lane)
    CHECK(!arr.set_envelope_program(0, 1, program, 2) && std::strcmp(arr.get_error_message(), "Lane out of range.") == 0, "a lane outside: %s", arr.get_error_message());
    CHECK(arr.set_polyphony(2) && arr.set_envelope_program(3, 1, program + 1, 2), "lane 1: %s", arr.get_error_message());
    CHECK(arr.get_envelope_program(3, 1, got, length) && length == 2 && std::memcmp(got, program + 1, 2 * sizeof(got[0])) == 0, "lane 1 read back");
    CHECK(arr.get_envelope_program(3, 0, got, length) && length == 1, "lane 0 beside it");
    // refusals come back as false with the library's message, and change nothing
    CHECK(!arr.set_envelope_program(3, 1, program, 0) && std::strcmp(arr.get_error_message(), "Envelope program length out of range.") == 0, "length 0: %s",
          arr.get_error_message());
    CHECK(!arr.set_envelope_program(3, 1, program, OALSFX_ENV_PROGRAM_MAX + 1) && std::strcmp(arr.get_error_message(), "Envelope program length out of range.") == 0,
          "length 9: %s", arr.get_error_message());
    oalsfx_envelope bad[2] = {program[0], program[1]};
    bad[1].flags = 0;
    CHECK(!arr.set_envelope_program(3, 1, bad, 2) && std::strcmp(arr.get_error_message(), "A program's segment is not active.") == 0, "not active: %s",
          arr.get_error_message());
    bad[1].flags = OALSFX_ENV_ACTIVE | OALSFX_ENV_GLIDE;
    CHECK(!arr.set_envelope_program(3, 1, bad, 2) && std::strcmp(arr.get_error_message(), "A program's segment glides.") == 0, "glides: %s", arr.get_error_message());
    bad[1].flags = OALSFX_ENV_ACTIVE;
    bad[1].reserved[1] = 1;
    CHECK(!arr.set_envelope_program(3, 1, bad, 2) && std::strstr(arr.get_error_message(), "reserved"), "a reserved field: %s", arr.get_error_message());
    CHECK(!arr.set_envelope_program(n, 0, program, 3) && !arr.get_envelope_program(-1, 0, got, length) && !arr.set_envelope_program(0, 0, nullptr, 1), "outside the array");
    CHECK(arr.get_envelope_program(3, 1, got, length) && length == 2 && std::memcmp(got, program + 1, 2 * sizeof(got[0])) == 0, "a refusal changed the program");
    arr.uninitialize();
    twin.uninitialize();
    (void)hipFree(dev);
    std::printf("ok\n");
    return 0;
}
