// oalsfxpp::ApiArray::set_stream / queue_sampler / stream_state and oalsfx_host_stream_chunks against the batch calls and against the
// whole asset.  Three arrays of two stereo instances without effects, each instance routed to bus 0 at gain 1: on `whole` instance 1
// plays a ramp of 96 fp32 frames as one asset at step 4096 + 1000; on `arr` the same record goes through oalsfx_host_stream_chunks into
// chunks of 20 frames -- the first three set with set_stream, the last two queued with queue_sampler --; on `twin` the same chunks are set
// with oalsfx_batch_set_streams and appended with oalsfx_batch_append_streams on the array's batch.  Two renders of 50 frames: the buses
// of the three must be the same bytes (nearest-sample playback: the chunks play the whole asset's bits), and the stream states and sampler
// records of arr and twin the same.  Then what is refused.
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
    const int n = 2, frames = 50, asset_frames = 96;
    float pcm[asset_frames];
    for (int i = 0; i < asset_frames; ++i) pcm[i] = 0.01F * static_cast<float>(i + 1) * ((i % 3) ? 1.0F : -1.0F);
    ApiArray whole, arr, twin;
    for (ApiArray* a : {&whole, &arr, &twin}) CHECK(a->initialize(n, ChannelFormat::stereo, 48000, 1), "initialize: %s", a->get_error_message());
    float* dev = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(pcm)) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(dev, pcm, sizeof(pcm), hipMemcpyHostToDevice) == hipSuccess, "hipMemcpy");
    oalsfx_sampler s;
    std::memset(&s, 0, sizeof(s));
    s.data = reinterpret_cast<uint64_t>(dev);
    s.frames = asset_frames;
    s.position = 777;
    s.step = 4096 + 1000;
    s.format = OALSFX_PCM_F32;
    s.channels = 1;
    s.flags = OALSFX_SAMPLER_PLAYING;
    s.gain[0] = 0.5F;
    s.gain[1] = -0.25F;
    oalsfx_sampler chunks[1 + OALSFX_STREAM_QUEUE];
    std::memset(chunks, 0, sizeof(chunks));
    // what the helper refuses, and what it makes
    oalsfx_sampler looped = s;
    looped.flags |= OALSFX_SAMPLER_LOOP;
    looped.loop_end = 10;
    CHECK(!oalsfx_host_stream_chunks(&looped, 20, 9, chunks) && !oalsfx_host_stream_chunks(&s, 0, 9, chunks) && !oalsfx_host_stream_chunks(&s, 20, 4, chunks) &&
          !oalsfx_host_stream_chunks(nullptr, 20, 9, chunks) && !oalsfx_host_stream_chunks(&s, 20, 9, nullptr), "oalsfx_host_stream_chunks takes what it must refuse");
    oalsfx_sampler late = s;
    late.position = 20ull << OALSFX_SAMPLER_FRAC_BITS;
    CHECK(!oalsfx_host_stream_chunks(&late, 20, 9, chunks) && chunks[0].data == 0, "a position outside the first chunk");
    CHECK(oalsfx_host_stream_chunks(&s, 20, 9, chunks) == 5, "five chunks");
    for (int k = 0; k < 5; ++k)
        CHECK(chunks[k].data == s.data + static_cast<uint64_t>(k) * 20 * sizeof(float) && chunks[k].frames == (k < 4 ? 20U : 16U) && chunks[k].position == (k ? 0U : 777U) &&
              chunks[k].step == s.step && chunks[k].flags == s.flags && std::memcmp(chunks[k].gain, s.gain, sizeof(s.gain)) == 0, "chunk %d", k);
    for (ApiArray* a : {&whole, &arr, &twin}) {
        for (int i = 0; i < n; ++i) CHECK(a->set_routing(i, 0, 1.0F), "set_routing: %s", a->get_error_message());
        CHECK(a->apply_changes(), "apply_changes");
    }
    CHECK(whole.set_sampler(1, s), "set_sampler: %s", whole.get_error_message());
    CHECK(arr.set_stream(1, chunks, 3) && arr.queue_sampler(1, chunks[3]) && arr.queue_sampler(1, 0, chunks[4]), "set_stream / queue_sampler: %s", arr.get_error_message());
    {
        const int voice = 1, three = 3, two = 2;
        CHECK(oalsfx_batch_set_streams(twin.batch(), &voice, 1, &three, chunks) && oalsfx_batch_append_streams(twin.batch(), &voice, 1, &two, chunks + 3),
              "the batch calls: %s", oalsfx_batch_error(twin.batch()));
    }
    uint32_t taken = 9, queued = 9, taken_twin = 9, queued_twin = 9;
    CHECK(arr.stream_state(1, taken, queued) && taken == 0 && queued == 4, "as set: taken %u, queued %u", taken, queued);
    CHECK(arr.stream_state(0, 0, taken, queued) && taken == 0 && queued == 0, "a voice without a stream");
    std::vector<float> bus(static_cast<size_t>(frames) * 2), bus_arr(bus.size()), bus_twin(bus.size());
    for (int call = 0; call < 2; ++call) {
        CHECK(whole.play_to_buses_metered(frames, 1, bus.data(), 0.0F, false, nullptr, nullptr), "play: %s", whole.get_error_message());
        CHECK(arr.play_to_buses_metered(frames, 1, bus_arr.data(), 0.0F, false, nullptr, nullptr), "play: %s", arr.get_error_message());
        CHECK(twin.play_to_buses_metered(frames, 1, bus_twin.data(), 0.0F, false, nullptr, nullptr), "play: %s", twin.get_error_message());
        CHECK(std::strcmp(oalsfx_debug_last_render_kernel(arr.batch()), "k_stream_rows") == 0 && std::strcmp(oalsfx_debug_last_render_kernel(whole.batch()), "k_sampler_rows") == 0,
              "the kernels: %s, %s", oalsfx_debug_last_render_kernel(arr.batch()), oalsfx_debug_last_render_kernel(whole.batch()));
        CHECK(std::memcmp(bus.data(), bus_arr.data(), bus.size() * sizeof(float)) == 0, "call %d: the chunks do not play the whole asset's bits", call);
        CHECK(std::memcmp(bus_arr.data(), bus_twin.data(), bus.size() * sizeof(float)) == 0, "call %d: the array and the batch calls differ", call);
        CHECK(arr.stream_state(1, taken, queued) && oalsfx_batch_get_stream_state(twin.batch(), nullptr, 2, nullptr, nullptr), "stream_state");
        const int voice = 1;
        CHECK(oalsfx_batch_get_stream_state(twin.batch(), &voice, 1, &taken_twin, &queued_twin) && taken == taken_twin && queued == queued_twin, "call %d: the states differ", call);
        // 50 frames at 5096 / 4096 from 777 / 4096: frame 62.4, in the fourth chunk; 100 frames: past the end, everything taken
        CHECK(taken == (call == 0 ? 3U : 4U) && queued == (call == 0 ? 1U : 0U), "call %d: taken %u, queued %u", call, taken, queued);
        oalsfx_sampler now, now_twin, now_whole;
        CHECK(arr.get_sampler(1, now) && twin.get_sampler(1, now_twin) && whole.get_sampler(1, now_whole) && std::memcmp(&now, &now_twin, sizeof(now)) == 0, "get_sampler");
        CHECK((now.flags & OALSFX_SAMPLER_PLAYING) == (now_whole.flags & OALSFX_SAMPLER_PLAYING), "call %d: PLAYING differs from the whole asset's", call);
        if (call == 0) CHECK(now.data == chunks[3].data && now.position + (60ull << OALSFX_SAMPLER_FRAC_BITS) == now_whole.position, "the position inside the fourth chunk");
    }
    // what is refused: a full ring, a record that does not play, a length out of range, an index outside the array; set_sampler empties the ring
    CHECK(arr.set_stream(0, chunks, 5), "set_stream: %s", arr.get_error_message());
    for (int k = 0; k < 4; ++k) CHECK(arr.queue_sampler(0, chunks[k]), "queue_sampler %d: %s", k, arr.get_error_message());
    CHECK(!arr.queue_sampler(0, chunks[0]) && std::strstr(arr.get_error_message(), "The stream queue is full."), "a full ring: %s", arr.get_error_message());
    oalsfx_sampler stopped = chunks[1];
    stopped.flags = 0;
    CHECK(!arr.queue_sampler(1, stopped) && std::strstr(arr.get_error_message(), "A queued sampler is not playing."), "not playing: %s", arr.get_error_message());
    CHECK(!arr.set_stream(1, chunks, 0) && std::strstr(arr.get_error_message(), "Stream length out of range.") && !arr.set_stream(1, chunks, 10), "lengths");
    CHECK(!arr.set_stream(2, chunks, 2) && !arr.queue_sampler(-1, chunks[0]) && !arr.stream_state(2, taken, queued) && !arr.set_stream(1, nullptr, 1), "indices");
    CHECK(!arr.set_stream(1, 1, chunks, 2) && std::strstr(arr.get_error_message(), "Lane out of range."), "lanes: %s", arr.get_error_message());
    CHECK(arr.stream_state(0, taken, queued) && taken == 0 && queued == 8, "the full ring: taken %u, queued %u", taken, queued);
    CHECK(arr.set_sampler(0, chunks[0]) && arr.stream_state(0, taken, queued) && taken == 0 && queued == 0, "set_sampler empties the ring");
    hipFree(dev);
    std::printf("ok\n");
    return 0;
}
