// oalsfxpp::ApiArray (include/oalsfxpp_array.h): many Api objects' worth of effect chains as one batch.  Argument checks, return
// values and messages follow Api's (api.cpp; reference src/oalsfxpp.cpp:3449-3903).
#include <cstdlib>
#include <cstring>

#include "oalsfx_hip.h"
#include "oalsfxpp_array.h"

namespace oalsfxpp {

namespace {
constexpr const char* err_none = "";
constexpr const char* err_not_initialized = "Not initialized.";
constexpr const char* err_index = "Effect index is out of range.";
constexpr const char* err_instance = "Instance index is out of range.";
constexpr const char* err_no_src = "No source samples.";
constexpr const char* err_no_dst = "No destination samples.";

const oalsfx_effect* as_c(const Effect& e) { return reinterpret_cast<const oalsfx_effect*>(&e); }
static_assert(sizeof(Effect) == sizeof(oalsfx_effect), "oalsfx_effect mirrors oalsfxpp::Effect");
static_assert(sizeof(SendProps) == sizeof(oalsfx_send_props), "oalsfx_send_props mirrors oalsfxpp::SendProps");
} // namespace

ApiArray::ApiArray() : batch_(nullptr), count_(0), channels_(0), effects_(0), error_(err_none) {}
ApiArray::~ApiArray() { uninitialize(); }

bool ApiArray::initialize(int count, ChannelFormat channel_format, int sampling_rate, int effect_count, int device)
{
    uninitialize();
    if (device < 0) {
        device = 0;
        if (const char* env = std::getenv("OALSFX_DEVICE")) {
            char* end = nullptr;
            const long v = std::strtol(env, &end, 10);
            device = (end != env && *end == 0 && v >= 0 && v < (1 << 16)) ? static_cast<int>(v) : -1;
        }
    }
    batch_ = oalsfx_batch_create(count, static_cast<int>(channel_format), sampling_rate, effect_count, device);
    if (!batch_) {
        error_ = oalsfx_last_error();
        return false;
    }
    count_ = count;
    channels_ = oalsfx_batch_channels(batch_);
    effects_ = effect_count;
    error_ = err_none;
    return true;
}

bool ApiArray::is_initialized() const { return batch_ != nullptr; }

void ApiArray::uninitialize()
{
    if (batch_) oalsfx_batch_destroy(batch_);
    batch_ = nullptr;
    count_ = channels_ = effects_ = 0;
}

int ApiArray::size() const { return count_; }
int ApiArray::get_channel_count() const { return channels_; }
int ApiArray::get_effect_count() const { return effects_; }
const char* ApiArray::get_error_message() const { return error_; }
oalsfx_batch* ApiArray::batch() const { return batch_; }

#define OALSFXPP_ARRAY_CHECK(index, effect_index, allow_direct)                                        \
    if (!batch_) { error_ = err_not_initialized; return false; }                                       \
    if ((index) < 0 || (index) >= count_) { error_ = err_instance; return false; }                      \
    if ((effect_index) >= effects_ || (!(allow_direct) && (effect_index) < 0)) { error_ = err_index; return false; }

bool ApiArray::get_effect(int index, int effect_index, Effect& effect) const
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, false);
    return oalsfx_batch_get_effect(batch_, index, effect_index, 0, reinterpret_cast<oalsfx_effect*>(&effect)) != 0;
}

bool ApiArray::get_deferred_effect(int index, int effect_index, Effect& effect) const
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, false);
    return oalsfx_batch_get_effect(batch_, index, effect_index, 1, reinterpret_cast<oalsfx_effect*>(&effect)) != 0;
}

bool ApiArray::set_effect_type(int index, int effect_index, EffectType effect_type)
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, false);
    if (!oalsfx_batch_set_effect_type(batch_, index, 1, effect_index, static_cast<int>(effect_type))) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_effect_props(int index, int effect_index, const EffectProps& effect_props)
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, false);
    if (!oalsfx_batch_set_effect_props(batch_, index, 1, effect_index, &effect_props, 0)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_effect(int index, int effect_index, const Effect& effect)
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, false);
    if (!oalsfx_batch_set_effect(batch_, index, 1, effect_index, as_c(effect), 0)) error_ = oalsfx_batch_error(batch_);
    return false; // (the reference's Api::set_effect returns false on success too, src/oalsfxpp.cpp:3657)
}

bool ApiArray::set_send_props(int index, int effect_index, const SendProps& send_props)
{
    OALSFXPP_ARRAY_CHECK(index, effect_index, true);
    if (!oalsfx_batch_set_send_props(batch_, index, 1, effect_index, reinterpret_cast<const oalsfx_send_props*>(&send_props))) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_effect_type_all(int effect_index, EffectType effect_type)
{
    OALSFXPP_ARRAY_CHECK(0, effect_index, false);
    if (!oalsfx_batch_set_effect_type(batch_, 0, count_, effect_index, static_cast<int>(effect_type))) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_effect_all(int effect_index, const Effect& effect)
{
    OALSFXPP_ARRAY_CHECK(0, effect_index, false);
    if (!oalsfx_batch_set_effect(batch_, 0, count_, effect_index, as_c(effect), 0)) error_ = oalsfx_batch_error(batch_);
    return false;
}

bool ApiArray::apply_changes()
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (!oalsfx_batch_apply_changes(batch_, 0, count_)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::apply_changes(int index)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!oalsfx_batch_apply_changes(batch_, index, 1)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::reset(int index)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!oalsfx_batch_reset(batch_, &index, 1)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_routing(int index, int bus, float gain)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!oalsfx_batch_set_routing(batch_, index, 1, &bus, &gain)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_send(int index, int send, int bus, float gain)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!oalsfx_batch_set_send_routing(batch_, send, index, 1, &bus, &gain)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::ramp_send(int index, int send, float gain_to, uint32_t frames)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!oalsfx_batch_set_send_ramps(batch_, send, index, 1, &gain_to, frames)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::get_send(int index, int send, int& bus, float& gain, float& gain_to, uint32_t& frames_left)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (send < 0 || send >= OALSFX_BUS_SENDS) { error_ = "Send out of range."; return false; }
    // (the get call is const and leaves no message: with the index and the send checked above it has nothing left to refuse)
    if (!oalsfx_batch_get_send_routing(batch_, index, send, &bus, &gain, &gain_to, &frames_left)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::mix_to_buses(int sample_count, const float* src_samples, int bus_count, float* dst_buses)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_buses) { error_ = err_no_dst; return false; }
    if (!oalsfx_batch_mix_downmix(batch_, sample_count, src_samples, bus_count, dst_buses)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::mix_to_buses(int sample_count, const float* const* src_samples, int bus_count, float* dst_buses)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_buses) { error_ = err_no_dst; return false; }
    if (sample_count < 0) { error_ = "Frame count is negative."; return false; }
    for (int i = 0; i < count_; ++i)
        if (!src_samples[i]) { error_ = err_no_src; return false; }
    // gathered into one interleaved source (what oalsfx_batch_mix_gather does for its two directions)
    const size_t per = static_cast<size_t>(sample_count) * channels_;
    gathered_.resize(per * count_);
    for (int i = 0; i < count_; ++i) std::memcpy(gathered_.data() + per * i, src_samples[i], per * sizeof(float));
    return mix_to_buses(sample_count, gathered_.data(), bus_count, dst_buses);
}

bool ApiArray::mix_to_buses_metered(int sample_count, const float* src_samples, int bus_count, float* dst_buses, float threshold, bool carry,
                                    oalsfx_meter* voice_meters, oalsfx_meter* bus_meters)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_buses) { error_ = err_no_dst; return false; }
    if (!oalsfx_batch_mix_downmix_meter(batch_, sample_count, src_samples, bus_count, dst_buses, threshold, carry ? OALSFX_METER_CARRY : 0, voice_meters,
                                        bus_meters)) {
        error_ = oalsfx_batch_error(batch_);
        return false;
    }
    return true;
}

bool ApiArray::mix_to_buses_metered(int sample_count, const float* const* src_samples, int bus_count, float* dst_buses, float threshold, bool carry,
                                    oalsfx_meter* voice_meters, oalsfx_meter* bus_meters)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_buses) { error_ = err_no_dst; return false; }
    if (sample_count < 0) { error_ = "Frame count is negative."; return false; }
    for (int i = 0; i < count_; ++i)
        if (!src_samples[i]) { error_ = err_no_src; return false; }
    const size_t per = static_cast<size_t>(sample_count) * channels_;
    gathered_.resize(per * count_);
    for (int i = 0; i < count_; ++i) std::memcpy(gathered_.data() + per * i, src_samples[i], per * sizeof(float));
    return mix_to_buses_metered(sample_count, gathered_.data(), bus_count, dst_buses, threshold, carry, voice_meters, bus_meters);
}

// The calls without a lane are the lane calls with lane 0, as the C calls are.
bool ApiArray::set_sampler(int index, const oalsfx_sampler& sampler) { return set_sampler(index, 0, sampler); }
bool ApiArray::get_sampler(int index, oalsfx_sampler& sampler) { return get_sampler(index, 0, sampler); }
bool ApiArray::set_envelope(int index, const oalsfx_envelope& envelope) { return set_envelope(index, 0, envelope); }
bool ApiArray::get_envelope(int index, oalsfx_envelope& envelope) { return get_envelope(index, 0, envelope); }
bool ApiArray::set_resampler(int index, int table) { return set_resampler(index, 0, table); }
bool ApiArray::get_resampler(int index, int& table) { return get_resampler(index, 0, table); }
bool ApiArray::set_voice_filter(int index, const oalsfx_voice_filter& filter) { return set_voice_filter(index, 0, filter); }
bool ApiArray::get_voice_filter(int index, oalsfx_voice_filter& filter) { return get_voice_filter(index, 0, filter); }
bool ApiArray::sweep_voice_filter(int index, const oalsfx_voice_filter& to, uint32_t frames) { return sweep_voice_filter(index, 0, to, frames); }
bool ApiArray::get_voice_filter_sweep(int index, oalsfx_filter_sweep& sweep) { return get_voice_filter_sweep(index, 0, sweep); }
bool ApiArray::program_voice_filter(int index, const oalsfx_filter_sweep* segments, int count) { return program_voice_filter(index, 0, segments, count); }
bool ApiArray::get_voice_filter_program(int index, oalsfx_filter_sweep* segments, int& count) { return get_voice_filter_program(index, 0, segments, count); }

bool ApiArray::set_fir_table(int table, int taps, int phase_bits, const float* coef)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (!oalsfx_batch_set_fir_table(batch_, table, taps, phase_bits, coef)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::set_polyphony(int lanes)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (!oalsfx_batch_set_polyphony(batch_, lanes)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

int ApiArray::get_polyphony() const { return batch_ ? oalsfx_batch_get_polyphony(batch_) : 0; }

// The tail of a call that hands on to the batch: the batch's message kept where it refuses.
#define OALSFXPP_ARRAY_CALL(call)                                                                      \
    if (!(call)) { error_ = oalsfx_batch_error(batch_); return false; }                                \
    return true
// A call on the record of one voice (lane, index): the index checked first.
#define OALSFXPP_ARRAY_VOICE(name, record)                                                             \
    OALSFXPP_ARRAY_CHECK(index, 0, false);                                                             \
    OALSFXPP_ARRAY_CALL(oalsfx_batch_##name(batch_, lane, &index, 1, &record))

bool ApiArray::set_sampler(int index, int lane, const oalsfx_sampler& sampler) { OALSFXPP_ARRAY_VOICE(set_lane_samplers, sampler); }
bool ApiArray::get_sampler(int index, int lane, oalsfx_sampler& sampler) { OALSFXPP_ARRAY_VOICE(get_lane_samplers, sampler); }
bool ApiArray::set_envelope(int index, int lane, const oalsfx_envelope& envelope) { OALSFXPP_ARRAY_VOICE(set_lane_envelopes, envelope); }
bool ApiArray::get_envelope(int index, int lane, oalsfx_envelope& envelope) { OALSFXPP_ARRAY_VOICE(get_lane_envelopes, envelope); }
bool ApiArray::set_resampler(int index, int lane, int table) { OALSFXPP_ARRAY_VOICE(set_lane_resamplers, table); }
bool ApiArray::get_resampler(int index, int lane, int& table) { OALSFXPP_ARRAY_VOICE(get_lane_resamplers, table); }
bool ApiArray::set_voice_filter(int index, int lane, const oalsfx_voice_filter& filter) { OALSFXPP_ARRAY_VOICE(set_lane_filters, filter); }
bool ApiArray::get_voice_filter(int index, int lane, oalsfx_voice_filter& filter) { OALSFXPP_ARRAY_VOICE(get_lane_filters, filter); }
bool ApiArray::get_voice_filter_sweep(int index, int lane, oalsfx_filter_sweep& sweep) { OALSFXPP_ARRAY_VOICE(get_lane_sweeps, sweep); }

bool ApiArray::sweep_voice_filter(int index, int lane, const oalsfx_voice_filter& to, uint32_t frames)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    oalsfx_voice_filter now;
    if (!oalsfx_batch_get_lane_filters(batch_, lane, &index, 1, &now)) { error_ = oalsfx_batch_error(batch_); return false; }
    oalsfx_filter_sweep sweep;
    if (!oalsfx_batch_get_lane_sweeps(batch_, lane, &index, 1, &sweep)) { error_ = oalsfx_batch_error(batch_); return false; }
    if ((sweep.flags & OALSFX_SWEEP_ACTIVE) && sweep.done < sweep.frames) {
        // a sweep is under way: the filter record still holds the coefficients it was set with, and the ramp stands at frame `done`, whose
        // coefficients are the contract's from[k] + ((float)done * step[k]) -- the new sweep starts there and not back at the old start
        float at[5];
        for (int k = 0; k < 5; ++k) at[k] = sweep.from[k] + (static_cast<float>(sweep.done) * sweep.step[k]);
        now.b0 = at[0];
        now.b1 = at[1];
        now.b2 = at[2];
        now.a1 = at[3];
        now.a2 = at[4];
    }
    if (!oalsfx_host_filter_sweep(&now, &to, frames, &sweep)) { error_ = "The filter sweep's frame count is out of range."; return false; }
    OALSFXPP_ARRAY_CALL(oalsfx_batch_set_lane_sweeps(batch_, lane, &index, 1, &sweep));
}

bool ApiArray::set_envelope_program(int index, int lane, const oalsfx_envelope* segments, int length)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!segments) { error_ = "No envelope records."; return false; }
    // (the C call reads a row of OALSFX_ENV_PROGRAM_MAX records per voice: the caller's array may be shorter)
    oalsfx_envelope row[OALSFX_ENV_PROGRAM_MAX] = {};
    for (int k = 0; k < length && k < OALSFX_ENV_PROGRAM_MAX; ++k) row[k] = segments[k];
    OALSFXPP_ARRAY_CALL(oalsfx_batch_set_lane_env_programs(batch_, lane, &index, 1, &length, row));
}

bool ApiArray::get_envelope_program(int index, int lane, oalsfx_envelope* segments, int& length)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!segments) { error_ = "No envelope records."; return false; }
    OALSFXPP_ARRAY_CALL(oalsfx_batch_get_lane_env_programs(batch_, lane, &index, 1, &length, segments));
}

bool ApiArray::set_stream(int index, int lane, const oalsfx_sampler* records, int length)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!records) { error_ = "No sampler records."; return false; }
    // (the C call reads a row of 1 + OALSFX_STREAM_QUEUE records per voice: the caller's array may be shorter)
    oalsfx_sampler row[1 + OALSFX_STREAM_QUEUE] = {};
    for (int k = 0; k < length && k < 1 + OALSFX_STREAM_QUEUE; ++k) row[k] = records[k];
    OALSFXPP_ARRAY_CALL(oalsfx_batch_set_lane_streams(batch_, lane, &index, 1, &length, row));
}

bool ApiArray::queue_sampler(int index, int lane, const oalsfx_sampler& record)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    oalsfx_sampler row[OALSFX_STREAM_QUEUE] = {};
    row[0] = record;
    const int one = 1;
    OALSFXPP_ARRAY_CALL(oalsfx_batch_append_lane_streams(batch_, lane, &index, 1, &one, row));
}

bool ApiArray::stream_state(int index, int lane, uint32_t& taken, uint32_t& queued)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    OALSFXPP_ARRAY_CALL(oalsfx_batch_get_lane_stream_state(batch_, lane, &index, 1, &taken, &queued));
}

bool ApiArray::set_stream(int index, const oalsfx_sampler* records, int length) { return set_stream(index, 0, records, length); }
bool ApiArray::queue_sampler(int index, const oalsfx_sampler& record) { return queue_sampler(index, 0, record); }
bool ApiArray::stream_state(int index, uint32_t& taken, uint32_t& queued) { return stream_state(index, 0, taken, queued); }

bool ApiArray::program_voice_filter(int index, int lane, const oalsfx_filter_sweep* segments, int count)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!segments) { error_ = "No filter sweep records."; return false; }
    // (the C call reads a row of OALSFX_FILTER_PROGRAM_MAX records per voice: the caller's array may be shorter)
    oalsfx_filter_sweep row[OALSFX_FILTER_PROGRAM_MAX] = {};
    for (int k = 0; k < count && k < OALSFX_FILTER_PROGRAM_MAX; ++k) row[k] = segments[k];
    OALSFXPP_ARRAY_CALL(oalsfx_batch_set_lane_filter_programs(batch_, lane, &index, 1, &count, row));
}

bool ApiArray::get_voice_filter_program(int index, int lane, oalsfx_filter_sweep* segments, int& count)
{
    OALSFXPP_ARRAY_CHECK(index, 0, false);
    if (!segments) { error_ = "No filter sweep records."; return false; }
    OALSFXPP_ARRAY_CALL(oalsfx_batch_get_lane_filter_programs(batch_, lane, &index, 1, &count, segments));
}

bool ApiArray::play_to_buses_metered(int sample_count, int bus_count, float* dst_buses, float threshold, bool carry, oalsfx_meter* voice_meters,
                                     oalsfx_meter* bus_meters)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!dst_buses) { error_ = err_no_dst; return false; }
    if (!oalsfx_batch_play_downmix_meter(batch_, sample_count, bus_count, dst_buses, threshold, carry ? OALSFX_METER_CARRY : 0, voice_meters, bus_meters)) {
        error_ = oalsfx_batch_error(batch_);
        return false;
    }
    return true;
}

bool ApiArray::mix(int sample_count, const float* const* src_samples, float* const* dst_samples)
{
    // Api::mix's preconditions (reference src/oalsfxpp.cpp:3790-3811)
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_samples) { error_ = err_no_dst; return false; }
    if (!oalsfx_batch_mix_gather(batch_, sample_count, src_samples, dst_samples)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

bool ApiArray::mix(int sample_count, const float* src_samples, float* dst_samples)
{
    if (!batch_) { error_ = err_not_initialized; return false; }
    if (sample_count == 0) return true;
    if (!src_samples) { error_ = err_no_src; return false; }
    if (!dst_samples) { error_ = err_no_dst; return false; }
    if (!oalsfx_batch_mix(batch_, sample_count, src_samples, dst_samples)) { error_ = oalsfx_batch_error(batch_); return false; }
    return true;
}

} // namespace oalsfxpp
