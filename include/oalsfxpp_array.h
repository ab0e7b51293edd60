// oalsfxpp::ApiArray -- many Api objects' worth of effect chains advanced together.
//
// The reference has one class, oalsfxpp::Api (src/oalsfxpp.h:760-922): one effect chain, one mix call per buffer.  A program that
// holds thousands of them -- a voice per object -- and relinks against this library gets thousands of one-instance GPU batches, one
// wavefront per launch.  ApiArray is the same surface for `count` chains at once: the setters take the instance's index in front of
// the reference's arguments (same meaning, same return values, same messages), apply_changes and mix act on all of them, and mix takes
// either one interleaved buffer pair for the whole array or one pair per instance (what the per-object code already has).  Everything
// goes through the batch C ABI (include/oalsfx_hip.h); nothing here is needed by code that keeps using Api.
#ifndef OALSFXPP_ARRAY_H
#define OALSFXPP_ARRAY_H

#include <cstdint>
#include <vector>

#include "oalsfxpp.h"

#include "oalsfx_hip.h" // oalsfx_meter, oalsfx_sampler, oalsfx_envelope, OALSFX_RESAMPLER_NONE

namespace oalsfxpp {

class ApiArray {
public:
    ApiArray();
    ApiArray(const ApiArray&) = delete;
    ApiArray& operator=(const ApiArray&) = delete;
    ~ApiArray();

    // `count` chains of one format, rate and effect count (Api::initialize's checks and messages); device: HIP ordinal
    // (-1: OALSFX_DEVICE or 0, as Api does).
    bool initialize(int count, ChannelFormat channel_format, int sampling_rate, int effect_count, int device = -1);
    bool is_initialized() const;
    void uninitialize();
    int size() const;
    int get_channel_count() const;
    int get_effect_count() const;
    const char* get_error_message() const;

    // Api's deferred setters and getters, for instance `index`.  set_effect returns false on success like the reference's
    // (src/oalsfxpp.cpp:3657); set_send_props with effect_index < 0 addresses the direct send.
    bool get_effect(int index, int effect_index, Effect& effect) const;
    bool get_deferred_effect(int index, int effect_index, Effect& effect) const;
    bool set_effect_type(int index, int effect_index, EffectType effect_type);
    bool set_effect_props(int index, int effect_index, const EffectProps& effect_props);
    bool set_effect(int index, int effect_index, const Effect& effect);
    bool set_send_props(int index, int effect_index, const SendProps& send_props);
    // ... and the same value for every instance in one call
    bool set_effect_type_all(int effect_index, EffectType effect_type);
    bool set_effect_all(int effect_index, const Effect& effect);

    bool apply_changes();          // Api::apply_changes on every instance
    bool apply_changes(int index); // ... on one
    // Api::initialize for one voice, the array's answer to reusing an Api object: Null effects, default sends, zeroed state (the other
    // instances are not touched; oalsfx_batch_reset)
    bool reset(int index);

    // Api::mix for every instance: one buffer pair per instance (sample_count * channels floats each) ...
    bool mix(int sample_count, const float* const* src_samples, float* const* dst_samples);
    // ... or the whole array in one interleaved pair, [instance][frame][channel]
    bool mix(int sample_count, const float* src_samples, float* dst_samples);

    // Buses (nothing in the reference; include/oalsfx_hip.h, "bus downmix"): instance `index` goes to bus `bus` (-1: to none) with `gain`;
    // every instance starts on bus 0 with gain 1.  mix_to_buses is mix() whose result is the buses' sums, [bus][frame][channel], in the
    // order the C header states: one interleaved source for the whole array, or one source buffer per instance.
    bool set_routing(int index, int bus, float gain);
    bool mix_to_buses(int sample_count, const float* src_samples, int bus_count, float* dst_buses);
    bool mix_to_buses(int sample_count, const float* const* src_samples, int bus_count, float* dst_buses);
    // Bus sends (include/oalsfx_hip.h, "bus sends"): instance `index` feeds up to OALSFX_BUS_SENDS buses; send 0 is set_routing's.
    // ramp_send takes the send's gain from its current value to `gain_to` over the next `frames` frames handed to mix_to_buses (0: at
    // once); get_send returns the bus, the gain the next frame gets, where a ramp leads and how many frames it still takes.
    bool set_send(int index, int send, int bus, float gain);
    bool ramp_send(int index, int send, float gain_to, uint32_t frames);
    bool get_send(int index, int send, int& bus, float& gain, float& gain_to, uint32_t& frames_left);
    // mix_to_buses plus level meters (include/oalsfx_hip.h, "level meters"): voice_meters[size()] for the instances' outputs, bus_meters
    // [bus_count] for the buses; either may be null.  A frame is quiet when every channel is within `threshold`; with `carry` the records
    // handed in are continued (quiet_run, peak_hold), otherwise they are overwritten.
    bool mix_to_buses_metered(int sample_count, const float* src_samples, int bus_count, float* dst_buses, float threshold, bool carry,
                              oalsfx_meter* voice_meters, oalsfx_meter* bus_meters);
    bool mix_to_buses_metered(int sample_count, const float* const* src_samples, int bus_count, float* dst_buses, float threshold, bool carry,
                              oalsfx_meter* voice_meters, oalsfx_meter* bus_meters);
    // Samplers (nothing in the reference's library; include/oalsfx_hip.h, "samplers"): instance `index` plays the asset its record names,
    // resident in device memory.  set_sampler holds from the next render on; get_sampler returns the record as the renders so far have
    // left it (position, and PLAYING cleared once a one-shot has finished).  play_to_buses_metered is mix_to_buses_metered without a
    // source: the samplers render the input on the device.  Either meter array may be null.
    bool set_sampler(int index, const oalsfx_sampler& sampler);
    bool get_sampler(int index, oalsfx_sampler& sampler);
    // Voice envelopes (include/oalsfx_hip.h, "voice envelopes"): the record beside instance `index`'s sampler -- a start after a delay, a
    // gain ramp, a fade that stops the voice, a pitch glide.  set_envelope holds from the next render on (set the sampler first where the
    // envelope glides); get_envelope returns the record as the renders so far have left it, and get_sampler the step, position and
    // PLAYING they have left.
    bool set_envelope(int index, const oalsfx_envelope& envelope);
    bool get_envelope(int index, oalsfx_envelope& envelope);
    // Resamplers (include/oalsfx_hip.h, "resamplers"): table `table` of the array becomes coef[1 << phase_bits][taps], 4 or 8 taps (taps 0
    // with a null coef clears it); instance `index` interpolates its asset through table `table` from the next render on, or as its
    // sampler says with OALSFX_RESAMPLER_NONE.
    bool set_fir_table(int table, int taps, int phase_bits, const float* coef);
    bool set_resampler(int index, int table);
    bool get_resampler(int index, int& table);
    bool play_to_buses_metered(int sample_count, int bus_count, float* dst_buses, float threshold, bool carry,
                               oalsfx_meter* voice_meters, oalsfx_meter* bus_meters);
    // Polyphony (include/oalsfx_hip.h, "polyphony"): every instance gets `lanes` voices, 1 to OALSFX_MAX_POLYPHONY, each a sampler, an
    // envelope and a resampler of its own, and a render sums them in ascending lanes into the instance's input.  A set-up call: it waits
    // for the renders so far.  The calls above address lane 0; these address the voice (index, lane).
    bool set_polyphony(int lanes);
    int get_polyphony() const;
    bool set_sampler(int index, int lane, const oalsfx_sampler& sampler);
    bool get_sampler(int index, int lane, oalsfx_sampler& sampler);
    bool set_envelope(int index, int lane, const oalsfx_envelope& envelope);
    bool get_envelope(int index, int lane, oalsfx_envelope& envelope);
    bool set_resampler(int index, int lane, int table);
    bool get_resampler(int index, int lane, int& table);
    // Voice filters (include/oalsfx_hip.h, "voice filters"): a biquad on the voice (index, lane) alone, in front of the sum of the
    // instance's voices.  Flags and coefficients hold from the next render on; with OALSFX_VF_LOAD the record's histories replace the
    // device's.  get_voice_filter waits for the renders so far.  The overloads without a lane address lane 0.
    bool set_voice_filter(int index, int lane, const oalsfx_voice_filter& filter);
    bool get_voice_filter(int index, int lane, oalsfx_voice_filter& filter);
    bool set_voice_filter(int index, const oalsfx_voice_filter& filter);
    bool get_voice_filter(int index, oalsfx_voice_filter& filter);
    // Voice filter sweeps (include/oalsfx_hip.h, "voice filter sweeps"): the filter of the voice (index, lane), which must be ACTIVE, ramps
    // from its current coefficients to those of `to` over `frames` frames, per frame, on the device (oalsfx_host_filter_sweep; waits for
    // the renders so far).  The current coefficients are those get_voice_filter returns, or, while a sweep is under way -- the filter
    // record then still holds what it was set with --, those of the frame the running sweep has reached, from[k] + ((float)done *
    // step[k]): a voice swept again in mid-sweep goes on from where it is.  The sweep that completes leaves `to` in the voice's filter;
    // set_voice_filter cancels a sweep under way.  get_voice_filter_sweep: the record as the renders so far leave it.
    bool sweep_voice_filter(int index, int lane, const oalsfx_voice_filter& to, uint32_t frames);
    bool sweep_voice_filter(int index, const oalsfx_voice_filter& to, uint32_t frames);
    bool get_voice_filter_sweep(int index, int lane, oalsfx_filter_sweep& sweep);
    bool get_voice_filter_sweep(int index, oalsfx_filter_sweep& sweep);
    // Filter programs (include/oalsfx_hip.h, "filter programs"): segments[0 .. count - 1], 1 to OALSFX_FILTER_PROGRAM_MAX sweeps (as
    // oalsfx_host_filter_program or oalsfx_host_filter_sweep_log make them), become the filter program of the voice (index, lane), whose
    // filter must be ACTIVE: the first the current sweep, the rest a queue the renders walk on the device, taking the next sweep at the
    // exact frame at which the current one completes.  The whole program is replaced; set_voice_filter and sweep_voice_filter empty the
    // queue.  get_voice_filter_program fills segments[0 .. count - 1] (room for OALSFX_FILTER_PROGRAM_MAX) with the current sweep and
    // what is still queued, as the renders so far have left them.
    bool program_voice_filter(int index, int lane, const oalsfx_filter_sweep* segments, int count);
    bool program_voice_filter(int index, const oalsfx_filter_sweep* segments, int count);
    bool get_voice_filter_program(int index, int lane, oalsfx_filter_sweep* segments, int& count);
    bool get_voice_filter_program(int index, oalsfx_filter_sweep* segments, int& count);
    // Envelope programs (include/oalsfx_hip.h, "envelope programs"): segments[0 .. length - 1], 1 to OALSFX_ENV_PROGRAM_MAX records, become
    // the program of the voice (index, lane): the first the current envelope, the rest a queue the renders walk on the device, taking
    // the next segment at the exact frame at which the current one completes.  The whole program is replaced, and set_envelope empties the
    // queue.  get_envelope_program fills segments[0 .. length - 1] (room for OALSFX_ENV_PROGRAM_MAX) with the current segment and
    // what is still queued, as the renders so far have left them.
    bool set_envelope_program(int index, int lane, const oalsfx_envelope* segments, int length);
    bool get_envelope_program(int index, int lane, oalsfx_envelope* segments, int& length);
    // Sampler streams (include/oalsfx_hip.h, "sampler streams"): set_stream gives the voice (index, lane) records[0 .. length - 1], 1 to
    // 1 + OALSFX_STREAM_QUEUE sampler records: the first its current record, the rest a ring the renders walk on the device, taking the
    // next record at the exact frame at which the current one-shot ends, the overshoot carried over.  The whole stream is replaced and
    // its taken count starts at 0; set_sampler empties the ring.  queue_sampler puts one more record behind those waiting ("The stream
    // queue is full." where there is no room, also by the device's own count).  stream_state waits for the renders queued and returns
    // how many records were taken since the stream was set and how many wait: record j of the stream is finished once taken > j.
    bool set_stream(int index, int lane, const oalsfx_sampler* records, int length);
    bool set_stream(int index, const oalsfx_sampler* records, int length);
    bool queue_sampler(int index, int lane, const oalsfx_sampler& record);
    bool queue_sampler(int index, const oalsfx_sampler& record);
    bool stream_state(int index, int lane, uint32_t& taken, uint32_t& queued);
    bool stream_state(int index, uint32_t& taken, uint32_t& queued);

    oalsfx_batch* batch() const; // for what the C ABI offers beyond this (device-resident buffers, pipelined host calls, read-backs)

private:
    oalsfx_batch* batch_;
    int count_, channels_, effects_;
    std::vector<float> gathered_; // mix_to_buses from one buffer per instance: the interleaved source
    mutable const char* error_;
};

} // namespace oalsfxpp

#endif // OALSFXPP_ARRAY_H
