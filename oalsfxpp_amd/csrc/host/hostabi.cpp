// Host-only entry points of the C ABI (include/oalsfx_hip.h, "host-only helpers").
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "core.hpp"
#include "oalsfx_hip.h"

using namespace oalsfx_host;
using oalsfxpp::Effect;
using oalsfxpp::EffectProps;
using oalsfxpp::ReverbPresets;

static_assert(sizeof(oalsfx_effect) == sizeof(Effect), "oalsfx_effect must mirror oalsfxpp::Effect");
static_assert(sizeof(oalsfx_send_props) == sizeof(oalsfxpp::SendProps), "oalsfx_send_props must mirror oalsfxpp::SendProps");

namespace {

struct PresetEntry { const char* name; const EffectProps::Reverb* props; };

#define OALSFX_PRESET(group, name) {#group "::" #name, &ReverbPresets::group::name},
const PresetEntry presets[] = {
#include "oalsfx_preset_names.inc"
};
#undef OALSFX_PRESET

oalsfxpp::SendProps to_send(const oalsfx_send_props& s)
{
    oalsfxpp::SendProps r;
    r.gain_ = s.gain; r.gain_hf_ = s.gain_hf; r.gain_lf_ = s.gain_lf;
    return r;
}

} // namespace

extern "C" {

void oalsfx_host_effect_defaults(int effect_type, oalsfx_effect* out)
{
    Effect e;
    std::memset(&e, 0, sizeof(e));
    e.set_type_and_defaults(static_cast<oalsfxpp::EffectType>(effect_type));
    std::memcpy(out, &e, sizeof(e));
}

void oalsfx_host_effect_normalize(oalsfx_effect* io)
{
    Effect e;
    std::memcpy(&e, io, sizeof(e));
    e.normalize();
    std::memcpy(io, &e, sizeof(e));
}

int oalsfx_host_derive_slot(int channel_format, int sampling_rate, const oalsfx_effect* normalized, oalsfx_slot_params* out)
{
    DeviceDesc dev;
    dev.init(static_cast<oalsfxpp::ChannelFormat>(channel_format), sampling_rate);
    if (dev.channels == 0) return 0;
    Effect e;
    std::memcpy(&e, normalized, sizeof(e));
    derive_slot(dev, e, *out);
    return 1;
}

int oalsfx_host_derive_source(int channel_format, int sampling_rate, int effect_count, const oalsfx_send_props* direct,
                              const oalsfx_send_props* aux, const int* slot_types, oalsfx_source_params* out)
{
    DeviceDesc dev;
    dev.init(static_cast<oalsfxpp::ChannelFormat>(channel_format), sampling_rate);
    if (dev.channels == 0 || effect_count < 1 || effect_count > OALSFX_MAX_SLOTS) return 0;
    oalsfxpp::SendProps a[OALSFX_MAX_SLOTS];
    int types[OALSFX_MAX_SLOTS] = {};
    for (int i = 0; i < effect_count; ++i) { a[i] = to_send(aux[i]); types[i] = slot_types[i]; }
    derive_source(dev, effect_count, to_send(*direct), a, types, *out);
    return 1;
}

int oalsfx_host_ring_floats(int effect_type, int sampling_rate) { return ring_floats_for(effect_type, sampling_rate); }

int oalsfx_host_channel_count(int channel_format) { return channel_count_of(static_cast<oalsfxpp::ChannelFormat>(channel_format)); }

int oalsfx_host_preset_count(void) { return static_cast<int>(sizeof(presets) / sizeof(presets[0])); }

const char* oalsfx_host_preset_name(int index)
{
    if (index < 0 || index >= oalsfx_host_preset_count()) return nullptr;
    return presets[index].name;
}

int oalsfx_host_preset(int index, void* reverb_props_out)
{
    if (index < 0 || index >= oalsfx_host_preset_count()) return 0;
    std::memcpy(reverb_props_out, presets[index].props, sizeof(EffectProps::Reverb));
    return 1;
}

// ---- voice envelopes (include/oalsfx_hip.h) ----
void oalsfx_host_envelope_ramp(const float* from, const float* to, int channels, uint32_t frames, oalsfx_envelope* inout)
{
    for (int c = 0; c < channels && c < OALSFX_MAX_CHANNELS; ++c) {
        inout->gain_from[c] = from[c];
        inout->gain_to[c] = to[c];
        inout->gain_step[c] = frames ? (to[c] - from[c]) / static_cast<float>(frames) : 0.0F;
    }
    inout->ramp_frames = frames;
    inout->ramp_done = 0;
}

void oalsfx_host_envelope_glide(uint32_t step, uint32_t step_to, uint32_t frames, oalsfx_envelope* inout)
{
    const int64_t fine = (static_cast<int64_t>(step_to) - static_cast<int64_t>(step)) * (int64_t{1} << OALSFX_ENV_SUB_BITS);
    inout->flags |= OALSFX_ENV_GLIDE;
    inout->glide_frames = frames;
    inout->glide_done = 0;
    int64_t slope = frames ? fine / static_cast<int64_t>(frames) : 0; // (truncated toward zero)
    if (slope > INT32_MAX) slope = INT32_MAX; // the steepest the record holds: the glide still ends on step_to
    if (slope < -INT32_MAX) slope = -INT32_MAX;
    inout->glide_slope = static_cast<int32_t>(slope);
    inout->step_to = step_to;
}

int oalsfx_host_envelope_check(const oalsfx_envelope* e, uint32_t sampler_step, const char** message)
{
    const char* why = nullptr;
    constexpr uint32_t kSteps = 1U << 20; // a gliding step lies below it: S_g < 2^36
    if (e->flags & ~static_cast<uint32_t>(OALSFX_ENV_ACTIVE | OALSFX_ENV_STOP | OALSFX_ENV_GLIDE)) why = "Unknown envelope flags.";
    else if (e->reserved[0] != 0 || e->reserved[1] != 0 || e->reserved[2] != 0) why = "The envelope's reserved fields are not 0.";
    else if (e->ramp_frames > (1U << 24)) why = "The envelope's ramp is longer than 2^24 frames.";
    else if (e->ramp_done > e->ramp_frames) why = "The envelope's ramp_done is beyond its ramp.";
    else if (e->sub > 0xFFFFU) why = "The envelope's sub is beyond 65535.";
    else if (e->flags & OALSFX_ENV_GLIDE) {
        // S_G, the fine step a glide from this step would end on (no overflow: the frames count only where they are at most 2^20)
        const int64_t last = (static_cast<int64_t>(sampler_step) << OALSFX_ENV_SUB_BITS) + static_cast<int64_t>(e->glide_frames & 0x1FFFFFU) * e->glide_slope;
        if (e->glide_frames > (1U << 20)) why = "The envelope's glide is longer than 2^20 frames.";
        else if (e->glide_done > e->glide_frames) why = "The envelope's glide_done is beyond its glide.";
        else if (e->step_to >= kSteps) why = "The envelope's step_to is out of range.";
        else if (sampler_step >= kSteps) why = "The gliding sampler's step is out of range.";
        else if (last < 0 || last >= (int64_t{1} << 36)) why = "The glide leaves the range of steps.";
    }
    if (message) *message = why;
    return why ? 0 : 1;
}

// ---- envelope programs (include/oalsfx_hip.h) ----
void oalsfx_host_envelope_adsr(int channels, const float* peak, const float* sustain, uint32_t attack_frames, uint32_t decay_frames, uint32_t hold_frames,
                               uint32_t release_frames, oalsfx_envelope out[4])
{
    const float silence[OALSFX_MAX_CHANNELS] = {};
    for (int k = 0; k < 4; ++k) {
        out[k] = oalsfx_envelope{};
        out[k].flags = OALSFX_ENV_ACTIVE;
    }
    oalsfx_host_envelope_ramp(silence, peak, channels, attack_frames, &out[0]);
    oalsfx_host_envelope_ramp(peak, peak, channels, hold_frames, &out[1]);
    oalsfx_host_envelope_ramp(peak, sustain, channels, decay_frames, &out[2]);
    oalsfx_host_envelope_ramp(sustain, silence, channels, release_frames, &out[3]);
    out[3].flags |= OALSFX_ENV_STOP;
}

// ---- resamplers (include/oalsfx_hip.h) ----
int oalsfx_host_fir_check(int taps, int phase_bits, const float* coef, const char** message)
{
    const char* why = nullptr;
    if (taps != 4 && taps != 8) why = "Unknown FIR tap count.";
    else if (phase_bits < 0 || phase_bits > OALSFX_SAMPLER_FRAC_BITS) why = "FIR phase bits out of range.";
    else if (!coef) why = "Null FIR coefficients.";
    else {
        const size_t count = (size_t{1} << phase_bits) * static_cast<size_t>(taps);
        for (size_t k = 0; k < count && !why; ++k)
            if (!std::isfinite(coef[k])) why = "Non-finite FIR coefficient.";
    }
    if (message) *message = why;
    return why ? 0 : 1;
}

void oalsfx_host_fir_cubic(int phase_bits, float* out)
{
    if (phase_bits < 0 || phase_bits > OALSFX_SAMPLER_FRAC_BITS || !out) return;
    const int P = 1 << phase_bits;
    for (int p = 0; p < P; ++p) {
        // (mu has at most 12 bits: every term below is exact in double)
        const double mu = static_cast<double>(p) / P, mu2 = mu * mu, mu3 = mu2 * mu;
        out[4 * p + 0] = static_cast<float>(-0.5 * mu3 + mu2 - 0.5 * mu);
        out[4 * p + 1] = static_cast<float>(1.5 * mu3 - 2.5 * mu2 + 1.0);
        out[4 * p + 2] = static_cast<float>(-1.5 * mu3 + 2.0 * mu2 + 0.5 * mu);
        out[4 * p + 3] = static_cast<float>(0.5 * mu3 - 0.5 * mu2);
    }
}

int oalsfx_host_fir_sinc(int taps, int phase_bits, double cutoff, float* out)
{
    if ((taps != 4 && taps != 8) || phase_bits < 0 || phase_bits > OALSFX_SAMPLER_FRAC_BITS || !(cutoff > 0.0 && cutoff <= 1.0) || !out) return 0;
    const double pi = 3.14159265358979323846;
    const int P = 1 << phase_bits, H = taps / 2;
    for (int p = 0; p < P; ++p) {
        double h[8];
        for (int k = 0; k < taps; ++k) {
            const double d = static_cast<double>(k - (H - 1)) - static_cast<double>(p) / P;
            const double x = pi * (cutoff * d);
            const double sinc = x == 0.0 ? 1.0 : std::sin(x) / x;
            const double w = d / H;
            h[k] = cutoff * sinc * (0.42 + 0.5 * std::cos(pi * w) + 0.08 * std::cos(2.0 * pi * w));
        }
        // (summed from the outside in, so that the phases p and P - p, whose taps mirror each other, divide by the same sum)
        double sum = 0.0;
        for (int k = 0; k < H; ++k) sum += h[k] + h[taps - 1 - k];
        for (int k = 0; k < taps; ++k) out[static_cast<size_t>(p) * taps + k] = static_cast<float>(h[k] / sum);
    }
    return 1;
}

// ---- voice filters (include/oalsfx_hip.h) ----
int oalsfx_host_voice_filter(int kind, float gain, float freq_mult, float rcp_q, oalsfx_voice_filter* inout)
{
    static const FilterKind kinds[] = {FilterKind::low_pass, FilterKind::high_pass, FilterKind::band_pass,
                                       FilterKind::low_shelf, FilterKind::high_shelf, FilterKind::peaking};
    if (kind < OALSFX_VF_LOW_PASS || kind > OALSFX_VF_PEAKING || !(gain > 0.00001F) || !(freq_mult > 0.0F && freq_mult < 0.5F) || !inout) return 0;
    oalsfx_biquad_t c;
    design_biquad(kinds[kind], gain, freq_mult, rcp_q, c);
    inout->b0 = c.b0;
    inout->b1 = c.b1;
    inout->b2 = c.b2;
    inout->a1 = c.a1;
    inout->a2 = c.a2;
    return 1;
}

float oalsfx_host_rcp_q_from_slope(float gain, float slope) { return rcp_q_from_slope(gain, slope); }
float oalsfx_host_rcp_q_from_bandwidth(float freq_mult, float bandwidth) { return rcp_q_from_bandwidth(freq_mult, bandwidth); }

int oalsfx_host_voice_filter_check(const oalsfx_voice_filter* f, const char** message)
{
    if (!f) {
        if (message) *message = "No voice filter record.";
        return 0;
    }
    const char* why = nullptr;
    uint32_t reserved1 = 0; // (the word, not the value: -0.0f is not 0)
    std::memcpy(&reserved1, &f->reserved1, sizeof(reserved1));
    if (f->flags & ~static_cast<uint32_t>(OALSFX_VF_ACTIVE | OALSFX_VF_LOAD)) why = "Unknown voice filter flags.";
    else if (f->reserved0 != 0 || reserved1 != 0) why = "The voice filter's reserved fields are not 0.";
    else if (!std::isfinite(f->b0) || !std::isfinite(f->b1) || !std::isfinite(f->b2) || !std::isfinite(f->a1) || !std::isfinite(f->a2))
        why = "Non-finite voice filter coefficient.";
    else {
        for (int c = 0; c < OALSFX_MAX_CHANNELS && !why; ++c)
            if (!std::isfinite(f->x[c][0]) || !std::isfinite(f->x[c][1]) || !std::isfinite(f->y[c][0]) || !std::isfinite(f->y[c][1]))
                why = "Non-finite voice filter history.";
    }
    if (message) *message = why;
    return why ? 0 : 1;
}

int oalsfx_host_filter_sweep(const oalsfx_voice_filter* from, const oalsfx_voice_filter* to, uint32_t frames, oalsfx_filter_sweep* out)
{
    if (!from || !to || !out || frames < 1 || frames > OALSFX_SWEEP_MAX_FRAMES) return 0;
    const float a[5] = {from->b0, from->b1, from->b2, from->a1, from->a2}, b[5] = {to->b0, to->b1, to->b2, to->a1, to->a2};
    oalsfx_filter_sweep s{};
    s.flags = OALSFX_SWEEP_ACTIVE;
    s.frames = frames;
    for (int k = 0; k < 5; ++k) {
        s.from[k] = a[k];
        s.to[k] = b[k];
        s.step[k] = (b[k] - a[k]) / static_cast<float>(frames);
    }
    *out = s;
    return 1;
}

int oalsfx_host_filter_sweep_check(const oalsfx_filter_sweep* s, const char** message)
{
    if (!s) {
        if (message) *message = "No filter sweep record.";
        return 0;
    }
    const char* why = nullptr;
    uint32_t reserved1 = 0; // (the word, not the value: -0.0f is not 0)
    std::memcpy(&reserved1, &s->reserved1, sizeof(reserved1));
    const uint32_t least = (s->flags & OALSFX_SWEEP_ACTIVE) ? 1U : 0U;
    if (s->flags & ~static_cast<uint32_t>(OALSFX_SWEEP_ACTIVE)) why = "Unknown filter sweep flags.";
    else if (s->reserved != 0 || reserved1 != 0) why = "The filter sweep's reserved fields are not 0.";
    else if (s->frames < least || s->frames > OALSFX_SWEEP_MAX_FRAMES) why = "The filter sweep's frame count is out of range.";
    else if (s->done > s->frames) why = "The filter sweep is past its end.";
    else {
        for (int k = 0; k < 5 && !why; ++k)
            if (!std::isfinite(s->from[k]) || !std::isfinite(s->step[k]) || !std::isfinite(s->to[k])) why = "Non-finite filter sweep coefficient.";
    }
    if (message) *message = why;
    return why ? 0 : 1;
}

// ---- filter programs (include/oalsfx_hip.h) ----
int oalsfx_host_stream_chunks(const oalsfx_sampler* record, uint32_t chunk_frames, int max_chunks, oalsfx_sampler* out)
{
    if (!record || !out || chunk_frames == 0 || max_chunks < 1 || record->frames == 0 || (record->flags & OALSFX_SAMPLER_LOOP)) return 0;
    if (record->format > OALSFX_PCM_F32 || record->channels == 0) return 0;
    if (record->position >= static_cast<uint64_t>(chunk_frames) << OALSFX_SAMPLER_FRAC_BITS) return 0;
    const uint64_t chunks = (static_cast<uint64_t>(record->frames) + chunk_frames - 1) / chunk_frames;
    if (chunks > static_cast<uint64_t>(max_chunks)) return 0;
    const uint64_t width = (record->format == OALSFX_PCM_F32 ? 4U : record->format == OALSFX_PCM_S16 ? 2U : 1U) * static_cast<uint64_t>(record->channels);
    for (uint64_t k = 0; k < chunks; ++k) {
        const uint64_t first = k * chunk_frames;
        oalsfx_sampler chunk = *record;
        chunk.data = record->data + first * width;
        chunk.frames = static_cast<uint32_t>(record->frames - first < chunk_frames ? record->frames - first : chunk_frames);
        chunk.position = k == 0 ? record->position : 0;
        out[k] = chunk;
    }
    return static_cast<int>(chunks);
}

int oalsfx_host_filter_program(const oalsfx_voice_filter* nodes, const uint32_t* frames, int segments, oalsfx_filter_sweep* out)
{
    if (!nodes || !frames || !out || segments < 1 || segments > OALSFX_FILTER_PROGRAM_MAX) return 0;
    for (int k = 0; k < segments; ++k)
        if (frames[k] < 1 || frames[k] > OALSFX_SWEEP_MAX_FRAMES) return 0;
    for (int k = 0; k < segments; ++k) oalsfx_host_filter_sweep(&nodes[k], &nodes[k + 1], frames[k], &out[k]);
    return 1;
}

int oalsfx_host_filter_sweep_log(int kind, float gain, float freq_mult_from, float freq_mult_to, float rcp_q, uint32_t frames, int segments,
                                 oalsfx_filter_sweep* out, float* node_freq_out)
{
    if (!out || segments < 1 || segments > OALSFX_FILTER_PROGRAM_MAX || frames < static_cast<uint32_t>(segments) || frames > OALSFX_SWEEP_MAX_FRAMES) return 0;
    if (!(freq_mult_from > 0.0F) || !(freq_mult_to > 0.0F)) return 0;
    oalsfx_voice_filter nodes[OALSFX_FILTER_PROGRAM_MAX + 1] = {};
    float freq[OALSFX_FILTER_PROGRAM_MAX + 1];
    uint32_t lengths[OALSFX_FILTER_PROGRAM_MAX];
    const double ratio = static_cast<double>(freq_mult_to) / static_cast<double>(freq_mult_from);
    for (int k = 0; k <= segments; ++k) {
        // (the ends as given: a power of 0 or 1 would be exact, but nothing is left to pow)
        freq[k] = k == 0          ? freq_mult_from
                  : k == segments ? freq_mult_to
                                  : static_cast<float>(static_cast<double>(freq_mult_from) * std::pow(ratio, static_cast<double>(k) / segments));
        if (!oalsfx_host_voice_filter(kind, gain, freq[k], rcp_q, &nodes[k])) return 0;
    }
    for (int k = 0; k < segments; ++k) lengths[k] = frames / static_cast<uint32_t>(segments) + (static_cast<uint32_t>(k) < frames % static_cast<uint32_t>(segments) ? 1U : 0U);
    if (!oalsfx_host_filter_program(nodes, lengths, segments, out)) return 0;
    if (node_freq_out)
        for (int k = 0; k <= segments; ++k) node_freq_out[k] = freq[k];
    return 1;
}

} // extern "C"
