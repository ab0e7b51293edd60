"""Python host mirror of the batch C ABI (include/oalsfx_hip.h).

`Batch` advances N independent effect chains with one call; `Api` is the one-instance view with the
method names of the reference's `oalsfxpp::Api` (reference src/oalsfxpp.h:760-922).  Both are thin:
every call goes straight to liboalsfx_hip.so, nothing is computed in Python.
"""
import ctypes as C
import operator
import weakref

import numpy as np

from . import desc, lib

_fp = C.POINTER(C.c_float)
DOWNMIX_CHUNK = 32  # OALSFX_DOWNMIX_CHUNK (include/oalsfx_hip.h): members per chunk of the bus downmix's sum
BUS_SENDS = 4  # OALSFX_BUS_SENDS: (bus, gain) pairs per instance
SEND_RAMP_MAX_FRAMES = 1 << 24  # the longest ramp of a send's gain
METER_LANES = 64    # OALSFX_METER_LANES: lanes of the meters' sum of squares
METER_CARRY = 1     # OALSFX_METER_CARRY
# one oalsfx_meter / desc.Meter record as a NumPy structured type
METER_DTYPE = np.dtype([("peak", np.float32, (desc.MAX_CHANNELS,)), ("sumsq", np.float32, (desc.MAX_CHANNELS,)), ("peak_hold", np.float32),
                        ("quiet_run", np.uint32), ("nonfinite", np.uint32), ("frames", np.uint32)])
assert METER_DTYPE.itemsize == C.sizeof(desc.Meter) == 80
# one oalsfx_sampler / desc.Sampler record as a NumPy structured type
SAMPLER_DTYPE = np.dtype([("data", np.uint64), ("position", np.uint64), ("frames", np.uint32), ("loop_start", np.uint32), ("loop_end", np.uint32),
                          ("step", np.uint32), ("format", np.uint32), ("channels", np.uint32), ("flags", np.uint32), ("reserved", np.uint32),
                          ("gain", np.float32, (desc.MAX_CHANNELS,))])
assert SAMPLER_DTYPE.itemsize == C.sizeof(desc.Sampler) == 80
SAMPLER_FRAC_BITS = desc.SAMPLER_FRAC_BITS
STREAM_QUEUE = desc.STREAM_QUEUE   # OALSFX_STREAM_QUEUE: the sampler records a voice's ring holds behind the current one
# a voice's row of the streams' ring table on the device / desc.StreamRing
STREAM_RING_DTYPE = np.dtype([("queued", np.uint32), ("reset", np.uint32), ("reserved", np.uint32, (2,)), ("entry", SAMPLER_DTYPE, (STREAM_QUEUE,))])
assert STREAM_RING_DTYPE.itemsize == C.sizeof(desc.StreamRing) == 656
# one oalsfx_envelope / desc.Envelope record as a NumPy structured type
ENVELOPE_DTYPE = np.dtype([("flags", np.uint32), ("delay", np.uint32), ("ramp_frames", np.uint32), ("ramp_done", np.uint32),
                           ("gain_from", np.float32, (desc.MAX_CHANNELS,)), ("gain_step", np.float32, (desc.MAX_CHANNELS,)),
                           ("gain_to", np.float32, (desc.MAX_CHANNELS,)), ("glide_frames", np.uint32), ("glide_done", np.uint32),
                           ("glide_slope", np.int32), ("step_to", np.uint32), ("sub", np.uint32), ("reserved", np.uint32, (3,))])
assert ENVELOPE_DTYPE.itemsize == C.sizeof(desc.Envelope) == 144
ENV_PROGRAM_MAX = 8   # OALSFX_ENV_PROGRAM_MAX: a program's segments, the current one included
# one oalsfx_voice_filter / desc.VoiceFilter record as a NumPy structured type
FILTER_DTYPE = np.dtype([("flags", np.uint32), ("reserved0", np.uint32), ("b0", np.float32), ("b1", np.float32), ("b2", np.float32), ("a1", np.float32),
                         ("a2", np.float32), ("reserved1", np.float32), ("x", np.float32, (desc.MAX_CHANNELS, 2)), ("y", np.float32, (desc.MAX_CHANNELS, 2))])
assert FILTER_DTYPE.itemsize == C.sizeof(desc.VoiceFilter) == 160
# one oalsfx_filter_sweep / desc.FilterSweep record as a NumPy structured type ("from": the C member's name, a keyword in Python)
SWEEP_DTYPE = np.dtype([("flags", np.uint32), ("frames", np.uint32), ("done", np.uint32), ("reserved", np.uint32), ("from", np.float32, (5,)),
                        ("step", np.float32, (5,)), ("to", np.float32, (5,)), ("reserved1", np.float32)])
assert SWEEP_DTYPE.itemsize == C.sizeof(desc.FilterSweep) == 80
FILTER_PROGRAM_MAX = desc.FILTER_PROGRAM_MAX   # OALSFX_FILTER_PROGRAM_MAX: a filter program's segments, the current one included
# a voice's row of the filter programs' queue table on the device / desc.FilterProgramQueue
FILTER_QUEUE_DTYPE = np.dtype([("head", np.uint32), ("count", np.uint32), ("reserved", np.uint32, (2,)), ("queue", SWEEP_DTYPE, (FILTER_PROGRAM_MAX - 1,))])
assert FILTER_QUEUE_DTYPE.itemsize == C.sizeof(desc.FilterProgramQueue) == 576
_PCM_BYTES = {desc.PCM_U8: 1, desc.PCM_S16: 2, desc.PCM_F32: 4}


FIR_TABLES = 8        # OALSFX_FIR_TABLES
RESAMPLER_NONE = -1   # OALSFX_RESAMPLER_NONE
MAX_POLYPHONY = 16    # OALSFX_MAX_POLYPHONY


class BatchError(RuntimeError):
    pass


# ---- resamplers: the host helpers (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def fir_shape(coef):
    """(taps, phase_bits) of a coefficient table [1 << phase_bits][taps], with everything refused that oalsfx_batch_set_fir_table refuses
    in a table."""
    if coef is None:
        raise BatchError("Null FIR coefficients.")
    coef = np.asarray(coef)
    if coef.ndim != 2 or coef.shape[1] not in (4, 8):
        raise BatchError("Unknown FIR tap count.")
    phases = coef.shape[0]
    if phases < 1 or phases & (phases - 1) or phases > 1 << SAMPLER_FRAC_BITS:
        raise BatchError("FIR phase bits out of range.")
    if not np.isfinite(coef).all():
        raise BatchError("Non-finite FIR coefficient.")
    return coef.shape[1], phases.bit_length() - 1


def fir_check(taps, phase_bits, coef):
    """oalsfx_host_fir_check: None, or the refusal's text.  coef: a contiguous float32 array of (1 << phase_bits) * taps values, or None."""
    message = C.c_char_p()
    if coef is not None:
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        if 0 <= phase_bits <= SAMPLER_FRAC_BITS and taps in (4, 8) and coef.size < (1 << phase_bits) * taps:
            raise BatchError(f"fir_check: {coef.size} coefficients, fewer than {1 << phase_bits} phases of {taps} taps")
    ok = lib.load().oalsfx_host_fir_check(taps, phase_bits, C.c_void_p(coef.ctypes.data if coef is not None else 0), C.byref(message))
    return None if ok else message.value.decode()


def fir_cubic(phase_bits):
    """oalsfx_host_fir_cubic: the Catmull-Rom table [1 << phase_bits][4], float32."""
    if not 0 <= operator.index(phase_bits) <= SAMPLER_FRAC_BITS:
        raise BatchError("FIR phase bits out of range.")
    out = np.empty((1 << phase_bits, 4), dtype=np.float32)
    lib.load().oalsfx_host_fir_cubic(phase_bits, C.c_void_p(out.ctypes.data))
    return out


def fir_sinc(taps, phase_bits, cutoff):
    """oalsfx_host_fir_sinc: the Blackman-windowed sinc low-pass [1 << phase_bits][taps], float32; 0 < cutoff <= 1, about 4096 / step for a
    voice pitched up."""
    if taps not in (4, 8):
        raise BatchError("Unknown FIR tap count.")
    if not 0 <= operator.index(phase_bits) <= SAMPLER_FRAC_BITS:
        raise BatchError("FIR phase bits out of range.")
    if not 0.0 < cutoff <= 1.0:
        raise BatchError("The FIR cutoff is outside (0, 1].")
    out = np.empty((1 << phase_bits, taps), dtype=np.float32)
    if not lib.load().oalsfx_host_fir_sinc(taps, phase_bits, float(cutoff), C.c_void_p(out.ctypes.data)):
        raise BatchError("oalsfx_host_fir_sinc refused its arguments.")
    return out


# ---- voice filters: the host helpers (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def voice_filter(kind, gain, freq_mult, rcp_q, record=None):
    """oalsfx_host_voice_filter: a record of FILTER_DTYPE (a copy of `record`, or an all-zero one) with the five coefficients of the
    reference's biquad of `kind` (desc.VF_LOW_PASS .. desc.VF_PEAKING) filled in."""
    out = np.zeros(1, FILTER_DTYPE) if record is None else np.array(record, dtype=FILTER_DTYPE).reshape(1)
    if not lib.load().oalsfx_host_voice_filter(operator.index(kind), float(gain), float(freq_mult), float(rcp_q), C.c_void_p(out.ctypes.data)):
        raise BatchError("oalsfx_host_voice_filter refused its arguments.")
    return out


def rcp_q_from_slope(gain, slope):
    """oalsfx_host_rcp_q_from_slope: one over Q of a shelf of linear gain `gain` and slope `slope`, in float32."""
    return np.float32(lib.load().oalsfx_host_rcp_q_from_slope(float(gain), float(slope)))


def rcp_q_from_bandwidth(freq_mult, bandwidth):
    """oalsfx_host_rcp_q_from_bandwidth: one over Q of a band `bandwidth` octaves wide at freq_mult of the sampling rate, in float32."""
    return np.float32(lib.load().oalsfx_host_rcp_q_from_bandwidth(float(freq_mult), float(bandwidth)))


def voice_filter_check(record):
    """oalsfx_host_voice_filter_check: None, or the refusal's text, for one record of FILTER_DTYPE."""
    record = np.ascontiguousarray(record, dtype=FILTER_DTYPE).reshape(1)
    message = C.c_char_p()
    ok = lib.load().oalsfx_host_voice_filter_check(C.c_void_p(record.ctypes.data), C.byref(message))
    return None if ok else message.value.decode()


# ---- voice filter sweeps: the host helpers (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def filter_sweep(from_filter, to_filter, frames):
    """oalsfx_host_filter_sweep: a record of SWEEP_DTYPE that ramps the coefficients of one record of FILTER_DTYPE to another's over
    `frames` frames: ACTIVE, done = 0, step = (to - from) / frames in float32."""
    a = np.ascontiguousarray(from_filter, dtype=FILTER_DTYPE).reshape(1)
    b = np.ascontiguousarray(to_filter, dtype=FILTER_DTYPE).reshape(1)
    out = np.zeros(1, SWEEP_DTYPE)
    frames = operator.index(frames)
    if not 0 <= frames < 2 ** 32 or not lib.load().oalsfx_host_filter_sweep(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), frames, C.c_void_p(out.ctypes.data)):
        raise BatchError("oalsfx_host_filter_sweep refused its arguments.")
    return out


def filter_sweep_check(record):
    """oalsfx_host_filter_sweep_check: None, or the refusal's text, for one record of SWEEP_DTYPE."""
    record = np.ascontiguousarray(record, dtype=SWEEP_DTYPE).reshape(1)
    message = C.c_char_p()
    ok = lib.load().oalsfx_host_filter_sweep_check(C.c_void_p(record.ctypes.data), C.byref(message))
    return None if ok else message.value.decode()


# ---- filter programs: the host helpers (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def filter_program(nodes, frames):
    """oalsfx_host_filter_program: len(frames) records of SWEEP_DTYPE through len(frames) + 1 designed records of FILTER_DTYPE: segment k
    ramps node k to node k + 1 over frames[k] frames, so that every segment starts on the bytes the one before ends on."""
    nodes = np.ascontiguousarray(nodes, dtype=FILTER_DTYPE).reshape(-1)
    lengths = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    if len(nodes) != len(lengths) + 1 or ((lengths < 0) | (lengths >= 2 ** 32)).any():
        raise BatchError("filter_program: one node more than lengths, each 1 .. 2^24")
    lengths = lengths.astype(np.uint32)
    out = np.zeros(len(lengths), SWEEP_DTYPE)
    if not lib.load().oalsfx_host_filter_program(C.c_void_p(nodes.ctypes.data), C.c_void_p(lengths.ctypes.data), len(lengths), C.c_void_p(out.ctypes.data)):
        raise BatchError("oalsfx_host_filter_program refused its arguments.")
    return out


def filter_sweep_log(kind, gain, freq_mult_from, freq_mult_to, rcp_q, frames, segments):
    """oalsfx_host_filter_sweep_log: (`segments` records of SWEEP_DTYPE, the segments + 1 node frequencies as float32): a chain of
    cookbook designs at frequencies spaced evenly in log-frequency, `frames` frames in all."""
    frames, segments = operator.index(frames), operator.index(segments)
    out, freq = np.zeros(max(segments, 1), SWEEP_DTYPE), np.zeros(max(segments, 1) + 1, np.float32)
    if not 0 <= frames < 2 ** 32 or not lib.load().oalsfx_host_filter_sweep_log(operator.index(kind), gain, freq_mult_from, freq_mult_to, rcp_q, frames, segments,
                                                                              C.c_void_p(out.ctypes.data), C.c_void_p(freq.ctypes.data)):
        raise BatchError("oalsfx_host_filter_sweep_log refused its arguments.")
    return out, freq


# ---- sampler streams: the host helper (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def stream_chunks(record, chunk_frames):
    """oalsfx_host_stream_chunks: the one-shot `record` (one record of SAMPLER_DTYPE) over a long asset as records of consecutive chunks of
    `chunk_frames` frames, the first at the record's position, the others at 0."""
    record = np.ascontiguousarray(np.asarray(record, dtype=SAMPLER_DTYPE).reshape(1))
    room = max(1, -(-int(record["frames"][0]) // max(1, int(chunk_frames))))
    out = np.zeros(room, dtype=SAMPLER_DTYPE)
    n = lib.load().oalsfx_host_stream_chunks(C.c_void_p(record.ctypes.data), int(chunk_frames) & 0xFFFFFFFF, room, C.c_void_p(out.ctypes.data)) if chunk_frames > 0 else 0
    if not n:
        raise BatchError("oalsfx_host_stream_chunks refused its arguments.")
    return out[:n]


# ---- envelope programs: the host helper (include/oalsfx_hip.h, "host-only helpers"); no device needed ----
def envelope_adsr(peak, sustain, attack_frames, decay_frames, hold_frames, release_frames):
    """oalsfx_host_envelope_adsr: four records of ENVELOPE_DTYPE -- attack, hold, decay, release (with STOP) -- for len(peak) channels.  A
    note-on is Batch.set_env_programs([adsr[:3]]), the note-off Batch.set_envelopes(adsr[3:])."""
    peak, sustain = np.ascontiguousarray(peak, dtype=np.float32).reshape(-1), np.ascontiguousarray(sustain, dtype=np.float32).reshape(-1)
    if peak.shape != sustain.shape or not 1 <= peak.shape[0] <= 8:
        raise BatchError("envelope_adsr: peak and sustain are 1 .. 8 gains each, one per channel")
    out = np.zeros(4, dtype=ENVELOPE_DTYPE)
    lib.load().oalsfx_host_envelope_adsr(peak.shape[0], peak.ctypes.data_as(_fp), sustain.ctypes.data_as(_fp), operator.index(attack_frames),
                                         operator.index(decay_frames), operator.index(hold_frames), operator.index(release_frames), C.c_void_p(out.ctypes.data))
    return out


class Batch:
    def __init__(self, n_instances, channel_format=desc.FMT_STEREO, sampling_rate=48000, effect_count=1, device_id=0):
        library = lib.load()
        h = library.oalsfx_batch_create(n_instances, channel_format, sampling_rate, effect_count, device_id)
        if not h:
            raise BatchError(library.oalsfx_last_error().decode())
        self._attach(library, h, channel_format, sampling_rate, effect_count, device_id, None)

    def _attach(self, library, handle, channel_format, sampling_rate, effect_count, device_id, owner):
        """Every attribute of a Batch, for a handle created here (owner None) or one that `owner` destroys."""
        self._lib, self._h, self._owner = library, C.c_void_p(handle), owner
        self.n = library.oalsfx_batch_instances(self._h)
        self.channel_format = channel_format
        self.rate = sampling_rate
        self.effect_count = effect_count
        self.channels = library.oalsfx_batch_channels(self._h)
        self.device_id = device_id

    @classmethod
    def _view(cls, library, handle, channel_format, sampling_rate, effect_count, device_id, owner):
        """A `Batch` over a handle that `owner` destroys (Group.batch): close() only lets go of it."""
        b = cls.__new__(cls)
        b._attach(library, handle, channel_format, sampling_rate, effect_count, device_id, owner)
        return b

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owner", None) is None:
                self._lib.oalsfx_batch_destroy(self._h)
            self._h = self._owner = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, ok):
        if not ok:
            raise BatchError(self._lib.oalsfx_batch_error(self._h).decode())

    @property
    def error(self):
        return self._lib.oalsfx_batch_error(self._h).decode()

    # ---- deferred setters (instance range [first, first+count)) ----
    def _range(self, first, count):
        return first, (self.n - first if count is None else count)

    def set_effect(self, slot, effect, first=0, count=None):
        """One `desc.Effect` broadcast to the range, or a sequence of them (one per instance)."""
        first, count = self._range(first, count)
        if isinstance(effect, desc.Effect):
            self._check(self._lib.oalsfx_batch_set_effect(self._h, first, count, slot, C.byref(effect), 0))
        else:
            arr = (desc.Effect * count)(*effect)
            self._check(self._lib.oalsfx_batch_set_effect(self._h, first, count, slot, arr, C.sizeof(desc.Effect)))

    def set_effect_at(self, slot, instances, effects):
        """`effects[k]` (or the one `desc.Effect`) for instance `instances[k]`: one foreign call for instances that are not neighbours."""
        idx = (C.c_int * len(instances))(*instances)
        if isinstance(effects, desc.Effect):
            self._check(self._lib.oalsfx_batch_set_effect_at(self._h, idx, len(instances), slot, C.byref(effects), 0))
        else:
            arr = (desc.Effect * len(instances))(*effects)
            self._check(self._lib.oalsfx_batch_set_effect_at(self._h, idx, len(instances), slot, arr, C.sizeof(desc.Effect)))

    def set_effect_type(self, slot, effect_type, first=0, count=None):
        first, count = self._range(first, count)
        self._check(self._lib.oalsfx_batch_set_effect_type(self._h, first, count, slot, effect_type))

    def set_effect_props(self, slot, props, first=0, count=None):
        """One `desc.EffectPropsU` broadcast to the range, or a sequence of them (one per instance); the deferred types stay."""
        first, count = self._range(first, count)
        if isinstance(props, desc.EffectPropsU):
            self._check(self._lib.oalsfx_batch_set_effect_props(self._h, first, count, slot, C.byref(props), 0))
        else:
            arr = (desc.EffectPropsU * count)(*props)
            self._check(self._lib.oalsfx_batch_set_effect_props(self._h, first, count, slot, arr, C.sizeof(desc.EffectPropsU)))

    def set_send_props(self, slot, gain, gain_hf, gain_lf, first=0, count=None):
        first, count = self._range(first, count)
        p = desc.SendProps(gain, gain_hf, gain_lf)
        self._check(self._lib.oalsfx_batch_set_send_props(self._h, first, count, slot, C.byref(p)))

    def get_effect(self, instance, slot, deferred=False):
        e = desc.Effect()
        self._check(self._lib.oalsfx_batch_get_effect(self._h, instance, slot, 1 if deferred else 0, C.byref(e)))
        return e

    def get_send_props(self, instance, slot, deferred=False):
        p = desc.SendProps()
        self._check(self._lib.oalsfx_batch_get_send_props(self._h, instance, slot, 1 if deferred else 0, C.byref(p)))
        return p

    def apply_changes(self, first=0, count=None):
        first, count = self._range(first, count)
        self._check(self._lib.oalsfx_batch_apply_changes(self._h, first, count))

    # ---- the hot path ----
    def mix(self, src):
        """src: float32 array [n][frames][channels] on the host; returns the same shape."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        assert src.ndim == 3 and src.shape[0] == self.n and src.shape[2] == self.channels, src.shape
        dst = np.empty_like(src)
        self._check(self._lib.oalsfx_batch_mix(self._h, src.shape[1], src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp)))
        return dst

    def mix_async(self, src, dst):
        """Queues one buffer from / to host arrays [n][frames][channels] (page-locked ones overlap with the kernels) and returns;
        both must stay untouched until wait() or until three more mix_async calls have returned."""
        assert src.dtype == np.float32 and dst.dtype == np.float32 and src.flags.c_contiguous and dst.flags.c_contiguous and src.shape == dst.shape
        assert src.ndim == 3 and src.shape[0] == self.n and src.shape[2] == self.channels, src.shape
        self._check(self._lib.oalsfx_batch_mix_async(self._h, src.shape[1], src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp)))

    def wait(self):
        self._check(self._lib.oalsfx_batch_wait(self._h))

    def pinned_array(self, frames):
        """A page-locked float32 array [n][frames][channels].  The allocation belongs to the array, not to the Batch: it is released
        (oalsfx_pinned_free) when the array and every view of it are gone, so an array may outlive close(), and a loop that asks for a
        fresh array per step holds only what it still references.  (Wait for the calls in flight -- wait() -- before dropping one.)"""
        count = self.n * frames * self.channels
        p = self._lib.oalsfx_pinned_alloc(count * 4)
        if not p:
            raise BatchError("oalsfx_pinned_alloc failed")
        buf = (C.c_float * count).from_address(p)
        # numpy keeps `buf` alive as the base of the array and of its views; the finalizer holds the library handle
        weakref.finalize(buf, self._lib.oalsfx_pinned_free, C.c_void_p(p))
        return np.frombuffer(buf, dtype=np.float32).reshape(self.n, frames, self.channels)

    def mix_device(self, frames, src_ptr, dst_ptr, stream=None):
        """Buffers already in device memory (raw addresses, e.g. torch.Tensor.data_ptr()); asynchronous."""
        self._check(self._lib.oalsfx_batch_mix_device(self._h, frames, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_void_p(stream or 0)))

    def mix_device_multi(self, frames, src_ptrs, dst_ptrs, stream=None):
        """len(src_ptrs) consecutive mix_device calls, buffer k src_ptrs[k] -> dst_ptrs[k], in as few launches as the instances allow."""
        if len(src_ptrs) != len(dst_ptrs):
            raise BatchError("mix_device_multi: as many source as destination buffers")
        s = (C.c_void_p * max(1, len(src_ptrs)))(*src_ptrs)
        d = (C.c_void_p * max(1, len(dst_ptrs)))(*dst_ptrs)
        self._check(self._lib.oalsfx_batch_mix_device_multi(self._h, frames, len(src_ptrs), s, d, C.c_void_p(stream or 0)))

    def multi_counts(self):
        """(buffers that went through multi-buffer passes, passes) of mix_device_multi so far."""
        k, p = C.c_longlong(0), C.c_longlong(0)
        self._check(self._lib.oalsfx_batch_multi_counts(self._h, C.byref(k), C.byref(p)))
        return k.value, p.value

    def join_counts(self):
        """(calls that joined a queued launch, joinable launches queued) so far."""
        j, l = C.c_longlong(0), C.c_longlong(0)
        self._check(self._lib.oalsfx_batch_join_counts(self._h, C.byref(j), C.byref(l)))
        return j.value, l.value

    def join_hold(self, k):
        """Test hook: a joinable launch is queued once it has k buffers, or when something closes it (0: off)."""
        self._lib.oalsfx_debug_join_hold(self._h, int(k))

    def synchronize(self):
        self._check(self._lib.oalsfx_batch_synchronize(self._h))

    @property
    def stream(self):
        return self._lib.oalsfx_batch_stream(self._h)

    def fill_synthetic(self, frames, buffer_index, dst_ptr, stream=None):
        self._check(self._lib.oalsfx_batch_fill_synthetic(self._h, frames, buffer_index, C.c_void_p(dst_ptr), C.c_void_p(stream or 0)))

    # ---- read-back ----
    def read_slot(self, instance, slot):
        p, s = desc.SlotParams(), desc.SlotState()
        self._check(self._lib.oalsfx_batch_read_slot(self._h, instance, slot, C.byref(p), C.byref(s)))
        return p, s

    def read_ring(self, instance, slot):
        n = self._lib.oalsfx_batch_read_ring(self._h, instance, slot, None, 0)
        out = np.zeros(n, dtype=np.float32)
        if n:
            self._lib.oalsfx_batch_read_ring(self._h, instance, slot, out.ctypes.data_as(_fp), n)
        return out

    def read_source(self, instance):
        p, s = desc.SourceParams(), desc.SourceState()
        self._check(self._lib.oalsfx_batch_read_source(self._h, instance, C.byref(p), C.byref(s)))
        return p, s

    # ---- instance state: snapshot, restore, reset (include/oalsfx_hip.h) ----
    def _instances(self, instances):
        """(ctypes int array or None, count) for a list of batch-local instance numbers; None: every instance."""
        if instances is None:
            return None, self.n
        try:
            idx = [operator.index(i) for i in instances]
        except TypeError:
            raise BatchError("Instances must be a sequence of integers.") from None
        bad = [i for i in idx if i < 0 or i >= self.n]
        if bad:
            raise BatchError(f"Instance range is out of bounds: {bad[:4]}")
        return (C.c_int * max(1, len(idx)))(*idx), len(idx)

    @staticmethod
    def _blob(ptr, nbytes):
        if not ptr:
            raise BatchError("No snapshot buffer.")
        if ptr % 16:
            raise BatchError("The snapshot buffer is not 16-byte aligned.")
        if operator.index(nbytes) < 0:
            raise BatchError("Snapshot bytes are negative.")

    def snapshot_bytes(self, instances=None):
        """Bytes a snapshot of `instances` (None: all) takes with the slot types they hold now."""
        idx, count = self._instances(instances)
        nbytes = self._lib.oalsfx_batch_snapshot_bytes(self._h, idx, count)
        self._check(nbytes != 0)
        return nbytes

    def snapshot(self, instances, dst_ptr, nbytes):
        """The complete state of `instances` (None: all) into device or page-locked memory at `dst_ptr` (e.g. a torch uint8 tensor's
        data_ptr()); asynchronous on the batch's stream: complete once synchronize() returns."""
        idx, count = self._instances(instances)
        self._blob(dst_ptr, nbytes)
        self._check(self._lib.oalsfx_batch_snapshot(self._h, idx, count, C.c_void_p(dst_ptr), nbytes))

    def restore(self, instances, src_ptr, nbytes):
        """Snapshot entry k into instance instances[k] (None: 0 .. count - 1)."""
        idx, count = self._instances(instances)
        if instances is not None and len(set(idx[:count])) != count:
            raise BatchError("An instance is listed twice as a restore target.")
        self._blob(src_ptr, nbytes)
        self._check(self._lib.oalsfx_batch_restore(self._h, idx, count, C.c_void_p(src_ptr), nbytes))

    def reset(self, instances=None):
        """Api::initialize for `instances` (None: all) only: Null effects, default sends, zeroed state."""
        idx, count = self._instances(instances)
        self._check(self._lib.oalsfx_batch_reset(self._h, idx, count))

    # ---- bus downmix (include/oalsfx_hip.h, "bus downmix") ----
    @staticmethod
    def _routing(n, first, bus, gain):
        """(count, ctypes int array or None, ctypes float array or None) for per-instance routing arrays from `first` on."""
        if bus is None and gain is None:
            raise BatchError("set_routing: give buses, gains or both.")
        try:
            buses = None if bus is None else [operator.index(v) for v in bus]
            gains = None if gain is None else [float(v) for v in gain]
        except TypeError:
            raise BatchError("Routing takes a sequence of bus numbers and a sequence of gains.") from None
        if buses is not None and gains is not None and len(buses) != len(gains):
            raise BatchError(f"set_routing: {len(buses)} buses but {len(gains)} gains")
        count = len(buses if buses is not None else gains)
        if first < 0 or first + count > n:
            raise BatchError("Instance range is out of bounds.")
        if buses is not None and any(v < -1 for v in buses):
            raise BatchError("Bus number is out of range.")
        return (count, None if buses is None else (C.c_int * max(1, count))(*buses),
                None if gains is None else (C.c_float * max(1, count))(*gains))

    @staticmethod
    def _send(send):
        send = operator.index(send)
        if not 0 <= send < BUS_SENDS:
            raise BatchError("Send out of range.")
        return send

    def set_routing(self, bus=None, gain=None, first=0, send=0):
        """bus[k], gain[k] for send `send` of instance first + k (-1: routed nowhere); None leaves the buses, or the gains, as they are.  A
        gain cancels the send's ramp; a new bus alone keeps it running."""
        send = self._send(send)
        count, buses, gains = self._routing(self.n, first, bus, gain)
        if send == 0:
            self._check(self._lib.oalsfx_batch_set_routing(self._h, first, count, buses, gains))
        else:
            self._check(self._lib.oalsfx_batch_set_send_routing(self._h, send, first, count, buses, gains))

    def get_routing(self, instance, send=0):
        """(bus, gain) of send `send`: the gain the next downmixed frame gets."""
        return self.get_send(instance, send)[:2]

    def get_send(self, instance, send=0):
        """(bus, gain, gain_to, frames_left) of send `send`; without a ramp gain_to == gain and frames_left == 0."""
        send = self._send(send)
        if not 0 <= operator.index(instance) < self.n:
            raise BatchError("Instance range is out of bounds.")
        bus, gain, gain_to, left = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_uint32(0)
        self._check(self._lib.oalsfx_batch_get_send_routing(self._h, instance, send, C.byref(bus), C.byref(gain), C.byref(gain_to), C.byref(left)))
        return bus.value, gain.value, gain_to.value, left.value

    def set_send_ramps(self, gain_to, frames, first=0, send=0):
        """Send `send` of instance first + k ramps from its current gain to gain_to[k] over the next `frames` downmixed frames (0: at
        once); every downmix call advances every ramp of the batch by its frames."""
        send = self._send(send)
        try:
            targets = [float(v) for v in gain_to]
        except TypeError:
            raise BatchError("A ramp takes a sequence of gains.") from None
        if first < 0 or first + len(targets) > self.n:
            raise BatchError("Instance range is out of bounds.")
        if not 0 <= operator.index(frames) <= SEND_RAMP_MAX_FRAMES:
            raise BatchError("Ramp length out of range.")
        count = len(targets)
        self._check(self._lib.oalsfx_batch_set_send_ramps(self._h, send, first, count, (C.c_float * max(1, count))(*targets), frames))

    @staticmethod
    def _downmix_counts(frames, n_buses):
        if operator.index(frames) < 0:
            raise BatchError("Frame count is negative.")
        if operator.index(n_buses) < 1:
            raise BatchError("Bus count is out of range.")

    def downmix_device(self, frames, src_ptr, n_buses, dst_ptr, stream=None):
        """Device buffers (raw addresses): src [n][frames][channels] summed into dst [n_buses][frames][channels]; asynchronous."""
        self._downmix_counts(frames, n_buses)
        self._check(self._lib.oalsfx_batch_downmix_device(self._h, frames, C.c_void_p(src_ptr), n_buses, C.c_void_p(dst_ptr), C.c_void_p(stream or 0)))

    def mix_downmix(self, src, n_buses, dst=None):
        """mix() whose result is the buses: src float32 [n][frames][channels] on the host; returns [n_buses][frames][channels]."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        if src.ndim != 3 or src.shape[0] != self.n or src.shape[2] != self.channels:
            raise BatchError(f"mix_downmix: the source is {src.shape}, not [{self.n}][frames][{self.channels}]")
        self._downmix_counts(src.shape[1], n_buses)
        if dst is None:
            dst = np.empty((n_buses, src.shape[1], self.channels), dtype=np.float32)
        elif dst.dtype != np.float32 or not dst.flags.c_contiguous or dst.shape != (n_buses, src.shape[1], self.channels):
            raise BatchError(f"mix_downmix: the bus array is {dst.shape}, not [{n_buses}][{src.shape[1]}][{self.channels}] float32")
        self._check(self._lib.oalsfx_batch_mix_downmix(self._h, src.shape[1], src.ctypes.data_as(_fp), n_buses, dst.ctypes.data_as(_fp)))
        return dst

    def downmix_uploads(self):
        """How often the routing table went to the device so far."""
        return self._lib.oalsfx_debug_downmix_uploads(self._h)

    # ---- level meters (include/oalsfx_hip.h, "level meters") ----
    @staticmethod
    def _meter_args(frames, threshold, carry):
        """The flags word for checked arguments."""
        if operator.index(frames) < 0:
            raise BatchError("Frame count is negative.")
        try:
            threshold = float(threshold)
        except (TypeError, ValueError):
            raise BatchError("The meter threshold is negative or not a number.") from None
        if not threshold >= 0.0:
            raise BatchError("The meter threshold is negative or not a number.")
        if isinstance(carry, bool):
            return METER_CARRY if carry else 0
        flags = operator.index(carry)
        if flags & ~METER_CARRY:
            raise BatchError("Unknown meter flags.")
        return flags

    @staticmethod
    def _meter_array(meters, count, what):
        """`meters` checked as `count` records of METER_DTYPE (None: a fresh zeroed array)."""
        if meters is None:
            return np.zeros(count, dtype=METER_DTYPE)
        if not isinstance(meters, np.ndarray) or meters.dtype != METER_DTYPE or meters.shape != (count,) or not meters.flags.c_contiguous:
            raise BatchError(f"{what}: the meter array is not {count} contiguous records of METER_DTYPE")
        return meters

    def meter_device(self, rows, frames, src_ptr, meters_ptr, threshold, carry=False, stream=None):
        """Device buffer (raw address) src [rows][frames][channels] metered into `rows` records at meters_ptr (device or page-locked
        memory, 16-byte aligned); asynchronous.  carry: the records there are continued (quiet_run, peak_hold)."""
        if operator.index(rows) < 1:
            raise BatchError("Row count is out of range.")
        flags = self._meter_args(frames, threshold, carry)
        if frames and not src_ptr:
            raise BatchError("No source samples.")
        if frames and not meters_ptr:
            raise BatchError("No meter records.")
        if src_ptr % 4:
            raise BatchError("The meter source is not 4-byte aligned.")
        if meters_ptr % 16:
            raise BatchError("The meter records are not 16-byte aligned.")
        self._check(self._lib.oalsfx_batch_meter_device(self._h, rows, frames, C.c_void_p(src_ptr), threshold, flags, C.c_void_p(meters_ptr),
                                                        C.c_void_p(stream or 0)))

    def mix_downmix_meter(self, src, n_buses, threshold, carry=False, voice_meters=None, bus_meters=None, dst=None, voices=True, buses=True):
        """mix_downmix() plus meters: returns (buses, voice records or None, bus records or None), the records as arrays of METER_DTYPE.
        voices / buses False skips that meter.  With carry the arrays given as voice_meters / bus_meters are continued and filled in
        place (zero-filled ones start a run); without it they are only a place to write to."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        if src.ndim != 3 or src.shape[0] != self.n or src.shape[2] != self.channels:
            raise BatchError(f"mix_downmix_meter: the source is {src.shape}, not [{self.n}][frames][{self.channels}]")
        self._downmix_counts(src.shape[1], n_buses)
        flags = self._meter_args(src.shape[1], threshold, carry)
        if dst is None:
            dst = np.empty((n_buses, src.shape[1], self.channels), dtype=np.float32)
        elif dst.dtype != np.float32 or not dst.flags.c_contiguous or dst.shape != (n_buses, src.shape[1], self.channels):
            raise BatchError(f"mix_downmix_meter: the bus array is {dst.shape}, not [{n_buses}][{src.shape[1]}][{self.channels}] float32")
        vm = self._meter_array(voice_meters, self.n, "mix_downmix_meter") if voices else None
        bm = self._meter_array(bus_meters, n_buses, "mix_downmix_meter") if buses else None
        self._check(self._lib.oalsfx_batch_mix_downmix_meter(
            self._h, src.shape[1], src.ctypes.data_as(_fp), n_buses, dst.ctypes.data_as(_fp), threshold, flags,
            C.c_void_p(vm.ctypes.data if vm is not None else 0), C.c_void_p(bm.ctypes.data if bm is not None else 0)))
        return dst, vm, bm

    # ---- the per-voice records (samplers, envelopes, voice filters): what their set and get methods share ----
    @staticmethod
    def _records(values, count, what, dtype, cls, texts):
        """`values` (an array of `dtype`, one `cls` object or a sequence of them) as `count` contiguous records of `dtype`.  texts: what
        method `what` says of values that are no records, of an array that is not contiguous records, and of a wrong count ({} and {}:
        instances and records)."""
        no_records, no_array, wrong_count = texts
        if isinstance(values, cls):
            values = [values]
        if not isinstance(values, np.ndarray):
            try:
                values = np.frombuffer(b"".join(bytes(v) for v in values), dtype=dtype)
            except (TypeError, ValueError):
                raise BatchError(f"{what}: {no_records}") from None
        if values.dtype != dtype or values.ndim != 1 or not values.flags.c_contiguous:
            raise BatchError(f"{what}: {no_array}")
        if values.shape[0] != count:
            raise BatchError(f"{what}: " + wrong_count.format(count, values.shape[0]))
        return values

    @staticmethod
    def _refuse(checks):
        """Raises the message of the first (bad, message) whose `bad` holds for any record."""
        for bad, message in checks:
            if bad.any():
                raise BatchError(message)

    def _targets(self, values, cls, instances, twice):
        """(ctypes int array or None, count): the voices a set call gives `values` to -- `instances`, none of them twice (`twice`: the
        call's text for one that is), or with None the first len(values) (one for a single `cls` object)."""
        if instances is None:
            count = 1 if cls is not None and isinstance(values, cls) else len(values)
            if count > self.n:
                raise BatchError("Instance range is out of bounds.")
            return None, count
        idx, count = self._instances(instances)
        if len(set(idx[:count])) != count:
            raise BatchError(twice)
        return idx, count

    def _set_records(self, call, lane, idx, count, records):
        """The library's `call` (its name: nothing is asked of the library before the arguments are in order) on `count` records."""
        self._check(getattr(self._lib, call)(self._h, operator.index(lane), idx, count, C.c_void_p(records.ctypes.data if count else 0)))

    def _get_records(self, call, dtype, instances, lane):
        idx, count = self._instances(instances)
        out = np.zeros(count, dtype=dtype)
        self._set_records(call, lane, idx, count, out)
        return out

    # ---- samplers (include/oalsfx_hip.h, "samplers") ----
    def _sampler_records(self, samplers, count, what):
        """`samplers` as `count` contiguous records of SAMPLER_DTYPE, with everything refused that can be seen without the device."""
        samplers = self._records(samplers, count, what, SAMPLER_DTYPE, desc.Sampler, (
            "samplers are an array of SAMPLER_DTYPE or a sequence of desc.Sampler", "the sampler array is not contiguous records of SAMPLER_DTYPE",
            "{} instances but {} samplers"))
        r, frac = samplers, np.uint64(SAMPLER_FRAC_BITS)
        known = np.isin(r["format"], list(_PCM_BYTES))
        width = np.where(r["format"] == desc.PCM_F32, 4, np.where(r["format"] == desc.PCM_S16, 2, 1)).astype(np.uint64)
        play = (r["flags"] & desc.SAMPLER_PLAYING) != 0
        loop = play & ((r["flags"] & desc.SAMPLER_LOOP) != 0)
        end = np.where(loop, r["loop_end"], r["frames"]).astype(np.uint64) << frac
        self._refuse((
                ((r["flags"] & ~np.uint32(desc.SAMPLER_PLAYING | desc.SAMPLER_LOOP | desc.SAMPLER_LINEAR)) != 0, "Unknown sampler flags."),
                (~known, "Unknown sampler format."),
                (r["reserved"] != 0, "The sampler's reserved field is not 0."),
                ((r["channels"] != 1) & (r["channels"] != self.channels), "The sampler's channel count is neither 1 nor the batch's."),
                (play & (r["data"] == 0), "A playing sampler has no data."),
                (play & ((r["frames"] == 0) | (r["frames"] >= 2 ** 31)), "The sampler's frame count is out of range."),
                (play & (r["data"] % width != 0), "The sampler's data is not aligned to its element size."),
                (loop & ((r["loop_start"] >= r["loop_end"]) | (r["loop_end"] > r["frames"])), "The sampler's loop region is out of range."),
                (play & (r["position"] >= end), "The sampler's position is past its end.")))
        return samplers

    def set_samplers(self, samplers, instances=None, lane=0):
        """samplers[k] (an array of SAMPLER_DTYPE, or desc.Sampler objects) becomes the record of instances[k] (None: 0 .. count - 1) in
        lane `lane`; it holds from the next render on.  The library checks in addition that every playing asset lies inside one device
        allocation."""
        idx, count = self._targets(samplers, desc.Sampler, instances, "An instance is listed twice as a sampler target.")
        records = self._sampler_records(samplers, count, "set_samplers")
        self._set_records("oalsfx_batch_set_lane_samplers", lane, idx, count, records)

    def get_samplers(self, instances=None, lane=0):
        """The records of `instances` (None: all) in lane `lane` as every render queued so far leaves them, as an array of SAMPLER_DTYPE;
        waits."""
        return self._get_records("oalsfx_batch_get_lane_samplers", SAMPLER_DTYPE, instances, lane)

    # ---- sampler streams (include/oalsfx_hip.h, "sampler streams") ----
    def _stream_records(self, streams, count, room, what, shortest):
        """(lengths, records [count][room]) for a stream call: streams[k] is `shortest` .. `room` sampler records."""
        streams = list(streams)
        if len(streams) != count:
            raise BatchError(f"{what}: {count} instances but {len(streams)} streams")
        lengths = (C.c_int * max(count, 1))()
        records = np.zeros((count, room), dtype=SAMPLER_DTYPE)
        for k, stream in enumerate(streams):
            length = 1 if isinstance(stream, desc.Sampler) else len(stream)
            if not shortest <= length <= room:
                raise BatchError("Stream length out of range.")
            lengths[k] = length
            if length:
                records[k, :length] = self._sampler_records(stream, length, what)
        return lengths, records

    def set_streams(self, streams, instances=None, lane=0):
        """streams[k], 1 .. 1 + STREAM_QUEUE sampler records (an array of SAMPLER_DTYPE, or desc.Sampler objects), becomes the stream of
        instances[k] (None: 0 .. count - 1) in lane `lane`: its first record the current sampler record, the rest the voice's ring, which
        the renders walk on the device.  The whole stream is replaced and its taken count starts at 0."""
        streams = list(streams)
        idx, count = self._targets(streams, None, instances, "An instance is listed twice as a stream target.")
        lengths, records = self._stream_records(streams, count, 1 + STREAM_QUEUE, "set_streams", 1)
        self._check(self._lib.oalsfx_batch_set_lane_streams(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(records.ctypes.data if count else 0)))

    def append_streams(self, streams, instances=None, lane=0):
        """streams[k], 0 .. STREAM_QUEUE sampler records, are put behind the entries the ring of instances[k] holds, all or none: "The
        stream queue is full." where a ring has too little room also by the device's own count, which the call then waits for."""
        streams = list(streams)
        idx, count = self._targets(streams, None, instances, "An instance is listed twice as a stream target.")
        lengths, records = self._stream_records(streams, count, STREAM_QUEUE, "append_streams", 0)
        self._check(self._lib.oalsfx_batch_append_lane_streams(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(records.ctypes.data if count else 0)))

    def get_streams(self, instances=None, lane=0):
        """The streams of `instances` (None: all) in lane `lane` as every render queued so far leaves them: a list of arrays of
        SAMPLER_DTYPE, the current record first, then the entries still waiting; waits."""
        idx, count = self._instances(instances)
        lengths = (C.c_int * max(count, 1))()
        out = np.zeros((count, 1 + STREAM_QUEUE), dtype=SAMPLER_DTYPE)
        self._check(self._lib.oalsfx_batch_get_lane_streams(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(out.ctypes.data if count else 0)))
        return [out[k, :lengths[k]].copy() for k in range(count)]

    def get_stream_state(self, instances=None, lane=0):
        """(taken, queued), two uint32 arrays: the entries taken since each voice's stream was last set, and those waiting in its ring, as
        every render queued so far leaves them; waits.  Also tells the batch which rings are empty."""
        idx, count = self._instances(instances)
        taken, queued = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
        self._check(self._lib.oalsfx_batch_get_lane_stream_state(self._h, operator.index(lane), idx, count, C.c_void_p(taken.ctypes.data if count else 0),
                                                                 C.c_void_p(queued.ctypes.data if count else 0)))
        return taken, queued

    def sample_device(self, frames, dst_ptr, stream=None):
        """Renders every instance's sampler into the device buffer (raw address) dst [n][frames][channels] and advances the records;
        asynchronous."""
        if operator.index(frames) < 0:
            raise BatchError("Frame count is negative.")
        if frames * self.channels > 0xFFFFFFFF:
            raise BatchError("Frame count is out of range.")
        if frames and not dst_ptr:
            raise BatchError("No destination samples.")
        if dst_ptr % 4:
            raise BatchError("The sampler destination is not 4-byte aligned.")
        self._check(self._lib.oalsfx_batch_sample_device(self._h, frames, C.c_void_p(dst_ptr), C.c_void_p(stream or 0)))

    def play_downmix_meter(self, frames, n_buses, threshold, carry=False, voice_meters=None, bus_meters=None, dst=None, voices=True, buses=True):
        """mix_downmix_meter() whose input the samplers render on the device: returns (buses, voice records or None, bus records or None)."""
        self._downmix_counts(frames, n_buses)
        flags = self._meter_args(frames, threshold, carry)
        if dst is None:
            dst = np.empty((n_buses, frames, self.channels), dtype=np.float32)
        elif dst.dtype != np.float32 or not dst.flags.c_contiguous or dst.shape != (n_buses, frames, self.channels):
            raise BatchError(f"play_downmix_meter: the bus array is {dst.shape}, not [{n_buses}][{frames}][{self.channels}] float32")
        vm = self._meter_array(voice_meters, self.n, "play_downmix_meter") if voices else None
        bm = self._meter_array(bus_meters, n_buses, "play_downmix_meter") if buses else None
        self._check(self._lib.oalsfx_batch_play_downmix_meter(
            self._h, frames, n_buses, dst.ctypes.data_as(_fp), threshold, flags,
            C.c_void_p(vm.ctypes.data if vm is not None else 0), C.c_void_p(bm.ctypes.data if bm is not None else 0)))
        return dst, vm, bm

    # ---- voice envelopes (include/oalsfx_hip.h, "voice envelopes") ----
    def _envelope_records(self, envelopes, count, what):
        """`envelopes` as `count` contiguous records of ENVELOPE_DTYPE, with everything refused that does not depend on the sampler."""
        r = envelopes = self._records(envelopes, count, what, ENVELOPE_DTYPE, desc.Envelope, (
            "envelopes are an array of ENVELOPE_DTYPE or a sequence of desc.Envelope", "the envelope array is not contiguous records of ENVELOPE_DTYPE",
            "{} instances but {} envelopes"))
        glide = (r["flags"] & desc.ENV_GLIDE) != 0
        self._refuse((
                ((r["flags"] & ~np.uint32(desc.ENV_ACTIVE | desc.ENV_STOP | desc.ENV_GLIDE)) != 0, "Unknown envelope flags."),
                ((r["reserved"] != 0).any(axis=1), "The envelope's reserved fields are not 0."),
                (r["ramp_frames"] > 2 ** 24, "The envelope's ramp is longer than 2^24 frames."),
                (r["ramp_done"] > r["ramp_frames"], "The envelope's ramp_done is beyond its ramp."),
                (r["sub"] > 0xFFFF, "The envelope's sub is beyond 65535."),
                (glide & (r["glide_frames"] > 2 ** 20), "The envelope's glide is longer than 2^20 frames."),
                (glide & (r["glide_done"] > r["glide_frames"]), "The envelope's glide_done is beyond its glide."),
                (glide & (r["step_to"] >= 2 ** 20), "The envelope's step_to is out of range.")))
        return envelopes

    def set_envelopes(self, envelopes, instances=None, lane=0):
        """envelopes[k] (an array of ENVELOPE_DTYPE, or desc.Envelope objects) becomes the envelope of instances[k] (None: 0 .. count - 1)
        in lane `lane`; it holds from the next render on.  The library checks a glide against the step of the voice's sampler in
        addition."""
        idx, count = self._targets(envelopes, desc.Envelope, instances, "An instance is listed twice as an envelope target.")
        records = self._envelope_records(envelopes, count, "set_envelopes")
        self._set_records("oalsfx_batch_set_lane_envelopes", lane, idx, count, records)

    def get_envelopes(self, instances=None, lane=0):
        """The envelopes of `instances` (None: all) in lane `lane` as every render queued so far leaves them, as an array of
        ENVELOPE_DTYPE; waits."""
        return self._get_records("oalsfx_batch_get_lane_envelopes", ENVELOPE_DTYPE, instances, lane)

    def envelope_uploads(self):
        """How many renders put changed envelopes on the device first so far."""
        return self._lib.oalsfx_debug_envelope_uploads(self._h)

    # ---- envelope programs (include/oalsfx_hip.h, "envelope programs") ----
    def set_env_programs(self, programs, instances=None, lane=0):
        """programs[k], 1 .. ENV_PROGRAM_MAX envelope records (an array of ENVELOPE_DTYPE, or desc.Envelope objects), becomes the program
        of instances[k] (None: 0 .. count - 1) in lane `lane`: its first segment the current envelope, the rest the voice's queue, which
        the renders walk on the device.  `programs` may be one array [count][length] where all have the same length.  The whole program
        is replaced; it holds from the next render on.  What a program of two or more must be beyond a valid record (ACTIVE, no GLIDE) is
        the library's to refuse."""
        same_length = isinstance(programs, np.ndarray) and programs.ndim == 2
        if not same_length:
            programs = list(programs)
        idx, count = self._targets(programs, None, instances, "An instance is listed twice as an envelope target.")
        if len(programs) != count:
            raise BatchError(f"set_env_programs: {count} instances but {len(programs)} programs")
        lengths = (C.c_int * max(count, 1))()
        segments = np.zeros((count, ENV_PROGRAM_MAX), dtype=ENVELOPE_DTYPE)
        if same_length:
            length = programs.shape[1]
            if not 1 <= length <= ENV_PROGRAM_MAX:
                raise BatchError("Envelope program length out of range.")
            segments[:, :length] = self._envelope_records(np.ascontiguousarray(programs).reshape(-1), count * length, "set_env_programs").reshape(count, length)
            lengths[:count] = [length] * count
        else:
            for k, program in enumerate(programs):
                length = 1 if isinstance(program, desc.Envelope) else len(program)
                if not 1 <= length <= ENV_PROGRAM_MAX:
                    raise BatchError("Envelope program length out of range.")
                lengths[k] = length
                segments[k, :length] = self._envelope_records(program, length, "set_env_programs")
        self._check(self._lib.oalsfx_batch_set_lane_env_programs(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(segments.ctypes.data if count else 0)))

    def get_env_programs(self, instances=None, lane=0):
        """The programs of `instances` (None: all) in lane `lane` as every render queued so far leaves them: a list of arrays of
        ENVELOPE_DTYPE, the current segment first, then the segments still queued; waits."""
        idx, count = self._instances(instances)
        lengths = (C.c_int * max(count, 1))()
        out = np.zeros((count, ENV_PROGRAM_MAX), dtype=ENVELOPE_DTYPE)
        self._check(self._lib.oalsfx_batch_get_lane_env_programs(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(out.ctypes.data if count else 0)))
        return [out[k, :lengths[k]].copy() for k in range(count)]

    def program_uploads(self):
        """How many renders put changed queues on the device first so far."""
        return self._lib.oalsfx_debug_program_uploads(self._h)

    # ---- resamplers (include/oalsfx_hip.h, "resamplers") ----
    def set_fir_table(self, table, coef):
        """Table `table` becomes `coef`, a float32 array [1 << phase_bits][taps] with 4 or 8 taps (None clears the slot).  A set-up call:
        it waits for the renders queued so far."""
        table = operator.index(table)
        if not 0 <= table < FIR_TABLES:
            raise BatchError("FIR table index out of range.")
        if coef is None:
            self._check(self._lib.oalsfx_batch_set_fir_table(self._h, table, 0, 0, C.c_void_p(0)))
            return
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        taps, phase_bits = fir_shape(coef)
        self._check(self._lib.oalsfx_batch_set_fir_table(self._h, table, taps, phase_bits, C.c_void_p(coef.ctypes.data)))

    def get_fir_table(self, table):
        """(taps, phase_bits) of table `table`; (0, 0) for an empty slot."""
        taps, bits = C.c_int(0), C.c_int(0)
        self._check(self._lib.oalsfx_batch_get_fir_table(self._h, operator.index(table), C.byref(taps), C.byref(bits)))
        return taps.value, bits.value

    def set_resamplers(self, tables, instances=None, lane=0):
        """tables[k] (a table index, or RESAMPLER_NONE) becomes the resampler of instances[k] (None: 0 .. count - 1) in lane `lane`; it
        holds from the next render on."""
        tables = np.ascontiguousarray(tables, dtype=np.int64).reshape(-1)
        idx, count = self._targets(tables, None, instances, "An instance is listed twice as a resampler target.")
        if len(tables) != count:
            raise BatchError(f"set_resamplers: {count} instances but {len(tables)} resamplers")
        if ((tables < RESAMPLER_NONE) | (tables >= FIR_TABLES)).any():
            raise BatchError("Unknown resampler.")
        t = (C.c_int * max(count, 1))(*[int(x) for x in tables])
        self._check(self._lib.oalsfx_batch_set_lane_resamplers(self._h, operator.index(lane), idx, count, t))

    def get_resamplers(self, instances=None, lane=0):
        """The resamplers of `instances` (None: all) in lane `lane` as an int32 array: table indices, RESAMPLER_NONE where there is none."""
        idx, count = self._instances(instances)
        t = (C.c_int * max(count, 1))()
        self._check(self._lib.oalsfx_batch_get_lane_resamplers(self._h, operator.index(lane), idx, count, t))
        return np.asarray(t[:count], dtype=np.int32)

    def resampler_uploads(self):
        """How many renders put changed resamplers on the device first so far."""
        return self._lib.oalsfx_debug_resampler_uploads(self._h)

    # ---- polyphony (include/oalsfx_hip.h, "polyphony") ----
    def set_polyphony(self, lanes):
        """Every instance gets `lanes` voices (1 .. MAX_POLYPHONY), which a render sums in ascending lanes; the record methods' `lane`
        keyword addresses them.  A set-up call: it waits for the renders queued so far.  Kept lanes keep their records."""
        lanes = operator.index(lanes)
        if not 1 <= lanes <= MAX_POLYPHONY:
            raise BatchError("Polyphony out of range.")
        self._check(self._lib.oalsfx_batch_set_polyphony(self._h, lanes))

    @property
    def polyphony(self):
        """How many lanes (voices per instance) the batch has."""
        return self._lib.oalsfx_batch_get_polyphony(self._h)

    # ---- voice filters (include/oalsfx_hip.h, "voice filters") ----
    def _filter_records(self, filters, count, what):
        """`filters` as `count` contiguous records of FILTER_DTYPE, with everything refused that the library refuses in a record."""
        r = filters = self._records(filters, count, what, FILTER_DTYPE, desc.VoiceFilter, (
            "filters are an array of FILTER_DTYPE or a sequence of desc.VoiceFilter", "the filter array is not contiguous records of FILTER_DTYPE",
            "{} instances but {} filters"))
        coefficients = np.stack([r[k] for k in ("b0", "b1", "b2", "a1", "a2")])
        self._refuse((
                ((r["flags"] & ~np.uint32(desc.VF_ACTIVE | desc.VF_LOAD)) != 0, "Unknown voice filter flags."),
                ((r["reserved0"] != 0) | (r["reserved1"].view(np.uint32) != 0), "The voice filter's reserved fields are not 0."),
                (~np.isfinite(coefficients), "Non-finite voice filter coefficient."),
                (~np.isfinite(r["x"]) | ~np.isfinite(r["y"]), "Non-finite voice filter history.")))
        return filters

    def set_filters(self, filters, instances=None, lane=0):
        """filters[k] (an array of FILTER_DTYPE, or desc.VoiceFilter objects) becomes the filter of instances[k] (None: 0 .. count - 1) in
        lane `lane`; flags and coefficients hold from the next render on, and with desc.VF_LOAD the record's histories replace the
        device's in front of it."""
        idx, count = self._targets(filters, desc.VoiceFilter, instances, "An instance is listed twice as a voice filter target.")
        records = self._filter_records(filters, count, "set_filters")
        self._set_records("oalsfx_batch_set_lane_filters", lane, idx, count, records)

    def get_filters(self, instances=None, lane=0):
        """The filters of `instances` (None: all) in lane `lane`, as an array of FILTER_DTYPE: the coefficients as set, the histories as
        every render queued so far leaves them; waits."""
        return self._get_records("oalsfx_batch_get_lane_filters", FILTER_DTYPE, instances, lane)

    def filter_uploads(self):
        """How many renders put changed voice filters on the device first so far."""
        return self._lib.oalsfx_debug_filter_uploads(self._h)

    # ---- voice filter sweeps (include/oalsfx_hip.h, "voice filter sweeps") ----
    def set_sweeps(self, sweeps, instances=None, lane=0):
        """sweeps[k] (an array of SWEEP_DTYPE, or desc.FilterSweep objects) becomes the sweep of instances[k] (None: 0 .. count - 1) in lane
        `lane`, from the next render on: the voice's filter, which must be ACTIVE, takes its coefficients per frame from the record."""
        idx, count = self._targets(sweeps, desc.FilterSweep, instances, "An instance is listed twice as a filter sweep target.")
        records = self._records(sweeps, count, "set_sweeps", SWEEP_DTYPE, desc.FilterSweep, (
            "sweeps are an array of SWEEP_DTYPE or a sequence of desc.FilterSweep", "the sweep array is not contiguous records of SWEEP_DTYPE",
            "{} instances but {} sweeps"))
        self._set_records("oalsfx_batch_set_lane_sweeps", lane, idx, count, records)

    def get_sweeps(self, instances=None, lane=0):
        """The sweeps of `instances` (None: all) in lane `lane`, as an array of SWEEP_DTYPE, as every render queued so far leaves them;
        waits."""
        return self._get_records("oalsfx_batch_get_lane_sweeps", SWEEP_DTYPE, instances, lane)

    def sweep_uploads(self):
        """How many renders put changed filter sweeps on the device first so far."""
        return self._lib.oalsfx_debug_sweep_uploads(self._h)

    # ---- filter programs (include/oalsfx_hip.h, "filter programs") ----
    def set_filter_programs(self, programs, instances=None, lane=0):
        """programs[k], 1 .. FILTER_PROGRAM_MAX sweep records (an array of SWEEP_DTYPE, or desc.FilterSweep objects), becomes the filter
        program of instances[k] (None: 0 .. count - 1) in lane `lane`: its first segment the current sweep, the rest the voice's queue,
        which the renders walk on the device.  `programs` may be one array [count][length] where all have the same length.  The whole
        program is replaced; it holds from the next render on.  What a record and a program must be is the library's to refuse."""
        same_length = isinstance(programs, np.ndarray) and programs.ndim == 2
        if not same_length:
            programs = list(programs)
        idx, count = self._targets(programs, None, instances, "An instance is listed twice as a filter program target.")
        if len(programs) != count:
            raise BatchError(f"set_filter_programs: {count} instances but {len(programs)} programs")
        lengths = (C.c_int * max(count, 1))()
        segments = np.zeros((count, FILTER_PROGRAM_MAX), dtype=SWEEP_DTYPE)
        what = ("sweeps are an array of SWEEP_DTYPE or a sequence of desc.FilterSweep", "the sweep array is not contiguous records of SWEEP_DTYPE",
                "{} segments but {} sweeps")
        for k in range(count):
            program = programs[k]
            length = 1 if isinstance(program, desc.FilterSweep) else len(program)
            if not 1 <= length <= FILTER_PROGRAM_MAX:
                raise BatchError("Filter program length out of range.")
            lengths[k] = length
            segments[k, :length] = self._records([program] if isinstance(program, desc.FilterSweep) else program, length, "set_filter_programs", SWEEP_DTYPE,
                                                 desc.FilterSweep, what)
        self._check(self._lib.oalsfx_batch_set_lane_filter_programs(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(segments.ctypes.data if count else 0)))

    def get_filter_programs(self, instances=None, lane=0):
        """The filter programs of `instances` (None: all) in lane `lane` as every render queued so far leaves them: a list of arrays of
        SWEEP_DTYPE, the current segment first, then the segments still queued; waits."""
        idx, count = self._instances(instances)
        lengths = (C.c_int * max(count, 1))()
        out = np.zeros((count, FILTER_PROGRAM_MAX), dtype=SWEEP_DTYPE)
        self._check(self._lib.oalsfx_batch_get_lane_filter_programs(self._h, operator.index(lane), idx, count, lengths, C.c_void_p(out.ctypes.data if count else 0)))
        return [out[k, :lengths[k]].copy() for k in range(count)]

    def filter_program_uploads(self):
        """How many renders put changed filter program queues on the device first so far."""
        return self._lib.oalsfx_debug_filter_program_uploads(self._h)

    def last_render_kernel(self):
        """"k_sampler_rows", "k_voice_rows", "k_fir_rows", with two lanes or more "k_mix_rows", while any voice's filter is ACTIVE
        "k_biquad_rows", or, while a voice's queue may hold a segment, "k_program_rows" and with an ACTIVE filter "k_program_biquad_rows";
        while a filter sweep may be under way "k_sweep_rows" and "k_sweep_program_rows" in the two filtered renders' place: what the last
        render launched ("" before the first).  While a filter program may hold a queued segment: "k_filter_program_rows", and
        "k_filter_program_env_rows" while an envelope program's queue may hold one as well."""
        return (self._lib.oalsfx_debug_last_render_kernel(self._h) or b"").decode()

    def sampler_uploads(self):
        """How many renders put changed sampler records on the device first so far."""
        return self._lib.oalsfx_debug_sampler_uploads(self._h)

    # ---- kernel timing (HIP events on the launch stream) ----
    def kernel_timing(self, enable=1):
        """0 / False: off; 1 / True: every mix call carries timing events; k > 1: every k-th call."""
        self._check(self._lib.oalsfx_batch_kernel_timing(self._h, int(enable)))

    def event_overhead(self, repeats=100):
        """Average microseconds an event pair around an empty kernel reads on the batch's stream."""
        us = C.c_double(0.0)
        self._check(self._lib.oalsfx_batch_event_overhead(self._h, repeats, C.byref(us)))
        return us.value

    def kernel_timing_samples(self, effect_type, max_samples=4096):
        """Per-launch durations (microseconds, raw event pairs) of the timed launches of `effect_type`."""
        buf = (C.c_double * max_samples)()
        n = self._lib.oalsfx_batch_kernel_timing_samples(self._h, effect_type, buf, max_samples)
        self._check(n >= 0)
        return list(buf[:min(n, max_samples)])

    def plan(self, slot=0):
        """(ring-light, reverbs proven steady, reverbs believed steady, reverbs on the general kernel) for the next mix call."""
        c = (C.c_int * 4)()
        self._check(self._lib.oalsfx_batch_plan(self._h, slot, c))
        return tuple(c)

    def placement(self):
        """(chunks, candidates probed, probe us on the chunk kept, probe us on the slowest candidate seen) of the delay-line placement search."""
        c, k = C.c_int(0), C.c_int(0)
        a, w = C.c_double(0.0), C.c_double(0.0)
        self._lib.oalsfx_batch_placement(self._h, C.byref(c), C.byref(k), C.byref(a), C.byref(w))
        return c.value, k.value, a.value, w.value

    @property
    def chained_calls(self):
        """mix_device calls (own stream) that overlapped with their neighbours on the device so far."""
        return self._lib.oalsfx_batch_chained_calls(self._h)

    def host_pipeline(self):
        """(form, probe us per call on three streams, probe us per call on one stream) of mix_async; form 0: still probing."""
        f, a, c = C.c_int(0), C.c_double(0), C.c_double(0)
        self._lib.oalsfx_debug_host_pipeline(self._h, C.byref(f), C.byref(a), C.byref(c))
        return f.value, a.value, c.value

    def chain_started(self):
        """(host count, device count) of the workgroups of chained launches started so far: the two must agree.  Waits."""
        h, d = C.c_uint(0), C.c_uint(0)
        self._check(self._lib.oalsfx_debug_chain_started(self._h, C.byref(h), C.byref(d)))
        return h.value, d.value

    @property
    def last_reverb_kernel(self):
        return (self._lib.oalsfx_batch_last_reverb_kernel(self._h) or b"").decode()

    def kernel_timing_read(self, effect_type):
        n, ms = C.c_int(0), C.c_double(0.0)
        self._check(self._lib.oalsfx_batch_kernel_timing_read(self._h, effect_type, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class Api:
    """One effect chain with the reference's method names; a `Batch` of one instance underneath."""

    def __init__(self):
        self._b = None
        self._error = ""

    def initialize(self, channel_format, sampling_rate, effect_count, device_id=0):
        self.uninitialize()
        try:
            self._b = Batch(1, channel_format, sampling_rate, effect_count, device_id)
        except BatchError as e:
            self._error = str(e)
            return False
        return True

    def is_initialized(self):
        return self._b is not None

    def uninitialize(self):
        if self._b is not None:
            self._b.close()
            self._b = None

    def get_error_message(self):
        return self._error

    def _guard(self, fn, fail=False):
        if self._b is None:
            self._error = "Not initialized."
            return fail
        try:
            return fn()
        except BatchError as e:
            self._error = str(e)
            return fail

    def get_sampling_rate(self):
        return self._guard(lambda: self._b.rate, 0)

    def get_channel_format(self):
        return self._guard(lambda: self._b.channel_format, desc.FMT_NONE)

    def get_channel_count(self):
        return self._guard(lambda: self._b.channels, 0)

    def get_effect_count(self):
        return self._guard(lambda: self._b.effect_count, 0)

    def set_effect_type(self, index, effect_type):
        return self._guard(lambda: self._b.set_effect_type(index, effect_type) or True)

    def set_effect(self, index, effect):
        # the reference's Api::set_effect stores the effect and returns false (src/oalsfxpp.cpp:3655-3657)
        self._guard(lambda: self._b.set_effect(index, effect))
        return False

    def get_effect(self, index, deferred=False):
        return self._guard(lambda: self._b.get_effect(0, index, deferred), None)

    def set_send_props(self, index, gain, gain_hf, gain_lf):
        return self._guard(lambda: self._b.set_send_props(index, gain, gain_hf, gain_lf) or True)

    def apply_changes(self):
        return self._guard(lambda: self._b.apply_changes() or True)

    def mix(self, src):
        """src: [frames][channels] float32; returns the mixed frames or None on failure."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        if src.size == 0:
            return src.copy()
        return self._guard(lambda: self._b.mix(src[None])[0], None)


def trim_pools():
    """Gives the uncached device memory that waits for reuse back to the runtime (oalsfx_trim_pools); returns the bytes freed."""
    return lib.load().oalsfx_trim_pools()


def pools_waiting_bytes():
    return lib.load().oalsfx_pools_waiting_bytes()


class Group:
    """One instance range over several devices (oalsfx_group_*): a batch and a host thread per device, contiguous shards."""

    def __init__(self, n_total, device_ids, channel_format=desc.FMT_STEREO, sampling_rate=48000, effect_count=1):
        self._lib = lib.load()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = self._lib.oalsfx_group_create(n_total, ids, len(device_ids), channel_format, sampling_rate, effect_count)
        if not h:
            raise BatchError(self._lib.oalsfx_group_last_error().decode())
        self._h = C.c_void_p(h)
        self.n = n_total
        self.channel_format, self.rate, self.effect_count = channel_format, sampling_rate, effect_count
        self.channels = self._lib.oalsfx_group_channels(self._h)
        self.shards = []
        for k in range(self._lib.oalsfx_group_devices(self._h)):
            d, f, c = C.c_int(), C.c_int(), C.c_int()
            self._lib.oalsfx_group_shard(self._h, k, C.byref(d), C.byref(f), C.byref(c))
            self.shards.append((d.value, f.value, c.value))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.oalsfx_group_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, ok):
        if not ok:
            raise BatchError(self._lib.oalsfx_group_error(self._h).decode())

    def batch(self, k):
        """Shard k's batch (oalsfx_group_batch) as a `Batch` that does not own it: instance numbers are the shard's own, global number
        shards[k][1] + i.  For what the group has no call of its own for (snapshot, restore, reset, read-backs); it must not be used
        while a group call is running, nor after the group is closed (the view keeps the group alive until it is closed itself)."""
        h = self._lib.oalsfx_group_batch(self._h, operator.index(k))
        if not h:
            raise BatchError("Shard number is out of range.")
        return Batch._view(self._lib, h, self.channel_format, self.rate, self.effect_count, self.shards[k][0], self)

    def set_effect_type(self, slot, effect_type, first=0, count=None):
        self._check(self._lib.oalsfx_group_set_effect_type(self._h, first, self.n - first if count is None else count, slot, effect_type))

    def set_effect(self, slot, effects, first=0):
        """effects: one desc.Effect for the whole range from `first` on, or a list of them (one per instance from `first` on)."""
        if isinstance(effects, desc.Effect):
            self._check(self._lib.oalsfx_group_set_effect(self._h, first, self.n - first, slot, C.byref(effects), 0))
        else:
            arr = (desc.Effect * len(effects))(*effects)
            self._check(self._lib.oalsfx_group_set_effect(self._h, first, len(effects), slot, arr, C.sizeof(desc.Effect)))

    def set_effect_props(self, slot, props, first=0, count=None):
        """props: one desc.EffectPropsU for the range, or a list of them (one per instance from `first` on)."""
        if isinstance(props, desc.EffectPropsU):
            self._check(self._lib.oalsfx_group_set_effect_props(self._h, first, self.n - first if count is None else count, slot, C.byref(props), 0))
        else:
            arr = (desc.EffectPropsU * len(props))(*props)
            self._check(self._lib.oalsfx_group_set_effect_props(self._h, first, len(props), slot, arr, C.sizeof(desc.EffectPropsU)))

    def set_send_props(self, slot, gain, gain_hf, gain_lf, first=0, count=None):
        sp = desc.SendProps(gain, gain_hf, gain_lf)
        self._check(self._lib.oalsfx_group_set_send_props(self._h, first, self.n - first if count is None else count, slot, C.byref(sp)))

    def apply_changes(self, first=0, count=None):
        self._check(self._lib.oalsfx_group_apply_changes(self._h, first, self.n - first if count is None else count))

    def mix(self, src):
        """src: float32 [n_total][frames][channels] in host memory; returns the output array."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        frames = src.shape[1]
        dst = np.empty_like(src)
        self._check(self._lib.oalsfx_group_mix(self._h, frames, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)))
        return dst

    def mix_device(self, frames, src_ptrs, dst_ptrs):
        """One device pointer per shard each (that shard's [count][frames][channels]); queues and returns."""
        s = (C.c_void_p * len(src_ptrs))(*src_ptrs)
        d = (C.c_void_p * len(dst_ptrs))(*dst_ptrs)
        self._check(self._lib.oalsfx_group_mix_device(self._h, frames, s, d))

    def mix_device_multi(self, frames, src_ptrs, dst_ptrs):
        """Several buffers per shard: src_ptrs[d][k], dst_ptrs[d][k] for shard d, buffer k (Batch.mix_device_multi on every shard)."""
        if len(src_ptrs) != len(self.shards) or len(dst_ptrs) != len(self.shards):
            raise BatchError(f"mix_device_multi: one row of buffers per shard ({len(self.shards)}), sources and destinations")
        buffers = len(src_ptrs[0]) if len(src_ptrs) else 0
        if any(len(x) != buffers for x in list(src_ptrs) + list(dst_ptrs)):
            raise BatchError("mix_device_multi: the same number of buffers for every shard, sources and destinations")
        s = (C.c_void_p * max(1, len(src_ptrs) * buffers))(*[p for row in src_ptrs for p in row])
        d = (C.c_void_p * max(1, len(dst_ptrs) * buffers))(*[p for row in dst_ptrs for p in row])
        self._check(self._lib.oalsfx_group_mix_device_multi(self._h, frames, buffers, s, d))

    def set_routing(self, bus=None, gain=None, first=0):
        """Batch.set_routing in the group's global instance numbering."""
        count, buses, gains = Batch._routing(self.n, first, bus, gain)
        self._check(self._lib.oalsfx_group_set_routing(self._h, first, count, buses, gains))

    def mix_downmix(self, src, n_buses):
        """Every shard's instances summed on its device, the shards' buses added on the host in shard order; returns
        [n_buses][frames][channels]."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        if src.ndim != 3 or src.shape[0] != self.n or src.shape[2] != self.channels:
            raise BatchError(f"mix_downmix: the source is {src.shape}, not [{self.n}][frames][{self.channels}]")
        Batch._downmix_counts(src.shape[1], n_buses)
        dst = np.empty((n_buses, src.shape[1], self.channels), dtype=np.float32)
        self._check(self._lib.oalsfx_group_mix_downmix(self._h, src.shape[1], src.ctypes.data_as(_fp), n_buses, dst.ctypes.data_as(_fp)))
        return dst

    def mix_downmix_meter(self, src, n_buses, threshold, carry=False, voice_meters=None):
        """mix_downmix() plus the voices' meters in the global instance numbering: returns (buses, records of api.METER_DTYPE).  A group's
        buses are finished on the host, so there are no bus meters."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        if src.ndim != 3 or src.shape[0] != self.n or src.shape[2] != self.channels:
            raise BatchError(f"mix_downmix_meter: the source is {src.shape}, not [{self.n}][frames][{self.channels}]")
        Batch._downmix_counts(src.shape[1], n_buses)
        flags = Batch._meter_args(src.shape[1], threshold, carry)
        vm = Batch._meter_array(voice_meters, self.n, "mix_downmix_meter")
        dst = np.empty((n_buses, src.shape[1], self.channels), dtype=np.float32)
        self._check(self._lib.oalsfx_group_mix_downmix_meter(self._h, src.shape[1], src.ctypes.data_as(_fp), n_buses, dst.ctypes.data_as(_fp),
                                                             threshold, flags, C.c_void_p(vm.ctypes.data)))
        return dst, vm

    def synchronize(self):
        self._check(self._lib.oalsfx_group_synchronize(self._h))
