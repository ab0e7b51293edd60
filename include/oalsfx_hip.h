/*
 * oalsfx_hip.h -- C ABI of liboalsfx_hip.so, the MI355X batch backend for the
 * oalsfxpp effect-process hot path.
 *
 * The reference has no FFI: its only seam is C++ (class oalsfxpp::Api, reference
 * src/oalsfxpp.h:760-922, and the internal EffectState::process virtual,
 * src/oalsfxpp.cpp:2239-2246).  This ABI is what a binding of that seam needs when
 * thousands of independent Api instances are advanced together: each call below
 * names the reference entry point it stands in for.  All handles are opaque, all
 * buffers are caller-owned plain pointers, no C++ or torch types cross the boundary.
 *
 * Conventions (same as the reference): calls return 1 on success and 0 on
 * failure; oalsfx_batch_error() then returns a static message.  Samples are
 * interleaved fp32 frames, [instance][frame][channel], and outputs are not clipped.
 * A batch is not thread-safe; distinct batches are independent.
 */
#ifndef OALSFX_HIP_H
#define OALSFX_HIP_H

#include "oalsfx_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oalsfx_batch oalsfx_batch;

/* Mirror of oalsfxpp::Effect (reference src/oalsfxpp.h:532-548): 4-byte type tag followed by
 * the 108-byte EffectProps union.  sizeof == 112. */
typedef struct {
    int32_t type;
    unsigned char props[108];
} oalsfx_effect;

/* Mirror of oalsfxpp::SendProps (reference src/oalsfxpp.h:550-581). */
typedef struct { float gain, gain_hf, gain_lf; } oalsfx_send_props;

/* ---- lifecycle: n_instances x Api::initialize (reference src/oalsfxpp.cpp:3480-3504, 2846-2905).
 * channel_format is an OALSFX_FMT_* value; device_id is the HIP device ordinal.  Fails (returns
 * NULL and sets the global message readable through oalsfx_last_error) when the arguments are
 * out of range or no HIP device is usable -- there is no CPU fallback. */
oalsfx_batch* oalsfx_batch_create(int n_instances, int channel_format, int sampling_rate, int effect_count, int device_id);
void oalsfx_batch_destroy(oalsfx_batch* b);                     /* Api::uninitialize, src/oalsfxpp.cpp:3831 */
const char* oalsfx_batch_error(const oalsfx_batch* b);          /* Api::get_error_message, src/oalsfxpp.cpp:3836 */
const char* oalsfx_last_error(void);                            /* message of a failed oalsfx_batch_create */

int oalsfx_batch_instances(const oalsfx_batch* b);
int oalsfx_batch_channels(const oalsfx_batch* b);               /* Api::get_channel_count, src/oalsfxpp.cpp:3533 */
int oalsfx_batch_sampling_rate(const oalsfx_batch* b);          /* Api::get_sampling_rate, src/oalsfxpp.cpp:3511 */
int oalsfx_batch_effect_count(const oalsfx_batch* b);           /* Api::get_effect_count, src/oalsfxpp.cpp:3544 */

/* ---- deferred property setters for the instance range [first, first+count).
 * `stride_bytes` is the distance between consecutive per-instance records at `effects` /
 * `props`; 0 broadcasts one record to the whole range. */
/* Api::set_effect (src/oalsfxpp.cpp:3639-3658; this ABI reports success as 1, the C++ facade keeps
 * the reference's quirk of returning false). */
int oalsfx_batch_set_effect(oalsfx_batch* b, int first, int count, int slot, const oalsfx_effect* effects, int stride_bytes);
/* The same for instances that are not neighbours: instances[k] gets effects[k] (stride_bytes apart; 0: one effect for all).  One call
 * where a loop over oalsfx_batch_set_effect would make one per instance -- a foreign-function call costs more than the setter. */
int oalsfx_batch_set_effect_at(oalsfx_batch* b, const int* instances, int count, int slot, const oalsfx_effect* effects, int stride_bytes);
/* Api::set_effect_type (src/oalsfxpp.cpp:3597-3616): type tag + that type's default properties. */
int oalsfx_batch_set_effect_type(oalsfx_batch* b, int first, int count, int slot, int effect_type);
/* Api::set_effect_props (src/oalsfxpp.cpp:3618-3637): replaces the 108-byte union only. */
int oalsfx_batch_set_effect_props(oalsfx_batch* b, int first, int count, int slot, const void* props, int stride_bytes);
/* Api::set_send_props (src/oalsfxpp.cpp:3712-3736); slot < 0 addresses the direct send. */
int oalsfx_batch_set_send_props(oalsfx_batch* b, int first, int count, int slot, const oalsfx_send_props* props);
/* Api::get_effect / get_deferred_effect (src/oalsfxpp.cpp:3555-3595) for one instance. */
int oalsfx_batch_get_effect(const oalsfx_batch* b, int instance, int slot, int deferred, oalsfx_effect* out);
/* Api::get_send_props / get_deferred_send_props (src/oalsfxpp.cpp:3660-3710). */
int oalsfx_batch_get_send_props(const oalsfx_batch* b, int instance, int slot, int deferred, oalsfx_send_props* out);
/* Api::apply_changes (src/oalsfxpp.cpp:3738-3783) on every instance of the range. */
int oalsfx_batch_apply_changes(oalsfx_batch* b, int first, int count);

/* ---- the hot path: Api::mix (src/oalsfxpp.cpp:3785-3829) for every instance at once.
 * src and dst hold n_instances * frames * channels floats.  frames may be any positive count;
 * more than 2048 are processed in 2048-frame chunks like the reference.  frames == 0 succeeds. */
int oalsfx_batch_mix(oalsfx_batch* b, int frames, const float* src_host, float* dst_host);
/* The same for a caller whose instances each have a source and a target buffer of their own (n_instances pointers each, every buffer
 * frames * channels floats): what a program that held one oalsfxpp::Api object per voice has.  Gathered, mixed as one call, scattered. */
int oalsfx_batch_mix_gather(oalsfx_batch* b, int frames, const float* const* src_per_instance, float* const* dst_per_instance);
/* Same with buffers already resident in device memory; launches on `hip_stream` (a hipStream_t, or
 * NULL for the batch's own stream) and returns without synchronising.
 * With hip_stream NULL the call is complete when oalsfx_batch_synchronize (or any other call on the batch that waits or reads back)
 * returns; consecutive such calls may overlap on the device where the instances allow it (a step that is one steady-state reverb
 * launch, a launch of reverb-free slots followed by one of the reverbs' slot, or one grid of ring-light effects and proven reverbs:
 * each instance of the later call starts when the earlier call is through with that instance), which takes the launch gap
 * between dependent kernels out of a streaming loop.  A caller that wants the launches in the order of a stream it can queue its
 * own work on passes that stream, or asks for the batch's with oalsfx_batch_stream, which switches the overlap off.
 * Alignment: stereo buffers must be 8-byte aligned; mono and more than two channels need 4 bytes.  A call whose dst_dev is not 8-byte
 * aligned does not overlap its neighbours: it runs in stream order. */
int oalsfx_batch_mix_device(oalsfx_batch* b, int frames, const float* src_dev, float* dst_dev, void* hip_stream);
/* The same as `buffers` consecutive oalsfx_batch_mix_device(b, frames, src_dev[k], dst_dev[k], hip_stream) calls, k = 0, 1, ...
 * (outputs, effect state and delay lines bit-identical), run in as few launches as the batch's instances allow: a caller with a queue
 * of device buffers, each [n_instances][frames][channels], hands them in at once.  Where every instance of a one-slot mono / stereo batch
 * is a proven-steady reverb, no send filter is on and frames is a multiple of 64, up to 2048 / frames buffers go through one launch;
 * otherwise, and where a buffer's output overlaps a later buffer's input or output, the buffers go through one call each.  The two
 * pointer tables are host memory, read during the call only; src_dev[k] == dst_dev[k] (in place) is allowed.  buffers == 0 or
 * frames == 0 succeeds and does nothing.  Stream semantics as for oalsfx_batch_mix_device. */
int oalsfx_batch_mix_device_multi(oalsfx_batch* b, int frames, int buffers, const float* const* src_dev, float* const* dst_dev, void* hip_stream);
int oalsfx_batch_synchronize(oalsfx_batch* b);
/* How many oalsfx_batch_mix_device calls overlapped with their neighbours that way so far (tests, benchmark records). */
long long oalsfx_batch_chained_calls(const oalsfx_batch* b);
/* Api::mix for a caller that streams buffer after buffer from host memory (what the reference's only entry point is used for,
 * src/oalsfxpp.cpp:3785-3829, src/oalsfxpp_test.cpp:891): returns as soon as the call is queued.  The copy in of call k + 1, the
 * kernels of call k and the copy out of call k - 1 overlap on three streams, ordered by events.  `src_host` and `dst_host` must stay
 * untouched until the call is through, which is the case once oalsfx_batch_wait has returned, or once three further
 * oalsfx_batch_mix_async calls have (a call first waits for the one that used its staging slot three calls earlier).  The copies
 * only run beside the kernels when the host buffers are page-locked (oalsfx_pinned_alloc, or the caller's own hipHostMalloc /
 * hipHostRegister); pageable buffers work but serialise.  Property setters and apply_changes may be called between the calls as
 * with oalsfx_batch_mix; they take effect from the next call on. */
int oalsfx_batch_mix_async(oalsfx_batch* b, int frames, const float* src_host, float* dst_host);
/* Waits until every queued oalsfx_batch_mix_async call has delivered its output. */
int oalsfx_batch_wait(oalsfx_batch* b);
/* Page-locked host memory for the two calls above (hipHostMalloc / hipHostFree), so that a caller need not link HIP itself. */
void* oalsfx_pinned_alloc(unsigned long long bytes);
void oalsfx_pinned_free(void* p);
/* The batch's own HIP stream (a hipStream_t) so callers can bracket launches with their own events.  From this call on every launch of
 * oalsfx_batch_mix_device(..., NULL) is in the order of that stream (no overlap of consecutive calls). */
void* oalsfx_batch_stream(oalsfx_batch* b);

/* ---- one instance range over several GPUs (BASELINE configs[4]: 262 144 EAX reverbs over the eight GPUs of a node).  The reference's
 * instances share nothing (src/oalsfxpp.cpp:2984-3037), so the split is a contiguous range per device -- sizes differ by at most one --,
 * one batch, one stream set and one host thread per device, no collective and no peer traffic.  device_ids lists the HIP ordinals (an
 * ordinal may appear more than once: two shards on one GPU, which is how the split is rehearsed on a one-GPU box).  Setters take ranges
 * of the global instance numbering; the buffers of oalsfx_group_mix hold the whole range, [n_total][frames][channels], in host memory,
 * and every device's thread copies its part in, runs its kernels and copies out (Api::mix, src/oalsfxpp.cpp:3785-3829, for every
 * instance); oalsfx_group_mix_device takes one device-resident source and target buffer per shard and only queues (consecutive calls
 * overlap on every device as for a batch alone), oalsfx_group_synchronize waits for all.  A failed call's message (oalsfx_group_error)
 * names the device; oalsfx_group_last_error is for a failed create.  Not thread-safe, like a batch. */
typedef struct oalsfx_group oalsfx_group;
oalsfx_group* oalsfx_group_create(int n_total, const int* device_ids, int n_devices, int channel_format, int sampling_rate, int effect_count);
void oalsfx_group_destroy(oalsfx_group* g);
const char* oalsfx_group_error(const oalsfx_group* g);
const char* oalsfx_group_last_error(void);
int oalsfx_group_instances(const oalsfx_group* g);
int oalsfx_group_channels(const oalsfx_group* g);
int oalsfx_group_devices(const oalsfx_group* g);
/* Shard k: its device ordinal, first global instance and instance count; and its batch, for what the group does not forward (read-backs,
 * oalsfx_batch_plan, the pipelined host path). */
int oalsfx_group_shard(const oalsfx_group* g, int k, int* device_id, int* first, int* count);
oalsfx_batch* oalsfx_group_batch(oalsfx_group* g, int k);
int oalsfx_group_set_effect(oalsfx_group* g, int first, int count, int slot, const oalsfx_effect* effects, int stride_bytes);
int oalsfx_group_set_effect_type(oalsfx_group* g, int first, int count, int slot, int effect_type);
int oalsfx_group_set_effect_props(oalsfx_group* g, int first, int count, int slot, const void* props, int stride_bytes);
int oalsfx_group_set_send_props(oalsfx_group* g, int first, int count, int slot, const oalsfx_send_props* props);
int oalsfx_group_apply_changes(oalsfx_group* g, int first, int count);
int oalsfx_group_mix(oalsfx_group* g, int frames, const float* src_host, float* dst_host);
int oalsfx_group_mix_device(oalsfx_group* g, int frames, const float* const* src_per_device, float* const* dst_per_device);
/* oalsfx_batch_mix_device_multi on every shard: shard d's buffers are src_dev[d * buffers + k], dst_dev[d * buffers + k]. */
int oalsfx_group_mix_device_multi(oalsfx_group* g, int frames, int buffers, const float* const* src_dev, float* const* dst_dev);
int oalsfx_group_synchronize(oalsfx_group* g);
/* Bus downmix over the group (see "bus downmix" below): routing in the global instance numbering; oalsfx_group_mix_downmix is
 * oalsfx_batch_mix_downmix on every shard -- each sums its own instances on its own device, a shard's chunks starting at the shard's
 * first member of the bus -- after which the host adds the shards' bus buffers in shard order, out = ((+0.0f + s_0) + s_1) + ...  This
 * is another arithmetic than that of one batch over the same instances: the results agree bit for bit only for a bus whose members all
 * lie in shard 0.  src_host: [n_total][frames][channels]; dst_bus_host: [n_buses][frames][channels].  No device-to-device traffic. */
int oalsfx_group_set_routing(oalsfx_group* g, int first, int count, const int* bus, const float* gain);
int oalsfx_group_mix_downmix(oalsfx_group* g, int frames, const float* src_host, int n_buses, float* dst_bus_host);

/* ---- device memory the library keeps between batches.  Batches whose calls can overlap on the device keep their delay lines, effect
 * state and hot records in uncached device memory, which the library takes from the runtime in 2 MiB granules and keeps for the next
 * batch that asks for a block of that size -- by default for the life of the process: on this runtime, uncached blocks given back with
 * hipFree have been seen to disturb ordinary allocations made afterwards (profiles/r04b_uncached_free_hazard/).  A process
 * that needs the memory back calls oalsfx_trim_pools: it waits for the device, frees everything that waits for reuse and returns the
 * bytes freed; OALSFX_UNCACHED_POOL_MAX_GIB=<GiB> (environment) does the same to whatever exceeds that much whenever a batch is
 * destroyed.  oalsfx_pools_waiting_bytes says how much waits.  Process-wide. */
unsigned long long oalsfx_trim_pools(void);
unsigned long long oalsfx_pools_waiting_bytes(void);

/* ---- state read-back for tests and checkpoints (the reference keeps this in private members of
 * the EffectState subclasses). */
int oalsfx_batch_read_slot(oalsfx_batch* b, int instance, int slot, oalsfx_slot_params* params, oalsfx_slot_state* state);
/* Copies up to max_floats of the slot's delay rings; returns the ring size in floats (0: no ring). */
int oalsfx_batch_read_ring(oalsfx_batch* b, int instance, int slot, float* out, int max_floats);
int oalsfx_batch_read_source(oalsfx_batch* b, int instance, oalsfx_source_params* params, oalsfx_source_state* state);

/* ---- instance state: snapshot, restore, reset.  What the reference keeps in private members written out and put
 * back -- rollback, moving voices between batches or devices, forking a voice, resuming an offline render -- and Api::initialize for
 * single instances (voice reuse).  `instances` lists batch-local instance numbers (NULL: 0 .. count - 1).
 *
 * A restored instance behaves exactly as the snapshotted one would have: every later call sequence gives bit-identical outputs, rings,
 * read_source states and read_slot states (the update stamps update_seq / seen_seq are renumbered, their relation kept), and
 * get_effect / get_send_props return what the source returned at snapshot time, active and deferred.  Changes that were applied but not
 * mixed yet are folded in first (as the read-backs do); deferred changes that were never applied travel as deferred values; an auxiliary
 * send written since the instance's sends were last derived leaves the sends as derived until the next update, as on the source.
 * Ordering: each of the three calls comes after every call already queued on the batch (a run of overlapping oalsfx_batch_mix_device
 * calls is joined, a launch on a caller's stream waited for) and ends that run.  Snapshot and the device part of restore and reset run
 * on the batch's stream: `dst` is complete, and `src` may be reused, once oalsfx_batch_synchronize (or any call that waits) returns.
 * The next oalsfx_batch_mix_device / _multi call on a caller's stream makes that stream wait for them before its own launches.
 * Restore waits for the batch's stream before it reads the blob's header.
 * Memory: `dst` / `src` are device memory of the batch's device or page-locked host memory (oalsfx_pinned_alloc), 16-byte aligned.
 * Blob: position-independent (offsets, no device pointers), versioned, with a magic value, the channel format, rate, effect count and
 * instance count, a per-instance offset table and 256-byte-aligned sections: per instance its host records (active and deferred effects,
 * direct and auxiliary send properties, pending flags; per slot its type, ring size, update stamp, the frames since its state started and
 * whether its late line was ever modulated), its device records (slot states, send-filter histories, the sends as derived) and each
 * slot's delay lines.  A blob copied to another device, or to disk and back, restores.  No batch-level cache travels (proven-steady
 * records, launch lists): a restored instance runs on the general and believed-steady builds until the device has proven it steady again
 * -- bit-identical by design, and slower for the first calls.
 * Refusals (return 0 with a message in oalsfx_batch_error; the batch is left as it was): restore of an unknown magic value or version,
 * another channel format, rate or effect count, `bytes` short of what the header says, a count other than the blob's, duplicate or
 * out-of-range targets, a batch a failed chained launch has poisoned; snapshot into `bytes` short of oalsfx_batch_snapshot_bytes. */
/* Bytes a snapshot of these instances takes; their slot types at this moment decide the ring sizes.  0 on error. */
unsigned long long oalsfx_batch_snapshot_bytes(oalsfx_batch* b, const int* instances, int count);
/* Writes the complete state of the listed instances into `dst` (entry k: instances[k]). */
int oalsfx_batch_snapshot(oalsfx_batch* b, const int* instances, int count, void* dst, unsigned long long bytes);
/* Puts snapshot entry k into instances[k], for k < count.  The target may be this batch or any batch with the same channel format, rate
 * and effect count; a target slot whose delay lines are of another size gives its slab back and takes one of the image's size. */
int oalsfx_batch_restore(oalsfx_batch* b, const int* instances, int count, const void* src, unsigned long long bytes);
/* Api::initialize for the listed instances only: Null effects, default sends, active == deferred, zeroed state, no delay lines. */
int oalsfx_batch_reset(oalsfx_batch* b, const int* instances, int count);

/* ---- bus downmix: the instances' outputs summed into buses on the device.  Nothing in the reference (Api::mix stops at one output per
 * instance); what OpenAL Soft does when it adds every source into the device's buffer, and what a caller of 4096 voices wants instead of
 * 4096 outputs.  Every instance is routed to one bus, or to none, with a gain; one call sums the routed outputs,
 * [instance][frame][channel], into [bus][frame][channel].  The order of the sum is part of the contract, so that the result is
 * bit-reproducible (fp32 throughout, product and sum rounded separately -- no fused multiply-add --, the reference's own mixing
 * convention dst += src * gain, src/oalsfxpp.cpp:2747):
 *   routing of instance i: bus[i] is -1 (nowhere) or a bus number from 0 up, gain[i] any fp32 value; after oalsfx_batch_create bus = 0
 *   and gain = 1.0f.  The members of bus B are the instances with bus[i] == B in ascending instance order, m_0 < m_1 < ..., cut into
 *   consecutive chunks of OALSFX_DOWNMIX_CHUNK members (the last may be short).  For every frame f and channel c:
 *     chunk j:  p_j = +0.0f;  for k in chunk j, ascending:  p_j = p_j + (x[m_k][f][c] * gain[m_k]);
 *     the bus:  out = +0.0f;  for j ascending:  out = out + p_j.
 *   Every member takes part whatever its gain or value (a gain of 0 still turns an Inf into a NaN); no silence threshold, no clipping,
 *   no flush of denormals.  A bus without members is +0.0f throughout.
 * Routing is state of the batch beside its instances, not instance state: oalsfx_batch_reset, _snapshot and _restore neither touch nor
 * carry it (the blob's version is unchanged), and no effect call reads it. */
#define OALSFX_DOWNMIX_CHUNK 32
/* Routing of the instances [first, first + count): bus[k] and gain[k] for instance first + k; bus == NULL leaves the buses, gain == NULL
 * the gains.  Not deferred (it is no property of the reference): it holds from the next downmix on.  Refuses a bus below -1 and a range
 * outside the batch (nothing is changed then); a NaN is a gain like any other value. */
int oalsfx_batch_set_routing(oalsfx_batch* b, int first, int count, const int* bus, const float* gain);
int oalsfx_batch_get_routing(const oalsfx_batch* b, int instance, int* bus, float* gain);
/* Sums src_dev, [n_instances][frames][channels] -- typically what oalsfx_batch_mix_device has just written, but any buffer of that shape
 * --, into dst_bus_dev, [n_buses][frames][channels], every element of which is overwritten.  Any frames >= 0 (no 2048 limit: the sum is
 * element-wise; frames == 0 succeeds and does nothing), n_buses >= 1.  Asynchronous.  Ordering as for the snapshot calls: it comes after
 * every call already queued on the batch; with hip_stream NULL it runs on the batch's stream and ends a run of overlapping
 * oalsfx_batch_mix_device calls, with a caller's stream it is queued there behind what the batch has in flight.  The routing table goes
 * to the device only when it has changed since the last downmix.  Alignment as for oalsfx_batch_mix_device (4 bytes are enough for any
 * format; wider loads are used where both pointers allow, with the same bits).
 * Refusals (return 0 with a message, nothing written): an instance routed to a bus the call does not have ("Instance %d is routed to bus
 * %d; the call has %d."), NULL pointers, negative counts, n_buses < 1, dst_bus_dev overlapping src_dev, a batch a failed chained launch
 * has poisoned. */
int oalsfx_batch_downmix_device(oalsfx_batch* b, int frames, const float* src_dev, int n_buses, float* dst_bus_dev, void* hip_stream);
/* oalsfx_batch_mix whose copy out is the buses only: copy in of n_instances * frames * channels floats, the effect launches into a
 * buffer the batch owns (more than 2048 frames in 2048-frame chunks, like oalsfx_batch_mix), the downmix, copy out of n_buses * frames *
 * channels floats, wait. */
int oalsfx_batch_mix_downmix(oalsfx_batch* b, int frames, const float* src_host, int n_buses, float* dst_bus_host);

/* ---- bus sends: an instance feeds up to OALSFX_BUS_SENDS buses, each with a gain of its own, and a gain may ramp.  The EFX topology
 * -- many sources, a few shared effect slots, a send level per source -- falls out of it: a batch of voices downmixes into
 * [bus][frame][channel] on the device, bus 0 the master and buses 1..R the inputs of R rooms; those buses are the src_dev of
 * oalsfx_batch_mix_device of a second batch of R reverbs (the shapes agree), whose own downmix gives the rooms' share of the master.
 *   Every instance has OALSFX_BUS_SENDS sends, (bus, gain) each.  Send 0 is the routing of "bus downmix": bus 0, gain 1.0f after
 *   oalsfx_batch_create; oalsfx_batch_set_routing and _get_routing are its forms and keep their contract.  Sends 1 .. are bus -1, gain
 *   1.0f after creation.
 *   Members: the members of bus B are the pairs (instance, send) with that bus, ordered by instance ascending and, inside one
 *   instance, by send ascending, cut into chunks of OALSFX_DOWNMIX_CHUNK exactly as stated above.  An instance that reaches one bus
 *   through two sends is two members of it.
 *   Element arithmetic: the stated one with gain[m_k] replaced by the member's gain for that frame, e:  p_j = p_j + (x[f][c] * e).
 *   Ramps: a send may carry a ramp (gain_from, gain_step, gain_to, R, done).  For frame f of a downmix call n = done + f, and
 *     n <  R:  e = gain_from + ((float)n * gain_step)     (product and sum rounded separately, nothing fused, no running sum)
 *     n >= R:  e = gain_to
 *   R <= 2^24, so (float)n is exact wherever it is formed.  Without a ramp e is the send's gain, and the bits are those of "bus
 *   downmix".  This is the voice envelopes' formula and not the reference's gain += step (MixHelpers::mix, src/oalsfxpp.cpp:2752), so
 *   that any split of a stretch of frames into calls gives the same bits.
 *   Clock: every downmix of F frames -- oalsfx_batch_downmix_device, _mix_downmix, _mix_downmix_meter, _play_downmix_meter -- advances
 *   every ramp of the batch by F, done = min(R, done + F), whatever the send's bus, -1 included; a ramp with done == R has ended, and
 *   the send's gain is gain_to.  The host knows F of every call: the counters live on the host, the device keeps no ramp state.  Two
 *   downmix calls over the same frames (the same outputs summed twice, say into two sets of buses) advance the ramps twice.
 * Sends and ramps are state of the batch beside its instances, like the routing: oalsfx_batch_reset, _snapshot and _restore neither
 * touch nor carry them.  A group offers send 0 only (oalsfx_group_set_routing; oalsfx_group_batch for the rest).
 * While no routed send ramps, the downmix launches what it launched before sends existed, from a longer member list; while one does,
 * level 1 is a kernel that forms e per frame, and the table goes to the device when sends or ramps are set and once more when the last
 * ramp has ended. */
#define OALSFX_BUS_SENDS 4
/* Send `send` of the instances [first, first + count): bus[k] and gain[k] for instance first + k.  bus == NULL leaves the buses, gain ==
 * NULL the gains.  A gain cancels the send's ramp; a new bus alone keeps it running.  Holds from the next downmix on.  Refusals (nothing
 * is changed): "Send out of range.", "Bus number is out of range." (below -1), a range outside the batch, a poisoned batch. */
int oalsfx_batch_set_send_routing(oalsfx_batch* b, int send, int first, int count, const int* bus, const float* gain);
/* bus; gain: the value the next downmixed frame gets, by the formula above in fp32; gain_to and frames_left: where the ramp leads and
 * how many frames it still takes -- without a ramp gain_to == gain and frames_left == 0.  Any pointer may be NULL. */
int oalsfx_batch_get_send_routing(const oalsfx_batch* b, int instance, int send, int* bus, float* gain, float* gain_to, uint32_t* frames_left);
/* Starts a ramp of `frames` downmixed frames on send `send` of the instances [first, first + count) towards gain_to[k]: gain_from is the
 * current value, as oalsfx_batch_get_send_routing returns it (so a ramp restarted in mid-ramp goes on from where its predecessor was),
 * gain_step = (gain_to - gain_from) / (float)frames -- one subtraction and one division in fp32 --, done = 0.  frames == 0 sets the gain
 * at once.  Any fp32 value is a gain.  Refusals as above, "Ramp length out of range." for frames > 2^24, and "No ramp
 * targets." for a NULL gain_to with count > 0. */
int oalsfx_batch_set_send_ramps(oalsfx_batch* b, int send, int first, int count, const float* gain_to, uint32_t frames);
/* A downmix call that has fewer buses than a send names is refused with the message of "bus downmix" for send 0 and with "Instance %d,
 * send %d is routed to bus %d; the call has %d." for the others. */

/* ---- level meters: peak, energy, non-finite count and trailing silence per row, on the device.  A row is one [frames][channels] block: an
 * instance's output or a bus.  Nothing in the reference; what every mixer has, and what a voice pool needs to see that a reverb tail has
 * died away (then oalsfx_batch_reset takes the voice back) or that a voice has gone NaN, without copying any output out: with
 * oalsfx_batch_mix_downmix the per-voice outputs never leave the device, and the answer is 80 bytes per voice.  The order of the
 * arithmetic is part of the contract, so that the records are bit-reproducible.  For row r, F frames, C channels, fp32 throughout,
 * denormals not flushed, product and sum rounded separately (no fused multiply-add), as in the downmix:
 *   peak[c]:    p = +0.0f; for every f: p = fmaxf(p, fabsf(x[f][c])).  A NaN takes no part (fmaxf returns the other operand); an Inf gives
 *               +Inf.  The order does not matter; the value is exact.
 *   sumsq[c]:   lane l of OALSFX_METER_LANES owns the frames f = l (mod 64).  q_l = +0.0f; for f = l, l + 64, l + 128, ... < F, ascending:
 *               q_l = q_l + (x[f][c] * x[f][c]).  Then for s = 32, 16, 8, 4, 2, 1: for every l < s, q_l = q_l + q_{l+s}.  sumsq[c] = q_0.
 *               Lanes without a frame hold +0.0f.  NaN and Inf propagate as IEEE arithmetic has them.
 *   nonfinite:  the number of elements x[f][c] with !(fabsf(x) < INFINITY).
 *   quiet:      frame f is quiet iff fabsf(x[f][c]) <= threshold for every channel c; a NaN makes the frame loud.
 *               T = F - 1 - (the last loud f), or F when no frame is loud.
 *   without OALSFX_METER_CARRY:  quiet_run = T, peak_hold = max_c peak[c].  What was at the destination is not read.
 *   with OALSFX_METER_CARRY the record already at the destination is read first:
 *               quiet_run = (T == F) ? min(old.quiet_run + F, UINT32_MAX) : T;  peak_hold = fmaxf(old.peak_hold, max_c peak[c]).
 *               A caller zero-fills the records once and then sees, call after call, for how many frames a voice has been silent and
 *               the loudest it ever was.
 * threshold is any fp32 value that is >= 0 and not NaN; the calls refuse others.  frames == 0 succeeds and writes nothing.  No 2048-frame
 * limit: the pass is element-wise over a row, like the downmix.
 * Meters are no instance state: oalsfx_batch_reset, _snapshot and _restore neither touch nor carry them (the blob's version is
 * unchanged), no effect call reads them, and nothing of them stays in the batch between calls. */
#define OALSFX_METER_LANES 64
#define OALSFX_METER_CARRY 1          /* flags bit 0 */
typedef struct {
    float    peak[OALSFX_MAX_CHANNELS];   /* per channel: largest |x| of the call; channels the format lacks: +0.0f */
    float    sumsq[OALSFX_MAX_CHANNELS];  /* per channel: sum of x*x over the call's frames, in the order above */
    float    peak_hold;                   /* largest peak[] of this call, or with CARRY of this and the earlier calls */
    uint32_t quiet_run;                   /* trailing quiet frames, or with CARRY carried over calls, saturating */
    uint32_t nonfinite;                   /* elements of the call that are NaN or +-Inf (all channels) */
    uint32_t frames;                      /* frames of the call that wrote the record */
} oalsfx_meter;                           /* 80 bytes */
/* Meters any device buffer src_dev, [rows][frames][channels] with the batch's channel count, into meters_dev[rows] (device memory or
 * page-locked host memory, 16-byte aligned).  rows >= 1 is free: n_instances for what oalsfx_batch_mix_device wrote, n_buses for what
 * oalsfx_batch_downmix_device wrote.  Asynchronous; ordering and stream semantics as for oalsfx_batch_downmix_device: it comes after every
 * call already queued on the batch; with hip_stream NULL it runs on the batch's stream and ends a run of overlapping
 * oalsfx_batch_mix_device calls, with a caller's stream it is queued there behind what the batch has in flight.  A read-only pass over
 * src_dev: it may follow a downmix of the same buffer on the same stream without an event.  src_dev needs 4-byte alignment; wider loads are
 * used where it allows, with the same bits.
 * Refusals (return 0 with a message, nothing written, the batch as it was): NULL pointers, rows < 1, frames < 0, a threshold below 0 or
 * NaN, unknown flag bits, src_dev not 4-byte or meters_dev not 16-byte aligned, meters_dev overlapping src_dev, a grid too large for one
 * launch, a batch a failed chained launch has poisoned. */
int oalsfx_batch_meter_device(oalsfx_batch* b, int rows, int frames, const float* src_dev, float threshold, int flags,
                              oalsfx_meter* meters_dev, void* hip_stream);
/* oalsfx_batch_mix_downmix plus meters of the voices (the instances' outputs, [n_instances] records, over the whole call's frames also
 * when the effects ran in 2048-frame chunks), of the buses ([n_buses] records), or both: either meter pointer may be NULL to skip that
 * meter, and with both NULL the call is exactly oalsfx_batch_mix_downmix.  The records go through device arrays the batch owns; with
 * OALSFX_METER_CARRY the caller's records are copied in first, so no state stays in the batch.  The copy out is the buses plus
 * 80 * (n_instances + n_buses) bytes, then it waits. */
int oalsfx_batch_mix_downmix_meter(oalsfx_batch* b, int frames, const float* src_host, int n_buses, float* dst_bus_host,
                                   float threshold, int flags, oalsfx_meter* voice_meters_host, oalsfx_meter* bus_meters_host);
/* The same on every shard of a group for the voices: voice_meters_host[n_total] in the global instance numbering (NULL: exactly
 * oalsfx_group_mix_downmix).  A group's buses are finished by the host, from the shards' bus buffers, so the group offers no bus meters. */
int oalsfx_group_mix_downmix_meter(oalsfx_group* g, int frames, const float* src_host, int n_buses, float* dst_bus_host,
                                   float threshold, int flags, oalsfx_meter* voice_meters_host);

/* ---- samplers: every instance plays sample data resident on the device.  Nothing in the reference's library (Api::mix is handed rendered
 * frames); what its demo program does on the host when it converts a WAV file and feeds it in (src/oalsfxpp_test.cpp:713-735), and what
 * OpenAL Soft's voices do.  A pool of thousands of voices plays a few hundred assets: the assets live in device memory once, a voice is
 * 80 bytes of playback state, and a step is render -> effects -> buses -> meters with nothing copied in.  ("Source" means the reference's
 * send properties in this ABI -- oalsfx_source_params --, hence "sampler".)  One record per instance; after oalsfx_batch_create every
 * record is all zero: not playing.  The arithmetic is part of the contract, so that the output is bit-reproducible.  For one instance and a
 * call of F frames: C is the batch's channel count, P the record's position when the call starts, E = frames << 12, L0 = loop_start << 12,
 * L1 = loop_end << 12.  Position arithmetic is exact in unsigned 64-bit integers; sample arithmetic is fp32, each operation rounded by
 * itself (no fused multiply-add), denormals not flushed, as in the downmix and the meters.
 *   not PLAYING:  every out[f][c] is +0.0f; the record is unchanged.
 *   wrap(q):      with LOOP, wrap(q) = q < L1 ? q : L0 + (q - L0) mod (L1 - L0); without LOOP, wrap(q) = q.  A position in front of
 *                 loop_start plays into the loop; a step longer than the loop wraps as often as it must.
 *   frame f:      q_f = wrap(P + f * step), i = q_f >> 12, m = q_f & 4095.
 *   past the end: without LOOP, q_f >= E: out[f][c] = +0.0f for every c.
 *   sample:       s(i, k) is element i * channels + k of the asset.  OALSFX_PCM_U8: (float)((int)v - 128) / 128.0F.  OALSFX_PCM_S16:
 *                 (float)v / 32768.0F.  OALSFX_PCM_F32: as stored; NaN, Inf and denormals pass through.
 *   neighbour:    j = i + 1; with LOOP, j == loop_end becomes loop_start; without LOOP, j == frames gives s(j, k) = +0.0f: a one-shot
 *                 interpolates into silence.
 *   value:        without LINEAR v_k = s(i, k).  With LINEAR v_k = a + ((b - a) * mu), a = s(i, k), b = s(j, k),
 *                 mu = (float)m * (1.0F / 4096.0F), which is exact: the reference's Math::lerp (src/oalsfxpp.cpp:180-186), evaluated as
 *                 written for every frame, also where m == 0 (an Inf neighbour then gives NaN).
 *   output:       out[f][c] = v_k * gain[c] for every c < C; k = c for an asset of C channels, k = 0 for a mono asset, which its gains
 *                 therefore pan.
 *   afterwards:   position = wrap(P + F * step); without LOOP a position >= E becomes E and PLAYING is cleared: the voice has finished.
 *                 Nothing else in the record changes.
 * Since wrap(wrap(x) + y) == wrap(x + y), any split of F frames into consecutive calls gives the same outputs and the same final record
 * as one call of F.
 * Samplers are state of the batch beside its instances, like the routing: oalsfx_batch_reset, _snapshot and _restore neither touch nor
 * carry them (the blob's version is unchanged), and no effect call reads them.  The caller owns the assets and keeps one alive until
 * every sampler that names it has been replaced or stopped and the batch synchronised.  A group (oalsfx_group_*) offers no samplers: an
 * asset would have to be resident on every shard's device, which is the caller's layout to decide; oalsfx_group_batch gives the shard's
 * batch to set them on. */
#define OALSFX_SAMPLER_FRAC_BITS 12
#define OALSFX_PCM_U8  0
#define OALSFX_PCM_S16 1
#define OALSFX_PCM_F32 2
#define OALSFX_SAMPLER_PLAYING 1      /* flags bit 0 */
#define OALSFX_SAMPLER_LOOP    2      /* flags bit 1 */
#define OALSFX_SAMPLER_LINEAR  4      /* flags bit 2 */
typedef struct {
    uint64_t data;        /* device address of the asset: frames * channels elements of `format`, interleaved; caller-owned */
    uint64_t position;    /* fixed point, OALSFX_SAMPLER_FRAC_BITS fractional bits: frame << 12 | fraction */
    uint32_t frames;      /* asset length in frames, 1 .. 2^31 - 1 */
    uint32_t loop_start;  /* loop region [loop_start, loop_end) in frames; read only with OALSFX_SAMPLER_LOOP */
    uint32_t loop_end;
    uint32_t step;        /* position advance per output frame, same fixed point: 4096 = the asset's own rate, 0 holds */
    uint32_t format;      /* OALSFX_PCM_U8, OALSFX_PCM_S16, OALSFX_PCM_F32 */
    uint32_t channels;    /* 1, or the batch's channel count */
    uint32_t flags;       /* OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP | OALSFX_SAMPLER_LINEAR */
    uint32_t reserved;    /* 0 */
    float    gain[OALSFX_MAX_CHANNELS];   /* per output channel */
} oalsfx_sampler;                         /* 80 bytes */
/* samplers[k] becomes the record of instances[k] (NULL: 0 .. count - 1).  Not deferred: it holds from the next render on, and is ordered
 * behind the renders already queued.  The changed records go to the device in front of the next render, and only then (a render after
 * which nothing was set uploads nothing).
 * Refusals (return 0 with a message; nothing is changed): an instance outside the batch or listed twice, unknown flags or format,
 * reserved != 0, channels other than 1 or the batch's; and for a PLAYING record data == 0, frames == 0 or >= 2^31, data not aligned to its
 * element size, with LOOP loop_start >= loop_end or loop_end > frames, position >= E or with LOOP >= L1, and an asset --
 * [data, data + frames * channels * element size) -- that does not lie inside one allocation on the batch's device: a wrong length is a
 * refusal on the host, never a read out of bounds on the device. */
int oalsfx_batch_set_samplers(oalsfx_batch* b, const int* instances, int count, const oalsfx_sampler* samplers);
/* The records as the arithmetic above leaves them after every render queued so far (waits for those): position and PLAYING are current. */
int oalsfx_batch_get_samplers(oalsfx_batch* b, const int* instances, int count, oalsfx_sampler* out);
/* Renders dst_dev, [n_instances][frames][channels], and advances the records on the device.  Any frames >= 0 (no 2048 limit: the pass is
 * element-wise over a row; frames == 0 succeeds and does nothing).  Asynchronous; ordering and stream semantics as for
 * oalsfx_batch_meter_device: it comes after every call already queued on the batch; with hip_stream NULL it runs on the batch's stream and
 * ends a run of overlapping oalsfx_batch_mix_device calls, with a caller's stream it is queued there.  Consecutive renders are ordered among
 * themselves whatever their streams.  dst_dev needs 4-byte alignment; wider stores are used where it allows, with the same bits.
 * Refusals (return 0 with a message, nothing written, records and batch as they were): a NULL or misaligned dst_dev, frames < 0 or
 * frames * channels beyond 2^32 - 1, a grid too large for one launch, a batch a failed chained launch has poisoned. */
int oalsfx_batch_sample_device(oalsfx_batch* b, int frames, float* dst_dev, void* hip_stream);
/* oalsfx_batch_mix_downmix_meter without src_host: the samplers render into the batch's own input buffer; then the effects in chunks of
 * 2048 frames, the downmix, the meters, the copy out and the wait.  Both meter pointers may be NULL. */
int oalsfx_batch_play_downmix_meter(oalsfx_batch* b, int frames, int n_buses, float* dst_bus_host, float threshold, int flags,
                                    oalsfx_meter* voice_meters_host, oalsfx_meter* bus_meters_host);

/* ---- voice envelopes: a second record per instance beside its sampler, which changes the voice smoothly inside a render: a start after
 * a delay counted in frames, a linear gain ramp per output channel, a fade that stops the voice when it completes, a linear pitch glide.
 * Nothing in the reference's library, which ramps every gain it changes (mix, src/oalsfxpp.cpp:2752-2798); what OpenAL Soft's voices do in
 * front of it, so that a stolen voice does not click and a moving one does not zipper.  One segment per record: the caller chains segments
 * (an ADSR) by setting the next one, or queues them ("envelope programs" below).  After oalsfx_batch_create every envelope is all zero: inactive.  The arithmetic is part of the
 * contract.  For one instance and one render of F frames; the sampler's record and contract are as above except where stated; R =
 * ramp_frames, G = glide_frames; integer arithmetic is exact, sample arithmetic fp32 with every operation rounded by itself:
 *   not ACTIVE:   the row is rendered by the samplers' arithmetic exactly, and the envelope is unchanged (sub is not looked at).  Rows
 *                 with and without an envelope share a launch.
 *   delay:        D = min(delay, F).  out[f][c] = +0.0f for f < D, and nothing else moves during those frames.  Afterwards delay -= D.
 *                 Sampler frame f' = f - D belongs to output frame f; F' = F - D.
 *   counters:     delay, ramp_done and glide_done advance as functions of the frames rendered alone, whether or not the sampler is
 *                 PLAYING.  A sampler that is not PLAYING writes +0.0f, never touches its asset and keeps its position and sub.
 *   gain:         frame f' has the ramp index n = ramp_done + f' and the factor e_c = gain_from[c] + ((float)n * gain_step[c]) for
 *                 n < R -- (float)n is exact; product and sum rounded separately, no fused multiply-add, no running sum --, e_c =
 *                 gain_to[c] for n >= R.  out[f][c] = (v_k * gain[c]) * e_c: the sampler's product first.  A frame past a one-shot's
 *                 end stays +0.0f whatever the sign of e_c.  Afterwards ramp_done = min(R, ramp_done + F').
 *   STOP:         frames with n >= R are +0.0f, and the sampler advances only over the F'' = min(F', R - ramp_done) frames in front of
 *                 them (without STOP, F'' = F').  When ramp_done == R after the render, PLAYING is cleared in the sampler's record.
 *                 With R == 0 the voice stops at once, silently.
 *   positions:    16 more fractional bits: PHI = (position << 16) | sub.  The fine step at glide index g is S_g = (step << 16) +
 *                 g * glide_slope for g < G and S_g = step_to << 16 for g >= G; without GLIDE, S_g = step << 16 for every g, and sub stays
 *                 what the caller set (0 unless they did).  Frame f' has the glide index glide_done + f' and reads at PHI_f' =
 *                 wrapF(PHI_0 + sum of S_(glide_done + j) over j < f'), in closed form m * S_g0 + glide_slope * m * (m - 1) / 2 +
 *                 (f' - m) * (step_to << 16) with g0 = glide_done, m = min(f', G - g0).  wrapF is wrap with L0, L1 and E shifted left by
 *                 16 as well.  q_f = PHI_f' >> 16; i, m, the neighbour, the value and a one-shot's end are the samplers'.
 *   afterwards:   PHI_end = wrapF(PHI_0 + the sum over the F'' frames advanced): position = PHI_end >> 16, sub = PHI_end & 65535; a
 *                 one-shot that has reached E gets position = E, sub = 0 and stops as before.  With GLIDE glide_done = min(G, glide_done
 *                 + F''), and once glide_done == G the sampler's step becomes step_to (also in a record that is not PLAYING).
 * Any split of F frames into consecutive renders gives the same outputs and the same two final records as one render of F.
 * No overflow: with GLIDE, step and step_to lie below 2^20 and S_G = (step << 16) + G * glide_slope in [0, 2^36), so every S_g does;
 * PHI < 2^59, a render has at most 2^24 frames, and every sum above stays below 2^63 (without GLIDE the kernel never
 * forms more than one tile's advance beyond a wrapped position).  The bounds are refusals on the host; the device clamps nothing.
 * Envelopes are state of the batch beside its instances, like routing and samplers: oalsfx_batch_reset, _snapshot and _restore neither
 * touch nor carry envelopes (the blob's version is unchanged), no effect call reads them, and a group (oalsfx_group_*) offers no
 * envelopes: oalsfx_group_batch gives the shard's batch to set them on. */
#define OALSFX_ENV_ACTIVE 1   /* flags bit 0: the envelope takes part in renders */
#define OALSFX_ENV_STOP   2   /* flags bit 1: when the gain ramp completes the voice stops */
#define OALSFX_ENV_GLIDE  4   /* flags bit 2: the pitch glide fields are in use */
#define OALSFX_ENV_SUB_BITS 16
typedef struct {
    uint32_t flags;         /* OALSFX_ENV_ACTIVE | OALSFX_ENV_STOP | OALSFX_ENV_GLIDE */
    uint32_t delay;         /* frames of silence still to come before the voice runs */
    uint32_t ramp_frames;   /* R, 0 .. 2^24 */
    uint32_t ramp_done;     /* n, 0 .. R */
    float    gain_from[OALSFX_MAX_CHANNELS];
    float    gain_step[OALSFX_MAX_CHANNELS];   /* per frame */
    float    gain_to[OALSFX_MAX_CHANNELS];
    uint32_t glide_frames;  /* G, 0 .. 2^20 */
    uint32_t glide_done;    /* g, 0 .. G */
    int32_t  glide_slope;   /* change of the fine step per frame */
    uint32_t step_to;       /* the sampler's step once the glide completes */
    uint32_t sub;           /* low 16 bits of the fine position, 0 .. 65535 */
    uint32_t reserved[3];   /* 0 */
} oalsfx_envelope;          /* 144 bytes */
/* envelopes[k] becomes the envelope of instances[k] (NULL: 0 .. count - 1).  Not deferred: it holds from the next render on, and is ordered
 * behind the renders already queued.  The changed records go to the device in front of the next render, and only then.  A record with
 * GLIDE is checked against the step of the instance's sampler as the renders queued so far leave it (the call waits for them where an
 * earlier glide may have changed a step), so set the sampler first.
 * Refusals (return 0 with a message; nothing is changed): unknown flags, reserved != 0, an instance outside the batch or listed twice,
 * ramp_frames > 2^24, ramp_done > ramp_frames, sub > 65535; and with GLIDE glide_frames > 2^20, glide_done > glide_frames, step_to >=
 * 2^20, a sampler step >= 2^20 ("The gliding sampler's step is out of range."), (step << 16) + glide_frames * glide_slope outside
 * [0, 2^36) ("The glide leaves the range of steps.").  With the last two messages oalsfx_batch_set_samplers refuses a record that would
 * give an instance whose envelope has GLIDE such a step.  While any envelope of a batch is ACTIVE, a render of more than 2^24 frames is
 * refused. */
int oalsfx_batch_set_envelopes(oalsfx_batch* b, const int* instances, int count, const oalsfx_envelope* envelopes);
/* The envelopes as the arithmetic above leaves them after every render queued so far (waits for those).  oalsfx_batch_get_samplers
 * returns step, position and PLAYING as the envelopes left them. */
int oalsfx_batch_get_envelopes(oalsfx_batch* b, const int* instances, int count, oalsfx_envelope* out);

/* ---- resamplers: a voice interpolates its asset through a 4- or 8-tap FIR whose coefficients come from a phase table, instead of taking
 * the nearest sample or interpolating linearly.  Nothing in the reference's library; what OpenAL Soft's cubic and band-limited resamplers
 * do in front of it.  A third piece of state beside each instance: a table index, or OALSFX_RESAMPLER_NONE (the state after
 * oalsfx_batch_create).  A batch owns up to OALSFX_FIR_TABLES coefficient tables; table t has T taps, T 4 or 8, and P = 1 << phase_bits
 * phases, 0 <= phase_bits <= OALSFX_SAMPLER_FRAC_BITS, and holds coef[P][T] fp32, every coefficient finite.
 *   without a table: the instance's sampler and envelope are exactly what they are above, bit for bit.
 *   with a table:    only the value of a frame changes.  Positions, wrapping, a one-shot's end, PLAYING, delay, ramp, STOP, glide, sub and
 *                    both records afterwards are the contracts above word for word.  The sampler's LINEAR flag is not looked at.
 *   the value:       q is the frame's wrapped 12-bit position (q_f = PHI_f' >> 16 under an envelope), i = q >> 12, phase = (q & 4095) >>
 *                    (12 - phase_bits), H = T / 2.  Tap k = 0 .. T - 1 reads frame j_k = i - (H - 1) + k, a signed number, and x_k is
 *                      j_k < 0:                              +0.0f;
 *                      without LOOP and j_k >= frames:       +0.0f: the one-shot rings into silence, as the linear one interpolates into it;
 *                      with LOOP and j_k >= loop_end:        the frame loop_start + (j_k - loop_end) mod (loop_end - loop_start) (the loop
 *                                                            may be shorter than H);
 *                      anything else:                        the asset's frame j_k, converted as above.  That includes j_k below
 *                                                            loop_start in a looping voice: the lead-in is read where it lies, because
 *                                                            the value must stay a function of the position alone.
 *                    v = (((+0.0f + c_0 * x_0) + c_1 * x_1) + ...) + c_(T-1) * x_(T-1), c = coef[phase], ascending k, every product and
 *                    every sum rounded by itself, no fused multiply-add.  out[f][c] = (v * gain[c]) * e_c as above.  A mono asset
 *                    computes v once.
 * An in-range tap is always multiplied, even by a zero coefficient, so that 0 * Inf is NaN like everywhere else in this library.  An
 * out-of-range tap may be multiplied or left out: with finite coefficients a sum that starts at +0.0f never becomes -0.0f, so both give
 * the same bits -- which is why non-finite coefficients are refused.  Because v depends on q alone, every split of a stretch of frames
 * into renders gives the same bits and the same records, as for samplers and envelopes.  The device forms no address outside [data,
 * data + frames * channels * element size): an out-of-range tap is never loaded.
 * Resamplers and tables are state of the batch beside its instances, like routing, samplers and envelopes: oalsfx_batch_reset, _snapshot
 * and _restore neither touch nor carry them (the blob's version is unchanged), and a group (oalsfx_group_*) offers none:
 * oalsfx_group_batch gives the shard's batch to set them on. */
#define OALSFX_FIR_TABLES 8
#define OALSFX_RESAMPLER_NONE (-1)
/* Table `table` becomes coef_host[P][taps], which the library copies.  A set-up call, not a hot one: it waits for the renders queued so
 * far, then puts the table on the device.  taps == 0 with coef_host NULL clears the slot.  Replacing the coefficients of a table of the
 * same shape is allowed while instances name it; the next render reads the new ones.
 * Refusals (return 0 with a message; nothing is changed): "FIR table index out of range.", "Unknown FIR tap count.", "FIR phase bits out
 * of range.", "Null FIR coefficients.", "Non-finite FIR coefficient."; clearing or re-shaping a slot an instance still names: "The FIR
 * table is still named by an instance.". */
int oalsfx_batch_set_fir_table(oalsfx_batch* b, int table, int taps, int phase_bits, const float* coef_host);
/* The shape of table `table`: *taps 0 (and *phase_bits 0) for an empty slot.  Either pointer may be NULL. */
int oalsfx_batch_get_fir_table(const oalsfx_batch* b, int table, int* taps, int* phase_bits);
/* tables[k] becomes the resampler of instances[k] (NULL: 0 .. count - 1).  Not deferred: it holds from the next render on.  The changed
 * indices go to the device in front of the next render, and only then.
 * Refusals (return 0 with a message; every instance stays as it was): an instance outside the batch or listed twice, "Unknown
 * resampler." (below -1 or >= OALSFX_FIR_TABLES), "The resampler names a table that has not been set.". */
int oalsfx_batch_set_resamplers(oalsfx_batch* b, const int* instances, int count, const int* tables);
int oalsfx_batch_get_resamplers(oalsfx_batch* b, const int* instances, int count, int* tables);

/* ---- polyphony: several voices per instance, summed on the device.  A batch has a polyphony K, 1 <= K <= OALSFX_MAX_POLYPHONY (the
 * state after oalsfx_batch_create: 1).  Every instance has K lanes, and every lane is a full voice: a sampler's record, an envelope and a
 * resampler, under the three contracts above exactly as they stand.  Lane 0 is the voice the calls above address.  A render
 * (oalsfx_batch_sample_device, oalsfx_batch_play_downmix_meter) sums the K voices of an instance into that instance's input.
 *   K == 1:  everything is as stated above, bit for bit, and the batch launches exactly what it launched before.
 *   K >= 2:  for instance i, frame f, channel c
 *                in[f][c] = (((+0.0f + o_0) + o_1) + ...) + o_(K-1)
 *            where o_k is the value the contracts above give the voice (lane k, instance i) by itself for that frame: (v * gain[c]) * e_c,
 *            or v * gain[c] without an active envelope.  Lanes are summed ascending, every addition is rounded by itself, and the voice's
 *            last product is not fused into the sum.
 * A frame that is +0.0f by the voice's own contract (not PLAYING, inside delay, behind a completed STOP, past a one-shot's end) may be
 * added or left out: both give the same bits, by the argument the resamplers use for out-of-range taps.  The sum starts at +0.0f; a
 * running sum in round-to-nearest is never -0.0f ((+0) + (-0) = +0, and an exact zero result of non-zero terms is +0); and x + (+0.0f) = x
 * for every other x, Inf and NaN included.  With K >= 2 a lone voice's -0.0f therefore reaches the input as +0.0f: that is part of the
 * contract, and the reason K == 1 keeps its own path.
 * Every voice's records advance by their own contracts, independently of the other lanes, and a frame's sum depends on the voices'
 * positions alone: any split of F frames into consecutive renders gives the same outputs and the same 3 * K records as one render of F.
 * The FIR tables are the batch's and are shared by all lanes; "The FIR table is still named by an instance.", the 2^24-frame rule of the
 * envelopes and the choice of kernel at K == 1 count the voices of every lane.  An envelope with GLIDE is checked against the sampler
 * of the same lane and instance.
 * Polyphony is state of the batch beside its instances, like routing: oalsfx_batch_reset, _snapshot and _restore neither touch nor
 * carry it, and a group (oalsfx_group_*) offers none. */
#define OALSFX_MAX_POLYPHONY 16
/* The batch gets `lanes` lanes.  A set-up call, like oalsfx_batch_set_fir_table: it waits for the renders queued so far, reads the records
 * back and gives the three record tables instances * lanes rows, lane-major: voice row = lane * instances + instance, so lane 0's rows
 * are the rows of K == 1 and growing K appends.  New lanes are in the state after creation (an all-zero sampler, an all-zero envelope,
 * OALSFX_RESAMPLER_NONE); kept lanes keep their records, positions in mid-asset included.  Setting the value the batch already has does
 * nothing.
 * Refusals (return 0 with a message; nothing is changed): "Polyphony out of range."; "A lane that would be dropped is still in use." (a
 * dropped lane holds a PLAYING sampler, an ACTIVE envelope or a table index); a poisoned batch. */
int oalsfx_batch_set_polyphony(oalsfx_batch* b, int lanes);
int oalsfx_batch_get_polyphony(const oalsfx_batch* b);
/* The six calls above for the voices of lane `lane`; those are the lane-0 forms of these, with every refusal and message word for word.
 * In addition: "Lane out of range." for a lane outside [0, K).  An instance may be listed once per call.  The rows set since the last
 * render, of whatever lane, go to the device in one launch per table in front of the next render. */
int oalsfx_batch_set_lane_samplers(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_sampler* samplers);
int oalsfx_batch_get_lane_samplers(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_sampler* out);
int oalsfx_batch_set_lane_envelopes(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_envelope* envelopes);
int oalsfx_batch_get_lane_envelopes(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_envelope* out);
int oalsfx_batch_set_lane_resamplers(oalsfx_batch* b, int lane, const int* instances, int count, const int* tables);
int oalsfx_batch_get_lane_resamplers(oalsfx_batch* b, int lane, const int* instances, int count, int* tables);

/* ---- voice filters: a biquad per voice, run on the device before the sum.  Nothing in the reference's library filters one voice by
 * itself (its two send shelves, oalsfx_source_params, see an instance's whole input); the arithmetic is its FilterState::process
 * (src/oalsfxpp.cpp:984-1036), and in OpenAL this is the per-source direct filter: a sound occluded behind a wall, the highs of a distant
 * one rolled off, a low-pass swept on one note.  A fourth record per voice beside sampler, envelope and resampler.  After
 * oalsfx_batch_create every record is all zero: no filter.  For a voice whose filter is ACTIVE, channel c below the batch's channel
 * count, and frame f of a render of F frames:
 *   input:      x_f is the value the contracts above give that voice for that frame, by itself: (v * gain[c]) * e_c, or v * gain[c]
 *               without an active envelope; +0.0f wherever those contracts say the voice is silent (not PLAYING, inside its delay, behind
 *               a completed STOP, past a one-shot's end).  The filter runs over every frame of the render, silent ones included: a
 *               stopped voice rings out.
 *   output:     y_f = ((((b0 * x_f) + (b1 * x_(f-1))) + (b2 * x_(f-2))) - (a1 * y_(f-1))) - (a2 * y_(f-2)), every product, sum and
 *               difference rounded by itself, nothing fused.  x_(-1), x_(-2), y_(-1) and y_(-2) are the record's histories.
 *   afterwards: the histories hold frames F - 1 and F - 2 (F == 1 shifts them, F == 0 leaves them); channels at and above the channel
 *               count are never touched.  A render of F frames and any split of it into consecutive renders give the same outputs and
 *               the same records.
 *   K == 1:     in[f][c] = y_f, stored as it is: a -0.0f stays negative.
 *   K >= 2:     y_f stands where o_k stood in the polyphony sum: lanes summed ascending from +0.0f, every addition rounded by itself.
 * A voice whose filter is not ACTIVE contributes exactly what it contributes without this section, and its filter record is not read
 * past its flags; a batch in which no filter is ACTIVE launches exactly what it launched before.  A voice is busy when it is PLAYING,
 * has an ACTIVE envelope or has an ACTIVE filter: the caller clears ACTIVE when the meters say the tail has died.  The device does not
 * do that, clamps nothing and flushes no denormals; stability is not checked either, and a filter that blows up shows in the meters'
 * non-finite count.
 * Filters are state of the batch beside its instances, like samplers: oalsfx_batch_reset, _snapshot and _restore neither touch nor carry
 * them, and a group (oalsfx_group_*) offers none.  oalsfx_batch_set_polyphony carries the fourth table like the other three (new lanes
 * all zero, kept lanes kept), and "A lane that would be dropped is still in use." also covers a dropped lane with an ACTIVE filter. */
#define OALSFX_VF_ACTIVE 1   /* flags bit 0: the filter takes part in renders */
#define OALSFX_VF_LOAD   2   /* flags bit 1, set calls only: the record's x and y replace the device's histories */
#define OALSFX_VF_LOW_PASS   0   /* kinds of oalsfx_host_voice_filter */
#define OALSFX_VF_HIGH_PASS  1
#define OALSFX_VF_BAND_PASS  2
#define OALSFX_VF_LOW_SHELF  3
#define OALSFX_VF_HIGH_SHELF 4
#define OALSFX_VF_PEAKING    5
typedef struct {
    uint32_t flags;        /* OALSFX_VF_ACTIVE | OALSFX_VF_LOAD; other bits refused */
    uint32_t reserved0;    /* 0 */
    float b0, b1, b2, a1, a2;   /* divided by a0, as FilterState::set_params leaves them */
    float reserved1;       /* 0 */
    float x[OALSFX_MAX_CHANNELS][2];   /* x[c][0] the last input of channel c, x[c][1] the one before */
    float y[OALSFX_MAX_CHANNELS][2];   /* the same for the output */
} oalsfx_voice_filter;     /* 160 bytes */
/* filters[k] becomes the filter of instances[k] (NULL: 0 .. count - 1), lane 0.  Not deferred: it holds from the next render on, at a
 * render boundary, and is ordered behind the renders already queued.  A set call always replaces flags and coefficients.  With LOAD the
 * record's x and y replace the device's histories in front of the next render: a voice started clean, or restored.  Without LOAD the
 * device's histories are kept: a coefficient change on a sounding voice.  LOAD is consumed by the upload: neither the device's copy nor a
 * later get shows it.  A row set with LOAD may be set again without it before any render: it keeps the pending histories and LOAD and
 * takes the new coefficients.  The changed rows, of whatever lane, go to the device in one launch in front of the next render.
 * Refusals (return 0 with a message; nothing is changed): "Unknown voice filter flags.", "The voice filter's reserved fields are not 0.",
 * "Non-finite voice filter coefficient.", "Non-finite voice filter history."; an instance outside the batch or listed twice ("An instance
 * is listed twice as a voice filter target."), "Lane out of range."; a poisoned batch. */
int oalsfx_batch_set_filters(oalsfx_batch* b, const int* instances, int count, const oalsfx_voice_filter* filters);
/* The coefficients as set and the histories as every render queued so far leaves them (waits for those); the host's row where one was
 * set since. */
int oalsfx_batch_get_filters(oalsfx_batch* b, const int* instances, int count, oalsfx_voice_filter* out);
int oalsfx_batch_set_lane_filters(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_voice_filter* filters);
int oalsfx_batch_get_lane_filters(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_voice_filter* out);

/* ---- voice filter sweeps: a voice filter's five coefficients ramp per frame, on the device, so that a low-pass swept on one note, an
 * occlusion that opens or a wah moves every frame and not in steps on the caller's buffer grid.  A sixth record per voice (lane,
 * instance), all zero after oalsfx_batch_create: no sweep.  The ramp is linear in the COEFFICIENTS, not in a corner frequency or a gain:
 * a long sweep across octaves is better made of several.  The arithmetic is part of the contract.  For a voice whose filter is
 * OALSFX_VF_ACTIVE and whose sweep is OALSFX_SWEEP_ACTIVE with done < frames (R below), and a render of F frames:
 *   coefficients: frame f has the index n = done + f.  Coefficient k (order b0, b1, b2, a1, a2) of that frame is
 *               from[k] + ((float)n * step[k]) for n < R and to[k] for n >= R.  (float)n is exact (R <= 2^24); the product and the sum are
 *               each rounded by themselves; there is no fused multiply-add and no running sum: the rules of the envelopes' ramps.
 *   output:     y_f = ((((b0_f * x_f) + (b1_f * x_(f-1))) + (b2_f * x_(f-2))) - (a1_f * y_(f-1))) - (a2_f * y_(f-2)), all five
 *               coefficients frame f's.  Everything else is the voice filters' contract word for word: the input, the silent frames, the
 *               histories, K == 1 stored as it is, K >= 2 summed in ascending lanes.
 *   afterwards: done = min(R, done + F).  In the render in which done reaches R the device writes `to` into b0 .. a2 of the voice's filter
 *               record and clears the sweep's ACTIVE: from then on the voice is a plain filtered voice, and oalsfx_batch_get_filters
 *               returns `to`.  Until then the filter record's coefficients stay what they were set to and are not looked at.
 *   splits:     any split of F frames into consecutive renders gives the same outputs and the same filter and sweep records.
 * A voice without an ACTIVE sweep (or with done == frames) contributes exactly the bits it contributes without this section, in the same
 * launch.  While no sweep can be under way the batch launches exactly what it launched before: it knows that without reading anything
 * back, from the frames every sweep had left when it was set and the frames rendered since (it may err on the late side).
 * Stability: the region of (a1, a2) in which a biquad is stable is a triangle and therefore convex, so a line between two stable designs
 * stays stable, up to the rounding of the formula above.  As before, the device checks nothing.
 * Sweeps are state of the batch beside its instances, like filters: oalsfx_batch_reset, _snapshot and _restore neither touch nor carry
 * them, and a group (oalsfx_group_*) offers none.  oalsfx_batch_set_polyphony carries the sixth table like the others (a dropped lane
 * with a sweep is refused through its ACTIVE filter). */
#define OALSFX_SWEEP_ACTIVE 1   /* flags bit 0: the sweep takes part in renders */
#define OALSFX_SWEEP_MAX_FRAMES (1u << 24)
typedef struct {
    uint32_t flags;      /* OALSFX_SWEEP_ACTIVE; other bits refused */
    uint32_t frames;     /* R, 1 .. 2^24 */
    uint32_t done;       /* n, 0 .. R */
    uint32_t reserved;   /* 0 */
    float from[5], step[5], to[5];   /* order b0, b1, b2, a1, a2 */
    float reserved1;     /* 0 */
} oalsfx_filter_sweep;   /* 80 bytes */
/* sweeps[k] becomes the sweep of instances[k] (NULL: 0 .. count - 1), lane 0.  Not deferred, ordered and uploaded as
 * oalsfx_batch_set_filters is: the changed rows, of whatever lane, go to the device in one launch in front of the next render.  A record
 * without ACTIVE cancels the voice's sweep.  oalsfx_batch_set_filters and _set_lane_filters keep their contract and also cancel the
 * voice's sweep: a plain set is a sweep of none.  Set the filter first (ACTIVE, with LOAD for a voice started clean), then its sweep.
 * Refusals (return 0 with a message; nothing is changed): "Unknown filter sweep flags.", "The filter sweep's reserved fields are not 0.",
 * "The filter sweep's frame count is out of range." (outside 1 .. 2^24; a record without ACTIVE may have 0), "The filter sweep is past
 * its end." (done > frames), "Non-finite filter sweep coefficient.", "The swept voice's filter is not active." (for an ACTIVE sweep);
 * "Lane out of range."; an instance outside the batch or listed twice ("An instance is listed twice as a filter sweep target."); a
 * poisoned batch. */
int oalsfx_batch_set_sweeps(oalsfx_batch* b, const int* instances, int count, const oalsfx_filter_sweep* sweeps);
/* The sweeps as every render queued so far leaves them (waits for those); the host's row where one was set since. */
int oalsfx_batch_get_sweeps(oalsfx_batch* b, const int* instances, int count, oalsfx_filter_sweep* out);
int oalsfx_batch_set_lane_sweeps(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_filter_sweep* sweeps);
int oalsfx_batch_get_lane_sweeps(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_filter_sweep* out);

/* ---- envelope programs: a voice's queued envelope segments take their turn on the device, inside a render, at the exact frame.  A voice
 * (lane, instance) has its envelope record as above, the current segment, and behind it a queue of up to OALSFX_ENV_PROGRAM_MAX - 1 further
 * oalsfx_envelope records: delay, attack, hold, decay, sustain, release and two spare.  After oalsfx_batch_create every queue is empty.
 * The arithmetic is part of the contract.
 *   complete:   a current segment is complete when it is ACTIVE, delay == 0 and ramp_done == ramp_frames.
 *   a render of F frames, for one voice, with t = 0:
 *     1. While the queue is not empty and the current segment is complete, the head of the queue becomes the current segment: copied
 *        whole, counters as they were set, and the queue shortens by one.  Several zero-length segments go in a row.  This check also
 *        runs at t == F: a segment that completes on a render's last frame is replaced in that render.
 *     2. If t == F, stop.
 *     3. The span is s = F - t when the queue is empty, otherwise s = min(F - t, delay + (ramp_frames - ramp_done)).
 *     4. Frames [t, t + s) are rendered, and both records advanced, exactly as the contracts above render a call of s frames for this
 *        voice -- samplers, envelopes and resamplers: delay, ramp, STOP, a one-shot's end, position and sub.  Then t += s, and go to 1.
 * The voice's output over [0, F) is the concatenation of its spans.  Every frame has the bits a caller would have got by splitting the
 * render at each boundary and calling oalsfx_batch_set_lane_envelopes with the next segment there.  Any split of F frames into renders
 * gives the same outputs, the same two records and the same queue as one render of F.  With an empty queue, everything is the contracts
 * above word for word.  Polyphony sums the voices' concatenated outputs as it does without programs (K == 1: stored as they are, a -0.0f
 * stays negative), and a voice filter runs over the whole row as it does without them.  A STOP segment that completes clears PLAYING as
 * before; later segments still take their turn and run their counters on the stopped voice.
 * Segments of a program of two or more are ACTIVE and do not GLIDE: a timed pitch program needs the chain of steps checked on the host
 * and is not offered.  A program of one is oalsfx_batch_set_envelopes exactly, GLIDE included.
 * Programs are state of the batch beside its instances, like envelopes: oalsfx_batch_reset, _snapshot and _restore neither touch nor carry
 * them, and a group (oalsfx_group_*) offers none.  oalsfx_batch_set_polyphony carries the queues like the other four tables (new lanes
 * empty, kept lanes kept); a dropped lane with a queue is refused through its ACTIVE envelope.  A batch none of whose queues can hold a
 * segment launches exactly what it launched before: the batch knows that without reading anything back, from the frames every program
 * had left when it was set and the frames rendered since (it may err on the late side). */
#define OALSFX_ENV_PROGRAM_MAX 8
/* segments[k][0 .. lengths[k] - 1] becomes the program of instances[k] (NULL: 0 .. count - 1), lane 0: segment 0 the current envelope, the
 * rest the queue; the whole program is replaced.  segments is [count][OALSFX_ENV_PROGRAM_MAX]; entries past the length are not read.  Not
 * deferred, ordered and uploaded as oalsfx_batch_set_envelopes is: the changed rows go to the device in front of the next render, and only
 * then.  oalsfx_batch_set_envelopes and _set_lane_envelopes keep their contract and also empty the voice's queue: a plain set is a
 * program of one.
 * Refusals (return 0 with a message; nothing is changed): every refusal of oalsfx_batch_set_envelopes, for every segment; "Envelope
 * program length out of range." (outside 1 .. OALSFX_ENV_PROGRAM_MAX); for a length of two or more "A program's segment is not active."
 * and "A program's segment glides."; "Lane out of range."; an instance outside the batch or listed twice; a poisoned batch. */
int oalsfx_batch_set_env_programs(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_envelope* segments);
/* lengths[k] = 1 + the segments queued, and out[k][0 .. lengths[k] - 1] the segments, the current one first, as every render queued so far
 * leaves them (waits for those); entries past the length are not written.  oalsfx_batch_get_envelopes keeps returning the current
 * segment.  Not a hot call: the first get behind a render that walked the queues copies the whole queue table back, a kilobyte per
 * voice of the batch, however few instances are asked for; further gets, and gets behind renders that no longer walk the queues, copy
 * nothing. */
int oalsfx_batch_get_env_programs(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_envelope* out);
int oalsfx_batch_set_lane_env_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_envelope* segments);
int oalsfx_batch_get_lane_env_programs(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_envelope* out);

/* ---- filter programs: a voice filter's queued sweeps take their turn on the device, inside a render, at the exact frame: a filter
 * envelope (attack, decay, sustain, release of a cutoff), a wah that goes up and comes back, a sweep across octaves made of several
 * linear pieces.  A voice (lane, instance) has its oalsfx_filter_sweep record as above, the current segment, and behind it a queue of up
 * to OALSFX_FILTER_PROGRAM_MAX - 1 further oalsfx_filter_sweep records.  After oalsfx_batch_create every queue is empty.  The arithmetic
 * is part of the contract.
 *   spent:      a current segment is spent when it is not under way: not OALSFX_SWEEP_ACTIVE, or done == frames.
 *   a render of F frames, for one voice whose filter is OALSFX_VF_ACTIVE, with t = 0:
 *     1. While the queue is not empty and the current segment is spent, the head of the queue becomes the current segment: copied whole,
 *        and the queue shortens by one.  This check also runs at t == F: a segment that completes on a render's last frame is replaced
 *        in that render, and the new one has done == 0.
 *     2. If t == F, stop.
 *     3. The span is s = F - t when the queue is empty, otherwise s = min(F - t, frames - done).
 *     4. Frames [t, t + s) are filtered exactly as "voice filter sweeps" filters a render of s frames for this voice: coefficient k of
 *        index n is from[k] + ((float)n * step[k]), the product and the sum each rounded by itself; the histories carry over; done
 *        advances; a sweep that reaches its length writes `to` into the filter record and clears its ACTIVE.  Then t += s, and go to 1.
 * Every frame has the bits a caller would have got by splitting the render at each boundary and calling oalsfx_batch_set_lane_sweeps with
 * the next segment there.  Any split of F frames into renders gives the same outputs and the same filter record, sweep record and queue
 * as one render of F.  After a render that ends inside segment k >= 1 the filter record's coefficients are `to` of segment k - 1; after
 * the last segment completes they are its `to`, and the sweep is not ACTIVE.  The first frame of a new segment takes its `from` (index
 * 0): continuity between `to` of one segment and `from` of the next is the caller's business, and oalsfx_host_filter_program and
 * oalsfx_host_filter_sweep_log provide it.  With an empty queue, everything is "voice filter sweeps" word for word.  The voice's input
 * row (sampler, envelope or envelope program, resampler) is rendered as before: only the filter stage looks at the queue.
 * Filter programs are state of the batch beside its instances, like sweeps: oalsfx_batch_reset, _snapshot and _restore neither touch nor
 * carry them, and a group (oalsfx_group_*) offers none.  oalsfx_batch_set_polyphony carries the queues like the other tables (new lanes
 * empty, kept lanes kept; a dropped lane with a queue is refused through its ACTIVE filter).  A batch none of whose queues can hold a
 * segment launches exactly what it launched before: the batch knows that without reading anything back, from the frames every program
 * had in front of its last segment when it was set and the frames rendered since (it may err on the late side). */
#define OALSFX_FILTER_PROGRAM_MAX 8
/* segments[k][0 .. lengths[k] - 1] becomes the filter program of instances[k] (NULL: 0 .. count - 1), lane 0: segment 0 the current sweep,
 * the rest the queue; the whole program is replaced.  segments is [count][OALSFX_FILTER_PROGRAM_MAX]; entries past the length are not
 * read.  A length of 1 is oalsfx_batch_set_lane_sweeps exactly.  Not deferred, ordered and uploaded as oalsfx_batch_set_sweeps is: the
 * changed rows of all lanes go to the device in one launch in front of the next render, and only then.  oalsfx_batch_set_sweeps,
 * _set_lane_sweeps, _set_filters and _set_lane_filters keep their contracts and also empty the voice's queue.
 * Refusals (return 0 with a message; nothing is changed): every refusal of oalsfx_batch_set_sweeps, for every segment; "Filter program
 * length out of range." (outside 1 .. OALSFX_FILTER_PROGRAM_MAX); for a length of two or more "A filter program's segment is not
 * active." and, for a segment behind the first with done != 0, "A queued filter sweep has already started."; "The swept voice's filter
 * is not active."; "Lane out of range."; an instance outside the batch or listed twice ("An instance is listed twice as a filter
 * program target."); a poisoned batch. */
int oalsfx_batch_set_filter_programs(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_filter_sweep* segments);
/* lengths[k] = 1 + the segments queued, and out[k][0 .. lengths[k] - 1] the segments, the current one first, as every render queued so far
 * leaves them (waits for those); entries past the length are not written.  oalsfx_batch_get_sweeps keeps returning the current segment.
 * Like oalsfx_batch_get_env_programs: the first get behind a render that walked the queues copies the whole queue table back, 576 bytes
 * per voice of the batch; further gets, and gets behind renders that no longer walk the queues, copy nothing. */
int oalsfx_batch_get_filter_programs(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_filter_sweep* out);
int oalsfx_batch_set_lane_filter_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_filter_sweep* segments);
int oalsfx_batch_get_lane_filter_programs(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_filter_sweep* out);

/* ---- sampler streams: a voice's queued sampler records take their turn on the device, inside a render, at the exact frame, and more may
 * be appended while the voice plays: music, dialogue, voice chat, anything decoded piecewise or too long to be resident as a whole.  What
 * OpenAL's buffer queue on a source does.  A voice (lane, instance) has its oalsfx_sampler record as above, the current entry; behind it a
 * ring of up to OALSFX_STREAM_QUEUE further oalsfx_sampler records; and a count `taken` of the entries taken since the stream was last
 * set.  After oalsfx_batch_create every ring is empty and taken is 0.  The arithmetic is part of the contract.  E = frames << 12 of the
 * current record.
 *   at its end: the current record is at its end when it has no LOOP and position >= E, whether or not it is PLAYING.  An all-zero record
 *               is at its end, so appending to an idle voice starts it.
 *   a render of F frames, for one voice, with t = 0 and over = 0:
 *     1. While the ring is not empty and the current record is at its end, the ring's head becomes the current record: copied whole --
 *        data, frames, loop, step, format, channels, flags, gains --, at position wrap(entry.position + over) with the entry's own wrap;
 *        taken goes up by one and the ring shortens by one.  If that start is at or past the new one-shot's end E', the record is left
 *        as the samplers leave one that has finished (position = E', PLAYING cleared), over becomes the start less E', and the check
 *        runs again: chains of takes are bounded by the ring.  Otherwise over = 0.  This check also runs at t == F: a record that
 *        reaches its end with a render's last frame is replaced in that render, with its over.
 *     2. If t == F, stop.
 *     3. The span is s = F - t, cut to delay + n where the ring is not empty and the record is PLAYING without LOOP at a step other than
 *        0: n = ceil((E - position) / step) is the first of the sampler's frames that would read at q >= E, `delay` the envelope's where
 *        it is ACTIVE.  (An envelope program's queue cuts spans as well, as "envelope programs" says; where the cuts fall is observable
 *        through the takes alone.)
 *     4. Frames [t, t + s) are rendered, and the records advanced, exactly as the contracts above render a call of s frames for this
 *        voice: sampler, envelope or envelope program, resampler.  If the record has reached its end in this span, over = position + n *
 *        step - E with the position in front of the span, the excess of the frame that would have read past the end; otherwise over = 0.
 *        Then t += s, and go to 1.
 * So the first frame at which a PLAYING one-shot would read at q >= E is frame 0 of the ring's head instead, which starts `over` further
 * in.  With the ring empty the end is the samplers' contract word for word: position = E and PLAYING cleared.  A record that was at its
 * end when the render began (the ring ran dry earlier) is replaced with over = 0.  Every frame has the bits a caller would have got by
 * splitting the render at each take and calling oalsfx_batch_set_lane_samplers there with the entry, its position advanced by over.
 *   envelope:   the envelope runs on across a take untouched: delay, ramp and STOP; sub is what the span in front of the take left (0
 *               where an ACTIVE envelope saw the one-shot end).  A completed STOP keeps the voice silent as it does without a stream.  An
 *               entry that never ends (LOOP, or step 0) holds the entries behind it until the caller replaces the stream: an intro and
 *               its loop are two entries.
 *   seam:       each span interpolates as the samplers' contract says: into silence at a one-shot's last frame and out of nothing in
 *               front of frame 0, with LINEAR and with a FIR table alike.  Nothing interpolates across the seam: a stream of chunks
 *               played with LINEAR or through a table differs from the whole asset in the frames that read across a cut.
 *   invariance: any split of F frames into renders gives the same outputs, records, taken counts and rings as one render of F, provided
 *               the appends fall at the same frames.
 *   chunks:     with nearest-sample playback (no LINEAR, no table) a stream of consecutive chunks of an asset, of equal step and gains
 *               and with every queued position 0, plays the whole asset's bits at any step and any start: q_j = P + j * step is carried
 *               across the cuts exactly.
 * Streams are state of the batch beside its instances, like samplers: oalsfx_batch_reset, _snapshot and _restore neither touch nor carry
 * them, and a group (oalsfx_group_*) offers none.  oalsfx_batch_set_polyphony carries the rings like the other tables (new lanes empty,
 * kept lanes kept); a dropped lane whose ring holds an entry is refused ("A lane that would be dropped is still in use.").  A batch on
 * which no stream of two or more was ever set, and one whose rings a call that reads `taken` back has shown empty, launches exactly what
 * it launched before; while the host cannot rule out a ring that holds an entry -- queued differs from the last taken count it read, for
 * some voice -- the renders walk the rings: k_stream_filter_rows if any voice filter is ACTIVE, in front of the filter stage with its sweeps
 * and filter programs, which runs over the voice's concatenated spans as it does without streams; else k_stream_rows.
 * Not done: interpolation across the seam; GLIDE on a streaming voice (a step that changes under a glide cannot be checked across a
 * take); rings longer than OALSFX_STREAM_QUEUE; streams in snapshots or groups; an upper bound in frames that would let a drained batch
 * leave the rings' kernels without a state call. */
#define OALSFX_STREAM_QUEUE 8
/* records[k][0 .. lengths[k] - 1] becomes the stream of instances[k] (NULL: 0 .. count - 1), lane 0: record 0 the current sampler record,
 * the rest the ring; the whole stream is replaced and taken becomes 0.  records is [count][1 + OALSFX_STREAM_QUEUE]; entries past the
 * length are not read.  A length of 1 is oalsfx_batch_set_lane_samplers exactly.  Not deferred, ordered and uploaded as
 * oalsfx_batch_set_samplers is; the first stream of two records or more on a batch makes the rings' table and waits for the batch's
 * stream once, as the first envelope program does.  oalsfx_batch_set_samplers and _set_lane_samplers keep their contracts and also empty the voice's ring
 * and zero taken: a plain set is a stream of one.  (Gain changes in mid-stream go through the envelope's ramps.)
 * Refusals (return 0 with a message; nothing is changed): every refusal of oalsfx_batch_set_samplers, for every record; "Stream length out
 * of range." (outside 1 .. 1 + OALSFX_STREAM_QUEUE); "A queued sampler is not playing." (a record behind the first without PLAYING); for
 * a length of two or more "The streaming voice's envelope glides."; "Lane out of range."; an instance outside the batch or listed twice
 * ("An instance is listed twice as a stream target."); a poisoned batch.  The other way round, oalsfx_batch_set_envelopes and
 * _set_env_programs refuse a record with GLIDE for a voice whose ring may hold an entry with "The gliding voice streams."; the call reads
 * taken back where the host cannot tell. */
int oalsfx_batch_set_streams(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_sampler* records);
/* records[k][0 .. lengths[k] - 1] are put behind the entries the ring of instances[k] holds; lengths[k] may be 0.  records is
 * [count][OALSFX_STREAM_QUEUE].  Ordered and uploaded as sampler sets are: in front of the next render, and only then.  Where the taken
 * count the host read last leaves too little room for some voice, the call first reads the counts back, which waits for the renders
 * queued; if a listed voice is still short of room the whole call is refused with "The stream queue is full." and nothing changes.
 * Refusals: those of oalsfx_batch_set_streams, every record counting as a queued one; "Stream length out of range." for a length
 * outside 0 .. OALSFX_STREAM_QUEUE. */
int oalsfx_batch_append_streams(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_sampler* records);
/* lengths[k] = 1 + the entries waiting, and out[k][0 .. lengths[k] - 1] the records, the current one first, as every render queued so far
 * leaves them (waits for those); out is [count][1 + OALSFX_STREAM_QUEUE], entries past the length are not written. */
int oalsfx_batch_get_streams(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_sampler* out);
/* taken[k] and queued[k], the entries waiting, as every render queued so far leaves them (waits for those; four bytes per voice of the
 * batch are copied).  Either pointer may be NULL.  Record j of a stream (0 is the first record of the set call, appended ones count on)
 * is finished once taken > j, or once its voice is no longer PLAYING with taken == j: the caller may reuse its memory after a state call
 * has shown that.  The call also tells the batch which rings are empty: see above. */
int oalsfx_batch_get_stream_state(oalsfx_batch* b, const int* instances, int count, uint32_t* taken, uint32_t* queued);
int oalsfx_batch_set_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_sampler* records);
int oalsfx_batch_append_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_sampler* records);
int oalsfx_batch_get_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_sampler* out);
int oalsfx_batch_get_lane_stream_state(oalsfx_batch* b, int lane, const int* instances, int count, uint32_t* taken, uint32_t* queued);

/* How the next mix call would lay out `slot` (pending property changes and read-backs folded in first): counts[0] instances on the
 * ring-light kernels, [1] reverbs proven steady (the builds without fallback), [2] reverbs believed steady, [3] reverbs on
 * the general kernel.  Nothing the reference has a counterpart for; tests and bench.py use it to say which kernel they measured. */
int oalsfx_batch_plan(oalsfx_batch* b, int slot, int counts[4]);
/* Symbol of the steady-state reverb kernel launched last, with its template arguments as rocprofv3 prints them ("" before the first). */
const char* oalsfx_batch_last_reverb_kernel(const oalsfx_batch* b);
/* PCI bus id ("0000:c1:00.0") of a HIP device ordinal, for benchmark records that must show N distinct GPUs.  Returns 1 on success. */
int oalsfx_device_pci_bus_id(int device_id, char* out, int len);

/* ---- host-only helpers (no GPU needed): the parameter-update path, exposed so the descriptors can be
 * checked against the reference and so the CPU oracle can be driven with identical parameters. */
void oalsfx_host_effect_defaults(int effect_type, oalsfx_effect* out);        /* Effect::set_type_and_defaults */
void oalsfx_host_effect_normalize(oalsfx_effect* e);                          /* Effect::normalize */
int oalsfx_host_derive_slot(int channel_format, int sampling_rate, const oalsfx_effect* normalized, oalsfx_slot_params* out);
int oalsfx_host_derive_source(int channel_format, int sampling_rate, int effect_count, const oalsfx_send_props* direct,
                              const oalsfx_send_props* aux /* [effect_count] */, const int* slot_types /* [effect_count] */,
                              oalsfx_source_params* out);
int oalsfx_host_ring_floats(int effect_type, int sampling_rate);
int oalsfx_host_channel_count(int channel_format);
int oalsfx_host_preset_count(void);
const char* oalsfx_host_preset_name(int index);
int oalsfx_host_preset(int index, void* reverb_props_out /* 108 bytes */);
/* Voice envelopes.  _ramp fills gain_from, gain_to and gain_step = (to - from) / (float)frames -- one subtraction and one division in
 * fp32; frames == 0: a step of 0 -- for `channels` channels, and sets ramp_frames = frames, ramp_done = 0.  _glide sets glide_frames =
 * frames, glide_done = 0, step_to, glide_slope = ((int64)(step_to - step) << 16) / frames truncated toward zero (frames == 0: 0; beyond
 * int32, more than eight times the asset's rate per frame: +-(2^31 - 1), the steepest the record holds, and the glide still ends on
 * step_to) and the GLIDE flag.  _check says whether oalsfx_batch_set_envelopes would take the record for an instance whose sampler has `sampler_step`
 * (returns 1, or 0 with *message, which may be NULL, pointing at the refusal's text). */
void oalsfx_host_envelope_ramp(const float* from, const float* to, int channels, uint32_t frames, oalsfx_envelope* inout);
void oalsfx_host_envelope_glide(uint32_t step, uint32_t step_to, uint32_t frames, oalsfx_envelope* inout);
int oalsfx_host_envelope_check(const oalsfx_envelope* envelope, uint32_t sampler_step, const char** message);
/* Envelope programs.  _adsr fills out[0 .. 3], all zero first, for `channels` channels, every ramp made by oalsfx_host_envelope_ramp and
 * with nothing beyond its arithmetic: out[0] the attack, +0.0f to peak[c] over attack_frames; out[1] the hold, peak to peak over
 * hold_frames; out[2] the decay, peak to sustain[c] over decay_frames; out[3] the release, sustain to +0.0f over release_frames, with
 * STOP.  All four are ACTIVE.  A note-on sets out[0 .. 2] as a program of three, whose last segment holds the sustain level once its ramp
 * has completed; the note-off sets out[3]. */
void oalsfx_host_envelope_adsr(int channels, const float* peak, const float* sustain, uint32_t attack_frames, uint32_t decay_frames, uint32_t hold_frames,
                               uint32_t release_frames, oalsfx_envelope out[4]);
/* Resamplers.  _check says whether oalsfx_batch_set_fir_table would take coef[1 << phase_bits][taps] (returns 1, or 0 with *message, which
 * may be NULL, pointing at the refusal's text).  _cubic fills out[1 << phase_bits][4] with the Catmull-Rom spline at mu = p / P: c0 =
 * -mu^3/2 + mu^2 - mu/2, c1 = 3mu^3/2 - 5mu^2/2 + 1, c2 = -3mu^3/2 + 2mu^2 + mu/2, c3 = mu^3/2 - mu^2/2, each computed in double as written (every
 * term is exact there; at mu = 0 the outer coefficients are +0.0f) and converted to float once; phase_bits outside 0 .. 12 writes nothing.  _sinc fills out[1 << phase_bits][taps]
 * with a Blackman-windowed sinc low-pass, 0 < cutoff <= 1 the pass band as a fraction of the asset's Nyquist frequency (about 4096 /
 * step for a voice pitched up, 1 otherwise): for phase p and tap k, d = (k - (H - 1)) - p / P, h = cutoff * sinc(cutoff * d) * w(d / H),
 * sinc(x) = sin(pi x) / (pi x), w(x) = 0.42 + 0.5 cos(pi x) + 0.08 cos(2 pi x); each phase's taps divided by their sum -- the pairs h_k + h_(T-1-k) added from the outside in, so that
 * the phases p and P - p, whose taps mirror each other, agree on their bits: coef[p][k] == coef[P - p][T - 1 - k] --, all in double,
 * and converted to float once.  Returns 0 with nothing written for taps other than 4 or 8, phase_bits outside 0 .. 12 or a cutoff
 * outside (0, 1]. */
int oalsfx_host_fir_check(int taps, int phase_bits, const float* coef, const char** message);
void oalsfx_host_fir_cubic(int phase_bits, float* out);
int oalsfx_host_fir_sinc(int taps, int phase_bits, double cutoff, float* out);
/* Voice filters.  _voice_filter fills b0, b1, b2, a1 and a2 of *inout (nothing else) with the reference's FilterState::set_params
 * (src/oalsfxpp.cpp:867-982) for kind OALSFX_VF_LOW_PASS .. OALSFX_VF_PEAKING: gain the shelf's or peak's linear gain (not looked at by the
 * three passes), freq_mult the corner frequency as a fraction of the sampling rate, rcp_q one over Q.  Returns 0 with nothing written for a
 * kind out of range, a gain at or below 0.00001 or not a number, or a freq_mult outside (0, 0.5).  _rcp_q_from_slope and
 * _rcp_q_from_bandwidth are the reference's two ways to rcp_q (:842-865): a shelf's slope, a band's width in octaves.  _check says
 * whether oalsfx_batch_set_filters would take the record (returns 1, or 0 with *message, which may be NULL, pointing at the refusal's
 * text; a NULL record: "No voice filter record."). */
int oalsfx_host_voice_filter(int kind, float gain, float freq_mult, float rcp_q, oalsfx_voice_filter* inout);
float oalsfx_host_rcp_q_from_slope(float gain, float slope);
float oalsfx_host_rcp_q_from_bandwidth(float freq_mult, float bandwidth);
int oalsfx_host_voice_filter_check(const oalsfx_voice_filter* filter, const char** message);
/* Voice filter sweeps.  _filter_sweep fills *out, all zero first: ACTIVE, frames, done = 0, from[k] and to[k] the coefficients of *from
 * and *to in the order b0, b1, b2, a1, a2, and step[k] = (to[k] - from[k]) / (float)frames, one subtraction and one division in fp32.
 * Returns 0 with nothing written for a NULL argument or frames outside 1 .. 2^24.  _check says whether oalsfx_batch_set_sweeps would take
 * the record, the target's filter apart (returns 1, or 0 with *message, which may be NULL, pointing at the refusal's text; a NULL
 * record: "No filter sweep record."). */
int oalsfx_host_filter_sweep(const oalsfx_voice_filter* from, const oalsfx_voice_filter* to, uint32_t frames, oalsfx_filter_sweep* out);
int oalsfx_host_filter_sweep_check(const oalsfx_filter_sweep* sweep, const char** message);
/* Filter programs.  _filter_program takes segments + 1 designed filters, nodes[0 .. segments], and `segments` lengths: out[k] is
 * oalsfx_host_filter_sweep(&nodes[k], &nodes[k + 1], frames[k]) bit for bit, so out[k].to equals out[k + 1].from in their bytes: a
 * continuous piecewise-linear program.  Returns 0 with nothing written for a NULL argument, segments outside 1 ..
 * OALSFX_FILTER_PROGRAM_MAX or a length outside 1 .. 2^24.
 * _filter_sweep_log approximates a sweep that is linear in log-frequency by such a chain of cookbook designs: node k of segments + 1
 * lies at freq_mult_from * (freq_mult_to / freq_mult_from)^(k / segments), the power computed in double (pow) and rounded to float once;
 * the two ends are taken as given, with no power.  Every node is designed through oalsfx_host_voice_filter(kind, gain, ., rcp_q).  The
 * lengths are frames / segments, the first frames % segments of them one frame longer.  node_freq_out (segments + 1 floats, may be
 * NULL) returns the frequencies used.  Returns 0 with nothing written for a NULL out, segments outside 1 ..
 * OALSFX_FILTER_PROGRAM_MAX, frames < segments or above 2^24, a frequency that is not positive, or whatever oalsfx_host_voice_filter
 * refuses for a node. */
int oalsfx_host_filter_program(const oalsfx_voice_filter* nodes, const uint32_t* frames, int segments, oalsfx_filter_sweep* out);
/* Sampler streams.  _stream_chunks cuts *record, a one-shot over a long asset, into records of consecutive chunks of chunk_frames frames
 * (the last one shorter where the length does not divide): out[k] is *record with data moved on by k * chunk_frames frames of its format
 * and channel count, frames the chunk's, and position 0 -- out[0] keeps the record's position, which must lie inside the first chunk.
 * Step, gains, format, channels and flags are the record's in every chunk, so that with nearest-sample playback the chunks, set and
 * appended in order, play the whole asset's bits.  Returns the number of chunks written, or 0 with nothing written for a NULL argument,
 * chunk_frames == 0, a record with LOOP, without frames or of an unknown format, a position outside the first chunk, or more chunks
 * than max_chunks. */
int oalsfx_host_stream_chunks(const oalsfx_sampler* record, uint32_t chunk_frames, int max_chunks, oalsfx_sampler* out);
int oalsfx_host_filter_sweep_log(int kind, float gain, float freq_mult_from, float freq_mult_to, float rcp_q, uint32_t frames, int segments,
                                 oalsfx_filter_sweep* out, float* node_freq_out);

#ifdef __cplusplus
}
#endif

/* Measurement and test helpers of bench.py, scripts/ and tests/ (kernel timing by events, counter calibration, placement probes, the
 * experiment switches): include/oalsfx_hip_debug.h.  Exported by the same library; nothing a caller of the effect path needs. */

#endif /* OALSFX_HIP_H */
