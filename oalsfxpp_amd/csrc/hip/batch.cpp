// Batch runtime behind the C ABI of include/oalsfx_hip.h.
//
// Owns, for N independent instances: the API-visible property bookkeeping (host), the derived
// descriptors (host shadow + device copy), the process-path state and delay rings (device only) and
// the launch plan (per slot, per effect type, a device list of instance indices).  One call to
// oalsfx_batch_mix* advances every instance by one buffer: the slot loop of the reference's
// Api::Impl::mix_data (reference src/oalsfxpp.cpp:2984-3037) becomes, per slot, one kernel launch per
// effect type present in that slot.
//
// There is no CPU implementation of the sample path in this library: without a usable HIP device
// oalsfx_batch_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../host/core.hpp"
#include "common.hpp"
#include "oalsfx_hip.h"
#include "state_io.hpp"
#include "downmix.hpp"
#include "meter.hpp"
#include "sampler.hpp"
#include "voice.hpp"
#include "resample.hpp"
#include "biquad.hpp"
#include "program.hpp"
#include "sweep.hpp"
#include "filter_program.hpp"
#include "stream.hpp"
#include "polyphony.hpp"
#include "record_table.hpp"
#include "oalsfx_hip_debug.h"

using namespace oalsfx_host;
using oalsfx_hip::KernelCtx;

namespace {

thread_local std::string g_last_error;

struct RingPool {
    size_t slab_floats = 0;
    std::vector<float*> free_clean; // zero-filled, never used since allocation
    std::vector<float*> free_dirty;
};

struct TimedLaunch { hipEvent_t start, stop; int type; };

constexpr int kSideStreams = 3; // ring-light effects, proven-steady reverbs, believed-steady reverbs, general reverbs: four kernel groups side by side at most

} // namespace

// How many launches of a run of chained launches may be in flight (streams taken in turn).  Two overlap one launch's tail with the next
// one's head; a third keeps the workgroup slots that fast workgroups free in use while the slowest of the launch two before are still
// at work (cross-fading instances, presets of the slower kinds): a launch starts when the launch kChainDepth before it has completed.
constexpr int kChainDepth = 3;
static_assert(kChainDepth >= 1 && kChainDepth <= 3, "a wavefront looks at the CUs of the two launches before it (reverb.hip, turn_cu / turn_cu2): at most three launches in flight");

// `rows` rows of a record table made beside the one in use (records_resized), until they take its place (records_replace).
template <class T>
struct ResizedRecords {
    T* d = nullptr;
    std::vector<T> host;
};

// A record per voice that lives on the device and is set from the host (samplers, voice envelopes, resamplers, voice filters, envelope
// programs, filter sweeps, filter programs): the host's table (record_table.hpp), the device's array, and the page-locked buffer through which one launch in front of
// the next render puts the rows set since the last one in place (records_upload).  Everything the records_* helpers need to know of a
// table is here; each_voice_table visits the seven.
template <class T>
struct DeviceRecords {
    const char* name;                             // in error texts: "hipMalloc(<name>)"
    const char* upload_name;                      // ... and of the upload's launch
    T init;                                       // a row nothing has been set in ...
    int fill;                                     // ... and the byte that says the same in every byte of a device row
    void (*launch)(T*, const int*, const T*, int, hipStream_t); // the scatter kernel of records_upload
    oalsfx_records::RecordTable<T> table;
    T* d = nullptr;                               // [n * lanes], lane-major
    char* h_stage = nullptr;                      // page-locked: [capacity] records, then [capacity] instance numbers
    size_t stage_capacity = 0;                    // records
    hipEvent_t ev_staged = nullptr;               // behind the last launch that read the staging buffer
    bool stage_pending = false;
    long long uploads = 0;
    bool ahead = false;                           // a render has changed the device's rows since `table` was read back
    ResizedRecords<T> resized;                    // oalsfx_batch_set_polyphony: the table with the new row count, until it is put in place
};

struct oalsfx_batch {
    int n = 0, slots = 0, channels = 0, rate = 0, device = 0;
    int format = 0;
    DeviceDesc dev;
    std::vector<InstanceHost> inst;

    // host shadows
    std::vector<oalsfx_slot_params> h_params;     // [n*slots]
    std::vector<oalsfx_slot_state> h_state_init;  // [n*slots] staging for restarted slots
    std::vector<oalsfx_source_params> h_source;   // [n]
    std::vector<uint32_t> seq;                    // [n*slots]
    std::vector<float*> h_rings;                  // [n*slots]
    std::vector<size_t> ring_floats;              // [n*slots] size class of the slab held
    bool rings_table_dirty = false;               // h_rings changed outside prepare_params (restore, reset): the next upload carries the table
    std::vector<uint8_t> inst_dirty;              // [n]
    // Host-side belief about the reverb slots, kept incrementally (a parameter change touches its own slot only):
    std::vector<int> since_update;                // [n*slots] frames mixed since the slot's last parameter update (capped)
    std::vector<uint8_t> slot_class;              // [n*slots] kClass* bits of the slot's current parameters
    std::vector<size_t> settling;                 // reverb slots updated less than kSettleFrames ago
    std::vector<uint8_t> in_settling;             // [n*slots] membership flag of `settling`
    std::vector<uint8_t> mod_ever;                // [n*slots] the slot's late line was modulated at some time since its state was created (the depth
                                                  // smoother keeps moving long after the depth is set to 0)
    std::vector<uint8_t> xf_ok;                   // [n*slots] settling, and in a way the cross-fading build of the steady-state kernel follows
                                                  // (taps of both sets a tile away, state kept): listed with the believed-steady instances
    int n_close[OALSFX_MAX_SLOTS] = {};           // per slot: reverbs with a tap between one and two tiles ...
    int n_short[OALSFX_MAX_SLOTS] = {};           // ... with a tap shorter than one tile
    bool modulated[OALSFX_MAX_SLOTS] = {};        // some reverb of the slot has, or had, a modulated late line (sticky: the depth
                                                  // smoother keeps moving long after the depth is set to 0)
    int n_filtered = 0;                           // instances with a send filter switched on
    std::vector<uint8_t> inst_filtered;           // [n] ... which
    std::vector<int> h_lists;                     // host copy of d_lists as last built
    uint32_t lists_version = 0;
    // how many filtered instances the SF builds take care of themselves (launch_reverb_kinds_part), cached per list version and boundary
    uint32_t inside_version = ~0u;
    int inside_end = -1, inside_filtered = 0;
    // What the host *knows* about the reverb slots (as opposed to believes): a slot is proven steady once the device has reported it
    // settled and at rest (d_exact, read back without ever waiting for the stream) and nothing has been uploaded for its instance since.
    std::vector<uint8_t> proven;                  // [n*slots] 0, or from how many tiles a block on the slot's output gains are at rest (1 .. 4)
    std::vector<uint32_t> updated_gen;            // [n*slots] upload generation of the last parameter upload that touched the slot's instance
    std::vector<uint32_t> inst_epoch;             // [n] stamps the hot records: bumped with every upload that touches the instance
    uint32_t upload_gen = 0;
    bool exact_wanted = false;                    // something changed that may let the next read-back prove more slots
    bool exact_pending = false;                   // a read-back of d_exact is in flight (ev_exact)
    uint32_t exact_gen = 0;                       // upload generation the read-back in flight was taken at
    std::vector<int> dirty_list;
    bool lists_dirty = true;
    // Instances a setter has written since they were last applied: apply_changes() visits only these (for the others the
    // reference's comparison of deferred and active properties finds nothing by construction).
    std::vector<uint8_t> touched;                 // [n]
    std::vector<int> touched_list;
    // An auxiliary send was written since the instance's sends were last derived.  The reference re-derives the sends from the
    // active aux props whenever a slot changed (update_context_sources, src/oalsfxpp.cpp:3397-3412), but apply_changes flags the
    // source only while an aux send differs from (1, 1, 1) (:3772-3780): a send set back to exactly (1, 1, 1) must still be seen.
    std::vector<uint8_t> aux_written;             // [n]

    // device
    oalsfx_slot_params* d_params = nullptr;
    oalsfx_hip::SlotStateLines* d_state = nullptr;
    oalsfx_source_params* d_source = nullptr;
    float** d_rings = nullptr;
    oalsfx_source_state* d_source_state = nullptr; // [n] histories of the send filters
    float* d_filtered = nullptr;                  // [1 + slots][n][chunk frames][channels] outputs of the send-filter pre-pass
    size_t filtered_capacity = 0;                 // floats per send plane
    float* d_mixbuf = nullptr;
    int* d_lists = nullptr;                       // [slots][n]: the one of d_lists_buf the next launches read
    int* d_lists_buf[kChainDepth + 1] = {};       // every rebuilt list goes to the next buffer: a launch that is still in flight -- chained
                                                  // launches -- keeps reading the list it was given
    int lists_turn = 0;
    int* d_progress = nullptr;                    // [n*slots] hand-off from the steady-state reverb kernel to the general kernel behind it
    unsigned* d_hot = nullptr;                    // [n*slots][hot::SIZE] start records of the proven-steady reverb kernel
    unsigned* d_inst_epoch = nullptr;             // [n]
    unsigned* d_exact = nullptr;                  // [n*slots] "settled and at rest" as the reverb kernels left it
    unsigned* h_exact = nullptr;                  // pinned copy of d_exact, filled by the read-back
    char fault_text[400] = {};
    long long host_prepare_ns = 0, host_stage_wait_ns = 0, host_derive_ns = 0, host_lists_ns = 0; // OALSFX_HOST_PROFILE: where the host's time inside mix_device goes
    unsigned* h_fault = nullptr;                  // pinned, device-visible: instances a proven-steady launch had to leave alone (must stay 0)
    unsigned* d_fault = nullptr;                  // device address of h_fault  ([1]: gates of chained launches that gave up waiting, a word of its own)
    bool chain_given_up = false;                  // gates counted out and nothing else did: something runs the queues' kernels one at a time; stream order from then on
    uint32_t gate_skew = 0;                       // test hook (oalsfx_debug_gate_skew): added to every gate's target, so that the gates count out
    hipEvent_t ev_exact = nullptr;
    // Snapshot / restore / reset (oalsfx_batch_snapshot ...): the call's tables -- copy segments, state fix-ups, records built on the host --
    // are packed into page-locked memory and go to device memory in one copy in front of the launches that read them; the page-locked
    // buffer is reused once ev_state_io (recorded behind those launches) has completed.
    char* h_state_io = nullptr;
    char* d_state_io = nullptr;
    size_t state_io_capacity = 0;
    hipEvent_t ev_state_io = nullptr;
    bool state_io_pending = false;
    bool state_io_unordered = false;              // ev_state_io marks launches on the batch's stream that the next launch on a caller's stream must wait for
    // Per slot the list is: ring-light types in ascending order (list_offset / list_count per type), then the reverb instances
    // proven steady (reverb, EAX reverb: steady_offset / fast_count), those believed steady (reverb, EAX reverb: slow_count), then
    // every other reverb instance of both types (general_offset / general_count).  list_count of a reverb type counts all its
    // instances.
    int list_offset[OALSFX_MAX_SLOTS][OALSFX_TYPE_COUNT] = {};
    int list_count[OALSFX_MAX_SLOTS][OALSFX_TYPE_COUNT] = {};
    int steady_offset[OALSFX_MAX_SLOTS] = {};     // start of the steady region: the proven instances, then the believed ones
    int fast_count[OALSFX_MAX_SLOTS] = {};        // proven steady (both reverb types)
    int kind_count[OALSFX_MAX_SLOTS][3] = {};     // ... of which, in list order: every tap two tiles away; a tap of one to two tiles; shorter taps or a
                                                  // modulated late line (the FP build each needs: plain, HY, ST)
    int rest_tiles[OALSFX_MAX_SLOTS] = {};        // ... whose output gains are at rest for blocks of that many tiles and longer (1 .. 4)
    int fast_first[OALSFX_MAX_SLOTS] = {};        // >= 0: the proven part of the list is the instance range fast_first, fast_first + 1, ...
    int slow_count[OALSFX_MAX_SLOTS] = {};        // believed steady (both reverb types)
    int general_offset[OALSFX_MAX_SLOTS] = {};
    int general_count[OALSFX_MAX_SLOTS] = {};
    std::map<size_t, RingPool> pools;
    std::vector<void*> chunks;
    struct RingChunk { char* base; size_t bytes; void* alloc; };
    std::vector<RingChunk> ring_chunks;            // the slab pools' chunks (for oalsfx_debug_move_rings)
    // placement search (place_ring_chunk): what it did for this batch, for benchmark records
    int placed_chunks = 0, placement_candidates = 0;
    double placement_best_us = 0.0, placement_worst_us = 0.0;

    // staging for host-pointer mixes
    float* d_io_src = nullptr;
    float* d_io_dst = nullptr;
    size_t io_capacity = 0;
    // ... and page-locked host buffers for callers whose instances each have buffers of their own (oalsfx_batch_mix_gather)
    float* h_io_src = nullptr;
    float* h_io_dst = nullptr;
    size_t h_io_capacity = 0;
    // ... and for the pipelined ones (oalsfx_batch_mix_async): kPipeDepth staging slots used in turn; the copy in, the kernels and the
    // copy out of successive calls run on three streams, ordered by events only
    static constexpr int kPipeDepth = 3;
    struct PipeSlot { float* d_src = nullptr; float* d_dst = nullptr; hipEvent_t copied_in = nullptr, mixed = nullptr, copied_out = nullptr; bool busy = false; };
    PipeSlot pipe[kPipeDepth];
    size_t pipe_capacity = 0;
    long long pipe_turn = 0;
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
    // How successive calls of oalsfx_batch_mix_async share the link: form 3: the copy in of call k + 1, the kernels of call k and the copy
    // out of call k - 1 on three streams, both directions busy at once; form 1: copy in, kernels and copy out of a call on the batch's one
    // stream, in order -- the synchronous call's sequence without its wait.  Some hosts' copy engines run the two directions far below the
    // link's rate when both are busy (round 3's driver box: 0.48 ms per step on three streams against 0.38 synchronous), on others three
    // streams are fastest (0.20 - 0.24 ms): decided per device by the first calls of the first batch that pipelines -- sixteen calls to
    // set everything up, sixteen on one stream, sixteen on three, the host's clock over the last twelve of either (the pipeline paces the caller: a call waits for
    // the one that used its staging slot three calls ago) -- and remembered; the single stream has to win by a tenth.
    // OALSFX_HOST_PIPELINE=1|3 fixes the form.  (Also built and measured, round 4: both copies on one stream in turn, the copy out of a
    // call queued behind the next call's copy in, the kernels beside them -- 0.41 ms where the synchronous call takes 0.37 and three
    // streams 0.24: a copy engine that changes direction every copy is slower than either.)
    int pipe_mode = 0;                      // 0: probing
    std::chrono::steady_clock::time_point pipe_probe_t0;
    double pipe_probe_us[2] = {0.0, 0.0};   // per call: what the probe saw on three streams / on one

    unsigned long long* d_timeline = nullptr;    // measurement only (OALSFX_DEBUG_TIMELINE=<file>)
    // Parameter uploads: the changed records are packed into pinned memory and put in place by one kernel (k_upload); four buffers
    // take turns so that the host never waits for the stream.
    struct Stage { char* host = nullptr; char* dev = nullptr; size_t capacity = 0; hipEvent_t done = nullptr; bool pending = false; };
    Stage stage[4];                               // (four: an event of this stack is seen complete only once the launch behind it has run,
                                                  // so the buffer of two uploads ago would still make the host wait for the GPU)
    int stage_turn = 0;
    hipEvent_t ev_uploaded = nullptr;             // parameter uploads of the batch's own stream -> a caller's launch stream
    hipEvent_t ev_mixed = nullptr;                // last launch on a caller's stream -> parameter uploads that overwrite what it reads
    hipStream_t last_launch_stream = nullptr;
    const char* last_steady_kernel = "";          // symbol of the last steady-state reverb launch

    hipStream_t stream = nullptr;
    // Chained launches: consecutive calls on the batch's own stream whose whole step is one steady-state reverb launch take turns on two
    // streams with nothing but a word per instance ordering them (KernelCtx::turn), so that the tail of one launch overlaps with the head
    // of the next (the ~6 us between dependent launches of one stream).  Off once the caller has asked for the stream handle: work
    // queued there by the caller expects the launches in stream order.
    hipStream_t chain_stream[kChainDepth] = {};   // [0] is `stream`; a run's launches take them in turn
    hipEvent_t ev_chain[kChainDepth] = {};
    int chain_pos = 0;                            // the stream of the last chained launch
    int chain_pos_last = -1, chain_pos_before = -1; // ... of the launch before this call's, and of the one before that (-1: none in this run)
    bool chain_used[kChainDepth] = {};            // streams the current run has launched on
    hipEvent_t ev_chain_start = nullptr;          // recorded in front of a run's first launch: the second (other stream) starts no earlier
    unsigned* d_turn = nullptr;                   // [n*slots], then the count of workgroups of chained launches that have started (k_chain_gate)
    uint32_t turn_counter = 0;                    // the number the last chained launch set
    uint32_t started_total = 0;                   // what that count comes to once the last chained launch has started as a whole
    int launched_groups = 0;                      // workgroups of the call's steady-state reverb launch (what its chained launch adds to that count)
    // Where the delay lines' write positions stand on the 128-byte line grid (32 frames of a ring line): a slot's position is the frames
    // mixed since its state was last started.  After a call that was not a multiple of 32 frames every ring store of a tile begins and
    // ends inside a line; the plain FP build then takes its line-aligned variant (reverb.hip, CR == 2).  A speed hint: the kernel goes by
    // the position it finds in the state.
    uint32_t frames_total = 0;                    // frames mixed by the batch so far (wraps)
    std::vector<uint32_t> started_at;             // [n*slots] frames_total when the slot's state was last started
    bool off_grid_known = false;                  // off_grid[] is up to date
    int off_grid[OALSFX_MAX_SLOTS] = {};          // per slot: reverbs whose write position is not a multiple of 32 frames
    bool poisoned = false;                        // a chained launch gave up waiting: some instance missed a buffer; every later call fails
    int chain_len = 0;                            // launches in the current run
    std::vector<std::pair<const char*, const char*>> chain_dsts; // ... and their output buffers
    bool uncached = false;                        // what launches hand on lives in uncached memory: calls can be chained launches
    bool chain_open = false;                      // the last call was a chained launch (its kernel may still run, on either stream)
    bool stream_handed_out = false;
    long long chained_calls = 0;
    long long multi_buffers = 0, multi_passes = 0; // mix_device_multi: buffers that went through multi-buffer passes, and the passes
    // Calls that join a queued launch (join_word.hpp): a chained launch that sits behind a gate of its own takes the plain
    // single-buffer calls that arrive before the gate lets it go.  One slot (word and buffer table, page-locked and device-visible) per
    // such launch, used in turn -- a slot is taken again only once its last gate has said it is through with it, else the launch is an
    // ordinary one --, and one device-side table per stream of a run: a stream's gate writes it, the grid behind that gate reads it, and
    // the stream's next gate comes behind that grid.
    static constexpr int kJoinSlots = 1024;       // (a host that runs further ahead than this many joinable launches gets ordinary ones meanwhile)
    oalsfx_join::JoinSlot* h_join = nullptr;      // [kJoinSlots]
    oalsfx_join::JoinSlot* d_join = nullptr;      // device address of h_join
    oalsfx_hip::BufferTable* d_join_tables = nullptr; // [kChainDepth], uncached device memory
    int join_turn = 0;
    struct JoinLaunch {
        bool accepting = false;                   // the last launch queued is joinable and nothing has come behind it: a call may try
        bool held = false;                        // test hook (join_hold): its gate and grid are not queued yet
        int slot = 0, table = 0;                  // h_join[slot], d_join_tables[table]
        unsigned count = 0;                       // buffers published so far
        int frames = 0;                           // per buffer
        KernelCtx ctx{};                          // the launch as it was (or will be) queued
        hipStream_t stream = nullptr;
        int reverb_slot = 0, flags = 0;
        const int* list = nullptr;
        int counts[4] = {};
        int groups = 0;                           // the grid's workgroups
        bool carry = false;
        const unsigned* gate_started = nullptr;
        unsigned gate_target = 0;
        const char* srcs[oalsfx_join::kMaxBuffers] = {}; // the table's buffers, for the overlap rules
        const char* dsts[oalsfx_join::kMaxBuffers] = {};
    } join;
    int join_hold = 0;                            // test hook (oalsfx_debug_join_hold): a joinable launch is queued once it has this many buffers
    long long joined_calls = 0, joinable_launches = 0;
    // Bus downmix (oalsfx_batch_set_routing, oalsfx_batch_downmix_device): the routing is state of the batch beside its instances -- no
    // effect call, snapshot, restore or reset reads or writes it.  The member lists per bus are built on the host, like the launch lists,
    // and go to the device when the routing or the number of buses a call names has changed since the last downmix.
    // Bus sends: OALSFX_BUS_SENDS (bus, gain) pairs per instance, send 0 the routing of oalsfx_batch_set_routing.  A ramp is kept as
    // (from, step, to, frames) and the value of dm_clock -- the frames downmixed so far -- at which it began: every downmix advances every
    // ramp by moving the clock, and a ramp whose frames have passed is folded into the send's gain where it is next looked at.
    struct SendRamp {
        float from = 0.0F, step = 0.0F, to = 0.0F;
        uint32_t frames = 0;                      // 0: none
        unsigned long long start = 0;
    };
    std::vector<int> route_bus[OALSFX_BUS_SENDS];       // [n] -1: nowhere
    std::vector<float> route_gain[OALSFX_BUS_SENDS];    // [n]
    std::vector<SendRamp> route_ramp[OALSFX_BUS_SENDS]; // [n]
    unsigned long long dm_clock = 0;              // frames downmixed so far
    unsigned long long dm_table_clock = 0;        // ... when the device's table was built
    unsigned long long dm_ramps_end = 0;          // the table has ramps, and the last of them ends at this value of dm_clock (0: no ramps)
    std::vector<oalsfx_hip::DownmixRamp> dm_ramp_rows; // [send][n], what DownmixTable::build reads while some routed send ramps
    bool routing_dirty = true;                    // ... changed since route_max and the device's table were made
    int route_max = -1;                           // highest bus a send names
    int dm_buses = 0;                             // the bus count the device's table was built for
    oalsfx_hip::DownmixTable dm_table;
    oalsfx_hip::DownmixDevice dm_dev;
    char* h_dm_table = nullptr;                   // page-locked, packed (DownmixTable::pack)
    char* d_dm_table = nullptr;
    size_t dm_table_capacity = 0;
    float* d_dm_partials = nullptr;               // [partial rows][frames * channels]: level 1 -> level 2
    size_t dm_partials_capacity = 0;              // floats
    float* d_dm_out = nullptr;                    // [buses][frames * channels] of oalsfx_batch_mix_downmix
    size_t dm_out_capacity = 0;
    hipEvent_t ev_downmix = nullptr;              // behind the last downmix's launches (they read the table and write the partials)
    hipEvent_t ev_dm_order = nullptr;             // the batch's stream -> a caller's stream a downmix is queued on
    hipStream_t dm_stream = nullptr;              // where the last downmix went
    bool dm_pending = false;
    long long dm_uploads = 0;
    // Level meters (oalsfx_batch_mix_downmix_meter): [n + buses] records the call's launches write; nothing in them outlives a call
    oalsfx_meter* d_meters = nullptr;
    size_t meters_capacity = 0;                   // records
    // Samplers (oalsfx_batch_set_samplers, oalsfx_batch_sample_device): state of the batch beside its instances, like the routing.  The
    // records live on the device, where every render advances them; the host keeps what it last knew of them and which it has written
    // since the last render.  Those go to the device in front of the next render, read by one kernel from page-locked memory.
    DeviceRecords<oalsfx_sampler> samplers{"samplers", "sampler upload", oalsfx_sampler{}, 0, oalsfx_hip::launch_sampler_upload};
    hipEvent_t ev_sampler = nullptr;              // behind the last render (it reads and writes the records)
    hipStream_t sampler_stream = nullptr;         // where the last render went
    bool sampler_pending = false;
    // Voice envelopes (oalsfx_batch_set_envelopes): a second record per instance beside the sampler's, kept as the samplers are.  The
    // renders read and write both, so ev_sampler orders them too.
    DeviceRecords<oalsfx_envelope> envelopes{"envelopes", "envelope upload", oalsfx_envelope{}, 0, oalsfx_hip::launch_voice_upload};
    bool steps_ahead = false;                     // a glide among the envelopes a render advanced may have changed a sampler's step
    int envelopes_active = 0;                     // records with OALSFX_ENV_ACTIVE: exact, only the caller sets or clears the flag
    int envelopes_gliding = 0;                    // ... with ACTIVE and GLIDE
    // Resamplers (oalsfx_batch_set_resamplers, oalsfx_batch_set_fir_table): a table index per instance beside the two records, and the
    // batch's coefficient tables.  No render writes either, so the host's copy is always the current one (resamplers.ahead stays false).
    // A row is a table index or OALSFX_RESAMPLER_NONE: -1, 0xFF in every byte.
    DeviceRecords<int> resamplers{"resamplers", "resampler upload", OALSFX_RESAMPLER_NONE, 0xFF, oalsfx_hip::launch_fir_upload};
    int resamplers_active = 0;                    // instances that name a table: exact, only oalsfx_batch_set_resamplers changes them
    oalsfx_hip::FirTables fir = {};               // the tables as the kernel gets them: device pointers, taps (0: empty slot), shifts
    int fir_named[OALSFX_FIR_TABLES] = {};        // instances that name each table
    // Polyphony (oalsfx_batch_set_polyphony): every record table (samplers, envelopes, resamplers, filters, and the programs once made)
    // has n * lanes rows, voice row = lane * n + instance; the counts above (envelopes_active, envelopes_gliding, resamplers_active,
    // fir_named) are of voices of every lane
    int lanes = 1;
    // Voice filters (oalsfx_batch_set_filters): a fourth record per voice.  A render that has an ACTIVE one among them (k_biquad_rows)
    // moves its histories on and renders the filtered voices into the scratch row of their instance first.
    DeviceRecords<oalsfx_voice_filter> filters{"voice filters", "voice filter upload", oalsfx_voice_filter{}, 0, oalsfx_hip::launch_biquad_upload};
    int filters_active = 0;                       // records with OALSFX_VF_ACTIVE, of every lane: exact, only the caller sets or clears the flag
    float* d_voice_scratch = nullptr;             // [n][frames][channels] of the last render that had an active filter
    size_t voice_scratch_capacity = 0;            // floats
    // Envelope programs (oalsfx_batch_set_env_programs): a fifth table, a queue of segments per voice, made with the first program of two
    // segments or more (programs.d == nullptr until then: a kilobyte per voice).  program_horizon: an upper bound of the frames still to
    // render until every queue is empty, known without a read-back -- a program's frames in front of its last segment when it is set,
    // one more so that a program of zero-length segments gets its render, less every render's frames.  While it is positive the renders
    // walk the queues (k_program_rows, k_program_biquad_rows); at 0 the batch launches what it launched before.
    DeviceRecords<oalsfx_hip::EnvProgram> programs{"envelope programs", "program upload", oalsfx_hip::EnvProgram{}, 0, oalsfx_hip::launch_program_upload};
    std::vector<uint8_t> program_set;             // [n * lanes] the voice's queue was filled since it was last emptied by a set call
    long long program_horizon = 0;                // frames
    // Voice filter sweeps (oalsfx_batch_set_sweeps): a sixth record per voice.  sweep_horizon: an upper bound of the frames still to
    // render until no sweep is under way, kept as program_horizon is -- the largest frames - done over the sweeps set, less the frames of
    // every render that ran them.  While it is positive and a filter is ACTIVE the renders look at the sweeps (k_sweep_rows,
    // k_sweep_program_rows); at 0 the batch launches what it launched before.
    DeviceRecords<oalsfx_filter_sweep> sweeps{"filter sweeps", "filter sweep upload", oalsfx_filter_sweep{}, 0, oalsfx_hip::launch_sweep_upload};
    std::vector<uint8_t> sweep_set;               // [n * lanes] the voice's row may be other than all zero on the device: a cancel has to go there
    long long sweep_horizon = 0;                  // frames
    // Filter programs (oalsfx_batch_set_filter_programs): a seventh table, a queue of sweeps per voice, made with the first program of
    // two segments or more (filter_programs.d == nullptr until then: 576 bytes per voice).  filter_program_horizon is kept exactly as
    // program_horizon is: 1 + the frames in front of a program's last segment when it is set, the largest over the programs set, less
    // every render's frames.  While it is positive and a filter is ACTIVE the renders walk the queues (k_filter_program_rows,
    // k_filter_program_env_rows); sweep_horizon covers the whole program, so the last segment is run by the sweeps' kernels, and at 0
    // the batch launches what it launched before.
    DeviceRecords<oalsfx_hip::FilterProgram> filter_programs{"filter programs", "filter program upload", oalsfx_hip::FilterProgram{}, 0,
                                                             oalsfx_hip::launch_filter_program_upload};
    std::vector<uint8_t> filter_program_set;      // [n * lanes] the voice's queue was filled since it was last emptied by a set call
    long long filter_program_horizon = 0;         // frames
    // Sampler streams (oalsfx_batch_set_streams, _append_streams): an eighth table, a ring of sampler records per voice, made with the
    // first stream of two records or more (streams.d == nullptr until then: 656 bytes per voice), and beside it the device's taken
    // counts, a word per voice, which only the renders advance and only a set call's upload zeroes.  The host owns the rings: no
    // render writes them, so streams.ahead stays false.  stream_taken is the host's last reading of the counts and streams_open the
    // number of voices whose ring may hold an entry: queued != stream_taken.  While it is positive the renders walk the rings
    // (k_stream_rows); at 0 the batch launches what it launched before.  It falls only with a read-back of the counts.
    DeviceRecords<oalsfx_hip::StreamRing> streams{"stream rings", "stream upload", oalsfx_hip::StreamRing{}, 0, nullptr};
    uint32_t* d_stream_taken = nullptr;           // [n * lanes]
    std::vector<uint32_t> stream_taken;           // [n * lanes] as last read back; 0 behind a set call
    std::vector<int> stream_reset_list;           // rows whose host row carries `reset` until the next upload has taken it along
    bool stream_taken_ahead = false;              // a render has walked the rings since stream_taken was read
    int streams_open = 0;
    const char* last_render_kernel = "";
    // the kernel groups of one slot (ring-light effects, reverb, EAX reverb) touch disjoint instances: when more than one
    // is populated they run side by side on these streams, forked from and joined to the launch stream with events
    hipStream_t side_stream[kSideStreams] = {};
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_join[kSideStreams] = {};
    const char* error = "";
    std::string error_store;

    bool timing = false;              // the launches of the current mix call carry events
    int timing_every = 0;             // 0: off; k: every k-th mix call is timed
    long long mix_calls = 0;
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool; // created when timing is switched on, so that the timed region creates none

    hipEvent_t take_event()
    {
        hipEvent_t e = nullptr;
        if (!event_pool.empty()) { e = event_pool.back(); event_pool.pop_back(); }
        else hipEventCreate(&e);
        return e;
    }
    bool fail(const char* msg) { error = msg; return false; }
    bool hip_ok(hipError_t e, const char* what)
    {
        if (e == hipSuccess) return true;
        error_store = std::string(what) + ": " + hipGetErrorString(e);
        error = error_store.c_str();
        return false;
    }
    // ... with what = "<call>(<subject>)"
    bool hip_ok(hipError_t e, const char* call, const char* subject)
    {
        return e == hipSuccess || hip_ok(e, (std::string(call) + "(" + subject + ")").c_str());
    }
};

namespace {

constexpr const char* kErrRange = "Instance range is out of bounds.";
constexpr const char* kErrSlot = "Effect index is out of range.";   // reference ApiErrorMessages::effect_index_out_of_range
constexpr const char* kErrNoSrc = "No source samples.";              // reference ApiErrorMessages::no_src_samples
constexpr const char* kErrNoDst = "No destination samples.";         // reference ApiErrorMessages::no_dst_samples

bool range_ok(oalsfx_batch* b, int first, int count)
{
    if (first < 0 || count < 0 || first + count > b->n) return b->fail(kErrRange);
    return true;
}

void mark_touched(oalsfx_batch* b, int first, int count)
{
    for (int i = first; i < first + count; ++i)
        if (!b->touched[i]) {
            b->touched[i] = 1;
            b->touched_list.push_back(i);
        }
}

void mark_dirty(oalsfx_batch* b, int i)
{
    if (!b->inst_dirty[i]) {
        b->inst_dirty[i] = 1;
        b->dirty_list.push_back(i);
    }
}

// `rows` rows, every one r.init on the host and, by the batch's stream, r.fill in every byte on the device: the two say the same.
template <class T>
bool records_create(oalsfx_batch* b, DeviceRecords<T>& r, size_t rows)
{
    if (!r.ev_staged && !b->hip_ok(hipEventCreateWithFlags(&r.ev_staged, hipEventDisableTiming), "hipEventCreate")) return false;
    T* d = nullptr;
    if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&d), rows * sizeof(T)), "hipMalloc", r.name)) return false;
    if (!b->hip_ok(hipMemsetAsync(d, r.fill, rows * sizeof(T), b->stream), "hipMemsetAsync", r.name)) {
        hipFree(d);
        return false;
    }
    r.table.assign(rows, r.init);
    r.d = d;
    return true;
}

// (nothing on the device reads the records or the staging buffer any more)
template <class T>
void records_release(DeviceRecords<T>& r)
{
    if (r.h_stage) (void)hipHostFree(r.h_stage);
    hipFree(r.d);
    if (r.ev_staged) hipEventDestroy(r.ev_staged);
}

// The rows of `r` set since the last render, put in place on the device in front of the next one by r.launch, its scatter kernel.
template <class T, class Launch>
bool records_upload(oalsfx_batch* b, DeviceRecords<T>& r, hipStream_t stream, Launch launch)
{
    const size_t count = r.table.pending();
    // (the page-locked buffer is free once the launch that read it last has run)
    if (r.stage_pending && !b->hip_ok(hipEventSynchronize(r.ev_staged), "hipEventSynchronize")) return false;
    r.stage_pending = false;
    const size_t capacity = r.table.staging_capacity(r.stage_capacity);
    if (capacity != r.stage_capacity) {
        if (r.h_stage) (void)hipHostFree(r.h_stage);
        r.h_stage = nullptr;
        r.stage_capacity = 0;
        if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&r.h_stage), capacity * (sizeof(T) + sizeof(int))), "hipHostMalloc", r.name)) return false;
        r.stage_capacity = capacity;
    }
    T* const changed = reinterpret_cast<T*>(r.h_stage);
    int* const index = reinterpret_cast<int*>(changed + r.stage_capacity);
    r.table.drain(changed, index);
    launch(r.d, index, changed, static_cast<int>(count), stream);
    // the launch reads the buffer from here on, whatever becomes of the render
    r.stage_pending = true;
    ++r.uploads;
    if (!b->hip_ok(hipGetLastError(), r.upload_name) || !b->hip_ok(hipEventRecord(r.ev_staged, stream), "hipEventRecord")) return false;
    // ... and writes the records the renders read: ordered as a render is
    b->sampler_pending = true;
    b->sampler_stream = stream;
    return b->hip_ok(hipEventRecord(b->ev_sampler, stream), "hipEventRecord");
}

// ... by r.launch, its scatter kernel.
template <class T>
bool records_upload(oalsfx_batch* b, DeviceRecords<T>& r, hipStream_t stream)
{
    return records_upload(b, r, stream, r.launch);
}

// The host's rows of `r` as every render queued so far leaves the records (waits for those), where a render has changed them since they
// were last read back (r.ahead): the whole device array fetched once behind the last render, then merge(now) to bring the host's rows
// up to date.
template <class T, class Merge>
bool records_read_back(oalsfx_batch* b, DeviceRecords<T>& r, Merge merge)
{
    if (!r.ahead) return true;
    std::vector<T> now(r.table.host.size());
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return false;
    if (b->sampler_pending && !b->hip_ok(hipEventSynchronize(b->ev_sampler), "hipEventSynchronize")) return false;
    if (!b->hip_ok(hipMemcpy(now.data(), r.d, now.size() * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy", r.name)) return false;
    b->sampler_pending = false; // (ev_sampler has been waited for: until it is recorded again, which sets this again, a wait for it is none)
    merge(now);
    r.ahead = false;
    return true;
}

// ... with the table's own merge: the device's value for every row that has not been set since.
template <class T>
bool records_read_back(oalsfx_batch* b, DeviceRecords<T>& r)
{
    return records_read_back(b, r, [&r](const std::vector<T>& now) { r.table.merge(now.data()); });
}

// r.resized: `r` with `rows` rows, made beside the one in use: the first rows as the host has them, the rest r.init, on the host and on
// the device.
template <class T>
bool records_resized(oalsfx_batch* b, DeviceRecords<T>& r, size_t rows)
{
    r.resized.host = r.table.host;
    r.resized.host.resize(rows, r.init);
    return b->hip_ok(hipMalloc(reinterpret_cast<void**>(&r.resized.d), rows * sizeof(T)), "hipMalloc", r.name) &&
           b->hip_ok(hipMemcpy(r.resized.d, r.resized.host.data(), rows * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy", r.name);
}

// ... put in its place.  Every render and upload queued so far has run and the host's rows were the current ones (read back): nothing
// of `r` is in flight, and with the whole table on the device no row is pending any more.
template <class T>
void records_replace(DeviceRecords<T>& r)
{
    hipFree(r.d);
    r.d = r.resized.d;
    r.table.assign(r.resized.host.size(), r.init);
    r.table.host = std::move(r.resized.host);
    r.resized = {};
}

// f(table) for the batch's record tables in turn, until one refuses: samplers, envelopes, resamplers, filters, sweeps and, once they have
// been made (programs_made, filter_programs_made), the envelope programs and the filter programs.
template <class F>
bool each_voice_table(oalsfx_batch* b, F f)
{
    return f(b->samplers) && f(b->envelopes) && f(b->resamplers) && f(b->filters) && f(b->sweeps) && (!b->programs.d || f(b->programs)) &&
           (!b->filter_programs.d || f(b->filter_programs));
}

// A device buffer of the batch's that holds at least `elements` of its type (its contents are not kept).
template <class T>
bool grow_device(oalsfx_batch* b, T** buffer, size_t* capacity, size_t elements, const char* what)
{
    if (elements <= *capacity) return true;
    hipFree(*buffer);
    *buffer = nullptr;
    *capacity = 0;
    if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(buffer), elements * sizeof(T)), what)) return false;
    *capacity = elements;
    return true;
}

void release_slab(oalsfx_batch* b, size_t idx)
{
    if (b->h_rings[idx]) {
        b->pools[b->ring_floats[idx]].free_dirty.push_back(b->h_rings[idx]);
        b->h_rings[idx] = nullptr;
        b->ring_floats[idx] = 0;
    }
}

// Test and diagnostic switches: OALSFX_DEBUG_FLAGS (decimal or 0x...), or oalsfx_debug_set_flags for A/B runs inside one process.  The
// low byte travels to the kernels as flags >> 8.  Environment beside the flags: OALSFX_RING_MEMORY=default|finegrained|uncached (where
// delay lines, state and hot records live), OALSFX_HOST_PROFILE (what the host spends in prepare_params, printed by synchronize).
enum DebugFlag : int {
    kDbgAcquireAlways = 0x1,      // chained hand-over: every wavefront pays for the acquire behind its wait (tests/test_gpu_chained.py)
    kDbgAcquireNever = 0x2,       // ... none does (with 4: the negative control, results must come out wrong)
    kDbgReadEarly = 0x4,          // ... instance lines read before the turn has come
    kDbgGeneralOnly = 0x8,        // every reverb through the general kernel (scripts/ragged_bench.py)
    kDbgTapRound128 = 0x20,       // steady-state kernel: tap distances rounded to 128 bytes (timing only, results wrong)
    kDbgTapRound256 = 0x40,       // ... to 256 bytes
    kDbgChainLight = 0x80,        // batches without any reverb chain their calls too (measured slower: chain_eligible)
    kDbgNoCuMajor = 0x100,        // grids in plain workgroup order instead of CU-major (oalsfx_hip::kNoCuMajor)
    kDbgNoChain = 0x400,          // no chained launches: consecutive calls in plain stream order (bench.py --no-chain)
    kDbgGateSecondOnly = 0x800,   // the gate of chained launches in front of a run's second launch only (negative control: must fail)
    kDbgNoJoin = OALSFX_DEBUG_NO_JOIN, // 0x1000: chained launches as ever, but none takes the calls that arrive behind it (A/B runs)
    kDbgChainAlways = 0x8000,     // chained launches for short calls of small batches too (measured slower: chain_eligible)
    kDbgForceProven = 0x2000000,  // every reverb listed as proven steady, whatever the device said (the fault counter's test)
    kDbgHandOverBits = kDbgAcquireAlways | kDbgAcquireNever | kDbgReadEarly,
    kDbgKernelBits = 0xFF,        // what the kernels read
};
int debug_flags();

constexpr int kSettleFrames = OALSFX_RV_FADE_SAMPLES; // the cross-fade (128 frames) is over, and with it at least one call, whose end
                                                      // snaps the output gains to their targets (reference MixHelpers::mix)

// What the host remembers of a slot's parameters (a speed hint only: the kernels decide from the device state).
enum : uint8_t {
    kClassReverb = 1,  // reverb or EAX reverb
    kClassSteady = 2,  // parameters the steady-state kernel builds accept
    kClassClose = 4,   // shortest tap distance 64 .. kPlainMinTap - 1 samples, or an early tap / late-line offset under kPlainMinTapAhead (the HY builds)
    kClassShort = 8,   // shortest tap distance below 64 samples
    kClassModulated = 16,
};

uint8_t classify_slot(const oalsfx_slot_params& sp)
{
    if (sp.type != OALSFX_REVERB && sp.type != OALSFX_EAX_REVERB) return 0;
    const oalsfx_reverb_params& p = sp.u.reverb;
    uint8_t cls = kClassReverb | kClassSteady;
    const int sway = p.mod_depth != 0.0F ? 1 + static_cast<int>(std::abs(p.mod_depth)) : 0; // a modulated late line reads that much closer
    int lo = 1 << 30, lo_ahead = 1 << 30; // (lo_ahead: early taps and late-line offsets, kPlainMinTapAhead)
    for (int j = 0; j < 4; ++j) {
        // what the most general build of the steady-state kernel accepts: early / late taps and early-line offsets of any length,
        // all-pass offsets from four samples, late-line offsets from one tile
        if (p.early_tap[j] < 0 || p.early_ap_off[j] < 4 || p.early_line_off[j] < 0 || p.late_ap_off[j] < 4 ||
            p.late_line_off[j] < 64 + sway || p.late_tap[j] < p.late_feed_tap)
            cls &= static_cast<uint8_t>(~kClassSteady);
        lo = std::min({lo, p.early_tap[j], p.early_ap_off[j], p.early_line_off[j], p.late_tap[j] - p.late_feed_tap, p.late_ap_off[j], p.late_line_off[j]});
        lo_ahead = std::min({lo_ahead, p.early_tap[j], p.late_line_off[j]});
    }
    if (lo >= 64 && (lo < static_cast<int>(oalsfx_hip::kPlainMinTap) || lo_ahead < static_cast<int>(oalsfx_hip::kPlainMinTapAhead))) cls |= kClassClose;
    if (lo < 64) cls |= kClassShort;
    if (p.mod_depth != 0.0F) cls |= kClassModulated;
    return cls;
}

// Host-side belief about which reverb instances the steady-state kernel will fully process: they are listed first and go
// to that kernel, the others straight to the general kernel (a speed hint; the steady-state kernel decides on the device
// from the real state and falls back by itself).
bool reverb_settled(const oalsfx_batch* b, size_t idx)
{
    return (b->slot_class[idx] & kClassSteady) != 0 && (b->since_update[idx] >= kSettleFrames || b->xf_ok[idx]);
}

// Can the cross-fading build (reverb.hip, XF) take an instance from parameters `from` to parameters `to`?  Both tap sets must be ones
// the most general steady-state build accepts (classify_slot), the late taps counted from the *new* late feed position and the late
// line given the sway of whichever modulation is deeper.  A hint like the rest: the kernel checks against the device state and falls
// back by itself.
bool crossfade_followable(const oalsfx_reverb_params& from, const oalsfx_reverb_params& to)
{
    const int sway = (from.mod_depth != 0.0F || to.mod_depth != 0.0F) ? 1 + static_cast<int>(std::max(std::abs(from.mod_depth), std::abs(to.mod_depth))) : 0;
    for (const oalsfx_reverb_params* p : {&from, &to})
        for (int j = 0; j < 4; ++j)
            if (p->early_tap[j] < 0 || p->early_ap_off[j] < 4 || p->early_line_off[j] < 0 || p->late_tap[j] < to.late_feed_tap ||
                p->late_ap_off[j] < 4 || p->late_line_off[j] < 64 + sway)
                return false;
    return true;
}

// Is some reverb of the slot in a transition the cross-fading build follows?  (`settling` is short: the instances updated within the
// last 128 frames.)
bool slot_in_transition(const oalsfx_batch* b, int slot)
{
    for (size_t idx : b->settling)
        if (static_cast<int>(idx % b->slots) == slot && b->xf_ok[idx]) return true;
    return false;
}

void reclassify_slot(oalsfx_batch* b, size_t idx, int slot)
{
    const uint8_t before = b->slot_class[idx], after = classify_slot(b->h_params[idx]);
    b->n_close[slot] += ((after & kClassClose) != 0) - ((before & kClassClose) != 0);
    b->n_short[slot] += ((after & kClassShort) != 0) - ((before & kClassShort) != 0);
    if (after & kClassModulated) b->modulated[slot] = true;
    b->slot_class[idx] = after;
}

// After a mix: the slots that were updated recently move towards "steady"; the list order is stale once one arrives.
void advance_settling(oalsfx_batch* b, int frames)
{
    size_t keep = 0;
    for (size_t k = 0; k < b->settling.size(); ++k) {
        const size_t idx = b->settling[k];
        b->since_update[idx] = std::min(b->since_update[idx] + frames, kSettleFrames);
        if (b->since_update[idx] < kSettleFrames) { b->settling[keep++] = idx; continue; }
        b->in_settling[idx] = 0;
        b->xf_ok[idx] = 0;
        if (b->slot_class[idx] & kClassSteady) { b->lists_dirty = true; b->exact_wanted = true; }
    }
    b->settling.resize(keep);
}

// `chunks` zero-filled chunks of `count` delay-line slabs each, appended to `out`.  Where such a chunk lands in the card's memory is not
// the same everywhere: the reverb's ring traffic (48 streams per instance, a few hundred thousand in all) runs at one of three rates
// depending on the physical pages behind it, up to 15 % apart, about a third of the card each (scripts/vram_map.py,
// profiles/README.md) -- and the steady-state kernel follows the traffic-only probe to the microsecond
// (scripts/move_rings_probe.py).  So for chunks of 1 GiB and more the runtime does not take the first allocations it is given: it
// allocates candidates (all held, or the driver would hand the same pages out again), times the probe on each (k_ring_probe, which
// leaves the memory zero-filled), stops once it holds enough of the fastest kind and has seen a clearly slower one (or after
// 96 candidates -- four times the chunks wanted if that is more --, or half the free memory), keeps the fastest and frees the rest.  A few hundred milliseconds, once per
// batch.  OALSFX_PLACEMENT=0 switches the search off.
// What one launch hands to the next -- delay lines, effect state, hot records, send-filter histories, the turn words of chained launches
// -- lives, for a batch whose calls can be chained launches (chain_capable), in memory the L2s do not cache (hipDeviceMallocUncached): a
// wavefront's acknowledged stores are then in memory for every XCD to see, which is what lets consecutive calls overlap without a
// write-back of the L2 in between.  The kernels stream through this memory anyway: measured neutral on every workload
// (profiles/r03k_chained_launches/uncached_memory.txt: headline 42.9 / 43.1 / 42.4 us for default / fine-grained / uncached, the other
// BASELINE configurations within their noise).  Fine-grained memory is not enough: plain loads and stores of it are as stale across XCDs
// as those of ordinary memory (tests/test_gpu_chained.py fails on it).
// OALSFX_RING_MEMORY=default | finegrained | uncached forces one kind for every batch (comparisons; no chained launches unless uncached).
//
// Uncached memory is not given back to the runtime unless the process asks for it.  Round 3 found that uncached blocks freed with hipFree
// disturbed allocations made afterwards -- 512 bytes of zeros at the start of a page of a later batch's output, or a reverb instance off
// for a whole buffer -- and kept every block for the life of the process.  What round 4 established with the reproducer
// (scripts/uncached_free_hazard.py, profiles/r04b_uncached_free_hazard/):
//  - the buffer that reads wrong is the later batch's own staging buffer in *ordinary* memory (hipMalloc, the host-pointer entry point):
//    with the caller's buffers in device memory from another allocator (MODE=device) no run ever failed;
//  - its addresses do not lie in a range that was uncached before (hazard_trace.txt: 0 of 36 staging allocations), but the failing runs
//    are the ones whose staging buffers the runtime placed in the 8 MiB neighbourhood of the recycled uncached pages;
//  - nothing of this library is still in flight when a block is freed (every stream is waited for first, oalsfx_batch_destroy), and a
//    hipDeviceSynchronize directly in front of the hipFree changes nothing (hazard_modes.txt);
//  - with every uncached block a whole number of 2 MiB granules, and all of them freed, 4 of 4 runs were clean (granule.txt) -- but
//    with the small blocks in arenas that stay and only the delay lines freed, granules or not, it is back in 1 run of 4
//    (hazard_granules.txt): the size of the pieces is not the whole story.
// So: not a use after free of this library's, reproducible only through hipFree of hipDeviceMallocUncached memory followed by fresh
// ordinary allocations, and not understood further -- which is why the default stays "keep".  The blocks do come in 2 MiB granules now
// (small ones out of arenas of the pool's own: fewer runtime calls, and no 4 KiB uncached pieces among ordinary pages), what waits for
// reuse can be capped (OALSFX_UNCACHED_POOL_MAX_GIB: beyond it the largest waiting blocks are freed when a batch goes; unset: no limit),
// and oalsfx_trim_pools() frees everything that waits: for a process that needs the memory back and allocates nothing on the device
// afterwards that it cannot afford to check -- INTEGRATION.md says so.
class UncachedPool {
public:
    static constexpr size_t kGranule = size_t(2) << 20;
    static constexpr size_t kSmall = size_t(1) << 20; // blocks below this come out of arenas, 4 KiB apart
    hipError_t take(int device, size_t bytes, void** p)
    {
        if (bytes < kSmall) return take_small(device, bytes, p);
        bytes = (bytes + kGranule - 1) / kGranule * kGranule;
        {
            // the smallest block that is waiting, large enough and not more than twice as large (a process that goes through many batch
            // shapes then keeps a block per size class rather than per size)
            std::lock_guard<std::mutex> lock(mutex_);
            auto it = free_.lower_bound({device, bytes});
            if (it != free_.end() && it->first.first == device && it->first.second <= 2 * bytes) {
                *p = it->second;
                live_[*p] = it->first;
                waiting_ -= it->first.second;
                free_.erase(it);
                return hipSuccess;
            }
        }
        const hipError_t e = hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached);
        if (e == hipSuccess) {
            std::lock_guard<std::mutex> lock(mutex_);
            live_[*p] = {device, bytes};
        }
        return e;
    }
    bool give_back(void* p) // false: not one of ours
    {
        std::vector<void*> to_free;
        {
            std::lock_guard<std::mutex> lock(mutex_);
            auto sm = small_.find(p);
            if (sm != small_.end()) {
                Arena& a = arenas_[sm->second];
                small_.erase(sm);
                if (--a.live == 0) a.used = 0; // (a bump allocator per arena: the batches that shared it are gone, it starts over)
                return true;
            }
            auto it = live_.find(p);
            if (it == live_.end()) return false;
            free_.insert({it->second, p});
            waiting_ += it->second.second;
            live_.erase(it);
            shrink_locked(cap(), to_free);
        }
        release(to_free);
        return true;
    }
    // Frees what waits for reuse down to `keep_bytes` (largest blocks first) and every arena nobody uses.  Returns the bytes freed.
    size_t trim(size_t keep_bytes)
    {
        std::vector<void*> to_free;
        size_t before = 0;
        {
            std::lock_guard<std::mutex> lock(mutex_);
            before = waiting_;
            shrink_locked(keep_bytes, to_free);
            before -= waiting_;
            if (keep_bytes == 0) {
                for (auto& a : arenas_)
                    if (a.base && a.live == 0) { to_free.push_back(a.base); a.base = nullptr; before += kGranule; }
            }
        }
        release(to_free);
        return before;
    }
    size_t bytes_waiting()
    {
        std::lock_guard<std::mutex> lock(mutex_);
        return waiting_;
    }

private:
    struct Arena { int device; char* base; size_t used; int live; };
    static size_t cap()
    {
        static const size_t c = [] {
            const char* e = std::getenv("OALSFX_UNCACHED_POOL_MAX_GIB");
            const double gib = e ? std::atof(e) : -1.0; // (unset: nothing is freed behind the caller's back)
            return gib < 0.0 ? ~size_t(0) : static_cast<size_t>(gib * 1073741824.0);
        }();
        return c;
    }
    hipError_t take_small(int device, size_t bytes, void** p)
    {
        bytes = (bytes + 4095) / 4096 * 4096; // (every block on pages of its own, as the runtime hands them out)
        std::lock_guard<std::mutex> lock(mutex_);
        for (size_t k = 0; k < arenas_.size(); ++k) {
            Arena& a = arenas_[k];
            if (a.base && a.device == device && a.used + bytes <= kGranule) {
                *p = a.base + a.used;
                a.used += bytes;
                a.live += 1;
                small_[*p] = k;
                return hipSuccess;
            }
        }
        void* base = nullptr;
        const hipError_t e = hipExtMallocWithFlags(&base, kGranule, hipDeviceMallocUncached);
        if (e != hipSuccess) return e;
        size_t k = 0;
        while (k < arenas_.size() && arenas_[k].base) ++k;
        if (k == arenas_.size()) arenas_.push_back({});
        arenas_[k] = {device, static_cast<char*>(base), bytes, 1};
        *p = base;
        small_[*p] = k;
        return hipSuccess;
    }
    void shrink_locked(size_t keep_bytes, std::vector<void*>& to_free)
    {
        while (waiting_ > keep_bytes && !free_.empty()) {
            auto largest = free_.begin();
            for (auto it = free_.begin(); it != free_.end(); ++it)
                if (it->first.second > largest->first.second) largest = it;
            waiting_ -= largest->first.second;
            to_free.push_back(largest->second);
            free_.erase(largest);
        }
    }
    static void release(const std::vector<void*>& blocks)
    {
        // (nothing of the library still uses a block that waits; the synchronisation is for whatever else the process has queued)
        if (blocks.empty()) return;
        (void)hipDeviceSynchronize();
        for (void* q : blocks) (void)hipFree(q);
    }
    std::mutex mutex_;
    std::multimap<std::pair<int, size_t>, void*> free_;
    std::map<void*, std::pair<int, size_t>> live_;
    std::vector<Arena> arenas_;
    std::map<void*, size_t> small_; // small block -> its arena
    size_t waiting_ = 0;
};

UncachedPool& uncached_pool()
{
    static UncachedPool* pool = new UncachedPool; // (never destroyed: batches may outlive static destruction order)
    return *pool;
}

// Does this runtime hand out uncached device memory at all?  Asked once per device; where it does not, batches keep everything in
// ordinary memory and their calls in stream order.
bool uncached_memory_available(int device)
{
    static std::mutex m;
    static std::map<int, bool> known;
    std::lock_guard<std::mutex> lock(m);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    // The hand-over between launches that run at the same time (reverb.hip) rests on how this part's caches behave -- an acknowledged
    // store to uncached memory is in memory for every XCD, a launch starts with empty vector L1s, HW_REG_XCC_ID names the XCD -- and has
    // been validated on gfx950 only: any other device keeps its calls in stream order (ADVICE, round 3).
    hipDeviceProp_t prop{};
    bool ok = hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    if (ok) {
        void* p = nullptr;
        ok = uncached_pool().take(device, 4096, &p) == hipSuccess;
        if (ok) uncached_pool().give_back(p);
        else (void)hipGetLastError();
    }
    known[device] = ok;
    return ok;
}

hipError_t handed_on_malloc(const oalsfx_batch* b, void** p, size_t bytes)
{
    const char* kind = std::getenv("OALSFX_RING_MEMORY");
    if (kind && std::strcmp(kind, "finegrained") == 0) return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained);
    if (kind && std::strcmp(kind, "default") == 0) return hipMalloc(p, bytes);
    if (b->uncached || (kind && std::strcmp(kind, "uncached") == 0)) return uncached_pool().take(b->device, bytes, p);
    return hipMalloc(p, bytes);
}

void handed_on_free(void* p)
{
    if (p && !uncached_pool().give_back(p)) (void)hipFree(p);
}

bool place_ring_chunks(oalsfx_batch* b, int chunks, int count, size_t slab_floats, std::vector<float*>& out)
{
    if (chunks <= 0) return true;
    const size_t bytes = static_cast<size_t>(count) * slab_floats * sizeof(float);
    struct Candidate { void* p; double us; };
    std::vector<Candidate> cands;
    size_t free_b = 0, total_b = 0;
    // OALSFX_PLACEMENT=0 switches the search off (a process that shares the card with other allocators: the candidates are held until
    // the search ends); OALSFX_PLACEMENT_MAX_GIB caps what it may hold at once (default: half of the free memory)
    const char* env_on = std::getenv("OALSFX_PLACEMENT");
    const char* env_cap = std::getenv("OALSFX_PLACEMENT_MAX_GIB");
    const bool wanted = bytes >= (static_cast<size_t>(3) << 28) && slab_floats >= 65536 && !(env_on && std::atoi(env_on) == 0);
    // one search at a time in a process: each budgets against the free memory it sees when it starts
    static std::mutex placement_mutex;
    std::unique_lock<std::mutex> placement_lock(placement_mutex, std::defer_lock);
    if (wanted) placement_lock.lock();
    size_t budget = 0;
    if (wanted && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        budget = free_b / 2;
        if (env_cap && std::atof(env_cap) > 0.0) budget = std::min(budget, static_cast<size_t>(std::atof(env_cap) * 1073741824.0));
    }
    const bool search = wanted && budget > bytes * (static_cast<size_t>(chunks) + 1);
    if (!search) {
        for (int k = 0; k < chunks; ++k) {
            void* p = nullptr;
            bool ok = b->hip_ok(handed_on_malloc(b, &p, bytes), "hipMalloc(rings)");
            if (ok) cands.push_back({p, 0.0});
            ok = ok && b->hip_ok(hipMemsetAsync(p, 0, bytes, b->stream), "hipMemsetAsync(rings)");
            if (!ok) {
                for (auto& c : cands) handed_on_free(c.p);
                return false;
            }
        }
    } else {
        const size_t max_tries = std::min<size_t>(std::max<size_t>(96, static_cast<size_t>(chunks) * 4), budget / bytes);
        const int waves_per_slab = std::max(1, 4096 / count); // a full load (4096 wavefronts) whatever the chunk's size
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (!b->hip_ok(hipEventCreate(&e0), "hipEventCreate") || !b->hip_ok(hipEventCreate(&e1), "hipEventCreate")) return false;
        bool ok = true;
        while (cands.size() < max_tries) {
            void* c = nullptr;
            if (handed_on_malloc(b, &c, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
            cands.push_back({c, 1e30});
            if (!(ok = b->hip_ok(hipMemsetAsync(c, 0, bytes, b->stream), "hipMemsetAsync(rings)"))) break;
            for (int r = 0; r < 2; ++r) oalsfx_hip::launch_ring_probe(static_cast<float*>(c), count, slab_floats, 256u * r, waves_per_slab, b->stream);
            hipEventRecord(e0, b->stream);
            for (int r = 0; r < 4; ++r) oalsfx_hip::launch_ring_probe(static_cast<float*>(c), count, slab_floats, 256u * (2 + r), waves_per_slab, b->stream);
            hipEventRecord(e1, b->stream);
            float ms = 0.0F;
            if (!(ok = b->hip_ok(hipEventSynchronize(e1), "hipEventSynchronize") && b->hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime"))) break;
            cands.back().us = ms * 1e3 / 4;
            b->placement_candidates += 1;
            if (cands.size() < std::min<size_t>(max_tries, static_cast<size_t>(chunks) * 3 + 4)) continue; // a fair sample first
            std::vector<double> us;
            for (const auto& c2 : cands) us.push_back(c2.us);
            std::sort(us.begin(), us.end());
            // enough candidates of the fastest kind in hand, and a clearly slower kind seen next to them: done
            if (us[chunks - 1] <= us[0] * 1.04 && us[0] * 1.12 <= us.back()) break;
        }
        hipEventDestroy(e0); hipEventDestroy(e1);
        std::stable_sort(cands.begin(), cands.end(), [](const Candidate& x, const Candidate& y) { return x.us < y.us; });
        if (!ok || static_cast<int>(cands.size()) < chunks) {
            for (auto& c : cands) handed_on_free(c.p);
            return ok ? b->fail("hipMalloc(rings) failed") : false;
        }
        for (size_t k = chunks; k < cands.size(); ++k) handed_on_free(cands[k].p);
        b->placement_worst_us = std::max(b->placement_worst_us, cands.back().us);
        cands.resize(chunks);
        b->placement_best_us = cands.front().us;
        // (address order within the batch: consecutive instances then sit in consecutive slabs of consecutive chunks)
        std::sort(cands.begin(), cands.end(), [](const Candidate& x, const Candidate& y) { return x.p < y.p; });
    }
    for (auto& c : cands) {
        b->placed_chunks += 1;
        b->chunks.push_back(c.p);
        b->ring_chunks.push_back({static_cast<char*>(c.p), bytes, c.p});
        out.push_back(static_cast<float*>(c.p));
    }
    return true;
}

// Every size class of `need` (size class -> slabs wanted) holds at least that many free slabs afterwards: the pool grows by zero-filled
// chunks where it has fewer.
bool grow_ring_pools(oalsfx_batch* b, const std::map<size_t, int>& need)
{
    for (auto& kv : need) {
        RingPool& pool = b->pools[kv.first];
        pool.slab_floats = kv.first;
        const int have = static_cast<int>(pool.free_clean.size() + pool.free_dirty.size());
        const int grow = kv.second - have;
        if (grow > 0) {
            // chunks of at most 1024 slabs (0.9 GiB of reverb delay lines), each placed on its own (place_ring_chunk); the slabs are
            // handed out in address order within a chunk, chunk after chunk, so that consecutive instances get consecutive slabs
            constexpr int kChunkSlabs = 1024; // 0.9 GiB of reverb delay lines
            std::vector<float*> bases;
            if (!place_ring_chunks(b, grow / kChunkSlabs, kChunkSlabs, kv.first, bases)) return false;
            const size_t full = bases.size();
            if (grow % kChunkSlabs && !place_ring_chunks(b, 1, grow % kChunkSlabs, kv.first, bases)) return false;
            std::vector<float*> fresh;
            for (size_t c = 0; c < bases.size(); ++c) {
                const int count = c < full ? kChunkSlabs : grow % kChunkSlabs;
                for (int k = 0; k < count; ++k) fresh.push_back(bases[c] + static_cast<size_t>(k) * kv.first);
            }
            for (size_t k = fresh.size(); k-- > 0;) pool.free_clean.push_back(fresh[k]);
        }
    }
    return true;
}

// Pinned staging buffer for one round of parameter uploads: four take turns, and a buffer is reused only once the launch that
// read it has run.
oalsfx_batch::Stage* acquire_stage(oalsfx_batch* b, size_t bytes)
{
    // the first buffer, oldest first, whose launch has run (a query: waiting for an event, however old, makes the host wait for
    // everything that is queued on this stack); only if all four are still being read does the host wait for the oldest
    int pick = -1;
    for (int k = 0; k < 4 && pick < 0; ++k) {
        oalsfx_batch::Stage& c = b->stage[(b->stage_turn + k) & 3];
        if (!c.pending || hipEventQuery(c.done) == hipSuccess) pick = (b->stage_turn + k) & 3;
    }
    if (pick < 0) {
        pick = b->stage_turn;
        const auto w0 = std::chrono::steady_clock::now();
        if (!b->hip_ok(hipEventSynchronize(b->stage[pick].done), "hipEventSynchronize")) return nullptr;
        b->host_stage_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - w0).count();
    }
    oalsfx_batch::Stage& st = b->stage[pick];
    b->stage_turn = (pick + 1) & 3;
    st.pending = false;
    if (!st.done && !b->hip_ok(hipEventCreateWithFlags(&st.done, hipEventDisableTiming), "hipEventCreate")) return nullptr;
    if (bytes > st.capacity) {
        if (st.host) (void)hipHostFree(st.host);
        if (st.dev) (void)hipFree(st.dev);
        st.host = st.dev = nullptr;
        st.capacity = 0;
        const size_t cap = std::max<size_t>(bytes * 2, 1 << 20);
        if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&st.host), cap), "hipHostMalloc(staging)")) return nullptr;
        if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&st.dev), cap), "hipMalloc(staging)")) return nullptr;
        st.capacity = cap;
    }
    return &st;
}

// Folds all pending property changes into descriptors, device state and the launch plan: what the
// reference does lazily at the top of mix_data (update_context_sources, src/oalsfxpp.cpp:3397-3412)
// plus EffectSlot::set_effect's state re-creation (src/oalsfxpp.cpp:2688-2709).
// In two steps: prepare_params does the host's part and packs the staging buffer; launch_params puts it in place on a stream.
// (sync_params: both, on the batch's own stream, without waiting for it; `consumer` -- the stream the next launches go to -- is made to
// wait for the uploads with an event when it is a different stream.  mix_device looks at what was prepared before it decides where the
// call's launches go: chained launches.)
struct PendingUpload {
    bool any = false;                  // something had changed
    oalsfx_batch::Stage* st = nullptr; // nullptr: nothing to upload
    size_t bytes = 0;
    bool direct = true;                // read by the kernel straight from the page-locked buffer
    bool chainable = true;             // only records that can take their turn instance by instance (slot parameters, epochs) and lists
    oalsfx_hip::UploadJobs jobs{};
};

bool chain_join(oalsfx_batch* b);
void join_flush(oalsfx_batch* b);

bool prepare_params(oalsfx_batch* b, PendingUpload& pu)
{
    if (b->dirty_list.empty() && !b->lists_dirty) return true;
    pu.any = true;
    const size_t total = static_cast<size_t>(b->n) * b->slots;
    std::map<size_t, int> need; // size class -> slabs needed
    std::vector<size_t> restarted;
    std::vector<int> up_params, up_state, up_source, up_touched; // indices of the records to upload
    std::vector<uint32_t> up_epoch;                  // new epochs of the instances in up_touched
    bool any_type_change = false;
    if (!b->dirty_list.empty()) b->upload_gen += 1;

    // a caller's stream may still be running kernels that read what is about to be overwritten
    if (b->last_launch_stream && b->last_launch_stream != b->stream) {
        if (!b->hip_ok(hipStreamWaitEvent(b->stream, b->ev_mixed, 0), "hipStreamWaitEvent")) return false;
    }

    const auto hd0 = std::chrono::steady_clock::now();
    for (int i : b->dirty_list) {
        InstanceHost& h = b->inst[i];
        bool updated = false, sends_moved = false;
        for (int s = 0; s < b->slots; ++s) {
            if (!h.slot_changed[s]) continue;
            h.slot_changed[s] = false;
            updated = true;
            sends_moved |= h.slot_retyped[s]; // (the send to a slot depends on what the slot holds: nothing, or an effect)
            const size_t idx = static_cast<size_t>(i) * b->slots + s;
            oalsfx_slot_params& p = b->h_params[idx];
            // a settled reverb whose properties change without a change of type keeps its state and cross-fades: what the XF build follows
            const bool was_settled = (b->slot_class[idx] & kClassSteady) != 0 && b->since_update[idx] >= kSettleFrames && !h.slot_retyped[s];
            const oalsfx_reverb_params before = p.u.reverb;
            derive_slot(b->dev, h.active[s], p);
            p.update_seq = ++b->seq[idx];
            up_params.push_back(static_cast<int>(idx));
            reclassify_slot(b, idx, s);
            if (h.slot_retyped[s]) b->mod_ever[idx] = 0;
            if (b->slot_class[idx] & kClassModulated) b->mod_ever[idx] = 1;
            b->xf_ok[idx] = was_settled && (b->slot_class[idx] & kClassSteady) != 0 && b->channels <= 2 && crossfade_followable(before, p.u.reverb);
            b->lists_dirty = true; // (it leaves the proven part of its list, or the steady part altogether)
            b->since_update[idx] = 0;
            if ((b->slot_class[idx] & kClassReverb) && !b->in_settling[idx]) {
                b->in_settling[idx] = 1;
                b->settling.push_back(idx);
            }
            if (h.slot_retyped[s]) {
                h.slot_retyped[s] = false;
                any_type_change = true;
                reset_slot_state(p.type, b->h_state_init[idx]);
                b->h_state_init[idx].seen_seq = p.update_seq - 1;
                up_state.push_back(static_cast<int>(idx));
                restarted.push_back(idx);
                b->started_at[idx] = b->frames_total;
                b->off_grid_known = false;
                release_slab(b, idx);
                const size_t floats = static_cast<size_t>(ring_floats_for(p.type, b->rate));
                if (floats) need[floats] += 1;
            }
        }
        if (h.source_changed) {
            h.source_changed = false;
            updated = true;
            sends_moved = true;
        }
        // The reference recomputes a source's sends whenever one of its slots' properties changed (update_context_sources,
        // src/oalsfxpp.cpp:3397-3412); their inputs -- send properties, which slots hold an effect -- did not move when only an effect's
        // own properties did, and the result is the same record: derived and uploaded only when they did, or when an aux send was
        // written since the last derivation (aux_written: one set back to (1, 1, 1) leaves source_changed clear).
        if (updated && (sends_moved || b->aux_written[i])) {
            b->aux_written[i] = 0;
            int types[OALSFX_MAX_SLOTS] = {};
            for (int s = 0; s < b->slots; ++s) types[s] = static_cast<int>(h.active[s].type_);
            oalsfx_source_params& sp = b->h_source[i];
            auto has_filter = [&](const oalsfx_source_params& x) {
                int any = x.direct.filter_type;
                for (int s = 0; s < b->slots; ++s)
                    if (x.aux[s].out_channels != 0) any |= x.aux[s].filter_type;
                return any != OALSFX_AF_NONE;
            };
            const bool before = has_filter(sp);
            derive_source(b->dev, b->slots, h.direct_props, h.aux_props, types, sp);
            b->n_filtered += static_cast<int>(has_filter(sp)) - static_cast<int>(before);
            b->inst_filtered[i] = has_filter(sp) ? 1 : 0;
            b->inside_version = ~0u;
            up_source.push_back(i);
        }
        if (updated) {
            up_touched.push_back(i);
            // whatever the device knew about this instance is out of date: its hot records (new epoch) and the proof that its reverbs
            // are steady (a send change alone leaves them steady, which the next read-back will confirm)
            up_epoch.push_back(++b->inst_epoch[i]);
            for (int s = 0; s < b->slots; ++s) {
                const size_t idx = static_cast<size_t>(i) * b->slots + s;
                if (b->proven[idx]) { b->proven[idx] = 0; b->lists_dirty = true; }
                b->updated_gen[idx] = b->upload_gen;
            }
            b->exact_wanted = true;
        }
        b->inst_dirty[i] = 0;
    }
    b->dirty_list.clear();
    b->host_derive_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - hd0).count();

    // slots that start over take and give back delay lines, which launches of a run of chained launches may still be at work on
    if (!restarted.empty() && !chain_join(b)) return false;

    // ring slabs: grow each size class once, zero fresh chunks in one memset
    if (!grow_ring_pools(b, need)) return false;
    bool rings_changed = b->rings_table_dirty;
    b->rings_table_dirty = false;
    for (size_t idx : restarted) {
        const size_t floats = static_cast<size_t>(ring_floats_for(b->h_params[idx].type, b->rate));
        rings_changed = true; // the slab it held is gone from the table in any case
        if (!floats) continue;
        RingPool& pool = b->pools[floats];
        float* slab = nullptr;
        if (!pool.free_clean.empty()) {
            slab = pool.free_clean.back();
            pool.free_clean.pop_back();
        } else {
            slab = pool.free_dirty.back();
            pool.free_dirty.pop_back();
            if (!b->hip_ok(hipMemsetAsync(slab, 0, floats * sizeof(float), b->stream), "hipMemsetAsync(ring)")) return false;
        }
        b->h_rings[idx] = slab;
        b->ring_floats[idx] = floats;
    }

    // ---- the launch plan: one counting sort over the slots of every instance ----
    const bool rebuild_lists = any_type_change || b->lists_dirty;
    const auto hl0 = std::chrono::steady_clock::now();
    std::vector<int> lists;
    if (rebuild_lists) {
        lists.resize(total);
        // ring-light types, then the reverbs of both types: proven steady by kind (the FP build each needs: plain, close taps, short taps or
        // modulated), believed steady or in a transition the XF build follows, the others
        constexpr int kFast = OALSFX_REVERB, kSlow = OALSFX_REVERB + 3, kGeneral = OALSFX_REVERB + 4, kBuckets = OALSFX_REVERB + 5;
        std::vector<uint8_t> bucket_of(b->n);
        const bool force = (debug_flags() & kDbgForceProven) != 0; // test of the fault path only: every reverb counts as proven
        for (int s = 0; s < b->slots; ++s) {
            // one pass over the slot's instances: bucket, type counts, and the shortest block (in tiles) that leaves the gains of every
            // proven instance of the slot alone (calls whose last block is shorter do not take the FP builds)
            int count[kBuckets] = {};
            b->list_count[s][OALSFX_REVERB] = b->list_count[s][OALSFX_EAX_REVERB] = 0;
            b->rest_tiles[s] = 0;
            for (int i = 0; i < b->n; ++i) {
                const size_t idx = static_cast<size_t>(i) * b->slots + s;
                const int t = b->h_params[idx].type;
                int k = t;
                if (t >= OALSFX_REVERB) {
                    b->list_count[s][t] += 1;
                    const uint8_t cls = b->slot_class[idx];
                    if (!force && !reverb_settled(b, idx)) k = kGeneral;
                    else if (!force && !b->proven[idx]) k = kSlow;
                    else {
                        k = kFast + (((cls & kClassShort) || b->mod_ever[idx]) ? 2 : (cls & kClassClose) ? 1 : 0);
                        b->rest_tiles[s] = std::max<int>(b->rest_tiles[s], b->proven[idx]);
                    }
                }
                bucket_of[i] = static_cast<uint8_t>(k);
                count[k] += 1;
            }
            int start[kBuckets];
            int off = s * b->n;
            for (int k = 0; k < kBuckets; ++k) { start[k] = off; off += count[k]; }
            for (int t = 0; t < OALSFX_REVERB; ++t) { b->list_offset[s][t] = start[t]; b->list_count[s][t] = count[t]; }
            for (int t = 0; t < 2; ++t) b->list_offset[s][OALSFX_REVERB + t] = start[kFast]; // the reverb region as a whole (the two types interleave)
            b->steady_offset[s] = start[kFast];
            for (int k = 0; k < 3; ++k) b->kind_count[s][k] = count[kFast + k];
            b->fast_count[s] = count[kFast] + count[kFast + 1] + count[kFast + 2];
            b->slow_count[s] = count[kSlow];
            b->general_offset[s] = start[kGeneral];
            b->general_count[s] = count[kGeneral];
            int fill[kBuckets];
            for (int k = 0; k < kBuckets; ++k) fill[k] = start[k];
            for (int i = 0; i < b->n; ++i) lists[fill[bucket_of[i]]++] = i;
            // a proven part that is simply a range of instances needs no list on the device
            b->fast_first[s] = b->fast_count[s] > 0 ? lists[start[kFast]] : -1;
            for (int k = 1; k < b->fast_count[s]; ++k)
                if (lists[start[kFast] + k] != b->fast_first[s] + k) { b->fast_first[s] = -1; break; }
        }
        b->lists_dirty = false;
        b->h_lists = lists;
        b->lists_version += 1;
    }

    b->host_lists_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - hl0).count();
    // ---- one packed upload: [indices | records] per array, the ring table, the lists ----
    auto padded = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
    const size_t n_p = up_params.size(), n_s = up_state.size(), n_src = up_source.size(), n_t = up_touched.size();
    size_t off = 0;
    const size_t o_pi = off; off += padded(n_p * sizeof(int));
    const size_t o_pr = off; off += padded(n_p * sizeof(oalsfx_slot_params));
    const size_t o_si = off; off += padded(n_s * sizeof(int));
    const size_t o_sr = off; off += padded(n_s * sizeof(oalsfx_hip::SlotStateLines)); // (records in whole lines, as they lie in device memory)
    const size_t o_ci = off; off += padded(n_src * sizeof(int));
    const size_t o_cr = off; off += padded(n_src * sizeof(oalsfx_source_params));
    const size_t o_ti = off; off += padded(n_t * sizeof(int));
    const size_t o_ep = off; off += padded(n_t * sizeof(uint32_t));
    const size_t o_rt = off; off += rings_changed ? padded(total * sizeof(float*)) : 0;
    const size_t o_li = off; off += rebuild_lists ? padded(total * sizeof(int)) : 0;
    if (off > 0) {
        oalsfx_batch::Stage* st = acquire_stage(b, off);
        if (!st) return false;
        if (n_p) std::memcpy(st->host + o_pi, up_params.data(), n_p * sizeof(int));
        for (size_t k = 0; k < n_p; ++k) std::memcpy(st->host + o_pr + k * sizeof(oalsfx_slot_params), &b->h_params[up_params[k]], sizeof(oalsfx_slot_params));
        if (n_s) std::memcpy(st->host + o_si, up_state.data(), n_s * sizeof(int));
        for (size_t k = 0; k < n_s; ++k) std::memcpy(st->host + o_sr + k * sizeof(oalsfx_hip::SlotStateLines), &b->h_state_init[up_state[k]], sizeof(oalsfx_slot_state));
        if (n_src) std::memcpy(st->host + o_ci, up_source.data(), n_src * sizeof(int));
        for (size_t k = 0; k < n_src; ++k) std::memcpy(st->host + o_cr + k * sizeof(oalsfx_source_params), &b->h_source[up_source[k]], sizeof(oalsfx_source_params));
        if (n_t) std::memcpy(st->host + o_ti, up_touched.data(), n_t * sizeof(int));
        if (n_t) std::memcpy(st->host + o_ep, up_epoch.data(), n_t * sizeof(uint32_t));
        if (rings_changed) std::memcpy(st->host + o_rt, b->h_rings.data(), total * sizeof(float*));
        if (rebuild_lists) std::memcpy(st->host + o_li, lists.data(), total * sizeof(int));
        // Small uploads (parameter changes while streaming) are read by the kernels straight from the page-locked staging buffer: a
        // copy-engine transfer between two kernels of one stream is ordered through the host on this stack and started ~90 us after
        // the kernel before it had ended (rocprofv3 trace of scripts/update_storm_bench.py), with the host waiting for it a step later.
        // Bulk uploads (creation of a batch) keep the transfer.
        const bool direct = off <= (static_cast<size_t>(1) << 20);
        const char* from = direct ? st->host : st->dev;
        // one launch puts everything in place
        auto words = [&](size_t o) { return reinterpret_cast<const unsigned*>(from + o); };
        auto ints = [&](size_t o) { return reinterpret_cast<const int*>(from + o); };
        if (rebuild_lists) b->d_lists = b->d_lists_buf[b->lists_turn = (b->lists_turn + 1) % (kChainDepth + 1)]; // (launches in flight keep the list they were given)
        oalsfx_hip::UploadJobs& jobs = pu.jobs;
        jobs = oalsfx_hip::UploadJobs{};
        // (slot parameters and epochs take their turn instance by instance when the upload runs beside the launch before it)
        jobs.scatter[0] = {reinterpret_cast<unsigned*>(b->d_params), words(o_pr), ints(o_pi), static_cast<int>(sizeof(oalsfx_slot_params) / 4), static_cast<int>(n_p), 1};
        jobs.scatter[1] = {reinterpret_cast<unsigned*>(b->d_state), words(o_sr), ints(o_si), static_cast<int>(sizeof(oalsfx_hip::SlotStateLines) / 4), static_cast<int>(n_s), 0};
        jobs.scatter[2] = {reinterpret_cast<unsigned*>(b->d_source), words(o_cr), ints(o_ci), static_cast<int>(sizeof(oalsfx_source_params) / 4), static_cast<int>(n_src), 0};
        jobs.scatter[3] = {reinterpret_cast<unsigned*>(b->d_inst_epoch), words(o_ep), ints(o_ti), 1, static_cast<int>(n_t), 1};
        jobs.copy[0] = {reinterpret_cast<unsigned*>(b->d_rings), words(o_rt), rings_changed ? total * (sizeof(float*) / 4) : 0, 0};
        jobs.copy[1] = {reinterpret_cast<unsigned*>(b->d_lists), words(o_li), rebuild_lists ? total : 0, 0};
        pu.st = st;
        pu.bytes = off;
        pu.direct = direct;
        pu.chainable = direct && n_s == 0 && n_src == 0 && !rings_changed && need.empty();
    }
    return true;
}

// `turn` / `turn_wait`: the upload runs beside a chained launch that may still be at work (see UploadJobs).
bool launch_params(oalsfx_batch* b, PendingUpload& pu, hipStream_t upload_stream, hipStream_t consumer, const unsigned* turn = nullptr, unsigned turn_wait = 0)
{
    if (pu.st) {
        oalsfx_batch::Stage* st = pu.st;
        pu.st = nullptr;
        if (!pu.direct && !b->hip_ok(hipMemcpyAsync(st->dev, st->host, pu.bytes, hipMemcpyHostToDevice, upload_stream), "hipMemcpyAsync(parameters)")) return false;
        pu.jobs.turn = turn;
        pu.jobs.turn_wait = turn_wait;
        pu.jobs.fault = b->d_fault;
        oalsfx_hip::launch_upload(pu.jobs, upload_stream);
        // the staging buffer is free again once everything that reads it has run
        if (!b->hip_ok(hipEventRecord(st->done, upload_stream), "hipEventRecord")) return false;
        st->pending = true;
        if (!b->hip_ok(hipGetLastError(), "parameter upload")) return false;
    }
    // a launch stream other than the one the uploads ran on must see them
    if (pu.any && consumer && consumer != upload_stream) {
        if (!b->hip_ok(hipEventRecord(b->ev_uploaded, upload_stream), "hipEventRecord")) return false;
        if (!b->hip_ok(hipStreamWaitEvent(consumer, b->ev_uploaded, 0), "hipStreamWaitEvent")) return false;
    }
    return true;
}

bool sync_params(oalsfx_batch* b, hipStream_t consumer)
{
    PendingUpload pu;
    return prepare_params(b, pu) && launch_params(b, pu, b->stream, consumer);
}

bool ensure_mixbuf(oalsfx_batch* b)
{
    if (b->d_mixbuf || b->slots == 1) return true;
    const size_t bytes = static_cast<size_t>(b->n) * b->channels * OALSFX_MAX_CHUNK * sizeof(float);
    // (handed from the reverb-free slots' launch to the reverbs' in a chained step: with the rest of what launches hand on)
    return b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_mixbuf), bytes), "hipMalloc(mixbuf)");
}

std::atomic<int> g_debug_flags{-1}; // process-wide, read by every batch on whatever host thread drives it
int debug_flags()
{
    int f = g_debug_flags.load(std::memory_order_relaxed);
    if (f < 0) {
        const char* env = std::getenv("OALSFX_DEBUG_FLAGS");
        f = env ? static_cast<int>(std::strtol(env, nullptr, 0)) & 0x7FFFFFFF : 0; // decimal or 0x...
        g_debug_flags.store(f, std::memory_order_relaxed);
    }
    return f;
}

// Brackets one kernel launch with events recorded on its stream.  (Events attached to the launch itself through
// hipExtLaunchKernel were tried: they read 5-6 us longer than rocprofv3's kernel trace of the same run, these 1-2 us.)
struct ScopedTiming {
    oalsfx_batch* b; hipStream_t stream; TimedLaunch tl{};
    ScopedTiming(oalsfx_batch* b_, int type, hipStream_t s) : b(b_), stream(s)
    {
        if (!b->timing) return;
        tl.start = b->take_event();
        tl.stop = b->take_event();
        tl.type = type;
        hipEventRecord(tl.start, stream);
    }
    ~ScopedTiming()
    {
        if (!b->timing) return;
        hipEventRecord(tl.stop, stream);
        b->timed.push_back(tl);
    }
};

constexpr size_t kTimelineBytes = (64 * 4 + 64) * 96 * sizeof(unsigned long long); // 64 sampled workgroups x 4 waves x 96 stamps (steady-state kernel) + 64 sampled instances x 96 (general path)
constexpr int kTimedGeneralOffset = 16; // TimedLaunch::type of a reverb type's general-kernel launches
constexpr int kTimedWaveEffects = -1; // TimedLaunch::type of the merged launch for the ring-light effect types
constexpr int kTimedMixed = -2;       // ... of the grid that serves ring-light effects and steady reverbs of a slot together

// TimedLaunch::type of the launches a caller means by an effect type (oalsfx_batch_kernel_timing_read).
int timed_key(int effect_type)
{
    // the ring-light types share one launch per slot: asking for any of them reads that launch
    int key = (effect_type >= 0 && effect_type < OALSFX_REVERB) ? kTimedWaveEffects : effect_type;
    // the two reverb types share their launches
    if (key == OALSFX_REVERB) key = OALSFX_EAX_REVERB;
    if (key == OALSFX_EAX_REVERB + kTimedGeneralOffset) key = OALSFX_REVERB + kTimedGeneralOffset;
    if (effect_type == 32) key = kTimedMixed;
    return key;
}

// Can the steady-state kernel be used for this chunk at all?
bool steady_kernel_usable(const KernelCtx& ctx) { return ctx.frames >= 1 && !(debug_flags() & kDbgGeneralOnly); } // any call size: a short call is one partial tile

// Does some reverb of the slot write its delay lines off the 128-byte line grid?  (Recounted after a call that was not a multiple of 32
// frames and after a slot restarted: every position moves with every call, by the same amount.)
bool slot_off_grid(oalsfx_batch* b, int slot)
{
    if (!b->off_grid_known) {
        for (int s = 0; s < b->slots; ++s) b->off_grid[s] = 0;
        const size_t total = static_cast<size_t>(b->n) * b->slots;
        for (size_t idx = 0; idx < total; ++idx)
            if ((b->slot_class[idx] & kClassReverb) && ((b->frames_total - b->started_at[idx]) & 31u) != 0u) b->off_grid[idx % b->slots] += 1;
        b->off_grid_known = true;
    }
    return b->off_grid[slot] > 0;
}

// One steady-state launch for steady instances of both reverb types (adjacent in the list; the kernel reads the type per
// instance): the proven ones (`proven`: the builds without steady-state test and general path), the believed ones, or both
// together through the believing builds.
void launch_reverb_steady_part(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, int offset, int count, bool proven, hipStream_t stream)
{
    const int* list = b->d_lists + offset;
    // Mono / stereo: one launch, an instance that turns out not to be steady falls back inside it.  More than two channels:
    // the steady-state kernel notes per instance whether it took it, and the general kernel right behind it does the others.
    // (A chunk that is not a whole number of 64-frame tiles ends in a partial tile inside the steady-state kernel.)
    const bool hand_over = ctx.channels > 2;
    KernelCtx c = ctx;
    c.progress = hand_over ? b->d_progress : nullptr;
    c.list_first = proven ? b->fast_first[slot] : -1;
    // the proven-steady instances lead the steady region of the list: in a call of whole tiles (what "proven" vouches for) the
    // general kernel need not look at them
    // (whose last, shortest block is long enough for the gains of all of them to be at rest)
    const int n = ctx.frames;
    const bool vouched = (n & 63) == 0 && (n - ((n - 1) / OALSFX_RV_MAX_UPDATE) * OALSFX_RV_MAX_UPDATE) / 64 >= b->rest_tiles[slot];
    const int lead = hand_over && vouched ? std::max(0, std::min(count, b->steady_offset[slot] + b->fast_count[slot] - offset)) : 0;
    c.no_follow_up = lead;
    {
        ScopedTiming timing(b, OALSFX_EAX_REVERB, stream);
        int groups = 0;
        const char* name = oalsfx_hip::launch_reverb_steady(c, slot, list, count, flags | ((debug_flags() & kDbgKernelBits) << 8), b->n_close[slot] > 0,
                                                            b->modulated[slot], b->n_short[slot] > 0, proven, !proven && slot_in_transition(b, slot), stream, &groups,
                                                            proven && slot_off_grid(b, slot));
        if (name) b->last_steady_kernel = name;
        b->launched_groups += groups;
    }
    if (hand_over && count > lead) {
        ScopedTiming timing(b, OALSFX_REVERB + kTimedGeneralOffset, stream);
        oalsfx_hip::launch_reverb_general(c, slot, list + lead, count - lead, flags, stream);
    }
}

// Mono / stereo, whole tiles: every steady reverb of the slot in one launch, each kind on the build it needs (the proven ones by their
// taps: plain, HY or ST FP build; the believed ones and those in a transition the XF build follows on that build).  `proven_usable`:
// the call's last block leaves the gains of the proven instances at rest; otherwise they go with the believed ones for this call (the
// XF build ramps gains).
void steady_kind_counts(const oalsfx_batch* b, int slot, bool proven_usable, int counts[4])
{
    counts[0] = counts[1] = counts[2] = 0;
    counts[3] = b->slow_count[slot];
    if (proven_usable) for (int k = 0; k < 3; ++k) counts[k] = b->kind_count[slot][k];
    else counts[3] += b->fast_count[slot];
    // Every kind starts a new workgroup, and 4096 instances are exactly the 1024 workgroups the chip holds at once: one workgroup more
    // runs behind all the others and takes the launch from 52 to 70 us (measured).  So a kind's last incomplete workgroup goes to the
    // next populated kind instead, whose build is the more general one (plain < HY < ST; the XF build takes any steady instance): the
    // boundary in the list moves down by up to three entries.
    for (int k = 0; k < 3; ++k) {
        int next = k + 1;
        while (next < 4 && counts[next] == 0) ++next;
        if (next == 4 || counts[k] == 0) continue;
        const int carry = counts[k] & 3;
        counts[k] -= carry;
        counts[next] += carry;
    }
}

// Single-slot batches whose steady reverbs go by kind: the first two kinds' builds filter their own sends (SF, reverb.hip), the pre-pass
// covers the rest of the list.  Returns how many filtered instances those two kinds hold (0: no SF builds this call).
int filters_inside_count(oalsfx_batch* b, int slot, const int counts[4])
{
    if (b->slots != 1 || b->channels > 2 || b->n_filtered == 0 || counts[0] + counts[1] == 0) return 0;
    const int end = counts[0] + counts[1];
    if (b->inside_version != b->lists_version || b->inside_end != end) {
        int inside = 0;
        const int* list = b->h_lists.data() + b->steady_offset[slot];
        for (int k = 0; k < end; ++k) inside += b->inst_filtered[list[k]];
        b->inside_version = b->lists_version;
        b->inside_end = end;
        b->inside_filtered = inside;
    }
    return b->inside_filtered;
}

void launch_reverb_kinds_part(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, bool proven_usable, bool filters_inside, hipStream_t stream)
{
    int counts[4];
    steady_kind_counts(b, slot, proven_usable, counts);
    KernelCtx c = ctx;
    c.progress = nullptr;
    // one proven kind alone: its list may be a plain range of instances
    const bool one_kind = counts[3] == 0 && (counts[0] > 0) + (counts[1] > 0) + (counts[2] > 0) == 1;
    c.list_first = one_kind ? b->fast_first[slot] : -1;
    ScopedTiming timing(b, OALSFX_EAX_REVERB, stream);
    int groups = 0;
    const char* name = oalsfx_hip::launch_reverb_steady_kinds(c, slot, b->d_lists + b->steady_offset[slot], counts,
                                                              flags | ((debug_flags() & kDbgKernelBits) << 8) | ((debug_flags() & kDbgNoCuMajor) ? oalsfx_hip::kNoCuMajor : 0),
                                                              filters_inside, stream, &groups, slot_off_grid(b, slot));
    if (name) b->last_steady_kernel = name;
    b->launched_groups += groups;
}

// A multi-buffer pass (mix_device): the slot's proven-steady kinds, as launch_reverb_kinds_part would launch them for each of the pass's
// buffers on its own (pass_usable), in one launch with the buffer table.
void launch_reverb_pass_part(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, const oalsfx_hip::BufferTable& table, hipStream_t stream)
{
    int counts[4];
    steady_kind_counts(b, slot, true, counts);
    ScopedTiming timing(b, OALSFX_EAX_REVERB, stream);
    int groups = 0;
    const char* name = oalsfx_hip::launch_reverb_steady_multi(ctx, slot, b->d_lists + b->steady_offset[slot], counts, table,
                                                              flags | ((debug_flags() & kDbgKernelBits) << 8) | ((debug_flags() & kDbgNoCuMajor) ? oalsfx_hip::kNoCuMajor : 0),
                                                              stream, &groups, slot_off_grid(b, slot));
    if (name) b->last_steady_kernel = name;
    b->launched_groups += groups;
}

// The general kernel takes the instances of both reverb types that are not believed steady, or every reverb instance of
// the slot when the steady-state kernel cannot be used for this chunk (the regions are adjacent in the list).
void launch_reverb_general_part(oalsfx_batch* b, bool everything, const KernelCtx& ctx, int slot, int flags, hipStream_t stream)
{
    const int offset = everything ? b->steady_offset[slot] : b->general_offset[slot];
    const int count = b->general_count[slot] + (everything ? b->fast_count[slot] + b->slow_count[slot] : 0);
    ScopedTiming timing(b, OALSFX_REVERB + kTimedGeneralOffset, stream);
    oalsfx_hip::launch_reverb_general(ctx, slot, b->d_lists + offset, count, flags, stream);
}

// Effect types whose filter recurrences gain from cooperative workgroups (wave_effects_body.hpp, chain_phase).
bool cooperative_type(int type)
{
    // (the compressor's follower goes through chain_phase too, but a wavefront's own is as fast: it is short, and what a
    // workgroup saves in instructions it loses at the two barriers)
    return type == OALSFX_DISTORTION || type == OALSFX_ECHO || type == OALSFX_EQUALIZER || type == OALSFX_RING_MODULATOR;
}

// The ring-light types of a slot from `first_type` on as segments of one grid: per type the whole workgroups (cooperative
// where the type gains from it), then the up to three instances left over.  Returns the number of instances covered.
int wave_segments(const oalsfx_batch* b, int slot, int first_type, oalsfx_hip::WaveSegments& seg)
{
    seg = oalsfx_hip::WaveSegments{};
    int n = 0, total = 0;
    auto add = [&](int count, bool coop) {
        if (count <= 0) return;
        seg.count[n] = count;
        seg.offset[n] = total;
        if (coop) seg.coop_mask |= 1u << n;
        ++n;
        total += count;
    };
    for (int t = first_type; t < OALSFX_REVERB; ++t) {
        const int count = b->list_count[slot][t];
        if (cooperative_type(t) && count >= 4) {
            add(count & ~3, true);
            add(count & 3, false);
        } else {
            add(count, false);
        }
    }
    seg.n = n;
    return total;
}

// All ring-light effect types of a slot in one grid: their instance lists are adjacent in d_lists (types in
// ascending order, the two reverb types last).
void launch_wave_group(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, hipStream_t stream)
{
    const bool null_has_duty = (flags & (oalsfx_hip::kFirst | oalsfx_hip::kLast)) != 0;
    const int first_type = null_has_duty ? OALSFX_NULL : OALSFX_NULL + 1;
    oalsfx_hip::WaveSegments seg;
    const int count = wave_segments(b, slot, first_type, seg);
    if (count == 0) return;
    ScopedTiming timing(b, kTimedWaveEffects, stream);
    if (ctx.turn != nullptr) { flags |= (debug_flags() & kDbgHandOverBits) << 8; b->launched_groups += seg.blocks(); } // (a chained launch: test switches, the gate's count)
    oalsfx_hip::launch_wave_effects(ctx, slot, 1, b->d_lists + b->list_offset[slot][first_type], count, &seg, flags, stream);
}

// Do the reverb groups of a slot's mixed grid take the proven build for a call of n frames?  Every reverb of the slot proven, whole
// tiles, and a last block that leaves their gains at rest.
bool mixed_grid_proven(const oalsfx_batch* b, int slot, int n)
{
    return b->slow_count[slot] == 0 && b->fast_count[slot] > 0 && (n & 63) == 0 &&
           (n - ((n - 1) / OALSFX_RV_MAX_UPDATE) * OALSFX_RV_MAX_UPDATE) / 64 >= b->rest_tiles[slot];
}

// Ring-light effects and believed-steady reverbs of one slot in one grid (k_slot_mixed).
void launch_mixed_part(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, hipStream_t stream)
{
    const bool null_has_duty = (flags & (oalsfx_hip::kFirst | oalsfx_hip::kLast)) != 0;
    const int first_type = null_has_duty ? OALSFX_NULL : OALSFX_NULL + 1;
    oalsfx_hip::WaveSegments seg;
    const int light = wave_segments(b, slot, first_type, seg);
    const int steady = b->fast_count[slot] + b->slow_count[slot];
    KernelCtx c = ctx;
    c.progress = nullptr; // an instance that turns out not to be steady falls back inside the grid
    // all of them proven, and a call whose last block leaves their gains at rest: the reverb groups take the FP build
    const bool proven = mixed_grid_proven(b, slot, ctx.frames);
    c.list_first = proven ? b->fast_first[slot] : -1;
    ScopedTiming timing(b, kTimedMixed, stream);
    if (ctx.turn != nullptr) flags |= (debug_flags() & kDbgKernelBits) << 8; // (a chained launch: the hand-over's test switches)
    int groups = 0;
    oalsfx_hip::launch_slot_mixed(c, slot, b->d_lists + b->steady_offset[slot], steady, b->d_lists + b->list_offset[slot][first_type], light,
                                  seg, flags, proven, stream, &groups);
    b->launched_groups += groups;
}

// Number of consecutive slots from `slot` on that hold no reverb at all: such a run is one fused launch over every instance.
int reverb_free_run(const oalsfx_batch* b, int slot)
{
    int n = 0;
    while (slot + n < b->slots && b->list_count[slot + n][OALSFX_REVERB] + b->list_count[slot + n][OALSFX_EAX_REVERB] == 0) ++n;
    return n;
}

// A finished read-back of the "settled and at rest" flags turns believed-steady reverbs into proven ones.  Never waits: an event that
// has not completed yet is looked at again by the next call.
void poll_exact(oalsfx_batch* b)
{
    if (!b->exact_pending || hipEventQuery(b->ev_exact) != hipSuccess) return;
    b->exact_pending = false;
    const size_t total = static_cast<size_t>(b->n) * b->slots;
    for (size_t idx = 0; idx < total; ++idx) {
        // the flag describes the slot as of the read-back's call: usable when nothing was uploaded for the instance after that
        if (b->proven[idx] || !b->h_exact[idx] || b->updated_gen[idx] > b->exact_gen || !reverb_settled(b, idx)) continue;
        b->proven[idx] = static_cast<uint8_t>(std::min(4u, (b->h_exact[idx] + 63u) / 64u)); // the rest level in tiles: 1 .. 4
        b->lists_dirty = true;
    }
}

// Reported by the calls that wait for the stream: a proven-steady launch found an instance that was not steady (it left it
// unprocessed).  The host's bookkeeping makes that impossible; if it happens anyway it must not pass silently.
bool check_fault(oalsfx_batch* b)
{
    if (!b->h_fault || (b->h_fault[0] == 0 && b->h_fault[1] == 0)) return true;
    const unsigned f = b->h_fault[0], gates = b->h_fault[1] / oalsfx_hip::kFaultGate;
    if (f == 0) {
        // Gates gave up waiting and nothing else went wrong: every launch behind them found its instances' turns (else the word above would
        // say so), the results are whole.  Something holds launches of one queue back until kernels of another have finished -- a tool
        // that runs kernels one at a time out of queue order -- and every gate costs its full wait (1.3 s).  The batch goes on in plain
        // stream order from here, and says so once.
        b->h_fault[1] = 0;
        if (!b->chain_given_up) {
            b->chain_given_up = true;
            std::fprintf(stderr, "oalsfx: %u gate(s) of chained launches gave up waiting although no launch was held up by it: the device runs this "
                                 "process's kernels one at a time and out of queue order (a profiler collecting counters?).  Calls of this batch "
                                 "stay in stream order from here on (OALSFX_DEBUG_FLAGS=0x400 does that from the start).\n", gates);
        }
        return true;
    }
    if (f >= oalsfx_hip::kFaultTurn) {
        std::snprintf(b->fault_text, sizeof(b->fault_text), "Internal error: a chained launch gave up waiting (fault word 0x%x: %u turns, %u gates, %u instances not steady).",
                      f, (f / oalsfx_hip::kFaultTurn) & 0xFFFu, f / oalsfx_hip::kFaultGate + gates, f & 0xFFFu);
        // (the instances concerned were left alone, and so were the launches behind them in the run: the batch's state is a buffer short
        // there.  No further call pretends otherwise.)
        b->poisoned = true;
        return b->fail(b->fault_text);
    }
    return b->fail("Internal error: a reverb instance listed as proven steady was not; its buffer was left unprocessed.");
}

// What a slot launches for a chunk of n frames: how many instances on the ring-light kernels, on the steady-state reverb kernels, reverbs
// in all, and which launch shape the steady ones take.
struct SlotPlan {
    int light, steady, reverbs;
    bool use_steady, mixed, by_kind, proven_usable;
    bool ragged_proven; // a call that ends in a partial tile, every steady reverb of the slot proven and at rest for its last block: the FP RG builds
};

SlotPlan plan_slot(const oalsfx_batch* b, const KernelCtx& ctx, int s, int n, bool null_has_duty)
{
    SlotPlan p{};
    for (int t = null_has_duty ? 0 : 1; t < OALSFX_REVERB; ++t) p.light += b->list_count[s][t];
    // the kernels of a slot work on disjoint instances: ring-light effects, the steady-state reverb kernel and the general
    // reverb kernel
    p.use_steady = steady_kernel_usable(ctx);
    p.steady = p.use_steady ? b->fast_count[s] + b->slow_count[s] : 0;
    p.reverbs = b->list_count[s][OALSFX_REVERB] + b->list_count[s][OALSFX_EAX_REVERB];
    // ring-light effects and steady reverbs in the same slot (mono / stereo): one grid serves both
    p.mixed = p.light > 0 && p.steady > 0 && b->channels <= 2 && !ctx.timeline;
    // (the last block of a call is its shortest: up to 256 frames; the proven instances' gains are at rest for blocks of rest_tiles tiles
    // and longer)
    const int last_block = n - ((n - 1) / OALSFX_RV_MAX_UPDATE) * OALSFX_RV_MAX_UPDATE;
    const bool gains_rest = last_block >= 64 * b->rest_tiles[s];
    // (round 3: the proven instances no longer wait for the last believed one of their slot: one grid serves every kind,
    // k_reverb_steady_kinds, each workgroup on the build its instances need)
    p.by_kind = p.use_steady && !p.mixed && b->channels <= 2 && (n & 63) == 0 && !ctx.timeline;
    p.proven_usable = gains_rest;
    p.ragged_proven = p.use_steady && !p.mixed && b->channels <= 2 && (n & 63) != 0 && !ctx.timeline && p.proven_usable && b->slow_count[s] == 0 &&
                      b->fast_count[s] > 0;
    return p;
}

// Ends a run of chained launches: everything queued on the batch's stream from here on comes behind the launch that may still run on
// the second stream.
bool chain_join(oalsfx_batch* b)
{
    join_flush(b);
    if (!b->chain_open) return true;
    b->chain_open = false;
    for (int k = 1; k < kChainDepth; ++k) {
        if (!b->chain_used[k]) continue;
        b->chain_used[k] = false;
        if (!b->hip_ok(hipEventRecord(b->ev_chain[k], b->chain_stream[k]), "hipEventRecord") ||
            !b->hip_ok(hipStreamWaitEvent(b->stream, b->ev_chain[k], 0), "hipStreamWaitEvent")) return false;
    }
    return true;
}

// Is this process run under a tool that collects hardware counters per kernel (rocprofv3 --pmc, or a counter file)?  Such a tool runs
// one kernel at a time, and not in the order the queues were fed: the gate in front of a chained launch then waits for a launch the tool
// holds back until the gate has finished -- every gate counts out (1.3 s each; measured: bench.py under `rocprofv3 --pmc SQ_WAVES`
// failed with "a chained launch gave up waiting (... 31 gates ...)", profiles/r04k_under_the_profiler/).  Kernels that cannot overlap
// gain nothing from chaining anyway: stream order there.  (Tracing -- --kernel-trace, --stats -- does not serialise and chains as usual.)
bool kernels_serialised_by_a_tool()
{
    static const bool yes = [] {
        const char* on = std::getenv("ROCPROF_COUNTER_COLLECTION");   // rocprofv3 --pmc / -i: "1"
        const char* which = std::getenv("ROCPROF_COUNTERS");          // ... and the counters asked for
        const char* v1 = std::getenv("ROCP_METRICS");                 // rocprof (v1) with an input file
        if (std::getenv("OALSFX_IGNORE_TOOLS")) return false;         // (tests of what happens under a tool this does not recognise)
        return (on && std::atoi(on) != 0) || (which && *which) || (v1 && *v1);
    }();
    return yes;
}

// Can this call be a run of chained launches?  The batch's own stream, nobody holding its handle, no per-launch events, one chunk, and a
// step of one of the shapes whose kernels take turns: one steady-state reverb launch (whole tiles, or the proven ragged builds); the
// reverb-free slots' launch followed by the reverbs' (several slots); one grid of ring-light effects and proven reverbs.  (Any number of
// workgroups: the gate in front of a launch sees to it that all but a few workgroups of the launch before have started, however many
// rounds of the chip that launch takes -- 32 768 instances, eight rounds: 380 -> 360 us per step.)
// (A multi-buffer pass, `buffers` > 1: frames is the pass's, src / dst its buffers' tables, each buffer frames / buffers frames.)
bool chain_eligible(oalsfx_batch* b, int frames, int buffers, const float* const* srcs, float* const* dsts, hipStream_t stream, bool uploading)
{
    if (kernels_serialised_by_a_tool() || b->chain_given_up) return false;
    const size_t buffer_bytes = static_cast<size_t>(b->n) * (frames / buffers) * b->channels * sizeof(float);
    for (int k = 0; k < buffers; ++k) {
        // chained launches write the caller's frames with 64-bit stores (stereo, and quad / 5.1 / 6.1 / 7.1 two channels a store): an
        // output that is not 8-byte aligned (mono or more than two channels at a 4-byte offset) goes in stream order, one float a store
        if (reinterpret_cast<uintptr_t>(dsts[k]) % 8 != 0) return false;
        if (b->chain_open && b->chain_dsts.size() >= 256) {
            // (a caller that hands in a fresh output buffer with every call: the list of a run's output buffers starts over with a new run)
            const char* lo = reinterpret_cast<const char*>(dsts[k]);
            bool known = false;
            for (const auto& d : b->chain_dsts) known |= d.first <= lo && lo < d.second;
            if (!known) return false;
        }
        // an input that is the output of a call of the current run (a feedback loop through the caller's buffers): stream order for this one
        const char* lo = reinterpret_cast<const char*>(srcs[k]);
        const char* hi = lo + buffer_bytes;
        if (b->chain_open)
            for (const auto& d : b->chain_dsts)
                if (lo < d.second && d.first < hi) return false;
        // an output that overlaps an output of the current run without starting where it starts: one instance's frames would land where
        // a launch that may still run writes another instance's, and turns are taken instance by instance: stream order
        const char* out_lo = reinterpret_cast<const char*>(dsts[k]);
        if (b->chain_open)
            for (const auto& d : b->chain_dsts)
                if (out_lo != d.first && out_lo < d.second && d.first < out_lo + buffer_bytes) return false;
    }
    if (stream != b->stream || b->stream_handed_out || (debug_flags() & (kDbgNoChain | kDbgGeneralOnly)) || b->timing_every > 0 || b->d_timeline) return false;
    if (!b->uncached) return false;
    for (const auto& kv : b->pools)
        if (kv.first % 32 != 0) return false; // (a slab of delay lines ends where its last cache line ends: reverb.hip, chained launches)
    if (frames > OALSFX_MAX_CHUNK) return false;
    if (b->channels > 2) {
        // More than two channels (round 4, late): one launch of the believing build for every instance, all of them proven and at rest (no
        // general kernel behind it); its output frames written through two channels a store.  Quad / 5.1 / 7.1, 4096 EAX reverbs:
        // 63.6 -> 59.5, 69.9 -> 63.0, 81.2 -> 74.1 us per step (profiles/r04m_multichannel_chained/; round 3 had measured a loss, with one
        // write-through store per channel).
        // (6.1, seven channels a frame: one write-through store per channel made it 74.6 -> 86.5 us per step chained -- what round 3 saw; its
        // pairs now start where the frame's parity puts an even float, three pairs and one channel alone: 75.3-76.7 -> 73.1-73.2.)
        const int last_block = frames - ((frames - 1) / OALSFX_RV_MAX_UPDATE) * OALSFX_RV_MAX_UPDATE;
        return b->slots == 1 && !uploading && (frames & 63) == 0 && b->n_filtered == 0 && b->general_count[0] == 0 && b->slow_count[0] == 0 &&
               b->fast_count[0] == b->n && last_block / 64 >= b->rest_tiles[0];
    }
    if (b->slots > 1) {
        // A step of two launches (round 4): every slot but the last free of reverbs for every instance -- one launch of the ring-light
        // kernel, a wavefront per instance walking its slots -- and the last slot one grid of steady-state reverbs.  Both take turns by
        // the same word per instance, the reverb slot's: launch after launch, whichever kernel it runs.  Whole tiles, no send filters,
        // and nothing to upload (a call that has a change to put in place goes in stream order, and ends the run).
        const int last = b->slots - 1, run = reverb_free_run(b, 0);
        if (uploading || (frames & 63) != 0 || b->n_filtered > 0 || run < last) return false;
        // (batches that leave workgroup places free lose by it: 1024 instances 65.5 against 61.8 us per step, 2048: 77.5 against 70.0,
        // 3072 level, 4096: 88.7 against 94.3, 6144: 134.8 against 162.2, 8192: 186.4 against 193.7 --
        // profiles/r04g_two_launch_steps/config3_by_size.txt)
        if ((b->n + 3) / 4 < 1024 && !(debug_flags() & kDbgChainAlways)) return false;
        // (no reverb anywhere: the ring-light kernel's launch would be the whole step.  Measured slower chained -- 4096 x chorus -> flanger
        // -> echo 47.4 against 44.7 us per step; see the single-slot case below -- unless the test switch asks for it)
        if (run == b->slots) return (debug_flags() & kDbgChainLight) != 0;
        if (b->fast_count[last] + b->slow_count[last] != b->n || b->general_count[last] != 0) return false;
        KernelCtx ctx{};
        ctx.frames = frames;
        const SlotPlan pl = plan_slot(b, ctx, last, frames, true);
        return pl.by_kind && !pl.mixed && pl.steady == b->n;
    }
    // Short calls of a batch that leaves workgroup slots free gain nothing from the overlap and can lose by it: the next launch's
    // workgroups are on the chip at once, waiting, beside the ones they wait for (2048 instances x 64 frames: 16.7 us per step chained,
    // 13.4 in stream order; x 128: 22.3 against 19.5; from 256 frames on, and with every slot taken, chained is level or ahead:
    // profiles/r04e_round4_end/chained/instances_and_call_sizes.txt).
    if ((b->n + 3) / 4 < 1024 && frames < 256 && !(debug_flags() & kDbgChainAlways)) return false;
    const int steady = b->fast_count[0] + b->slow_count[0];
    if (b->general_count[0] != 0) return false;
    if (steady != b->n) {
        // A slot of ring-light effects, or of ring-light effects and proven reverbs (BASELINE configs[3]): the step is one grid as well --
        // k_wave_effects with its segments, or k_slot_mixed on its proven build -- whose ring-light wavefronts take turns like the reverb
        // groups do.  Whole tiles, no send filters, nothing to upload.
        if (uploading || (frames & 63) != 0 || b->n_filtered > 0) return false;
        KernelCtx ctx{};
        ctx.frames = frames;
        const SlotPlan pl = plan_slot(b, ctx, 0, frames, true);
        if (pl.light + pl.steady != b->n || pl.reverbs != pl.steady) return false;
        // Ring-light effects alone: measured slower chained than in stream order (4096 instances, 256-frame calls: chorus 18.9 against
        // 15.1 us per step, dedicated 19.9 against 10.4, eight types in one slot 38 against 30.7 -- launches of 10 to 30 us are about what
        // the host and the gate in front of each cost; profiles/r04h_mixed_grid_chained/ring_light_chained.txt).  With reverbs in the grid
        // a launch is 45 us and more: BASELINE configs[3] 59.7 -> 51.5 us per step.  (kDbgChainLight: the test switch that chains them anyway.)
        if (pl.steady == 0) return (debug_flags() & kDbgChainLight) != 0;
        // ... and what chaining gains there is the partly filled last round of the chip: a grid that fits the chip at once loses (4096
        // instances 42.8 against 36.0 us per step, 2048: 37.3 against 35.1 -- whatever the order of its workgroups), one of one to two
        // rounds gains (6144: 41.4 against 44.9; 8192: 51.6 against 59.9), four full rounds are level (16 384: 108.2 against 107.3;
        // profiles/r04h_mixed_grid_chained/config4_by_size.txt).
        if ((b->n + 3) / 4 <= 1024 && !(debug_flags() & kDbgChainAlways)) return false;
        return pl.mixed && mixed_grid_proven(b, 0, frames);
    }
    if ((frames & 63) != 0) {
        // a call that ends in a partial tile chains when its step is one launch of the proven ragged builds (no general path inside, no
        // send-filter pre-pass in front)
        KernelCtx ctx{};
        ctx.frames = frames;
        if (!plan_slot(b, ctx, 0, frames, true).ragged_proven || b->n_filtered > 0) return false;
    }
    if (b->n_filtered > 0) {
        // send filters: only when every filtered instance's build has them inside (no pre-pass launch in front of the reverb's)
        KernelCtx ctx{};
        ctx.frames = frames;
        const SlotPlan p0 = plan_slot(b, ctx, 0, frames, true);
        if (!p0.by_kind || p0.steady != b->n) return false;
        int counts[4];
        steady_kind_counts(b, 0, p0.proven_usable, counts);
        if (filters_inside_count(b, 0, counts) != b->n_filtered) return false;
    }
    return true;
}

// The next launch of a run of chained launches: its stream, the number it waits for and the one it leaves, the gate in front of it.
// joinable (may be nullptr; in: the caller would like the launch to take later calls, out: it can): a launch behind a k_chain_gate of its
// own.  That gate is then queued with the grid (join_queue), not here.
bool chain_next_launch(oalsfx_batch* b, KernelCtx& ctx, int depth, PendingUpload* upload, hipStream_t* stream_out, bool* joinable = nullptr)
{
    bool own_gate = false;
    b->chain_pos_before = b->chain_open ? b->chain_pos_last : -1;
    b->chain_pos_last = b->chain_open ? b->chain_pos : -1;
    b->chain_pos = b->chain_open ? (b->chain_pos + 1) % depth : 0;
    hipStream_t stream = b->chain_stream[b->chain_pos];
    const bool first_on_its_stream = b->chain_open && !b->chain_used[b->chain_pos]; // (of the current run)
    b->chain_used[b->chain_pos] = true;
    const size_t total = static_cast<size_t>(b->n) * b->slots;
    ctx.turn = b->d_turn;
    ctx.turn_cu = b->d_turn + total + 16;
    ctx.turn_cu2 = ctx.turn_cu + total;
    ctx.turn_slot = b->slots - 1;
    // (this launch sits behind the launch two before it in its stream -- two streams taking turns -- or that launch may still run)
    ctx.turn_two_back = (b->chain_pos_before >= 0 && b->chain_pos_before != b->chain_pos) ? 1u : 0u;
    ctx.turn_wait = b->chain_open ? b->turn_counter : 0u;
    if (++b->turn_counter == 0u) b->turn_counter = 1u;
    ctx.turn_set = b->turn_counter;
    // A launch whose workgroups wait for the launch before must not take the chip before that launch has its workgroups on it: they
    // would wait for workgroups that cannot start.  Stream order does not see to that (this launch comes behind the launch two
    // before it, on its own stream; the launch before it sits in another queue, which the hardware may get to later -- the first
    // launch ever on the second stream waited for its queue to be set up while the third launch of the run filled the chip).  So
    // every workgroup of a chained launch counts itself in as it starts, and every launch but a run's first comes behind a gate
    // (one wavefront, k_chain_gate) that waits until all but a few workgroups of the launch before have.  Then a workgroup that
    // waits always waits for one that is on the chip or through: at most those few are not, fewer than the chip has places.
    unsigned* started = b->d_turn + total;
    if (!b->chain_open) {
        if (!b->hip_ok(hipEventRecord(b->ev_chain_start, b->stream), "hipEventRecord")) return false;
        b->chain_len = 1;
    } else {
        // (the first launch of the run on one of the other streams: not before the run's first could start either)
        ++b->chain_len;
        if (first_on_its_stream && !b->hip_ok(hipStreamWaitEvent(stream, b->ev_chain_start, 0), "hipStreamWaitEvent")) return false;
        // (kDbgGateSecondOnly: the gate in front of a run's second launch only, as first built -- the negative control of
        // tests/test_gpu_chained.py::test_the_first_run_of_a_fresh_process)
        if (b->chain_len == 2 || !(debug_flags() & kDbgGateSecondOnly)) {
            const unsigned target = b->started_total - static_cast<uint32_t>(std::min(8, (b->n + 3) / 4 - 1));
            if (upload && upload->st) { upload->jobs.gate_started = started; upload->jobs.gate_target = target + b->gate_skew; } // (the upload kernel is the gate as well)
            else if (joinable && *joinable) { own_gate = true; b->join.gate_started = started; b->join.gate_target = target + b->gate_skew; b->join.table = b->chain_pos; }
            else oalsfx_hip::launch_chain_gate(started, target + b->gate_skew, b->d_fault + 1, stream);
        }
    }
    if (joinable) *joinable = own_gate;
    ctx.turn_started = started;
    b->chain_open = true;
    b->launched_groups = 0;
    *stream_out = stream;
    return true;
}

// ... and behind it: every workgroup of the launch counts itself in on the device (reverb.hip, turn_started): the grid as launched, which
// for a grid of several kinds is up to three workgroups more than a quarter of the instances (ADVICE, round 3: the host added (n + 3) / 4
// and drifted behind the device's count by up to three per call).
bool chain_launch_done(oalsfx_batch* b)
{
    if (b->launched_groups <= 0) return b->fail("Internal error: a chained call launched no grid that takes turns.");
    b->started_total += static_cast<uint32_t>(b->launched_groups);
    b->launched_groups = 0;
    return true;
}

// Can the calls of `frames` frames that follow go through multi-buffer passes of `total` frames (one launch each)?  Exactly when every one
// of them on its own would be one launch of the proven-steady kinds (launch_reverb_kinds_part): one slot, mono / stereo, whole tiles, no
// send filter, every instance a reverb proven steady and at rest for the call's last block -- and for the pass's, whose blocks (256 frames
// but its last, OALSFX_RV_MAX_UPDATE) are not the calls' blocks.  At rest, a block boundary changes nothing a proven instance computes
// (DESIGN 4b); what the calls carry from one to the next -- delay lines, filter histories, the write position, the modulator's index --
// the pass carries from tile to tile as it does inside a single call.  A pass is one chunk of the mix loop: at most OALSFX_MAX_CHUNK
// frames (calls longer than that are chunked by mix_pass and go one at a time).
bool pass_usable(oalsfx_batch* b, int frames, int total)
{
    if (total > OALSFX_MAX_CHUNK || frames > total) return false;
    if (b->slots != 1 || b->channels > 2 || (frames & 63) != 0 || b->n_filtered > 0 || b->d_timeline) return false;
    if (b->fast_count[0] != b->n || b->slow_count[0] != 0 || b->general_count[0] != 0) return false;
    for (const int n : {frames, total}) {
        KernelCtx ctx{};
        ctx.frames = n;
        const SlotPlan p = plan_slot(b, ctx, 0, n, true);
        if (!p.by_kind || p.mixed || p.steady != b->n || !p.proven_usable) return false;
    }
    return true;
}

// Do the buffers of a pass keep out of each other's way as consecutive calls would?  A pass reads and writes its buffers tile by tile,
// interleaved across instances, so no buffer's output may overlap another buffer's input or output (in place, src[k] == dst[k], is
// what a single call allows as well).  Every buffer is the same number of bytes, so in address order a buffer overlaps one before it
// exactly when it overlaps the last one before it of that kind (source / output) and of another call -- one of the last two: a sort and
// one sweep, O(K log K) for K buffers.
bool buffers_apart(const oalsfx_batch* b, int frames, int buffers, const float* const* srcs, float* const* dsts)
{
    if (buffers < 2) return true;
    const uintptr_t bytes = static_cast<uintptr_t>(b->n) * frames * b->channels * sizeof(float);
    struct Range { uintptr_t lo; int call; bool out; };
    std::vector<Range> r;
    r.reserve(2 * static_cast<size_t>(buffers));
    for (int k = 0; k < buffers; ++k) {
        r.push_back({reinterpret_cast<uintptr_t>(srcs[k]), k, false});
        r.push_back({reinterpret_cast<uintptr_t>(dsts[k]), k, true});
    }
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.lo < y.lo || (x.lo == y.lo && x.call < y.call); });
    const Range* last[2][2] = {}; // [kind: source, output][the last one, the one before]
    for (const Range& x : r) {
        for (int kind = 0; kind < 2; ++kind) {
            // an output overlapping anything of another call, or a source overlapping an output of another call
            if (!x.out && kind == 0) continue;
            for (const Range* y : last[kind])
                if (y && y->call != x.call && y->lo + bytes > x.lo) return false;
        }
        const int kind = x.out ? 1 : 0;
        last[kind][1] = last[kind][0];
        last[kind][0] = &x;
    }
    return true;
}

// ---- calls that join a queued launch (the protocol: join_word.hpp) ----
// Does the link between this device and the host carry the device's atomic exchange on host memory?  Asked once per device; where it
// does not, no launch of the process takes later calls, and one line says so.
bool join_atomics(int device)
{
    static std::mutex m;
    static std::map<int, bool> known;
    std::lock_guard<std::mutex> lock(m);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    int v = 0;
    const bool ok = hipDeviceGetAttribute(&v, hipDeviceAttributeHostNativeAtomicSupported, device) == hipSuccess && v != 0;
    if (!ok) std::fprintf(stderr, "oalsfx: device %d reports no native atomics on host memory: queued launches take no later calls (chained launches as before).\n", device);
    known[device] = ok;
    return ok;
}

// Queues the gate and the grid of the joinable launch that join_begin set up.
void join_queue(oalsfx_batch* b)
{
    auto& j = b->join;
    if (!j.held) return;
    j.held = false;
    oalsfx_hip::launch_chain_gate(j.gate_started, j.gate_target, b->d_fault + 1, j.stream, b->d_join + j.slot, b->d_join_tables + j.table, static_cast<unsigned>(j.groups));
    const char* name = oalsfx_hip::launch_reverb_steady_joined(j.ctx, j.reverb_slot, j.list, j.counts, b->d_join_tables + j.table, j.flags, j.stream, nullptr, j.carry);
    if (name) b->last_steady_kernel = name;
}

// Nothing joins the last launch from here on, and a launch the test hook holds back is queued.  (Whatever ends a run comes through here --
// chain_join -- and so does every call that launches for itself.)
void join_flush(oalsfx_batch* b)
{
    b->join.accepting = false;
    join_queue(b);
}

// Would a chained call of `frames` frames, about to be queued, be a launch that later calls can join?  The proven-steady kinds alone, as
// a pass of one buffer (pass_usable), on a link that has the atomics, with a slot free -- and nothing of the call left to queue behind
// the grid (the read-back of the "at rest" flags).
bool join_wanted(oalsfx_batch* b, int frames)
{
    if ((debug_flags() & (kDbgNoJoin | kDbgGateSecondOnly)) || frames > OALSFX_MAX_CHUNK || b->exact_wanted) return false;
    if (!pass_usable(b, frames, frames) || !join_atomics(b->device)) return false;
    if (!b->h_join) {
        // (the first time: the slots, and the tables the gates fill)
        if (hipHostMalloc(reinterpret_cast<void**>(&b->h_join), oalsfx_batch::kJoinSlots * sizeof(oalsfx_join::JoinSlot), hipHostMallocMapped) != hipSuccess) { b->h_join = nullptr; return false; }
        std::memset(b->h_join, 0, oalsfx_batch::kJoinSlots * sizeof(oalsfx_join::JoinSlot));
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&b->d_join), b->h_join, 0) != hipSuccess ||
            handed_on_malloc(b, reinterpret_cast<void**>(&b->d_join_tables), kChainDepth * sizeof(oalsfx_hip::BufferTable)) != hipSuccess) {
            (void)hipHostFree(b->h_join);
            b->h_join = nullptr;
            (void)hipGetLastError();
            return false;
        }
    }
    if (!b->d_join_tables) return false;
    return oalsfx_join::join_reusable(b->h_join + b->join_turn);
}

// The joinable launch itself, in place of launch_reverb_kinds_part: the call is buffer 0 of a table that may grow until the gate closes it.
bool join_begin(oalsfx_batch* b, const KernelCtx& ctx, int slot, int flags, const float* src, float* dst, hipStream_t stream)
{
    auto& j = b->join;
    j.slot = b->join_turn;
    b->join_turn = (b->join_turn + 1) % oalsfx_batch::kJoinSlots;
    j.count = 1;
    j.frames = ctx.frames;
    j.ctx = ctx;
    j.stream = stream;
    j.reverb_slot = slot;
    j.flags = flags | ((debug_flags() & kDbgKernelBits) << 8) | ((debug_flags() & kDbgNoCuMajor) ? oalsfx_hip::kNoCuMajor : 0);
    j.list = b->d_lists + b->steady_offset[slot];
    steady_kind_counts(b, slot, true, j.counts);
    j.carry = slot_off_grid(b, slot);
    j.srcs[0] = reinterpret_cast<const char*>(src);
    j.dsts[0] = reinterpret_cast<const char*>(dst);
    int groups = 0;
    for (int k = 0; k < 3; ++k) groups += (j.counts[k] + 3) >> 2;
    if (groups <= 0) return b->fail("Internal error: a joinable launch without instances.");
    b->launched_groups += groups;
    j.groups = groups;
    oalsfx_join::join_start(b->h_join + j.slot, j.frames, src, dst);
    j.accepting = j.frames * 2 <= OALSFX_MAX_CHUNK;
    j.held = true;
    b->joinable_launches += 1;
    // (the test hook: queued once it has join_hold buffers, or when something closes it -- join_try, join_flush)
    if (b->join_hold <= 1 || !j.accepting) join_queue(b);
    return true;
}

// A plain single-buffer call on the batch's own stream: one more buffer of the launch queued last, if that launch still takes any and the
// call is what that launch's next buffer may be.  True: the call is done (nothing was launched, nothing waits).
bool join_try(oalsfx_batch* b, int frames, const float* src, float* dst, hipStream_t stream, const PendingUpload& upload)
{
    auto& j = b->join;
    if (!j.accepting) return false;
    if (!b->chain_open || stream != b->stream || frames != j.frames || upload.st || upload.any || b->exact_wanted || (debug_flags() & kDbgNoJoin)) return false;
    const int total = static_cast<int>(j.count + 1) * frames;
    // (the device may close at any count: every total so far was checked when its buffer joined, and nothing has changed since -- a change
    // comes with an upload, which ends joining)
    if (total > OALSFX_MAX_CHUNK || !pass_usable(b, frames, total)) return false;
    float* out = dst;
    if (!chain_eligible(b, frames, 1, &src, &out, stream, false)) return false; // (8-byte aligned output, an input that is no output of the run, ...)
    const size_t bytes = static_cast<size_t>(b->n) * frames * b->channels * sizeof(float);
    const char* lo = reinterpret_cast<const char*>(dst);
    const char* in = reinterpret_cast<const char*>(src);
    for (unsigned k = 0; k < j.count; ++k) {
        // An output the same as or apart from every output of the table: an instance's region is written by one wavefront in buffer
        // order.  A partial overlap puts one instance's frames where another wavefront writes another's.  And apart from the inputs
        // of the buffers before it, which other wavefronts may not have read yet.
        if (lo != j.dsts[k] && lo < j.dsts[k] + bytes && j.dsts[k] < lo + bytes) return false;
        if (lo < j.srcs[k] + bytes && j.srcs[k] < lo + bytes) return false;
    }
    if (in != lo && in < lo + bytes && lo < in + bytes) return false;
    if (!oalsfx_join::join_append(b->h_join + j.slot, j.count, src, dst)) { j.accepting = false; return false; } // closed: this call queues its own
    j.srcs[j.count] = in;
    j.dsts[j.count] = lo;
    j.count += 1;
    // the call's bookkeeping, as mix_pass does it
    b->mix_calls += 1;
    b->chained_calls += 1;
    b->joined_calls += 1;
    // (the count of started workgroups is one per call: the launch's gate adds this call's share on the device once it knows the call is in)
    b->started_total += static_cast<uint32_t>(j.groups);
    {
        bool known = false;
        for (auto& d : b->chain_dsts) known |= d.first <= lo && lo + bytes <= d.second;
        if (!known) b->chain_dsts.push_back({lo, lo + bytes});
    }
    advance_settling(b, frames);
    b->frames_total += static_cast<uint32_t>(frames);
    b->last_launch_stream = b->stream;
    if (static_cast<int>(j.count + 1) * frames > OALSFX_MAX_CHUNK) j.accepting = false;
    if (j.held && (static_cast<int>(j.count) >= b->join_hold || !j.accepting)) join_flush(b); // (the hook: groupings the tests can count on)
    return true;
}

// One step of the mix loop: a call of `frames` frames (buffers == 1), or a multi-buffer pass (`pass`, from mix_device below: `buffers`
// consecutive calls of `frames` frames each in one launch of k_reverb_steady_multi).  `upload`: what prepare_params put together.
bool mix_pass(oalsfx_batch* b, int frames, int buffers, const float* const* srcs, float* const* dsts, hipStream_t stream, bool may_chain,
              PendingUpload& upload, bool pass)
{
    const float* const src = srcs[0];
    float* const dst = dsts[0];
    const int total = frames * buffers; // (the pass's frames: at most OALSFX_MAX_CHUNK when buffers > 1)
    if (pass && total > OALSFX_MAX_CHUNK) return b->fail("Internal error: a multi-buffer pass longer than one chunk.");
    const bool chained = may_chain && (!upload.st || upload.chainable) && chain_eligible(b, total, buffers, srcs, dsts, stream, upload.st != nullptr);
    if (!chained && !chain_join(b)) return false;
    int depth = 2;
    if (chained) {
        // The streams in turn; the first launch of a run stays on the batch's stream, behind whatever was queued there before.  Two streams
        // while every workgroup takes the same time (one kind of proven instances, nothing uploaded), three when workgroups differ
        // (several kinds, cross-fading instances): a launch then does not wait for the slowest workgroups of the launch two before it.
        const int rs = b->slots - 1; // (the reverbs' slot)
        int populated = 0;
        for (int k = 0; k < 3; ++k) populated += b->kind_count[rs][k] > 0;
        // (Round 4 looked at three for the uniform workload again: the gate in front of a launch is a kernel of its own behind the launch
        // two before it, and with two streams it starts when that launch ends, 5 us before the launch behind it can be dispatched
        // (profiles/r04f_round4_end/chained/timeline_chained.txt); with three it is through by then.  400-call runs 40.3 -> 39.8 us per
        // step -- and the driver's own command, bench.py --steps 20 --warmup 5, 43.0-43.7 -> 49.0-51.6: a short run pays for the third
        // stream's start three times over.  Two it stays.  profiles/r04c_instruction_diet/chain_depth_uniform.txt)
        depth = (populated > 1 || b->slow_count[rs] > 0 || upload.st) ? kChainDepth : 2;
    }
    if (!chained && !launch_params(b, upload, b->stream, stream)) return false;
    if (!ensure_mixbuf(b)) return false;
    // (every timing_every-th call is timed: a pass, when one of its buffers is such a call)
    b->timing = b->timing_every > 0 && (b->mix_calls % b->timing_every == 0 || b->mix_calls % b->timing_every + buffers > b->timing_every);
    b->mix_calls += buffers;
    const bool filtered = b->n_filtered > 0;
    const int chunk_max = std::min(total, OALSFX_MAX_CHUNK);
    const size_t plane = static_cast<size_t>(b->n) * chunk_max * b->channels;
    if (filtered && plane > b->filtered_capacity) {
        if (!b->hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize")) return false;
        for (int k = 1; k < kChainDepth && b->chain_open; ++k) // (a run of chained launches: the planes' readers may be on its other streams)
            if (!b->hip_ok(hipStreamSynchronize(b->chain_stream[k]), "hipStreamSynchronize")) return false;
        hipFree(b->d_filtered);
        b->d_filtered = nullptr;
        b->filtered_capacity = 0;
        if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_filtered), plane * (1 + b->slots) * sizeof(float)), "hipMalloc(filtered sends)")) return false;
        b->filtered_capacity = plane;
    }
    KernelCtx ctx{};
    ctx.params = b->d_params;
    ctx.state = b->d_state;
    ctx.rings = b->d_rings;
    ctx.source = b->d_source;
    ctx.source_state = b->d_source_state;
    ctx.mixbuf = b->d_mixbuf;
    ctx.timeline = b->d_timeline;
    ctx.hot = b->d_hot;
    ctx.inst_epoch = b->d_inst_epoch;
    ctx.exact = b->d_exact;
    ctx.fault = b->d_fault;
    ctx.list_first = -1;
    ctx.no_follow_up = 0;
    bool joinable = false; // a chained launch that takes the calls arriving while its gate waits (join_begin)
    if (chained) {
        if (!b->chain_open) b->chain_dsts.clear();
        for (int k = 0; k < buffers; ++k) {
            const char* lo = reinterpret_cast<const char*>(dsts[k]);
            const char* hi = lo + static_cast<size_t>(b->n) * frames * b->channels * sizeof(float);
            bool known = false;
            for (auto& d : b->chain_dsts) known |= d.first <= lo && hi <= d.second;
            if (!known) b->chain_dsts.push_back({lo, hi});
        }
        // the step's first launch (of two, for a batch of several slots: chain_eligible)
        // (from a run's third launch on: a second launch that closes with its own buffer alone -- a caller that synchronises after every
        // second call -- measured 65.2 us per call on the table build against 63.7-64.5, the gate's round trips to host memory with
        // nothing to hide them behind: profiles/r06a_joined_launches/)
        joinable = !pass && b->chain_open && b->chain_len >= 2 && !upload.st && join_wanted(b, frames);
        if (!chain_next_launch(b, ctx, depth, &upload, &stream, &joinable)) return false;
        // Parameters that changed since the call before: put in place on this launch's stream, behind the gate -- beside the launch
        // before, which may still be at work with the old ones: a slot's record (and its instance's epoch) is stored once that launch is
        // through with the instance; a rebuilt list went to the buffer that launch does not read.
        if (!launch_params(b, upload, stream, nullptr, b->d_turn, ctx.turn_wait)) return false;
        b->chained_calls += 1;
    }
    ctx.slots = b->slots;
    ctx.channels = b->channels;
    ctx.io_stride = static_cast<long long>(frames) * b->channels;
    // (a chained step of two kernels: workgroups of one size, so that either kernel's fit the places the other's give up -- common.hpp)
    struct EqualPlaces {
        bool on;
        explicit EqualPlaces(bool o) : on(o) { if (on) oalsfx_hip::set_lds_per_workgroup(40960); }
        ~EqualPlaces() { if (on) oalsfx_hip::set_lds_per_workgroup(0); }
    } equal_places(chained && b->slots > 1);
    // Api::mix chunking (reference src/oalsfxpp.cpp:3818-3826); a pass is one chunk, buffer after buffer
    oalsfx_hip::BufferTable table{};
    if (pass) {
        for (int k = 0; k < buffers; ++k) { table.src[k] = srcs[k]; table.dst[k] = dsts[k]; }
        table.frames = frames;
        table.buffers = buffers;
    }
    for (int done = 0; done < total;) {
        const int n = std::min(total - done, OALSFX_MAX_CHUNK);
        const float* chunk_src = src + static_cast<size_t>(done) * b->channels;
        ctx.raw_src = chunk_src;
        ctx.dst = dst + static_cast<size_t>(done) * b->channels;
        ctx.frames = n;
        bool planes = filtered; // the pre-pass ran: the instances it covers read their sends from its planes (flag kFiltered)
        // Single-slot batches: the steady-state reverb builds of the first two kinds filter their own sends (SF); the pre-pass then covers
        // the rest of the slot's list only, or is not launched at all.
        bool filters_inside = false;
        if (filtered && b->slots == 1) {
            const SlotPlan p0 = plan_slot(b, ctx, 0, n, true);
            if (p0.by_kind && p0.steady > 0) {
                int counts[4];
                steady_kind_counts(b, 0, p0.proven_usable, counts);
                const int inside = filters_inside_count(b, 0, counts);
                if (inside > 0) {
                    filters_inside = true;
                    ctx.src_stride = static_cast<long long>(n) * b->channels;
                    planes = inside < b->n_filtered;
                    if (planes) {
                        const int before = b->steady_offset[0], behind = before + counts[0] + counts[1];
                        oalsfx_hip::launch_send_filters(ctx, chunk_src, ctx.io_stride, b->d_filtered, b->filtered_capacity, b->d_lists, before, stream);
                        oalsfx_hip::launch_send_filters(ctx, chunk_src, ctx.io_stride, b->d_filtered, b->filtered_capacity, b->d_lists + behind, b->n - behind, stream);
                    }
                }
            }
        }
        if (filters_inside) {
            ctx.src = planes ? b->d_filtered : chunk_src;
            if (!planes) ctx.src_stride = ctx.io_stride;
        } else if (filtered) {
            // apply_filters for every send (reference src/oalsfxpp.cpp:2929-2965): planes of [instance][n][channels]
            ctx.src_stride = static_cast<long long>(n) * b->channels;
            oalsfx_hip::launch_send_filters(ctx, chunk_src, ctx.io_stride, b->d_filtered, b->filtered_capacity, nullptr, b->n, stream);
            ctx.src = b->d_filtered;
        } else {
            ctx.src_stride = ctx.io_stride;
            ctx.src = chunk_src;
        }
        ctx.wet_plane = planes ? static_cast<long long>(b->filtered_capacity) : 0;
        for (int s = 0; s < b->slots; ++s) {
            ctx.wet_src = planes ? b->d_filtered + static_cast<size_t>(1 + s) * b->filtered_capacity : ctx.src;
            const int run = reverb_free_run(b, s);
            if (run >= 2) {
                // slots s .. s+run-1 hold ring-light effects (or nothing) for every instance: one launch, one wavefront per
                // instance, the slots in order inside it; the slot's list in type order lists every instance exactly once
                const int run_flags = (s == 0 ? oalsfx_hip::kFirst : 0) | (s + run == b->slots ? oalsfx_hip::kLast : 0) |
                                      (planes ? oalsfx_hip::kFiltered : 0);
                {
                    ScopedTiming timing(b, kTimedWaveEffects, stream);
                    // (a chained step: in the order of the reverbs' grid -- its list names every instance once as well; otherwise the
                    // kernel's bit 8 of flags >> 8 takes the list as it comes)
                    const bool grid_order = chained && s + run < b->slots;
                    const int* every = grid_order ? b->d_lists + b->steady_offset[b->slots - 1] : b->d_lists + b->list_offset[s][OALSFX_NULL];
                    oalsfx_hip::launch_wave_effects(ctx, s, run, every, b->n, nullptr,
                                                    run_flags | (chained ? ((debug_flags() & kDbgHandOverBits) | (grid_order ? 0 : 8)) << 8 : 0), stream);
                }
                if (chained) b->launched_groups = (b->n + 3) / 4;
                s += run - 1;
                continue;
            }
            // (a chained step's second launch: the reverbs' grid, next in the run)
            if (chained && s > 0 && (!chain_launch_done(b) || !chain_next_launch(b, ctx, depth, nullptr, &stream))) return false;
            const int flags = (s == 0 ? oalsfx_hip::kFirst : 0) | (s == b->slots - 1 ? oalsfx_hip::kLast : 0) |
                              (planes ? oalsfx_hip::kFiltered : 0);
            const bool null_has_duty = (flags & (oalsfx_hip::kFirst | oalsfx_hip::kLast)) != 0;
            const SlotPlan sp = plan_slot(b, ctx, s, n, null_has_duty);
            const int light = sp.light, steady = sp.steady, reverbs = sp.reverbs;
            const bool use_steady = sp.use_steady, mixed = sp.mixed, by_kind = sp.by_kind, proven_usable = sp.proven_usable;
            // parts: ring-light effects | (unused) | steady reverbs | general reverbs
            bool part_on[4] = {light > 0 && !mixed, false, steady > 0, reverbs - steady > 0};
            int parts = 0;
            for (bool on : part_on) parts += on;
            const bool fork = parts > 1;
            if (fork && !b->hip_ok(hipEventRecord(b->ev_fork, stream), "hipEventRecord")) return false;
            // The caller's stream takes the part the step will wait for longest -- the general kernel, if there is one (a few
            // wavefronts, each a long chain of latencies) -- and the others go beside it: what the stream then waits for at the
            // join has long finished, and neither fork nor join (about 12 us each on this stack) lies on the step's critical path.
            int main_part = -1;
            for (int g = 0; g < 4; ++g)
                if (part_on[g]) main_part = (main_part < 0 || g == 3) ? g : main_part;
            int side = 0;
            for (int g = 0; g < 4; ++g) {
                if (!part_on[g]) continue;
                hipStream_t gs = stream;
                if (fork && g != main_part) {
                    gs = b->side_stream[side];
                    if (!b->hip_ok(hipStreamWaitEvent(gs, b->ev_fork, 0), "hipStreamWaitEvent")) return false;
                }
                if (g == 0) {
                    launch_wave_group(b, ctx, s, flags, gs);
                } else if (g == 2 && mixed) {
                    launch_mixed_part(b, ctx, s, flags, gs);
                } else if (g == 2 && joinable) {
                    if (!join_begin(b, ctx, s, flags, src, dst, gs)) return false;
                } else if (g == 2 && pass) {
                    launch_reverb_pass_part(b, ctx, s, flags, table, gs);
                } else if (g == 2 && by_kind) {
                    launch_reverb_kinds_part(b, ctx, s, flags, proven_usable, filters_inside, gs);
                } else if (g == 2) {
                    // ragged calls, more than two channels, the timeline build: one launch of the believing builds for all of them -- or,
                    // for a ragged call of proven instances only, of the proven ragged builds
                    launch_reverb_steady_part(b, ctx, s, flags, b->steady_offset[s], steady, sp.ragged_proven, gs);
                } else {
                    launch_reverb_general_part(b, !use_steady, ctx, s, flags, gs);
                }
                if (gs != stream) {
                    if (!b->hip_ok(hipEventRecord(b->ev_join[side], gs), "hipEventRecord")) return false;
                    ++side;
                }
            }
            for (int k = 0; k < side; ++k)
                if (!b->hip_ok(hipStreamWaitEvent(stream, b->ev_join[k], 0), "hipStreamWaitEvent")) return false;
        }
        done += n;
    }
    if (chained && !chain_launch_done(b)) return false;
    if (pass) { b->multi_buffers += buffers; b->multi_passes += 1; }
    if ((total % OALSFX_MAX_CHUNK) & 63) {
        // a ragged chunk: a cross-fade in flight no longer stands at a tile boundary, which the XF build needs
        for (size_t idx : b->settling)
            if (b->xf_ok[idx]) { b->xf_ok[idx] = 0; b->lists_dirty = true; }
    }
    advance_settling(b, total);
    b->frames_total += static_cast<uint32_t>(total);
    if (total & 31) b->off_grid_known = false;
    if (b->exact_wanted && !b->exact_pending) {
        // what this call's kernels found out about the reverbs that are not proven steady yet, fetched behind them
        const size_t total = static_cast<size_t>(b->n) * b->slots;
        if (!b->hip_ok(hipMemcpyAsync(b->h_exact, b->d_exact, total * sizeof(unsigned), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(exact)")) return false;
        if (!b->hip_ok(hipEventRecord(b->ev_exact, stream), "hipEventRecord")) return false;
        b->exact_pending = true;
        b->exact_wanted = false;
        b->exact_gen = b->upload_gen;
    }
    b->last_launch_stream = chained ? b->stream : stream;
    if (!chained && stream != b->stream && !b->hip_ok(hipEventRecord(b->ev_mixed, stream), "hipEventRecord")) return false;
    return b->hip_ok(hipGetLastError(), "kernel launch");
}

// `buffers` consecutive calls of `frames` frames, src[k] -> dst[k]: each call one step of the mix loop, or -- `multi` (the caller asked
// for several at once, oalsfx_batch_mix_device_multi), the buffers apart and the instances right for it (pass_usable) -- up to
// OALSFX_MAX_CHUNK / frames of them in one multi-buffer pass.  What changed since the last call goes up in front of the first launch; a
// pass has nothing to upload behind it (its buffers are consecutive calls with no setter between them).  Where the instances are not right
// for it yet -- the first calls of a stream, before the device has proven them steady -- the calls one at a time get them there.
bool mix_device(oalsfx_batch* b, int frames, int buffers, const float* const* srcs, float* const* dsts, hipStream_t stream, bool may_chain,
                bool multi)
{
    // a snapshot, restore or reset on the batch's stream reads or writes what these launches read and write: a caller's stream waits for it
    // (the batch's own stream, and the chained runs that start on it, are behind it already)
    if (b->state_io_unordered && stream != b->stream) {
        if (!b->hip_ok(hipStreamWaitEvent(stream, b->ev_state_io, 0), "hipStreamWaitEvent")) return false;
        b->state_io_unordered = false;
    }
    const int per_pass = std::max(1, OALSFX_MAX_CHUNK / std::max(frames, 1));
    // (buffers that overlap anywhere in the call: one call each, all of them)
    const bool apart = multi && buffers_apart(b, frames, buffers, srcs, dsts);
    for (int k = 0; k < buffers;) {
        if (b->poisoned) return b->fail(b->fault_text);
        poll_exact(b);
        b->launched_groups = 0;
        // what has changed since the last call: the host's part first (it decides what this call launches), the upload itself in mix_pass,
        // where the call's launches go
        PendingUpload upload;
        const auto hp0 = std::chrono::steady_clock::now();
        if (!prepare_params(b, upload)) return false;
        b->host_prepare_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - hp0).count();
        if (buffers == 1 && !multi && may_chain && join_try(b, frames, srcs[k], dsts[k], stream, upload)) return true;
        join_flush(b); // (whatever this call launches comes behind the last launch: nothing joins that one any more)
        const int take = std::min(buffers - k, per_pass);
        const bool pass = apart && !(debug_flags() & kDbgGeneralOnly) && pass_usable(b, frames, take * frames);
        const int step = pass ? take : 1;
        if (!mix_pass(b, frames, step, srcs + k, dsts + k, stream, may_chain, upload, pass)) return false;
        k += step;
    }
    return true;
}

bool mix_device(oalsfx_batch* b, int frames, const float* src, float* dst, hipStream_t stream, bool may_chain = false)
{
    float* out = dst;
    return mix_device(b, frames, 1, &src, &out, stream, may_chain, false);
}

} // namespace

extern "C" {

const char* oalsfx_last_error(void) { return g_last_error.c_str(); }

oalsfx_batch* oalsfx_batch_create(int n_instances, int channel_format, int sampling_rate, int effect_count, int device_id)
{
    g_last_error.clear();
    const int channels = channel_count_of(static_cast<oalsfxpp::ChannelFormat>(channel_format));
    // same checks and messages as Api::Impl::initialize (reference src/oalsfxpp.cpp:2853-2871)
    if (channels == 0) { g_last_error = "Invalid channel format."; return nullptr; }
    if (sampling_rate < min_sampling_rate) { g_last_error = "Sampling rate is out of range."; return nullptr; }
    if (effect_count <= 0 || effect_count > OALSFX_MAX_SLOTS) { g_last_error = "Effect count is out of range."; return nullptr; }
    if (n_instances <= 0) { g_last_error = "Instance count is out of range."; return nullptr; }

    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count <= 0) {
        g_last_error = "No HIP device available: the effect process path has no CPU fallback.";
        return nullptr;
    }
    if (device_id < 0 || device_id >= device_count) { g_last_error = "HIP device ordinal is out of range."; return nullptr; }
    if (hipSetDevice(device_id) != hipSuccess) { g_last_error = "hipSetDevice failed."; return nullptr; }

    auto* b = new (std::nothrow) oalsfx_batch{};
    if (!b) { g_last_error = "Failed to allocate the batch."; return nullptr; }
    b->n = n_instances;
    b->slots = effect_count;
    b->channels = channels;
    b->rate = sampling_rate;
    b->format = channel_format;
    b->device = device_id;
    b->dev.init(static_cast<oalsfxpp::ChannelFormat>(channel_format), sampling_rate);
    b->channels = b->dev.channels;
    const size_t total = static_cast<size_t>(n_instances) * effect_count;
    b->inst.resize(n_instances);
    b->h_params.assign(total, oalsfx_slot_params{});
    b->h_state_init.assign(total, oalsfx_slot_state{});
    b->started_at.assign(total, 0);
    b->h_source.assign(n_instances, oalsfx_source_params{});
    b->seq.assign(total, 0);
    b->h_rings.assign(total, nullptr);
    b->ring_floats.assign(total, 0);
    b->inst_dirty.assign(n_instances, 0);
    b->inst_filtered.assign(n_instances, 0);
    b->touched.assign(n_instances, 0);
    b->aux_written.assign(n_instances, 0);
    for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
        b->route_bus[s].assign(n_instances, s == 0 ? 0 : -1);
        b->route_gain[s].assign(n_instances, 1.0F);
        b->route_ramp[s].assign(n_instances, oalsfx_batch::SendRamp{});
    }
    b->since_update.assign(total, 0);
    b->slot_class.assign(total, 0);
    b->in_settling.assign(total, 0);
    b->xf_ok.assign(total, 0);
    b->mod_ever.assign(total, 0);
    b->proven.assign(total, 0);
    b->updated_gen.assign(total, 0);
    b->inst_epoch.assign(n_instances, 1); // a zero-filled hot record never carries a valid stamp
    for (int i = 0; i < n_instances; ++i) {
        b->inst[i].initialize(effect_count);
        mark_dirty(b, i);
    }
    mark_touched(b, 0, n_instances);

    bool ok = b->hip_ok(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking), "hipStreamCreate");
    b->chain_stream[0] = b->stream;
    for (int k = 1; k < kChainDepth; ++k) {
        ok = ok && b->hip_ok(hipStreamCreateWithFlags(&b->chain_stream[k], hipStreamNonBlocking), "hipStreamCreate");
        ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_chain[k], hipEventDisableTiming), "hipEventCreate");
    }
    {
        // can a call of this batch ever be a chained launch?  (chain_eligible has the conditions that change from call to call)
        const char* kind = std::getenv("OALSFX_RING_MEMORY");
        b->uncached = (!kind || std::strcmp(kind, "uncached") == 0) && uncached_memory_available(b->device);
    }
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_chain_start, hipEventDisableTiming), "hipEventCreate");
    for (int k = 0; k < kSideStreams; ++k) {
        ok = ok && b->hip_ok(hipStreamCreateWithFlags(&b->side_stream[k], hipStreamNonBlocking), "hipStreamCreate");
        ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_join[k], hipEventDisableTiming), "hipEventCreate");
    }
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_uploaded, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_mixed, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_downmix, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_dm_order, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_sampler, hipEventDisableTiming), "hipEventCreate");
    ok = ok && each_voice_table(b, [b](auto& r) { return records_create(b, r, b->n); });
    b->sweep_set.assign(n_instances, 0);
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_params), total * sizeof(oalsfx_slot_params)), "hipMalloc(params)");
    ok = ok && b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_state), total * sizeof(oalsfx_hip::SlotStateLines)), "hipMalloc(state)");
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_source), n_instances * sizeof(oalsfx_source_params)), "hipMalloc(source)");
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_rings), total * sizeof(float*)), "hipMalloc(ring table)");
    ok = ok && b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_source_state), n_instances * sizeof(oalsfx_source_state)), "hipMalloc(source state)");
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_lists_buf[0]), (kChainDepth + 1) * total * sizeof(int)), "hipMalloc(lists)");
    if (ok) {
        for (int k = 1; k <= kChainDepth; ++k) b->d_lists_buf[k] = b->d_lists_buf[0] + k * total;
        b->d_lists = b->d_lists_buf[0];
    }
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_progress), total * sizeof(int)), "hipMalloc(progress)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_progress, 0, total * sizeof(int), b->stream), "hipMemsetAsync(progress)");
    ok = ok && b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_hot), total * oalsfx_hip::hot::SIZE * sizeof(unsigned)), "hipMalloc(hot records)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_hot, 0, total * oalsfx_hip::hot::SIZE * sizeof(unsigned), b->stream), "hipMemsetAsync(hot records)");
    ok = ok && b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_inst_epoch), n_instances * sizeof(unsigned)), "hipMalloc(epochs)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_inst_epoch, 0, n_instances * sizeof(unsigned), b->stream), "hipMemsetAsync(epochs)");
    ok = ok && b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_turn), (3 * total + 16) * sizeof(unsigned)), "hipMalloc(turns)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_turn, 0, (3 * total + 16) * sizeof(unsigned), b->stream), "hipMemsetAsync(turns)");
    ok = ok && b->hip_ok(handed_on_malloc(b, reinterpret_cast<void**>(&b->d_exact), total * sizeof(unsigned)), "hipMalloc(exact)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_exact, 0, total * sizeof(unsigned), b->stream), "hipMemsetAsync(exact)");
    ok = ok && b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_exact), total * sizeof(unsigned)), "hipHostMalloc(exact)");
    ok = ok && b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_fault), 2 * sizeof(unsigned), hipHostMallocMapped), "hipHostMalloc(fault)");
    if (ok) b->h_fault[0] = b->h_fault[1] = 0;
    ok = ok && b->hip_ok(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->d_fault), b->h_fault, 0), "hipHostGetDevicePointer");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_exact, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipEventCreateWithFlags(&b->ev_state_io, hipEventDisableTiming), "hipEventCreate");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_state, 0, total * sizeof(oalsfx_hip::SlotStateLines), b->stream), "hipMemsetAsync(state)");
    ok = ok && b->hip_ok(hipMemsetAsync(b->d_source_state, 0, n_instances * sizeof(oalsfx_source_state), b->stream), "hipMemsetAsync(source state)");
    if (ok && std::getenv("OALSFX_DEBUG_TIMELINE")) {
        ok = b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_timeline), kTimelineBytes), "hipMalloc(timeline)");
        ok = ok && b->hip_ok(hipMemsetAsync(b->d_timeline, 0, kTimelineBytes, b->stream), "hipMemsetAsync(timeline)");
    }
    if (!ok) {
        g_last_error = b->error;
        oalsfx_batch_destroy(b);
        return nullptr;
    }
    return b;
}

void oalsfx_batch_destroy(oalsfx_batch* b)
{
    if (!b) return;
    hipSetDevice(b->device);
    join_flush(b);
    for (int k = 1; k < kChainDepth; ++k)
        if (b->chain_stream[k]) hipStreamSynchronize(b->chain_stream[k]);
    if (b->stream) hipStreamSynchronize(b->stream);
    for (int k = 0; k < kSideStreams; ++k)
        if (b->side_stream[k]) hipStreamSynchronize(b->side_stream[k]);
    if (b->exact_pending) hipEventSynchronize(b->ev_exact); // a read-back on a caller's stream still writes to h_exact
    if (b->d_timeline) {
        // phase stamps of the last steady-state reverb launch, for scripts/timeline.py
        std::vector<unsigned long long> h(kTimelineBytes / sizeof(unsigned long long));
        if (hipMemcpy(h.data(), b->d_timeline, kTimelineBytes, hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE* f = std::fopen(std::getenv("OALSFX_DEBUG_TIMELINE"), "wb")) { std::fwrite(h.data(), 1, kTimelineBytes, f); std::fclose(f); }
        hipFree(b->d_timeline);
    }
    for (auto& t : b->timed) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
    for (hipEvent_t e : b->event_pool) hipEventDestroy(e);
    if (std::getenv("OALSFX_HOST_PROFILE"))
        std::fprintf(stderr, "host profile: prepare_params %.1f ms (of which waiting for a staging buffer %.1f ms), %lld mix_device calls chained\n",
                     b->host_prepare_ns * 1e-6, b->host_stage_wait_ns * 1e-6, b->chained_calls);
    for (void* c : b->chunks) handed_on_free(c);
    hipFree(b->d_params); handed_on_free(b->d_state); hipFree(b->d_source); hipFree(b->d_rings); handed_on_free(b->d_source_state); hipFree(b->d_filtered);
    handed_on_free(b->d_mixbuf); hipFree(b->d_lists_buf[0]); hipFree(b->d_progress); hipFree(b->d_io_src); hipFree(b->d_io_dst);
    handed_on_free(b->d_hot); hipFree(b->d_inst_epoch); handed_on_free(b->d_exact); handed_on_free(b->d_turn);
    for (int k = 1; k < kChainDepth; ++k)
        if (b->ev_chain[k]) hipEventDestroy(b->ev_chain[k]);
    if (b->ev_chain_start) hipEventDestroy(b->ev_chain_start);
    for (int k = 1; k < kChainDepth; ++k)
        if (b->chain_stream[k]) hipStreamDestroy(b->chain_stream[k]);
    if (b->h2d_stream) hipStreamSynchronize(b->h2d_stream);
    if (b->d2h_stream) hipStreamSynchronize(b->d2h_stream);
    for (auto& ps : b->pipe) {
        hipFree(ps.d_src); hipFree(ps.d_dst);
        if (ps.copied_in) hipEventDestroy(ps.copied_in);
        if (ps.mixed) hipEventDestroy(ps.mixed);
        if (ps.copied_out) hipEventDestroy(ps.copied_out);
    }
    if (b->h2d_stream) hipStreamDestroy(b->h2d_stream);
    if (b->d2h_stream) hipStreamDestroy(b->d2h_stream);
    if (b->h_io_src) (void)hipHostFree(b->h_io_src);
    if (b->h_io_dst) (void)hipHostFree(b->h_io_dst);
    if (b->h_exact) (void)hipHostFree(b->h_exact);
    if (b->h_fault) (void)hipHostFree(b->h_fault);
    if (b->h_join) (void)hipHostFree(b->h_join);
    handed_on_free(b->d_join_tables);
    if (b->ev_exact) hipEventDestroy(b->ev_exact);
    if (b->h_state_io) (void)hipHostFree(b->h_state_io);
    hipFree(b->d_state_io);
    if (b->ev_state_io) hipEventDestroy(b->ev_state_io);
    if (b->dm_pending) hipEventSynchronize(b->ev_downmix); // a downmix on a caller's stream still reads the table
    if (b->h_dm_table) (void)hipHostFree(b->h_dm_table);
    hipFree(b->d_dm_table); hipFree(b->d_dm_partials); hipFree(b->d_dm_out);
    hipFree(b->d_meters);
    if (b->sampler_pending) hipEventSynchronize(b->ev_sampler); // a render on a caller's stream still reads and writes the records
    if (b->ev_sampler) hipEventDestroy(b->ev_sampler);
    each_voice_table(b, [](auto& r) { records_release(r); return true; });
    if (!b->programs.d) records_release(b->programs); // (never made, or not to the end: its event may be there)
    if (!b->filter_programs.d) records_release(b->filter_programs);
    records_release(b->streams);
    hipFree(b->d_stream_taken);
    hipFree(b->d_voice_scratch);
    for (int t = 0; t < OALSFX_FIR_TABLES; ++t) hipFree(const_cast<float*>(b->fir.coef[t]));
    if (b->ev_downmix) hipEventDestroy(b->ev_downmix);
    if (b->ev_dm_order) hipEventDestroy(b->ev_dm_order);
    for (int k = 0; k < kSideStreams; ++k) {
        if (b->side_stream[k]) hipStreamDestroy(b->side_stream[k]);
        if (b->ev_join[k]) hipEventDestroy(b->ev_join[k]);
    }
    if (b->ev_fork) hipEventDestroy(b->ev_fork);
    if (b->ev_uploaded) hipEventDestroy(b->ev_uploaded);
    if (b->ev_mixed) hipEventDestroy(b->ev_mixed);
    for (auto& st : b->stage) {
        if (st.host) (void)hipHostFree(st.host);
        if (st.dev) (void)hipFree(st.dev);
        if (st.done) hipEventDestroy(st.done);
    }
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
}

const char* oalsfx_batch_error(const oalsfx_batch* b) { return b ? b->error : g_last_error.c_str(); }
int oalsfx_batch_instances(const oalsfx_batch* b) { return b->n; }
int oalsfx_batch_channels(const oalsfx_batch* b) { return b->channels; }
int oalsfx_batch_sampling_rate(const oalsfx_batch* b) { return b->rate; }
int oalsfx_batch_effect_count(const oalsfx_batch* b) { return b->slots; }

int oalsfx_batch_set_effect(oalsfx_batch* b, int first, int count, int slot, const oalsfx_effect* effects, int stride_bytes)
{
    if (!range_ok(b, first, count)) return 0;
    if (slot < 0 || slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    const auto* base = reinterpret_cast<const unsigned char*>(effects);
    for (int i = 0; i < count; ++i)
        std::memcpy(&b->inst[first + i].deferred[slot], base + static_cast<size_t>(i) * stride_bytes, sizeof(oalsfx_effect));
    mark_touched(b, first, count);
    return 1;
}

int oalsfx_batch_set_effect_at(oalsfx_batch* b, const int* instances, int count, int slot, const oalsfx_effect* effects, int stride_bytes)
{
    if (count < 0 || (count > 0 && (!instances || !effects))) return b->fail(kErrRange) ? 1 : 0;
    if (slot < 0 || slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    for (int k = 0; k < count; ++k)
        if (instances[k] < 0 || instances[k] >= b->n) return b->fail(kErrRange) ? 1 : 0; // (nothing is set when one index is out of range)
    const auto* base = reinterpret_cast<const unsigned char*>(effects);
    for (int k = 0; k < count; ++k) {
        std::memcpy(&b->inst[instances[k]].deferred[slot], base + static_cast<size_t>(k) * stride_bytes, sizeof(oalsfx_effect));
        mark_touched(b, instances[k], 1);
    }
    return 1;
}

int oalsfx_batch_set_effect_type(oalsfx_batch* b, int first, int count, int slot, int effect_type)
{
    if (!range_ok(b, first, count)) return 0;
    if (slot < 0 || slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    for (int i = 0; i < count; ++i) b->inst[first + i].deferred[slot].set_type_and_defaults(static_cast<oalsfxpp::EffectType>(effect_type));
    mark_touched(b, first, count);
    return 1;
}

int oalsfx_batch_set_effect_props(oalsfx_batch* b, int first, int count, int slot, const void* props, int stride_bytes)
{
    if (!range_ok(b, first, count)) return 0;
    if (slot < 0 || slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    const auto* base = static_cast<const unsigned char*>(props);
    for (int i = 0; i < count; ++i)
        std::memcpy(&b->inst[first + i].deferred[slot].props_, base + static_cast<size_t>(i) * stride_bytes, sizeof(oalsfxpp::EffectProps));
    mark_touched(b, first, count);
    return 1;
}

int oalsfx_batch_set_send_props(oalsfx_batch* b, int first, int count, int slot, const oalsfx_send_props* props)
{
    if (!range_ok(b, first, count)) return 0;
    if (slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    oalsfxpp::SendProps p;
    p.gain_ = props->gain; p.gain_hf_ = props->gain_hf; p.gain_lf_ = props->gain_lf;
    for (int i = 0; i < count; ++i) {
        InstanceHost& h = b->inst[first + i];
        // direct: deferred copy; auxiliary: the reference writes the active properties (src/oalsfxpp.cpp:3728-3733)
        if (slot < 0) h.direct_deferred = p;
        else { h.aux_props[slot] = p; b->aux_written[first + i] = 1; }
    }
    mark_touched(b, first, count);
    return 1;
}

int oalsfx_batch_get_effect(const oalsfx_batch* b, int instance, int slot, int deferred, oalsfx_effect* out)
{
    if (instance < 0 || instance >= b->n || slot < 0 || slot >= b->slots) return 0;
    const InstanceHost& h = b->inst[instance];
    std::memcpy(out, deferred ? &h.deferred[slot] : &h.active[slot], sizeof(oalsfx_effect));
    return 1;
}

int oalsfx_batch_get_send_props(const oalsfx_batch* b, int instance, int slot, int deferred, oalsfx_send_props* out)
{
    if (instance < 0 || instance >= b->n || slot >= b->slots) return 0;
    const InstanceHost& h = b->inst[instance];
    const oalsfxpp::SendProps& p = slot < 0 ? (deferred ? h.direct_deferred : h.direct_props) : (deferred ? h.aux_deferred[slot] : h.aux_props[slot]);
    out->gain = p.gain_; out->gain_hf = p.gain_hf_; out->gain_lf = p.gain_lf_;
    return 1;
}

int oalsfx_batch_apply_changes(oalsfx_batch* b, int first, int count)
{
    if (!range_ok(b, first, count)) return 0;
    size_t kept = 0;
    for (size_t k = 0; k < b->touched_list.size(); ++k) {
        const int i = b->touched_list[k];
        if (i < first || i >= first + count) { b->touched_list[kept++] = i; continue; }
        InstanceHost& h = b->inst[i];
        h.apply_changes();
        bool dirty = h.source_changed;
        for (int s = 0; s < b->slots; ++s) dirty |= h.slot_changed[s];
        if (dirty) mark_dirty(b, i);
        // An auxiliary send whose properties were ever set differs from its never-written deferred copy for good, and the
        // reference then recomputes that source on every apply (src/oalsfxpp.cpp:3772-3780): such an instance stays listed.
        bool sticky = false;
        for (int s = 0; s < b->slots; ++s) sticky |= !oalsfxpp::SendProps::are_equal(h.aux_props[s], h.aux_deferred[s]);
        if (sticky) b->touched_list[kept++] = i;
        else b->touched[i] = 0;
    }
    b->touched_list.resize(kept);
    return 1;
}

int oalsfx_batch_mix_device(oalsfx_batch* b, int frames, const float* src_dev, float* dst_dev, void* hip_stream)
{
    if (frames == 0) return 1;
    if (frames < 0) return b->fail("Frame count is negative.") ? 1 : 0;
    if (!src_dev) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_dev) return b->fail(kErrNoDst) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0;
    // (calls on the batch's own stream may overlap with their neighbours: chained launches)
    return mix_device(b, frames, src_dev, dst_dev, hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream, hip_stream == nullptr) ? 1 : 0;
}

int oalsfx_batch_mix_device_multi(oalsfx_batch* b, int frames, int buffers, const float* const* src_dev, float* const* dst_dev, void* hip_stream)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (frames < 0) return b->fail("Frame count is negative.") ? 1 : 0;
    if (buffers < 0) return b->fail("Buffer count is negative.") ? 1 : 0;
    if (frames == 0 || buffers == 0) return 1;
    if (!src_dev) return b->fail("Null source buffer table.") ? 1 : 0;
    if (!dst_dev) return b->fail("Null destination buffer table.") ? 1 : 0;
    for (int k = 0; k < buffers; ++k) {
        if (!src_dev[k]) return b->fail(kErrNoSrc) ? 1 : 0;
        if (!dst_dev[k]) return b->fail(kErrNoDst) ? 1 : 0;
    }
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0;
    return mix_device(b, frames, buffers, src_dev, dst_dev, hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream, hip_stream == nullptr, true) ? 1 : 0;
}

namespace {

// The device staging buffers of the host-pointer calls, d_io_src and d_io_dst, for `floats` floats each.
bool grow_io(oalsfx_batch* b, size_t floats)
{
    if (floats <= b->io_capacity) return true;
    hipFree(b->d_io_src); hipFree(b->d_io_dst);
    b->d_io_src = b->d_io_dst = nullptr;
    b->io_capacity = 0;
    if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_io_src), floats * sizeof(float)), "hipMalloc(io)")) return false;
    if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_io_dst), floats * sizeof(float)), "hipMalloc(io)")) return false;
    b->io_capacity = floats;
    return true;
}

// Api::mix from host buffers: copy in, kernels, copy out on the batch's stream, then wait.  legs_us (may be null): the three legs as
// HIP events on that stream saw them.
int mix_host(oalsfx_batch* b, int frames, const float* src_host, float* dst_host, double* legs_us)
{
    if (legs_us) legs_us[0] = legs_us[1] = legs_us[2] = 0.0;
    if (frames == 0) return 1;
    if (frames < 0) return b->fail("Frame count is negative.") ? 1 : 0;
    if (!src_host) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_host) return b->fail(kErrNoDst) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    const size_t floats = static_cast<size_t>(b->n) * frames * b->channels;
    if (!grow_io(b, floats)) return 0;
    hipEvent_t ev[4] = {};
    if (legs_us)
        for (auto& e : ev) e = b->take_event();
    if (legs_us) hipEventRecord(ev[0], b->stream);
    if (!b->hip_ok(hipMemcpyAsync(b->d_io_src, src_host, floats * sizeof(float), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(src)")) return 0;
    if (legs_us) hipEventRecord(ev[1], b->stream);
    if (!mix_device(b, frames, b->d_io_src, b->d_io_dst, b->stream)) return 0;
    if (legs_us) hipEventRecord(ev[2], b->stream);
    if (!b->hip_ok(hipMemcpyAsync(dst_host, b->d_io_dst, floats * sizeof(float), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(dst)")) return 0;
    if (legs_us) hipEventRecord(ev[3], b->stream);
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    if (legs_us) {
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0F;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) legs_us[k] = ms * 1e3;
        }
        for (auto& e : ev) b->event_pool.push_back(e);
    }
    poll_exact(b);
    return check_fault(b) ? 1 : 0;
}

} // namespace

int oalsfx_batch_mix(oalsfx_batch* b, int frames, const float* src_host, float* dst_host) { return mix_host(b, frames, src_host, dst_host, nullptr); }

// Api::mix for callers that keep one source and one target buffer per instance -- thousands of oalsfxpp::Api objects' worth of them
// (reference src/oalsfxpp.h:872-875 takes one pair per object): the frames are gathered into one page-locked buffer, go through the
// batch as one call, and are scattered back.  The two passes over host memory cost more than the device's part (8 MB each way at 4096
// stereo instances of 256 frames), and still some thirty times less than a batch of one per object.
int oalsfx_batch_mix_gather(oalsfx_batch* b, int frames, const float* const* src_per_instance, float* const* dst_per_instance)
{
    if (frames == 0) return 1;
    if (frames < 0) return b->fail("Frame count is negative.") ? 1 : 0;
    if (!src_per_instance) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_per_instance) return b->fail(kErrNoDst) ? 1 : 0;
    const size_t per = static_cast<size_t>(frames) * b->channels, floats = per * b->n;
    for (int i = 0; i < b->n; ++i) {
        if (!src_per_instance[i]) return b->fail(kErrNoSrc) ? 1 : 0;
        if (!dst_per_instance[i]) return b->fail(kErrNoDst) ? 1 : 0;
    }
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0;
    if (floats > b->h_io_capacity) {
        if (b->h_io_src) (void)hipHostFree(b->h_io_src);
        if (b->h_io_dst) (void)hipHostFree(b->h_io_dst);
        b->h_io_src = b->h_io_dst = nullptr;
        b->h_io_capacity = 0;
        if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_io_src), floats * sizeof(float), hipHostMallocDefault), "hipHostMalloc(io)")) return 0;
        if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_io_dst), floats * sizeof(float), hipHostMallocDefault), "hipHostMalloc(io)")) return 0;
        b->h_io_capacity = floats;
    }
    for (int i = 0; i < b->n; ++i) std::memcpy(b->h_io_src + per * i, src_per_instance[i], per * sizeof(float));
    if (!mix_host(b, frames, b->h_io_src, b->h_io_dst, nullptr)) return 0;
    for (int i = 0; i < b->n; ++i) std::memcpy(dst_per_instance[i], b->h_io_dst + per * i, per * sizeof(float));
    return 1;
}

int oalsfx_batch_mix_timed(oalsfx_batch* b, int frames, const float* src_host, float* dst_host, double legs_us[3])
{
    return mix_host(b, frames, src_host, dst_host, legs_us);
}

namespace {

std::mutex g_pipe_mutex;
std::map<int, int> g_pipe_mode; // device -> form, once a batch has probed it

// Which form this call of oalsfx_batch_mix_async takes (oalsfx_batch::pipe_mode); while probing, also the probe's bookkeeping.
int pipe_form(oalsfx_batch* b)
{
    if (b->pipe_mode) return b->pipe_mode;
    if (const char* e = std::getenv("OALSFX_HOST_PIPELINE")) {
        const int m = std::atoi(e);
        if (m == 1 || m == 3) return b->pipe_mode = m;
    }
    {
        std::lock_guard<std::mutex> lock(g_pipe_mutex);
        auto it = g_pipe_mode.find(b->device);
        if (it != g_pipe_mode.end()) return b->pipe_mode = it->second;
    }
    // probing: calls 0 .. 15 on three streams (streams, events and staging buffers come into being, the copy engines see the caller's
    // buffers for the first time: not timed -- these calls took 1.2 ms each where the steady state takes 0.24), 16 .. 31 on one stream,
    // 32 .. 47 on three again; the clock runs over the last twelve of the second and third sixteen
    const long long k = b->pipe_turn;
    const auto now = std::chrono::steady_clock::now();
    if ((k & 15) == 4) b->pipe_probe_t0 = now;
    if (k == 32 || k == 48) b->pipe_probe_us[k == 48 ? 0 : 1] = std::chrono::duration<double, std::micro>(now - b->pipe_probe_t0).count() / 12.0;
    if (k < 48) return (k >= 16 && k < 32) ? 1 : 3;
    b->pipe_mode = b->pipe_probe_us[1] < b->pipe_probe_us[0] * 0.9 ? 1 : 3;
    std::lock_guard<std::mutex> lock(g_pipe_mutex);
    g_pipe_mode[b->device] = b->pipe_mode;
    return b->pipe_mode;
}

} // namespace

int oalsfx_batch_mix_async(oalsfx_batch* b, int frames, const float* src_host, float* dst_host)
{
    if (frames == 0) return 1;
    if (frames < 0) return b->fail("Frame count is negative.") ? 1 : 0;
    if (!src_host) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_host) return b->fail(kErrNoDst) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    const size_t floats = static_cast<size_t>(b->n) * frames * b->channels;
    if (!b->h2d_stream) {
        if (!b->hip_ok(hipStreamCreateWithFlags(&b->h2d_stream, hipStreamNonBlocking), "hipStreamCreate")) return 0;
        if (!b->hip_ok(hipStreamCreateWithFlags(&b->d2h_stream, hipStreamNonBlocking), "hipStreamCreate")) return 0;
        for (auto& ps : b->pipe) {
            if (!b->hip_ok(hipEventCreateWithFlags(&ps.copied_in, hipEventDisableTiming), "hipEventCreate")) return 0;
            if (!b->hip_ok(hipEventCreateWithFlags(&ps.mixed, hipEventDisableTiming), "hipEventCreate")) return 0;
            if (!b->hip_ok(hipEventCreateWithFlags(&ps.copied_out, hipEventDisableTiming), "hipEventCreate")) return 0;
        }
    }
    if (floats > b->pipe_capacity) {
        // a larger call than any before: let the pipeline drain, then grow every slot
        if (!b->hip_ok(hipStreamSynchronize(b->d2h_stream), "hipStreamSynchronize") || !b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
        for (auto& ps : b->pipe) {
            hipFree(ps.d_src); hipFree(ps.d_dst);
            ps.d_src = ps.d_dst = nullptr;
            ps.busy = false;
        }
        b->pipe_capacity = 0;
        for (auto& ps : b->pipe) {
            if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&ps.d_src), floats * sizeof(float)), "hipMalloc(io)")) return 0;
            if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&ps.d_dst), floats * sizeof(float)), "hipMalloc(io)")) return 0;
        }
        b->pipe_capacity = floats;
    }
    const int form = pipe_form(b);
    oalsfx_batch::PipeSlot& ps = b->pipe[b->pipe_turn++ % oalsfx_batch::kPipeDepth];
    // the call that used this staging slot kPipeDepth calls ago must be through: its output copy is the last thing it does
    if (ps.busy && !b->hip_ok(hipEventSynchronize(ps.copied_out), "hipEventSynchronize")) return 0;
    ps.busy = true;
    if (form == 1) {
        // one stream: the synchronous call's sequence, without its wait
        if (!b->hip_ok(hipMemcpyAsync(ps.d_src, src_host, floats * sizeof(float), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(src)")) return 0;
        if (!mix_device(b, frames, ps.d_src, ps.d_dst, b->stream)) return 0;
        if (!b->hip_ok(hipMemcpyAsync(dst_host, ps.d_dst, floats * sizeof(float), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(dst)")) return 0;
        return b->hip_ok(hipEventRecord(ps.copied_out, b->stream), "hipEventRecord") ? 1 : 0;
    }
    // The copies go through the runtime's copy engines.  (Measured in round 4 against kernels reading / writing the page-locked buffers
    // directly: 0.20 against 0.32 ms per step -- the reverb grid holds every CU, and the copy kernels' workgroups wait for its slots.)
    if (!b->hip_ok(hipMemcpyAsync(ps.d_src, src_host, floats * sizeof(float), hipMemcpyHostToDevice, b->h2d_stream), "hipMemcpyAsync(src)")) return 0;
    if (!b->hip_ok(hipEventRecord(ps.copied_in, b->h2d_stream), "hipEventRecord")) return 0;
    if (!b->hip_ok(hipStreamWaitEvent(b->stream, ps.copied_in, 0), "hipStreamWaitEvent")) return 0;
    if (!mix_device(b, frames, ps.d_src, ps.d_dst, b->stream)) return 0;
    if (!b->hip_ok(hipEventRecord(ps.mixed, b->stream), "hipEventRecord")) return 0;
    if (!b->hip_ok(hipStreamWaitEvent(b->d2h_stream, ps.mixed, 0), "hipStreamWaitEvent")) return 0;
    if (!b->hip_ok(hipMemcpyAsync(dst_host, ps.d_dst, floats * sizeof(float), hipMemcpyDeviceToHost, b->d2h_stream), "hipMemcpyAsync(dst)")) return 0;
    return b->hip_ok(hipEventRecord(ps.copied_out, b->d2h_stream), "hipEventRecord") ? 1 : 0;
}

int oalsfx_batch_wait(oalsfx_batch* b)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    if (b->d2h_stream && !b->hip_ok(hipStreamSynchronize(b->d2h_stream), "hipStreamSynchronize")) return 0;
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    for (auto& ps : b->pipe) ps.busy = false;
    poll_exact(b);
    return check_fault(b) ? 1 : 0;
}

void* oalsfx_pinned_alloc(unsigned long long bytes)
{
    void* p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void oalsfx_pinned_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int oalsfx_batch_synchronize(oalsfx_batch* b)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    if (std::getenv("OALSFX_HOST_PROFILE")) {
        std::fprintf(stderr, "host profile since the last synchronize: prepare_params %.1f us, of which staging-buffer waits %.1f us, derive %.1f us, lists %.1f us; %lld calls chained so far\n",
                     b->host_prepare_ns * 1e-3, b->host_stage_wait_ns * 1e-3, b->host_derive_ns * 1e-3, b->host_lists_ns * 1e-3, b->chained_calls);
        b->host_prepare_ns = b->host_stage_wait_ns = b->host_derive_ns = b->host_lists_ns = 0;
    }
    poll_exact(b);
    return check_fault(b) ? 1 : 0;
}

void* oalsfx_batch_stream(oalsfx_batch* b)
{
    // whoever holds the handle may queue work that expects the launches in stream order: no more chained launches for this batch
    b->stream_handed_out = true;
    if (hipSetDevice(b->device) == hipSuccess) (void)chain_join(b);
    return b->stream;
}

int oalsfx_batch_read_slot(oalsfx_batch* b, int instance, int slot, oalsfx_slot_params* params, oalsfx_slot_state* state)
{
    if (instance < 0 || instance >= b->n || slot < 0 || slot >= b->slots) return b->fail(kErrRange) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    if (!sync_params(b, nullptr)) return 0;
    const size_t idx = static_cast<size_t>(instance) * b->slots + slot;
    if (params) *params = b->h_params[idx];
    if (state) {
        if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
        if (!b->hip_ok(hipMemcpy(state, static_cast<const oalsfx_slot_state*>(b->d_state + idx), sizeof(*state), hipMemcpyDeviceToHost), "hipMemcpy(state)")) return 0;
    }
    return 1;
}

int oalsfx_batch_read_ring(oalsfx_batch* b, int instance, int slot, float* out, int max_floats)
{
    if (instance < 0 || instance >= b->n || slot < 0 || slot >= b->slots) return 0;
    if (hipSetDevice(b->device) != hipSuccess || !chain_join(b) || !sync_params(b, nullptr)) return 0;
    const size_t idx = static_cast<size_t>(instance) * b->slots + slot;
    const int floats = static_cast<int>(b->ring_floats[idx]);
    if (out && floats) {
        hipStreamSynchronize(b->stream);
        const int n = std::min(floats, max_floats);
        if (!b->hip_ok(hipMemcpy(out, b->h_rings[idx], static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(ring)")) return 0;
    }
    return floats;
}

int oalsfx_batch_read_source(oalsfx_batch* b, int instance, oalsfx_source_params* params, oalsfx_source_state* state)
{
    if (instance < 0 || instance >= b->n) return b->fail(kErrRange) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    if (!sync_params(b, nullptr)) return 0;
    if (params) *params = b->h_source[instance];
    if (state) {
        if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
        if (!b->hip_ok(hipMemcpy(state, b->d_source_state + instance, sizeof(*state), hipMemcpyDeviceToHost), "hipMemcpy(source state)")) return 0;
    }
    return 1;
}

// ---- instance state: snapshot, restore, reset -------------------------------------------------------------------------------------------
namespace {

// The blob (include/oalsfx_hip.h describes it for callers).  Position-independent: every place in it is an offset from its start, and
// every section starts on a 256-byte boundary.
//   header | entry table [count] | host records [count] | device records [count] | delay lines (each slot's ring, in entry order)
// The first three parts -- the prefix -- are what restore reads on the host; the device records and delay lines go from device to device.
constexpr uint32_t kBlobMagic = 0x58465342u; // "BSFX"
constexpr uint32_t kBlobVersion = 1;
constexpr size_t kBlobAlign = 256;

size_t blob_round(size_t v) { return (v + kBlobAlign - 1) / kBlobAlign * kBlobAlign; }

struct BlobHeader {
    uint32_t magic, version;
    int32_t format, rate, slots, count;
    uint64_t total_bytes;    // the whole blob
    uint64_t table_offset;   // BlobEntry[count]
    uint64_t prefix_bytes;   // header, entry table and host records
    uint64_t device_stride;  // bytes of one instance's device records
    uint64_t host_stride;    // bytes of one instance's host record
};
static_assert(sizeof(BlobHeader) <= kBlobAlign, "the header fits its section");

struct BlobEntry { uint64_t host, device, ring[OALSFX_MAX_SLOTS]; }; // offsets from the blob's start; ring 0: the slot holds none

struct BlobSlot {
    int32_t type;
    uint32_t ring_floats;
    uint32_t update_seq;          // of the parameters the slot ran with: the state has folded them in when its seen_seq says so
    uint32_t frames_since_start;  // frames mixed since the slot's state was started (the write position's place on the line grid)
    uint32_t mod_ever;            // the late line was modulated at some time since then (selects the builds that carry modulation)
    uint32_t reserved[3];
};

struct BlobHost {
    oalsfxpp::Effect active[OALSFX_MAX_SLOTS], deferred[OALSFX_MAX_SLOTS];
    oalsfxpp::SendProps direct_props, direct_deferred, aux_props[OALSFX_MAX_SLOTS], aux_deferred[OALSFX_MAX_SLOTS];
    BlobSlot slot[OALSFX_MAX_SLOTS];
    uint32_t touched;      // setters have written the instance since it was last applied (apply_changes visits it)
    uint32_t aux_written;  // an auxiliary send was written since the sends were last derived: the device records hold the sends as derived
};
static_assert(std::is_trivially_copyable<oalsfxpp::Effect>::value && std::is_trivially_copyable<oalsfxpp::SendProps>::value, "records are bytes");

// One instance's device records: each slot's state (whole 128-byte lines, as in the batch), the send-filter histories and the sends as
// derived last.
constexpr size_t kStateBytes = sizeof(oalsfx_hip::SlotStateLines);
constexpr size_t kSourceStateBytes = sizeof(oalsfx_source_state);
constexpr size_t kSourceParamsBytes = sizeof(oalsfx_source_params);
static_assert(kStateBytes % 16 == 0 && kSourceStateBytes % 16 == 0 && kSourceParamsBytes % 16 == 0, "records copy in 16-byte pieces");
size_t source_state_at(int slots) { return slots * kStateBytes; }
size_t source_params_at(int slots) { return source_state_at(slots) + kSourceStateBytes; }
size_t device_stride(int slots) { return blob_round(source_params_at(slots) + kSourceParamsBytes); }

int instance_at(const int* instances, int k) { return instances ? instances[k] : k; }

bool instances_ok(oalsfx_batch* b, const int* instances, int count)
{
    if (count < 0 || (!instances && count > b->n)) return b->fail(kErrRange);
    if (instances)
        for (int k = 0; k < count; ++k)
            if (instances[k] < 0 || instances[k] >= b->n) return b->fail(kErrRange);
    return true;
}

// No instance is named twice (instances_ok has passed); `message` is the call's own text for one that is.
bool targets_distinct(oalsfx_batch* b, const int* instances, int count, const char* message)
{
    if (!instances) return true;
    std::vector<uint8_t> taken(b->n, 0);
    for (int k = 0; k < count; ++k) {
        if (taken[instances[k]]) return b->fail(message);
        taken[instances[k]] = 1;
    }
    return true;
}

// Layout of a snapshot of these instances with the slot types they hold now (applied changes included): entries, header; returns bytes.
uint64_t blob_layout(const oalsfx_batch* b, const int* instances, int count, std::vector<BlobEntry>& entries, BlobHeader& h)
{
    h = BlobHeader{};
    h.magic = kBlobMagic;
    h.version = kBlobVersion;
    h.format = b->format;
    h.rate = b->rate;
    h.slots = b->slots;
    h.count = count;
    h.table_offset = kBlobAlign;
    h.host_stride = blob_round(sizeof(BlobHost));
    h.device_stride = device_stride(b->slots);
    const uint64_t host0 = h.table_offset + blob_round(static_cast<size_t>(count) * sizeof(BlobEntry));
    h.prefix_bytes = host0 + static_cast<uint64_t>(count) * h.host_stride;
    uint64_t at = h.prefix_bytes + static_cast<uint64_t>(count) * h.device_stride;
    entries.assign(count, BlobEntry{});
    for (int k = 0; k < count; ++k) {
        const int i = instance_at(instances, k);
        entries[k].host = host0 + k * h.host_stride;
        entries[k].device = h.prefix_bytes + k * h.device_stride;
        for (int s = 0; s < b->slots; ++s) {
            const size_t floats = static_cast<size_t>(ring_floats_for(static_cast<int>(b->inst[i].active[s].type_), b->rate));
            if (!floats) continue;
            entries[k].ring[s] = at;
            at += blob_round(floats * sizeof(float));
        }
    }
    h.total_bytes = at;
    return at;
}

// Everything that is queued on the batch first: a run of chained launches joined, a launch on a caller's stream waited for (as
// prepare_params does).  The run ends here.
bool state_io_begin(oalsfx_batch* b)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return false;
    if (b->last_launch_stream && b->last_launch_stream != b->stream && !b->hip_ok(hipStreamWaitEvent(b->stream, b->ev_mixed, 0), "hipStreamWaitEvent"))
        return false;
    return true;
}

// The device side of a snapshot, restore or reset: the segments in one launch, then the seen_seq fix-ups, on the batch's stream.  `extra`:
// bytes built on the host, placed behind the tables in device memory; the first `from_extra` segments read from there (their src is an
// offset into `extra`).
bool state_io_launch(oalsfx_batch* b, std::vector<oalsfx_hip::StateSegment>& segs, const std::vector<oalsfx_hip::StateSeenFix>& fixes,
                     const std::vector<char>& extra, int from_extra, bool nontemporal)
{
    unsigned long long pieces = 0;
    for (const auto& s : segs) pieces += (s.bytes + oalsfx_hip::kStatePieceBytes - 1) / oalsfx_hip::kStatePieceBytes;
    const size_t seg_bytes = blob_round(segs.size() * sizeof(oalsfx_hip::StateSegment));
    const size_t piece_bytes = blob_round(pieces * sizeof(unsigned));
    const size_t fix_bytes = blob_round(fixes.size() * sizeof(oalsfx_hip::StateSeenFix));
    const size_t total = seg_bytes + piece_bytes + fix_bytes + blob_round(extra.size());
    if (total == 0) return true;
    // (the page-locked buffer of the call before is free once the launches that read its copy have run)
    if (b->state_io_pending && !b->hip_ok(hipEventSynchronize(b->ev_state_io), "hipEventSynchronize")) return false;
    b->state_io_pending = false;
    if (total > b->state_io_capacity) {
        if (b->h_state_io) (void)hipHostFree(b->h_state_io);
        hipFree(b->d_state_io);
        b->h_state_io = b->d_state_io = nullptr;
        b->state_io_capacity = 0;
        if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_state_io), total), "hipHostMalloc(state tables)")) return false;
        if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_state_io), total), "hipMalloc(state tables)")) return false;
        b->state_io_capacity = total;
    }
    char* const extra_dev = b->d_state_io + seg_bytes + piece_bytes + fix_bytes;
    unsigned* const piece_seg = reinterpret_cast<unsigned*>(b->h_state_io + seg_bytes);
    pieces = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
        oalsfx_hip::StateSegment& s = segs[k];
        if (static_cast<int>(k) < from_extra) s.src = extra_dev + reinterpret_cast<uintptr_t>(s.src);
        if ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) | s.bytes) % 16 != 0)
            return b->fail("Internal error: a state segment is not 16-byte aligned.");
        s.first_piece = pieces;
        const unsigned long long n = (s.bytes + oalsfx_hip::kStatePieceBytes - 1) / oalsfx_hip::kStatePieceBytes;
        for (unsigned long long g = 0; g < n; ++g) piece_seg[pieces + g] = static_cast<unsigned>(k);
        pieces += n;
    }
    std::memcpy(b->h_state_io, segs.data(), segs.size() * sizeof(oalsfx_hip::StateSegment));
    std::memcpy(b->h_state_io + seg_bytes + piece_bytes, fixes.data(), fixes.size() * sizeof(oalsfx_hip::StateSeenFix));
    if (!extra.empty()) std::memcpy(b->h_state_io + seg_bytes + piece_bytes + fix_bytes, extra.data(), extra.size());
    if (!b->hip_ok(hipMemcpyAsync(b->d_state_io, b->h_state_io, total, hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(state tables)")) return false;
    oalsfx_hip::launch_state_copy(reinterpret_cast<const oalsfx_hip::StateSegment*>(b->d_state_io), reinterpret_cast<const unsigned*>(b->d_state_io + seg_bytes),
                                  pieces, nontemporal, b->stream);
    oalsfx_hip::launch_state_seen_fix(reinterpret_cast<const oalsfx_hip::StateSeenFix*>(b->d_state_io + seg_bytes + piece_bytes), static_cast<int>(fixes.size()), b->stream);
    if (!b->hip_ok(hipGetLastError(), "state copy launch")) return false;
    if (!b->hip_ok(hipEventRecord(b->ev_state_io, b->stream), "hipEventRecord")) return false;
    b->state_io_pending = true;
    b->state_io_unordered = true; // (mix_device: a launch on a caller's stream waits for these)
    return true;
}

// Puts image k into instance instances[k]: host records recs[k]; device records and delay lines from the blob at `blob` (entries[k]), or
// zeros where blob is nullptr (reset).  Everything has been validated: from here on only a HIP error can stop it.
// The host records become the instance's, every slot goes through prepare_params as a changed slot (parameters and sends derived anew, a
// new update_seq, a new epoch: no hot record of the instance is used again; proven, cross-fade and settling start over), and the device
// records and rings are copied over behind that upload.  A slot whose ring is of another size class gives its slab back and takes one of
// the image's.
bool put_images(oalsfx_batch* b, const int* instances, int count, const std::vector<BlobHost>& recs, const char* blob,
                const std::vector<BlobEntry>& entries, const std::vector<oalsfx_source_params>& sends)
{
    // pending changes of the targets first (what they held is replaced anyway; this keeps prepare_params' view simple)
    if (!sync_params(b, nullptr)) return false;
    // delay lines: slabs of the wrong size class go back to their pools, the pools grow where the images need more than they hold
    std::map<size_t, int> take, give;
    for (int k = 0; k < count; ++k)
        for (int s = 0; s < b->slots; ++s) {
            const size_t idx = static_cast<size_t>(instances[k]) * b->slots + s, want = recs[k].slot[s].ring_floats;
            if (b->ring_floats[idx] == want) continue;
            if (want) take[want] += 1;
            if (b->ring_floats[idx]) give[b->ring_floats[idx]] += 1;
        }
    std::map<size_t, int> need;
    for (auto& kv : take) {
        const int more = kv.second - give[kv.first];
        if (more > 0) need[kv.first] = more; // (the slabs given back below are there to be taken as well)
    }
    if (!grow_ring_pools(b, need)) return false;
    std::vector<size_t> taking;
    for (int k = 0; k < count; ++k)
        for (int s = 0; s < b->slots; ++s) {
            const size_t idx = static_cast<size_t>(instances[k]) * b->slots + s;
            if (b->ring_floats[idx] == recs[k].slot[s].ring_floats) continue;
            release_slab(b, idx);
            b->rings_table_dirty = true;
            if (recs[k].slot[s].ring_floats) taking.push_back(idx);
        }
    for (int k = 0, t = 0; k < count; ++k)
        for (int s = 0; s < b->slots; ++s) {
            const size_t idx = static_cast<size_t>(instances[k]) * b->slots + s;
            if (t >= static_cast<int>(taking.size()) || taking[t] != idx) continue;
            ++t;
            const size_t floats = recs[k].slot[s].ring_floats;
            RingPool& pool = b->pools[floats];
            std::vector<float*>& from = pool.free_clean.empty() ? pool.free_dirty : pool.free_clean; // (overwritten whole below: no zeroing)
            b->h_rings[idx] = from.back();
            from.pop_back();
            b->ring_floats[idx] = floats;
        }
    // host records; every slot and the sends count as changed
    for (int k = 0; k < count; ++k) {
        const int i = instances[k];
        const BlobHost& r = recs[k];
        InstanceHost& h = b->inst[i];
        h.effect_count = b->slots;
        for (int s = 0; s < OALSFX_MAX_SLOTS; ++s) {
            h.active[s] = r.active[s];
            h.deferred[s] = r.deferred[s];
            h.aux_props[s] = r.aux_props[s];
            h.aux_deferred[s] = r.aux_deferred[s];
            h.slot_changed[s] = s < b->slots;
            h.slot_retyped[s] = false; // (state and rings come from the image, not from a restart)
        }
        h.direct_props = r.direct_props;
        h.direct_deferred = r.direct_deferred;
        h.source_changed = true;
        for (int s = 0; s < b->slots; ++s) b->started_at[static_cast<size_t>(i) * b->slots + s] = b->frames_total - r.slot[s].frames_since_start;
        mark_dirty(b, i);
    }
    b->off_grid_known = false;
    if (!sync_params(b, nullptr)) return false;
    // what prepare_params decided from the targets' old selves, and what the image carries
    std::vector<oalsfx_hip::StateSegment> segs;
    std::vector<oalsfx_hip::StateSeenFix> fixes;
    for (int k = 0; k < count; ++k) {
        const int i = instances[k];
        const BlobHost& r = recs[k];
        const char* dev = blob ? blob + entries[k].device : nullptr;
        for (int s = 0; s < b->slots; ++s) {
            const size_t idx = static_cast<size_t>(i) * b->slots + s;
            b->xf_ok[idx] = 0; // (a cross-fade in flight continues on the general builds; the lists are sorted again below)
            b->mod_ever[idx] = r.slot[s].mod_ever ? 1 : 0; // (after prepare_params: it clears the flag on a type change)
            if (b->mod_ever[idx]) b->modulated[s] = true;
            segs.push_back({dev ? dev + s * kStateBytes : nullptr, b->d_state + idx, kStateBytes, 0});
            fixes.push_back({&b->d_state[idx].seen_seq, dev ? reinterpret_cast<const unsigned*>(dev + s * kStateBytes) : nullptr, r.slot[s].update_seq,
                             b->h_params[idx].update_seq});
            if (b->h_rings[idx]) segs.push_back({blob ? blob + entries[k].ring[s] : nullptr, b->h_rings[idx], b->ring_floats[idx] * sizeof(float), 0});
        }
        segs.push_back({dev ? dev + source_state_at(b->slots) : nullptr, b->d_source_state + i, kSourceStateBytes, 0});
        b->aux_written[i] = r.aux_written ? 1 : 0;
        if (r.aux_written && dev) {
            // the sends as the source had derived them (an auxiliary send written since waits for the next update there as well); read
            // back by restore, all of them in one copy
            const oalsfx_source_params& sp = sends[k];
            auto has_filter = [&](const oalsfx_source_params& x) {
                int any = x.direct.filter_type;
                for (int s = 0; s < b->slots; ++s)
                    if (x.aux[s].out_channels != 0) any |= x.aux[s].filter_type;
                return any != OALSFX_AF_NONE;
            };
            b->n_filtered += static_cast<int>(has_filter(sp)) - static_cast<int>(has_filter(b->h_source[i]));
            b->inst_filtered[i] = has_filter(sp) ? 1 : 0;
            b->inside_version = ~0u;
            b->h_source[i] = sp;
            segs.push_back({dev + source_params_at(b->slots), b->d_source + i, kSourceParamsBytes, 0});
            b->lists_dirty = true;
        }
        if (r.touched && !b->touched[i]) { b->touched[i] = 1; b->touched_list.push_back(i); }
        if (!r.touched) b->touched[i] = 0;
    }
    b->lists_dirty = true;
    b->touched_list.erase(std::remove_if(b->touched_list.begin(), b->touched_list.end(), [&](int i) { return !b->touched[i]; }), b->touched_list.end());
    return state_io_launch(b, segs, fixes, {}, 0, false);
}

} // namespace

unsigned long long oalsfx_batch_snapshot_bytes(oalsfx_batch* b, const int* instances, int count)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!instances_ok(b, instances, count)) return 0;
    std::vector<BlobEntry> entries;
    BlobHeader h;
    return blob_layout(b, instances, count, entries, h);
}

int oalsfx_batch_snapshot(oalsfx_batch* b, const int* instances, int count, void* dst, unsigned long long bytes)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!instances_ok(b, instances, count)) return 0;
    if (!dst) return b->fail("No snapshot buffer.") ? 1 : 0;
    if (reinterpret_cast<uintptr_t>(dst) % 16 != 0) return b->fail("The snapshot buffer is not 16-byte aligned.") ? 1 : 0;
    if (b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    std::vector<BlobEntry> entries;
    BlobHeader h;
    if (blob_layout(b, instances, count, entries, h) > bytes) return b->fail("The snapshot buffer is too small (oalsfx_batch_snapshot_bytes).") ? 1 : 0;
    // applied changes folded in first (as the read-backs do), so that parameters, state and rings describe one moment
    if (!state_io_begin(b) || !sync_params(b, nullptr)) return 0;
    std::vector<char> prefix(h.prefix_bytes, 0);
    std::memcpy(prefix.data(), &h, sizeof(h));
    std::memcpy(prefix.data() + h.table_offset, entries.data(), entries.size() * sizeof(BlobEntry));
    char* const out = static_cast<char*>(dst);
    std::vector<oalsfx_hip::StateSegment> segs;
    segs.push_back({nullptr, out, h.prefix_bytes, 0}); // (from the prefix built here: offset 0 of `extra`)
    for (int k = 0; k < count; ++k) {
        const int i = instance_at(instances, k);
        const InstanceHost& ih = b->inst[i];
        BlobHost r{};
        for (int s = 0; s < OALSFX_MAX_SLOTS; ++s) {
            r.active[s] = ih.active[s];
            r.deferred[s] = ih.deferred[s];
            r.aux_props[s] = ih.aux_props[s];
            r.aux_deferred[s] = ih.aux_deferred[s];
        }
        r.direct_props = ih.direct_props;
        r.direct_deferred = ih.direct_deferred;
        r.touched = b->touched[i];
        r.aux_written = b->aux_written[i];
        char* const dev = out + entries[k].device;
        for (int s = 0; s < b->slots; ++s) {
            const size_t idx = static_cast<size_t>(i) * b->slots + s;
            BlobSlot& sl = r.slot[s];
            sl.type = b->h_params[idx].type;
            sl.ring_floats = static_cast<uint32_t>(b->ring_floats[idx]);
            sl.update_seq = b->h_params[idx].update_seq;
            sl.frames_since_start = b->frames_total - b->started_at[idx];
            sl.mod_ever = b->mod_ever[idx];
            if (sl.ring_floats != static_cast<uint32_t>(ring_floats_for(sl.type, b->rate)) || (sl.ring_floats && !entries[k].ring[s]))
                return b->fail("Internal error: a slot's delay lines do not match its effect type.") ? 1 : 0;
            segs.push_back({b->d_state + idx, dev + s * kStateBytes, kStateBytes, 0});
            if (sl.ring_floats) segs.push_back({b->h_rings[idx], out + entries[k].ring[s], sl.ring_floats * sizeof(float), 0});
        }
        segs.push_back({b->d_source_state + i, dev + source_state_at(b->slots), kSourceStateBytes, 0});
        segs.push_back({b->d_source + i, dev + source_params_at(b->slots), kSourceParamsBytes, 0});
        std::memcpy(prefix.data() + entries[k].host, &r, sizeof(r));
    }
    return state_io_launch(b, segs, {}, prefix, 1, true) ? 1 : 0;
}

int oalsfx_batch_restore(oalsfx_batch* b, const int* instances, int count, const void* src, unsigned long long bytes)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!instances_ok(b, instances, count)) return 0;
    if (!src) return b->fail("No snapshot buffer.") ? 1 : 0;
    if (reinterpret_cast<uintptr_t>(src) % 16 != 0) return b->fail("The snapshot buffer is not 16-byte aligned.") ? 1 : 0;
    if (b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    if (!targets_distinct(b, instances, count, "An instance is listed twice as a restore target.")) return 0;
    std::vector<int> targets(count);
    for (int k = 0; k < count; ++k) targets[k] = instance_at(instances, k);
    if (bytes < sizeof(BlobHeader)) return b->fail("The snapshot is shorter than its header.") ? 1 : 0;
    // the blob may be the output of a snapshot queued on this batch: everything queued is through before its header is read
    if (!state_io_begin(b) || !b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    const char* const blob = static_cast<const char*>(src);
    BlobHeader h;
    if (!b->hip_ok(hipMemcpy(&h, blob, sizeof(h), hipMemcpyDefault), "hipMemcpy(snapshot header)")) return 0;
    if (h.magic != kBlobMagic) return b->fail("Not a snapshot (bad magic value).") ? 1 : 0;
    if (h.version != kBlobVersion) return b->fail("Snapshot version is not supported.") ? 1 : 0;
    if (h.format != b->format || h.rate != b->rate || h.slots != b->slots)
        return b->fail("The snapshot's channel format, sampling rate or effect count differs from the batch's.") ? 1 : 0;
    if (h.count != count) return b->fail("The snapshot holds another number of instances than the target list.") ? 1 : 0;
    if (h.total_bytes > bytes) return b->fail("The snapshot is larger than the bytes given.") ? 1 : 0;
    if (h.table_offset != kBlobAlign || h.host_stride != blob_round(sizeof(BlobHost)) || h.device_stride != device_stride(b->slots) ||
        h.prefix_bytes > h.total_bytes || h.table_offset + static_cast<uint64_t>(count) * sizeof(BlobEntry) > h.prefix_bytes)
        return b->fail("The snapshot's layout is damaged.") ? 1 : 0;
    std::vector<char> prefix(h.prefix_bytes);
    if (!b->hip_ok(hipMemcpy(prefix.data(), blob, prefix.size(), hipMemcpyDefault), "hipMemcpy(snapshot records)")) return 0;
    std::vector<BlobEntry> entries(count);
    std::memcpy(entries.data(), prefix.data() + h.table_offset, count * sizeof(BlobEntry));
    std::vector<BlobHost> recs(count);
    auto within = [&](uint64_t off, uint64_t len, uint64_t lo, uint64_t hi) { return off % 16 == 0 && off >= lo && off <= hi && len <= hi - off; };
    for (int k = 0; k < count; ++k) {
        const BlobEntry& e = entries[k];
        if (!within(e.host, sizeof(BlobHost), h.table_offset, h.prefix_bytes) || !within(e.device, h.device_stride, h.prefix_bytes, h.total_bytes))
            return b->fail("The snapshot's layout is damaged.") ? 1 : 0;
        std::memcpy(&recs[k], prefix.data() + e.host, sizeof(BlobHost));
        for (int s = 0; s < b->slots; ++s) {
            const BlobSlot& sl = recs[k].slot[s];
            const bool type_ok = sl.type >= 0 && sl.type < OALSFX_TYPE_COUNT && static_cast<int>(recs[k].active[s].type_) == sl.type;
            if (!type_ok || sl.ring_floats != static_cast<uint32_t>(ring_floats_for(sl.type, b->rate)) ||
                (sl.ring_floats && !within(e.ring[s], sl.ring_floats * sizeof(float), h.prefix_bytes, h.total_bytes)))
                return b->fail("The snapshot's records are damaged.") ? 1 : 0;
        }
    }
    // the sends as derived of the instances whose auxiliary sends were written since (BlobHost::aux_written): one copy of the device
    // records that span them
    std::vector<oalsfx_source_params> sends(count);
    uint64_t lo = ~uint64_t(0), hi = 0;
    for (int k = 0; k < count; ++k)
        if (recs[k].aux_written) { lo = std::min(lo, entries[k].device); hi = std::max(hi, entries[k].device + h.device_stride); }
    if (hi > lo) {
        std::vector<char> span(hi - lo);
        if (!b->hip_ok(hipMemcpy(span.data(), blob + lo, span.size(), hipMemcpyDefault), "hipMemcpy(sends)")) return 0;
        for (int k = 0; k < count; ++k)
            if (recs[k].aux_written) std::memcpy(&sends[k], span.data() + (entries[k].device - lo) + source_params_at(b->slots), sizeof(oalsfx_source_params));
    }
    return put_images(b, targets.data(), count, recs, blob, entries, sends) ? 1 : 0;
}

int oalsfx_batch_reset(oalsfx_batch* b, const int* instances, int count)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!instances_ok(b, instances, count)) return 0;
    if (b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    std::vector<int> targets(count);
    for (int k = 0; k < count; ++k) targets[k] = instance_at(instances, k);
    // the image of a freshly created instance (oalsfx_batch_create): Null effects, default sends, zeroed state, no delay lines
    InstanceHost fresh;
    fresh.initialize(b->slots);
    BlobHost r{};
    for (int s = 0; s < OALSFX_MAX_SLOTS; ++s) {
        r.active[s] = fresh.active[s];
        r.deferred[s] = fresh.deferred[s];
        r.aux_props[s] = fresh.aux_props[s];
        r.aux_deferred[s] = fresh.aux_deferred[s];
        r.slot[s].type = static_cast<int32_t>(fresh.active[s].type_);
    }
    r.direct_props = fresh.direct_props;
    r.direct_deferred = fresh.direct_deferred;
    if (!state_io_begin(b)) return 0;
    return put_images(b, targets.data(), count, std::vector<BlobHost>(count, r), nullptr, std::vector<BlobEntry>(count, BlobEntry{}),
                      std::vector<oalsfx_source_params>()) ? 1 : 0;
}

// ---- bus downmix (include/oalsfx_hip.h): routing, the device call, the host-pointer call ----
namespace {

std::atomic<int> g_downmix_vector{4}; // oalsfx_debug_downmix_vector

// The arguments every downmix call checks before anything is queued: counts, and that no instance is routed past the call's buses.
bool downmix_args_ok(oalsfx_batch* b, int frames, int n_buses)
{
    if (frames < 0) return b->fail("Frame count is negative.");
    if (n_buses < 1) return b->fail("Bus count is out of range.");
    if (b->poisoned) return b->fail(b->fault_text);
    if (static_cast<size_t>(frames) * b->channels > 0xFFFFFFFFull) return b->fail("Frame count is out of range.");
    if (b->routing_dirty) {
        b->route_max = -1;
        for (const std::vector<int>& send : b->route_bus)
            for (int v : send) b->route_max = std::max(b->route_max, v);
    }
    if (b->route_max >= n_buses)
        for (int i = 0; i < b->n; ++i)
            for (int s = 0; s < OALSFX_BUS_SENDS; ++s)
                if (b->route_bus[s][i] >= n_buses) {
                    char text[112];
                    if (s == 0) std::snprintf(text, sizeof(text), "Instance %d is routed to bus %d; the call has %d.", i, b->route_bus[s][i], n_buses);
                    else std::snprintf(text, sizeof(text), "Instance %d, send %d is routed to bus %d; the call has %d.", i, s, b->route_bus[s][i], n_buses);
                    b->error_store = text;
                    return b->fail(b->error_store.c_str());
                }
    return true;
}

// Frames of the ramp that have passed, at most all of them.
uint32_t ramp_done(const oalsfx_batch* b, const oalsfx_batch::SendRamp& r)
{
    const unsigned long long passed = b->dm_clock - r.start;
    return passed < r.frames ? static_cast<uint32_t>(passed) : r.frames;
}

// The gain the next downmixed frame gets from a send: the stated formula at n = done, the ramp's end once its frames have passed.
float send_gain_now(const oalsfx_batch* b, int send, int instance)
{
    const oalsfx_batch::SendRamp& r = b->route_ramp[send][instance];
    if (!r.frames) return b->route_gain[send][instance];
    const uint32_t done = ramp_done(b, r);
    return done < r.frames ? r.from + static_cast<float>(done) * r.step : r.to;
}

// A ramp whose frames have all passed ends: the send's gain is where it led.
void fold_ramp(oalsfx_batch* b, int send, int instance)
{
    oalsfx_batch::SendRamp& r = b->route_ramp[send][instance];
    if (r.frames && ramp_done(b, r) == r.frames) {
        b->route_gain[send][instance] = r.to;
        r = oalsfx_batch::SendRamp{};
    }
}

// Do [a, a + a_bytes) and [b, b + b_bytes) share a byte?
bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char* const a0 = static_cast<const char*>(a);
    const char* const b0 = static_cast<const char*>(b);
    return b0 < a0 + a_bytes && a0 < b0 + b_bytes;
}

// Puts `stream` behind whatever the batch has in flight (a run of chained launches is joined already): what a pass over the instances'
// outputs that is no effect call -- the downmix, the meters -- does before its own launches.
bool queue_behind_batch(oalsfx_batch* b, hipStream_t stream)
{
    if (stream == b->stream) {
        if (b->last_launch_stream && b->last_launch_stream != b->stream && !b->hip_ok(hipStreamWaitEvent(b->stream, b->ev_mixed, 0), "hipStreamWaitEvent"))
            return false;
    } else {
        // the batch's stream carries the joined run, parameter uploads, snapshots and restores; another caller's stream its last launch
        if (!b->hip_ok(hipEventRecord(b->ev_dm_order, b->stream), "hipEventRecord") || !b->hip_ok(hipStreamWaitEvent(stream, b->ev_dm_order, 0), "hipStreamWaitEvent"))
            return false;
        if (b->last_launch_stream && b->last_launch_stream != b->stream && b->last_launch_stream != stream &&
            !b->hip_ok(hipStreamWaitEvent(stream, b->ev_mixed, 0), "hipStreamWaitEvent"))
            return false;
    }
    return true;
}

// Queues the downmix of src, [n][elements], into dst, [n_buses][elements], on `stream` (arguments checked, device selected, a run of
// chained launches joined): behind whatever the batch has in flight, the table first where it has changed.
bool downmix_queue(oalsfx_batch* b, size_t elements, const float* src, int n_buses, float* dst, hipStream_t stream)
{
    if (!queue_behind_batch(b, stream)) return false;
    // a downmix still running elsewhere reads the table and writes the partials this one is about to
    if (b->dm_pending && b->dm_stream != stream && !b->hip_ok(hipStreamWaitEvent(stream, b->ev_downmix, 0), "hipStreamWaitEvent")) return false;
    // (a table with ramps whose last ramp has ended goes back to the plain level 1: one more upload)
    if (b->routing_dirty || b->dm_buses != n_buses || (b->dm_ramps_end && b->dm_clock >= b->dm_ramps_end)) {
        // (the page-locked copy is free once the copy of the table before, and with it the launches behind that, have run)
        if (b->dm_pending && !b->hip_ok(hipEventSynchronize(b->ev_downmix), "hipEventSynchronize")) return false;
        b->dm_pending = false;
        b->dm_buses = 0;
        // the ramps as of now: rows for the table only where a routed send still ramps
        const int* bus[OALSFX_BUS_SENDS];
        const float* gain[OALSFX_BUS_SENDS];
        const oalsfx_hip::DownmixRamp* ramp[OALSFX_BUS_SENDS];
        b->dm_ramps_end = 0;
        for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
            for (int i = 0; i < b->n; ++i) {
                fold_ramp(b, s, i);
                const oalsfx_batch::SendRamp& r = b->route_ramp[s][i];
                if (r.frames && b->route_bus[s][i] >= 0) b->dm_ramps_end = std::max(b->dm_ramps_end, r.start + r.frames);
            }
            bus[s] = b->route_bus[s].data();
            gain[s] = b->route_gain[s].data();
        }
        if (b->dm_ramps_end) {
            b->dm_ramp_rows.assign(static_cast<size_t>(OALSFX_BUS_SENDS) * b->n, oalsfx_hip::DownmixRamp{});
            for (int s = 0; s < OALSFX_BUS_SENDS; ++s) {
                oalsfx_hip::DownmixRamp* const rows = b->dm_ramp_rows.data() + static_cast<size_t>(s) * b->n;
                for (int i = 0; i < b->n; ++i) {
                    const oalsfx_batch::SendRamp& r = b->route_ramp[s][i];
                    if (r.frames) rows[i] = {r.from, r.step, r.to, r.frames, ramp_done(b, r)};
                }
                ramp[s] = rows;
            }
        }
        b->dm_table.build(bus, gain, b->dm_ramps_end ? ramp : nullptr, b->n, n_buses);
        b->dm_table_clock = b->dm_clock;
        size_t at[5];
        const size_t bytes = std::max<size_t>(b->dm_table.packed_bytes(at), 16);
        if (bytes > b->dm_table_capacity) {
            if (b->h_dm_table) (void)hipHostFree(b->h_dm_table);
            hipFree(b->d_dm_table);
            b->h_dm_table = b->d_dm_table = nullptr;
            b->dm_table_capacity = 0;
            if (!b->hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b->h_dm_table), bytes), "hipHostMalloc(downmix table)")) return false;
            if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&b->d_dm_table), bytes), "hipMalloc(downmix table)")) return false;
            b->dm_table_capacity = bytes;
        }
        b->dm_table.pack(b->h_dm_table);
        if (!b->hip_ok(hipMemcpyAsync(b->d_dm_table, b->h_dm_table, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(downmix table)")) return false;
        b->dm_dev.chunks = reinterpret_cast<const oalsfx_hip::DownmixChunk*>(b->d_dm_table + at[0]);
        b->dm_dev.sums = reinterpret_cast<const oalsfx_hip::DownmixSum*>(b->d_dm_table + at[1]);
        b->dm_dev.members = reinterpret_cast<const int*>(b->d_dm_table + at[2]);
        b->dm_dev.gains = reinterpret_cast<const float*>(b->d_dm_table + at[3]);
        b->dm_dev.ramps = b->dm_table.ramps.empty() ? nullptr : reinterpret_cast<const oalsfx_hip::DownmixRamp*>(b->d_dm_table + at[4]);
        b->dm_dev.n_chunks = static_cast<int>(b->dm_table.chunks.size());
        b->dm_dev.n_sums = static_cast<int>(b->dm_table.sums.size());
        b->dm_buses = n_buses;
        b->routing_dirty = false;
        ++b->dm_uploads;
        // the copy is in flight from here on, whatever becomes of the launches
        b->dm_pending = true;
        b->dm_stream = stream;
        if (!b->hip_ok(hipEventRecord(b->ev_downmix, stream), "hipEventRecord")) return false;
    }
    const int vector = oalsfx_hip::downmix_vector(src, dst, elements, g_downmix_vector.load(std::memory_order_relaxed));
    if (!oalsfx_hip::downmix_fits(b->dm_dev, elements, vector)) return b->fail("The downmix is too large for one launch.");
    if (!grow_device(b, &b->d_dm_partials, &b->dm_partials_capacity, static_cast<size_t>(b->dm_table.partial_rows) * elements, "hipMalloc(downmix partials)"))
        return false;
    oalsfx_hip::launch_downmix(b->dm_dev, src, dst, b->d_dm_partials, elements, vector, stream, b->channels, b->dm_clock - b->dm_table_clock);
    if (!b->hip_ok(hipGetLastError(), "downmix launch")) return false;
    b->dm_clock += elements / b->channels; // every ramp of the batch has moved on by the call's frames
    if (!b->hip_ok(hipEventRecord(b->ev_downmix, stream), "hipEventRecord")) return false;
    b->dm_pending = true;
    b->dm_stream = stream;
    return true;
}

} // namespace

int oalsfx_batch_set_routing(oalsfx_batch* b, int first, int count, const int* bus, const float* gain)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!range_ok(b, first, count)) return 0;
    if (bus)
        for (int k = 0; k < count; ++k)
            if (bus[k] < -1) return b->fail("Bus number is out of range.") ? 1 : 0;
    if (!bus && !gain) return 1;
    for (int k = 0; k < count; ++k) {
        if (bus) b->route_bus[0][first + k] = bus[k];
        if (gain) {
            b->route_gain[0][first + k] = gain[k];
            b->route_ramp[0][first + k] = oalsfx_batch::SendRamp{};
        }
    }
    if (count) b->routing_dirty = true;
    return 1;
}

int oalsfx_batch_get_routing(const oalsfx_batch* b, int instance, int* bus, float* gain)
{
    if (!b || instance < 0 || instance >= b->n) return 0;
    if (bus) *bus = b->route_bus[0][instance];
    if (gain) *gain = send_gain_now(b, 0, instance);
    return 1;
}

// ---- bus sends (include/oalsfx_hip.h) ----
namespace {

constexpr uint32_t kRampMaxFrames = 1U << 24;

// What the three send calls check before anything is changed.
bool send_args_ok(oalsfx_batch* b, int send, int first, int count)
{
    if (send < 0 || send >= OALSFX_BUS_SENDS) return b->fail("Send out of range.");
    if (!range_ok(b, first, count)) return false;
    if (b->poisoned) return b->fail(b->fault_text);
    return true;
}

} // namespace

int oalsfx_batch_set_send_routing(oalsfx_batch* b, int send, int first, int count, const int* bus, const float* gain)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!send_args_ok(b, send, first, count)) return 0;
    if (bus)
        for (int k = 0; k < count; ++k)
            if (bus[k] < -1) return b->fail("Bus number is out of range.") ? 1 : 0;
    if (!bus && !gain) return 1;
    for (int k = 0; k < count; ++k) {
        // (the table holds routed sends only: one that was and stays at bus -1 changes nothing in it)
        if (b->route_bus[send][first + k] >= 0 || (bus && bus[k] >= 0)) b->routing_dirty = true;
        if (bus) b->route_bus[send][first + k] = bus[k];
        if (gain) {
            b->route_gain[send][first + k] = gain[k];
            b->route_ramp[send][first + k] = oalsfx_batch::SendRamp{};
        }
    }
    return 1;
}

int oalsfx_batch_get_send_routing(const oalsfx_batch* b, int instance, int send, int* bus, float* gain, float* gain_to, uint32_t* frames_left)
{
    if (!b || instance < 0 || instance >= b->n || send < 0 || send >= OALSFX_BUS_SENDS) return 0;
    const oalsfx_batch::SendRamp& r = b->route_ramp[send][instance];
    const uint32_t left = r.frames ? r.frames - ramp_done(b, r) : 0;
    const float now = send_gain_now(b, send, instance);
    if (bus) *bus = b->route_bus[send][instance];
    if (gain) *gain = now;
    if (gain_to) *gain_to = left ? r.to : now;
    if (frames_left) *frames_left = left;
    return 1;
}

int oalsfx_batch_set_send_ramps(oalsfx_batch* b, int send, int first, int count, const float* gain_to, uint32_t frames)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!send_args_ok(b, send, first, count)) return 0;
    if (frames > kRampMaxFrames) return b->fail("Ramp length out of range.") ? 1 : 0;
    if (!gain_to) return count == 0 ? 1 : (b->fail("No ramp targets.") ? 1 : 0);
    for (int k = 0; k < count; ++k) {
        const int i = first + k;
        if (b->route_bus[send][i] >= 0) b->routing_dirty = true; // (a send at bus -1 ramps on the clock alone: nothing of it is in the table)
        if (frames == 0) {
            b->route_gain[send][i] = gain_to[k];
            b->route_ramp[send][i] = oalsfx_batch::SendRamp{};
            continue;
        }
        const float from = send_gain_now(b, send, i);
        oalsfx_batch::SendRamp r;
        r.from = from;
        r.step = (gain_to[k] - from) / static_cast<float>(frames);
        r.to = gain_to[k];
        r.frames = frames;
        r.start = b->dm_clock;
        b->route_gain[send][i] = from;
        b->route_ramp[send][i] = r;
    }
    return 1;
}

int oalsfx_batch_downmix_device(oalsfx_batch* b, int frames, const float* src_dev, int n_buses, float* dst_bus_dev, void* hip_stream)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!downmix_args_ok(b, frames, n_buses)) return 0;
    if (frames == 0) return 1;
    if (!src_dev) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_bus_dev) return b->fail(kErrNoDst) ? 1 : 0;
    const size_t elements = static_cast<size_t>(frames) * b->channels;
    if ((reinterpret_cast<uintptr_t>(src_dev) | reinterpret_cast<uintptr_t>(dst_bus_dev)) % sizeof(float) != 0)
        return b->fail("A downmix buffer is not 4-byte aligned.") ? 1 : 0;
    if (ranges_overlap(src_dev, static_cast<size_t>(b->n) * elements * sizeof(float), dst_bus_dev, static_cast<size_t>(n_buses) * elements * sizeof(float)))
        return b->fail("The bus buffer overlaps the source buffer.") ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    return downmix_queue(b, elements, src_dev, n_buses, dst_bus_dev, hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream) ? 1 : 0;
}

int oalsfx_batch_mix_downmix(oalsfx_batch* b, int frames, const float* src_host, int n_buses, float* dst_bus_host)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!downmix_args_ok(b, frames, n_buses)) return 0;
    if (frames == 0) return 1;
    if (!src_host) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_bus_host) return b->fail(kErrNoDst) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    const size_t elements = static_cast<size_t>(frames) * b->channels, floats = elements * b->n, bus_floats = elements * n_buses;
    if (!grow_io(b, floats) || !grow_device(b, &b->d_dm_out, &b->dm_out_capacity, bus_floats, "hipMalloc(bus output)")) return 0;
    if (!b->hip_ok(hipMemcpyAsync(b->d_io_src, src_host, floats * sizeof(float), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(src)")) return 0;
    if (!mix_device(b, frames, b->d_io_src, b->d_io_dst, b->stream)) return 0;
    if (!downmix_queue(b, elements, b->d_io_dst, n_buses, b->d_dm_out, b->stream)) return 0;
    if (!b->hip_ok(hipMemcpyAsync(dst_bus_host, b->d_dm_out, bus_floats * sizeof(float), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(buses)")) return 0;
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    b->dm_pending = false;
    poll_exact(b);
    return check_fault(b) ? 1 : 0;
}

// ---- level meters (include/oalsfx_hip.h) ----
namespace {

// What every meter call checks before anything is queued.
bool meter_args_ok(oalsfx_batch* b, int frames, float threshold, int flags)
{
    if (frames < 0) return b->fail("Frame count is negative.");
    if (!(threshold >= 0.0F)) return b->fail("The meter threshold is negative or not a number.");
    if (flags & ~OALSFX_METER_CARRY) return b->fail("Unknown meter flags.");
    if (b->poisoned) return b->fail(b->fault_text);
    if (static_cast<size_t>(frames) * b->channels > 0xFFFFFFFFull) return b->fail("Frame count is out of range.");
    return true;
}

// One launch on `stream`, which is behind the batch already; frames >= 1.
bool meter_launch(oalsfx_batch* b, int rows, int frames, const float* src, float threshold, int flags, oalsfx_meter* meters, hipStream_t stream)
{
    if (!oalsfx_hip::meter_fits(rows)) return b->fail("The meter pass is too large for one launch.");
    if (!oalsfx_hip::launch_meter(src, rows, static_cast<unsigned>(frames), b->channels, threshold, (flags & OALSFX_METER_CARRY) != 0, meters, stream))
        return b->fail("No meter kernel for this channel count.");
    return b->hip_ok(hipGetLastError(), "meter launch");
}

} // namespace

int oalsfx_batch_meter_device(oalsfx_batch* b, int rows, int frames, const float* src_dev, float threshold, int flags, oalsfx_meter* meters_dev,
                              void* hip_stream)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (rows < 1) return b->fail("Row count is out of range.") ? 1 : 0;
    if (!meter_args_ok(b, frames, threshold, flags)) return 0;
    if (!oalsfx_hip::meter_fits(rows)) return b->fail("The meter pass is too large for one launch.") ? 1 : 0;
    if (frames == 0) return 1;
    if (!src_dev) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!meters_dev) return b->fail("No meter records.") ? 1 : 0;
    if (reinterpret_cast<uintptr_t>(src_dev) % sizeof(float) != 0) return b->fail("The meter source is not 4-byte aligned.") ? 1 : 0;
    if (reinterpret_cast<uintptr_t>(meters_dev) % 16 != 0) return b->fail("The meter records are not 16-byte aligned.") ? 1 : 0;
    if (ranges_overlap(src_dev, static_cast<size_t>(rows) * frames * b->channels * sizeof(float), meters_dev, static_cast<size_t>(rows) * sizeof(oalsfx_meter)))
        return b->fail("The meter records overlap the source buffer.") ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    const hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream;
    if (!queue_behind_batch(b, stream)) return 0;
    return meter_launch(b, rows, frames, src_dev, threshold, flags, meters_dev, stream) ? 1 : 0;
}

namespace {

bool sampler_queue(oalsfx_batch* b, int frames, float* dst, hipStream_t stream);
constexpr int kEnvelopeMaxFrames = 1 << 24;
const char* const kErrEnvelopeFrames = "A render while an envelope is active has more than 2^24 frames.";

// oalsfx_batch_mix_downmix_meter, its input copied from src_host; or, with `play`, oalsfx_batch_play_downmix_meter, its input rendered by
// the samplers.
int downmix_meter_call(oalsfx_batch* b, int frames, const float* src_host, bool play, int n_buses, float* dst_bus_host, float threshold, int flags,
                       oalsfx_meter* voice_meters_host, oalsfx_meter* bus_meters_host)
{
    if (!meter_args_ok(b, frames, threshold, flags)) return 0;
    if (!play && !voice_meters_host && !bus_meters_host) return oalsfx_batch_mix_downmix(b, frames, src_host, n_buses, dst_bus_host);
    if (!downmix_args_ok(b, frames, n_buses)) return 0;
    if (!oalsfx_hip::meter_fits(std::max(b->n, n_buses))) return b->fail("The meter pass is too large for one launch.") ? 1 : 0;
    if (play && !oalsfx_hip::sampler_fits(b->n)) return b->fail("The sampler pass is too large for one launch.") ? 1 : 0;
    if (play && b->envelopes_active > 0 && frames > kEnvelopeMaxFrames) return b->fail(kErrEnvelopeFrames) ? 1 : 0;
    if (frames == 0) return 1;
    if (!play && !src_host) return b->fail(kErrNoSrc) ? 1 : 0;
    if (!dst_bus_host) return b->fail(kErrNoDst) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    const size_t elements = static_cast<size_t>(frames) * b->channels, floats = elements * b->n, bus_floats = elements * n_buses;
    const size_t records = static_cast<size_t>(b->n) + n_buses;
    if (!grow_io(b, floats) || !grow_device(b, &b->d_dm_out, &b->dm_out_capacity, bus_floats, "hipMalloc(bus output)")) return 0;
    if ((voice_meters_host || bus_meters_host) && !grow_device(b, &b->d_meters, &b->meters_capacity, records, "hipMalloc(meters)")) return 0;
    oalsfx_meter* const d_voices = b->d_meters;
    oalsfx_meter* const d_buses = b->d_meters + b->n;
    if (flags & OALSFX_METER_CARRY) {
        if (voice_meters_host &&
            !b->hip_ok(hipMemcpyAsync(d_voices, voice_meters_host, b->n * sizeof(oalsfx_meter), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(meters)"))
            return 0;
        if (bus_meters_host &&
            !b->hip_ok(hipMemcpyAsync(d_buses, bus_meters_host, n_buses * sizeof(oalsfx_meter), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(meters)"))
            return 0;
    }
    if (play) {
        if (!sampler_queue(b, frames, b->d_io_src, b->stream)) return 0;
    } else if (!b->hip_ok(hipMemcpyAsync(b->d_io_src, src_host, floats * sizeof(float), hipMemcpyHostToDevice, b->stream), "hipMemcpyAsync(src)")) return 0;
    if (!mix_device(b, frames, b->d_io_src, b->d_io_dst, b->stream)) return 0;
    if (!downmix_queue(b, elements, b->d_io_dst, n_buses, b->d_dm_out, b->stream)) return 0;
    // (behind the downmix on its stream: both only read the outputs, and the buses are written by then)
    if (voice_meters_host && !meter_launch(b, b->n, frames, b->d_io_dst, threshold, flags, d_voices, b->stream)) return 0;
    if (bus_meters_host && !meter_launch(b, n_buses, frames, b->d_dm_out, threshold, flags, d_buses, b->stream)) return 0;
    if (!b->hip_ok(hipMemcpyAsync(dst_bus_host, b->d_dm_out, bus_floats * sizeof(float), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(buses)")) return 0;
    if (voice_meters_host && bus_meters_host && bus_meters_host == voice_meters_host + b->n) {
        // one array for both: one copy
        if (!b->hip_ok(hipMemcpyAsync(voice_meters_host, d_voices, records * sizeof(oalsfx_meter), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(meters)"))
            return 0;
    } else {
        if (voice_meters_host &&
            !b->hip_ok(hipMemcpyAsync(voice_meters_host, d_voices, b->n * sizeof(oalsfx_meter), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(meters)"))
            return 0;
        if (bus_meters_host &&
            !b->hip_ok(hipMemcpyAsync(bus_meters_host, d_buses, n_buses * sizeof(oalsfx_meter), hipMemcpyDeviceToHost, b->stream), "hipMemcpyAsync(meters)"))
            return 0;
    }
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    b->dm_pending = false;
    poll_exact(b);
    return check_fault(b) ? 1 : 0;
}

} // namespace

int oalsfx_batch_mix_downmix_meter(oalsfx_batch* b, int frames, const float* src_host, int n_buses, float* dst_bus_host, float threshold, int flags,
                                   oalsfx_meter* voice_meters_host, oalsfx_meter* bus_meters_host)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    return downmix_meter_call(b, frames, src_host, false, n_buses, dst_bus_host, threshold, flags, voice_meters_host, bus_meters_host);
}

long long oalsfx_debug_downmix_uploads(const oalsfx_batch* b) { return b ? b->dm_uploads : 0; }
void oalsfx_debug_downmix_vector(int max_floats) { g_downmix_vector.store(max_floats, std::memory_order_relaxed); }

// ---- samplers (include/oalsfx_hip.h) ----
namespace {

constexpr uint32_t kSamplerFlags = OALSFX_SAMPLER_PLAYING | OALSFX_SAMPLER_LOOP | OALSFX_SAMPLER_LINEAR;

size_t pcm_bytes(uint32_t format) { return format == OALSFX_PCM_F32 ? 4 : format == OALSFX_PCM_S16 ? 2 : 1; }

// The device allocation a checked asset lay in: the records of one call mostly name a few assets, and the runtime is asked once for each run.
struct AssetRange { uintptr_t lo = 0, hi = 0; };

// Does [data, data + bytes) lie inside one allocation on the batch's device?
bool asset_resident(oalsfx_batch* b, uintptr_t data, uint64_t bytes, AssetRange& known)
{
    if (data >= known.lo && data <= known.hi && bytes <= known.hi - data) return true;
    hipPointerAttribute_t attr{};
    void* base = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&attr, reinterpret_cast<const void*>(data)) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != b->device ||
        hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, reinterpret_cast<hipDeviceptr_t>(data)) != hipSuccess) {
        (void)hipGetLastError(); // (an address the runtime does not know is an error of the caller's, not of the next launch)
        return false;
    }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
    if (data < lo || data - lo > size || bytes > size - (data - lo)) return false;
    known.lo = lo;
    known.hi = lo + size;
    return true;
}

// What oalsfx_batch_set_samplers refuses in one record.
bool sampler_ok(oalsfx_batch* b, const oalsfx_sampler& s, AssetRange& known)
{
    if (s.flags & ~kSamplerFlags) return b->fail("Unknown sampler flags.");
    if (s.format != OALSFX_PCM_U8 && s.format != OALSFX_PCM_S16 && s.format != OALSFX_PCM_F32) return b->fail("Unknown sampler format.");
    if (s.reserved != 0) return b->fail("The sampler's reserved field is not 0.");
    if (s.channels != 1 && s.channels != static_cast<uint32_t>(b->channels)) return b->fail("The sampler's channel count is neither 1 nor the batch's.");
    if (!(s.flags & OALSFX_SAMPLER_PLAYING)) return true;
    if (s.data == 0) return b->fail("A playing sampler has no data.");
    if (s.frames == 0 || s.frames >= 0x80000000U) return b->fail("The sampler's frame count is out of range.");
    if (s.data % pcm_bytes(s.format) != 0) return b->fail("The sampler's data is not aligned to its element size.");
    uint64_t end = static_cast<uint64_t>(s.frames) << OALSFX_SAMPLER_FRAC_BITS;
    if (s.flags & OALSFX_SAMPLER_LOOP) {
        if (s.loop_start >= s.loop_end || s.loop_end > s.frames) return b->fail("The sampler's loop region is out of range.");
        end = static_cast<uint64_t>(s.loop_end) << OALSFX_SAMPLER_FRAC_BITS;
    }
    if (s.position >= end) return b->fail("The sampler's position is past its end.");
    if (!asset_resident(b, static_cast<uintptr_t>(s.data), static_cast<uint64_t>(s.frames) * s.channels * pcm_bytes(s.format), known))
        return b->fail("The sampler's data does not lie inside one allocation on the batch's device.");
    return true;
}

// What both render calls check before anything is queued.
bool sampler_args_ok(oalsfx_batch* b, int frames)
{
    if (frames < 0) return b->fail("Frame count is negative.");
    if (b->poisoned) return b->fail(b->fault_text);
    if (static_cast<size_t>(frames) * b->channels > 0xFFFFFFFFull) return b->fail("Frame count is out of range.");
    if (!oalsfx_hip::sampler_fits(b->n)) return b->fail("The sampler pass is too large for one launch.");
    if (b->envelopes_active > 0 && frames > kEnvelopeMaxFrames) return b->fail(kErrEnvelopeFrames);
    return true;
}

// Room in the voice scratch for a render of `frames` frames with an active filter: a filtered voice goes through its instance's scratch
// row, which is grown behind the last render that used it (waited for only where the buffer is too small).
bool voice_scratch_fits(oalsfx_batch* b, int frames)
{
    const size_t floats = static_cast<size_t>(b->n) * static_cast<size_t>(frames) * b->channels;
    if (floats <= b->voice_scratch_capacity) return true;
    if (b->sampler_pending && !b->hip_ok(hipEventSynchronize(b->ev_sampler), "hipEventSynchronize")) return false;
    return grow_device(b, &b->d_voice_scratch, &b->voice_scratch_capacity, floats, "hipMalloc(voice scratch)");
}

// Queues a render of every instance's `frames` frames into dst on `stream` (arguments checked, device selected, a run of chained launches
// joined; frames >= 1): behind whatever the batch has in flight and behind the render before, the records set since then first.
bool sampler_queue(oalsfx_batch* b, int frames, float* dst, hipStream_t stream)
{
    if (!queue_behind_batch(b, stream)) return false;
    if (b->sampler_pending && b->sampler_stream != stream && !b->hip_ok(hipStreamWaitEvent(stream, b->ev_sampler, 0), "hipStreamWaitEvent")) return false;
    if (!each_voice_table(b, [b, stream](auto& r) { return r.table.pending() == 0 || records_upload(b, r, stream); })) return false;
    if (b->streams.d && b->streams.table.pending() != 0) {
        uint32_t* const taken = b->d_stream_taken;
        const auto launch = [taken](oalsfx_hip::StreamRing* rings, const int* index, const oalsfx_hip::StreamRing* changed, int count, hipStream_t s) {
            oalsfx_hip::launch_stream_upload(rings, taken, index, changed, count, s);
        };
        // (a failure behind the launch leaves `reset` in rows whose counts the device has zeroed: the batch's stream is broken then, and a
        // second zeroing of a count no render has advanced since changes nothing)
        if (!records_upload(b, b->streams, stream, launch)) return false;
        // (the staged rows have taken `reset` along: the host's rows drop it, so that an append does not zero the count again)
        for (const int i : b->stream_reset_list) b->streams.table.host[i].reset = 0;
        b->stream_reset_list.clear();
    }
    // While the host cannot rule out a ring that holds an entry (streams_open > 0) the render walks the rings and the envelope queues,
    // at any polyphony: k_stream_filter_rows if any filter is ACTIVE, in front of the filter stage at its most general (it looks at the
    // sweeps and at the filter programs' queues whatever their horizons say), else k_stream_rows.  Otherwise the ladder as it stood:
    // What is launched: while a voice's queue may hold a segment (program_horizon > 0) the renders with the queues beside the other
    // tables, at any polyphony; else while any voice's filter is ACTIVE the voices' render with the filters, at any polyphony (and
    // while a sweep may be under way, sweep_horizon > 0, either of the two with the sweeps beside the filters); else with
    // two lanes or more every instance's voices summed into its row; else while any instance names a table the render with the
    // resamplers; else while any envelope takes part the render with the envelopes; else the samplers alone.
    // While a voice's filter program may hold a queued segment (filter_program_horizon > 0) the swept renders walk those queues too.
    const bool rings = b->streams_open > 0, biquads = b->filters_active > 0;
    const bool queues = rings ? b->programs.d != nullptr : b->program_horizon > 0, swept = biquads && (rings || b->sweep_horizon > 0);
    const bool filter_queues = biquads && (rings ? b->filter_programs.d != nullptr : b->filter_program_horizon > 0);
    const unsigned length = static_cast<unsigned>(frames);
    if (biquads && !voice_scratch_fits(b, frames)) return false;
    bool launched = false;
    const char* kernel = "";
    if (rings && biquads) {
        kernel = "k_stream_filter_rows";
        launched = oalsfx_hip::launch_stream_filter(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->sweeps.d, b->filter_programs.d, b->programs.d,
                                                    b->streams.d, b->d_stream_taken, b->fir, b->n, b->lanes, length, b->channels, dst, b->d_voice_scratch, stream);
    } else if (rings) {
        kernel = "k_stream_rows";
        launched = oalsfx_hip::launch_stream(b->samplers.d, b->envelopes.d, b->resamplers.d, b->programs.d, b->streams.d, b->d_stream_taken, b->fir, b->n, b->lanes,
                                             length, b->channels, dst, stream);
    } else if (filter_queues && queues) {
        kernel = "k_filter_program_env_rows";
        launched = oalsfx_hip::launch_filter_program_env(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->sweeps.d, b->filter_programs.d, b->programs.d,
                                                         b->fir, b->n, b->lanes, length, b->channels, dst, b->d_voice_scratch, stream);
    } else if (filter_queues) {
        kernel = "k_filter_program_rows";
        launched = oalsfx_hip::launch_filter_program(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->sweeps.d, b->filter_programs.d, b->fir, b->n,
                                                     b->lanes, length, b->channels, dst, b->d_voice_scratch, stream);
    } else if (swept && queues) {
        kernel = "k_sweep_program_rows";
        launched = oalsfx_hip::launch_program_sweep(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->sweeps.d, b->programs.d, b->fir, b->n, b->lanes,
                                                    length, b->channels, dst, b->d_voice_scratch, stream);
    } else if (swept) {
        kernel = "k_sweep_rows";
        launched = oalsfx_hip::launch_sweep(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->sweeps.d, b->fir, b->n, b->lanes, length, b->channels,
                                            dst, b->d_voice_scratch, stream);
    } else if (queues && biquads) {
        kernel = "k_program_biquad_rows";
        launched = oalsfx_hip::launch_program_biquad(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->programs.d, b->fir, b->n, b->lanes, length,
                                                     b->channels, dst, b->d_voice_scratch, stream);
    } else if (queues) {
        kernel = "k_program_rows";
        launched = oalsfx_hip::launch_program(b->samplers.d, b->envelopes.d, b->resamplers.d, b->programs.d, b->fir, b->n, b->lanes, length, b->channels, dst, stream);
    } else if (biquads) {
        kernel = "k_biquad_rows";
        launched = oalsfx_hip::launch_biquad(b->samplers.d, b->envelopes.d, b->resamplers.d, b->filters.d, b->fir, b->n, b->lanes, length, b->channels, dst,
                                             b->d_voice_scratch, stream);
    } else if (b->lanes >= 2) {
        kernel = "k_mix_rows";
        launched = oalsfx_hip::launch_mix(b->samplers.d, b->envelopes.d, b->resamplers.d, b->fir, b->n, b->lanes, length, b->channels, dst, stream);
    } else if (b->resamplers_active > 0) {
        kernel = "k_fir_rows";
        launched = oalsfx_hip::launch_fir(b->samplers.d, b->envelopes.d, b->resamplers.d, b->fir, b->n, length, b->channels, dst, stream);
    } else if (b->envelopes_active > 0) {
        kernel = "k_voice_rows";
        launched = oalsfx_hip::launch_voice(b->samplers.d, b->envelopes.d, b->n, length, b->channels, dst, stream);
    } else {
        kernel = "k_sampler_rows";
        launched = oalsfx_hip::launch_sampler(b->samplers.d, b->n, length, b->channels, dst, stream);
    }
    if (!launched) return b->fail("No sampler kernel for this channel count.");
    b->last_render_kernel = kernel;
    // what the render has changed on the device: a filtered voice's histories, the queues (and the bound on what they still hold) ...
    if (biquads) b->filters.ahead = true;
    // ... the taken counts of the rings it walked
    if (rings) b->stream_taken_ahead = true;
    // ... a swept voice's sweep, and with the sweep that completes the filter's coefficients
    if (swept || filter_queues) {
        b->sweeps.ahead = true;
        b->sweep_horizon = std::max<long long>(0, b->sweep_horizon - frames);
    }
    // ... a programmed filter's queue
    if (filter_queues) b->filter_programs.ahead = true;
    b->filter_program_horizon = std::max<long long>(0, b->filter_program_horizon - frames);
    if (queues) {
        b->programs.ahead = true;
        b->program_horizon = std::max<long long>(0, b->program_horizon - frames);
    }
    // ... the envelopes (k_sampler_rows is launched only while none is ACTIVE; the others advance those that are) and the samplers
    if (b->envelopes_active > 0) {
        b->envelopes.ahead = true;
        if (b->envelopes_gliding > 0) b->steps_ahead = true;
    }
    b->samplers.ahead = true;
    b->sampler_pending = true;
    b->sampler_stream = stream;
    if (!b->hip_ok(hipGetLastError(), "sampler launch")) return false;
    return b->hip_ok(hipEventRecord(b->ev_sampler, stream), "hipEventRecord");
}

// The row of the record tables that holds the voice (lane, instances[k]).
int voice_row_at(const oalsfx_batch* b, int lane, const int* instances, int k) { return lane * b->n + instance_at(instances, k); }

// An array a record call reads or fills, and the call's text where it is missing.
struct CallArray { const void* data; const char* missing; };

// How the ten record calls of a lane begin.  What is refused, in this order: a null batch, a lane or an instance out of range, in a set
// call a poisoned batch (a get call still answers with what the host knows); then a call for no instance has nothing to do; then a
// missing array, in the order given, and in a set call an instance listed twice (`twice`: the call's text; null marks a get call).
// Returns what the call returns -- 0 with the text set, 1 with nothing to do -- or -1: go on.
int lane_call_begin(oalsfx_batch* b, int lane, const int* instances, int count, std::initializer_list<CallArray> arrays, const char* twice)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (lane < 0 || lane >= b->lanes) return b->fail("Lane out of range.") ? 1 : 0;
    if (!instances_ok(b, instances, count)) return 0;
    if (twice && b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    if (count == 0) return 1;
    for (const CallArray& a : arrays)
        if (!a.data) return b->fail(a.missing) ? 1 : 0;
    if (twice && !targets_distinct(b, instances, count, twice)) return 0;
    return -1;
}

constexpr const char* kErrNoSamplers = "No sampler records.";
constexpr const char* kErrNoEnvelopes = "No envelope records.";
constexpr const char* kErrNoLengths = "No envelope program lengths.";
constexpr const char* kErrNoResamplers = "No resampler indices.";
constexpr const char* kErrNoFilters = "No voice filter records.";
constexpr const char* kErrNoSweeps = "No filter sweep records.";
constexpr const char* kErrNoFilterLengths = "No filter program lengths.";
constexpr const char* kErrEnvelopeTwice = "An instance is listed twice as an envelope target.";
constexpr const char* kErrNoStreamLengths = "No stream lengths.";
constexpr uint32_t kEnvGlides = OALSFX_ENV_ACTIVE | OALSFX_ENV_GLIDE;

// ---- sampler streams (include/oalsfx_hip.h): what the samplers' and the envelopes' set calls need of them ----

// The rings' table and the taken counts, made with the first stream of two records or more: every ring empty and every count 0, on the
// host and on the device.
bool streams_made(oalsfx_batch* b)
{
    if (b->streams.d) return true;
    const size_t rows = static_cast<size_t>(b->n) * b->lanes;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return false;
    uint32_t* taken = nullptr;
    if (!b->hip_ok(hipMalloc(reinterpret_cast<void**>(&taken), rows * sizeof(uint32_t)), "hipMalloc(stream counts)")) return false;
    // (a set-up step: rings and counts are zero before anything else is queued, on whatever stream the next render goes)
    if (!b->hip_ok(hipMemsetAsync(taken, 0, rows * sizeof(uint32_t), b->stream), "hipMemsetAsync(stream counts)") || !records_create(b, b->streams, rows)) {
        hipFree(taken);
        return false;
    }
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) {
        hipFree(b->streams.d);
        b->streams.d = nullptr;
        hipFree(taken);
        return false;
    }
    b->d_stream_taken = taken;
    b->stream_taken.assign(rows, 0);
    b->stream_taken_ahead = false;
    b->streams_open = 0;
    return true;
}

// Whether, by what the host knows, the ring of the voice in row i may hold an entry.
bool stream_open(const oalsfx_batch* b, int i) { return b->streams.d && b->streams.table.host[i].queued != b->stream_taken[i]; }

// The taken counts as every render queued so far leaves them (waits for those), where a render has walked the rings since they were
// last read; a voice whose stream was set since has 0.  Every reading says anew which rings may hold an entry.
bool stream_taken_read_back(oalsfx_batch* b)
{
    if (!b->streams.d || !b->stream_taken_ahead) return true;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return false;
    if (b->sampler_pending && !b->hip_ok(hipEventSynchronize(b->ev_sampler), "hipEventSynchronize")) return false;
    if (!b->hip_ok(hipMemcpy(b->stream_taken.data(), b->d_stream_taken, b->stream_taken.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(stream counts)"))
        return false;
    b->sampler_pending = false;
    for (const int i : b->stream_reset_list) b->stream_taken[i] = 0;
    b->stream_taken_ahead = false;
    b->streams_open = 0;
    for (size_t i = 0; i < b->stream_taken.size(); ++i) b->streams_open += stream_open(b, static_cast<int>(i)) ? 1 : 0;
    return true;
}

// The ring of the voice in row i becomes `row`, its taken count as the host knows it `taken`.
void stream_ring_set(oalsfx_batch* b, int i, const oalsfx_hip::StreamRing& row, uint32_t taken)
{
    b->streams_open -= stream_open(b, i) ? 1 : 0;
    b->streams.table.set(i, row);
    b->stream_taken[i] = taken;
    b->streams_open += stream_open(b, i) ? 1 : 0;
    if (row.reset) b->stream_reset_list.push_back(i);
}

// The ring of the voice in row i emptied and its count zeroed by a set call: the row goes to the device only where a stream may have
// left something there.
void stream_emptied(oalsfx_batch* b, int i)
{
    if (!b->streams.d) return;
    // (nothing queued since the last set call: nothing can have been taken either, whatever the renders since)
    if (b->streams.table.host[i].queued == 0 && b->stream_taken[i] == 0) return;
    oalsfx_hip::StreamRing row{};
    row.reset = 1;
    stream_ring_set(b, i, row, 0);
}

// What the stream calls refuse in the records of one voice beyond sampler_ok: `queued` says from which record on they go into the ring.
bool stream_records_ok(oalsfx_batch* b, int i, const oalsfx_sampler* records, int length, int queued_from, AssetRange& known)
{
    for (int j = 0; j < length; ++j) {
        if (!sampler_ok(b, records[j], known)) return false;
        if (j >= queued_from && !(records[j].flags & OALSFX_SAMPLER_PLAYING)) return b->fail("A queued sampler is not playing.");
    }
    if (length > queued_from && (b->envelopes.table.host[i].flags & kEnvGlides) == kEnvGlides) return b->fail("The streaming voice's envelope glides.");
    return true;
}

// An envelope that glides, for the voice in row i: refused while its ring may hold an entry.
bool glide_streams_ok(oalsfx_batch* b, int i)
{
    if (!stream_open(b, i)) return true;
    if (!stream_taken_read_back(b)) return false;
    return stream_open(b, i) ? b->fail("The gliding voice streams.") : true;
}

// The call has begun (lane_call_begin): records[k * stride .. + lengths[k]) becomes the stream of the voice (lane, instances[k]).
// lengths == nullptr: every stream is one record, which is what a plain set is (oalsfx_batch_set_lane_samplers: stride 1).
int set_streams(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_sampler* records, size_t stride)
{
    const auto length = [lengths](int k) { return lengths ? lengths[k] : 1; };
    bool rings = false;
    for (int k = 0; k < count; ++k) {
        if (length(k) < 1 || length(k) > 1 + OALSFX_STREAM_QUEUE) return b->fail("Stream length out of range.") ? 1 : 0;
        rings = rings || length(k) >= 2;
    }
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0; // (asset_resident asks the runtime)
    AssetRange known;
    for (int k = 0; k < count; ++k)
        if (!stream_records_ok(b, voice_row_at(b, lane, instances, k), records + k * stride, length(k), 1, known)) return 0;
    for (int k = 0; k < count; ++k) {
        // an instance whose envelope glides keeps a step the glide's arithmetic has room for
        const char* message = nullptr;
        const oalsfx_envelope& e = b->envelopes.table.host[voice_row_at(b, lane, instances, k)];
        if ((e.flags & OALSFX_ENV_GLIDE) && !oalsfx_host_envelope_check(&e, records[k * stride].step, &message)) return b->fail(message) ? 1 : 0;
    }
    if (rings && !streams_made(b)) return 0;
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        const oalsfx_sampler* const stream = records + k * stride;
        b->samplers.table.set(i, stream[0]);
        if (length(k) == 1) {
            stream_emptied(b, i);
            continue;
        }
        oalsfx_hip::StreamRing row{};
        row.queued = static_cast<uint32_t>(length(k) - 1);
        row.reset = 1;
        for (int j = 1; j < length(k); ++j) row.entry[j - 1] = stream[j];
        stream_ring_set(b, i, row, 0);
    }
    return 1;
}

} // namespace

int oalsfx_batch_set_lane_samplers(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_sampler* samplers)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{samplers, kErrNoSamplers}}, "An instance is listed twice as a sampler target.");
    return begun >= 0 ? begun : set_streams(b, lane, instances, count, nullptr, samplers, 1);
}

int oalsfx_batch_set_samplers(oalsfx_batch* b, const int* instances, int count, const oalsfx_sampler* samplers)
{
    return oalsfx_batch_set_lane_samplers(b, 0, instances, count, samplers);
}

namespace {

// The samplers' records read back (records_read_back), and with them the steps the envelopes' glides have changed
bool samplers_read_back(oalsfx_batch* b)
{
    if (!records_read_back(b, b->samplers)) return false;
    b->steps_ahead = false;
    return true;
}

} // namespace

int oalsfx_batch_get_lane_samplers(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_sampler* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{out, kErrNoSamplers}}, nullptr);
    if (begun >= 0) return begun;
    if (!samplers_read_back(b)) return 0;
    for (int k = 0; k < count; ++k) out[k] = b->samplers.table.host[voice_row_at(b, lane, instances, k)];
    return 1;
}

int oalsfx_batch_get_samplers(oalsfx_batch* b, const int* instances, int count, oalsfx_sampler* out)
{
    return oalsfx_batch_get_lane_samplers(b, 0, instances, count, out);
}

// ---- sampler streams: the calls (include/oalsfx_hip.h) ----
int oalsfx_batch_set_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_sampler* records)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoStreamLengths}, {records, kErrNoSamplers}},
                                      "An instance is listed twice as a stream target.");
    return begun >= 0 ? begun : set_streams(b, lane, instances, count, lengths, records, 1 + OALSFX_STREAM_QUEUE);
}

int oalsfx_batch_set_streams(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_sampler* records)
{
    return oalsfx_batch_set_lane_streams(b, 0, instances, count, lengths, records);
}

int oalsfx_batch_append_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_sampler* records)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoStreamLengths}, {records, kErrNoSamplers}},
                                      "An instance is listed twice as a stream target.");
    if (begun >= 0) return begun;
    bool any = false;
    for (int k = 0; k < count; ++k) {
        if (lengths[k] < 0 || lengths[k] > OALSFX_STREAM_QUEUE) return b->fail("Stream length out of range.") ? 1 : 0;
        any = any || lengths[k] > 0;
    }
    if (!any) return 1;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0; // (asset_resident asks the runtime)
    AssetRange known;
    for (int k = 0; k < count; ++k)
        if (!stream_records_ok(b, voice_row_at(b, lane, instances, k), records + static_cast<size_t>(k) * OALSFX_STREAM_QUEUE, lengths[k], 0, known)) return 0;
    if (!streams_made(b)) return 0;
    // room by the counts the host read last; where that is too little, by the device's
    const auto short_of_room = [&]() {
        for (int k = 0; k < count; ++k) {
            const int i = voice_row_at(b, lane, instances, k);
            const uint32_t waiting = b->streams.table.host[i].queued - b->stream_taken[i];
            if (static_cast<uint32_t>(lengths[k]) > OALSFX_STREAM_QUEUE - waiting) return true;
        }
        return false;
    };
    if (short_of_room()) {
        if (!stream_taken_read_back(b)) return 0;
        if (short_of_room()) return b->fail("The stream queue is full.") ? 1 : 0;
    }
    for (int k = 0; k < count; ++k) {
        if (lengths[k] == 0) continue;
        const int i = voice_row_at(b, lane, instances, k);
        oalsfx_hip::StreamRing row = b->streams.table.host[i];
        for (int j = 0; j < lengths[k]; ++j) row.entry[(row.queued + static_cast<uint32_t>(j)) % OALSFX_STREAM_QUEUE] = records[static_cast<size_t>(k) * OALSFX_STREAM_QUEUE + j];
        row.queued += static_cast<uint32_t>(lengths[k]);
        stream_ring_set(b, i, row, b->stream_taken[i]);
    }
    return 1;
}

int oalsfx_batch_append_streams(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_sampler* records)
{
    return oalsfx_batch_append_lane_streams(b, 0, instances, count, lengths, records);
}

int oalsfx_batch_get_lane_streams(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_sampler* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoStreamLengths}, {out, kErrNoSamplers}}, nullptr);
    if (begun >= 0) return begun;
    if (!samplers_read_back(b) || !stream_taken_read_back(b)) return 0;
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        oalsfx_sampler* const stream = out + static_cast<size_t>(k) * (1 + OALSFX_STREAM_QUEUE);
        stream[0] = b->samplers.table.host[i];
        lengths[k] = 1;
        if (!b->streams.d) continue;
        const oalsfx_hip::StreamRing& row = b->streams.table.host[i];
        const uint32_t taken = b->stream_taken[i], waiting = row.queued - taken;
        for (uint32_t j = 0; j < waiting; ++j) stream[1 + j] = row.entry[(taken + j) % OALSFX_STREAM_QUEUE];
        lengths[k] = 1 + static_cast<int>(waiting);
    }
    return 1;
}

int oalsfx_batch_get_streams(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_sampler* out)
{
    return oalsfx_batch_get_lane_streams(b, 0, instances, count, lengths, out);
}

int oalsfx_batch_get_lane_stream_state(oalsfx_batch* b, int lane, const int* instances, int count, uint32_t* taken, uint32_t* queued)
{
    const int begun = lane_call_begin(b, lane, instances, count, {}, nullptr);
    if (begun >= 0) return begun;
    if (!stream_taken_read_back(b)) return 0;
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        const uint32_t t = b->streams.d ? b->stream_taken[i] : 0U;
        if (taken) taken[k] = t;
        if (queued) queued[k] = b->streams.d ? b->streams.table.host[i].queued - t : 0U;
    }
    return 1;
}

int oalsfx_batch_get_stream_state(oalsfx_batch* b, const int* instances, int count, uint32_t* taken, uint32_t* queued)
{
    return oalsfx_batch_get_lane_stream_state(b, 0, instances, count, taken, queued);
}

// ---- voice envelopes and envelope programs (include/oalsfx_hip.h) ----
namespace {

// The queues' table, made with the first program of two segments or more: every row empty, on the host and on the device.
bool programs_made(oalsfx_batch* b)
{
    if (b->programs.d) return true;
    const size_t rows = static_cast<size_t>(b->n) * b->lanes;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !records_create(b, b->programs, rows)) return false;
    // (a set-up step: the rows are zero before anything else is queued, on whatever stream the next render goes)
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) {
        hipFree(b->programs.d);
        b->programs.d = nullptr;
        return false;
    }
    b->program_set.assign(rows, 0);
    return true;
}

// The voices (lane, instances[k]) given a program each: lengths[k] records at segments + k * stride, the first the voice's envelope from
// the next render on, the rest its queue.  lengths == nullptr: every program is one record, which is what a plain set is
// (oalsfx_batch_set_lane_envelopes: stride 1).  The call has begun (lane_call_begin).
int set_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_envelope* segments, size_t stride)
{
    const auto length = [lengths](int k) { return lengths ? lengths[k] : 1; };
    bool glides = false, queues = false;
    for (int k = 0; k < count; ++k) {
        if (length(k) < 1 || length(k) > OALSFX_ENV_PROGRAM_MAX) return b->fail("Envelope program length out of range.") ? 1 : 0;
        queues = queues || length(k) >= 2;
        glides = glides || (length(k) == 1 && (segments[k * stride].flags & OALSFX_ENV_GLIDE) != 0);
    }
    // (only a program of one may glide: it is checked against its sampler's step, which a glide before it may have changed on the device)
    if (glides && b->steps_ahead && !samplers_read_back(b)) return 0;
    for (int k = 0; k < count; ++k) {
        const oalsfx_envelope* const program = segments + k * stride;
        if (length(k) == 1 && (program[0].flags & kEnvGlides) == kEnvGlides && !glide_streams_ok(b, voice_row_at(b, lane, instances, k))) return 0;
        const uint32_t step = b->samplers.table.host[voice_row_at(b, lane, instances, k)].step;
        for (int j = 0; j < length(k); ++j) {
            if (length(k) >= 2 && (program[j].flags & OALSFX_ENV_GLIDE)) return b->fail("A program's segment glides.") ? 1 : 0;
            const char* message = nullptr;
            if (!oalsfx_host_envelope_check(&program[j], step, &message)) return b->fail(message) ? 1 : 0;
            if (length(k) >= 2 && !(program[j].flags & OALSFX_ENV_ACTIVE)) return b->fail("A program's segment is not active.") ? 1 : 0;
        }
    }
    if (queues && !programs_made(b)) return 0;
    const auto counted = [](const oalsfx_envelope& e, uint32_t bits) { return (e.flags & bits) == bits ? 1 : 0; };
    for (int k = 0; k < count; ++k) {
        const oalsfx_envelope* const program = segments + k * stride;
        const int i = voice_row_at(b, lane, instances, k);
        b->envelopes_active += counted(program[0], OALSFX_ENV_ACTIVE) - counted(b->envelopes.table.host[i], OALSFX_ENV_ACTIVE);
        b->envelopes_gliding += counted(program[0], OALSFX_ENV_ACTIVE | OALSFX_ENV_GLIDE) - counted(b->envelopes.table.host[i], OALSFX_ENV_ACTIVE | OALSFX_ENV_GLIDE);
        b->envelopes.table.set(i, program[0]);
        if (length(k) == 1) {
            // the voice's queue emptied: the row goes to the device only where a program may have left something in it
            if (b->programs.d && b->program_set[i]) {
                b->program_set[i] = 0;
                b->programs.table.set(i, oalsfx_hip::EnvProgram{});
            }
            continue;
        }
        oalsfx_hip::EnvProgram row{};
        row.count = static_cast<uint32_t>(length(k) - 1);
        // the frames until the last segment is the current one: every queue is empty once that many have been rendered
        long long left = 1;
        for (int j = 0; j + 1 < length(k); ++j) {
            row.queue[j] = program[j + 1];
            left += static_cast<long long>(program[j].delay) + (program[j].ramp_frames - program[j].ramp_done);
        }
        b->program_set[i] = 1;
        b->programs.table.set(i, row);
        b->program_horizon = std::max(b->program_horizon, left);
    }
    return 1;
}

} // namespace

int oalsfx_batch_set_lane_envelopes(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_envelope* envelopes)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{envelopes, kErrNoEnvelopes}}, kErrEnvelopeTwice);
    return begun >= 0 ? begun : set_programs(b, lane, instances, count, nullptr, envelopes, 1);
}

int oalsfx_batch_set_envelopes(oalsfx_batch* b, const int* instances, int count, const oalsfx_envelope* envelopes)
{
    return oalsfx_batch_set_lane_envelopes(b, 0, instances, count, envelopes);
}

int oalsfx_batch_get_lane_envelopes(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_envelope* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{out, kErrNoEnvelopes}}, nullptr);
    if (begun >= 0) return begun;
    if (!records_read_back(b, b->envelopes)) return 0;
    for (int k = 0; k < count; ++k) out[k] = b->envelopes.table.host[voice_row_at(b, lane, instances, k)];
    return 1;
}

int oalsfx_batch_get_envelopes(oalsfx_batch* b, const int* instances, int count, oalsfx_envelope* out)
{
    return oalsfx_batch_get_lane_envelopes(b, 0, instances, count, out);
}

int oalsfx_batch_set_lane_env_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_envelope* segments)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoLengths}, {segments, kErrNoEnvelopes}}, kErrEnvelopeTwice);
    return begun >= 0 ? begun : set_programs(b, lane, instances, count, lengths, segments, OALSFX_ENV_PROGRAM_MAX);
}

int oalsfx_batch_set_env_programs(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_envelope* segments)
{
    return oalsfx_batch_set_lane_env_programs(b, 0, instances, count, lengths, segments);
}

int oalsfx_batch_get_lane_env_programs(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_envelope* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoLengths}, {out, kErrNoEnvelopes}}, nullptr);
    if (begun >= 0) return begun;
    if (!records_read_back(b, b->envelopes)) return 0;
    if (b->programs.d && !records_read_back(b, b->programs)) return 0;
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        oalsfx_envelope* const program = out + static_cast<size_t>(k) * OALSFX_ENV_PROGRAM_MAX;
        program[0] = b->envelopes.table.host[i];
        lengths[k] = 1;
        if (!b->programs.d) continue;
        const oalsfx_hip::EnvProgram& row = b->programs.table.host[i];
        for (uint32_t j = 0; j < row.count; ++j) program[1 + j] = row.queue[row.head + j];
        lengths[k] = 1 + static_cast<int>(row.count);
    }
    return 1;
}

int oalsfx_batch_get_env_programs(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_envelope* out)
{
    return oalsfx_batch_get_lane_env_programs(b, 0, instances, count, lengths, out);
}

// ---- resamplers (include/oalsfx_hip.h) ----
int oalsfx_batch_set_fir_table(oalsfx_batch* b, int table, int taps, int phase_bits, const float* coef_host)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    if (table < 0 || table >= OALSFX_FIR_TABLES) return b->fail("FIR table index out of range.") ? 1 : 0;
    const bool clear = taps == 0 && !coef_host;
    if (!clear) {
        const char* message = nullptr;
        if (!oalsfx_host_fir_check(taps, phase_bits, coef_host, &message)) return b->fail(message) ? 1 : 0;
    }
    const int shift = OALSFX_SAMPLER_FRAC_BITS - phase_bits;
    const bool same_shape = !clear && b->fir.taps[table] == taps && b->fir.shift[table] == shift;
    if (!same_shape && b->fir_named[table] > 0) return b->fail("The FIR table is still named by an instance.") ? 1 : 0;
    if (clear && b->fir.taps[table] == 0) return 1;
    // a set-up call: behind every render queued so far, which may still read the table
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0;
    if (b->sampler_pending && !b->hip_ok(hipEventSynchronize(b->ev_sampler), "hipEventSynchronize")) return 0;
    if (!same_shape) {
        hipFree(const_cast<float*>(b->fir.coef[table]));
        b->fir.coef[table] = nullptr;
        b->fir.taps[table] = 0;
        b->fir.shift[table] = 0;
        if (clear) return 1;
    }
    const size_t bytes = (size_t{1} << phase_bits) * static_cast<size_t>(taps) * sizeof(float);
    float* d_coef = const_cast<float*>(b->fir.coef[table]);
    if (!d_coef && !b->hip_ok(hipMalloc(reinterpret_cast<void**>(&d_coef), bytes), "hipMalloc(FIR table)")) return 0;
    // (synchronous: the caller's array is free when the call returns, and the next render finds the table in place)
    if (!b->hip_ok(hipMemcpy(d_coef, coef_host, bytes, hipMemcpyHostToDevice), "hipMemcpy(FIR table)")) {
        if (!same_shape) hipFree(d_coef);
        return 0;
    }
    b->fir.coef[table] = d_coef;
    b->fir.taps[table] = taps;
    b->fir.shift[table] = shift;
    return 1;
}

int oalsfx_batch_get_fir_table(const oalsfx_batch* b, int table, int* taps, int* phase_bits)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (table < 0 || table >= OALSFX_FIR_TABLES) return const_cast<oalsfx_batch*>(b)->fail("FIR table index out of range.") ? 1 : 0;
    const int t = b->fir.taps[table];
    if (taps) *taps = t;
    if (phase_bits) *phase_bits = t ? OALSFX_SAMPLER_FRAC_BITS - b->fir.shift[table] : 0;
    return 1;
}

int oalsfx_batch_set_lane_resamplers(oalsfx_batch* b, int lane, const int* instances, int count, const int* tables)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{tables, kErrNoResamplers}}, "An instance is listed twice as a resampler target.");
    if (begun >= 0) return begun;
    for (int k = 0; k < count; ++k) {
        if (tables[k] < OALSFX_RESAMPLER_NONE || tables[k] >= OALSFX_FIR_TABLES) return b->fail("Unknown resampler.") ? 1 : 0;
        if (tables[k] >= 0 && b->fir.taps[tables[k]] == 0) return b->fail("The resampler names a table that has not been set.") ? 1 : 0;
    }
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        const int before = b->resamplers.table.host[i];
        if (before == tables[k]) continue;
        if (before >= 0) { --b->fir_named[before]; --b->resamplers_active; }
        if (tables[k] >= 0) { ++b->fir_named[tables[k]]; ++b->resamplers_active; }
        b->resamplers.table.set(i, tables[k]);
    }
    return 1;
}

int oalsfx_batch_set_resamplers(oalsfx_batch* b, const int* instances, int count, const int* tables)
{
    return oalsfx_batch_set_lane_resamplers(b, 0, instances, count, tables);
}

int oalsfx_batch_get_lane_resamplers(oalsfx_batch* b, int lane, const int* instances, int count, int* tables)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{tables, kErrNoResamplers}}, nullptr);
    if (begun >= 0) return begun;
    for (int k = 0; k < count; ++k) tables[k] = b->resamplers.table.host[voice_row_at(b, lane, instances, k)];
    return 1;
}

int oalsfx_batch_get_resamplers(oalsfx_batch* b, const int* instances, int count, int* tables)
{
    return oalsfx_batch_get_lane_resamplers(b, 0, instances, count, tables);
}

// ---- voice filters (include/oalsfx_hip.h) ----
namespace {

// The queue of the voice in row i emptied by a set call: the row goes to the device only where a filter program may have left something
// in it.
void filter_queue_emptied(oalsfx_batch* b, int i)
{
    if (!b->filter_programs.d || !b->filter_program_set[i]) return;
    b->filter_program_set[i] = 0;
    b->filter_programs.table.set(i, oalsfx_hip::FilterProgram{});
}

// The filters' rows as every render queued so far leaves them (waits for those): a row that is not set takes the device's; a row set
// since without LOAD keeps the flags and coefficients as set and takes the device's histories, which that set call did not touch.
bool filters_read_back(oalsfx_batch* b)
{
    auto& table = b->filters.table;
    return records_read_back(b, b->filters, [&table](const std::vector<oalsfx_voice_filter>& now) {
        for (size_t i = 0; i < now.size(); ++i) {
            if (!table.is_set(static_cast<int>(i))) {
                table.host[i] = now[i];
            } else if (!(table.host[i].flags & OALSFX_VF_LOAD)) {
                std::memcpy(table.host[i].x, now[i].x, sizeof(now[i].x));
                std::memcpy(table.host[i].y, now[i].y, sizeof(now[i].y));
            }
        }
    });
}

} // namespace

int oalsfx_batch_set_lane_filters(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_voice_filter* filters)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{filters, kErrNoFilters}}, "An instance is listed twice as a voice filter target.");
    if (begun >= 0) return begun;
    for (int k = 0; k < count; ++k) {
        const char* message = nullptr;
        if (!oalsfx_host_voice_filter_check(&filters[k], &message)) return b->fail(message) ? 1 : 0;
    }
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        const oalsfx_voice_filter& before = b->filters.table.host[i];
        oalsfx_voice_filter row = filters[k];
        if (!(row.flags & OALSFX_VF_LOAD)) {
            // the histories stay: the device's, or those of a LOAD that is still pending, which stays pending
            std::memcpy(row.x, before.x, sizeof(row.x));
            std::memcpy(row.y, before.y, sizeof(row.y));
            if (b->filters.table.is_set(i)) row.flags |= before.flags & OALSFX_VF_LOAD;
        }
        b->filters_active += static_cast<int>(row.flags & OALSFX_VF_ACTIVE) - static_cast<int>(before.flags & OALSFX_VF_ACTIVE);
        b->filters.table.set(i, row);
        // a plain set is a sweep of none: the row goes to the device only where a sweep may have left something in it
        if (b->sweep_set[i]) {
            b->sweep_set[i] = 0;
            b->sweeps.table.set(i, oalsfx_filter_sweep{});
        }
        filter_queue_emptied(b, i);
    }
    return 1;
}

int oalsfx_batch_set_filters(oalsfx_batch* b, const int* instances, int count, const oalsfx_voice_filter* filters)
{
    return oalsfx_batch_set_lane_filters(b, 0, instances, count, filters);
}

int oalsfx_batch_get_lane_filters(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_voice_filter* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{out, kErrNoFilters}}, nullptr);
    if (begun >= 0) return begun;
    if (!filters_read_back(b)) return 0;
    for (int k = 0; k < count; ++k) {
        out[k] = b->filters.table.host[voice_row_at(b, lane, instances, k)];
        out[k].flags &= ~static_cast<uint32_t>(OALSFX_VF_LOAD); // (consumed by the upload: never shown)
    }
    return 1;
}

int oalsfx_batch_get_filters(oalsfx_batch* b, const int* instances, int count, oalsfx_voice_filter* out)
{
    return oalsfx_batch_get_lane_filters(b, 0, instances, count, out);
}

// ---- voice filter sweeps and filter programs (include/oalsfx_hip.h) ----
namespace {

// The queues' table, made with the first filter program of two segments or more: every row empty, on the host and on the device.
bool filter_programs_made(oalsfx_batch* b)
{
    if (b->filter_programs.d) return true;
    const size_t rows = static_cast<size_t>(b->n) * b->lanes;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !records_create(b, b->filter_programs, rows)) return false;
    // (a set-up step: the rows are zero before anything else is queued, on whatever stream the next render goes)
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) {
        hipFree(b->filter_programs.d);
        b->filter_programs.d = nullptr;
        return false;
    }
    b->filter_program_set.assign(rows, 0);
    return true;
}

// The voices (lane, instances[k]) given a filter program each: lengths[k] records at segments + k * stride, the first the voice's sweep
// from the next render on, the rest its queue.  lengths == nullptr: every program is one record, which is what a plain set is
// (oalsfx_batch_set_lane_sweeps: stride 1).  The call has begun (lane_call_begin).
int set_filter_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_filter_sweep* segments, size_t stride)
{
    const auto length = [lengths](int k) { return lengths ? lengths[k] : 1; };
    bool queues = false;
    for (int k = 0; k < count; ++k) {
        if (length(k) < 1 || length(k) > OALSFX_FILTER_PROGRAM_MAX) return b->fail("Filter program length out of range.") ? 1 : 0;
        queues = queues || length(k) >= 2;
    }
    for (int k = 0; k < count; ++k) {
        const oalsfx_filter_sweep* const program = segments + k * stride;
        // (the filters' flags are exact on the host: only the caller sets or clears ACTIVE)
        const bool filtered = (b->filters.table.host[voice_row_at(b, lane, instances, k)].flags & OALSFX_VF_ACTIVE) != 0;
        for (int j = 0; j < length(k); ++j) {
            const char* message = nullptr;
            if (!oalsfx_host_filter_sweep_check(&program[j], &message)) return b->fail(message) ? 1 : 0;
            if (length(k) >= 2 && !(program[j].flags & OALSFX_SWEEP_ACTIVE)) return b->fail("A filter program's segment is not active.") ? 1 : 0;
            if (j >= 1 && program[j].done != 0) return b->fail("A queued filter sweep has already started.") ? 1 : 0;
            if ((program[j].flags & OALSFX_SWEEP_ACTIVE) && !filtered) return b->fail("The swept voice's filter is not active.") ? 1 : 0;
        }
    }
    if (queues && !filter_programs_made(b)) return 0;
    for (int k = 0; k < count; ++k) {
        const oalsfx_filter_sweep* const program = segments + k * stride;
        const int i = voice_row_at(b, lane, instances, k);
        if (length(k) == 1) {
            filter_queue_emptied(b, i);
            // (an all-zero record on a row that is all zero on the device changes nothing there)
            static const oalsfx_filter_sweep none{};
            const bool something = std::memcmp(&program[0], &none, sizeof(none)) != 0;
            if (!something && !b->sweep_set[i]) continue;
            b->sweep_set[i] = something ? 1 : 0;
            b->sweeps.table.set(i, program[0]);
            if (program[0].flags & OALSFX_SWEEP_ACTIVE) b->sweep_horizon = std::max<long long>(b->sweep_horizon, static_cast<long long>(program[0].frames) - program[0].done);
            continue;
        }
        b->sweep_set[i] = 1;
        b->sweeps.table.set(i, program[0]);
        oalsfx_hip::FilterProgram row{};
        row.count = static_cast<uint32_t>(length(k) - 1);
        // the frames until the last segment is the current one -- every queue is empty once that many have been rendered -- and the frames
        // of the whole program, behind which no sweep is under way
        long long in_front = 0;
        for (int j = 0; j + 1 < length(k); ++j) {
            row.queue[j] = program[j + 1];
            in_front += static_cast<long long>(program[j].frames) - program[j].done;
        }
        const oalsfx_filter_sweep& last = program[length(k) - 1];
        b->filter_program_set[i] = 1;
        b->filter_programs.table.set(i, row);
        b->filter_program_horizon = std::max(b->filter_program_horizon, 1 + in_front);
        b->sweep_horizon = std::max(b->sweep_horizon, in_front + (static_cast<long long>(last.frames) - last.done));
    }
    return 1;
}

} // namespace

int oalsfx_batch_set_lane_sweeps(oalsfx_batch* b, int lane, const int* instances, int count, const oalsfx_filter_sweep* sweeps)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{sweeps, kErrNoSweeps}}, "An instance is listed twice as a filter sweep target.");
    return begun >= 0 ? begun : set_filter_programs(b, lane, instances, count, nullptr, sweeps, 1);
}

int oalsfx_batch_set_sweeps(oalsfx_batch* b, const int* instances, int count, const oalsfx_filter_sweep* sweeps)
{
    return oalsfx_batch_set_lane_sweeps(b, 0, instances, count, sweeps);
}

int oalsfx_batch_get_lane_sweeps(oalsfx_batch* b, int lane, const int* instances, int count, oalsfx_filter_sweep* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{out, kErrNoSweeps}}, nullptr);
    if (begun >= 0) return begun;
    if (!records_read_back(b, b->sweeps)) return 0;
    for (int k = 0; k < count; ++k) out[k] = b->sweeps.table.host[voice_row_at(b, lane, instances, k)];
    return 1;
}

int oalsfx_batch_get_sweeps(oalsfx_batch* b, const int* instances, int count, oalsfx_filter_sweep* out)
{
    return oalsfx_batch_get_lane_sweeps(b, 0, instances, count, out);
}

int oalsfx_batch_set_lane_filter_programs(oalsfx_batch* b, int lane, const int* instances, int count, const int* lengths, const oalsfx_filter_sweep* segments)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoFilterLengths}, {segments, kErrNoSweeps}},
                                      "An instance is listed twice as a filter program target.");
    return begun >= 0 ? begun : set_filter_programs(b, lane, instances, count, lengths, segments, OALSFX_FILTER_PROGRAM_MAX);
}

int oalsfx_batch_set_filter_programs(oalsfx_batch* b, const int* instances, int count, const int* lengths, const oalsfx_filter_sweep* segments)
{
    return oalsfx_batch_set_lane_filter_programs(b, 0, instances, count, lengths, segments);
}

int oalsfx_batch_get_lane_filter_programs(oalsfx_batch* b, int lane, const int* instances, int count, int* lengths, oalsfx_filter_sweep* out)
{
    const int begun = lane_call_begin(b, lane, instances, count, {{lengths, kErrNoFilterLengths}, {out, kErrNoSweeps}}, nullptr);
    if (begun >= 0) return begun;
    if (!records_read_back(b, b->sweeps)) return 0;
    if (b->filter_programs.d && !records_read_back(b, b->filter_programs)) return 0;
    for (int k = 0; k < count; ++k) {
        const int i = voice_row_at(b, lane, instances, k);
        oalsfx_filter_sweep* const program = out + static_cast<size_t>(k) * OALSFX_FILTER_PROGRAM_MAX;
        program[0] = b->sweeps.table.host[i];
        lengths[k] = 1;
        if (!b->filter_programs.d) continue;
        const oalsfx_hip::FilterProgram& row = b->filter_programs.table.host[i];
        for (uint32_t j = 0; j < row.count; ++j) program[1 + j] = row.queue[row.head + j];
        lengths[k] = 1 + static_cast<int>(row.count);
    }
    return 1;
}

int oalsfx_batch_get_filter_programs(oalsfx_batch* b, const int* instances, int count, int* lengths, oalsfx_filter_sweep* out)
{
    return oalsfx_batch_get_lane_filter_programs(b, 0, instances, count, lengths, out);
}

// ---- polyphony (include/oalsfx_hip.h) ----
int oalsfx_batch_set_polyphony(oalsfx_batch* b, int lanes)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (b->poisoned) return b->fail(b->fault_text) ? 1 : 0;
    if (lanes < 1 || lanes > OALSFX_MAX_POLYPHONY) return b->fail("Polyphony out of range.") ? 1 : 0;
    if (lanes == b->lanes) return 1;
    // a set-up call: behind every render queued so far, with the records as those leave them
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice")) return 0;
    if (!samplers_read_back(b) || !records_read_back(b, b->envelopes) || !filters_read_back(b) || !records_read_back(b, b->sweeps)) return 0;
    if (b->programs.d && !records_read_back(b, b->programs)) return 0;
    if (b->filter_programs.d && !records_read_back(b, b->filter_programs)) return 0;
    if (!stream_taken_read_back(b)) return 0;
    if (b->sampler_pending && !b->hip_ok(hipEventSynchronize(b->ev_sampler), "hipEventSynchronize")) return 0;
    b->sampler_pending = false;
    const size_t rows = static_cast<size_t>(b->n) * lanes;
    for (size_t row = rows; b->streams.d && row < b->stream_taken.size(); ++row)
        if (stream_open(b, static_cast<int>(row))) return b->fail("A lane that would be dropped is still in use.") ? 1 : 0;
    for (size_t row = rows; row < b->samplers.table.host.size(); ++row)
        if ((b->samplers.table.host[row].flags & OALSFX_SAMPLER_PLAYING) || (b->envelopes.table.host[row].flags & OALSFX_ENV_ACTIVE) ||
            b->resamplers.table.host[row] != OALSFX_RESAMPLER_NONE || (b->filters.table.host[row].flags & OALSFX_VF_ACTIVE))
            return b->fail("A lane that would be dropped is still in use.") ? 1 : 0;
    // (the host's rows are the current ones, those set since the last render included: the whole tables go to the device here, made
    // beside the ones in use -- the queues' first, where there is one: a dropped lane's queue is empty or never looked at again)
    const auto resized = [b, rows](auto& r) { return r.resized.d || records_resized(b, r, rows); };
    // (the rings' rows without `reset`, and the counts as the host knows them, which are 0 where a set call's upload was still to come:
    // the copy of both whole tables carries that upload out)
    uint32_t* taken_new = nullptr;
    std::vector<uint32_t> taken_host;
    const auto streams_resized = [&]() {
        if (!b->streams.d) return true;
        auto& r = b->streams;
        r.resized.host = r.table.host;
        r.resized.host.resize(rows, r.init);
        for (oalsfx_hip::StreamRing& ring : r.resized.host) ring.reset = 0;
        taken_host = b->stream_taken;
        taken_host.resize(rows, 0);
        return b->hip_ok(hipMalloc(reinterpret_cast<void**>(&r.resized.d), rows * sizeof(oalsfx_hip::StreamRing)), "hipMalloc", r.name) &&
               b->hip_ok(hipMemcpy(r.resized.d, r.resized.host.data(), rows * sizeof(oalsfx_hip::StreamRing), hipMemcpyHostToDevice), "hipMemcpy", r.name) &&
               b->hip_ok(hipMalloc(reinterpret_cast<void**>(&taken_new), rows * sizeof(uint32_t)), "hipMalloc(stream counts)") &&
               b->hip_ok(hipMemcpy(taken_new, taken_host.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(stream counts)");
    };
    if ((b->programs.d && !resized(b->programs)) || (b->filter_programs.d && !resized(b->filter_programs)) || !streams_resized() || !each_voice_table(b, resized)) {
        each_voice_table(b, [](auto& r) { hipFree(r.resized.d); r.resized = {}; return true; });
        hipFree(b->streams.resized.d);
        b->streams.resized = {};
        hipFree(taken_new);
        return 0;
    }
    if (b->streams.d) {
        records_replace(b->streams);
        hipFree(b->d_stream_taken);
        b->d_stream_taken = taken_new;
        b->stream_taken = std::move(taken_host);
        b->stream_reset_list.clear();
    }
    // (a pending LOAD has been carried out by the copy of the whole table -- the host's histories were the ones to load -- and is cleared
    // only here, where nothing can fail any more; the device's copy never shows the bit)
    for (oalsfx_voice_filter& f : b->filters.resized.host) f.flags &= ~static_cast<uint32_t>(OALSFX_VF_LOAD);
    each_voice_table(b, [](auto& r) { records_replace(r); return true; });
    if (b->programs.d) b->program_set.resize(rows, 0);
    if (b->filter_programs.d) b->filter_program_set.resize(rows, 0);
    b->sweep_set.resize(rows, 0);
    b->lanes = lanes;
    return 1;
}

int oalsfx_batch_get_polyphony(const oalsfx_batch* b)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    return b->lanes;
}

int oalsfx_batch_sample_device(oalsfx_batch* b, int frames, float* dst_dev, void* hip_stream)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (!sampler_args_ok(b, frames)) return 0;
    if (frames == 0) return 1;
    if (!dst_dev) return b->fail(kErrNoDst) ? 1 : 0;
    if (reinterpret_cast<uintptr_t>(dst_dev) % sizeof(float) != 0) return b->fail("The sampler destination is not 4-byte aligned.") ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    return sampler_queue(b, frames, dst_dev, hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream) ? 1 : 0;
}

int oalsfx_batch_play_downmix_meter(oalsfx_batch* b, int frames, int n_buses, float* dst_bus_host, float threshold, int flags,
                                    oalsfx_meter* voice_meters_host, oalsfx_meter* bus_meters_host)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    return downmix_meter_call(b, frames, nullptr, true, n_buses, dst_bus_host, threshold, flags, voice_meters_host, bus_meters_host);
}

long long oalsfx_debug_sampler_uploads(const oalsfx_batch* b) { return b ? b->samplers.uploads : 0; }
long long oalsfx_debug_envelope_uploads(const oalsfx_batch* b) { return b ? b->envelopes.uploads : 0; }
long long oalsfx_debug_resampler_uploads(const oalsfx_batch* b) { return b ? b->resamplers.uploads : 0; }
long long oalsfx_debug_filter_uploads(const oalsfx_batch* b) { return b ? b->filters.uploads : 0; }
long long oalsfx_debug_program_uploads(const oalsfx_batch* b) { return b ? b->programs.uploads : 0; }
long long oalsfx_debug_sweep_uploads(const oalsfx_batch* b) { return b ? b->sweeps.uploads : 0; }
long long oalsfx_debug_filter_program_uploads(const oalsfx_batch* b) { return b ? b->filter_programs.uploads : 0; }
const char* oalsfx_debug_last_render_kernel(const oalsfx_batch* b) { return b ? b->last_render_kernel : ""; }

int oalsfx_batch_fill_synthetic(oalsfx_batch* b, int frames, unsigned buffer_index, float* dst_dev, void* hip_stream)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    oalsfx_hip::launch_fill_synthetic(dst_dev, b->n, frames * b->channels, buffer_index, hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream);
    return b->hip_ok(hipGetLastError(), "fill_synthetic") ? 1 : 0;
}

int oalsfx_batch_kernel_timing(oalsfx_batch* b, int enable)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    for (auto& t : b->timed) { b->event_pool.push_back(t.start); b->event_pool.push_back(t.stop); }
    b->timed.clear();
    b->timing_every = enable > 0 ? enable : 0;
    b->timing = false;
    b->mix_calls = 0;
    while (b->timing_every && b->event_pool.size() < 2048) {
        hipEvent_t e = nullptr;
        if (!b->hip_ok(hipEventCreate(&e), "hipEventCreate")) return 0;
        b->event_pool.push_back(e);
    }
    return 1;
}

int oalsfx_batch_kernel_timing_read(oalsfx_batch* b, int effect_type, int* launches, double* total_ms)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    int n = 0;
    double ms = 0.0;
    const int key = timed_key(effect_type);
    for (auto& t : b->timed) {
        if (t.type != key) continue;
        if (!b->hip_ok(hipEventSynchronize(t.stop), "hipEventSynchronize")) return 0;
        float e = 0.0F;
        if (!b->hip_ok(hipEventElapsedTime(&e, t.start, t.stop), "hipEventElapsedTime")) return 0;
        ms += e;
        ++n;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    return 1;
}

int oalsfx_batch_kernel_timing_samples(oalsfx_batch* b, int effect_type, double* out_us, int max_samples)
{
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return -1;
    const int key = timed_key(effect_type);
    int n = 0;
    for (auto& t : b->timed) {
        if (t.type != key) continue;
        if (out_us && n < max_samples) {
            if (!b->hip_ok(hipEventSynchronize(t.stop), "hipEventSynchronize")) return -1;
            float e = 0.0F;
            if (!b->hip_ok(hipEventElapsedTime(&e, t.start, t.stop), "hipEventElapsedTime")) return -1;
            out_us[n] = e * 1e3;
        }
        ++n;
    }
    return n;
}

int oalsfx_batch_plan(oalsfx_batch* b, int slot, int counts[4])
{
    if (slot < 0 || slot >= b->slots) return b->fail(kErrSlot) ? 1 : 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    poll_exact(b);
    if (!sync_params(b, nullptr)) return 0;
    int light = 0;
    for (int t = 0; t < OALSFX_REVERB; ++t) light += b->list_count[slot][t];
    counts[0] = light;
    counts[1] = b->fast_count[slot];
    counts[2] = b->slow_count[slot];
    counts[3] = b->general_count[slot];
    return 1;
}

const char* oalsfx_batch_last_reverb_kernel(const oalsfx_batch* b) { return b->last_steady_kernel; }

long long oalsfx_batch_chained_calls(const oalsfx_batch* b) { return b->chained_calls; }

int oalsfx_batch_multi_counts(const oalsfx_batch* b, long long* buffers_in_passes, long long* passes)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (buffers_in_passes) *buffers_in_passes = b->multi_buffers;
    if (passes) *passes = b->multi_passes;
    return 1;
}

int oalsfx_batch_join_counts(const oalsfx_batch* b, long long* joined_calls, long long* joinable_launches)
{
    if (!b) { g_last_error = "Null batch."; return 0; }
    if (joined_calls) *joined_calls = b->joined_calls;
    if (joinable_launches) *joinable_launches = b->joinable_launches;
    return 1;
}

void oalsfx_debug_join_hold(oalsfx_batch* b, int k)
{
    if (!b) return;
    b->join_hold = k;
    if (k <= 1 && hipSetDevice(b->device) == hipSuccess) join_queue(b); // (a launch held back under the old setting)
}

long long oalsfx_debug_chain_same_cu(oalsfx_batch* b)
{
    // how many instance hand-overs of chained launches stayed on one CU (and paid for an L1 invalidate) so far
    unsigned v = 0;
    if (hipSetDevice(b->device) != hipSuccess || !chain_join(b) || hipStreamSynchronize(b->stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, b->d_turn + static_cast<size_t>(b->n) * b->slots + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

int oalsfx_debug_host_pipeline(oalsfx_batch* b, int* form, double* probe_us_three_streams, double* probe_us_one_stream)
{
    if (form) *form = b->pipe_mode;
    if (probe_us_three_streams) *probe_us_three_streams = b->pipe_probe_us[0];
    if (probe_us_one_stream) *probe_us_one_stream = b->pipe_probe_us[1];
    return 1;
}

unsigned long long oalsfx_trim_pools(void)
{
    return uncached_pool().trim(0);
}

unsigned long long oalsfx_pools_waiting_bytes(void) { return uncached_pool().bytes_waiting(); }

void oalsfx_debug_gate_skew(oalsfx_batch* b, unsigned skew) { if (b) b->gate_skew = skew; }
int oalsfx_debug_chain_given_up(const oalsfx_batch* b) { return b && b->chain_given_up ? 1 : 0; }

int oalsfx_debug_chain_started(oalsfx_batch* b, unsigned* host_total, unsigned* device_total)
{
    unsigned v = 0;
    if (!b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b) || !b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    if (b->d_turn && !b->hip_ok(hipMemcpy(&v, b->d_turn + static_cast<size_t>(b->n) * b->slots, sizeof(v), hipMemcpyDeviceToHost), "hipMemcpy")) return 0;
    if (host_total) *host_total = b->started_total;
    if (device_total) *device_total = v;
    return 1;
}

int oalsfx_device_pci_bus_id(int device_id, char* out, int len)
{
    if (!out || len < 16) return 0;
    return hipDeviceGetPCIBusId(out, len, device_id) == hipSuccess ? 1 : 0;
}

int oalsfx_batch_event_overhead(oalsfx_batch* b, int repeats, double* avg_us)
{
    if (repeats <= 0 || !b->hip_ok(hipSetDevice(b->device), "hipSetDevice") || !chain_join(b)) return 0;
    hipEvent_t e0 = b->take_event(), e1 = b->take_event();
    double total = 0.0;
    bool ok = true;
    for (int r = 0; r < repeats && ok; ++r) {
        oalsfx_hip::launch_null(b->stream); // something ahead in the stream, as in the timed region
        hipEventRecord(e0, b->stream);
        hipEventRecord(e1, b->stream);
        ok = hipEventSynchronize(e1) == hipSuccess;
        float ms = 0.0F;
        ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        total += ms;
    }
    b->event_pool.push_back(e0);
    b->event_pool.push_back(e1);
    if (avg_us) *avg_us = total * 1e3 / repeats;
    return ok ? 1 : 0;
}

int oalsfx_batch_placement(const oalsfx_batch* b, int* chunks, int* candidates, double* best_us, double* worst_us)
{
    if (chunks) *chunks = b->placed_chunks;
    if (candidates) *candidates = b->placement_candidates;
    if (best_us) *best_us = b->placement_best_us;
    if (worst_us) *worst_us = b->placement_worst_us;
    return 1;
}

int oalsfx_debug_probe_pointer(void* slabs, int instances, int slab_floats, int repeats, double* avg_us)
{
    // the placement probe on any device buffer of instances * slab_floats floats, always 4096 wavefronts (scripts/vram_map.py)
    if (!slabs || instances <= 0 || repeats <= 0 || slab_floats < 65536) return 0;
    const int wps = std::max(1, 4096 / instances);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int r = 0; r < 2; ++r) oalsfx_hip::launch_ring_probe(static_cast<float*>(slabs), instances, slab_floats, 256u * r, wps, nullptr);
    hipEventRecord(e0, nullptr);
    for (int r = 0; r < repeats; ++r) oalsfx_hip::launch_ring_probe(static_cast<float*>(slabs), instances, slab_floats, 256u * (2 + r), wps, nullptr);
    hipEventRecord(e1, nullptr);
    bool ok = hipEventSynchronize(e1) == hipSuccess;
    float ms = 0.0F;
    ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (avg_us) *avg_us = ms * 1e3 / repeats;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ok ? 1 : 0;
}

int oalsfx_debug_probe_rings(oalsfx_batch* b, int repeats, double* avg_us)
{
    // the reverb's ring traffic without its arithmetic (k_stream_pattern) on the batch's own delay-line chunk: overwrites the delay lines
    if (hipSetDevice(b->device) != hipSuccess || !chain_join(b) || !sync_params(b, nullptr) || b->ring_chunks.empty() || repeats <= 0) return 0;
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    const auto& rc = b->ring_chunks.front();
    const size_t slab_floats = static_cast<size_t>(ring_floats_for(OALSFX_EAX_REVERB, b->rate));
    const int instances = static_cast<int>(rc.bytes / (slab_floats * sizeof(float)));
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int r = 0; r < 4; ++r) oalsfx_hip::launch_stream_pattern(reinterpret_cast<float*>(rc.base), instances, 1, 256u * r, slab_floats, 0, b->stream);
    hipEventRecord(e0, b->stream);
    for (int r = 0; r < repeats; ++r) oalsfx_hip::launch_stream_pattern(reinterpret_cast<float*>(rc.base), instances, 1, 256u * (4 + r), slab_floats, 0, b->stream);
    hipEventRecord(e1, b->stream);
    bool ok = hipEventSynchronize(e1) == hipSuccess;
    float ms = 0.0F;
    ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (avg_us) *avg_us = ms * 1e3 / repeats;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ok ? 1 : 0;
}

int oalsfx_debug_move_rings(oalsfx_batch* b, int keep_old)
{
    if (hipSetDevice(b->device) != hipSuccess || !chain_join(b) || !sync_params(b, nullptr)) return 0;
    if (!b->hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize")) return 0;
    const size_t total = static_cast<size_t>(b->n) * b->slots;
    for (auto& rc : b->ring_chunks) {
        void* fresh = nullptr;
        if (!b->hip_ok(handed_on_malloc(b, &fresh, rc.bytes), "hipMalloc(rings)")) return 0;
        if (!b->hip_ok(hipMemcpy(fresh, rc.base, rc.bytes, hipMemcpyDeviceToDevice), "hipMemcpy(rings)")) return 0;
        const ptrdiff_t delta = static_cast<char*>(fresh) - rc.base;
        auto inside = [&](float* p) { return reinterpret_cast<char*>(p) >= rc.base && reinterpret_cast<char*>(p) < rc.base + rc.bytes; };
        auto moved = [&](float* p) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + delta); };
        for (size_t idx = 0; idx < total; ++idx)
            if (b->h_rings[idx] && inside(b->h_rings[idx])) b->h_rings[idx] = moved(b->h_rings[idx]);
        for (auto& kv : b->pools) {
            for (auto& p : kv.second.free_clean) if (inside(p)) p = moved(p);
            for (auto& p : kv.second.free_dirty) if (inside(p)) p = moved(p);
        }
        if (keep_old) {
            // stays allocated (and counted in `chunks`) so that the next move lands somewhere else again
        } else {
            for (auto& c : b->chunks) if (c == rc.alloc) c = nullptr;
            handed_on_free(rc.alloc);
        }
        b->chunks.push_back(fresh);
        rc.base = static_cast<char*>(fresh);
        rc.alloc = fresh;
    }
    return b->hip_ok(hipMemcpy(b->d_rings, b->h_rings.data(), total * sizeof(float*), hipMemcpyHostToDevice), "hipMemcpy(ring table)") ? 1 : 0;
}

unsigned long long oalsfx_debug_ring_address(oalsfx_batch* b, int instance, int slot)
{
    if (instance < 0 || instance >= b->n || slot < 0 || slot >= b->slots) return 0;
    if (hipSetDevice(b->device) != hipSuccess || !chain_join(b) || !sync_params(b, nullptr)) return 0;
    return reinterpret_cast<unsigned long long>(b->h_rings[static_cast<size_t>(instance) * b->slots + slot]);
}

void oalsfx_debug_set_flags(int flags) { g_debug_flags.store(flags < 0 ? 0 : flags, std::memory_order_relaxed); }

int oalsfx_debug_hbm_sweep(int device_id, unsigned long long bytes, int write, int repeats)
{
    if (hipSetDevice(device_id) != hipSuccess) return 0;
    float* buf = nullptr;
    float* sink = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&buf), bytes) != hipSuccess) return 0;
    if (hipMalloc(reinterpret_cast<void**>(&sink), 256) != hipSuccess) { (void)hipFree(buf); return 0; }
    (void)hipMemset(buf, 0, bytes);
    for (int r = 0; r < repeats; ++r) oalsfx_hip::launch_hbm_sweep(buf, bytes / sizeof(float), write, sink, nullptr);
    const bool ok = hipDeviceSynchronize() == hipSuccess;
    (void)hipFree(buf);
    (void)hipFree(sink);
    return ok ? 1 : 0;
}

int oalsfx_debug_sinf(int device_id, int mode, const float* in_host, void* out_host, unsigned long long count)
{
    if (mode != 0 && mode != 1) return 0;
    if (count == 0) return 1;
    if (in_host == nullptr || out_host == nullptr || hipSetDevice(device_id) != hipSuccess) return 0;
    const size_t bytes = static_cast<size_t>(count) * sizeof(float);
    float* in = nullptr;
    void* out = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&in), bytes) != hipSuccess) return 0;
    if (hipMalloc(&out, bytes) != hipSuccess) { (void)hipFree(in); return 0; }
    bool ok = hipMemcpy(in, in_host, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        oalsfx_hip::launch_debug_sinf(in, out, static_cast<size_t>(count), mode, nullptr);
        ok = hipGetLastError() == hipSuccess; // (a launch that failed leaves `out` as it was allocated)
    }
    ok = ok && hipMemcpy(out_host, out, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(in);
    (void)hipFree(out);
    return ok ? 1 : 0;
}

int oalsfx_debug_stream_pattern(int device_id, int instances, int dwords_per_lane, int repeats, int slab_floats, int pos_skew, double* avg_us)
{
    if (hipSetDevice(device_id) != hipSuccess || instances <= 0 || repeats <= 0) return 0;
    if (dwords_per_lane != 1 && dwords_per_lane != 2 && dwords_per_lane != 4) return 0;
    float* slabs = nullptr;
    if (slab_floats < 235520) return 0;
    const size_t bytes = static_cast<size_t>(instances) * slab_floats * sizeof(float);
    if (hipMalloc(reinterpret_cast<void**>(&slabs), bytes) != hipSuccess) return 0;
    (void)hipMemset(slabs, 0, bytes);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int r = 0; r < 8; ++r) oalsfx_hip::launch_stream_pattern(slabs, instances, dwords_per_lane, 256u * r, slab_floats, pos_skew, nullptr);
    hipEventRecord(e0, nullptr);
    for (int r = 0; r < repeats; ++r) oalsfx_hip::launch_stream_pattern(slabs, instances, dwords_per_lane, 256u * (8 + r), slab_floats, pos_skew, nullptr);
    hipEventRecord(e1, nullptr);
    bool ok = hipEventSynchronize(e1) == hipSuccess;
    float ms = 0.0F;
    ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (avg_us) *avg_us = ms * 1e3 / repeats;
    hipEventDestroy(e0); hipEventDestroy(e1);
    (void)hipFree(slabs);
    return ok ? 1 : 0;
}

} // extern "C"
