// Bus downmix (batch.cpp: oalsfx_batch_downmix_device, oalsfx_batch_mix_downmix): the tables the host builds from the sends and the
// launchers of downmix.hip and bus_sends.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("bus downmix", "bus sends"): per
// bus the members -- (instance, send) pairs -- in ascending order, cut into chunks of OALSFX_DOWNMIX_CHUNK; per element a chunk's partial
// p = p + (x * gain) member after member from +0.0f, then out = out + p chunk after chunk from +0.0f; fp32, product and sum rounded
// separately.  A ramping send's gain is a function of the frame.
#ifndef OALSFX_HIP_DOWNMIX_HPP
#define OALSFX_HIP_DOWNMIX_HPP

// (bus_sends.hip and the table builder are also compiled for the host, behind a shim that stands in for the runtime:
// tests/cpp/bus_sends_host.cpp)
#ifndef OALSFX_FIR_HOST_SHIM
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>
#include <vector>

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// One chunk of one bus: members[first .. first + count) and their gains, 1 <= count <= OALSFX_DOWNMIX_CHUNK.  row >= 0: the partial goes
// to that row of the scratch buffer; row < 0: the bus has this chunk only, and +0.0f + partial goes straight to the bus's output.
struct DownmixChunk { int bus, first, count, row; };
// One bus the second level writes: rows partial rows from first_row on, in chunk order (rows == 0: a bus without members, zeros).
struct DownmixSum { int bus, first_row, rows; };

// One member's gain as a function of the frame, as of the table's build.  With `since` frames downmixed since then, frame f of a call
// is n = done + since + f of the ramp: e = n < frames ? from + ((float)n * step) : to.  A member without a ramp has frames == 0 and
// to == its gain.
struct DownmixRamp {
    float from, step, to;
    uint32_t frames, done; // done <= frames <= 2^24
};

// What the host builds whenever the sends (or the number of buses a call names) have changed.
struct DownmixTable {
    std::vector<DownmixChunk> chunks;
    std::vector<DownmixSum> sums;
    std::vector<int> members;       // the instances of the routed (instance, send) pairs, bus after bus, ascending inside a bus
    std::vector<float> gains;       // gains[k]: that of members[k] (of a ramping member: where its ramp ends)
    std::vector<DownmixRamp> ramps; // ramps[k]: that of members[k]; empty where no member ramps, and the plain level 1 is launched
    int partial_rows = 0;

    // Send s of instance i: bus[s][i] in -1 .. n_buses - 1 (the caller has checked), gain[s][i]; ramp[s][i] where ramp is not null (then
    // every member gets a row, and a send that does not ramp has frames == 0 there).
    void build(const int* const bus[OALSFX_BUS_SENDS], const float* const gain[OALSFX_BUS_SENDS], const DownmixRamp* const ramp[OALSFX_BUS_SENDS], int n,
               int n_buses);
    // the five arrays packed for one copy to the device, each 16-byte aligned; offsets of the arrays in `at`
    size_t packed_bytes(size_t at[5]) const;
    void pack(char* dst) const;
};

// The same arrays in device memory.
struct DownmixDevice {
    const DownmixChunk* chunks = nullptr;
    const DownmixSum* sums = nullptr;
    const int* members = nullptr;
    const float* gains = nullptr;
    const DownmixRamp* ramps = nullptr; // null: no member ramps
    int n_chunks = 0, n_sums = 0;
};

// Floats one lane loads and stores at once (4, 2 or 1): as wide as the two buffers' addresses and the row length allow, at most
// `max_vector`.  Every width computes the same bits (the sum is element-wise).
int downmix_vector(const void* src, const void* dst, size_t elements, int max_vector);
// Whether the two grids fit a launch (elements = frames * channels of one instance).
bool downmix_fits(const DownmixDevice& t, size_t elements, int vector);
// Level 1 (one wavefront per chunk and span of 64 * vector elements) and, where some bus has no or several chunks, level 2 behind it.
// `partials`: [partial_rows][elements].  dst: [n_buses][elements], every element of every bus written exactly once.  `channels` and
// `since` are read only where the table has ramps (then level 1 is launch_ramp_chunks).
void launch_downmix(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int vector, hipStream_t stream, int channels,
                    unsigned long long since);
// Level 1 of a table with ramps (bus_sends.hip): the same grid, every member's gain formed per frame from its row of t.ramps; `since` is
// the number of frames downmixed since the table was built.  launch_downmix calls it and puts its own level 2 behind it.
void launch_ramp_chunks(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int channels, unsigned long long since,
                        int vector, hipStream_t stream);

} // namespace oalsfx_hip

#endif
