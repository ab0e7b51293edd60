// Bus downmix (batch.cpp: oalsfx_batch_downmix_device, oalsfx_batch_mix_downmix): the tables the host builds from the routing and the
// launchers of downmix.hip.  The arithmetic is the contract of include/oalsfx_hip.h ("bus downmix"): per bus the members in ascending
// instance order, cut into chunks of OALSFX_DOWNMIX_CHUNK; per element a chunk's partial p = p + (x * gain) member after member from
// +0.0f, then out = out + p chunk after chunk from +0.0f; fp32, product and sum rounded separately.
#ifndef OALSFX_HIP_DOWNMIX_HPP
#define OALSFX_HIP_DOWNMIX_HPP

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "oalsfx_hip.h"

namespace oalsfx_hip {

// One chunk of one bus: members[first .. first + count) and their gains, 1 <= count <= OALSFX_DOWNMIX_CHUNK.  row >= 0: the partial goes
// to that row of the scratch buffer; row < 0: the bus has this chunk only, and +0.0f + partial goes straight to the bus's output.
struct DownmixChunk { int bus, first, count, row; };
// One bus the second level writes: rows partial rows from first_row on, in chunk order (rows == 0: a bus without members, zeros).
struct DownmixSum { int bus, first_row, rows; };

// What the host builds whenever the routing (or the number of buses a call names) has changed.
struct DownmixTable {
    std::vector<DownmixChunk> chunks;
    std::vector<DownmixSum> sums;
    std::vector<int> members;   // routed instances, bus after bus, ascending inside a bus
    std::vector<float> gains;   // gains[k]: that of members[k]
    int partial_rows = 0;

    // bus[i] in -1 .. n_buses - 1 (the caller has checked)
    void build(const int* bus, const float* gain, int n, int n_buses);
    // the four arrays packed for one copy to the device, each 16-byte aligned; offsets of the arrays in `at`
    size_t packed_bytes(size_t at[4]) const;
    void pack(char* dst) const;
};

// The same arrays in device memory.
struct DownmixDevice {
    const DownmixChunk* chunks = nullptr;
    const DownmixSum* sums = nullptr;
    const int* members = nullptr;
    const float* gains = nullptr;
    int n_chunks = 0, n_sums = 0;
};

// Floats one lane loads and stores at once (4, 2 or 1): as wide as the two buffers' addresses and the row length allow, at most
// `max_vector`.  Every width computes the same bits (the sum is element-wise).
int downmix_vector(const void* src, const void* dst, size_t elements, int max_vector);
// Whether the two grids fit a launch (elements = frames * channels of one instance).
bool downmix_fits(const DownmixDevice& t, size_t elements, int vector);
// Level 1 (one wavefront per chunk and span of 64 * vector elements) and, where some bus has no or several chunks, level 2 behind it.
// `partials`: [partial_rows][elements].  dst: [n_buses][elements], every element of every bus written exactly once.
void launch_downmix(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int vector, hipStream_t stream);

} // namespace oalsfx_hip

#endif
