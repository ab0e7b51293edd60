// Bus downmix: the routed instances' outputs, [instance][frame][channel], summed into [bus][frame][channel] in the order that
// include/oalsfx_hip.h states (chunks of OALSFX_DOWNMIX_CHUNK members, then the chunks' partials), bit for bit.
//
// A streaming read of every routed row with a tiny output: what decides the time is how many loads are in flight, not the arithmetic.
// Level 1 gives every (chunk, span of the row) a wavefront of its own, which issues the loads of all its members' rows -- they do not
// depend on each other -- before the first addition; only the additions are a serial chain.  Level 2 adds a bus's partials in chunk
// order; a bus of one chunk is finished by level 1, and one without members is zeroed by level 2.  Two launches on one stream; no
// atomics (their order is not fixed), no LDS, no cross-lane traffic: the sum is element-wise, a lane owns its elements from load to store.
#include "downmix.hpp"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#pragma clang fp contract(off)

namespace oalsfx_hip {

namespace {

constexpr int kChunk = OALSFX_DOWNMIX_CHUNK;
constexpr int kWave = 64;     // one wavefront per workgroup: a (chunk, span) is the unit the grid is sized from
constexpr int kSumBatch = 8;  // loads in flight per lane in a short chunk
constexpr int kRowBatch = 32; // ... and in level 2: a big bus is a few wavefronts walking 128 rows, and every batch is a round trip

#ifndef OALSFX_FIR_HOST_SHIM
template <int V> struct Vec { typedef float type __attribute__((ext_vector_type(V))); };
template <> struct Vec<1> { typedef float type; };
#endif

} // namespace

// (the table builder below is also compiled for the host, without the kernels: tests/cpp/bus_sends_host.cpp)
#ifndef OALSFX_FIR_HOST_SHIM

// (the two kernels have names outside the anonymous namespace so that the code object's notes list them by name: tests/test_downmix_abi.py)
// Workgroup g: chunk g / spans, span g % spans of the row; lane l owns elements (span * 64 + l) * V .. + V.
template <int V>
__global__ __launch_bounds__(kWave) void k_downmix_chunks(const DownmixChunk* __restrict__ chunks, const int* __restrict__ members,
                                                          const float* __restrict__ gains, const float* __restrict__ src,
                                                          float* __restrict__ dst, float* __restrict__ partials, unsigned elements, unsigned spans)
{
    typedef typename Vec<V>::type vec;
    const DownmixChunk c = chunks[blockIdx.x / spans];
    const size_t e = (static_cast<size_t>(blockIdx.x % spans) * kWave + threadIdx.x) * V;
    if (e >= elements) return;
    const int* const m = members + c.first;
    const float* const g = gains + c.first;
    const float* const col = src + e;
    vec p;
    if (c.count == kChunk) {
        vec x[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) x[k] = *reinterpret_cast<const vec*>(col + static_cast<size_t>(m[k]) * elements);
        p = 0.0F + x[0] * g[0];
#pragma unroll
        for (int k = 1; k < kChunk; ++k) p = p + x[k] * g[k];
    } else {
        // (a bus's last chunk, or all of a small bus: the rows beyond the chunk's end are read again as its last row and not added)
        p = 0.0F;
        for (int base = 0; base < c.count; base += kSumBatch) {
            vec x[kSumBatch];
#pragma unroll
            for (int k = 0; k < kSumBatch; ++k) {
                const int at = base + k < c.count ? base + k : c.count - 1;
                x[k] = *reinterpret_cast<const vec*>(col + static_cast<size_t>(m[at]) * elements);
            }
#pragma unroll
            for (int k = 0; k < kSumBatch; ++k)
                if (base + k < c.count) p = p + x[k] * g[base + k];
        }
    }
    if (c.row < 0) *reinterpret_cast<vec*>(dst + static_cast<size_t>(c.bus) * elements + e) = 0.0F + p;
    else *reinterpret_cast<vec*>(partials + static_cast<size_t>(c.row) * elements + e) = p;
}

// Workgroup g: bus sums[g / spans], the same span and lanes as above.
template <int V>
__global__ __launch_bounds__(kWave) void k_downmix_sums(const DownmixSum* __restrict__ sums, const float* __restrict__ partials,
                                                        float* __restrict__ dst, unsigned elements, unsigned spans)
{
    typedef typename Vec<V>::type vec;
    const DownmixSum s = sums[blockIdx.x / spans];
    const size_t e = (static_cast<size_t>(blockIdx.x % spans) * kWave + threadIdx.x) * V;
    if (e >= elements) return;
    const float* const col = partials + static_cast<size_t>(s.first_row) * elements + e;
    vec out = 0.0F;
    for (int base = 0; base < s.rows; base += kRowBatch) {
        vec x[kRowBatch];
#pragma unroll
        for (int k = 0; k < kRowBatch; ++k) {
            const int at = base + k < s.rows ? base + k : s.rows - 1;
            x[k] = *reinterpret_cast<const vec*>(col + static_cast<size_t>(at) * elements);
        }
#pragma unroll
        for (int k = 0; k < kRowBatch; ++k)
            if (base + k < s.rows) out = out + x[k];
    }
    *reinterpret_cast<vec*>(dst + static_cast<size_t>(s.bus) * elements + e) = out;
}

namespace {

template <int V>
void launch(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, hipStream_t stream)
{
    const unsigned spans = static_cast<unsigned>((elements + kWave * V - 1) / (kWave * V));
    if (t.n_chunks && !t.ramps)
        hipLaunchKernelGGL(k_downmix_chunks<V>, dim3(static_cast<unsigned>(t.n_chunks) * spans), dim3(kWave), 0, stream, t.chunks, t.members, t.gains, src, dst,
                           partials, static_cast<unsigned>(elements), spans);
    if (t.n_sums)
        hipLaunchKernelGGL(k_downmix_sums<V>, dim3(static_cast<unsigned>(t.n_sums) * spans), dim3(kWave), 0, stream, t.sums, partials, dst,
                           static_cast<unsigned>(elements), spans);
}

} // namespace
#endif

namespace {

size_t round16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }

} // namespace

void DownmixTable::build(const int* const bus[OALSFX_BUS_SENDS], const float* const gain[OALSFX_BUS_SENDS], const DownmixRamp* const ramp[OALSFX_BUS_SENDS],
                         int n, int n_buses)
{
    chunks.clear();
    sums.clear();
    partial_rows = 0;
    // counting sort by bus: ascending (instance, send) order inside a bus comes with it
    std::vector<int> start(static_cast<size_t>(n_buses) + 1, 0);
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < OALSFX_BUS_SENDS; ++s)
            if (bus[s][i] >= 0) ++start[bus[s][i] + 1];
    for (int k = 0; k < n_buses; ++k) start[k + 1] += start[k];
    members.assign(start[n_buses], 0);
    gains.assign(start[n_buses], 0.0F);
    ramps.assign(ramp ? start[n_buses] : 0, DownmixRamp{});
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < OALSFX_BUS_SENDS; ++s)
            if (bus[s][i] >= 0) {
                const int at = fill[bus[s][i]]++;
                members[at] = i;
                const bool ramping = ramp && ramp[s][i].frames;
                gains[at] = ramping ? ramp[s][i].to : gain[s][i];
                if (ramp) ramps[at] = ramping ? ramp[s][i] : DownmixRamp{gain[s][i], 0.0F, gain[s][i], 0, 0};
            }
    for (int k = 0; k < n_buses; ++k) {
        const int count = start[k + 1] - start[k], rows = (count + kChunk - 1) / kChunk;
        if (rows == 1) {
            chunks.push_back({k, start[k], count, -1});
            continue;
        }
        sums.push_back({k, partial_rows, rows});
        for (int j = 0; j < rows; ++j) {
            const int first = start[k] + j * kChunk;
            chunks.push_back({k, first, std::min(kChunk, start[k + 1] - first), partial_rows++});
        }
    }
}

size_t DownmixTable::packed_bytes(size_t at[5]) const
{
    at[0] = 0;
    at[1] = at[0] + round16(chunks.size() * sizeof(DownmixChunk));
    at[2] = at[1] + round16(sums.size() * sizeof(DownmixSum));
    at[3] = at[2] + round16(members.size() * sizeof(int));
    at[4] = at[3] + round16(gains.size() * sizeof(float));
    return at[4] + round16(ramps.size() * sizeof(DownmixRamp));
}

void DownmixTable::pack(char* dst) const
{
    size_t at[5];
    packed_bytes(at);
    if (!chunks.empty()) std::memcpy(dst + at[0], chunks.data(), chunks.size() * sizeof(DownmixChunk));
    if (!sums.empty()) std::memcpy(dst + at[1], sums.data(), sums.size() * sizeof(DownmixSum));
    if (!members.empty()) std::memcpy(dst + at[2], members.data(), members.size() * sizeof(int));
    if (!gains.empty()) std::memcpy(dst + at[3], gains.data(), gains.size() * sizeof(float));
    if (!ramps.empty()) std::memcpy(dst + at[4], ramps.data(), ramps.size() * sizeof(DownmixRamp));
}

int downmix_vector(const void* src, const void* dst, size_t elements, int max_vector)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (elements * sizeof(float));
    const int fits = bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1;
    const int cap = max_vector >= 4 ? 4 : max_vector >= 2 ? 2 : 1;
    return fits < cap ? fits : cap;
}

bool downmix_fits(const DownmixDevice& t, size_t elements, int vector)
{
    if (elements > UINT_MAX) return false;
    const unsigned long long spans = (elements + static_cast<size_t>(kWave) * vector - 1) / (static_cast<size_t>(kWave) * vector);
    return spans * static_cast<unsigned long long>(t.n_chunks) <= INT_MAX && spans * static_cast<unsigned long long>(t.n_sums) <= INT_MAX;
}

#ifndef OALSFX_FIR_HOST_SHIM
void launch_downmix(const DownmixDevice& t, const float* src, float* dst, float* partials, size_t elements, int vector, hipStream_t stream, int channels,
                    unsigned long long since)
{
    // (a table with ramps: level 1 is bus_sends.hip's, and level 2, below, the same)
    if (t.ramps && t.n_chunks) launch_ramp_chunks(t, src, dst, partials, elements, channels, since, vector, stream);
    if (vector >= 4) launch<4>(t, src, dst, partials, elements, stream);
    else if (vector >= 2) launch<2>(t, src, dst, partials, elements, stream);
    else launch<1>(t, src, dst, partials, elements, stream);
}
#endif

} // namespace oalsfx_hip
