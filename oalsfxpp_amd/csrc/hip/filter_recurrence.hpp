// The serial half of a biquad over one tile, shared by the send-filter pre-pass (support_kernels.hip: k_send_filters) and the voice
// filters (biquad.hip: k_biquad_rows): a lane runs y = (u - a1 y1) - a2 y2 over an LDS row that holds the feed-forward sums u, which
// the lane = frame phases in front of it have computed in parallel.  The including file is compiled with fp contraction off.
#ifndef OALSFX_HIP_FILTER_RECURRENCE_HPP
#define OALSFX_HIP_FILTER_RECURRENCE_HPP

// (biquad.hip is also compiled for the host, behind a shim that stands in for the runtime and has a float4 of its own:
// tests/cpp/biquad_rows_host.cpp)
#ifndef OALSFX_FIR_HOST_SHIM
#include <hip/hip_runtime.h>
#endif

namespace oalsfx_hip {

// (both with internal linkage, on purpose: every file that includes this gets a copy of its own, inlined into its kernels, and
// support_kernels.hip's code stays the code it was when the function lived there)
constexpr int kFilterRow = 4 + 64; // [2], [3]: the two samples before the tile; data from [4], 16-byte aligned

// y = (u - a1 y1) - a2 y2 over n entries of a row that holds the feed-forward sums; outputs replace them
static __device__ __forceinline__ void filter_recurrence(float* row, int n, float a1, float a2, float& y1, float& y2)
{
    auto step4 = [&](float4& v) {
        v.x = (v.x - (a1 * y1)) - (a2 * y2);
        v.y = (v.y - (a1 * v.x)) - (a2 * y1);
        v.z = (v.z - (a1 * v.y)) - (a2 * v.x);
        v.w = (v.w - (a1 * v.z)) - (a2 * v.y);
        y2 = v.z;
        y1 = v.w;
    };
    int i = 0;
    if (n == 64) {
        float4* r4 = reinterpret_cast<float4*>(row + 4);
        float4 c0 = r4[0], c1 = r4[1], c2 = r4[2], c3 = r4[3];
#pragma unroll
        for (int q = 0; q < 16; q += 4) {
            float4 n0 = c0, n1 = c1, n2 = c2, n3 = c3;
            if (q + 4 < 16) { n0 = r4[q + 4]; n1 = r4[q + 5]; n2 = r4[q + 6]; n3 = r4[q + 7]; }
            step4(c0); step4(c1); step4(c2); step4(c3);
            r4[q] = c0; r4[q + 1] = c1; r4[q + 2] = c2; r4[q + 3] = c3;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        }
        i = 64;
    }
    for (; i < n; ++i) {
        const float y = (row[4 + i] - (a1 * y1)) - (a2 * y2);
        row[4 + i] = y;
        y2 = y1;
        y1 = y;
    }
}

// The same with a pair of feedback coefficients per entry (sweep.hip: a swept voice's filter): y_i = (u_i - a1[i] y1) - a2[i] y2, a1 and
// a2 at the data of two further rows of the block (16-byte aligned, n entries each), which every channel's lane reads at the same
// address: a broadcast, no bank conflict.
static __device__ __forceinline__ void filter_recurrence_swept(float* row, const float* a1, const float* a2, int n, float& y1, float& y2)
{
    auto step4 = [&](float4& v, const float4& p, const float4& q) {
        v.x = (v.x - (p.x * y1)) - (q.x * y2);
        v.y = (v.y - (p.y * v.x)) - (q.y * y1);
        v.z = (v.z - (p.z * v.y)) - (q.z * v.x);
        v.w = (v.w - (p.w * v.z)) - (q.w * v.y);
        y2 = v.z;
        y1 = v.w;
    };
    int i = 0;
    if (n == 64) {
        float4* r4 = reinterpret_cast<float4*>(row + 4);
        const float4* p4 = reinterpret_cast<const float4*>(a1);
        const float4* q4 = reinterpret_cast<const float4*>(a2);
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            // (blocks of 8 samples, not 16: with two coefficient rows beside the sums a block of 16 holds 48 registers, which takes the
            // seven-channel kernel past 128)
            float4 c0 = r4[q], c1 = r4[q + 1];
            const float4 p0 = p4[q], p1 = p4[q + 1];
            const float4 q0 = q4[q], q1 = q4[q + 1];
            step4(c0, p0, q0); step4(c1, p1, q1);
            r4[q] = c0; r4[q + 1] = c1;
        }
        i = 64;
    }
    for (; i < n; ++i) {
        const float y = (row[4 + i] - (a1[i] * y1)) - (a2[i] * y2);
        row[4 + i] = y;
        y2 = y1;
        y1 = y;
    }
}

} // namespace oalsfx_hip

#endif
