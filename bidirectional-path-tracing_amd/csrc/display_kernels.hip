// Display output's kernels (bdpt_meter, bdpt_display; bdpt_amd.h): exposure metered from a
// luminance histogram, then exposure, tone curve and the 8-bit encode. Not in the reference beyond its
// viewer's linear -> sRGB pass: pinned to the formulas of include/bdpt_amd.h and to their numpy restatements
// (bdpt_amd.py meter_numpy, display_numpy), bit for bit. Only + - * /, comparisons and integer work, each
// float operation rounded on its own (the build's -ffp-contract=off, restated below); no exp, log or pow:
// the encode is a search in a table of 255 thresholds the host made. Unlike the other post-process files this
// one HAS atomics: the histogram's counts, in LDS and in global memory. They are integer additions, so
// whatever order they land in the words are the same, and two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "bdpt_amd.h"

#pragma clang fp contract(off)

namespace bdpt {
namespace dev {

constexpr int kBins = BDPT_METER_BINS;  // bits(Y) >> 19: 8 exponent bits, 4 mantissa bits
static_assert(kBins == 4096 && kBins == 256 * 16, "the resolve block owns 16 bins per lane");

// ------------------------------------------------------------------ display
struct DisplayConsts {
    float norm, exposure, white;
    int32_t tone;
};

// steps 1 - 5 of bdpt_display for one channel value; T: the block's copy of the thresholds in LDS
template <int TONE>
__device__ __forceinline__ uint32_t display_code(float v, float norm, float e, float iw2, const float* T) {
    float x = (v * norm) * e;
    x = x > 0.f ? x : 0.f;
    x = x < 65536.f ? x : 65536.f;
    float y = x;
    if constexpr (TONE == BDPT_TONE_REINHARD) {
        const float a = 1.f + x * iw2;
        y = (x * a) / (1.f + x);
    } else if constexpr (TONE == BDPT_TONE_FILMIC) {
        const float a = 2.51f * x + 0.03f;
        const float n = x * a;
        const float b = 2.43f * x + 0.59f;
        const float d = x * b + 0.14f;
        y = n / d;
    }
    // #{k : T_k <= y} over the ascending table: 8 steps, each a compare and a conditional add
    // (the highest index read is 127 + 64 + ... + 1 - 1 = 254)
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1) pos += T[pos + step - 1] <= y ? step : 0u;
    return pos;
}

// CH: bytes per pixel of out (4: alpha 255). VEC: with CH 3 a lane owns 4 pixels, three 16-byte loads and
// three dword stores (color 16-byte, out 4-byte aligned), the W * H mod 4 pixels left over pixel by pixel;
// with CH 4 a pixel is one dword store (out 4-byte aligned). Without VEC everything goes byte by byte.
// meter: bdpt_meter's words, or null for the constants' exposure and white.
template <int TONE, int CH, bool VEC>
__global__ __launch_bounds__(256) void display_kernel(const float* __restrict__ color, const float* __restrict__ thresholds,
                                                      const uint32_t* __restrict__ meter, DisplayConsts k, size_t N,
                                                      unsigned char* __restrict__ out) {
    __shared__ float T[256];
    // (entry 255 is never read; it keeps the copy a whole block wide)
    T[threadIdx.x] = threadIdx.x < 255 ? thresholds[threadIdx.x] : 0.f;
    const float e = meter ? __uint_as_float(meter[0]) : k.exposure;
    const float w = meter ? __uint_as_float(meter[1]) : k.white;
    const float iw2 = 1.f / (w * w);
    __syncthreads();
    const size_t stride = static_cast<size_t>(gridDim.x) * 256, first = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    auto pixel = [&](size_t p) {
        const uint32_t r = display_code<TONE>(color[3 * p], k.norm, e, iw2, T);
        const uint32_t g = display_code<TONE>(color[3 * p + 1], k.norm, e, iw2, T);
        const uint32_t b = display_code<TONE>(color[3 * p + 2], k.norm, e, iw2, T);
        if constexpr (CH == 4 && VEC) {
            reinterpret_cast<uint32_t*>(out)[p] = r | g << 8 | b << 16 | 0xff000000u;
        } else {
            unsigned char* o = out + CH * p;
            o[0] = static_cast<unsigned char>(r), o[1] = static_cast<unsigned char>(g), o[2] = static_cast<unsigned char>(b);
            if constexpr (CH == 4) o[3] = 255;
        }
    };
    if constexpr (CH == 3 && VEC) {
        const size_t units = N / 4;
        for (size_t u = first; u < units; u += stride) {
            const float4* src = reinterpret_cast<const float4*>(color) + 3 * u;
            const float4 q0 = src[0], q1 = src[1], q2 = src[2];
            const float v[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            uint32_t c[12];
#pragma unroll
            for (int j = 0; j < 12; j++) c[j] = display_code<TONE>(v[j], k.norm, e, iw2, T);
            uint32_t* dst = reinterpret_cast<uint32_t*>(out) + 3 * u;
#pragma unroll
            for (int j = 0; j < 3; j++) dst[j] = c[4 * j] | c[4 * j + 1] << 8 | c[4 * j + 2] << 16 | c[4 * j + 3] << 24;
        }
        // the pixels left over, by the first lanes of the grid
        if (first < N - 4 * units) pixel(4 * units + first);
    } else {
        for (size_t p = first; p < N; p += stride) pixel(p);
    }
}

// ------------------------------------------------------------------ meter
struct MeterConsts {
    float norm, key, rate, fallback_exposure, fallback_white;
    int32_t key_permille, white_permille;
};

// A block counts its pixels into a histogram in LDS, then adds the bins it touched to the global one. A flat
// image puts every lane of a wave in one bin; collapsing such a wave to one addition (ballot, shuffle, ballot)
// was built and measured no faster on a constant image, so every counted lane adds its own 1.
__global__ __launch_bounds__(256) void meter_histogram_kernel(const float* __restrict__ color, const float* __restrict__ aov,
                                                              float norm, size_t N, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[kBins];
    for (int i = threadIdx.x; i < kBins; i += 256) bins[i] = 0;
    __syncthreads();
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    for (size_t base = static_cast<size_t>(blockIdx.x) * 256; base < N; base += stride) {
        const size_t p = base + threadIdx.x;
        bool counted = false;
        uint32_t bin = 0;
        if (p < N) {
            const float r = color[3 * p] * norm, g = color[3 * p + 1] * norm, b = color[3 * p + 2] * norm;
            const float Y = (0.212671f * r + 0.715160f * g) + 0.072169f * b;
            bin = __float_as_uint(Y) >> 19;
            counted = bin >= 16u && bin < 4080u;
            if (aov && counted) counted = aov[8 * p + 7] * norm > 0.f;
        }
        if (counted) atomicAdd(&bins[bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += 256) {
        const uint32_t c = bins[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// One block of 256 lanes, lane l owning bins 16 l .. 16 l + 15: the lanes' sums scanned through LDS, the lane
// whose range holds a rank walks its bins to it. Writes [e, w, T, b_key | b_white << 16].
__global__ __launch_bounds__(256) void meter_resolve_kernel(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ prev,
                                                            MeterConsts k, uint32_t* __restrict__ out) {
    __shared__ uint32_t scan[256];
    __shared__ uint32_t found[2];
    const int l = threadIdx.x;
    uint32_t c[16];
    const uint4* src = reinterpret_cast<const uint4*>(hist) + 4 * l;  // (the context's buffer: 16-byte aligned)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 q = src[j];
        c[4 * j] = q.x, c[4 * j + 1] = q.y, c[4 * j + 2] = q.z, c[4 * j + 3] = q.w;
    }
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) sum += c[j];
    scan[l] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the lane sums (the total is below 2^28)
        const uint32_t v = l >= d ? scan[l - d] : 0u;
        __syncthreads();
        scan[l] += v;
        __syncthreads();
    }
    const uint32_t total = scan[255];
    if (total == 0) {
        if (l == 0) {
            out[0] = __float_as_uint(k.fallback_exposure), out[1] = __float_as_uint(k.fallback_white);
            out[2] = 0, out[3] = 0;
        }
        return;
    }
    const uint32_t before = scan[l] - sum;
    const int32_t permille[2] = {k.key_permille, k.white_permille};
#pragma unroll
    for (int which = 0; which < 2; which++) {
        const uint64_t rank = (static_cast<uint64_t>(total) * static_cast<uint64_t>(permille[which]) + 999u) / 1000u;
        // rank is in 1 .. total, so exactly one lane has before < rank <= before + sum
        if (rank > before && rank <= static_cast<uint64_t>(before) + sum) {
            uint32_t run = before, b = 0;
            bool hit = false;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                run += c[j];
                if (!hit && run >= rank) hit = true, b = static_cast<uint32_t>(16 * l + j);
            }
            found[which] = b;
        }
    }
    __syncthreads();
    if (l == 0) {
        const uint32_t b_key = found[0], b_white = found[1];
        const float Y_key = __uint_as_float(b_key << 19 | 1u << 18), Y_white = __uint_as_float(b_white << 19 | 1u << 18);
        const float e_m = k.key / Y_key;
        float e = e_m;
        if (prev && k.rate < 1.f) {  // (rate 1: this frame's own exposure, not the rounded blend)
            const float e_p = __uint_as_float(prev[0]);
            if (e_p > 0.f) e = e_p + (e_m - e_p) * k.rate;
        }
        const float ew = e * Y_white;
        const float w = ew > 1.f ? ew : 1.f;
        out[0] = __float_as_uint(e), out[1] = __float_as_uint(w), out[2] = total, out[3] = b_key | b_white << 16;
    }
}

}  // namespace dev

// thresholds: the device copy of the encode's 255 floats. N = width * height < 2^28 (the caller checks).
hipError_t launch_display(const float* color, const float* thresholds, const uint32_t* meter, float norm, float exposure,
                          float white, int tone, int channels, size_t N, unsigned char* out, hipStream_t st) {
    const dev::DisplayConsts k{norm, exposure, white, tone};
    const bool vec = channels == 3 ? reinterpret_cast<uintptr_t>(color) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0
                                   : reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const size_t units = channels == 3 && vec ? std::max<size_t>(N / 4, N % 4) : N;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((std::max<size_t>(units, 1) + 255) / 256, 4096));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, color, thresholds, meter, k, N, out);
    };
    auto by_layout = [&](auto tone_c) {
        constexpr int TONE = decltype(tone_c)::value;
        if (channels == 3) vec ? go(dev::display_kernel<TONE, 3, true>) : go(dev::display_kernel<TONE, 3, false>);
        else vec ? go(dev::display_kernel<TONE, 4, true>) : go(dev::display_kernel<TONE, 4, false>);
    };
    if (tone == BDPT_TONE_CLAMP) by_layout(std::integral_constant<int, BDPT_TONE_CLAMP>{});
    else if (tone == BDPT_TONE_REINHARD) by_layout(std::integral_constant<int, BDPT_TONE_REINHARD>{});
    else by_layout(std::integral_constant<int, BDPT_TONE_FILMIC>{});
    return hipGetLastError();
}

// hist: the context's kBins words, zeroed here on the stream. A block sweeps at least 4096 pixels when the
// frame has them, so that zeroing and flushing its 4096 LDS bins is a small part of its work.
hipError_t launch_meter(const float* color, const float* aov, const uint32_t* prev, float norm, float key, int key_permille,
                        int white_permille, float rate, float fallback_exposure, float fallback_white, size_t N,
                        uint32_t* hist, uint32_t* out, hipStream_t st) {
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * dev::kBins, st);
    if (e != hipSuccess) return e;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((N + 4095) / 4096, 1024));
    hipLaunchKernelGGL(dev::meter_histogram_kernel, dim3(blocks), dim3(256), 0, st, color, aov, norm, N, hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dev::MeterConsts k{norm, key, rate, fallback_exposure, fallback_white, key_permille, white_permille};
    hipLaunchKernelGGL(dev::meter_resolve_kernel, dim3(1), dim3(256), 0, st, hist, prev, k, out);
    return hipGetLastError();
}

}  // namespace bdpt
