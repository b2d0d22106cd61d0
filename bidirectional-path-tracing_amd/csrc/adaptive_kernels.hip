// Adaptive sampling's state kernels (bdpt_adaptive_resolve, bdpt_adaptive_select; bdpt_amd.h,
// DESIGN.md §7j). Neither exists in the reference: both are pinned to the formulas of
// include/bdpt_amd.h and to their numpy restatements (bdpt_amd.py adaptive_resolve_numpy,
// adaptive_select_numpy), bit for bit. No atomics anywhere, so two runs give the same bits; every
// float operation is rounded on its own (the build's -ffp-contract=off, restated below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

namespace bdpt {
namespace dev {

// ------------------------------------------------------------------ resolve
// K plane pairs, pair b at planes + b * 2 n: T_b (the camera splats of batch b's light paths,
// t = 1) then E_b (what a pixel's own samples of batch b formed at it, t >= 2), n = W * H * 3
// floats each, as bdpt_render_pixels accumulates them. m[p]: samples per batch pixel p has had. Per float
// i of pixel p = i / 3:
//   a = m[p] > 0 ? (float)spp / (float)(K * m[p]) : 0      one IEEE division
//   plane_b = E_b * a + T_b * t                              two products, one sum
// then batch_moments_kernel's arithmetic on the K planes (aov_kernels.hip): S ascending, mu = S / K,
// Q ascending over d_b = plane_b - mu, var = Q * c. The pairs are read twice (the second pass from
// L2) rather than kept in a runtime-indexed register array. A lane owns UNIT consecutive floats:
// UNIT 4 reads and writes 16 bytes (n a multiple of 4 and 16-byte aligned pointers:
// launch_adaptive_resolve decides), UNIT 1 dwords.
template <int UNIT>
__global__ __launch_bounds__(256) void adaptive_resolve_kernel(const float* __restrict__ planes,
                                                               const int32_t* __restrict__ m, size_t n, int K, float Kf,
                                                               float sppf, float t, float c, float* __restrict__ sum,
                                                               float* __restrict__ var) {
    const size_t units = n / UNIT;
    for (size_t u = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<size_t>(gridDim.x) * 256) {
        float a[UNIT], v[UNIT], S[UNIT], mu[UNIT], Q[UNIT];
#pragma unroll
        for (int j = 0; j < UNIT; j++) {
            const int32_t mp = m[(u * UNIT + j) / 3];
            a[j] = mp > 0 ? sppf / static_cast<float>(K * mp) : 0.f;
        }
        auto load = [&](int b) {
            const float* tp = planes + static_cast<size_t>(b) * 2 * n + u * UNIT;  // T_b, then E_b
            float ev[UNIT], tv[UNIT];
            if constexpr (UNIT == 4) {
                const float4 y = *reinterpret_cast<const float4*>(tp), x = *reinterpret_cast<const float4*>(tp + n);
                ev[0] = x.x, ev[1] = x.y, ev[2] = x.z, ev[3] = x.w;
                tv[0] = y.x, tv[1] = y.y, tv[2] = y.z, tv[3] = y.w;
            } else {
                tv[0] = tp[0], ev[0] = tp[n];
            }
#pragma unroll
            for (int j = 0; j < UNIT; j++) {
                const float x = ev[j] * a[j], y = tv[j] * t;
                v[j] = x + y;
            }
        };
        for (int b = 0; b < K; b++) {  // (wave-uniform, as the second pass)
            load(b);
#pragma unroll
            for (int j = 0; j < UNIT; j++) S[j] = b == 0 ? v[j] : S[j] + v[j];
        }
#pragma unroll
        for (int j = 0; j < UNIT; j++) mu[j] = S[j] / Kf;
        for (int b = 0; b < K; b++) {
            load(b);
#pragma unroll
            for (int j = 0; j < UNIT; j++) {
                const float d = v[j] - mu[j];
                Q[j] = b == 0 ? d * d : Q[j] + d * d;
            }
        }
        if constexpr (UNIT == 4) {
            *reinterpret_cast<float4*>(sum + u * UNIT) = make_float4(S[0], S[1], S[2], S[3]);
            *reinterpret_cast<float4*>(var + u * UNIT) = make_float4(Q[0] * c, Q[1] * c, Q[2] * c, Q[3] * c);
        } else {
            sum[u] = S[0];
            var[u] = Q[0] * c;
        }
    }
}

// ------------------------------------------------------------------- select
// An ordered stream compaction for wave64 in three launches. A block owns kSelItems consecutive
// pixels and visits them in kSelRounds rounds of 256, lane by lane, so ascending lane, wave, round
// and block order is ascending pixel order.
//   flags:   every pixel's decision, one byte, and the block's count of active pixels
//            (ballot and popcount per wave, the four wave counts added through LDS)
//   scan:    one block turns the block counts into exclusive offsets and writes the total
//   scatter: rank within the wave from the ballot, the lower waves' counts through LDS, the
//            block's offset: list[offset] = p and m[p] += step for the active pixels
// The decision reads m[p] of the pixel alone, and m is written only by the scatter launch.
constexpr int kSelBlock = 256, kSelRounds = 4, kSelItems = kSelBlock * kSelRounds, kSelWaves = kSelBlock / 64;

// noisy(p): (var_r + var_g + var_b) > (thr thr) ((S_r + S_g + S_b + eps) (S_r + S_g + S_b + eps))
__device__ __forceinline__ bool adaptive_noisy(const float* __restrict__ S, const float* __restrict__ var, size_t p,
                                               float thr2, float eps) {
    const float v = (var[3 * p] + var[3 * p + 1]) + var[3 * p + 2];
    const float s = ((S[3 * p] + S[3 * p + 1]) + S[3 * p + 2]) + eps;
    return v > thr2 * (s * s);
}

__device__ __forceinline__ int lane_rank(uint64_t mask) {  // set bits of mask below this lane
    return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u)));
}

__global__ __launch_bounds__(kSelBlock) void adaptive_select_flags_kernel(const float* __restrict__ S,
                                                                          const float* __restrict__ var,
                                                                          const int32_t* __restrict__ m, int W, int H,
                                                                          float thr2, float eps, int step, int m_max,
                                                                          int dilate, uint8_t* __restrict__ flags,
                                                                          uint32_t* __restrict__ block_count) {
    __shared__ uint32_t wave_count[kSelWaves];
    const size_t N = static_cast<size_t>(W) * H;
    uint32_t cnt = 0;  // wave-uniform
    for (int r = 0; r < kSelRounds; r++) {
        const size_t p = static_cast<size_t>(blockIdx.x) * kSelItems + static_cast<size_t>(r) * kSelBlock + threadIdx.x;
        bool act = false;
        if (p < N && m[p] + step <= m_max) {
            if (!dilate) {
                act = adaptive_noisy(S, var, p, thr2, eps);
            } else {  // any pixel of the clipped 3 x 3 neighbourhood
                const int x = static_cast<int>(p % W), y = static_cast<int>(p / W);
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        act = act || adaptive_noisy(S, var, static_cast<size_t>(qy) * W + qx, thr2, eps);
                    }
            }
        }
        if (p < N) flags[p] = act ? 1 : 0;
        cnt += static_cast<uint32_t>(__popcll(__ballot(act)));
    }
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kSelWaves; w++) s += wave_count[w];
        block_count[blockIdx.x] = s;
    }
}

// block_count[0 .. nblocks) -> exclusive offsets in place; count[0] = the total
__global__ __launch_bounds__(kSelBlock) void adaptive_select_scan_kernel(uint32_t* __restrict__ block_count, uint32_t nblocks,
                                                                         int32_t* __restrict__ count) {
    __shared__ uint32_t part[kSelBlock];
    const uint32_t per = (nblocks + kSelBlock - 1) / kSelBlock;
    const uint32_t lo = min(threadIdx.x * per, nblocks), hi = min(lo + per, nblocks);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += block_count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < kSelBlock; i++) {
            const uint32_t v = part[i];
            part[i] = run;
            run += v;
        }
        count[0] = static_cast<int32_t>(run);
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t v = block_count[i];
        block_count[i] = run;
        run += v;
    }
}

// list has room for W * H entries; an offset is below the total, which is at most W * H
__global__ __launch_bounds__(kSelBlock) void adaptive_select_scatter_kernel(const uint8_t* __restrict__ flags, size_t N,
                                                                            const uint32_t* __restrict__ block_offset,
                                                                            int step, int32_t* __restrict__ m,
                                                                            int32_t* __restrict__ list) {
    __shared__ uint32_t wave_count[kSelWaves];
    uint32_t base = block_offset[blockIdx.x];  // block-uniform
    const int wave = static_cast<int>(threadIdx.x >> 6);
    for (int r = 0; r < kSelRounds; r++) {
        const size_t p = static_cast<size_t>(blockIdx.x) * kSelItems + static_cast<size_t>(r) * kSelBlock + threadIdx.x;
        const bool act = p < N && flags[p] != 0;
        const uint64_t mask = __ballot(act);
        if ((threadIdx.x & 63) == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(mask));
        __syncthreads();
        uint32_t below = 0, total = 0;
        for (int w = 0; w < kSelWaves; w++) {
            const uint32_t v = wave_count[w];
            below += w < wave ? v : 0u;
            total += v;
        }
        if (act) {
            list[base + below + static_cast<uint32_t>(lane_rank(mask))] = static_cast<int32_t>(p);
            m[p] += step;
        }
        base += total;
        __syncthreads();  // (wave_count is rewritten in the next round)
    }
}

// the driver's start: every pixel listed, every pixel at `step` samples per batch
__global__ __launch_bounds__(256) void adaptive_start_kernel(size_t N, int step, int32_t* __restrict__ m,
                                                             int32_t* __restrict__ list) {
    for (size_t p = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; p < N; p += static_cast<size_t>(gridDim.x) * 256) {
        m[p] = step;
        list[p] = static_cast<int32_t>(p);
    }
}

// samples[p] = K * m[p], the samples pixel p has had
__global__ __launch_bounds__(256) void adaptive_samples_kernel(size_t N, int K, const int32_t* __restrict__ m,
                                                               int32_t* __restrict__ samples) {
    for (size_t p = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; p < N; p += static_cast<size_t>(gridDim.x) * 256)
        samples[p] = K * m[p];
}

}  // namespace dev

// ------------------------------------------------------------ host launchers
static unsigned stride_blocks(size_t items) { return static_cast<unsigned>(std::min<size_t>((items + 255) / 256, 4096)); }

// n floats per plane, K plane pairs; t the splat scale, c = K / (K - 1) in float
hipError_t launch_adaptive_resolve(const float* planes, const int32_t* m, size_t n, int K, int spp, float t, float c,
                                   float* sum, float* var, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(var);
    const bool vec = n % 4 == 0 && ptrs % 16 == 0;  // (n % 4 == 0 keeps every plane's start aligned too)
    const unsigned blocks = stride_blocks(n / (vec ? 4 : 1));
    const float Kf = static_cast<float>(K), sppf = static_cast<float>(spp);
    if (vec)
        hipLaunchKernelGGL(dev::adaptive_resolve_kernel<4>, dim3(blocks), dim3(256), 0, st, planes, m, n, K, Kf, sppf, t, c, sum, var);
    else
        hipLaunchKernelGGL(dev::adaptive_resolve_kernel<1>, dim3(blocks), dim3(256), 0, st, planes, m, n, K, Kf, sppf, t, c, sum, var);
    return hipGetLastError();
}

// the scratch launch_adaptive_select needs: W * H flag bytes, then (16-byte aligned) a word per block
size_t adaptive_select_blocks(size_t pixels) { return (pixels + dev::kSelItems - 1) / dev::kSelItems; }
size_t adaptive_select_scratch_bytes(size_t pixels) {
    return ((pixels + 15) & ~static_cast<size_t>(15)) + sizeof(uint32_t) * adaptive_select_blocks(pixels);
}

// list: W * H entries; count: one int32 (the active pixels); m is updated for the listed pixels
hipError_t launch_adaptive_select(const float* S, const float* var, int W, int H, float thr, float eps, int step, int m_max,
                                  int dilate, int32_t* m, int32_t* list, int32_t* count, void* scratch, hipStream_t st) {
    const size_t N = static_cast<size_t>(W) * H;
    const unsigned nblocks = static_cast<unsigned>(adaptive_select_blocks(N));
    uint8_t* const flags = static_cast<uint8_t*>(scratch);
    uint32_t* const block_count = reinterpret_cast<uint32_t*>(flags + ((N + 15) & ~static_cast<size_t>(15)));
    const float thr2 = thr * thr;
    hipLaunchKernelGGL(dev::adaptive_select_flags_kernel, dim3(nblocks), dim3(dev::kSelBlock), 0, st, S, var, m, W, H, thr2, eps,
                       step, m_max, dilate, flags, block_count);
    hipLaunchKernelGGL(dev::adaptive_select_scan_kernel, dim3(1), dim3(dev::kSelBlock), 0, st, block_count, nblocks, count);
    hipLaunchKernelGGL(dev::adaptive_select_scatter_kernel, dim3(nblocks), dim3(dev::kSelBlock), 0, st, flags, N, block_count,
                       step, m, list);
    return hipGetLastError();
}

hipError_t launch_adaptive_start(size_t pixels, int step, int32_t* m, int32_t* list, hipStream_t st) {
    hipLaunchKernelGGL(dev::adaptive_start_kernel, dim3(stride_blocks(pixels)), dim3(256), 0, st, pixels, step, m, list);
    return hipGetLastError();
}

hipError_t launch_adaptive_samples(size_t pixels, int K, const int32_t* m, int32_t* samples, hipStream_t st) {
    hipLaunchKernelGGL(dev::adaptive_samples_kernel, dim3(stride_blocks(pixels)), dim3(256), 0, st, pixels, K, m, samples);
    return hipGetLastError();
}

}  // namespace bdpt
