// Temporal accumulation's kernel (bdpt_reproject; bdpt_amd.h): the history of the previous
// camera's frames gathered at the place the current pixel's first hit had in them, blended with the
// current frame by sample counts. Not in the reference: pinned to the formulas of include/bdpt_amd.h and
// to their numpy restatement (bdpt_amd.py reproject_numpy), bit for bit. Only + - * /, sqrt, floor and
// comparisons, each rounded on its own (the build's -ffp-contract=off, restated below); no exp and no
// atomics, so two runs give the same bits. The primary ray's direction is the frame kernels' own
// camera_dir at spp 1 (bdpt_path.hpp), the function bdpt_debug_sampling's camera entry pins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "bdpt_path.hpp"

#pragma clang fp contract(off)

namespace bdpt {
namespace dev {

// camera_dir draws its jitter from the generator it is given iff spp != 1; the launcher's frame has spp 1
struct NoDraws {};
__device__ __forceinline__ F2 next2(NoDraws&) { return F2{0.5f, 0.5f}; }

struct ReprojectConsts {
    float w2c[12];              // the previous camera's worldToCamera, rows x, y, z: (m0 m1 m2 m3) each
    float eye_cur[3], eye_prev[3];
    float tan_x, tan_y;         // tan_prev * aspect_prev, tan_prev
    float norm, n_c, max_history, sigma_n2, sigma_depth, min_weight, clamp_k;
    int32_t demodulate;
};

// eight consecutive floats of a pixel record (feature buffers, history state): two 16-byte accesses when
// the launcher found the buffers 16-byte aligned (VEC), dwords otherwise
template <bool VEC>
__device__ __forceinline__ void load8(const float* __restrict__ p, float4& lo, float4& hi) {
    if constexpr (VEC) {
        lo = gld4(reinterpret_cast<const float4*>(p)), hi = gld4(reinterpret_cast<const float4*>(p) + 1);
    } else {
        lo = make_float4(gld1(p), gld1(p + 1), gld1(p + 2), gld1(p + 3));
        hi = make_float4(gld1(p + 4), gld1(p + 5), gld1(p + 6), gld1(p + 7));
    }
}
template <bool VEC>
__device__ __forceinline__ void store8(float* __restrict__ p, float4 lo, float4 hi) {
    if constexpr (VEC) {
        gst4(reinterpret_cast<float4*>(p), lo), gst4(reinterpret_cast<float4*>(p) + 1, hi);
    } else {
        gst1(p, lo.x), gst1(p + 1, lo.y), gst1(p + 2, lo.z), gst1(p + 3, lo.w);
        gst1(p + 4, hi.x), gst1(p + 5, hi.y), gst1(p + 6, hi.z), gst1(p + 7, hi.w);
    }
}

// I_cur of pixel q, if it is covered: c = color * norm, over m = max(alb, 1e-3) when demodulated
template <bool VEC>
__device__ __forceinline__ bool filter_colour(const float* __restrict__ color, const float* __restrict__ aov, size_t q,
                                              float norm, int demodulate, f3& I) {
    float4 a0, a1;
    load8<VEC>(aov + 8 * q, a0, a1);
    const float cov = a1.w * norm;
    if (!(cov > 0.f)) return false;
    I = mk(gld1(color + 3 * q) * norm, gld1(color + 3 * q + 1) * norm, gld1(color + 3 * q + 2) * norm);
    if (demodulate)
        I = mk(I.x / fmaxf((a0.x * norm) / cov, 1e-3f), I.y / fmaxf((a0.y * norm) / cov, 1e-3f),
               I.z / fmaxf((a0.z * norm) / cov, 1e-3f));
    return true;
}

// the snap of step 3: a coordinate within 2^-10 of an integer is that integer
__device__ __forceinline__ float snap(float f) {
    const float r = floorf(f + 0.5f);
    return fabsf(f - r) <= 0.0009765625f ? r : f;
}

// One lane per pixel, grid-stride. fr: the current camera's frame at spp 1 (camera_dir reads cam, W, spp).
template <bool VEC>
__global__ __launch_bounds__(256) void reproject_kernel(DevFrame fr, ReprojectConsts k, const float* __restrict__ color,
                                                        const float* __restrict__ aov, const float* __restrict__ hist_in,
                                                        float* __restrict__ out, float* __restrict__ hist_out) {
    const int W = fr.W, H = fr.H;
    const size_t N = static_cast<size_t>(W) * H;
    for (size_t p = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; p < N; p += static_cast<size_t>(gridDim.x) * 256) {
        float4 a0, a1;
        load8<VEC>(aov + 8 * p, a0, a1);
        const f3 c = mk(gld1(color + 3 * p) * k.norm, gld1(color + 3 * p + 1) * k.norm, gld1(color + 3 * p + 2) * k.norm);
        const float cov = a1.w * k.norm;
        if (!(cov > 0.f)) {  // a miss carries its own colour and no surface
            gst1(out + 3 * p, c.x), gst1(out + 3 * p + 1, c.y), gst1(out + 3 * p + 2, c.z);
            store8<VEC>(hist_out + 8 * p, make_float4(c.x, c.y, c.z, k.n_c), make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const f3 alb = mk((a0.x * k.norm) / cov, (a0.y * k.norm) / cov, (a0.z * k.norm) / cov);
        const f3 Np = mk((a0.w * k.norm) / cov, (a1.x * k.norm) / cov, (a1.y * k.norm) / cov);
        const float z = (a1.z * k.norm) / cov;
        const f3 m = mk(fmaxf(alb.x, 1e-3f), fmaxf(alb.y, 1e-3f), fmaxf(alb.z, 1e-3f));
        const f3 Ic = k.demodulate ? mk(c.x / m.x, c.y / m.y, c.z / m.z) : c;

        bool has = false;
        f3 Hh = mk(0.f, 0.f, 0.f);
        float n_h = 0.f;
        if (hist_in) {
            NoDraws rng;
            const f3 d = camera_dir(fr, static_cast<int>(p), rng);
            const f3 X = mk(k.eye_cur[0] + z * d.x, k.eye_cur[1] + z * d.y, k.eye_cur[2] + z * d.z);
            const float* w = k.w2c;
            const float xc = ((w[0] * X.x + w[1] * X.y) + w[2] * X.z) + w[3];
            const float yc = ((w[4] * X.x + w[5] * X.y) + w[6] * X.z) + w[7];
            const float zc = -(((w[8] * X.x + w[9] * X.y) + w[10] * X.z) + w[11]);
            if (zc >= 1.f) {  // in front of the previous camera's near plane
                const float u = xc / (zc * k.tan_x), v = yc / (zc * k.tan_y);
                const float fx = snap(((u + 1.f) * 0.5f) * static_cast<float>(W) - 0.5f);
                const float fy = snap(((1.f - v) * 0.5f) * static_cast<float>(H) - 0.5f);
                const float x0f = floorf(fx), y0f = floorf(fy);
                // (also what keeps the conversions to int defined; a tap's own test follows)
                if (x0f >= -1.f && x0f < 1073741824.f && y0f >= -1.f && y0f < 1073741824.f) {
                    const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
                    const float ax = fx - x0f, ay = fy - y0f;
                    const float bx[2] = {1.f - ax, ax}, by[2] = {1.f - ay, ay};
                    const f3 e = mk(X.x - k.eye_prev[0], X.y - k.eye_prev[1], X.z - k.eye_prev[2]);
                    const float zp = sqrt_cr(dot(e, e));
                    const float ztol = k.sigma_depth * zp;
                    float sw = 0.f, sn = 0.f;
                    f3 sI = mk(0.f, 0.f, 0.f);
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                        const float b = bx[t & 1] * by[t >> 1];
                        if (b == 0.f || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        float4 h0, h1;
                        load8<VEC>(hist_in + 8 * (static_cast<size_t>(qy) * W + qx), h0, h1);
                        if (!(h1.w > 0.f) || !(fabsf(h1.w - zp) <= ztol)) continue;
                        // (the state is [I_r I_g I_b n | N_x N_y N_z z])
                        const float nx = Np.x - h1.x, ny = Np.y - h1.y, nz = Np.z - h1.z;
                        if (!((nx * nx + ny * ny) + nz * nz <= k.sigma_n2)) continue;
                        has = true;
                        sw += b;
                        sI = mk(sI.x + b * h0.x, sI.y + b * h0.y, sI.z + b * h0.z);
                        sn += b * h0.w;
                    }
                    has = has && sw >= k.min_weight;
                    if (has) {
                        Hh = mk(sI.x / sw, sI.y / sw, sI.z / sw);
                        n_h = fminf(sn / sw, k.max_history);
                    }
                }
            }
        }

        if (!has) {  // the plain estimator
            gst1(out + 3 * p, c.x), gst1(out + 3 * p + 1, c.y), gst1(out + 3 * p + 2, c.z);
            store8<VEC>(hist_out + 8 * p, make_float4(Ic.x, Ic.y, Ic.z, k.n_c), make_float4(Np.x, Np.y, Np.z, z));
            continue;
        }
        if (k.clamp_k > 0.f) {  // the history pulled into the current frame's 3 x 3 neighbourhood
            const int x = static_cast<int>(p % W), y = static_cast<int>(p / W);
            f3 I[9];
            bool ok[9];
#pragma unroll
            for (int t = 0; t < 9; t++) {
                const int qx = x + t % 3 - 1, qy = y + t / 3 - 1;
                ok[t] = false;
                I[t] = mk(0.f, 0.f, 0.f);
                if (t == 4) {
                    ok[t] = true, I[t] = Ic;
                } else if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                    ok[t] = filter_colour<VEC>(color, aov, static_cast<size_t>(qy) * W + qx, k.norm, k.demodulate, I[t]);
                }
            }
            f3 S = mk(0.f, 0.f, 0.f), Q = mk(0.f, 0.f, 0.f);
            float cnt = 0.f;
#pragma unroll
            for (int t = 0; t < 9; t++)
                if (ok[t]) S = S + I[t], cnt += 1.f;
            const f3 mu = mk(S.x / cnt, S.y / cnt, S.z / cnt);
#pragma unroll
            for (int t = 0; t < 9; t++)
                if (ok[t]) {
                    const f3 dI = I[t] - mu;
                    Q = Q + dI * dI;
                }
            const f3 sd = mk(sqrt_cr(Q.x / cnt), sqrt_cr(Q.y / cnt), sqrt_cr(Q.z / cnt));
            const f3 lo = mu - sd * k.clamp_k, hi = mu + sd * k.clamp_k;
            Hh.x = Hh.x < lo.x ? lo.x : (Hh.x > hi.x ? hi.x : Hh.x);
            Hh.y = Hh.y < lo.y ? lo.y : (Hh.y > hi.y ? hi.y : Hh.y);
            Hh.z = Hh.z < lo.z ? lo.z : (Hh.z > hi.z ? hi.z : Hh.z);
        }
        const float n_out = n_h + k.n_c;
        const float alpha = k.n_c / n_out;
        const f3 Io = mk(Hh.x + (Ic.x - Hh.x) * alpha, Hh.y + (Ic.y - Hh.y) * alpha, Hh.z + (Ic.z - Hh.z) * alpha);
        const f3 o = k.demodulate ? Io * m : Io;
        gst1(out + 3 * p, o.x), gst1(out + 3 * p + 1, o.y), gst1(out + 3 * p + 2, o.z);
        store8<VEC>(hist_out + 8 * p, make_float4(Io.x, Io.y, Io.z, n_out), make_float4(Np.x, Np.y, Np.z, z));
    }
}

}  // namespace dev

// fr: the current camera's frame with spp 1; prev: the previous camera's constants for the same image.
// hist_in may be null (no history). width * height < 2^28 (the caller checks), so a pixel index is an int
// and 8 * pixels fits the index arithmetic with room.
hipError_t launch_reproject(const dev::DevFrame& fr, const CameraConstants& prev, float norm, float n_c, float max_history,
                            float sigma_normal, float sigma_depth, float min_weight, float clamp_sigma, int demodulate,
                            const float* color, const float* aov, const float* hist_in, float* out, float* hist_out,
                            hipStream_t st) {
    dev::ReprojectConsts k{};
    for (int r = 0; r < 3; r++) {
        for (int col = 0; col < 4; col++) k.w2c[4 * r + col] = prev.w2c[4 * col + r];  // (column-major)
        // a camera's eye is its cameraToWorld's translation
        k.eye_cur[r] = fr.cam.c2w[12 + r], k.eye_prev[r] = prev.c2w[12 + r];
    }
    k.tan_x = prev.angle * prev.aspect, k.tan_y = prev.angle;
    k.norm = norm, k.n_c = n_c, k.max_history = max_history, k.sigma_n2 = sigma_normal * sigma_normal;
    k.sigma_depth = sigma_depth, k.min_weight = min_weight, k.clamp_k = clamp_sigma, k.demodulate = demodulate;
    const size_t N = static_cast<size_t>(fr.W) * fr.H;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((N + 255) / 256, 4096));
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(aov) | reinterpret_cast<uintptr_t>(hist_in) | reinterpret_cast<uintptr_t>(hist_out);
    if (ptrs % 16 == 0)
        hipLaunchKernelGGL(dev::reproject_kernel<true>, dim3(blocks), dim3(256), 0, st, fr, k, color, aov, hist_in, out, hist_out);
    else
        hipLaunchKernelGGL(dev::reproject_kernel<false>, dim3(blocks), dim3(256), 0, st, fr, k, color, aov, hist_in, out, hist_out);
    return hipGetLastError();
}

}  // namespace bdpt
