// First-hit feature buffers and the edge-avoiding a-trous filter for preview frames
// (DESIGN.md §11). Neither exists in the reference: the feature buffers are pinned to
// what the frame kernels compute for a sample's primary query (camera_dir, the product
// traversal, shade_hit and its texel lookup: the very functions, compiled here with
// BDPT_TEXTURED 1 so one build serves scenes with and without maps), the filter to the
// formulas of include/bdpt_amd.h.
#define BDPT_TEXTURED 1
#include <hip/hip_runtime.h>

#include <cstring>

#include "bdpt_path.hpp"

namespace bdpt {
namespace dev {

// ------------------------------------------------------------ feature buffers
// One wave per 8 x 8 pixel tile of the shard (local rows x columns): the primary rays
// of a tile are coherent, so its lanes walk the same nodes. A lane owns its pixel: the
// window's samples accumulate in registers and are added to aov[pixel][0..8) once, with
// a plain read-modify-write. Blocks stride over the tiles; a block's lanes keep the
// traversal-stack overflow columns blockIdx.x * 64 + lane (< nslots) throughout.
// mats: per material (Kd, mode) (Ks, 0) with mode 0 = albedo 1 (mirror, glass, the null
// BSDF), 1 = Kd (diffuse), 2 = min(Kd + Ks, 1) (mixture, Phong) of the material as
// ingested; read from HBM per hit (no LDS table, so no material-count limit).
constexpr int kAovTile = 8;
constexpr int kAovBlock = kAovTile * kAovTile;
constexpr int kAovChannels = 8;

__global__ __launch_bounds__(kAovBlock) void aov_kernel(DevScene sc, DevFrame fr, const float4* __restrict__ mats,
                                                        float* __restrict__ aov, uint2* __restrict__ gstack,
                                                        uint32_t nslots, int tiles_x, int ntiles) {
    __shared__ uint2 stack_mem[kLdsStack * kAovBlock];
    const uint32_t slot = blockIdx.x * kAovBlock + threadIdx.x;
    const Stack stk{stack_mem + threadIdx.x, kAovBlock, kLdsStack, gstack, nslots, slot};
    const int lx = static_cast<int>(threadIdx.x) % kAovTile, ly = static_cast<int>(threadIdx.x) / kAovTile;
    const f3 eye = mk(fr.cam_o[0], fr.cam_o[1], fr.cam_o[2]);
    for (int tile = static_cast<int>(blockIdx.x); tile < ntiles; tile += static_cast<int>(gridDim.x)) {
        const int j = (tile % tiles_x) * kAovTile + lx, lr = (tile / tiles_x) * kAovTile + ly;
        if (j >= fr.W || lr >= fr.nrows) continue;
        const int pixel = (fr.row_offset + lr * fr.row_stride) * fr.W + j;
        float acc[kAovChannels];
#pragma unroll
        for (int c = 0; c < kAovChannels; c++) acc[c] = 0.f;
        for (int i = 0; i < fr.win_count; i++) {
            const int k = fr.win_first + i * fr.win_stride;
            LazyMT rng{};
            // the jitter is the sample's first two draws, taken iff the frame's full spp > 1
            if (fr.spp != 1)
                mt_seed(rng, fr.seed_base + static_cast<uint32_t>(pixel) * static_cast<uint32_t>(fr.spp) +
                                 static_cast<uint32_t>(k));
            const Ray ray{eye, camera_dir(fr, pixel, rng), 1.f, 1000.f};  // start_sample's primary ray
            Counts cnt;
            float t = 0.f, u = 0.f, v = 0.f;
            const int res = traverse<false, false>(sc, ray, false, stk, t, u, v, cnt, kCullNear);
            if (!(res >= 0 && t <= ray.max_t && t >= ray.min_t)) continue;  // accel.h:133
            Hit h;
            shade_hit(sc, res, u, v, t, ray.d, h);
            const float4 m0 = gld4(mats + 2 * static_cast<size_t>(h.mat)), m1 = gld4(mats + 2 * static_cast<size_t>(h.mat) + 1);
            const int mode = __float_as_int(m0.w);
            f3 alb = mk(1.f, 1.f, 1.f);
            if (mode != 0) {
                alb = h.tkd >= 0 ? xyz(gld4(sc.tex_tab + h.tkd)) : xyz(m0);
                if (mode == 2) {
                    const f3 ks = h.tks >= 0 ? xyz(gld4(sc.tex_tab + h.tks)) : xyz(m1);
                    alb = mk(fminf(alb.x + ks.x, 1.f), fminf(alb.y + ks.y, 1.f), fminf(alb.z + ks.z, 1.f));
                }
            }
            acc[0] += alb.x, acc[1] += alb.y, acc[2] += alb.z;
            acc[3] += h.n.x, acc[4] += h.n.y, acc[5] += h.n.z;
            acc[6] += t, acc[7] += 1.f;
        }
        float* o = aov + kAovChannels * static_cast<size_t>(pixel);
#pragma unroll
        for (int c = 0; c < kAovChannels; c++) gst1(o + c, gld1(o + c) + acc[c] * fr.inv_spp);
    }
}

// --------------------------------------------------------------------- filter
// One lane per pixel, 32 x 8 pixel blocks (a wave: two rows of 32). Guides are packed
// once per call into two float4 per pixel — (albedo, z) and (N, coverage flag) — and the
// colour ping-pongs between two float4 images, so a tap is three 16-byte cached loads.
constexpr int kDnX = 32, kDnY = 8;

// c = color * norm, a = aov * norm; guides and I_0 (bdpt_amd.h, bdpt_denoise).
__global__ __launch_bounds__(kDnX* kDnY) void denoise_prepare_kernel(int W, int H, const float* __restrict__ color,
                                                                     const float* __restrict__ aov, float norm,
                                                                     int demodulate, float4* __restrict__ guide,
                                                                     float4* __restrict__ img) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    float a[kAovChannels];
#pragma unroll
    for (int c = 0; c < kAovChannels; c++) a[c] = gld1(aov + kAovChannels * p + c) * norm;
    const float cov = a[7];
    f3 alb = mk(1.f, 1.f, 1.f), n = mk(0.f, 0.f, 0.f);
    float z = 0.f;
    if (cov > 0.f) {
        alb = mk(a[0] / cov, a[1] / cov, a[2] / cov);
        n = mk(a[3] / cov, a[4] / cov, a[5] / cov);
        z = a[6] / cov;
    }
    f3 c = mk(gld1(color + 3 * p) * norm, gld1(color + 3 * p + 1) * norm, gld1(color + 3 * p + 2) * norm);
    if (demodulate) c = mk(c.x / fmaxf(alb.x, 1e-3f), c.y / fmaxf(alb.y, 1e-3f), c.z / fmaxf(alb.z, 1e-3f));
    gst4(guide + 2 * p, make_float4(alb.x, alb.y, alb.z, z));
    gst4(guide + 2 * p + 1, make_float4(n.x, n.y, n.z, cov > 0.f ? 1.f : 0.f));
    gst4(img + p, make_float4(c.x, c.y, c.z, 0.f));
}

// iterations == 0: out = color * norm.
__global__ __launch_bounds__(256) void denoise_scale_kernel(size_t n, const float* __restrict__ color, float norm,
                                                            float* __restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) gst1(out + i, gld1(color + i) * norm);
}

// One a-trous iteration with step s: 5 x 5 taps at p + s (dx, dy), dy outer and dx inner
// (a fixed summation order and no atomics: two runs give the same bits). inv_c / inv_n /
// inv_z2 = 1 / (sigma_color 2^-i)^2, 1 / sigma_normal^2, 1 / sigma_depth^2. LAST: the
// result goes to out (3 floats per pixel), multiplied back by max(albedo, 1e-3) when
// demodulated.
template <bool LAST>
__global__ __launch_bounds__(kDnX* kDnY) void denoise_iter_kernel(int W, int H, int s, float inv_c, float inv_n,
                                                                  float sigma_z, int demodulate,
                                                                  const float4* __restrict__ guide,
                                                                  const float4* __restrict__ src,
                                                                  float4* __restrict__ dst, float* __restrict__ out) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    const float4 ip = gld4(src + p), g0 = gld4(guide + 2 * p), g1 = gld4(guide + 2 * p + 1);
    const float zs = sigma_z * fmaxf(g0.w, 1e-6f);
    const float inv_z = 1.f / (zs * zs);
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;
        const float hy = (dy == 0 ? 6.f : (dy == -1 || dy == 1 ? 4.f : 1.f)) * 0.0625f;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float hx = (dx == 0 ? 6.f : (dx == -1 || dx == 1 ? 4.f : 1.f)) * 0.0625f;
            const size_t q = static_cast<size_t>(qy) * W + qx;
            const float4 iq = gld4(src + q);
            float w = 1.f;
            if (dx != 0 || dy != 0) {
                const float4 h0 = gld4(guide + 2 * q), h1 = gld4(guide + 2 * q + 1);
                const float cr = ip.x - iq.x, cg = ip.y - iq.y, cb = ip.z - iq.z;
                const float nx = g1.x - h1.x, ny = g1.y - h1.y, nz = g1.z - h1.z;
                const float dz = g0.w - h0.w;
                const float wc = expf(-fminf(((cr * cr + cg * cg) + cb * cb) * inv_c, 80.f));
                const float wn = expf(-fminf(((nx * nx + ny * ny) + nz * nz) * inv_n, 80.f));
                const float wz = expf(-fminf((dz * dz) * inv_z, 80.f));
                w = g1.w == h1.w ? (wc * wn) * wz : 0.f;
            }
            const float hw = (hy * hx) * w;
            sr += hw * iq.x, sg += hw * iq.y, sb += hw * iq.z, sw += hw;
        }
    }
    float r = sr / sw, g = sg / sw, b = sb / sw;
    if (LAST) {
        if (demodulate) r *= fmaxf(g0.x, 1e-3f), g *= fmaxf(g0.y, 1e-3f), b *= fmaxf(g0.z, 1e-3f);
        gst1(out + 3 * p, r), gst1(out + 3 * p + 1, g), gst1(out + 3 * p + 2, b);
    } else {
        gst4(dst + p, make_float4(r, g, b, 0.f));
    }
}

// --------------------------------------------------------- filter, many planes
// bdpt_denoise_planes (bdpt_amd.h): the planes of one frame filtered kDnP at a
// time. A lane still owns one pixel of a 32 x 8 block, and per tap it loads the two guide
// vectors of q and forms wn and wz once for the kDnP planes it carries; the planes' colours are
// kDnP float4 images (plane k of the chunk at src + k * W * H), so a tap is 2 + kDnP loads of 16
// bytes (3 + kDnP in SHARED mode) where kDnP single-plane calls take 3 kDnP. The expressions
// are denoise_iter_kernel's, restated so that kernel's device code stays what it was; a plane of
// OWN mode gets the bits of that kernel.
constexpr int kDnP = 4;

// out[i] = (planes[i] + planes[n + i] + ... in ascending plane order, starting from plane 0's
// value) * scale: float32, no atomics, the bits of that loop on the host (layers_compose_kernel
// with every bit set, for any plane count). scale 1 leaves the sum's bits.
__global__ __launch_bounds__(256) void planes_sum_kernel(const float* __restrict__ planes, size_t n, int n_planes,
                                                         float scale, float* __restrict__ out) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256) {
        float acc = gld1(planes + i);
        for (int k = 1; k < n_planes; k++) acc += gld1(planes + static_cast<size_t>(k) * n + i);  // (wave-uniform)
        gst1(out + i, acc * scale);
    }
}

// I_0 of the chunk's cnt <= kDnP planes (planes: the chunk's first, W * H * 3 floats each): c =
// plane * norm, divided by max(alb, 1e-3) of the packed guides when demodulated — the albedo
// denoise_prepare_kernel stored, so the quotient it forms.
__global__ __launch_bounds__(kDnX* kDnY) void denoise_planes_prepare_kernel(int W, int H, const float* __restrict__ planes,
                                                                            int cnt, float norm, int demodulate,
                                                                            const float4* __restrict__ guide,
                                                                            float4* __restrict__ img) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t px = static_cast<size_t>(W) * H, p = static_cast<size_t>(y) * W + x;
    const float4 g0 = gld4(guide + 2 * p);
    for (int k = 0; k < cnt; k++) {  // (wave-uniform)
        const float* src = planes + 3 * (k * px + p);
        f3 c = mk(gld1(src) * norm, gld1(src + 1) * norm, gld1(src + 2) * norm);
        if (demodulate) c = mk(c.x / fmaxf(g0.x, 1e-3f), c.y / fmaxf(g0.y, 1e-3f), c.z / fmaxf(g0.z, 1e-3f));
        gst4(img + k * px + p, make_float4(c.x, c.y, c.z, 0.f));
    }
}

// One a-trous iteration of a chunk. SHARED: the colour weight comes from the guide's image B_i
// (b: the trajectory bdpt_denoise_planes keeps), so w and the weight sum are the pixel's, one
// expf per tap beyond wn and wz whatever kDnP. Otherwise each plane has its own wc and weight
// sum from its own colour, the product kept as (wc * wn) * wz. Planes at or beyond cnt (the last
// chunk) are neither loaded nor stored. LAST: out is the chunk's first output plane.
template <bool SHARED, bool LAST>
__global__ __launch_bounds__(kDnX* kDnY) void denoise_planes_iter_kernel(int W, int H, int s, float inv_c, float inv_n,
                                                                         float sigma_z, int demodulate, int cnt,
                                                                         const float4* __restrict__ guide,
                                                                         const float4* __restrict__ b,
                                                                         const float4* __restrict__ src,
                                                                         float4* __restrict__ dst, float* __restrict__ out) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t px = static_cast<size_t>(W) * H, p = static_cast<size_t>(y) * W + x;
    const float4 g0 = gld4(guide + 2 * p), g1 = gld4(guide + 2 * p + 1);
    const float zs = sigma_z * fmaxf(g0.w, 1e-6f);
    const float inv_z = 1.f / (zs * zs);
    float4 ip[kDnP];  // the centre colours: B_i(p) in [0] when SHARED, the planes' own otherwise
    if (SHARED) {
        ip[0] = gld4(b + p);
    } else {
#pragma unroll
        for (int k = 0; k < kDnP; k++) ip[k] = k < cnt ? gld4(src + k * px + p) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sr[kDnP], sg[kDnP], sb[kDnP], sw[kDnP];
#pragma unroll
    for (int k = 0; k < kDnP; k++) sr[k] = sg[k] = sb[k] = sw[k] = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;
        const float hy = (dy == 0 ? 6.f : (dy == -1 || dy == 1 ? 4.f : 1.f)) * 0.0625f;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float hx = (dx == 0 ? 6.f : (dx == -1 || dx == 1 ? 4.f : 1.f)) * 0.0625f;
            const size_t q = static_cast<size_t>(qy) * W + qx;
            float4 iq[kDnP];
#pragma unroll
            for (int k = 0; k < kDnP; k++) iq[k] = k < cnt ? gld4(src + k * px + q) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool centre = dx == 0 && dy == 0;
            float wn = 1.f, wz = 1.f;
            bool same = true;
            float4 bq = ip[0];
            if (!centre) {
                const float4 h0 = gld4(guide + 2 * q), h1 = gld4(guide + 2 * q + 1);
                if (SHARED) bq = gld4(b + q);
                const float nx = g1.x - h1.x, ny = g1.y - h1.y, nz = g1.z - h1.z;
                const float dz = g0.w - h0.w;
                wn = expf(-fminf(((nx * nx + ny * ny) + nz * nz) * inv_n, 80.f));
                wz = expf(-fminf((dz * dz) * inv_z, 80.f));
                same = g1.w == h1.w;
            }
            float hw = 0.f;  // SHARED: plane 0's turn forms the tap's one weight, the others reuse it
#pragma unroll
            for (int k = 0; k < kDnP; k++) {
                if (!SHARED || k == 0) {
                    float w = 1.f;
                    if (!centre) {
                        const float4 cq = SHARED ? bq : iq[k];
                        const float cr = ip[k].x - cq.x, cg = ip[k].y - cq.y, cb = ip[k].z - cq.z;
                        const float wc = expf(-fminf(((cr * cr + cg * cg) + cb * cb) * inv_c, 80.f));
                        w = same ? (wc * wn) * wz : 0.f;
                    }
                    hw = (hy * hx) * w;
                    sw[k] += hw;
                }
                sr[k] += hw * iq[k].x, sg[k] += hw * iq[k].y, sb[k] += hw * iq[k].z;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kDnP; k++) {
        if (k >= cnt) break;
        const float den = sw[SHARED ? 0 : k];
        float r = sr[k] / den, g = sg[k] / den, bl = sb[k] / den;
        if (LAST) {
            if (demodulate) r *= fmaxf(g0.x, 1e-3f), g *= fmaxf(g0.y, 1e-3f), bl *= fmaxf(g0.z, 1e-3f);
            float* o = out + 3 * (k * px + p);
            gst1(o, r), gst1(o + 1, g), gst1(o + 2, bl);
        } else {
            gst4(dst + k * px + p, make_float4(r, g, bl, 0.f));
        }
    }
}

// ------------------------------------------------------------ batch moments
// bdpt_batch_moments (bdpt_amd.h): K planes of n = W * H * 3 floats, each a complete
// estimate of the frame from its own samples. Per float, every operation float32 and rounded on its
// own (the build's -ffp-contract=off; a true division):
//   S = plane_0 + plane_1 + ...  (ascending: planes_sum_kernel's loop, so layers_compose_kernel's bits)
//   mu = S / K;   Q = d_0 d_0 + d_1 d_1 + ...  (ascending, d_b = plane_b - mu);   var = Q * c
// with c = K / (K - 1) formed on the host. No atomics: the same bits every run and the bits of that
// loop on the host. The planes are read twice (the second pass from L2) rather than kept in a
// runtime-indexed register array. A lane owns UNIT consecutive floats: UNIT 4 reads and writes 16
// bytes (n a multiple of 4 and 16-byte aligned pointers: launch_batch_moments decides), UNIT 1 dwords.
// sum: null = not wanted.
template <int UNIT>
__global__ __launch_bounds__(256) void batch_moments_kernel(const float* __restrict__ planes, size_t n, int K, float Kf,
                                                            float c, float* __restrict__ sum, float* __restrict__ var) {
    const size_t units = n / UNIT;
    for (size_t u = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<size_t>(gridDim.x) * 256) {
        float v[UNIT], S[UNIT], mu[UNIT], Q[UNIT];
        auto load = [&](int b) {
            const float* src = planes + static_cast<size_t>(b) * n + u * UNIT;
            if constexpr (UNIT == 4) {
                const float4 t = gld4(reinterpret_cast<const float4*>(src));
                v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
            } else {
                v[0] = gld1(src);
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
            if (sum) gst4(reinterpret_cast<float4*>(sum + u * UNIT), make_float4(S[0], S[1], S[2], S[3]));
            gst4(reinterpret_cast<float4*>(var + u * UNIT),
                 make_float4(Q[0] * c, Q[1] * c, Q[2] * c, Q[3] * c));
        } else {
            if (sum) gst1(sum + u, S[0]);
            gst1(var + u, Q[0] * c);
        }
    }
}

// ------------------------------------------------- filter, variance-normalised
// bdpt_denoise_var (bdpt_amd.h): the a-trous filter whose colour weight measures a
// difference in standard deviations of the centre pixel, the variance carried in .w of the float4
// images and filtered with the squared weights. The shape is denoise_iter_kernel's (one lane per
// pixel, 32 x 8 blocks, three 16-byte loads per tap) and the guide expressions are restated from it
// and from denoise_prepare_kernel, so those kernels' device code stays what it was.

// Guides and I_0 as denoise_prepare_kernel forms them; img.w = U, the channel-summed variance of the
// pixel in the filter's domain: v = var * norm^2, divided by m^2 per channel when demodulated.
__global__ __launch_bounds__(kDnX* kDnY) void denoise_var_prepare_kernel(int W, int H, const float* __restrict__ color,
                                                                         const float* __restrict__ var,
                                                                         const float* __restrict__ aov, float norm,
                                                                         int demodulate, float4* __restrict__ guide,
                                                                         float4* __restrict__ img) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    float a[kAovChannels];
#pragma unroll
    for (int c = 0; c < kAovChannels; c++) a[c] = gld1(aov + kAovChannels * p + c) * norm;
    const float cov = a[7];
    f3 alb = mk(1.f, 1.f, 1.f), n = mk(0.f, 0.f, 0.f);
    float z = 0.f;
    if (cov > 0.f) {
        alb = mk(a[0] / cov, a[1] / cov, a[2] / cov);
        n = mk(a[3] / cov, a[4] / cov, a[5] / cov);
        z = a[6] / cov;
    }
    const float n2 = norm * norm;
    f3 c = mk(gld1(color + 3 * p) * norm, gld1(color + 3 * p + 1) * norm, gld1(color + 3 * p + 2) * norm);
    f3 v = mk(gld1(var + 3 * p) * n2, gld1(var + 3 * p + 1) * n2, gld1(var + 3 * p + 2) * n2);
    if (demodulate) {
        const f3 m = mk(fmaxf(alb.x, 1e-3f), fmaxf(alb.y, 1e-3f), fmaxf(alb.z, 1e-3f));
        c = mk(c.x / m.x, c.y / m.y, c.z / m.z);
        v = mk(v.x / (m.x * m.x), v.y / (m.y * m.y), v.z / (m.z * m.z));
    }
    gst4(guide + 2 * p, make_float4(alb.x, alb.y, alb.z, z));
    gst4(guide + 2 * p + 1, make_float4(n.x, n.y, n.z, cov > 0.f ? 1.f : 0.f));
    gst4(img + p, make_float4(c.x, c.y, c.z, (v.x + v.y) + v.z));
}

// V_0 = the 3 x 3 blur of U with the outer product of [1, 2, 1] / 4, renormalised over the taps inside
// the image (dy outer, dx inner): dst = (I_0, V_0). A single pixel's variance from K batches is itself
// noisy; its neighbourhood's is what the weights divide by. out_var (iterations == 0): V_0, or null.
__global__ __launch_bounds__(kDnX* kDnY) void denoise_var_blur_kernel(int W, int H, const float4* __restrict__ src,
                                                                      float4* __restrict__ dst,
                                                                      float* __restrict__ out_var) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    const float4 ip = gld4(src + p);
    float su = 0.f, sk = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        const float ky = (dy == 0 ? 2.f : 1.f) * 0.25f;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float k = ky * ((dx == 0 ? 2.f : 1.f) * 0.25f);
            su += k * gld1(&src[static_cast<size_t>(qy) * W + qx].w), sk += k;
        }
    }
    const float v0 = su / sk;
    gst4(dst + p, make_float4(ip.x, ip.y, ip.z, v0));
    if (out_var) gst1(out_var + p, v0);
}

// One iteration with step s: denoise_iter_kernel's taps, h, w_n, w_z, w_cov and order, with
//   w_c = exp(-min(|I(p) - I(q)|^2 / (sc2 V(p) + 1e-10), 80)),  sc2 = sigma_color^2 (no 2^-i: V shrinks
// by itself), the quotient formed as a product with the pixel's one reciprocal as inv_c is there;
//   I'(p) = sum hw I(q) / sum hw,   V'(p) = sum (hw hw) V(q) / ((sum hw) (sum hw)).
// LAST: out = I' (times max(albedo, 1e-3) when demodulated), out_var (null: not wanted) = V'.
template <bool LAST>
__global__ __launch_bounds__(kDnX* kDnY) void denoise_var_iter_kernel(int W, int H, int s, float sc2, float inv_n,
                                                                      float sigma_z, int demodulate,
                                                                      const float4* __restrict__ guide,
                                                                      const float4* __restrict__ src,
                                                                      float4* __restrict__ dst, float* __restrict__ out,
                                                                      float* __restrict__ out_var) {
    const int x = blockIdx.x * kDnX + threadIdx.x, y = blockIdx.y * kDnY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    const float4 ip = gld4(src + p), g0 = gld4(guide + 2 * p), g1 = gld4(guide + 2 * p + 1);
    const float zs = sigma_z * fmaxf(g0.w, 1e-6f);
    const float inv_z = 1.f / (zs * zs);
    const float inv_c = 1.f / (sc2 * ip.w + 1e-10f);
    float sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;
        const float hy = (dy == 0 ? 6.f : (dy == -1 || dy == 1 ? 4.f : 1.f)) * 0.0625f;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float hx = (dx == 0 ? 6.f : (dx == -1 || dx == 1 ? 4.f : 1.f)) * 0.0625f;
            const size_t q = static_cast<size_t>(qy) * W + qx;
            const float4 iq = gld4(src + q);
            float w = 1.f;
            if (dx != 0 || dy != 0) {
                const float4 h0 = gld4(guide + 2 * q), h1 = gld4(guide + 2 * q + 1);
                const float cr = ip.x - iq.x, cg = ip.y - iq.y, cb = ip.z - iq.z;
                const float nx = g1.x - h1.x, ny = g1.y - h1.y, nz = g1.z - h1.z;
                const float dz = g0.w - h0.w;
                const float wc = expf(-fminf(((cr * cr + cg * cg) + cb * cb) * inv_c, 80.f));
                const float wn = expf(-fminf(((nx * nx + ny * ny) + nz * nz) * inv_n, 80.f));
                const float wz = expf(-fminf((dz * dz) * inv_z, 80.f));
                w = g1.w == h1.w ? (wc * wn) * wz : 0.f;
            }
            const float hw = (hy * hx) * w;
            sr += hw * iq.x, sg += hw * iq.y, sb += hw * iq.z, sv += (hw * hw) * iq.w, sw += hw;
        }
    }
    float r = sr / sw, g = sg / sw, b = sb / sw;
    const float vn = sv / (sw * sw);
    if (LAST) {
        if (demodulate) r *= fmaxf(g0.x, 1e-3f), g *= fmaxf(g0.y, 1e-3f), b *= fmaxf(g0.z, 1e-3f);
        gst1(out + 3 * p, r), gst1(out + 3 * p + 1, g), gst1(out + 3 * p + 2, b);
        if (out_var) gst1(out_var + p, vn);
    } else {
        gst4(dst + p, make_float4(r, g, b, vn));
    }
}

// ------------------------------------------------------------ path-length layers
// out[i] = the sum over the layers l in `mask` of layers[l * n + i] (n = W * H * 3 floats per
// plane, bdpt_render_layers), float32 additions in ascending layer order starting from the
// lowest layer's value: no atomics, so the same bits every run and the bits of that sequential
// sum on the host. Grid-stride over the floats; a wave reads 256 consecutive bytes of each
// plane. mask != 0 with no bit at or above the plane count (bdpt_layers_compose checks).
__global__ __launch_bounds__(256) void layers_compose_kernel(const float* __restrict__ layers, size_t n, uint64_t mask,
                                                             float* __restrict__ out) {
    const int first = __ffsll(static_cast<unsigned long long>(mask)) - 1;
    const uint64_t rest = mask & (mask - 1);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256) {
        float acc = gld1(layers + static_cast<size_t>(first) * n + i);
        for (uint64_t m = rest; m; m &= m - 1)  // (wave-uniform)
            acc += gld1(layers + static_cast<size_t>(__ffsll(static_cast<unsigned long long>(m)) - 1) * n + i);
        gst1(out + i, acc);
    }
}

// ------------------------------------------------------------ light groups
// out[p][c] = gains[0][c] * plane_0[p][c], then + gains[g][c] * plane_g[p][c] for g = 1 ..
// n_groups - 1 in ascending order (planes of n = W * H * 3 floats, bdpt_render_light_groups):
// float32, the product and the sum rounded separately (the build's -ffp-contract=off), every
// group multiplied whatever its gain, no atomics: the same bits every run and the bits of that
// loop on the host. The gains are a kernel argument, so a slider move is one launch and no
// copy. A lane owns UNIT consecutive pixels, whose channels are then compile-time positions and
// the gains wave-uniform scalars: UNIT 4 reads each plane with three 16-byte loads (n a multiple
// of 12 and 16-byte aligned pointers: launch_relight decides), UNIT 1 with three dword loads.
struct RelightGains {
    float g[64][3];
};
template <int UNIT>
__global__ __launch_bounds__(256) void relight_kernel(const float* __restrict__ planes, size_t n, int n_groups,
                                                      RelightGains gains, float* __restrict__ out) {
    constexpr int kF = 3 * UNIT;  // floats per lane and step
    const size_t units = n / kF;
    for (size_t u = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<size_t>(gridDim.x) * 256) {
        float acc[kF];
        for (int g = 0; g < n_groups; g++) {  // (wave-uniform)
            const float* src = planes + static_cast<size_t>(g) * n + u * kF;
            float v[kF];
            if (UNIT == 4) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const float4 t = gld4(reinterpret_cast<const float4*>(src) + q);
                    v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kF; j++) v[j] = gld1(src + j);
            }
#pragma unroll
            for (int j = 0; j < kF; j++) {
                const float t = gains.g[g][j % 3] * v[j];
                acc[j] = g == 0 ? t : acc[j] + t;
            }
        }
        float* dst = out + u * kF;
        if (UNIT == 4) {
#pragma unroll
            for (int q = 0; q < 3; q++)
                gst4(reinterpret_cast<float4*>(dst) + q, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
        } else {
#pragma unroll
            for (int j = 0; j < kF; j++) gst1(dst + j, acc[j]);
        }
    }
}

// ------------------------------------------------------------ crossed planes
// The two-axis form of the relight kernel and the layer compose (bdpt_render_group_layers /
// bdpt_render_group_strategies: n_groups * n_inner planes of n = W * H * 3 floats, plane
// g * n_inner + j). With acc the first term, for g ascending and within it j ascending:
//   t = weights[j] * plane[g * n_inner + j][p][c];  t = gains[g][c] * t;  acc = acc + t
// float32, each of the three operations rounded on its own (the build's -ffp-contract=off),
// every plane multiplied whatever its gain or weight, no atomics: the same bits every run and
// the bits of that loop on the host. The gains are a kernel argument as in relight_kernel;
// weights is a device table of n_inner floats (wave-uniform reads). Lanes and UNIT as there.
template <int UNIT>
__global__ __launch_bounds__(256) void group_planes_combine_kernel(const float* __restrict__ planes, size_t n,
                                                                   int n_groups, int n_inner, RelightGains gains,
                                                                   const float* __restrict__ weights,
                                                                   float* __restrict__ out) {
    constexpr int kF = 3 * UNIT;  // floats per lane and step
    const size_t units = n / kF;
    for (size_t u = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<size_t>(gridDim.x) * 256) {
        float acc[kF];
        for (int g = 0; g < n_groups; g++) {  // (wave-uniform, as the inner loop)
            for (int i = 0; i < n_inner; i++) {
                const float* src = planes + (static_cast<size_t>(g) * n_inner + i) * n + u * kF;
                const float w = weights[i];
                float v[kF];
                if (UNIT == 4) {
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const float4 t = gld4(reinterpret_cast<const float4*>(src) + q);
                        v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kF; j++) v[j] = gld1(src + j);
                }
#pragma unroll
                for (int j = 0; j < kF; j++) {
                    const float t = gains.g[g][j % 3] * (w * v[j]);
                    acc[j] = (g | i) == 0 ? t : acc[j] + t;
                }
            }
        }
        float* dst = out + u * kF;
        if (UNIT == 4) {
#pragma unroll
            for (int q = 0; q < 3; q++)
                gst4(reinterpret_cast<float4*>(dst) + q, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
        } else {
#pragma unroll
            for (int j = 0; j < kF; j++) gst1(dst + j, acc[j]);
        }
    }
}

// ------------------------------------------------------------ strategy images
// The contact sheet of a strategy render (bdpt_render_strategies: n_s * n_t planes of W x H x 3
// floats, plane s * n_t + t - 1): one image of n_s columns by n_t rows of W x H tiles, the tile
// of (s, t) at column s, row t - 1. Float i of the sheet is gains[plane][channel] * the plane's
// float (gains null: the plane's float itself): one float32 product, no atomics, every output
// written once by one lane — the same bits every run and the bits of that loop on the host.
// Grid-stride over the sheet's floats (fewer than 2^31: bdpt_strategies_sheet checks), so a
// wave writes 256 consecutive bytes and reads 256 consecutive bytes of one plane (two at a
// tile's edge).
__global__ __launch_bounds__(256) void strategies_sheet_kernel(const float* __restrict__ planes, int n_s, int n_t,
                                                               int W, int H, const float* __restrict__ gains,
                                                               float* __restrict__ out) {
    const uint32_t row = 3u * static_cast<uint32_t>(n_s) * static_cast<uint32_t>(W);  // floats per sheet row
    const uint32_t total = row * static_cast<uint32_t>(n_t) * static_cast<uint32_t>(H);
    const size_t plane_floats = static_cast<size_t>(W) * H * 3;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t Y = i / row, q = i % row;  // sheet row; float within it
        const uint32_t X = q / 3u, c = q % 3u;
        const uint32_t s = X / static_cast<uint32_t>(W), x = X % static_cast<uint32_t>(W);
        const uint32_t r = Y / static_cast<uint32_t>(H), y = Y % static_cast<uint32_t>(H);  // r = t - 1
        const uint32_t plane = s * static_cast<uint32_t>(n_t) + r;
        const float v = gld1(planes + plane * plane_floats + (static_cast<size_t>(y) * W + x) * 3 + c);
        gst1(out + i, gains ? gld1(gains + 3u * plane + c) * v : v);
    }
}

}  // namespace dev

// gains: a device table of n_s * n_t x 3 floats, or null. The sheet has fewer than 2^31 floats.
hipError_t launch_strategies_sheet(const float* planes, int n_s, int n_t, int W, int H, const float* gains, float* out,
                                   hipStream_t st) {
    const size_t total = static_cast<size_t>(n_s) * n_t * W * H * 3;
    if (total == 0) return hipSuccess;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(dev::strategies_sheet_kernel, dim3(blocks), dim3(256), 0, st, planes, n_s, n_t, W, H, gains, out);
    return hipGetLastError();
}

// gains: n_groups x 3 floats (host). n is a multiple of 3 (W * H * 3).
hipError_t launch_relight(const float* planes, size_t n, int n_groups, const float* gains, float* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    dev::RelightGains k{};
    std::memcpy(k.g, gains, sizeof(float) * 3 * static_cast<size_t>(n_groups));
    const bool vec = n % 12 == 0 && (reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const size_t units = n / (vec ? 12 : 3);
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((units + 255) / 256, 4096));
    if (vec) hipLaunchKernelGGL(dev::relight_kernel<4>, dim3(blocks), dim3(256), 0, st, planes, n, n_groups, k, out);
    else hipLaunchKernelGGL(dev::relight_kernel<1>, dim3(blocks), dim3(256), 0, st, planes, n, n_groups, k, out);
    return hipGetLastError();
}

// gains: n_groups x 3 floats (host); weights: a device table of n_inner floats. n is a multiple of 3.
hipError_t launch_group_planes_combine(const float* planes, size_t n, int n_groups, int n_inner, const float* gains,
                                       const float* weights, float* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    dev::RelightGains k{};
    std::memcpy(k.g, gains, sizeof(float) * 3 * static_cast<size_t>(n_groups));
    const bool vec = n % 12 == 0 && (reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const size_t units = n / (vec ? 12 : 3);
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((units + 255) / 256, 4096));
    if (vec)
        hipLaunchKernelGGL(dev::group_planes_combine_kernel<4>, dim3(blocks), dim3(256), 0, st, planes, n, n_groups,
                           n_inner, k, weights, out);
    else
        hipLaunchKernelGGL(dev::group_planes_combine_kernel<1>, dim3(blocks), dim3(256), 0, st, planes, n, n_groups,
                           n_inner, k, weights, out);
    return hipGetLastError();
}

hipError_t launch_layers_compose(const float* layers, size_t n, uint64_t mask, float* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(dev::layers_compose_kernel, dim3(blocks), dim3(256), 0, st, layers, n, mask, out);
    return hipGetLastError();
}

// tiles of the shard; the grid never exceeds the lane slots the overflow columns serve
hipError_t launch_aov(const dev::DevScene& sc, const dev::DevFrame& fr, const void* mats, float* aov, uint2* gstack,
                      uint32_t nslots, hipStream_t st) {
    const int tiles_x = (fr.W + dev::kAovTile - 1) / dev::kAovTile, tiles_y = (fr.nrows + dev::kAovTile - 1) / dev::kAovTile;
    const int64_t ntiles = static_cast<int64_t>(tiles_x) * tiles_y;
    const int64_t max_grid = nslots / dev::kAovBlock;
    if (ntiles <= 0 || fr.win_count <= 0) return hipSuccess;
    if (max_grid < 1 || ntiles > 0x7fffffff) return hipErrorInvalidValue;
    const unsigned grid = static_cast<unsigned>(ntiles < max_grid ? ntiles : max_grid);
    hipLaunchKernelGGL(dev::aov_kernel, dim3(grid), dim3(dev::kAovBlock), 0, st, sc, fr,
                       static_cast<const float4*>(mats), aov, gstack, nslots, tiles_x, static_cast<int>(ntiles));
    return hipGetLastError();
}

static dim3 dn_grid(int W, int H) { return dim3((W + dev::kDnX - 1) / dev::kDnX, (H + dev::kDnY - 1) / dev::kDnY); }

hipError_t launch_denoise_prepare(int W, int H, const float* color, const float* aov, float norm, int demodulate,
                                  void* guide, void* img, hipStream_t st) {
    hipLaunchKernelGGL(dev::denoise_prepare_kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, color, aov,
                       norm, demodulate, static_cast<float4*>(guide), static_cast<float4*>(img));
    return hipGetLastError();
}
hipError_t launch_denoise_scale(size_t n, const float* color, float norm, float* out, hipStream_t st) {
    hipLaunchKernelGGL(dev::denoise_scale_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, n,
                       color, norm, out);
    return hipGetLastError();
}
hipError_t launch_denoise_iter(int W, int H, int step, float inv_c, float inv_n, float sigma_z, int demodulate,
                               const void* guide, const void* src, void* dst, float* out, bool last, hipStream_t st) {
    if (last)
        hipLaunchKernelGGL(dev::denoise_iter_kernel<true>, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, step,
                           inv_c, inv_n, sigma_z, demodulate, static_cast<const float4*>(guide),
                           static_cast<const float4*>(src), static_cast<float4*>(dst), out);
    else
        hipLaunchKernelGGL(dev::denoise_iter_kernel<false>, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H,
                           step, inv_c, inv_n, sigma_z, demodulate, static_cast<const float4*>(guide),
                           static_cast<const float4*>(src), static_cast<float4*>(dst), out);
    return hipGetLastError();
}

// n floats per plane, K planes; c = K / (K - 1) in float; sum may be null.
hipError_t launch_batch_moments(const float* planes, size_t n, int K, float c, float* sum, float* var, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(var);
    const bool vec = n % 4 == 0 && ptrs % 16 == 0;  // (n % 4 == 0 keeps every plane's start aligned too)
    const size_t units = n / (vec ? 4 : 1);
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((units + 255) / 256, 4096));
    const float Kf = static_cast<float>(K);
    if (vec) hipLaunchKernelGGL(dev::batch_moments_kernel<4>, dim3(blocks), dim3(256), 0, st, planes, n, K, Kf, c, sum, var);
    else hipLaunchKernelGGL(dev::batch_moments_kernel<1>, dim3(blocks), dim3(256), 0, st, planes, n, K, Kf, c, sum, var);
    return hipGetLastError();
}

hipError_t launch_denoise_var_prepare(int W, int H, const float* color, const float* var, const float* aov, float norm,
                                      int demodulate, void* guide, void* img, hipStream_t st) {
    hipLaunchKernelGGL(dev::denoise_var_prepare_kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, color, var,
                       aov, norm, demodulate, static_cast<float4*>(guide), static_cast<float4*>(img));
    return hipGetLastError();
}
// out_var: V_0 as W * H floats too (iterations == 0), or null.
hipError_t launch_denoise_var_blur(int W, int H, const void* src, void* dst, float* out_var, hipStream_t st) {
    hipLaunchKernelGGL(dev::denoise_var_blur_kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H,
                       static_cast<const float4*>(src), static_cast<float4*>(dst), out_var);
    return hipGetLastError();
}
// sc2 = sigma_color^2. last: the result goes to out and (unless null) out_var, not to dst.
hipError_t launch_denoise_var_iter(int W, int H, int step, float sc2, float inv_n, float sigma_z, int demodulate,
                                   const void* guide, const void* src, void* dst, float* out, float* out_var, bool last,
                                   hipStream_t st) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, step, sc2, inv_n, sigma_z,
                           demodulate, static_cast<const float4*>(guide), static_cast<const float4*>(src),
                           static_cast<float4*>(dst), out, out_var);
    };
    last ? go(dev::denoise_var_iter_kernel<true>) : go(dev::denoise_var_iter_kernel<false>);
    return hipGetLastError();
}

int denoise_planes_chunk() { return dev::kDnP; }

hipError_t launch_planes_sum(const float* planes, size_t n, int n_planes, float scale, float* out, hipStream_t st) {
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(dev::planes_sum_kernel, dim3(blocks), dim3(256), 0, st, planes, n, n_planes, scale, out);
    return hipGetLastError();
}
// planes: the chunk's first plane; cnt planes (1 .. denoise_planes_chunk()) go to img.
hipError_t launch_denoise_planes_prepare(int W, int H, const float* planes, int cnt, float norm, int demodulate,
                                         const void* guide, void* img, hipStream_t st) {
    hipLaunchKernelGGL(dev::denoise_planes_prepare_kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, planes,
                       cnt, norm, demodulate, static_cast<const float4*>(guide), static_cast<float4*>(img));
    return hipGetLastError();
}
// b: the guide's image of this iteration (shared weights), or null (every plane its own).
hipError_t launch_denoise_planes_iter(int W, int H, int step, float inv_c, float inv_n, float sigma_z, int demodulate,
                                      int cnt, const void* guide, const void* b, const void* src, void* dst, float* out,
                                      bool last, hipStream_t st) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dn_grid(W, H), dim3(dev::kDnX, dev::kDnY), 0, st, W, H, step, inv_c, inv_n, sigma_z,
                           demodulate, cnt, static_cast<const float4*>(guide), static_cast<const float4*>(b),
                           static_cast<const float4*>(src), static_cast<float4*>(dst), out);
    };
    if (b) last ? go(dev::denoise_planes_iter_kernel<true, true>) : go(dev::denoise_planes_iter_kernel<true, false>);
    else last ? go(dev::denoise_planes_iter_kernel<false, true>) : go(dev::denoise_planes_iter_kernel<false, false>);
    return hipGetLastError();
}

}  // namespace bdpt
