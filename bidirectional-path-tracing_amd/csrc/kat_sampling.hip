// Per-function entry points of the path's sampling side, batched on the device, one
// element per lane (bdpt_debug_sampling, include/bdpt_amd.h): the word -> float conversion
// of every draw (canonical_f32: std::generate_canonical<float, 24> with its >= 1 clamp),
// the warps the light subpath and the direct integrator call outside the BSDFs
// (uniform_hemisphere, uniform_triangle, uniform_sphere, sphere_solid_angle), the ray-sphere
// test, the emitter selection (cdf_sample / cdf_sample_lds, sample_emitter) and the camera
// ray (camera_dir). The kernel calls the frame kernels' own device functions; the two that
// draw random numbers (sample_emitter, camera_dir) are templates on the generator and get
// their draws from a list of raw 32-bit generator outputs (DrawList), so a test can place a
// draw on a CDF knot, on 0xFFFFFF80 or on the largest float below 1.
//
// Compiled twice: kat_sampling.hip with the IEEE weight arithmetic (bit-exact to the
// reference), kat_sampling_fw.hip with BDPT_FAST_WEIGHTS 1, where sample_emitter's
// pos_pdf is rcp_w(area). Which body of sample_emitter runs (the LDS copy of the emitter
// faces and CDFs, or HBM) follows the DevScene the launch is given: sc.lds_etri_off.
#include <hip/hip_runtime.h>

#ifndef SKAT_VARIANT
#define SKAT_VARIANT
#endif
#define SKAT_PASTE(a, b) a##b
#define SKAT_NAME_(a, b) SKAT_PASTE(a, b)
#define SKAT_NAME(x) SKAT_NAME_(x, SKAT_VARIANT)  // x with the build's suffix

#include "bdpt_path.hpp"
#include "pt_sphere.hpp"

namespace bdpt {
namespace dev {

constexpr int kSamplingBlock = 64;

// A lane's next draws as the generator's raw 32-bit outputs, converted as every draw is.
struct DrawList {
    const uint32_t* w;
};
__device__ __forceinline__ float next1(DrawList& r) { return canonical_f32(*r.w++); }
__device__ __forceinline__ F2 next2(DrawList& r) {
    F2 o;
    o.x = next1(r);
    o.y = next1(r);
    return o;
}

// The face Distribution1D::sample picks for emitter e and draw u, by the body sample_emitter
// runs for this DevScene.
__device__ __forceinline__ int emitter_face(const DevScene& sc, const EmitterRecord& e, float u) {
    if (sc.lds_etri_off != kNoLds)
        return cdf_sample_lds(reinterpret_cast<const float*>(g_scene_lds + sc.lds_ecdf_off) + e.cdf_offset,
                              e.nfaces + 1, u);
    return cdf_sample(sc.emit_cdf + e.cdf_offset, e.nfaces + 1, u);
}

// fn (BDPT_SAMPLING_*), words in -> words out per element:
//   0 canonical      word                            -> float
//   1 hemisphere     u[2]                            -> d[3]
//   2 triangle       u[2]                            -> uv[2]
//   3 sphere         u[2]                            -> d[3]
//   4 solid angle    u[2], p[3], center[3], radius   -> wi[3], pdf
//   5 ray-sphere     ray[8], center[3], radius       -> hit (int)
//   6 cdf            emitter (int), u                -> face (int)
//   7 emitter        4 words                         -> id (int), emitter_pdf, face (int), pos[3], n[3], pos_pdf
//   8 camera         pixel (int), 2 words            -> d[3]
__global__ __launch_bounds__(kSamplingBlock) void SKAT_NAME(sampling_kat_kernel)(DevScene sc, DevFrame fr, int fn,
                                                                                int nin, int nout, int64_t n,
                                                                                const uint32_t* __restrict__ in,
                                                                                uint32_t* __restrict__ out) {
    scene_tables_to_lds(sc);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSamplingBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t* q = in + nin * i;
    uint32_t* o = out + nout * i;
    auto f = [&](int k) { return __uint_as_float(q[k]); };
    auto put3 = [&](int k, f3 v) {
        o[k] = __float_as_uint(v.x), o[k + 1] = __float_as_uint(v.y), o[k + 2] = __float_as_uint(v.z);
    };
    if (fn == 0) {
        o[0] = __float_as_uint(canonical_f32(q[0]));
    } else if (fn == 1) {
        put3(0, uniform_hemisphere(F2{f(0), f(1)}));
    } else if (fn == 2) {
        const F2 uv = uniform_triangle(F2{f(0), f(1)});
        o[0] = __float_as_uint(uv.x), o[1] = __float_as_uint(uv.y);
    } else if (fn == 3) {
        put3(0, uniform_sphere(F2{f(0), f(1)}));
    } else if (fn == 4) {
        float pdf;
        put3(0, sphere_solid_angle(F2{f(0), f(1)}, mk(f(2), f(3), f(4)), mk(f(5), f(6), f(7)), f(8), pdf));
        o[3] = __float_as_uint(pdf);
    } else if (fn == 5) {
        const Ray ray{mk(f(0), f(1), f(2)), mk(f(3), f(4), f(5)), f(6), f(7)};
        o[0] = ray_sphere_hit(ray, mk(f(8), f(9), f(10)), f(11)) ? 1u : 0u;
    } else if (fn == 6) {
        o[0] = static_cast<uint32_t>(emitter_face(sc, emitter_of(sc, static_cast<int>(q[0])), f(1)));
    } else if (fn == 7) {
        DrawList rng{q};
        float epdf, ppdf;
        f3 nrm, pos;
        const int id = sample_emitter(sc, rng, epdf, nrm, pos, ppdf);
        o[0] = static_cast<uint32_t>(id), o[1] = __float_as_uint(epdf);
        o[2] = static_cast<uint32_t>(emitter_face(sc, emitter_of(sc, id), canonical_f32(q[1])));
        put3(3, pos);
        put3(6, nrm);
        o[9] = __float_as_uint(ppdf);
    } else {
        DrawList rng{q + 1};
        put3(0, camera_dir(fr, static_cast<int>(q[0]), rng));
    }
}

}  // namespace dev

// launch_sampling_kat (exact), launch_sampling_kat_fw; the dynamic LDS is that of sc
hipError_t SKAT_NAME(launch_sampling_kat)(const dev::DevScene& sc, const dev::DevFrame& fr, int fn, int nin, int nout,
                                          int64_t n, const uint32_t* in, uint32_t* out, hipStream_t st) {
    if (n > 0)
        hipLaunchKernelGGL(dev::SKAT_NAME(sampling_kat_kernel),
                           dim3(static_cast<unsigned>((n + dev::kSamplingBlock - 1) / dev::kSamplingBlock)),
                           dim3(dev::kSamplingBlock), 4 * static_cast<size_t>(sc.lds_words), st, sc, fr, fn, nin, nout,
                           n, in, out);
    return hipGetLastError();
}

}  // namespace bdpt
