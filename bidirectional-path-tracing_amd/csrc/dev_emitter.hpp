// Emitter sampling: the CDF search (HBM and LDS copies) and selectEmitter + sampleEmitterPosition.
// Reads no build switch.
#pragma once

#include "dev_warp.hpp"

namespace bdpt {
namespace dev {

// ---------------------------------------------------------------- emitters
// Distribution1D::sample (math.h:107-111): upper_bound, then clamp.
__device__ __forceinline__ int cdf_sample(const float* cdf, int ncdf, float u) {
    int lo = 0, hi = ncdf;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    int i = lo - 1;
    i = i < 0 ? 0 : i;
    return i > ncdf - 2 ? ncdf - 2 : i;
}

// The same search over an LDS copy of the CDF (address space 3: ds_read).
__device__ __forceinline__ int cdf_sample_lds(const float* cdf_generic, int ncdf, float u) {
    const __attribute__((address_space(3))) float* cdf =
        (const __attribute__((address_space(3))) float*)(cdf_generic);
    int lo = 0, hi = ncdf;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    int i = lo - 1;
    i = i < 0 ? 0 : i;
    return i > ncdf - 2 ? ncdf - 2 : i;
}

// selectEmitter + sampleEmitterPosition (integrator.cpp:46-51, :73-100): 4 draws.
// Returns the emitter index.
template <class Rng>
__device__ __forceinline__ int sample_emitter(const DevScene& sc, Rng& rng, float& emitter_pdf, f3& n, f3& pos,
                                              float& pos_pdf, int* graze = nullptr) {
    const float u0 = next1(rng);
    uint32_t id = static_cast<uint32_t>(u0 * static_cast<float>(sc.nemit));
    id = id < static_cast<uint32_t>(sc.nemit - 1) ? id : static_cast<uint32_t>(sc.nemit - 1);
    emitter_pdf = sc.inv_nemit;  // 1.f / nemit
    const EmitterRecord& e = emitter_of(sc, static_cast<int>(id));
    const bool lds = sc.lds_etri_off != kNoLds;  // uniform: LDS copies of the faces and CDFs
    const float* cdf = lds ? reinterpret_cast<const float*>(g_scene_lds + sc.lds_ecdf_off) : sc.emit_cdf;
    const float u1 = next1(rng);
    const int f = lds ? cdf_sample_lds(cdf + e.cdf_offset, e.nfaces + 1, u1)
                      : cdf_sample(cdf + e.cdf_offset, e.nfaces + 1, u1);
    const F2 uv = uniform_triangle(next2(rng));
    // Typed loads on both sides (ds_read / global_load): through one generic
    // pointer the compiler emitted FLAT loads, which wait for vmcnt(0) and
    // lgkmcnt(0) together.
    float4 a, b, c, d, g;
    if (lds) {
        typedef const __attribute__((address_space(3))) v4f_t lds_v4f;
        const lds_v4f* q = (const lds_v4f*)(g_scene_lds + sc.lds_etri_off) + 5 * (e.face_offset + f);
        const v4f_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
        a = make_float4(q0.x, q0.y, q0.z, q0.w), b = make_float4(q1.x, q1.y, q1.z, q1.w);
        c = make_float4(q2.x, q2.y, q2.z, q2.w), d = make_float4(q3.x, q3.y, q3.z, q3.w);
        g = make_float4(q4.x, q4.y, q4.z, q4.w);
    } else {
        const float4* q = sc.emit_tri + 5 * static_cast<size_t>(e.face_offset + f);
        a = gld4(q), b = gld4(q + 1), c = gld4(q + 2), d = gld4(q + 3), g = gld4(q + 4);
    }
    const f3 v0 = mk(a.x, a.y, a.z), v1 = mk(a.w, b.x, b.y), v2 = mk(b.z, b.w, c.x);
    const f3 n0 = mk(c.y, c.z, c.w), n1 = mk(d.x, d.y, d.z), n2 = mk(d.w, g.x, g.y);
    const float w = 1 - uv.x - uv.y;
    pos = (v0 * w + v1 * uv.x) + v2 * uv.y;
    n = normalize((n0 * w + n1 * uv.x) + n2 * uv.y);
    pos_pdf = rcp_w(e.area);
    if (graze) *graze = __float_as_int(g.z) << 24;  // the face's graze code (bdpt_capi.cpp device_emit_tri)
    return static_cast<int>(id);
}

}  // namespace dev
}  // namespace bdpt
