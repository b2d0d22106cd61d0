// The sampling warps (hemisphere, Phong lobe, triangle) and the shading frame of a normal.
// Reads no build switch (phong_lobe_pdf's pow_w follows device_math.hpp's BDPT_FAST_WEIGHTS).
#pragma once

#include "dev_rng.hpp"

namespace bdpt {
namespace dev {

// -------------------------------------------------------------------- warps
// squareToUniformHemisphere (math.h:136-144)
__device__ __forceinline__ f3 uniform_hemisphere(F2 u) {
    float phi = u.x * kPi * 2.0f;
    float cosTheta = u.y;
    float sinTheta = sqrt_cr(glibc_fmaxf(1.f - (cosTheta * cosTheta), 0.f));
    const SinCos sc = glibc_sincosf2(phi);
    return mk(sinTheta * sc.c, sinTheta * sc.s, cosTheta);
}
// squareToUniformDiskConcentric + squareToCosineHemisphere (math.h:153-192)
__device__ __forceinline__ f3 cosine_hemisphere(F2 u) {
    float rx = (2.f * u.x) - 1.f;
    float ry = (2.f * u.y) - 1.f;
    // Both branches of the reference as selects (one division, one sincos per
    // lane, same operations and bits); the (0, 0) sample keeps dx = dy = 0.
    const bool zero = rx == 0 && ry == 0;
    const bool xb = (rx * rx) > (ry * ry);
    const float radius = xb ? rx : ry;
    const float q = (kPi * 0.25f) * ((xb ? ry : rx) * rcp_cr(xb ? rx : ry));
    const float phi = zero ? 0.f : (xb ? q : (kPi * 0.5f) - q);
    const SinCos sc = glibc_sincosf2(phi);
    const float dx = zero ? 0.f : radius * sc.c;
    const float dy = zero ? 0.f : radius * sc.s;
    float z = 1.0f - (dx * dx + dy * dy);
    z = glibc_fmaxf(z, 0.f);
    return mk(dx, dy, sqrt_cr(z));
}
__device__ __forceinline__ float cosine_hemisphere_pdf(f3 v) { return v.z >= 0.f ? v.z * kInvPi : 0.f; }
// squareToPhongLobe / Pdf (math.h:210-227)
__device__ __forceinline__ f3 phong_lobe(F2 u, float ex) {
    float cosTheta = glibc_powf(u.x, 1.f / (ex + 2));
    float sinTheta = sqrt_cr(glibc_fmaxf(1.f - (cosTheta * cosTheta), 0.f));
    float phi = u.y * 2.f * kPi;
    const SinCos sc = glibc_sincosf2(phi);
    return mk(sinTheta * sc.c, sinTheta * sc.s, cosTheta);
}
// EXACT: glibc's powf even in the fast-weight builds (the BSDF sampler, below)
template <bool EXACT = false>
__device__ __forceinline__ float phong_lobe_pdf(f3 v, float ex) {
    return v.z >= 0.f ? (ex + 2) * kInvTwoPi * (EXACT ? glibc_powf(v.z, ex) : pow_w(v.z, ex)) : 0.f;
}
// squareToUniformTriangle (math.h:229-234)
__device__ __forceinline__ F2 uniform_triangle(F2 s) {
    float u = sqrt_cr(1.f - s.x);
    return F2{1 - u, u * s.y};
}

// -------------------------------------------------------------------- frame
// Frame(n) with coordinateSystem (core.h:155-157, math.h:42-51): t = c, s = cross(c, n).
__device__ __forceinline__ void make_frame(f3 a, f3& s, f3& t) {
    if (fabsf(a.x) > fabsf(a.y)) {
        float inv = rcp_cr(sqrt_cr(a.x * a.x + a.z * a.z));
        t = mk(a.z * inv, 0.f, -a.x * inv);
    } else {
        float inv = rcp_cr(sqrt_cr(a.y * a.y + a.z * a.z));
        t = mk(0.f, a.z * inv, -a.y * inv);
    }
    s = cross(t, a);
}
__device__ __forceinline__ f3 to_local(f3 s, f3 t, f3 n, f3 v) { return mk(dot(v, s), dot(v, t), dot(v, n)); }
__device__ __forceinline__ f3 to_world(f3 s, f3 t, f3 n, f3 v) { return (s * v.x + t * v.y) + n * v.z; }
__device__ __forceinline__ f3 reflect_z(f3 d) { return mk(-d.x, -d.y, d.z); }
// Shading-frame conversions at a vertex with shading normal n (the frame is
// rebuilt on use rather than kept live in registers between queries).
__device__ __forceinline__ f3 local_at(f3 n, f3 v) {
    f3 s, t;
    make_frame(n, s, t);
    return to_local(s, t, n, v);
}
__device__ __forceinline__ f3 world_at(f3 n, f3 v) {
    f3 s, t;
    make_frame(n, s, t);
    return to_world(s, t, n, v);
}

}  // namespace dev
}  // namespace bdpt
