// The direct integrator's sphere emitters (reference src/integrators/direct.h:17-141, with
// Warp::squareToUniformSphere, math.h:119-127): the ray-sphere test and the two sphere
// samplers, shared by the path / direct frame kernels (pt_kernels.hip) and the per-function
// sampling kernel (kat_sampling.hip).
#pragma once

#include "dev_warp.hpp"

namespace bdpt {
namespace dev {

// quadratic + raySphereIntersect (direct.h:17-67) in double, as there: true
// when a root lies strictly inside (min_t, max_t).
__device__ BDPT_NOINLINE bool ray_sphere_hit(Ray r, f3 center, float radius) {
    const f3 no = r.o - center;
    const double cc = static_cast<double>(dot(no, no) - (radius * radius));
    const double b = static_cast<double>(dot(no, r.d)) * 2.0;
    const double a = static_cast<double>(dot(r.d, r.d));
    const double disc = b * b - 4 * a * cc;
    double t0, t1;
    if (disc > 0) {
        const double sq = __builtin_sqrt(disc);
        const double inv2a = 1 / (2 * a);
        t0 = (-b + sq) * inv2a;
        t1 = (-b - sq) * inv2a;
    } else if (disc == 0) {
        t0 = (-b + __builtin_sqrt(disc)) / (2 * a);
        t1 = t0;
    } else {
        return false;
    }
    const double lo = r.min_t, hi = r.max_t;
    return (t0 > lo && t0 < hi) || (t1 > lo && t1 < hi);
}
// Warp::squareToUniformSphere (math.h:119-127)
__device__ __forceinline__ f3 uniform_sphere(F2 u) {
    const float phi = u.x * kPi * 2.0f;
    const float cosTheta = 1.f - (2.f * u.y);
    const float sinTheta = sqrt_cr(glibc_fmaxf(1.f - cosTheta * cosTheta, 0.f));
    const SinCos sc = glibc_sincosf2(phi);
    return mk(sinTheta * sc.c, sinTheta * sc.s, cosTheta);
}
// sampleSphereBySolidAngle (direct.h:109-141)
__device__ __forceinline__ f3 sphere_solid_angle(F2 u, f3 p, f3 center, float radius, float& pdf) {
    const f3 cdir = normalize(center - p);
    const f3 dd = center - p;
    const float sin2 = radius * radius / dot(dd, dd);
    const float cosMax = sqrt_cr(glibc_fmaxf(0.f, 1.f - sin2));
    const float cosTheta = (1.f - u.x) + (u.x * cosMax);
    const float phi = u.y * kPi * 2.0f;
    const float sinTheta = sqrt_cr(glibc_fmaxf(1.f - (cosTheta * cosTheta), 0.f));
    const SinCos sc = glibc_sincosf2(phi);
    pdf = kInvTwoPi * rcp_cr(1.f - cosMax);
    return world_at(cdir, mk(sinTheta * sc.c, sinTheta * sc.s, cosTheta));
}

}  // namespace dev
}  // namespace bdpt
