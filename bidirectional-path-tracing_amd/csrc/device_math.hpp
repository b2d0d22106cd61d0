// Device math for the BDPT kernels, bit-faithful to the reference's x86 build.
//
// Every float operation here must round exactly like the reference's g++ -O2
// SSE2 code: the kernels are compiled with -ffp-contract=off (no a*b+c fusion)
// and HIP's default correctly-rounded f32 division and square root. glm's
// operation order is mirrored explicitly (externals/glm/glm/detail/
// func_geometric.inl: dot = (x*x' + y*y') + z*z', normalize = v * (1/sqrt(dot)),
// cross as written at :74-83).
//
// The transcendental functions reproduce glibc 2.35's x86_64 FMA-multiarch
// sinf / cosf / powf (the ARM optimized-routines algorithms: double-precision
// polynomials on a 16/32-entry table), which is what the reference's
// std::sinf / std::cosf / std::powf calls (src/core/math.h:125-242,
// src/bsdfs/mixture.h:70) resolve to on an FMA+AVX2 host. CDNA4 has full-rate
// enough FP64 FMA for this to cost a few dozen cycles per call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bdpt {
namespace dev {

// Large, rarely-divergent helpers are real calls: one copy of their code in the
// megakernel instead of one per call site (i-cache and register pressure).
#define BDPT_NOINLINE __attribute__((noinline))

// Relaxed agent-scope atomic adds on pointers named global (global_atomic_*):
// HIP's atomicAdd on a generic pointer the compiler cannot place becomes a FLAT
// atomic, which also makes the wave's next waits cover LDS (lgkmcnt) too.
typedef __attribute__((address_space(1))) float gfloat_t;
typedef __attribute__((address_space(1))) uint32_t gu32_t;
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
__device__ __forceinline__ void gadd(float* p, float v) {
    __hip_atomic_fetch_add((gfloat_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t gadd(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add((gu32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long gadd(unsigned long long* p, unsigned long long v) {
    return __hip_atomic_fetch_add((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gmax(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_max((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gmin(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_min((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- float3
struct f3 {
    float x, y, z;
};
__device__ __forceinline__ f3 mk(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float div_cr(float a, float b);
__device__ __forceinline__ float rcp_cr(float x);
__device__ __forceinline__ f3 operator/(f3 a, float s) { return mk(div_cr(a.x, s), div_cr(a.y, s), div_cr(a.z, s)); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
    return mk(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
__device__ __forceinline__ float sqrt_cr(float x) { return __builtin_sqrtf(x); }

// Correctly rounded reciprocal and division in a few instructions instead of
// the ~10 of the IEEE division sequence. rcp: v_rcp_f32 (1 ulp) plus one FMA
// Newton step, equal to 1.0f / x for every x with 2^-126 <= |x| < 2^126
// (checked on the GPU over all 2^32 inputs, tools/numerics/rcp_check.hip).
// div: q = a * rcp(b) corrected by one FMA residual step (Markstein), equal to
// a / b when the reciprocal is correctly rounded and nothing over/underflows;
// the guard keeps |a| in [2^-60, 2^60] and |b| in [2^-40, 2^40] (0 mismatches
// over 2^32 random pairs there). Anything else takes the IEEE division, so both
// return exactly what `/` returns.
__device__ __forceinline__ float rcp_nr(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ float rcp_cr(float x) {
    return 1.0f / x;
}
// The triangle test's 1 / det: |det| >= 1e-8 is known, so only the upper bound is checked.
__device__ __forceinline__ float rcp_det(float det) {
    if (__builtin_expect(__builtin_fabsf(det) < 0x1p126f, 1)) return rcp_nr(det);
    return 1.0f / det;
}
__device__ __forceinline__ float div_cr(float a, float b) {
    return a / b;
}
__device__ __forceinline__ f3 normalize(f3 v) { return v * rcp_cr(sqrt_cr(dot(v, v))); }

// Arithmetic that only WEIGHTS a path — the MIS recursion (vc, vcm), pdf ratios,
// throughput and contributions — and never steers it (no direction, hit, pixel or
// random-number decision depends on it; a cosine sign computed from a direction
// normalized this way flips only where the connection's contribution is 0). With
// BDPT_FAST_WEIGHTS these take the hardware's 1-ulp v_rcp_f32 / v_sqrt_f32 /
// v_rsq_f32 instead of the correctly rounded ~11-instruction sequences: every
// sample still follows the reference's path bit for bit, its contributions differ
// by a few ulp (per-pixel ~1e-6 relative, against the 1e-4 bound). The frame
// kernels without Russian roulette build with it (bdpt_kernels.hip); the Russian-
// roulette build (whose throughput steers the roulette) and the single-sample and
// per-function kernels keep the IEEE operations.
#ifndef BDPT_FAST_WEIGHTS
#define BDPT_FAST_WEIGHTS 0
#endif
__device__ __forceinline__ float rcp_w(float x) { return BDPT_FAST_WEIGHTS ? __builtin_amdgcn_rcpf(x) : rcp_cr(x); }
// a * rcp(b) alone is NaN where a / b is not: 0 * inf for a zero a over a denormal b (whose
// reciprocal overflows) and inf * 0 for an infinite a over |b| >= 2^126 (whose reciprocal, a
// denormal, is flushed). v_div_fixup_f32 (quotient, denominator, numerator) returns IEEE's
// signed 0 / inf / NaN when an operand is 0, inf or NaN and the quotient's own bits otherwise,
// so every other result is that of the bare product (tests/test_gpu_kat_connection.py).
__device__ __forceinline__ float div_w(float a, float b) {
    return BDPT_FAST_WEIGHTS ? __builtin_amdgcn_div_fixupf(a * __builtin_amdgcn_rcpf(b), b, a) : div_cr(a, b);
}
__device__ __forceinline__ float sqrt_w(float x) { return BDPT_FAST_WEIGHTS ? __builtin_amdgcn_sqrtf(x) : sqrt_cr(x); }
__device__ __forceinline__ float rsqrt_w(float x) { return BDPT_FAST_WEIGHTS ? __builtin_amdgcn_rsqf(x) : rcp_cr(sqrt_cr(x)); }
__device__ __forceinline__ bool is_zero(f3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }
__device__ __forceinline__ f3 xyz(float4 q) { return mk(q.x, q.y, q.z); }

// glibc 2.35 x86_64 fmaxf / fminf (maxss / minss): the second operand wins ties.
__device__ __forceinline__ float glibc_fmaxf(float x, float y) {
    if (x != x) return y;
    if (y != y) return x;
    return x > y ? x : y;
}
__device__ __forceinline__ float glibc_fminf(float x, float y) {
    if (x != x) return y;
    if (y != y) return x;
    return x < y ? x : y;
}

// static_cast<int>(float) as x86 cvttss2si: NaN / out of range -> INT_MIN.
__device__ __forceinline__ int x86_trunc_i32(float f) {
    if (!(f > -2147483648.f && f < 2147483648.f)) return INT32_MIN;
    return static_cast<int>(f);
}

// ------------------------------------------------------------- sin / cos
// glibc __inv_pio4: bits of 4/pi.
static __constant__ uint32_t kInvPio4[24] = {0xa2,       0xa2f9,     0xa2f983,   0xa2f9836e, 0xf9836e4e, 0x836e4e44,
                               0x6e4e4415, 0x4e441529, 0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1,
                               0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0, 0x34ddc0db, 0xddc0db62,
                               0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041};

__device__ __forceinline__ uint32_t f2u(float f) { return __float_as_uint(f); }
__device__ __forceinline__ uint32_t abstop12(float x) { return (f2u(x) >> 20) & 0x7ff; }

// glibc sincosf.h tables, in its field order {c0, c1, s1, c2, s2, c3, s3, c4}.
struct SinCosPoly {
    double c0, c1, s1, c2, s2, c3, s3, c4;
};
__device__ __forceinline__ SinCosPoly sincos_poly_table(bool negate_cos) {
    const double c0 = 0x1p+0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10,
                 c4 = 0x1.99343027bf8c3p-16;
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    if (negate_cos) return SinCosPoly{-c0, -c1, s1, -c2, s2, -c3, s3, -c4};
    return SinCosPoly{c0, c1, s1, c2, s2, c3, s3, c4};
}

// sinf_poly: even n -> sine polynomial of x, odd n -> cosine polynomial.
__device__ __forceinline__ float sincos_poly(double x, double x2, const SinCosPoly& p, int n) {
    if ((n & 1) == 0) {
        double x3 = x * x2;
        double s1 = __builtin_fma(x2, p.s3, p.s2);
        double x7 = x3 * x2;
        double s = __builtin_fma(x3, p.s1, x);
        return static_cast<float>(__builtin_fma(x7, s1, s));
    }
    double x4 = x2 * x2;
    double c2 = __builtin_fma(x2, p.c4, p.c3);
    double c1 = __builtin_fma(x2, p.c1, p.c0);
    double x6 = x4 * x2;
    double c = __builtin_fma(x4, p.c2, c1);
    return static_cast<float>(__builtin_fma(x6, c2, c));
}

// reduce_large for |x| >= 120 (4/pi bit table, 2^-62 pi scale).
__device__ __noinline__ double sincos_reduce_large(uint32_t xi, int* np) {
    const uint32_t* arr = &kInvPio4[(xi >> 26) & 15];
    int shift = (xi >> 23) & 7;
    xi = (xi & 0xffffff) | 0x800000;
    xi <<= shift;
    uint64_t res0 = static_cast<uint32_t>(xi * arr[0]);
    uint64_t res1 = static_cast<uint64_t>(xi) * arr[4];
    uint64_t res2 = static_cast<uint64_t>(xi) * arr[8];
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    uint64_t n = (res0 + (1ULL << 61)) >> 62;
    res0 -= n << 62;
    *np = static_cast<int>(n);
    return static_cast<double>(static_cast<int64_t>(res0)) * 0x1.921fb54442d18p-62;
}

// which = 0: sinf, 1: cosf
__device__ BDPT_NOINLINE float glibc_sincosf(float y, int which) {
    double x = y;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        double x2 = x * x;
        if (abstop12(y) < abstop12(0x1p-12f)) return which ? 1.0f : y;
        return sincos_poly(x, x2, sincos_poly_table(false), which);
    }
    int n;
    double s;
    bool neg;
    if (abstop12(y) < abstop12(120.0f)) {
        double r = x * 0x1.45f306dc9c883p+23;
        n = (static_cast<int32_t>(r) + 0x800000) >> 24;
        x = __builtin_fma(-static_cast<double>(n), 0x1.921fb54442d18p+0, x);
        s = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;
        neg = (n & 2) != 0;
    } else if (abstop12(y) < abstop12(__builtin_inff())) {
        uint32_t xi = f2u(y);
        int sign = xi >> 31;
        x = sincos_reduce_large(xi, &n);
        int q = n + sign;
        s = ((q & 3) == 1 || (q & 3) == 2) ? -1.0 : 1.0;
        neg = (q & 2) != 0;
    } else {
        return (y - y) / (y - y);
    }
    return sincos_poly(x * s, x * x, sincos_poly_table(neg), which ? (n ^ 1) : n);
}

struct SinCos {
    float s, c;
};
#ifndef BDPT_SINCOS_ATTR
#define BDPT_SINCOS_ATTR __forceinline__  // branch-free below 120: inline costs fewer registers than a call
#endif
// |y| >= 120, inf, NaN: reduce_large (never reached by the warps' angles).
__device__ __noinline__ SinCos glibc_sincosf2_large(float y) {
    if (abstop12(y) >= abstop12(__builtin_inff())) {
        const float nan = (y - y) / (y - y);
        return SinCos{nan, nan};
    }
    int n;
    const uint32_t xi = f2u(y);
    const int sign = xi >> 31;
    const double x = sincos_reduce_large(xi, &n);
    const int q = n + sign;
    const double s = ((q & 3) == 1 || (q & 3) == 2) ? -1.0 : 1.0;
    const SinCosPoly p = sincos_poly_table((q & 2) != 0);
    return SinCos{sincos_poly(x * s, x * x, p, n), sincos_poly(x * s, x * x, p, n ^ 1)};
}
// sinf(y) and cosf(y) from one range reduction, each bit-identical to the
// single calls above, without divergent branches for |y| < 120 (every angle the
// warps produce): glibc's reduce_fast path, with both polynomials evaluated once
// and assigned by the quadrant's parity. It also covers glibc's two small-
// argument paths: for |y| < pi/4 the reduction gives n = 0 and x = y exactly
// (the same polynomial call), and for |y| < 2^-12 both polynomials round to
// glibc's (y, 1.0f) (the terms past x / 1 are below half an ulp; only the sign
// of a zero sine needs the explicit select). A negated
// cosine table negates the polynomial's value exactly (fma is sign-symmetric
// under round-to-nearest), so the quadrant's sign is applied to the float.
// tools/numerics/sincos_check.hip compares it with the branchy form over every
// float with |y| < 120.
__device__ BDPT_SINCOS_ATTR SinCos glibc_sincosf2(float y) {
    if (abstop12(y) >= abstop12(120.0f)) return glibc_sincosf2_large(y);
    double x = y;
    const double r = x * 0x1.45f306dc9c883p+23;
    const int n = (static_cast<int32_t>(r) + 0x800000) >> 24;
    x = __builtin_fma(-static_cast<double>(n), 0x1.921fb54442d18p+0, x);
    const double xs = ((n & 3) == 1 || (n & 3) == 2) ? -x : x;
    const double x2 = x * x;
    const SinCosPoly p = sincos_poly_table(false);
    float sp = sincos_poly(xs, x2, p, 0);  // sine polynomial
    sp = (y == 0.f) ? y : sp;              // sinf(-0) = -0 (glibc's tiny-argument path)
    float cp = sincos_poly(xs, x2, p, 1);        // cosine polynomial
    cp = (n & 2) ? -cp : cp;
    return (n & 1) ? SinCos{cp, sp} : SinCos{sp, cp};
}

__device__ __forceinline__ float glibc_sinf(float x) { return glibc_sincosf(x, 0); }
__device__ __forceinline__ float glibc_cosf(float x) { return glibc_sincosf(x, 1); }

// ------------------------------------------------------------------ powf
__device__ __forceinline__ double d_from_u(uint64_t u) { return __longlong_as_double(static_cast<long long>(u)); }
__device__ __forceinline__ uint64_t u_from_d(double d) { return static_cast<uint64_t>(__double_as_longlong(d)); }

__device__ __forceinline__ float pf_u2f(uint32_t u) { return __uint_as_float(u); }

#ifndef BDPT_POWF_ATTR
#define BDPT_POWF_ATTR BDPT_NOINLINE
#endif
// glibc_powf and its tables: one source for the kernels and the host ingest (scene.cpp)
#define BDPT_PF_TABLE static __constant__
#define BDPT_PF_INLINE __device__ __forceinline__
#define BDPT_PF_NOINLINE __device__ __noinline__
#define BDPT_PF_ENTRY __device__ BDPT_POWF_ATTR
#include "powf_restated.inc"
#undef BDPT_PF_TABLE
#undef BDPT_PF_INLINE
#undef BDPT_PF_NOINLINE
#undef BDPT_PF_ENTRY

// x^y for a Phong lobe's value or pdf (weights only, see rcp_w): with
// BDPT_FAST_WEIGHTS exp2(y * log2(x)) on the hardware's v_log_f32 / v_exp_f32,
// else glibc's powf. The callers pass x in [0, 1] (or just above 1 by rounding)
// and y = the exponent >= 0; the relative error y * |log2 x| * ~2^-22 is largest
// where x^y is tiny. y == 0 gives 1 as powf does (also for x == 0).
#ifndef BDPT_FAST_POW
#define BDPT_FAST_POW BDPT_FAST_WEIGHTS
#endif
__device__ __forceinline__ float pow_w(float x, float y) {
#if BDPT_FAST_POW
    return y == 0.f ? 1.f : __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
#else
    return glibc_powf(x, y);
#endif
}

}  // namespace dev
}  // namespace bdpt
