// Shading a hit (shade_hit, texels, the deferred reference-leaf check), the shadow ray, and the
// BSDFs: eval, pdf and sample of every lobe, and the BSDF record of a path vertex.
// Reads BDPT_TEXTURED (texel lookup, bsdf_tex) and BDPT_GLOSSY (Mixture / Phong lobes compiled in).
#pragma once

#include "dev_traverse.hpp"
#include "dev_warp.hpp"

namespace bdpt {
namespace dev {

#if BDPT_TEXTURED
// w * y + x of core.h:582-584 (int(float) as x86's cvttss2si, clamp to [0, size - 1]).
__device__ __forceinline__ int texel_of(float sx, float sy, int tw, int th) {
    int x = x86_trunc_i32(sx * static_cast<float>(tw)), y = x86_trunc_i32(sy * static_cast<float>(th));
    x = x < 0 ? 0 : (x > tw - 1 ? tw - 1 : x);
    y = y < 0 ? 0 : (y > th - 1 ? th - 1 : y);
    return tw * y + x;
}
#endif
// AcceleratorBVH::intersect's shading of a closest hit (accel.h:133-166).
// box (optional): the record's last two vectors, loaded with the others — the
// triangle's reference leaf box, or in the textured layout the word that names it
// (leaf_box_passes).
__device__ __forceinline__ void shade_hit(const DevScene& sc, int i, float u, float v, float t, f3 dir, Hit& h,
                                          float4* box = nullptr) {
    const float4* sh = sc.shade + kShadeStride * static_cast<size_t>(i);
    if (box) box[0] = gld4(sh + kShadeBox), box[1] = gld4(sh + kShadeBox + 1);
    const f3 v0 = xyz(gld4(sh + kShadeV0)),
             v1 = xyz(gld4(sh + 3)), v2 = xyz(gld4(sh + 4));
    const float4 s0 = gld4(sh), s1 = gld4(sh + 1), s2 = gld4(sh + 2);
    const float w = 1 - u - v;
    h.p = (v0 * w + v1 * u) + v2 * v;
    h.n = normalize((xyz(s0) * w + xyz(s1) * u) + xyz(s2) * v);
    f3 fs, ft;
    make_frame(h.n, fs, ft);
    h.wo = to_local(fs, ft, h.n, -dir);
    h.dist = t;
    h.mat = __float_as_int(s0.w);
    h.shape = __float_as_int(s1.w);
#if BDPT_TEXTURED
    // BitmapTexture3f::eval (core.h:569-587): st = barycentric(st0, st1, st2, u, v) + 1
    // (math.h:20-22), st -= floor(st), x = clamp(int(st.x * w), 0, w - 1), likewise y,
    // texel w * y + x; the hit's u, v and 1 - u - v are the ones the hit point uses.
    h.tkd = h.tks = -1;
    const float4 mk_ = gld4(sc.tex_tab + 2 * static_cast<size_t>(h.mat)), ms_ = gld4(sc.tex_tab + 2 * static_cast<size_t>(h.mat) + 1);
    const int kd0 = __float_as_int(mk_.x), ks0 = __float_as_int(ms_.x);
    if (kd0 >= 0 || ks0 >= 0) {
        const float4 t0 = gld4(sh + kShadeSt), t1 = gld4(sh + kShadeSt + 1);
        float sx = (t0.x * w + t0.z * u) + t1.x * v;
        float sy = (t0.y * w + t0.w * u) + t1.y * v;
        sx = sx + 1.f, sy = sy + 1.f;
        sx = sx - __builtin_floorf(sx), sy = sy - __builtin_floorf(sy);
        if (kd0 >= 0) h.tkd = kd0 + texel_of(sx, sy, __float_as_int(mk_.y), __float_as_int(mk_.z));
        if (ks0 >= 0) h.tks = ks0 + texel_of(sx, sy, __float_as_int(ms_.y), __float_as_int(ms_.z));
    }
#endif
}

// The deferred reference-leaf check of a closest-hit walk's winner (wleaf_tests,
// `defer`): box_test on the reference leaf box of triangle `tri` with the query's
// ray, the test the walk would have made in its leaf step. box = the two vectors
// at kShadeBox of the triangle's shade record (shade_hit loads them with the rest
// of the line; shade_box loads just them): the six floats of lbox[leaf], or with
// by_id (the textured layout: those slots hold texture coordinates) the leaf id in
// the last word, and the box is read from lbox.
__device__ __forceinline__ void shade_box(const DevScene& sc, int tri, float4* box) {
    const float4* sh = sc.shade + kShadeStride * static_cast<size_t>(tri);
    box[0] = gld4(sh + kShadeBox), box[1] = gld4(sh + kShadeBox + 1);
}
template <bool COUNT>
__device__ __forceinline__ bool leaf_box_passes(const DevScene& sc, const float4* box, bool by_id, const Ray& r,
                                                const RayInv& ri, Counts& cnt) {
    if (by_id) return ref_leaf_passes<COUNT>(sc.lbox, __float_as_uint(box[1].w), r, ri, cnt);
    float tn, tf;
    uint32_t fb = 0;
    const bool pass = box_test<COUNT>(box[0].x, box[0].y, box[0].z, box[1].x, box[1].y, box[1].z, r, ri, tn, tf, fb);
    if (COUNT) cnt.c[15] += fb;
    return pass;
}

// The shadow ray of visibilityQuery (bdpt.h:498-505).
__device__ __forceinline__ Ray shadow_ray(f3 start, f3 end) {
    f3 dir = end - start;
    const float dist = sqrt_cr(dot(dir, dir));
    dir = dir / dist;
    return Ray{start, dir, kEpsilon, dist - 0.00001f};
}

// -------------------------------------------------------------------- BSDFs
__device__ __forceinline__ f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }

// BDPT_GLOSSY 0 (bdpt_kernels_ng.hip): a build for material tables whose records are all
// DiffuseBSDF, PerfectMirrorBSDF or GlassBSDF (no Mixture / Phong record, no null BSDF; the
// host checks the table, bdpt_capi.cpp). The Mixture / Phong branches, their out-of-line calls
// and powf are compiled out, and a vertex that is not delta is then diffuse without a test of
// its kind (bsdf_eval_pdfs, local_for). The remaining lobes run the same operations in the
// same order.
#ifndef BDPT_GLOSSY
#define BDPT_GLOSSY 1
#endif
// MixtureBSDF::eval == PhongBSDF::eval (mixture.h:59-75, phong.h:56-71).
// With Ks == 0 the specular term is (0 * (n + 2)) * INV_TWOPI * powf(c, n) = +0
// (powf of c in [0, 1] is finite), and val + 0 == val: skipping it is exact.
template <bool EXACT = false>
__device__ __forceinline__ f3 glossy_eval(const BsdfRecord& b, f3 wi, f3 wo) {
    f3 val = mk(0.f, 0.f, 0.f);
    if (wi.z >= 0.f && wo.z >= 0.f) {
        val = val + ld3(b.kd) * kInvPi;
        if (b.ks[0] != 0.f || b.ks[1] != 0.f || b.ks[2] != 0.f) {
            const float ex = b.exponent;
            const float c = glibc_fminf(glibc_fmaxf(dot(wi, reflect_z(wo)), 0.f), 1.f);
            val = val + ((ld3(b.ks) * (ex + 2)) * kInvTwoPi) * (EXACT ? glibc_powf(c, ex) : pow_w(c, ex));
        }
        val = val * b.scale;
        val = val * wi.z;
    }
    return val;
}

// (the Phong-bearing eval / pdf, glossy_pdf_call below, inline: measured +2 % over a call)
__device__ __forceinline__ f3 glossy_eval_call(const BsdfRecord& b, f3 wi, f3 wo) { return glossy_eval(b, wi, wo); }

// BSDF::eval. The diffuse and delta lobes are a few instructions and stay
// inline; only the Phong-bearing lobes (powf) go through a call.
__device__ __forceinline__ f3 bsdf_eval(const BsdfRecord& b, f3 wi, f3 wo) {
    const int kind = b.kind;
    if (kind == BSDF_DIFFUSE) {  // diffuse.h:35-43
        if (wi.z >= 0.f && wo.z >= 0.f) return (ld3(b.kd) * kInvPi) * wi.z;
        return mk(0.f, 0.f, 0.f);
    }
#if BDPT_GLOSSY
    if (kind == BSDF_MIXTURE || kind == BSDF_PHONG) return glossy_eval_call(b, wi, wo);
#endif
    return mk(0.f, 0.f, 0.f);  // delta lobes (perfectmirror.h:41-47, glass.h:55-59)
}

template <bool EXACT = false>
__device__ __forceinline__ float phong_part_pdf(const BsdfRecord& b, f3 wi, f3 wo) {
    f3 rs, rt;
    const f3 rn = reflect_z(wo);
    make_frame(rn, rs, rt);
    return phong_lobe_pdf<EXACT>(to_local(rs, rt, rn, wi), b.exponent);
}

// With specw == 0, pdfPhong * 0 = +0 (pdfPhong is finite and >= 0) and
// 0 + pdfDiffuse * (1 - 0) == pdfDiffuse: skipping the Phong lobe is exact.
__device__ __forceinline__ float glossy_pdf_call(const BsdfRecord& b, f3 wi, f3 wo) {
    if (b.kind == BSDF_MIXTURE) {  // mixture.h:78-100
        const float pd = cosine_hemisphere_pdf(wi);
        const float pp = phong_part_pdf(b, wi, wo);
        return (pp * b.specw) + (pd * (1.f - b.specw));
    }
    return phong_part_pdf(b, wi, wo);  // phong.h:73-83
}
__device__ __forceinline__ float bsdf_pdf(const BsdfRecord& b, f3 wi, f3 wo) {
    const int kind = b.kind;
#if BDPT_GLOSSY
    if (kind == BSDF_DIFFUSE || (kind == BSDF_MIXTURE && b.specw == 0.f))  // diffuse.h:45-50
        return cosine_hemisphere_pdf(wi);
    if (kind == BSDF_MIXTURE || kind == BSDF_PHONG) return glossy_pdf_call(b, wi, wo);
#else
    if (kind == BSDF_DIFFUSE) return cosine_hemisphere_pdf(wi);  // diffuse.h:45-50
#endif
    return 0.f;
}

// eval(wi, wo), pdf(wi, wo) and pdf(wo, wi) of one BSDF — what every
// connection needs at each end (bdpt.h:374-483) — with ONE powf for the Phong
// lobe: the cosine of eval (dot(wi, reflect(wo)), clamped to [0, 1]) and the
// lobe's local z in both pdfs (Frame(reflect(wo)).toLocal(wi).z = dot(wi,
// reflect(wo)), and dot(wo, reflect(wi)) has the same products in the same
// order) are one value z. eval takes powf(clamp(z)), the pdfs powf(z) for
// z >= 0: the same call unless z > 1, where eval's powf(1, n) is exactly 1.
// Each output is bit-identical to bsdf_eval / bsdf_pdf above.
// Its callers connect vertices that are not delta (connectToLight, connectToCamera,
// connectVertices); in a BDPT_GLOSSY 0 build those are diffuse, so the kind is not read.
struct EvalPdfs {
    f3 f;
    float fwd, rev;  // pdf(wi, wo), pdf(wo, wi)
};
__device__ __forceinline__ EvalPdfs bsdf_eval_pdfs(const BsdfRecord& b, f3 wi, f3 wo) {
#if !BDPT_GLOSSY
    EvalPdfs r{mk(0.f, 0.f, 0.f), 0.f, 0.f};
    if (wi.z >= 0.f && wo.z >= 0.f) r.f = (ld3(b.kd) * kInvPi) * wi.z;
    r.fwd = cosine_hemisphere_pdf(wi);
    r.rev = cosine_hemisphere_pdf(wo);
    return r;
#else
    EvalPdfs r{mk(0.f, 0.f, 0.f), 0.f, 0.f};
    const int kind = b.kind;
    if (kind == BSDF_DIFFUSE) {
        if (wi.z >= 0.f && wo.z >= 0.f) r.f = (ld3(b.kd) * kInvPi) * wi.z;
        r.fwd = cosine_hemisphere_pdf(wi);
        r.rev = cosine_hemisphere_pdf(wo);
        return r;
    }
    if (kind != BSDF_MIXTURE && kind != BSDF_PHONG) return r;  // delta lobes
    const float ex = b.exponent;
    const float z = dot(wi, reflect_z(wo));
    const bool eval_on = wi.z >= 0.f && wo.z >= 0.f;
    const bool ks_on = b.ks[0] != 0.f || b.ks[1] != 0.f || b.ks[2] != 0.f;
    const bool lobe_pdf = kind == BSDF_PHONG || b.specw != 0.f;
    float pw = 0.f;
    if ((eval_on && ks_on) || (lobe_pdf && z >= 0.f))
        pw = pow_w(z > 1.f ? z : glibc_fminf(glibc_fmaxf(z, 0.f), 1.f), ex);
    if (eval_on) {  // glossy_eval
        f3 val = mk(0.f, 0.f, 0.f);
        val = val + ld3(b.kd) * kInvPi;
        if (ks_on) val = val + ((ld3(b.ks) * (ex + 2)) * kInvTwoPi) * (z > 1.f ? 1.f : pw);
        val = val * b.scale;
        r.f = val * wi.z;
    }
    const float pp = z >= 0.f ? (ex + 2) * kInvTwoPi * pw : 0.f;  // phong_lobe_pdf
    if (kind == BSDF_PHONG) {
        r.fwd = r.rev = pp;
    } else if (b.specw == 0.f) {
        r.fwd = cosine_hemisphere_pdf(wi);
        r.rev = cosine_hemisphere_pdf(wo);
    } else {
        r.fwd = (pp * b.specw) + (cosine_hemisphere_pdf(wi) * (1.f - b.specw));
        r.rev = (pp * b.specw) + (cosine_hemisphere_pdf(wo) * (1.f - b.specw));
    }
    return r;
#endif
}

// glass.h:40-53
__device__ __forceinline__ float fresnel_dielectric(float eta_i, float eta_t, float cos_i, float cos_t) {
    const float eta = div_cr(eta_i, eta_t);
    const float sin2_t = eta * eta * (glibc_fmaxf(0.f, 1.f - cos_i * cos_i));
    if (sin2_t >= 1.f) return 1.f;
    const float rpar = div_cr((eta_t * cos_i) - (eta_i * cos_t), (eta_t * cos_i) + (eta_i * cos_t));
    const float rper = div_cr((eta_i * cos_i) - (eta_t * cos_t), (eta_i * cos_i) + (eta_t * cos_t));
    return (rpar * rpar + rper * rper) * 0.5f;
}

// GlassBSDF::sample (glass.h:67-108: pdf 1, no eta^2 scaling).
__device__ __forceinline__ f3 glass_sample(const BsdfRecord& b, f3 wo, F2 u, f3& wi, float& pdf) {
    pdf = 1.f;
    const bool entering = wo.z > 0.f;
    float eta_i = 1.f, eta_t = b.ior;
    if (!entering) {
        const float q = eta_i;
        eta_i = eta_t;
        eta_t = q;
    }
    const float eta = div_cr(eta_i, eta_t);
    const float sin2_i = glibc_fmaxf(0.f, 1.f - wo.z * wo.z);
    const float sin2_t = eta * eta * sin2_i;
    float cos_t = sqrt_cr(glibc_fmaxf(0.f, 1.f - sin2_t));
    cos_t = entering ? -cos_t : cos_t;
    const float fr = fresnel_dielectric(eta_i, eta_t, fabsf(wo.z), fabsf(cos_t));
    if (u.x < fr) {
        wi = reflect_z(wo);
        return mk(1.f, 1.f, 1.f);
    }
    wi = mk(eta * -wo.x, eta * -wo.y, cos_t);
    return ld3(b.tf);
}

// BSDF::sample: sets wi, returns f*cos, writes the solid-angle pdf.
__device__ __forceinline__ f3 bsdf_sample_body(const BsdfRecord& b, f3 wo, F2 u, f3& wi, float& pdf) {
    switch (b.kind) {
        case BSDF_MIRROR:  // perfectmirror.h:49-59
            pdf = 1.f;
            wi = reflect_z(wo);
            return mk(1.f, 1.f, 1.f);
        case BSDF_GLASS:
            return glass_sample(b, wo, u, wi, pdf);
        // The sampled value steers the walk (ContinuePathRandomWalk ends it on f == 0,
        // bdpt.h:253), so the Phong powers here stay glibc's powf in every build: the
        // fast-weight pow_w flushes results below 2^-126 to 0, which for a
        // lobe with Kd = 0 would end a path the reference continues.
#if BDPT_GLOSSY
        case BSDF_MIXTURE: {  // mixture.h:102-151
            f3 val;
            if (u.x < b.specw) {
                const F2 ns{div_cr(u.x, b.specw), u.y};
                f3 rs, rt;
                const f3 rn = reflect_z(wo);
                make_frame(rn, rs, rt);
                wi = to_world(rs, rt, rn, phong_lobe(ns, b.exponent));
            } else {
                const F2 ns{div_cr(u.x - b.specw, 1.f - b.specw), u.y};
                wi = cosine_hemisphere(ns);
            }
            val = glossy_eval<true>(b, wi, wo);
            if (b.specw == 0.f) pdf = cosine_hemisphere_pdf(wi);  // bsdf_pdf's exact shortcut
            else pdf = (phong_part_pdf<true>(b, wi, wo) * b.specw) + (cosine_hemisphere_pdf(wi) * (1.f - b.specw));
            return val;
        }
        case BSDF_PHONG: {  // phong.h:85-100
            f3 rs, rt;
            const f3 rn = reflect_z(wo);
            make_frame(rn, rs, rt);
            const f3 ls = phong_lobe(u, b.exponent);
            pdf = phong_lobe_pdf<true>(ls, b.exponent);
            wi = to_world(rs, rt, rn, ls);
            return glossy_eval<true>(b, wi, wo);
        }
#endif
        default:  // null BSDF (illum 5): the reference dereferences nullptr
            pdf = 0.f;
            wi = mk(0.f, 0.f, 0.f);
            return mk(0.f, 0.f, 0.f);
    }
}
// The non-diffuse BSDF samplers run out of line. The call returns everything by value
// (in VGPRs): with reference outputs the caller's wi / pdf went through scratch around
// every call.
struct BsdfSample {
    f3 f, wi;
    float pdf;
};
__device__ BDPT_NOINLINE BsdfSample bsdf_sample_call(const BsdfRecord& b, f3 wo, F2 u) {
    BsdfSample s;
    s.f = bsdf_sample_body(b, wo, u, s.wi, s.pdf);
    return s;
}
__device__ __forceinline__ f3 bsdf_sample_call(const BsdfRecord& b, f3 wo, F2 u, f3& wi, float& pdf) {
    const BsdfSample s = bsdf_sample_call(b, wo, u);
    wi = s.wi;
    pdf = s.pdf;
    return s.f;
}
__device__ __forceinline__ f3 bsdf_sample(const BsdfRecord& b, f3 wo, F2 u, f3& wi, float& pdf) {
    if (b.kind == BSDF_DIFFUSE) {  // diffuse.h:52-61
        wi = cosine_hemisphere(u);
        pdf = cosine_hemisphere_pdf(wi);
        return bsdf_eval(b, wi, wo);
    }
    if (b.kind == BSDF_GLASS) return glass_sample(b, wo, u, wi, pdf);
    if (b.kind == BSDF_MIRROR) {  // perfectmirror.h:49-59
        pdf = 1.f;
        wi = reflect_z(wo);
        return mk(1.f, 1.f, 1.f);
    }
#if BDPT_GLOSSY
    return bsdf_sample_call(b, wo, u, wi, pdf);
#else
    pdf = 0.f;  // (no other kind in this build's tables; bsdf_sample_body's default)
    wi = mk(0.f, 0.f, 0.f);
    return mk(0.f, 0.f, 0.f);
#endif
}

__device__ __forceinline__ bool is_delta(const BsdfRecord& b) { return (b.type & kTypeDelta) != 0; }

// The BSDF of a path vertex. Textured builds: a copy of the material's record with Kd / Ks
// replaced by the vertex's texels (diffuse.h:40, mixture.h:66-70, phong.h:66-70 evaluate the
// Texture<v3f> at the hit), fetched here, where eval / sample need them; a vertex carries
// the two texel indices, not the reflectances.
#if BDPT_TEXTURED
__device__ __forceinline__ BsdfRecord bsdf_tex(const DevScene& sc, int mat, int tkd, int tks) {
    BsdfRecord b = bsdf_of(sc, mat);
    if (tkd >= 0) {
        const float4 t = gld4(sc.tex_tab + tkd);
        b.kd[0] = t.x, b.kd[1] = t.y, b.kd[2] = t.z;
    }
    if (tks >= 0) {
        const float4 t = gld4(sc.tex_tab + tks);
        b.ks[0] = t.x, b.ks[1] = t.y, b.ks[2] = t.z;
    }
    return b;
}
#define BDPT_VERTEX_BSDF(NAME, SC, MAT, TKD, TKS) const BsdfRecord NAME = bsdf_tex(SC, MAT, TKD, TKS)
#else
#define BDPT_VERTEX_BSDF(NAME, SC, MAT, TKD, TKS) const BsdfRecord& NAME = bsdf_of(SC, MAT)
#endif

// The direction v in the shading frame of normal n, for evaluating BSDF b:
// DiffuseBSDF's eval and pdf read only the z component, dot(v, n) (to_local),
// so a diffuse lane skips Frame(n) (a sqrt, a division and a branch); the x, y
// it leaves at 0 are never read. Called for
// the ends of a connection, which are not delta: diffuse in a BDPT_GLOSSY 0 build.
__device__ __forceinline__ f3 local_for(const BsdfRecord& b, f3 n, f3 v) {
#if !BDPT_GLOSSY
    return mk(0.f, 0.f, dot(v, n));
#else
    if (b.kind == BSDF_DIFFUSE) return mk(0.f, 0.f, dot(v, n));
    return local_at(n, v);
#endif
}

}  // namespace dev
}  // namespace bdpt
