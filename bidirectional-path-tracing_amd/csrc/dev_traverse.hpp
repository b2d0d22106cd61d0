// BVH traversal: slab and triangle tests, the per-lane stack, counters, the reference's binary
// walk, the 4-wide node and leaf steps with the root in LDS, and the whole-wave cooperative walks.
// Reads BDPT_LEAF_GROUP and BDPT_WLEAF_GROUP (triangles fetched per leaf round trip).
#pragma once

#include "dev_scene.hpp"

namespace bdpt {
namespace dev {

// ---------------------------------------------------------------- traversal
// BBox::intersect (bvh.h:33-69): the reference's slab test, bit for bit (true
// divisions, same swaps and comparisons), also returning the clipped interval.
__device__ __forceinline__ bool slab(float lx, float ly, float lz, float hx, float hy, float hz, const Ray& r,
                                     float& tn, float& tf) {
    float tmin = (lx - r.o.x) / r.d.x, tmax = (hx - r.o.x) / r.d.x;
    if (tmin > tmax) { float q = tmin; tmin = tmax; tmax = q; }
    float tymin = (ly - r.o.y) / r.d.y, tymax = (hy - r.o.y) / r.d.y;
    if (tymin > tymax) { float q = tymin; tymin = tymax; tymax = q; }
    if ((tmin > tymax) || (tymin > tmax)) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (lz - r.o.z) / r.d.z, tzmax = (hz - r.o.z) / r.d.z;
    if (tzmin > tzmax) { float q = tzmin; tzmin = tzmax; tzmax = q; }
    if ((tmin > tzmax) || (tzmin > tmax)) return false;
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    tn = tmin;
    tf = tmax;
    return true;
}

// Fast form of the same decision. The reference's test (after its swaps every
// per-axis interval is [lo_i, hi_i]) hits exactly when max_i lo_i <= min_j hi_j.
// Here t = (l - o) * RN(1/d) differs from the reference's RN((l - o) / d) by at
// most ~1.8e-7 |t| (three roundings instead of one), so tf - tn differs from the
// reference's by < 3e-7 (|tn| + |tf|). Decisions within a slack of
// 1e-6 (|tn| + |tf|) + 1e-30 of the boundary defer to slab() above, so the
// hit / miss outcome is always the reference's. Rays whose reciprocal
// direction or origin is not finite (where 0 * inf = NaN could arise) take
// slab() for every box (RayInv::fast == false).
constexpr float kCullNear = 5e-4f;
// The near cull assumes Moller-Trumbore puts a hit where the ray meets its
// triangle. For a ray nearly parallel to a triangle's plane whose origin lies on
// that plane (a grazing ray leaving a surface) the computed t, u, v are rounding
// noise the reference still accepts (t > 1e-3), so such queries walk without the
// near cull: every query leaving a surface (a path vertex or the emitter) at
// |cos| < kGrazeCos to its triangle's plane. Below it the
// t error of a coplanar triangle, ~1.2e-7 |o - v0| / (|cos| sin(corner)), can
// pass 1e-3 only for triangles with a corner under ~0.35 degrees.
constexpr float kGrazeCos = 0.02f;
// The rule is about the origin triangle's geometric plane; the path only holds
// the interpolated shading normal n_s, so each triangle carries a graze code (top
// byte of its shading record's shape word, bdpt_capi.cpp graze_code): n_s lies
// within code / 64 of the geometric normal's direction, and |dot(d, n_s)| <
// kGrazeCos + code / 64 covers every |dot(d, n_g)| < kGrazeCos. Code 0 (flat
// triangles: n_s is n_g) leaves the plain test.
__device__ __forceinline__ int shape_id(int packed) { return packed & 0xffffff; }
__device__ __forceinline__ float graze_threshold(int packed) {
    return kGrazeCos + static_cast<float>(static_cast<uint32_t>(packed) >> 24) * 0.015625f;
}
__device__ __forceinline__ bool graze_exempt(f3 d, f3 n, int packed) { return fabsf(dot(d, n)) < graze_threshold(packed); }
enum : int { kSlabMiss = 0, kSlabHit = 1, kSlabAmbiguous = 2 };
struct RayInv {
    f3 inv;
    bool fast;
    float near;  // boxes left before t = near are culled (kCullNear, or -inf: no near cull, see cull_near_for)
};
__device__ __forceinline__ bool far_origin(const DevScene& sc, f3 o) {
    return !(o.x >= sc.near_lo[0] && o.x <= sc.near_hi[0] && o.y >= sc.near_lo[1] && o.y <= sc.near_hi[1] &&
             o.z >= sc.near_lo[2] && o.z <= sc.near_hi[2]);
}
constexpr float kNoCullNear = -__builtin_huge_valf();
__device__ __forceinline__ RayInv ray_inv(const Ray& r, float near);
__device__ __forceinline__ RayInv ray_inv(const Ray& r, float near) {
    RayInv ri;
    ri.near = near;
    ri.inv = mk(rcp_cr(r.d.x), rcp_cr(r.d.y), rcp_cr(r.d.z));
    // slab_fma's o inv must be finite too
    const float probe = (ri.inv.x + ri.inv.y + ri.inv.z) * 0.f + ((r.o.x + r.o.y + r.o.z) * 0.f) +
                        ((r.o.x * ri.inv.x + r.o.y * ri.inv.y + r.o.z * ri.inv.z) * 0.f);
    ri.fast = (probe == 0.f);  // false iff some component is +-inf or NaN
    return ri;
}
__device__ __forceinline__ int slab_planes(float x0, float x1, float y0, float y1, float z0, float z1, float& tn,
                                           float& tf) {
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    const float d = tf - tn, s = fmaf(fabsf(tn) + fabsf(tf), 1e-6f, 1e-30f);
    return d > s ? kSlabHit : (d < -s ? kSlabMiss : kSlabAmbiguous);  // inf operands: ambiguous
}
__device__ __forceinline__ int slab_fast(float lx, float ly, float lz, float hx, float hy, float hz, f3 o, f3 inv,
                                         float& tn, float& tf) {
    const float x0 = (lx - o.x) * inv.x, x1 = (hx - o.x) * inv.x;
    const float y0 = (ly - o.y) * inv.y, y1 = (hy - o.y) * inv.y;
    const float z0 = (lz - o.z) * inv.z, z1 = (hz - o.z) * inv.z;
    return slab_planes(x0, x1, y0, y1, z0, z1, tn, tf);
}
// The slack-free interior test's plane distances as one fma each,
// fma(l, inv, -RN(o inv)) instead of a subtraction and a product (24 VALU
// instead of 48 per 4-wide node; Caustic +1.1 %, HardLight +1.0 %, synth1m
// +1.3 %). Against the exact (l - o) / d the error is at most
// 2^-23 |t| + 2^-24 |o_i inv_i| per plane, i.e. 2^-23 |l_i - o_i| + 2^-24 |o_i| in
// scene units along axis i: node_slack_needed admits it only while every origin
// and the scene box lie within kFmaCoordDiags diagonals of 0 (bdpt_capi.cpp), where
// it stays below slab_fast's own bound and inside the boxes' padding.
__device__ __forceinline__ f3 slab_fma_origin(f3 o, f3 inv) {
    f3 oi = mk(-(o.x * inv.x), -(o.y * inv.y), -(o.z * inv.z));
    return oi;
}
__device__ __forceinline__ void slab_fma(float lx, float ly, float lz, float hx, float hy, float hz, f3 oi, f3 inv,
                                         float& tn, float& tf) {
    const float x0 = fmaf(lx, inv.x, oi.x), x1 = fmaf(hx, inv.x, oi.x);
    const float y0 = fmaf(ly, inv.y, oi.y), y1 = fmaf(hy, inv.y, oi.y);
    const float z0 = fmaf(lz, inv.z, oi.z), z1 = fmaf(hz, inv.z, oi.z);
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
}

__device__ __forceinline__ int cross_le(float a, float b) {  // a <= b with the same slack
    const float d = b - a, s = fmaf(fabsf(a) + fabsf(b), 1e-6f, 1e-30f);
    return d > s ? kSlabHit : (d < -s ? kSlabMiss : kSlabAmbiguous);
}
// Second chance for an ambiguous max-lo vs min-hi decision: the reference's
// test is the six cross pairs lo_i <= hi_j (i != j) — the pair of a flat
// (zero-thickness) box axis, tn == tf on a planar wall, never enters it.
__device__ __forceinline__ int slab_cross(float lx, float ly, float lz, float hx, float hy, float hz, f3 o,
                                          f3 inv) {
    const float x0 = (lx - o.x) * inv.x, x1 = (hx - o.x) * inv.x;
    const float y0 = (ly - o.y) * inv.y, y1 = (hy - o.y) * inv.y;
    const float z0 = (lz - o.z) * inv.z, z1 = (hz - o.z) * inv.z;
    const float lox = fminf(x0, x1), hix = fmaxf(x0, x1);
    const float loy = fminf(y0, y1), hiy = fmaxf(y0, y1);
    const float loz = fminf(z0, z1), hiz = fmaxf(z0, z1);
    const int a = cross_le(lox, fminf(hiy, hiz)), b = cross_le(loy, fminf(hix, hiz)),
              c = cross_le(loz, fminf(hix, hiy));
    if (a == kSlabMiss || b == kSlabMiss || c == kSlabMiss) return kSlabMiss;
    return (a & b & c) == kSlabHit ? kSlabHit : kSlabAmbiguous;
}

template <bool COUNT>
__device__ __forceinline__ bool box_test(float lx, float ly, float lz, float hx, float hy, float hz, const Ray& r,
                                         const RayInv& ri, float& tn, float& tf, uint32_t& fallbacks) {
    if (ri.fast) {
        int f = slab_fast(lx, ly, lz, hx, hy, hz, r.o, ri.inv, tn, tf);
        if (f == kSlabAmbiguous) f = slab_cross(lx, ly, lz, hx, hy, hz, r.o, ri.inv);
        if (f != kSlabAmbiguous) return f == kSlabHit;
    }
    if (COUNT) fallbacks++;
    return slab(lx, ly, lz, hx, hy, hz, r, tn, tf);
}

// rayTriangleIntersect (core.h:379-400) + accel.h:43's t > 1e-3, on the
// triangle's v0 and edges (e1 = v1 - v0, e2 = v2 - v0 rounded as the
// reference rounds them).
__device__ __forceinline__ bool tri_test_raw(f3 v0, f3 e1, f3 e2, const Ray& r, float& t, float& u, float& v) {
    const f3 pvec = cross(r.d, e2);
    const float det = dot(e1, pvec);
    if (fabsf(det) < kEpsilon) return false;
    const float invDet = rcp_det(det);  // |det| >= kEpsilon here
    const f3 tvec = r.o - v0;
    u = dot(tvec, pvec) * invDet;
    if (u < 0.f || u > 1.f) return false;
    const f3 qvec = cross(tvec, e1);
    v = dot(r.d, qvec) * invDet;
    if (v < 0.f || u + v > 1.f) return false;
    t = dot(e2, qvec) * invDet;
    return true;
}
__device__ __forceinline__ bool tri_test_edges(f3 v0, f3 e1, f3 e2, const Ray& r, float& t, float& u, float& v) {
    return tri_test_raw(v0, e1, e2, r, t, u, v) && t >= kTriMinT;
}
__device__ __forceinline__ bool tri_test(const float4* __restrict__ tri, uint32_t i, const Ray& r, float& t, float& u,
                                         float& v) {
    return tri_test_edges(xyz(gld4(tri + 3 * i)), xyz(gld4(tri + 3 * i + 1)), xyz(gld4(tri + 3 * i + 2)), r, t, u, v);
}

// Traversal stack of (link, t_near) entries: the first kLdsStack entries of a
// lane live in LDS (entry k of thread x at lds[k * stride + x]: 8-byte lanes,
// conflict-free), deeper ones spill to a per-lane HBM column (rare; the host
// sizes it to the scene's worst case).
constexpr int kLdsStack = 7;  // entries per lane in LDS; 7 leaves the LDS room for the root nodes
constexpr uint32_t kEmptyLinkDev = 0xffffffffu;  // unused 4-wide child slot
// The accesses name their address space (LDS: ds_*, HBM: global_*): through
// the generic pointers the compiler merged the two branches into one FLAT
// access, and every FLAT load waits for vmcnt(0) and lgkmcnt(0) together —
// each pop then also waited for all of the wave's outstanding global loads.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2 lds_uint2;
typedef __attribute__((address_space(1))) u32x2 gbl_uint2;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(1))) uint32_t gbl_u32;
typedef __attribute__((address_space(1))) int32_t gbl_i32;
// threadIdx.x, re-read at each use (opaque to the optimiser): per-lane
// addresses derived from it at their use are not held in registers across the
// persistent loop (only threadIdx.x itself is).
__device__ __forceinline__ uint32_t opaque_tid() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

struct Stack {
    uint2* lds;
    int stride;
    int nlds;    // entries held in LDS
    uint2* gbl;  // entry k >= nlds at gbl[(k - nlds) * nslots + slot] (the frame kernels: the slot's block, nslots 1)
    uint32_t nslots, slot;
    bool tid_rel = false;  // lds and slot are the block's bases; the lane adds threadIdx.x at each access
    __device__ __forceinline__ uint32_t lane_off() const { return tid_rel ? opaque_tid() : 0u; }
    __device__ __forceinline__ void put(int k, uint32_t link, float tn) const {
        const u32x2 e = {link, __float_as_uint(tn)};
        const uint32_t t = lane_off();
        if (k < nlds) ((lds_uint2*)lds)[t + k * stride] = e;
        else ((gbl_uint2*)gbl)[static_cast<size_t>(k - nlds) * nslots + slot + t] = e;
    }
    __device__ __forceinline__ uint2 get(int k) const {
        const uint32_t t = lane_off();
        const u32x2 e = k < nlds ? ((const lds_uint2*)lds)[t + k * stride]
                                 : ((const gbl_uint2*)gbl)[static_cast<size_t>(k - nlds) * nslots + slot + t];
        return make_uint2(e.x, e.y);
    }
};

// Conservative distance culling. The reference never culls by distance
// (bbhits stay 0, bvh.h:265-337): its result is the minimum-t triangle among
// ALL reachable leaves, first-found (= lowest leaf index) on ties. Boxes
// entered beyond best + margin, or exited before t = 5e-4, cannot hold a
// triangle that changes that result.
__device__ __forceinline__ float cull_far(float best) {
    return fmaf(fabsf(best), 1e-3f, best) + 1e-4f;
}
// (A walk in progress passes ts.best_t for either kind of query: an occlusion
// query's best_t stays its max_t — trav_begin; wleaf_tests returns at its first
// hit without lowering it.)

struct Counts {
    uint32_t c[kCounters];
    uint32_t m[3];  // maxima (counting pass): light-subpath depth, eye-subpath depth, queries per sample
    // connection-task histogram of the shading steps (frame kernels' counting pass): the
    // tasks a wave holds when it shades — connectVertices still to run (nl - ci at A_CONN),
    // connectToLight + all connections of a new eye vertex, connectToCamera of a new light
    // vertex — summed over steps, the steps, steps with >= 32 and >= 64 tasks. The
    // BDPT_HELP builds count their task rings here instead: tasks pushed, pushes
    // refused (ring full: the owner traces the ray), claim rounds, tasks claimed.
    uint32_t q[4];
    uint32_t t_step;  // this lane's tasks in the current shading step
};
// [5..8] Russian-roulette build: the most walks past BDPT_EXPRESS_DEPTH bounces one wave
// held at once, and the express-mode loop iterations of waves holding 1, 2..BDPT_COOP_MAX,
// more such walks
enum : int { kDiagStart = 0, kDiagLastClaim = 1, kDiagEnd = 2, kDiagErrors = 3, kDiagParked = 4, kDiagLongMax = 5,
             kDiagExpress1 = 6, kDiagExpressCoop = 7, kDiagExpressMore = 8,
             // counting pass, BDPT_LEAF_DEFER builds: checked re-walks begun, closest hits applied
             // (bdpt_path.hpp closest_apply)
             kDiagLeafRewalks = 9, kDiagLeafHits = 10, kDiagWords = 11 };

// Set bits of a wave mask as an int. (HIP's __popcll is typed unsigned long long
// here: mixed with int in min / max it selected the double overloads, and the
// refill and shade-threshold arithmetic ran in f64.)
__device__ __forceinline__ int popc64(uint64_t m) { return __builtin_popcountll(m); }
// The lane's rank among the set lanes of m below it (mbcnt: no per-lane mask
// held across the loop).
__device__ __forceinline__ int lanes_below(uint64_t m) {
    return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
}

// Lane i's value in every lane, for a wave-uniform i: v_readlane (a scalar
// result, a few cycles) where __shfl's ds_bpermute takes an LDS round trip.
// The value is the lane's register whether or not it is active.
__device__ __forceinline__ int lane_val(int x, int i) { return __builtin_amdgcn_readlane(x, i); }
__device__ __forceinline__ float lane_val(float x, int i) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i));
}

// SIMD-efficiency probe: true on the lowest active lane of the wave only.
__device__ __forceinline__ bool first_active_lane() {
    return (__lane_id()) == static_cast<unsigned>(__ffsll(static_cast<unsigned long long>(__ballot(1))) - 1);
}

// Triangle tests of one reference leaf (bvh.h:291-309). Closest: keeps the
// minimum t, ties to the lowest index (the reference's strict `<` in its
// left-first DFS = leaf order). Any: true on a hit with t <= max_t — the
// reference's occlusion query returns at a hit inside [min_t, max_t] and
// otherwise reports any hit closer than max_t it kept (bvh.h:298-305, :350).
// The triangles are fetched BDPT_LEAF_GROUP at a time with all their loads in
// flight together (one memory round trip per group instead of two per
// triangle); indices past the leaf's count are clamped and their results unused.
#ifndef BDPT_LEAF_GROUP
#define BDPT_LEAF_GROUP 1
#endif
template <bool COUNT>
__device__ __forceinline__ bool leaf_tests(const float4* __restrict__ tri, uint32_t link, const Ray& r, bool any, float& best_t,
                                           int& best, float& best_u, float& best_v, uint32_t& tri_count) {
    constexpr uint32_t G = BDPT_LEAF_GROUP;
    const uint32_t start = (link >> 3) & 0x0fffffffu, count = link & 7u;
    for (uint32_t k0 = 0; k0 < count; k0 += G) {
        float4 q[G][3];
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            const uint32_t i = start + (k0 + g < count ? k0 + g : count - 1);
            q[g][0] = gld4(tri + 3 * i), q[g][1] = gld4(tri + 3 * i + 1), q[g][2] = gld4(tri + 3 * i + 2);
        }
#pragma unroll
        for (uint32_t g = 0; g < G; g++)
#pragma unroll
            for (int j = 0; j < 3; j++) asm volatile("" ::"v"(q[g][j].x), "v"(q[g][j].y), "v"(q[g][j].z));
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            const uint32_t k = k0 + g;
            if (k >= count) break;
            const uint32_t i = start + k;
            float t, u, v;
            if (COUNT) tri_count++;
            if (tri_test_edges(xyz(q[g][0]), xyz(q[g][1]), xyz(q[g][2]), r, t, u, v)) {
                if (any) {
                    if (t <= r.max_t) {
                        best = 1;
                        return true;
                    }
                } else if (t < best_t || (t == best_t && best >= 0 && static_cast<int>(i) < best)) {
                    best_t = t, best = static_cast<int>(i), best_u = u, best_v = v;
                }
            }
        }
    }
    return false;
}

struct TravResult {
    int best;
    float t, u, v;
    uint32_t nodes, tris, exact;  // counting pass only
};

// BVH::getIntersection (bvh.h:259-352) over the reference's own binary tree:
// every box decided exactly as the reference decides it. Used for rays the
// 4-wide hierarchy cannot serve (zero / non-finite reciprocal direction, where
// the slab test is not monotone) and for BDPT_FLAG_FULL_TRAVERSAL (cull =
// false: every box the reference visits). Out of line, arguments by value
// (nothing of the caller's lives in scratch).
template <bool COUNT, typename StackT>
__device__ BDPT_NOINLINE TravResult traverse_binary(const DevScene& sc, Ray r, bool any, bool cull, StackT stk) {
    TravResult res{-1, r.max_t, 0.f, 0.f, 0u, 0u, 0u};
    uint32_t link = sc.root_link;
    int sp = 0;
    for (;;) {
        if (link & kLeafBit) {
            if (leaf_tests<COUNT>(sc.tri, link, r, any, res.t, res.best, res.u, res.v, res.tris)) break;
        } else {
            if (COUNT) res.nodes++, res.exact += 2;
            const float4* nd = sc.nodes + 4 * static_cast<size_t>(link);
            const float4 q0 = gld4(nd), q1 = gld4(nd + 1), q2 = gld4(nd + 2), q3 = gld4(nd + 3);
            float tn0, tf0, tn1, tf1;
            bool h0 = slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r, tn0, tf0);
            bool h1 = slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r, tn1, tf1);
            const uint32_t l0 = __float_as_uint(q3.x), l1 = __float_as_uint(q3.y);
            if (cull) {
                const float far = cull_far(any ? r.max_t : res.t);
                h0 = h0 && !(tn0 > far) && !(tf0 < kCullNear);
                h1 = h1 && !(tn1 > far) && !(tf1 < kCullNear);
            }
            if (h0 && h1) {
                stk.put(sp++, l1, 0.f);
                link = l0;
                continue;
            }
            if (h0) { link = l0; continue; }
            if (h1) { link = l1; continue; }
        }
        if (sp == 0) break;
        link = stk.get(--sp).x;
    }
    return res;
}

// Closest-hit / occlusion query over the 4-wide hierarchy (wide_bvh.hpp),
// written as a resumable step so persistent kernels can refill finished lanes.
// Every child box is tested conservatively (an ambiguous fast test counts as a
// hit): the boxes bound the (padded) triangles below them. Whether a triangle
// is a candidate of the reference's search at all is decided per triangle hit,
// by the exact test of its reference leaf box (wleaf_tests). Children are
// visited near-first; stacked entries carry their entry distance and are
// dropped on pop once a closer hit exists.
// The scene pointers a walk needs, copied once per query into registers: the
// DevScene lives in a parameter block in global memory, and reading a field
// through it inside the node loop would put a dependent load in front of
// every node fetch (the compiler must assume the block may change).
struct TravScene {
    const float4* __restrict__ wtri;
    const float4* __restrict__ lbox;
    const float4* __restrict__ wnodes;  // the records the walk reads
    uint32_t wroot_link;
    uint32_t node_slack;  // 0: interior boxes tested without the ambiguity slack (DevScene::node_slack)
};
__device__ __forceinline__ const float4* uniform_ptr(const float4* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v & 0xffffffffu)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32)));
    return reinterpret_cast<const float4*>((static_cast<uint64_t>(hi) << 32) | lo);
}
__device__ __forceinline__ TravScene trav_scene(const DevScene& sc) {
    return TravScene{uniform_ptr(sc.wtri), uniform_ptr(sc.lbox), uniform_ptr(sc.wnodes),
                     static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(sc.wroot_link))),
                     static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(sc.node_slack)))};
}

// Triangle tests of one traversal leaf (wtri records). A hit is a candidate of
// the reference's search iff the triangle's reference leaf box passes
// BBox::intersect (bvh.h:33-69; wide_bvh.hpp) — checked exactly (fast test,
// cross pairs, the reference's divisions) and only for a hit that would become
// the closest (minimum t, ties to the lowest reference index = the reference's
// strict `<` in its left-first DFS) or that ends an occlusion query (t <= max_t,
// see leaf_tests). A closest-hit walk with `defer` set (BDPT_LEAF_DEFER, the frame
// kernels without Russian roulette) accepts on the comparison alone: only the
// walk's final winner is checked, once, where its result is applied
// (leaf_box_passes, bdpt_path.hpp closest_apply).
template <bool COUNT>
__device__ __forceinline__ bool ref_leaf_passes(const float4* __restrict__ lbox, uint32_t leaf, const Ray& r,
                                                const RayInv& ri, Counts& cnt) {
    const float4 lo = gld4(lbox + 2 * static_cast<size_t>(leaf)), hi = gld4(lbox + 2 * static_cast<size_t>(leaf) + 1);
    float tn, tf;
    uint32_t fb = 0;
    const bool pass = box_test<COUNT>(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, r, ri, tn, tf, fb);
    if (COUNT) cnt.c[15] += fb;
    return pass;
}
// The triangles are fetched BDPT_WLEAF_GROUP at a time, all loads of a group
// issued before its first test (the magnitude of leaf_tests' BDPT_LEAF_GROUP
// for this walk):
//   1  one triangle per round trip: triangle k + 1's loads sit behind triangle
//      k's test and its branch, a leaf of `count` triangles exposes `count`
//      dependent latencies (the device code before the grouped form; A/B runs)
//   2  pairs (k, k + 1): half the round trips. An odd count's last pair loads
//      the leaf's last triangle twice (the second index clamped to count - 1:
//      no address outside [start, start + count)), its second result unused.
// The tests run in index order with the ungrouped loop's decisions; a triangle
// the ungrouped loop would not have reached (past the count, or behind the hit
// that ends an occlusion query) is loaded but neither tested nor counted.
// 24 VGPRs per pair, under the node step's 28 (WNode), which is dead here.
#ifndef BDPT_WLEAF_GROUP
#define BDPT_WLEAF_GROUP 2
#endif
template <bool COUNT>
__device__ __forceinline__ bool wleaf_tests(const float4* __restrict__ wtri, const float4* __restrict__ lbox,
                                            uint32_t link, const Ray& r, const RayInv& ri, bool any, float& best_t,
                                            int& best, float& best_u, float& best_v, Counts& cnt,
                                            bool defer = false) {
    constexpr uint32_t G = BDPT_WLEAF_GROUP;
    static_assert(G == 1 || G == 2, "BDPT_WLEAF_GROUP: 1 or 2 (four triangles do not fit under the node step's registers)");
    const uint32_t start = (link >> 3) & 0x0fffffffu, count = link & 7u;
    if constexpr (G == 1) {  // the ungrouped loop as it was written: the same device code (tools/asm_identity.sh)
        for (uint32_t k = 0; k < count; k++) {
            const size_t i = static_cast<size_t>(start + k);
            const float4 q0 = gld4(wtri + 3 * i), q1 = gld4(wtri + 3 * i + 1), q2 = gld4(wtri + 3 * i + 2);
            float t, u, v;
            if (COUNT) cnt.c[3]++;
            if (!tri_test_edges(xyz(q0), xyz(q1), xyz(q2), r, t, u, v)) continue;
            const int idx = __float_as_int(q0.w);
            if (any) {
                if (t <= r.max_t && ref_leaf_passes<COUNT>(lbox, __float_as_uint(q1.w), r, ri, cnt)) {
                    best = idx;
                    return true;
                }
            } else if ((t < best_t || (t == best_t && best >= 0 && idx < best)) &&
                       (defer || ref_leaf_passes<COUNT>(lbox, __float_as_uint(q1.w), r, ri, cnt))) {
                best_t = t, best = idx, best_u = u, best_v = v;
            }
        }
        return false;
    }
    for (uint32_t k0 = 0; k0 < count; k0 += G) {
        float4 q[G][3];
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            const size_t i = static_cast<size_t>(start + (g == 0 || k0 + g < count ? k0 + g : count - 1));
            q[g][0] = gld4(wtri + 3 * i), q[g][1] = gld4(wtri + 3 * i + 1), q[g][2] = gld4(wtri + 3 * i + 2);
        }
        if (G > 1) {  // every load of the group in flight before the first test
#pragma unroll
            for (uint32_t g = 0; g < G; g++)
#pragma unroll
                for (int j = 0; j < 3; j++) asm volatile("" ::"v"(q[g][j].x), "v"(q[g][j].y), "v"(q[g][j].z), "v"(q[g][j].w));
        }
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            if (g > 0 && k0 + g >= count) break;
            const float4 q0 = q[g][0], q1 = q[g][1], q2 = q[g][2];
            float t, u, v;
            if (COUNT) cnt.c[3]++;
            if (!tri_test_edges(xyz(q0), xyz(q1), xyz(q2), r, t, u, v)) continue;
            const int idx = __float_as_int(q0.w);
            if (any) {
                if (t <= r.max_t && ref_leaf_passes<COUNT>(lbox, __float_as_uint(q1.w), r, ri, cnt)) {
                    best = idx;
                    return true;
                }
            } else if ((t < best_t || (t == best_t && best >= 0 && idx < best)) &&
                       (defer || ref_leaf_passes<COUNT>(lbox, __float_as_uint(q1.w), r, ri, cnt))) {
                best_t = t, best = idx, best_u = u, best_v = v;
            }
        }
    }
    return false;
}

struct TravState {
    uint32_t link;
    int sp;
    int best;
    float best_t, best_u, best_v;
};

__device__ __forceinline__ TravState trav_begin(const TravScene& sc, const Ray& r) {
    return TravState{sc.wroot_link, 0, -1, r.max_t, 0.f, 0.f};
}

// Pops the nearest pending entry that can still hold a closer hit; false when
// the traversal is complete.
__device__ __forceinline__ bool trav_pop(const Ray& r, bool any, TravState& ts, const Stack& stk,
                                         uint32_t* culled = nullptr) {
    while (ts.sp > 0) {
        const uint2 e = stk.get(--ts.sp);
        if (!(__uint_as_float(e.y) > cull_far(ts.best_t))) {
            ts.link = e.x;
            return true;
        }
        if (culled) (*culled)++;
    }
    return false;
}

// A 4-wide node record as the walk reads it: the 128-byte float record
// (wide_bvh.hpp; v[0..5] = lo.x hi.x lo.y hi.y lo.z hi.z, v[6] = links).
constexpr int kNodeVecs = 7, kNodeStride = 8, kNodeLinks = 6;
struct WNode {
    float4 v[kNodeVecs];
};
__device__ __forceinline__ WNode load_wnode(const float4* __restrict__ base, uint32_t link) {
    const float4* nd = base + kNodeStride * static_cast<size_t>(link);
    WNode n;
#pragma unroll
    for (int j = 0; j < kNodeVecs; j++) n.v[j] = gld4(nd + j);
    return n;
}
// The node as the slack-free test reads it (NF): v[0] / v[1] the near / far x
// planes of the four children for this ray — lo.x / hi.x when d.x > 0, hi.x /
// lo.x otherwise (RayInv::fast: inv is finite and nonzero) — likewise v[2..5] for
// y and z, v[6] the links. Each pair is one 128-byte record's 16-byte vectors at
// offsets (s, s ^ 16) from the axis's base with s = 16 for a negative direction:
// per-lane 32-bit offsets from the uniform base (the host keeps the node array
// under 4 GiB for this test, node_slack_needed). With inv > 0, l <= h gives
// fma(l, inv, oi) <= fma(h, inv, oi) (rounding is monotone), so max3 / min3 of
// the picked planes are the entry / exit distances slab_fma's six min / max form
// (one max3 and one min3 per child instead of eight operations; with the merged
// culls below: Caustic +2.3 %, HardLight +3.4 %, synth1m +3.7 %).
__device__ __forceinline__ uint32_t plane_sel(float inv) { return (__float_as_uint(inv) >> 27) & 16u; }
__device__ __forceinline__ WNode load_wnode_nf(const float4* __restrict__ base, uint32_t link, f3 inv) {
    const char* b = reinterpret_cast<const char*>(base);
    const uint32_t off = link << 7;
    uint32_t sx = plane_sel(inv.x), sy = plane_sel(inv.y), sz = plane_sel(inv.z);
    const uint32_t ax = off | sx, ay = off | sy, az = off | sz;
    WNode n;
    n.v[0] = gld4(reinterpret_cast<const float4*>(b + ax));
    n.v[1] = gld4(reinterpret_cast<const float4*>(b + (ax ^ 16u)));
    n.v[2] = gld4(reinterpret_cast<const float4*>(b + ay + 32));
    n.v[3] = gld4(reinterpret_cast<const float4*>(b + (ay ^ 16u) + 32));
    n.v[4] = gld4(reinterpret_cast<const float4*>(b + az + 64));
    n.v[5] = gld4(reinterpret_cast<const float4*>(b + (az ^ 16u) + 64));
    n.v[6] = gld4(reinterpret_cast<const float4*>(b + off + 96));
    return n;
}

// Interior 4-wide node ts.link: tests the four children, descends into the
// nearest hit child (true) and stacks the others far-to-near; false when no
// child is hit (the caller pops).
template <bool COUNT, bool SLACK, bool NF = false>
__device__ __forceinline__ bool trav_node_vals(const WNode& n, const Ray& r, const RayInv& ri, bool any,
                                               TravState& ts, const Stack& stk, Counts& cnt);
template <bool COUNT, bool SLACK>
__device__ __forceinline__ bool trav_node(const TravScene& sc, const Ray& r, const RayInv& ri, bool any, TravState& ts,
                                          const Stack& stk, Counts& cnt) {
    if (!SLACK) return trav_node_vals<COUNT, false, true>(load_wnode_nf(sc.wnodes, ts.link, ri.inv), r, ri, any, ts, stk, cnt);
    return trav_node_vals<COUNT, SLACK>(load_wnode(sc.wnodes, ts.link), r, ri, any, ts, stk, cnt);
}
// The four children of a 4-wide node: key = entry distance of each child the
// walk must visit (box hit, entered before `far`, left after the near cull), +inf
// otherwise, sorted near-first together with the links (kEmptyLinkDev for none).
template <bool SLACK, bool NF = false>
__device__ __forceinline__ void node_child_keys(const WNode& n, const Ray& r, const RayInv& ri, float far, float (&key)[4],
                                                uint32_t (&lnk)[4]) {
    const float4 lk = n.v[kNodeLinks];
    const f3 oi = SLACK ? mk(0.f, 0.f, 0.f) : slab_fma_origin(r.o, ri.inv);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t l = __float_as_uint((&lk.x)[c]);
        float tn, tf;
        const float clx = (&n.v[0].x)[c], chx = (&n.v[1].x)[c], cly = (&n.v[2].x)[c], chy = (&n.v[3].x)[c],
                    clz = (&n.v[4].x)[c], chz = (&n.v[5].x)[c];
        int d = kSlabHit;
        if (NF) {  // v[0], v[2], v[4]: near planes; v[1], v[3], v[5]: far planes (load_wnode_nf)
            tn = fmaxf(fmaxf(fmaf(clx, ri.inv.x, oi.x), fmaf(cly, ri.inv.y, oi.y)), fmaf(clz, ri.inv.z, oi.z));
            tf = fminf(fminf(fmaf(chx, ri.inv.x, oi.x), fmaf(chy, ri.inv.y, oi.y)), fmaf(chz, ri.inv.z, oi.z));
        } else if (SLACK) {
            d = slab_fast(clx, cly, clz, chx, chy, chz, r.o, ri.inv, tn, tf);
        } else {
            slab_fma(clx, cly, clz, chx, chy, chz, oi, ri.inv, tn, tf);
        }
        const bool pass = SLACK ? d != kSlabMiss : !(tn > tf);
        // !(tn > tf), !(tn > far) and !(tf < near) as one comparison: it also drops the
        // boxes when far < near, where no hit can be accepted (the query's max_t or
        // best hit lies below kTriMinT); tn, tf are finite here (RayInv::fast)
        const bool hit = NF ? l != kEmptyLinkDev && !(fmaxf(tn, ri.near) > fminf(tf, far))
                            : l != kEmptyLinkDev && pass && !(tn > far) && !(tf < ri.near);
        key[c] = hit ? tn : __builtin_inff();
        lnk[c] = hit ? l : kEmptyLinkDev;
    }
    // near-first order: sorting network on (key, link)
#define BDPT_CE(a, b)                                                       \
    {                                                                       \
        const bool sw = key[b] < key[a];                                    \
        const float k0 = sw ? key[b] : key[a], k1 = sw ? key[a] : key[b];   \
        const uint32_t l0 = sw ? lnk[b] : lnk[a], l1 = sw ? lnk[a] : lnk[b]; \
        key[a] = k0, key[b] = k1, lnk[a] = l0, lnk[b] = l1;                 \
    }
    BDPT_CE(0, 1) BDPT_CE(2, 3) BDPT_CE(0, 2) BDPT_CE(1, 3) BDPT_CE(1, 2)
#undef BDPT_CE
}
template <bool COUNT, bool SLACK, bool NF>
__device__ __forceinline__ bool trav_node_vals(const WNode& n, const Ray& r, const RayInv& ri, bool any,
                                               TravState& ts, const Stack& stk, Counts& cnt) {
    if (COUNT) cnt.c[2]++;
    float key[4];
    uint32_t lnk[4];
    node_child_keys<SLACK, NF>(n, r, ri, cull_far(ts.best_t), key, lnk);
    if (lnk[0] == kEmptyLinkDev) return false;
    if (lnk[3] != kEmptyLinkDev) stk.put(ts.sp++, lnk[3], key[3]);
    if (lnk[2] != kEmptyLinkDev) stk.put(ts.sp++, lnk[2], key[2]);
    if (lnk[1] != kEmptyLinkDev) stk.put(ts.sp++, lnk[1], key[1]);
    if (COUNT) {  // stack-depth probe: entries held at depth >= 8, >= 12, >= 16
        cnt.c[16] += ts.sp > 8 ? ts.sp - 8 : 0;
        cnt.c[17] += ts.sp > 12 ? ts.sp - 12 : 0;
        cnt.c[18] += ts.sp > 16 ? ts.sp - 16 : 0;
    }
    ts.link = lnk[0];
    return true;
}

// The traversal tree's root node and its interior children (slot k = the
// root's child k) in LDS, copied by each block at kernel start (before the
// barrier of scene_tables_to_lds). Every walk starts at the root, so a query's
// first two node tests run when the lane issues it — with the other lanes of
// the shading step, from broadcast LDS reads — instead of as the first two
// global-memory steps of the walk loop (walk_begin_lds).
struct RootLds {
    WNode root;
    WNode kid[4];
};
__device__ __forceinline__ bool root_lds_usable(const DevScene& sc) { return !(sc.wroot_link & kLeafBit); }
__device__ __forceinline__ void root_lds_fill(RootLds& m, const DevScene& sc) {
    if (!root_lds_usable(sc)) return;
    const float4* const base = sc.wnodes;
    const float4* rn = base + kNodeStride * static_cast<size_t>(sc.wroot_link);
    if (threadIdx.x < kNodeVecs) {
        m.root.v[threadIdx.x] = gld4(rn + threadIdx.x);
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 4 * kNodeVecs) {
        const int k = (threadIdx.x - 64) / kNodeVecs, j = (threadIdx.x - 64) % kNodeVecs;
        const float4 lk = gld4(rn + kNodeLinks);
        const uint32_t l = __float_as_uint((&lk.x)[k]);
        if (l != kEmptyLinkDev && !(l & kLeafBit)) m.kid[k].v[j] = gld4(base + kNodeStride * static_cast<size_t>(l) + j);
    }
}
// The root and (when the walk descends into an interior child) that child;
// false when the query is already complete (a miss: nothing below was hit).
// load_wnode_nf's plane vectors from an LDS copy of a node (the same 16-byte
// vectors at the same offsets: the copy is the record's first 112 bytes)
__device__ __forceinline__ WNode lds_wnode_nf(const WNode& m, f3 inv) {
    const char* b = reinterpret_cast<const char*>(&m);
    const uint32_t sx = plane_sel(inv.x), sy = plane_sel(inv.y), sz = plane_sel(inv.z);
    WNode n;
    n.v[0] = *reinterpret_cast<const float4*>(b + sx);
    n.v[1] = *reinterpret_cast<const float4*>(b + (sx ^ 16u));
    n.v[2] = *reinterpret_cast<const float4*>(b + 32 + sy);
    n.v[3] = *reinterpret_cast<const float4*>(b + 32 + (sy ^ 16u));
    n.v[4] = *reinterpret_cast<const float4*>(b + 64 + sz);
    n.v[5] = *reinterpret_cast<const float4*>(b + 64 + (sz ^ 16u));
    n.v[6] = m.v[6];
    return n;
}
template <bool COUNT, bool SLACK>
__device__ __forceinline__ bool root_node_vals(const WNode& m, const Ray& r, const RayInv& ri, bool any, TravState& ts,
                                               const Stack& stk, Counts& cnt) {
    if (!SLACK) return trav_node_vals<COUNT, false, true>(lds_wnode_nf(m, ri.inv), r, ri, any, ts, stk, cnt);
    return trav_node_vals<COUNT, SLACK>(m, r, ri, any, ts, stk, cnt);
}
template <bool COUNT, bool SLACK>
__device__ __forceinline__ bool walk_begin_lds(const RootLds& m, const Ray& r, const RayInv& ri, bool any,
                                               TravState& ts, const Stack& stk, Counts& cnt) {
    if (COUNT) cnt.c[8]++;
    bool live = root_node_vals<COUNT, SLACK>(m.root, r, ri, any, ts, stk, cnt);
    if (live && !(ts.link & kLeafBit)) {
        const float4 lk = m.root.v[kNodeLinks];
        const int k = ts.link == __float_as_uint(lk.x) ? 0
                      : ts.link == __float_as_uint(lk.y) ? 1
                      : ts.link == __float_as_uint(lk.z) ? 2 : 3;
        if (COUNT) cnt.c[8]++;
        live = root_node_vals<COUNT, SLACK>(m.kid[k], r, ri, any, ts, stk, cnt) || trav_pop(r, any, ts, stk);
    }
    return live;
}

// One loop iteration (a 4-wide node or a leaf, then the pop). Returns true
// when the query is complete (result in ts.best / best_t / best_u / best_v).
template <bool COUNT, bool SLACK = true>
__device__ __forceinline__ bool trav_step(const TravScene& sc, const Ray& r, const RayInv& ri, bool any, TravState& ts,
                                          const Stack& stk, Counts& cnt, bool defer = false) {
    if (COUNT) {
        cnt.c[8]++;
        if (first_active_lane()) cnt.c[9]++;
    }
    if (ts.link & kLeafBit) {
        if (wleaf_tests<COUNT>(sc.wtri, sc.lbox, ts.link, r, ri, any, ts.best_t, ts.best, ts.best_u, ts.best_v, cnt,
                               defer))
            return true;
    } else if (trav_node<COUNT, SLACK>(sc, r, ri, any, ts, stk, cnt)) {
        return false;
    }
    return !trav_pop(r, any, ts, stk, COUNT ? &cnt.c[19] : nullptr);
}

// The same walk as a while-while loop (Aila & Laine 2009): lanes descend
// through interior nodes together until each holds a leaf (or is done), then
// the leaves are tested together — a wave iteration runs one kind of work.
template <bool COUNT>
__device__ __forceinline__ void trav_while_while(const TravScene& sc, const Ray& r, const RayInv& ri, bool any,
                                                 TravState& ts, const Stack& stk, Counts& cnt, bool defer = false) {
    for (;;) {
        bool live = true;
        while (!(ts.link & kLeafBit)) {
            if (COUNT) {
                cnt.c[8]++;
                if (first_active_lane()) cnt.c[9]++;
            }
            if (!trav_node<COUNT, true>(sc, r, ri, any, ts, stk, cnt) && !trav_pop(r, any, ts, stk)) {
                live = false;
                break;
            }
        }
        if (!live) return;
        if (COUNT) {
            cnt.c[8]++;
            if (first_active_lane()) cnt.c[9]++;
        }
        if (wleaf_tests<COUNT>(sc.wtri, sc.lbox, ts.link, r, ri, any, ts.best_t, ts.best, ts.best_u, ts.best_v, cnt,
                               defer))
            return;
        if (!trav_pop(r, any, ts, stk)) return;
    }
}

template <bool FULL, bool COUNT>
__device__ __forceinline__ int traverse(const DevScene& sc, const Ray& r, bool any, const Stack& stk, float& bt,
                                        float& bu, float& bv, Counts& cnt, float near = kNoCullNear) {
    if (r.min_t > r.max_t) return -1;  // the root's entry mint is min_t (bvh.h:277, :287)
    const RayInv ri = ray_inv(r, near);
    if (FULL || !ri.fast || far_origin(sc, r.o)) {  // the reference's tree, unculled
        const TravResult q = traverse_binary<COUNT, Stack>(sc, r, any, false, stk);
        if (COUNT) cnt.c[2] += q.nodes, cnt.c[3] += q.tris, cnt.c[15] += q.exact;
        bt = q.t, bu = q.u, bv = q.v;
        return q.best;
    }
    const TravScene tsc = trav_scene(sc);
    TravState ts = trav_begin(tsc, r);
    trav_while_while<COUNT>(tsc, r, ri, any, ts, stk, cnt);
    bt = ts.best_t, bu = ts.best_u, bv = ts.best_v;
    return ts.best;
}

// The closest hit of ONE ray (the same in every lane of the wave) walked by the
// whole wave (coop_closest below): each round pops pending entries from an LDS
// stack, tests them (a 4-wide node's children, a leaf's triangles against the
// best so far), takes the lexicographic minimum (t, reference index) over the
// lanes and pushes the children. The result is the serial walk's: the minimum
// over the candidates of every entry the walk cannot cull (the same conservative
// per-entry tests, cull_far of the best so far), ties to the lowest reference
// index, accepted only below r.max_t — the order the entries are visited in does
// not enter it. For the Russian-roulette build's trapped subpaths (bdpt_kernels.hip,
// express mode and the chain kernel): a walk takes ~9 rounds instead of ~30
// dependent steps. `stack` holds `cap` entries; false if they did not suffice
// (the caller reports it). With bound < r.max_t only candidates below `bound`
// are accepted (and entries beyond it culled): a hit found is then the same
// result — the minimum over all candidates lies below it — and none found
// (best -1) means the walk must be repeated unbounded.
__device__ __forceinline__ uint64_t coop_key(float t, int idx) {
    const uint32_t b = __float_as_uint(t);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // float order as unsigned order
    return (static_cast<uint64_t>(o) << 32) | static_cast<uint32_t>(idx);
}
// The walk's LDS stack: entry e at base[e] (a wave's own array), or spread over
// the columns a wave's lanes own in a block's per-lane stack (entry e at
// base[(e / 64) * stride + e % 64], base = the wave's first lane).
typedef __attribute__((address_space(3))) u32x2 coop_lds_e;
struct CoopStack {
    uint2* base;
    int stride;  // 0: contiguous
    __device__ __forceinline__ coop_lds_e* at(int e) const {
        return (coop_lds_e*)base + (stride ? (e >> 6) * stride + (e & 63) : e);
    }
};
// A lane's share of a cooperative walk's entry `link`: child c of an interior
// node (its six planes and its link: seven dword loads instead of the node's
// seven 16-byte vectors) — node_child_keys' test of that child (slab_fast with
// the slack, slab_fma without; the same culls), its entry distance and link in
// (key, lnk) when the walk must visit it — or triangles c, c + 4 of a leaf, with
// wleaf_tests' acceptance rule against (lt, lb).
template <bool SLACK>
__device__ __forceinline__ void coop_entry(const TravScene& sc, const Ray& r, const RayInv& ri, f3 oi, float far,
                                              uint32_t link, int c, float& lt, int& lb, float& lu, float& lv,
                                              float& key, uint32_t& lnk) {
    if (link & kLeafBit) {
        const uint32_t start = (link >> 3) & 0x0fffffffu, count = link & 7u;
        Counts cnt;  // (not a counting pass)
        for (uint32_t j = static_cast<uint32_t>(c); j < count; j += 4) {
            const float4* p = sc.wtri + 3 * static_cast<size_t>(start + j);
            const float4 q0 = gld4(p), q1 = gld4(p + 1), q2 = gld4(p + 2);
            float t, u, v;
            if (!tri_test_edges(xyz(q0), xyz(q1), xyz(q2), r, t, u, v)) continue;
            const int idx = __float_as_int(q0.w);
            if ((t < lt || (t == lt && lb >= 0 && idx < lb)) &&
                ref_leaf_passes<false>(sc.lbox, __float_as_uint(q1.w), r, ri, cnt))
                lt = t, lb = idx, lu = u, lv = v;
        }
    } else {
        // child c of the 128-byte record: lo.x hi.x lo.y hi.y lo.z hi.z links, four floats each
        const float* nd = reinterpret_cast<const float*>(sc.wnodes + kNodeStride * static_cast<size_t>(link)) + c;
        const float clx = gld1(nd), chx = gld1(nd + 4), cly = gld1(nd + 8), chy = gld1(nd + 12), clz = gld1(nd + 16),
                    chz = gld1(nd + 20);
        const uint32_t l = __float_as_uint(gld1(nd + 24));
        float tn, tf;
        int d = kSlabHit;
        if (SLACK) d = slab_fast(clx, cly, clz, chx, chy, chz, r.o, ri.inv, tn, tf);
        else slab_fma(clx, cly, clz, chx, chy, chz, oi, ri.inv, tn, tf);
        const bool pass = SLACK ? d != kSlabMiss : !(tn > tf);
        if (l != kEmptyLinkDev && pass && !(tn > far) && !(tf < ri.near)) key = tn, lnk = l;
    }
}
// The walk with the work of an entry spread over 4 lanes: each round pops up to 16
// entries, and lane 4s + c takes child c (or triangles c, c + 4) of entry s, one
// box or triangle test per lane. A lone walk's frontier rarely holds more than 16
// entries, and a round of one wave alone on its SIMD costs its instructions, not
// its loads. Entries are pushed unsorted (the visiting order does not enter the
// result).
template <bool SLACK>
__device__ __forceinline__ bool coop_closest(const TravScene& sc, const Ray& r, const RayInv& ri, float bound,
                                             CoopStack stk, int cap, float& best_t, int& best, float& best_u,
                                             float& best_v) {
    const uint32_t lane = __lane_id();
    const int slot = static_cast<int>(lane >> 2), c = static_cast<int>(lane & 3u);
    const f3 oi = SLACK ? mk(0.f, 0.f, 0.f) : slab_fma_origin(r.o, ri.inv);
    best_t = bound < r.max_t ? bound : r.max_t, best = -1, best_u = best_v = 0.f;
    if (lane == 0) *stk.at(0) = u32x2{sc.wroot_link, __float_as_uint(-__builtin_inff())};
    int sp = 1;
    bool ok = true;
    while (sp > 0) {
        const int k = sp < 16 ? sp : 16;
        u32x2 e = {kEmptyLinkDev, 0u};
        if (slot < k) e = *stk.at(sp - k + slot);
        sp -= k;
        const float far = cull_far(best_t);
        const bool live = e.x != kEmptyLinkDev && !(__uint_as_float(e.y) > far);
        float lt = best_t, lu = best_u, lv = best_v;
        int lb = best;
        float key = __builtin_inff();
        uint32_t lnk = kEmptyLinkDev;
        if (live) coop_entry<SLACK>(sc, r, ri, oi, far, e.x, c, lt, lb, lu, lv, key, lnk);
        // the wave's lexicographic minimum of (t, index) over the lanes that found a better hit
        uint64_t imp = __ballot(lb != best);
        if (imp) {
            uint64_t m = ~0ull;
            int w = 0;
            while (imp) {
                const int i = __ffsll(static_cast<unsigned long long>(imp)) - 1;
                imp &= imp - 1;
                const uint64_t ki = coop_key(lane_val(lt, i), lane_val(lb, i));
                if (ki < m) m = ki, w = i;
            }
            best_t = lane_val(lt, w), best = lane_val(lb, w), best_u = lane_val(lu, w), best_v = lane_val(lv, w);
        }
        const uint64_t has = __ballot(lnk != kEmptyLinkDev);
        const int n = popc64(has);
        if (sp + n > cap) {
            ok = false;
        } else {
            if (lnk != kEmptyLinkDev) *stk.at(sp + lanes_below(has)) = u32x2{lnk, __float_as_uint(key)};
            sp += n;
        }
    }
    return ok;
}

// coop_closest for up to four rays at once: the wave split into 64 / G groups
// of G lanes (G = 32 or 16), group g walking its own ray on its own range
// [base, base + cap) of the stack entries; inactive groups idle. Each group's
// result is coop_closest's for its ray (the same per-entry tests, the minimum
// (t, index) over the group's candidates); false for a group whose entries did
// not fit. For the Russian-roulette build's express waves holding 2-4 long walks,
// which otherwise take turns with all 64 lanes. Group g's lane 4s + c takes child
// c (or triangles c, c + 4) of the group's entry s, G / 4 entries per round.
template <bool SLACK>
__device__ __forceinline__ bool coop_closest_groups(const TravScene& sc, const Ray& r, const RayInv& ri, float bound,
                                                    bool active, CoopStack stk, int base, int cap, int G,
                                                    float& best_t, int& best, float& best_u, float& best_v) {
    const uint32_t lane = __lane_id();
    const int gl = static_cast<int>(lane) & (G - 1);
    const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (static_cast<int>(lane) - gl);
    const int slot = gl >> 2, c = gl & 3, per = G >> 2;
    const f3 oi = SLACK ? mk(0.f, 0.f, 0.f) : slab_fma_origin(r.o, ri.inv);
    best_t = bound < r.max_t ? bound : r.max_t, best = -1, best_u = best_v = 0.f;
    if (active && gl == 0) *stk.at(base) = u32x2{sc.wroot_link, __float_as_uint(-__builtin_inff())};
    int sp = active ? 1 : 0;
    bool ok = true;
    while (__ballot(sp > 0)) {
        const int k = sp < per ? sp : per;
        u32x2 e = {kEmptyLinkDev, 0u};
        if (slot < k) e = *stk.at(base + sp - k + slot);
        sp -= k;
        const float far = cull_far(best_t);
        const bool live = e.x != kEmptyLinkDev && !(__uint_as_float(e.y) > far);
        float lt = best_t, lu = best_u, lv = best_v;
        int lb = best;
        float key = __builtin_inff();
        uint32_t lnk = kEmptyLinkDev;
        if (live) coop_entry<SLACK>(sc, r, ri, oi, far, e.x, c, lt, lb, lu, lv, key, lnk);
        // each group's lexicographic minimum of (t, index) over its improving lanes
        uint64_t imp = __ballot(lb != best);
        if (imp) {
            uint64_t m = ~0ull;
            int w = static_cast<int>(lane);
            while (imp) {
                const int i = __ffsll(static_cast<unsigned long long>(imp)) - 1;
                imp &= imp - 1;
                const uint64_t ki = coop_key(lane_val(lt, i), lane_val(lb, i));
                if ((gmask >> i) & 1ull && ki < m) m = ki, w = i;
            }
            best_t = __shfl(lt, w), best = __shfl(lb, w), best_u = __shfl(lu, w), best_v = __shfl(lv, w);
        }
        const uint64_t has = __ballot(lnk != kEmptyLinkDev) & gmask;
        const int n = popc64(has);
        if (sp + n > cap) {
            ok = false;
        } else {
            if (lnk != kEmptyLinkDev) *stk.at(base + sp + lanes_below(has)) = u32x2{lnk, __float_as_uint(key)};
            sp += n;
        }
    }
    return ok;
}

}  // namespace dev
}  // namespace bdpt
