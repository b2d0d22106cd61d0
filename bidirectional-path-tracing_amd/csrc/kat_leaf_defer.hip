// AcceleratorBVH::intersect (accel.h:125-172) through the closest-hit protocol of
// the frame kernels built with BDPT_LEAF_DEFER (bdpt_kernels.hip), one
// ray per lane, so the parity tests can pin it against the reference's own results:
// the walk that accepts triangle hits without the reference-leaf check (wleaf_tests,
// `defer`), the check of its winner against the box in the winner's shade record
// (leaf_box_passes) and, when that fails, the same query walked again with the check
// in the leaf step. force != 0 fails the first check of every hit, as the frame
// kernels' kSchedLeafRecheck does. Output as intersect_kat_kernel's (kat_kernels.hip),
// and per ray whether it was walked again.
#include <hip/hip_runtime.h>

#include "dev_shade.hpp"

namespace bdpt {
namespace dev {

constexpr int kDeferBlock = 64;

__global__ __launch_bounds__(kDeferBlock) void intersect_defer_kernel(DevScene sc, int64_t n, int by_id, int force,
                                                                     const float* __restrict__ rays,
                                                                     const float* __restrict__ nrm,
                                                                     const int32_t* __restrict__ otri,
                                                                     uint2* __restrict__ gstack, uint32_t nslots,
                                                                     float* __restrict__ out,
                                                                     int32_t* __restrict__ rewalked) {
    __shared__ uint2 stack_mem[kLdsStack * kDeferBlock];
    scene_tables_to_lds(sc);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kDeferBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = static_cast<uint32_t>(i % nslots);
    const Stack stk{stack_mem + threadIdx.x, kDeferBlock, kLdsStack, gstack, nslots, slot};
    const float* r = rays + 8 * i;
    const Ray ray{mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], r[7]};
    Counts cnt;
    float near = kNoCullNear;  // the frame kernels' near-cull rule, as intersect_kat_kernel applies it
    if (nrm) {
        const f3 sn = mk(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        const bool camera = sn.x == 0.f && sn.y == 0.f && sn.z == 0.f;
        const int ot = otri ? otri[i] : -1;
        const int code = ot >= 0 ? __float_as_int(gld4(sc.shade + kShadeStride * static_cast<size_t>(ot) + 1).w) : 0;
        near = (camera || !graze_exempt(ray.d, sn, code)) ? kCullNear : kNoCullNear;
    }
    int res = -1, again = 0;
    float t = 0.f, u = 0.f, v = 0.f;
    const RayInv ri = ray_inv(ray, near);
    if (ray.min_t > ray.max_t) {  // the reference culls the root (bvh.h:277, :287)
    } else if (!ri.fast || far_origin(sc, ray.o)) {  // the reference's tree, unculled: nothing deferred
        const TravResult q = traverse_binary<false, Stack>(sc, ray, false, false, stk);
        res = q.best, t = q.t, u = q.u, v = q.v;
    } else {
        const TravScene tsc = trav_scene(sc);
        TravState ts = trav_begin(tsc, ray);
        trav_while_while<false>(tsc, ray, ri, false, ts, stk, cnt, true);
        if (ts.best >= 0) {
            float4 box[2];
            shade_box(sc, ts.best, box);
            if (force || !leaf_box_passes<false>(sc, box, by_id != 0, ray, ri, cnt)) {
                again = 1;
                ts = trav_begin(tsc, ray);
                trav_while_while<false>(tsc, ray, ri, false, ts, stk, cnt, false);
            }
        }
        res = ts.best, t = ts.best_t, u = ts.best_u, v = ts.best_v;
    }
    rewalked[i] = again;
    float* o = out + 20 * i;
    for (int k = 0; k < 20; k++) o[k] = 0.f;
    const bool hit = res >= 0 && t <= ray.max_t && t >= ray.min_t;  // accel.h:133
    o[1] = t;
    if (!hit) return;
    Hit h;
    shade_hit(sc, res, u, v, t, ray.d, h);
    const float4* sh = sc.shade + kShadeStride * static_cast<size_t>(res);
    const f3 v0 = xyz(gld4(sc.tri + 3 * static_cast<size_t>(res))), v1 = xyz(gld4(sh + 3)), v2 = xyz(gld4(sh + 4));
    const f3 ng = normalize(cross(v1 - v0, v2 - v0));
    o[0] = __int_as_float(1), o[2] = u, o[3] = v;
    o[4] = __int_as_float(shape_id(h.shape)), o[5] = __int_as_float(__float_as_int(gld4(sh + 2).w)), o[6] = __int_as_float(h.mat);
    o[7] = h.p.x, o[8] = h.p.y, o[9] = h.p.z;
    o[10] = h.n.x, o[11] = h.n.y, o[12] = h.n.z;
    o[13] = ng.x, o[14] = ng.y, o[15] = ng.z;
    o[16] = h.wo.x, o[17] = h.wo.y, o[18] = h.wo.z;
    o[19] = __int_as_float(res);
}

}  // namespace dev

hipError_t launch_intersect_defer(const dev::DevScene& sc, int64_t n, int by_id, int force, const float* rays,
                                  const float* nrm, const int32_t* otri, uint2* gstack, uint32_t nslots, float* out,
                                  int32_t* rewalked, hipStream_t st) {
    if (n > 0)
        hipLaunchKernelGGL(dev::intersect_defer_kernel,
                           dim3(static_cast<unsigned>((n + dev::kDeferBlock - 1) / dev::kDeferBlock)),
                           dim3(dev::kDeferBlock), 4 * static_cast<size_t>(sc.lds_words), st, sc, n, by_id, force, rays,
                           nrm, otri, gstack, nslots, out, rewalked);
    return hipGetLastError();
}

}  // namespace bdpt
