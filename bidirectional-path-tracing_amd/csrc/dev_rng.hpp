// The sampler: std::mt19937 computed lazily per lane (LazyMT), its HBM continuation ring
// for draws past 226, and the canonical float draws next1 / next2.
// Reads BDPT_SAMPLER_STATE (the single-sample build's generator) and BDPT_DEEP_RNG (the ring).
#pragma once

#include "dev_scene.hpp"

namespace bdpt {
namespace dev {

// ------------------------------------------------------------------ sampler
// std::mt19937(seed) + uniform_real_distribution<float> (math.h:63-76). A BDPT
// sample draws at most 10 + 8 (rrDepth - 1) numbers (< 227 for rrDepth <= 28),
// all from the first twist, so output n is computed lazily from the seeding
// recurrence: out_n = temper(x[n+397] ^ twist(x[n], x[n+1])). State: x[n],
// x[n+1], x[n+397] and n. Draws past 226 continue from a per-lane ring of 624
// untempered outputs in HBM, which only deeper rrDepth needs: generated ahead for the
// BDPT builds (mt_ring_ahead), per draw for the path tracer (mt_ring_step).
struct LazyMT {
    uint32_t a0, a1, b, n;
};

__device__ __forceinline__ uint32_t mt_init_step(uint32_t x, uint32_t i) { return 1812433253u * (x ^ (x >> 30)) + i; }

// x[397] of the seeding recurrence: the 397 dependent steps (each with a
// quarter-rate 32-bit multiply) that dominate seeding.
__device__ __forceinline__ uint32_t mt_x397(uint32_t seed) {
    uint32_t x = seed;
#pragma unroll 4
    for (uint32_t i = 1; i <= 397; i++) x = mt_init_step(x, i);
    return x;
}
// Seeds from a precomputed x[397] (mt_x397(seed)).
__device__ __forceinline__ void mt_seed_with(LazyMT& r, uint32_t seed, uint32_t x397) {
    r.a0 = seed;
    r.a1 = mt_init_step(seed, 1);
    r.b = x397;
    r.n = 0;
}
__device__ __forceinline__ void mt_seed(LazyMT& r, uint32_t seed) { mt_seed_with(r, seed, mt_x397(seed)); }

__device__ __forceinline__ uint32_t mt_next_u32(LazyMT& r) {
    uint32_t y = (r.a0 & 0x80000000u) | (r.a1 & 0x7fffffffu);
    uint32_t v = r.b ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    r.a0 = r.a1;
    r.a1 = mt_init_step(r.a1, r.n + 2);
    r.b = mt_init_step(r.b, r.n + 398);
    r.n++;
    v ^= (v >> 11);
    v ^= (v << 7) & 0x9d2c5680u;
    v ^= (v << 15) & 0xefc60000u;
    v ^= (v >> 18);
    return v;
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t v) {
    v ^= (v >> 11);
    v ^= (v << 7) & 0x9d2c5680u;
    v ^= (v << 15) & 0xefc60000u;
    v ^= (v >> 18);
    return v;
}
__device__ __forceinline__ uint32_t mt_twist(uint32_t a, uint32_t b, uint32_t c) {  // c ^ twist(a, b)
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// Output n >= 227 of std::mt19937(seed): u[n] = u[n-227] ^ twist(u[n-624],
// u[n-623]) (with the seeding values x[n], x[n+1] while n + 1 < 624), kept in a
// 624-word ring (word k at ring[k * st]). The first call materialises outputs
// 0..226 (the seed is needed then only).
__device__ __forceinline__ uint32_t mt_ring_step(LazyMT& m, uint32_t seed, uint32_t* ring, uint32_t st) {
    const uint32_t n = m.n;
    if (n == 227) {
        LazyMT t;
        t.a0 = seed;
        t.a1 = mt_init_step(seed, 1);
        t.b = seed;
        for (uint32_t i = 1; i <= 397; i++) t.b = mt_init_step(t.b, i);
        for (uint32_t k = 0; k < 227; k++) {
            ring[k * st] = mt_twist(t.a0, t.a1, t.b);
            t.a0 = t.a1;
            t.a1 = mt_init_step(t.a1, k + 2);
            t.b = mt_init_step(t.b, k + 398);
        }
    }
    uint32_t un, un1;
    if (n < 623) un = m.a0, un1 = m.a1;
    else if (n == 623) un = m.a0, un1 = ring[0];
    else un = ring[((n - 624) % 624) * st], un1 = ring[((n - 623) % 624) * st];
    const uint32_t v = mt_twist(un, un1, ring[((n - 227) % 624) * st]);
    ring[(n % 624) * st] = v;
    if (n + 2 <= 623) {
        m.a0 = m.a1;
        m.a1 = mt_init_step(m.a1, n + 2);
    } else if (n + 1 <= 623) {
        m.a0 = m.a1;
    }
    m.n = n + 1;
    return mt_temper(v);
}

#ifndef BDPT_SAMPLER_STATE
#define BDPT_SAMPLER_STATE 0  // 1: the single-sample build (sample_state.hip): draws from a caller's std::mt19937
#endif
#if BDPT_SAMPLER_STATE
// The single-sample entry points (Integrator::render(const Ray&, Sampler&),
// integrator.h:31) take the caller's whole std::mt19937 (Sampler::g, math.h:63-76):
// libstdc++'s _M_x[624] then _M_p, in the order its operator<< writes them. It is
// advanced exactly as mersenne_twister_engine::operator() does (random.tcc:
// _M_gen_rand when _M_p reaches 624, then tempering). One lane uses it; the
// state lives in global memory, its address in LDS header words 0-1.
__device__ BDPT_NOINLINE uint32_t mt_state_u32() {
    const uint64_t base = (static_cast<uint64_t>(g_scene_lds[1]) << 32) | g_scene_lds[0];
    uint32_t* const x = reinterpret_cast<uint32_t*>(base);
    uint32_t p = x[624];
    if (p >= 624u) {
        for (int k = 0; k < 227; k++) x[k] = mt_twist(x[k], x[k + 1], x[k + 397]);
        for (int k = 227; k < 623; k++) x[k] = mt_twist(x[k], x[k + 1], x[k - 227]);
        x[623] = mt_twist(x[623], x[0], x[396]);
        p = 0;
    }
    x[624] = p + 1;
    return mt_temper(x[p]);
}
#endif

// x[0] (the seed) from x[i]: the seeding step x -> 1812433253 (x ^ x >> 30) + i
// is a bijection (odd multiplier; a 30-bit xorshift undoes itself).
__device__ __forceinline__ uint32_t mt_seed_from(uint32_t x, uint32_t i) {
    constexpr uint32_t kInv = 0x9638806du;  // 1812433253^-1 mod 2^32
    for (; i >= 1; i--) {
        x = (x - i) * kInv;
        x ^= x >> 30;
    }
    return x;
}

#ifndef BDPT_DEEP_RNG
#define BDPT_DEEP_RNG 0  // 1: the deep-path build of the megakernel (bdpt_kernels_deep.hip)
#endif
#if BDPT_DEEP_RNG
// BDPT draw n >= 227 (rrDepth > 28: the deep build of the megakernel; the
// host refuses such depths elsewhere). The ring of this lane slot is found
// through the LDS header. Only this build carries the branch and the ring read at
// every draw site: in the default build they cost ~30 % of the throughput.
#ifndef BDPT_RING_AHEAD
#define BDPT_RING_AHEAD 32  // draws generated ahead into the ring at one call site per shading step (a count, > 0)
#endif
// The ring, generated ahead: outputs n >= 227 are produced by mt_ring_ahead,
// called once per shading step (before the sweep) for lanes within
// BDPT_RING_AHEAD draws of the ring, so every draw site reads
// ring[n mod 624] (one load, no call: an out-of-line call at each of the ~20
// draw sites made the caller keep its live registers in scratch). A sweep draws
// far fewer than BDPT_RING_AHEAD numbers (the action DAG's draw sites sum to
// < 20). Per lane slot kMtRingWords words: the 624-word ring, then the
// generator's cursor (x[g], x[g+1] of the seeding sequence while g < 623, g,
// the seed whose outputs the ring holds, and that seed's x[227] — the value a
// lane's LazyMT::a0 keeps from draw 227 on, so a lane past 227 checks on every
// call that the ring is its own).
constexpr uint32_t kMtRingWords = kMtRingSlotWords;
// The lane's slot: header word 3 (the block's first slot; the Russian-roulette
// chain kernel stores the slot of the sample it continues there) + threadIdx.x.
__device__ __forceinline__ uint32_t* mt_ring_slot() {
    const uint64_t base = (static_cast<uint64_t>(g_scene_lds[1]) << 32) | g_scene_lds[0];
    return reinterpret_cast<uint32_t*>(base) + static_cast<size_t>(g_scene_lds[3] + threadIdx.x) * kMtRingWords;
}
// Generates outputs up to r.n + BDPT_RING_AHEAD - 1; false if the lane had
// already drawn past what was generated (a schedule error: the caller reports it).
__device__ BDPT_NOINLINE bool mt_ring_ahead(const LazyMT& r) {
    uint32_t* const ring = mt_ring_slot();
    uint32_t xa0 = ring[624], xa1 = ring[625], g = ring[626];
    const uint32_t want = r.n + BDPT_RING_AHEAD;
    bool moved = false;  // the cursor changed: store it
    if (r.n < 227) {  // (x[n], x[n+1], x[n+397]) still in registers: the seed is recoverable
        const uint32_t seed = mt_seed_from(r.a0, r.n);
        // another seed's outputs, or this seed's past the window that still holds
        // output 227 (g > 851): outputs 0..226 again
        if (ring[627] != seed || g < 227 || g > 851) {
            uint32_t a0 = seed, a1 = mt_init_step(seed, 1), b = seed;
            for (uint32_t i = 1; i <= 397; i++) b = mt_init_step(b, i);
            for (uint32_t k = 0; k < 227; k++) {
                ring[k] = mt_twist(a0, a1, b);
                a0 = a1;
                a1 = mt_init_step(a1, k + 2);
                b = mt_init_step(b, k + 398);
            }
            xa0 = a0, xa1 = a1, g = 227;  // x[227], x[228]
            ring[627] = seed;
            ring[628] = a0;  // x[227]: the ring's tag for lanes past draw 227
            moved = true;
        }
    } else if (ring[628] != r.a0 || g < r.n) {
        // another sample's ring (a stale cursor or tag), or this lane drew past
        // what was generated: a schedule error the caller reports
        return false;
    }
    for (; g < want; g++) {
        moved = true;
        uint32_t un, un1;
        if (g < 623) un = xa0, un1 = xa1;
        else if (g == 623) un = xa0, un1 = ring[0];
        else un = ring[(g - 624) % 624], un1 = ring[(g - 623) % 624];
        ring[g % 624] = mt_twist(un, un1, ring[(g - 227) % 624]);
        if (g + 2 <= 623) {
            xa0 = xa1;
            xa1 = mt_init_step(xa1, g + 2);
        } else if (g + 1 <= 623) {
            xa0 = xa1;
        }
    }
    // (also after outputs 0..226 alone: a cursor left from the slot's previous seed
    // next to this seed's ring[627] would read as this seed's outputs)
    if (moved) ring[624] = xa0, ring[625] = xa1, ring[626] = g;
    return true;
}
// The wave generates lane b's ring ahead (the Russian-roulette build's inline
// chain: one lane draws while 63 wait): outputs g .. n + 63, lane j computing
// output g + j from the three words it reads. Every lane reads before any lane
// writes (each store waits on the wave's loads), and fewer than 227 consecutive
// outputs never read one another, so the words are mt_ring_ahead's; only once
// output 624 is past (no seeding values left). n and a0 are lane b's (wave-
// uniform). Returns the outputs generated so far, or 0 when lane b's ring is not
// its own or not that far (lane b then calls mt_ring_ahead, which reports it).
__device__ __forceinline__ uint32_t mt_ring_ahead_wave(int b, uint32_t n, uint32_t a0) {
    const uint64_t base = (static_cast<uint64_t>(g_scene_lds[1]) << 32) | g_scene_lds[0];
    uint32_t* const ring =
        reinterpret_cast<uint32_t*>(base) + static_cast<size_t>(g_scene_lds[3] + (threadIdx.x & ~63u) + b) * kMtRingWords;
    const uint32_t g = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring[626])));
    const uint32_t tag = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring[628])));
    if (tag != a0 || g < n || g < 624) return 0;
    const uint32_t want = n + 64;
    if (g >= want) return g;
    const uint32_t gj = g + __lane_id();
    uint32_t v = 0;
    if (gj < want) v = mt_twist(ring[(gj - 624) % 624], ring[(gj - 623) % 624], ring[(gj - 227) % 624]);
    if (gj < want) ring[gj % 624] = v;
    if (__lane_id() == 0) ring[626] = want;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (the stores done before lane b reads them)
    return want;
}
__device__ __forceinline__ uint32_t mt_u32_long(LazyMT& r) {
    const uint32_t v = mt_ring_slot()[r.n % 624];
    r.n++;
    return mt_temper(v);
}
#endif  // BDPT_DEEP_RNG

// generate_canonical<float, 24> (libstdc++ 11 random.tcc:3348-3380) of one 32-bit draw: the
// draws >= 0xFFFFFF80 round to 1.0f in the division and are moved to the float below 1.
__device__ __forceinline__ float canonical_f32(uint32_t u) {
    const float f = static_cast<float>(u) / 4294967296.0f;
    return f >= 1.0f ? 0x1.fffffep-1f : f;
}
__device__ __forceinline__ float next1(LazyMT& r) {
#if BDPT_SAMPLER_STATE
    const uint32_t u = mt_state_u32();
    r.n++;
#elif BDPT_DEEP_RNG
    const uint32_t u = r.n < 227 ? mt_next_u32(r) : mt_u32_long(r);
#else
    const uint32_t u = mt_next_u32(r);
#endif
    return canonical_f32(u);
}
struct F2 {
    float x, y;
};
__device__ __forceinline__ F2 next2(LazyMT& r) {
    F2 o;
    o.x = next1(r);
    o.y = next1(r);
    return o;
}

}  // namespace dev
}  // namespace bdpt
