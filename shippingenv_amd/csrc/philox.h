// philox.h — device-side counter-based RNG for the step kernels (gfx950).
//
// Philox4x32-10 (Salmon et al., SC'11; constants of Random123's philox4x32),
// keyed by the 64-bit seed and indexed by (global env id, step counter, slot):
// no RNG state lives in HBM. The draw conventions below are the "RNG contract"
// of DESIGN.md; oracle/shipenv_oracle.c states the same contract independently
// on the CPU, and tests compare the two bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shipenv {

// Step draws (contract v5) are keyed by the quad k = env / 4: quad blocks, where word
// j belongs to env 4k+j (a 32-bit uniform u = w * 2^-32 or an integer draw), and the
// LOSS_r / RESET_r blocks, which belong whole to the r-th env of the quad whose gate
// fired / that auto-resets.
// The reset kernel and the synthetic agent draw one block per env.
enum Slot : uint32_t {
    kSlotFuel = 0,           // u_fuel (fuel-cost noise, every step)
    kSlotLoss0 = 1,          // LOSS_r, r = 0..3 at slots 1, 2, 8, 9 (kSlotLoss[r]): the r-th env
    kSlotLoss1 = 2,          // of the quad whose gate fired takes the whole block: word 0
                             // u_type, words 1-3 the Beta(2,2) uniforms
    kSlotArrive = 3,         // new destination != origin on arrival
    kSlotReset = 4,          // RESET_r, r = 0..3 at slots 4, 10, 16, 17 (reset_slot(r)): the
                             // r-th env of the quad auto-reset in step t: word 0 origin, 1 dest
    kSlotExplicitReset = 5,  // se_reset, per env, epoch in the t word: words 0 origin, 1 dest
    kSlotAction = 6,         // synthetic bench agent, per env
    kSlotGate = 7,           // u_gate (cargo-loss gate)
    kSlotLoss2 = 8,
    kSlotLoss3 = 9,
    kSlotReset1 = 10,
    kSlotSample = 11,        // se_sample_actions, per env: word 0
    kSlotRollout = 12,       // rollout attempt, per rollout: sample word, u_fuel, u_gate, u_type
    kSlotRolloutB = 13,      // rollout attempt (partial loss / arrival): 3 beta uniforms, dest
    kSlotPolicy = 14,        // se_policy, per env: explore draw, random.choice index
    kSlotReplay = 15,        // se_replay_sample, key (seed, 2^64 - 1), t = update: Feistel round keys
    kSlotReset2 = 16,
    kSlotReset3 = 17,
    kSlotMcts = 18,          // MCTS tree step d, per simulation: untried-action choice, u_fuel, u_gate, u_type
    kSlotMctsB = 19,         // MCTS tree step d (partial loss / arrival): 3 beta uniforms, dest
    kSlotSarsa = 20,         // se_sarsa_step, per env, t = the vector step: explore uniform and sample word of
                             // next_action (words 0, 1) and of a fresh env's first choice (words 2, 3)
    kSlotSarsaReset = 21,    // se_sarsa_step's restart: words 0 origin, 1 dest (as kSlotExplicitReset)
    kSlotRolloutQ = 22,      // se_rollout_sarsa, per rollout, t = the position: word 0 the explore uniform (drawn
                             // only with epsilon > 0 and outside _try_action's fallback)
    kSlotSarsaTry = 32,      // _try_action attempt j at 32 + 2j: sample word (j >= 1), u_fuel, u_gate, u_type;
                             // 33 + 2j (partial loss / arrival): 3 beta uniforms, dest; j < 64, up to slot 159
};

// RESET_r slot of the r-th auto-reset env of a quad
__host__ __device__ constexpr uint32_t reset_slot(uint32_t r) {
    return r == 0 ? kSlotReset : r == 1 ? kSlotReset1 : r == 2 ? kSlotReset2 : kSlotReset3;
}

// LOSS_r slot of the r-th firing env of a quad
__host__ __device__ constexpr uint32_t loss_slot(uint32_t r) {
    return r == 0 ? kSlotLoss0 : r == 1 ? kSlotLoss1 : r == 2 ? kSlotLoss2 : kSlotLoss3;
}

struct U4 {
    uint32_t v[4];
};

// three-way xor in one v_bitop3_b32 (truth table 0x96, gfx950)
__host__ __device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// One 32x32 -> 64-bit product per multiplier (v_mad_u64_u32) instead of a
// separate mul_hi / mul_lo pair; the key schedule is wave-uniform (scalar).
// Compiled for the host too (tools/philox_pair_check.cpp checks draw2 against it there).
__host__ __device__ __forceinline__ U4 philox10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                       uint32_t k0, uint32_t k1) {
    // The key is opaque here, so each block recomputes its 18 scalar key adds
    // instead of the compiler hoisting every block's schedule out of the step
    // loop: ~20 live SGPRs per block spilled to VGPR lanes (v_readlane + s_nop).
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+s"(k0), "+s"(k1));
#endif
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, k0);
        const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, k1);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

// (seed, env, t, slot) -> 4 words
struct Key {
    uint32_t k0, k1;  // seed
    uint32_t e0, e1;  // global env id
};

__host__ __device__ __forceinline__ U4 draw(const Key& k, uint32_t t, uint32_t slot) {
    return philox10(k.e0, k.e1, t, slot, k.k0, k.k1);
}

// The FUEL and GATE blocks of one quad at one counter, drawn together (the state-only step of
// a fused sequence draws both every step). Their counters (e0, e1, t, slot) differ in the slot
// alone, and the slot enters a block through c3 only, so of rounds 1-3:
//   round 1  n0 = hi(M1 t) ^ e1 ^ k0 and c1 = lo(M1 t) are common to both blocks;
//            n2 = hi(M0 e0) ^ slot ^ k1 and c3 = lo(M0 e0) depend on neither t nor state;
//   round 2  the product M0 n0 and n2' = hi(M0 n0) ^ c3 ^ (k1 + W1) are common; the product
//            M1 n2 is per slot and step-invariant, so n0' = hi(M1 n2) ^ c1 ^ (k0 + W0) is one
//            xor per block;
//   round 3  the product M1 n2' is common; M0 n0' is the first per-block product of a step.
// PairInv holds the step-invariant parts, computed once per lane before the step loop (n2 itself
// is read by its product alone, so only the product's halves are kept); draw2
// computes the common parts once and runs rounds 4-10 as philox10 does. The words are those of
// draw(k, t, kSlotFuel) and draw(k, t, kSlotGate) bit for bit, for any e1, key and t.
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct PairInv {
    uint32_t c3;          // lo(M0 e0): round 1's c3 of both blocks
    uint32_t hi[2], lo[2];  // the halves of M1 n2, n2 = hi(M0 e0) ^ slot ^ k1; [0] FUEL, [1] GATE
};
struct U4x2 {
    U4 fuel, gate;
};

__host__ __device__ __forceinline__ PairInv pair_invariants(const Key& k) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * k.e0;
    const uint32_t slot[2] = {kSlotFuel, kSlotGate};
    PairInv v;
    v.c3 = (uint32_t)p0;
    for (int b = 0; b < 2; ++b) {
        const uint64_t p1 = (uint64_t)kPhiloxM1 * xor3((uint32_t)(p0 >> 32), slot[b], k.k1);
        v.hi[b] = (uint32_t)(p1 >> 32);
        v.lo[b] = (uint32_t)p1;
    }
    return v;
}

__host__ __device__ __forceinline__ U4x2 draw2(const Key& k, const PairInv& v, uint32_t t) {
    uint32_t k0 = k.k0, k1 = k.k1;
    // round 1, common
    const uint64_t q1 = (uint64_t)kPhiloxM1 * t;
    const uint32_t n0 = xor3((uint32_t)(q1 >> 32), k.e1, k0);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
    // round 2: the common product and n2', one xor per block
    const uint64_t q0 = (uint64_t)kPhiloxM0 * n0;
    const uint32_t n2 = xor3((uint32_t)(q0 >> 32), v.c3, k1);
    const uint32_t c3 = (uint32_t)q0;
    k1 += kPhiloxW1;
    // round 3's common product
    const uint64_t q2 = (uint64_t)kPhiloxM1 * n2;
    U4 o[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        // the key opaque per block, as in philox10: each block computes its scalar key adds
        // where it runs (the compiler moves the two blocks apart) instead of one schedule
        // held in ~16 SGPRs across the whole step
        uint32_t r0 = k0, r1 = k1;
#ifdef __HIP_DEVICE_COMPILE__
        asm volatile("" : "+s"(r0), "+s"(r1));
#endif
        uint32_t a0 = xor3(v.hi[b], (uint32_t)q1, r0);  // round 2's n0
        uint32_t a1, a2, a3;
        r0 += kPhiloxW0;
        {   // round 3
            const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
            a0 = xor3((uint32_t)(q2 >> 32), v.lo[b], r0);
            a2 = xor3((uint32_t)(p0 >> 32), c3, r1);
            a1 = (uint32_t)q2;
            a3 = (uint32_t)p0;
            r0 += kPhiloxW0;
            r1 += kPhiloxW1;
        }
#pragma unroll
        for (int r = 3; r < 10; ++r) {
            const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
            const uint64_t p1 = (uint64_t)kPhiloxM1 * a2;
            a0 = xor3((uint32_t)(p1 >> 32), a1, r0);
            a2 = xor3((uint32_t)(p0 >> 32), a3, r1);
            a1 = (uint32_t)p1;
            a3 = (uint32_t)p0;
            r0 += kPhiloxW0;
            r1 += kPhiloxW1;
        }
        o[b] = U4{{a0, a1, a2, a3}};
    }
    return U4x2{o[0], o[1]};
}

// One block of the pair by itself: draw2's arithmetic for block b alone, the three rounds it
// shares with the other block included, from the key and the four words of the quad that the
// block depends on: e1, PairInv's c3 and the block's hi / lo. The state-only step draws FUEL
// this way when its GATE words come from the wave's pool (step_seq.h), and a pool refill draws
// GATE this way for another lane's quad, whose four words (GateSeed) came through LDS. The words
// are those of draw(k, t, slot) bit for bit (tools/philox_gate_pool_check.cpp, on the host).
struct GateSeed {
    uint32_t c3, hi, lo, e1;  // PairInv's c3, hi[1], lo[1] and the key's e1
};

__host__ __device__ __forceinline__ U4 draw_half(uint32_t k0, uint32_t k1, uint32_t e1, uint32_t vc3, uint32_t hi,
                                                 uint32_t lo, uint32_t t) {
    // rounds 1-3, the common parts (as in draw2)
    const uint64_t q1 = (uint64_t)kPhiloxM1 * t;
    const uint32_t n0 = xor3((uint32_t)(q1 >> 32), e1, k0);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
    const uint64_t q0 = (uint64_t)kPhiloxM0 * n0;
    const uint32_t n2 = xor3((uint32_t)(q0 >> 32), vc3, k1);
    const uint32_t c3 = (uint32_t)q0;
    k1 += kPhiloxW1;
    const uint64_t q2 = (uint64_t)kPhiloxM1 * n2;
    uint32_t r0 = k0, r1 = k1;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+s"(r0), "+s"(r1));
#endif
    uint32_t a0 = xor3(hi, (uint32_t)q1, r0);  // round 2's n0
    uint32_t a1, a2, a3;
    r0 += kPhiloxW0;
    {   // round 3
        const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
        a0 = xor3((uint32_t)(q2 >> 32), lo, r0);
        a2 = xor3((uint32_t)(p0 >> 32), c3, r1);
        a1 = (uint32_t)q2;
        a3 = (uint32_t)p0;
        r0 += kPhiloxW0;
        r1 += kPhiloxW1;
    }
#pragma unroll
    for (int r = 3; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * a2;
        a0 = xor3((uint32_t)(p1 >> 32), a1, r0);
        a2 = xor3((uint32_t)(p0 >> 32), a3, r1);
        a1 = (uint32_t)p1;
        a3 = (uint32_t)p0;
        r0 += kPhiloxW0;
        r1 += kPhiloxW1;
    }
    return U4{{a0, a1, a2, a3}};
}

__host__ __device__ __forceinline__ U4 draw_fuel(const Key& k, const PairInv& v, uint32_t t) {
    return draw_half(k.k0, k.k1, k.e1, v.c3, v.hi[0], v.lo[0], t);
}

__host__ __device__ __forceinline__ GateSeed gate_seed(const Key& k, const PairInv& v) {
    return GateSeed{v.c3, v.hi[1], v.lo[1], k.e1};
}

// the GATE block of the quad whose seed is g, at counter t, under the key (k0, k1)
__host__ __device__ __forceinline__ U4 draw_gate_pooled(uint32_t k0, uint32_t k1, const GateSeed& g, uint32_t t) {
    return draw_half(k0, k1, g.e1, g.c3, g.hi, g.lo, t);
}

// The key schedule of one launch: the key words of rounds 1-10, k0 + r W0 and k1 + r W1 at
// index r. The seed is the same for every env of a launch, so the fused sequence's state-only
// steps fill it once before the group loop and keep it in vector registers (pin_schedule: as
// scalars the schedule spilled, which is why philox10 and draw_half recompute it per block).
// A draw that reads it has no key add at all, and a v_bitop3_b32 of three VGPRs needs no copy.
struct KeySched {
    uint32_t k0[10], k1[10];
};
// opaque vector registers: the compiler neither folds the words back into scalar adds nor
// rematerialises them inside the step loop
__device__ __forceinline__ void pin_schedule(KeySched& s) {
#pragma unroll
    for (int r = 0; r < 10; ++r) asm volatile("" : "+v"(s.k0[r]), "+v"(s.k1[r]));
}

__host__ __device__ __forceinline__ KeySched key_schedule(uint32_t k0, uint32_t k1) {
    KeySched s;
    for (int r = 0; r < 10; ++r) {
        s.k0[r] = k0 + (uint32_t)r * kPhiloxW0;
        s.k1[r] = k1 + (uint32_t)r * kPhiloxW1;
    }
    return s;
}

// draw(k, t, slot) with the key words read from the schedule of (k.k0, k.k1): philox10's rounds
// without its key adds. For the state-only step's rare whole-block draws (LOSS_r, ARRIVE).
__host__ __device__ __forceinline__ U4 draw_sched(const KeySched& s, const Key& k, uint32_t t, uint32_t slot) {
    uint32_t c0 = k.e0, c1 = k.e1, c2 = t, c3 = slot;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, s.k0[r]);
        const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, s.k1[r]);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return U4{{c0, c1, c2, c3}};
}

// draw_half with the key words read from the schedule: the same rounds, no key add.
__host__ __device__ __forceinline__ U4 draw_half_sched(const KeySched& s, uint32_t e1, uint32_t vc3, uint32_t hi,
                                                       uint32_t lo, uint32_t t) {
    // rounds 1-3, the common parts (as in draw2)
    const uint64_t q1 = (uint64_t)kPhiloxM1 * t;
    const uint32_t n0 = xor3((uint32_t)(q1 >> 32), e1, s.k0[0]);
    const uint64_t q0 = (uint64_t)kPhiloxM0 * n0;
    const uint32_t n2 = xor3((uint32_t)(q0 >> 32), vc3, s.k1[1]);
    const uint32_t c3 = (uint32_t)q0;
    const uint64_t q2 = (uint64_t)kPhiloxM1 * n2;
    uint32_t a0 = xor3(hi, (uint32_t)q1, s.k0[1]);  // round 2's n0
    uint32_t a1, a2, a3;
    {   // round 3
        const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
        a0 = xor3((uint32_t)(q2 >> 32), lo, s.k0[2]);
        a2 = xor3((uint32_t)(p0 >> 32), c3, s.k1[2]);
        a1 = (uint32_t)q2;
        a3 = (uint32_t)p0;
    }
#pragma unroll
    for (int r = 3; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * a0;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * a2;
        a0 = xor3((uint32_t)(p1 >> 32), a1, s.k0[r]);
        a2 = xor3((uint32_t)(p0 >> 32), a3, s.k1[r]);
        a1 = (uint32_t)p1;
        a3 = (uint32_t)p0;
    }
    return U4{{a0, a1, a2, a3}};
}

__host__ __device__ __forceinline__ U4 draw_fuel_sched(const KeySched& s, const Key& k, const PairInv& v, uint32_t t) {
    return draw_half_sched(s, k.e1, v.c3, v.hi[0], v.lo[0], t);
}

// the GATE block of the quad whose seed is g, at counter t, under the schedule's key
__host__ __device__ __forceinline__ U4 draw_gate_pooled_sched(const KeySched& s, const GateSeed& g, uint32_t t) {
    return draw_half_sched(s, g.e1, g.c3, g.hi, g.lo, t);
}

// integer uniform on [0, m): high word of r * m (bias < m / 2^32)
__device__ __forceinline__ int32_t uniform_int(uint32_t r, uint32_t m) {
    return (int32_t)__umulhi(r, m);
}

// port index uniform over the P-1 ports other than `other`
__device__ __forceinline__ int32_t pick_other(uint32_t r, int32_t P, int32_t other) {
    const int32_t k = uniform_int(r, (uint32_t)(P - 1));
    return k + (k >= other ? 1 : 0);
}

}  // namespace shipenv
