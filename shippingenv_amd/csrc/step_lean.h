// step_lean.h — the state-only step's action decode and fuel update (step_seq.h,
// step_group_state), as host + device helpers: tools/step_lean_check.cpp compares them on the
// host with the forms they replaced (the error cascade's terms, the select of -scale / -0.0),
// and tools/step_trim_check.cpp the move test on val, the fuel scale's FMA and the GATE pool's
// window choice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shipenv {

// The state-only step needs two bits of an agent action, not which error a bad one raises:
// does the ship try to move, and does a SELECT pass. Both are unsigned range compares, so
// nothing overflows at the int32 ends.
//   move:   -4 <= act < 4 in a world with ports (P == 0: every action is an error), with a
//           destination, and the target inside the map;
//   select: 4 <= act < 4 + P (which implies P != 0) of a port other than the origin.
__host__ __device__ __forceinline__ bool lean_do_move(int act, int P, bool nodest, bool inb) {
    const bool is_mv = (uint32_t)act + 4u < (P != 0 ? 8u : 0u);
    return is_mv & !nodest & inb;
}
// The move test on val = act - 4, which the step has for SELECT anyway: -4 <= act < 4 is
// val in [-8, -1], as unsigned above 0xFFFFFFF7 (act -> act - 4 is a bijection mod 2^32, so this
// holds at the int32 ends too). With the bound 0xFFFFFFFF in a world without ports nothing is
// above it: the bound depends on the world alone, so the step computes it once per launch and
// the test is one compare, without lean_do_move's add and its `P != 0` mask.
__host__ __device__ __forceinline__ uint32_t lean_move_bound(int P) {
    return P != 0 ? 0xFFFFFFF7u : 0xFFFFFFFFu;
}
__host__ __device__ __forceinline__ bool lean_do_move_val(int val, uint32_t bound, bool nodest, bool inb) {
    const bool is_mv = (uint32_t)val > bound;
    return is_mv & !nodest & inb;
}
__host__ __device__ __forceinline__ bool lean_sel_ok(int act, int P, bool same) {
    const bool is_sel = (uint32_t)act - 4u < (uint32_t)P;
    return is_sel & !same;
}

// fuel - (moved ? scale : 0) with the bits of fuel + (moved ? -scale : -0.0): (-scale) * 1 is
// exact, so the FMA rounds fuel - scale once, as the add did; (-scale) * 0 is -0.0 (scale > 0),
// and fuel + -0.0 is the add of a ship that stays. The one explicit FMA of a build that
// contracts nothing.
__host__ __device__ __forceinline__ double lean_fuel(double fuel, double scale, bool moved) {
    return __builtin_fma(-scale, moved ? 1.0 : 0.0, fuel);
}

// The fuel cost's scale 1.0 + (-0.1 + (double)w * fifth), fifth = fl(0.2) * 2^-32
// (env_core.h, kFifthPerWord), with the product and the inner add as one FMA: for every one of
// the 2^32 words the FMA's single rounding gives the bits of the two roundings
// (tools/step_trim_check.cpp compares all of them). The outer add stays an add: fma(w, fifth,
// 0.9) differs for 858,993,459 words. The second explicit FMA of the build.
__host__ __device__ __forceinline__ double lean_fuel_scale(uint32_t w, double fifth) {
    return 1.0 + __builtin_fma((double)w, fifth, -0.1);
}

// The GATE pool's window for a wave with m carrier lanes (step_seq.h): log2 of W, the largest
// power of two <= 8 with m W <= 64, the pool's entries per wave. 8 steps for m <= 8, 4 for
// m <= 16; beyond 16 carriers (where the kernel draws directly) 2.
__host__ __device__ __forceinline__ uint32_t gate_window_log2(uint32_t m) {
    return m <= 8 ? 3u : m <= 16 ? 2u : 1u;
}

}  // namespace shipenv
