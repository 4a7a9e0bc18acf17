// step_lean.h — the state-only step's action decode and fuel update (step_seq.h,
// step_group_state), as host + device helpers: tools/step_lean_check.cpp compares them on the
// host with the forms they replaced (the error cascade's terms, the select of -scale / -0.0).
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

}  // namespace shipenv
