// step_lean.h — the state-only step's action decode and fuel update (step_seq.h,
// step_group_state), as host + device helpers: tools/step_lean_check.cpp compares them on the
// host with the forms they replaced (the error cascade's terms, the select of -scale / -0.0),
// tools/step_trim_check.cpp the move test on val, the fuel scale's FMA and the GATE pool's
// window choice, tools/step_ring_check.cpp the regular step's decode on the bordered cell
// table with the general form's, tools/step_screen_check.cpp the GATE pool's screen, and
// tools/step_addr_check.cpp the carried cell address with the packed position.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
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

// The bordered cell table of the regular state-only step (step_seq.h, step_group_ring): the
// map's cell codes with one ring of kRingBorder around them, (H + 2) x (W + 2) bytes, so the
// target of any unit move from a cell of the map is a byte of the table and "off the map" is a
// cell code like ground. A position is carried biased by one in both halves, (x + 1) | (y + 1)
// << 16: its index in the table is (x + 1) (W + 2) + (y + 1), one dot product against
// (W + 2) | 1 << 16, and v_pk_add_u16 of a unit move never wraps (x + 1 - 1 >= 0).
// kRingBorder is 254: with kCellGround at 255, port 253's code in a world of 254 ports. So the
// table exists for P <= kRingMaxPorts only, and only where the launch's LDS with it keeps four
// workgroups on a CU (kRingLdsPerBlock: a quarter of the CU's 160 KiB), which is the launch's
// occupancy without it.
constexpr uint32_t kRingBorder = 254;
constexpr uint32_t kRingGround = 255;  // world.h's kCellGround
constexpr int kRingMaxPorts = 253;
constexpr size_t kRingLdsPerBlock = 160 * 1024 / 4;
constexpr uint32_t kRingBias = 0x00010001u;

// bytes of the table, in whole 16-byte units (it is staged by 16-byte loads)
__host__ __device__ __forceinline__ uint32_t ring_table_bytes(int H, int W) {
    return ((uint32_t)(H + 2) * (uint32_t)(W + 2) + 15u) & ~15u;
}
// Does a launch whose other LDS is `lds_without` bytes carry the table?
__host__ __device__ __forceinline__ bool ring_table_fits(int H, int W, int P, size_t lds_without) {
    return P <= kRingMaxPorts && lds_without + ring_table_bytes(H, W) <= kRingLdsPerBlock;
}
// The table of an H x W map's cell codes (cell[x * W + y]) into ring_table_bytes(H, W) bytes;
// the bytes past the last row are zero.
__host__ __forceinline__ void ring_table_build(int H, int W, const uint8_t* cell, uint8_t* out) {
    const uint32_t n = ring_table_bytes(H, W);
    for (uint32_t i = 0; i < n; ++i) out[i] = i < (uint32_t)(H + 2) * (uint32_t)(W + 2) ? (uint8_t)kRingBorder : 0;
    for (int x = 0; x < H; ++x)
        for (int y = 0; y < W; ++y) out[(size_t)(x + 1) * (size_t)(W + 2) + (size_t)(y + 1)] = cell[(size_t)x * W + y];
}
// x | y << 16 (x, y < 256) to the biased form and back: no carry crosses the halves
__host__ __device__ __forceinline__ uint32_t ring_bias(uint32_t p) { return p + kRingBias; }
__host__ __device__ __forceinline__ uint32_t ring_unbias(uint32_t bp) { return bp - kRingBias; }
// index of a biased position (or of a unit move's target from one) in the table
__host__ __device__ __forceinline__ uint32_t ring_index(uint32_t bp, int W) {
    return (bp & 0xffffu) * (uint32_t)(W + 2) + (bp >> 16);
}
// The regular step's decode from the target's code in the bordered table: a move that passed
// its checks (the target is on the map; an env of a regular wave has a destination), and one
// that changes the position (the target is no ground either). A move off the map is an error
// and draws no gate; a move blocked by ground is a move.
__host__ __device__ __forceinline__ bool ring_do_move(int val, uint32_t bound, uint32_t code) {
    return ((uint32_t)val > bound) & (code != kRingBorder);
}
__host__ __device__ __forceinline__ bool ring_moved(int val, uint32_t bound, uint32_t code) {
    return ((uint32_t)val > bound) & (code < kRingBorder);
}

// The carried cell address (step_seq.h, step_group_ring<kAddr>). A regular wave's inner steps read
// a ship's x and y only to make the target's index in the table again, so the position is carried
// as that index plus the table's LDS address, and a move adds one signed delta, dx (W + 2) + dy, read
// from a four-entry table that the launch derives from the image's packed moves. Up to W = 125 the
// deltas are bytes (|dx (W + 2) + dy| <= 127) and the entry's address is (act & 3) | base in one
// instruction, so the table sits at a 4-byte-aligned address, behind the bordered table
// (kRingDeltaBytes of the launch's LDS, counted where the host asks ring_table_fits). Wider maps
// keep the packed position (another instantiation of the kernel, chosen by the host).
// After the inner steps the index goes back to x + 1 | y + 1 << 16 once: a division by W + 2 as a
// multiply by ceil(2^32 / (W + 2)) and the product's high word, exact while index (W + 2) < 2^32
// (the quotient's error is below index (W + 2) / 2^32 / (W + 2)); tools/step_addr_check.cpp
// compares it with / and % for every W and every index a table of that width can hold.
constexpr size_t kRingDeltaBytes = 16;
__host__ __device__ __forceinline__ bool ring_byte_deltas(int W) { return W + 2 <= 127; }
// the delta of a packed move dx | dy << 16 (16-bit halves, -1 as 0xffff)
__host__ __device__ __forceinline__ int ring_delta(uint32_t mv, int W) {
    return (int)(int16_t)(mv & 0xffffu) * (W + 2) + (int)(int16_t)(mv >> 16);
}
__host__ __device__ __forceinline__ uint32_t ring_unindex_mul(int W) { return 0xffffffffu / (uint32_t)(W + 2) + 1u; }
// index -> the biased position (x + 1) | (y + 1) << 16; mul: ring_unindex_mul(W)
__host__ __device__ __forceinline__ uint32_t ring_unindex(uint32_t index, int W, uint32_t mul) {
    const uint32_t q = (uint32_t)(((uint64_t)index * mul) >> 32);
    return q | ((index - q * (uint32_t)(W + 2)) << 16);
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

// The window sized to the carriers: W = min(16, 64 / m) steps for 1 <= m <= 16 carrier lanes, so
// 4 <= W <= 16 and m W <= 64 (16 steps up to 4 lanes, 12, 10, 9, 8, 7, 6, 5, 5 for 5 .. 12, 4
// beyond). W is no power of two, so the pool's entries are offset-major: lane L = s m + c draws
// carrier c's block for window offset s, and the split needs L / m for a wave-uniform m. That is
// a multiply by ceil(2^16 / m) and a shift, exact for every L < 64 and m <= 16 (the quotient's
// error is below L m / 2^16 < 1 / m), so lanes at or past m W get an offset >= W and a carrier
// below m too: a valid block that nobody reads. gate_window_entry(m) packs both as
// W | ceil(2^16 / m) << 8, one constant per m (one scalar load at a refill, no division);
// m == 0 (a window without a carrier, which draws nothing): 16 | 0.
constexpr uint32_t kGatePoolLimit = 16;   // carrier lanes up to which a wave pools (W >= 4)
constexpr uint32_t kGatePoolSeeds = 32;   // seed rows per wave: the carriers' seeds, then their thresholds
constexpr uint32_t kGatePoolRow = 64 + kGatePoolSeeds;  // uint4 entries per wave: the pool's 64, then the seed rows
constexpr uint32_t kGateWindowMax = 16;
constexpr uint32_t gate_window_entry_of(uint32_t m) {
    return m == 0 ? kGateWindowMax : (64u / m < kGateWindowMax ? 64u / m : kGateWindowMax) | ((65535u / m + 1u) << 8);
}
__host__ __device__ __forceinline__ uint32_t gate_window_entry(uint32_t m) {  // m <= 16
    constexpr auto e = gate_window_entry_of;
    static constexpr uint32_t tab[17] = {e(0), e(1), e(2), e(3), e(4), e(5), e(6), e(7), e(8), e(9), e(10), e(11), e(12), e(13), e(14), e(15), e(16)};
    return tab[m];
}
__host__ __device__ __forceinline__ uint32_t gate_window_len(uint32_t entry) { return entry & 0xffu; }
// lane L's window offset s = L / m and carrier c = L - s m
__host__ __device__ __forceinline__ uint32_t gate_lane_offset(uint32_t L, uint32_t entry) { return (L * (entry >> 8)) >> 16; }
__host__ __device__ __forceinline__ uint32_t gate_lane_carrier(uint32_t L, uint32_t offset, uint32_t m) { return L - offset * m; }
// The pool entry a lane of rank `slot` reads at offset s: its own where it is a carrier (slot < m).
// Any lane's slot is at most m (the carriers below it), so the index is at most
// (W - 1) m + m = m W <= 64: inside the wave's kGatePoolRow = 96 rows (the seed rows follow the pool).
__host__ __device__ __forceinline__ uint32_t gate_pool_index(uint32_t s, uint32_t m, uint32_t slot) { return s * m + slot; }
// That bound, checked where the library is compiled: for every m the window is 4 .. 16 steps, fills
// at most the pool's 64 entries, and the entry of the last offset and the largest rank lies in the rows.
constexpr bool gate_pool_reads_in_rows() {
    for (uint32_t m = 1; m <= kGatePoolLimit; ++m) {
        const uint32_t W = gate_window_entry_of(m) & 0xffu;
        if (W < 4 || W > kGateWindowMax || m * W > 64 || (W - 1u) * m + m >= kGatePoolRow) return false;
    }
    return true;
}
// The refill's 64-bit ballot of screen_hot needs no fold with offset-major entries: step s is hot
// iff bits [s m, s m + m) hold a one. The window keeps the ballot shifted right by m per step and
// tests its low m bits (m == 0: the launch's screen_all alone, every bit of it).
__host__ __device__ __forceinline__ uint64_t gate_screen_mask(uint32_t m) { return m != 0 ? (1ull << m) - 1ull : ~0ull; }
__host__ __device__ __forceinline__ bool gate_screen_step(uint64_t shifted, uint64_t mask) { return (shifted & mask) != 0; }

// The by-code arrival test of a launch whose ports lie on distinct cells (step_seq.h,
// step_group_ring): port i's cell then carries code i + 1 and no other cell does, so a ship with
// dest < P is on its destination's cell iff the code under it is dest + 1. The launch takes the
// test only with P >= 2 (arrive_by_code_allowed): an arrival in a world of one port writes
// pick_other's 1 = P as the new dest, which the position compare clamps to port 0 and the code never equals.
__host__ __forceinline__ bool ports_on_distinct_cells(int P, const int32_t* px, const int32_t* py) {
    for (int i = 0; i < P; ++i)
        for (int k = 0; k < i; ++k)
            if (px[i] == px[k] && py[i] == py[k]) return false;
    return true;
}
__host__ __forceinline__ bool arrive_by_code_allowed(int P, bool distinct) { return distinct && P >= 2; }
__host__ __device__ __forceinline__ bool arrive_by_code(bool do_move, uint32_t code, int dst) {
    return do_move & (code == (uint32_t)dst + 1u);
}

// Entry c of the world image's gate thresholds: the gate of a ship with cargo c fires for a word
// <= floor(c / max_cargo * 2^32) (random() < cargo / 50, the quotient correctly rounded and the
// product exact), and for every word from max_cargo on. Entry 0 is 0 and the entries never fall
// as c rises, which the screen below rests on.
__host__ __forceinline__ uint32_t gate_thr_entry(int c, double max_cargo) {
    return c < (int)max_cargo ? (uint32_t)floor(ldexp((double)c / max_cargo, 32)) : 0xffffffffu;
}

// The screened GATE pool (step_seq.h). At a refill the lane that drew a carrier's block for one
// window offset compares its four words with that carrier's four thresholds as they stood at the
// vote: screen_hot. Inside a window cargo only falls (a loss or an arrival lowers it; a take ends
// the window, and its env did not move in that step), the thresholds never rise as cargo falls,
// and an env without cargo has threshold 0 and fires for no word. So a gate can fire at an offset
// only if the screen passed there: a word above its threshold at the refill stays above it.
// (A word equal to 0 passes for an env without cargo, for nothing: the screen is only wider.)
__host__ __device__ __forceinline__ bool screen_hot(const uint32_t word[4], const uint32_t thr[4]) {
    return (word[0] <= thr[0]) | (word[1] <= thr[1]) | (word[2] <= thr[2]) | (word[3] <= thr[3]);
}
// The ballot of screen_hot over the wave's 64 lanes, lane L = carrier L >> logw at offset
// L & (W - 1), W = 1 << logw, folded to one bit per window offset: the OR of the ballot's groups
// of W lanes, in bits 0 .. W - 1. The bits from W up hold partial ORs that nobody reads (a window's
// steps test bits 0 .. W - 1 only), so the kernel masks nothing. logw is gate_window_log2's, 1 .. 3.
__host__ __device__ __forceinline__ uint32_t screen_fold(uint64_t ballot, uint32_t logw) {
    uint32_t b = (uint32_t)ballot | (uint32_t)(ballot >> 32);
    b |= b >> 16;
    b |= b >> 8;
    b |= logw < 3u ? b >> 4 : 0u;
    b |= logw < 2u ? b >> 2 : 0u;
    return b;
}

}  // namespace shipenv
