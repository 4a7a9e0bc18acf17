#pragma once
// env_core.h — one step of one env, compiled for the device and for the host
// (se_host_step_replay, the server wave): Ship, load_ship / store_ship, EnvArgs, env_key,
// needs_gate, Pending, env_begin / env_finish, replay_env, beta_part, decode_agent, reset_ship.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld and its lookups, mul24i, sqrt_rn) and philox.h.

// ------------------------------------------------------------------ one env
struct Ship {
    int x, y;
    double fuel;
    int cargo, origin, dest;  // origin/dest: SE_NONE = None
};

// Env i's ship out of the bound state, and back into it (the six fields, nothing else).
__host__ __device__ __forceinline__ Ship load_ship(const se_state& st, int64_t i) {
    return Ship{st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i]};
}

__host__ __device__ __forceinline__ void store_ship(const se_state& st, int64_t i, const Ship& s) {
    st.x[i] = (uint8_t)s.x;
    st.y[i] = (uint8_t)s.y;
    st.fuel[i] = s.fuel;
    st.cargo[i] = s.cargo;
    st.origin[i] = (uint8_t)s.origin;
    st.dest[i] = (uint8_t)s.dest;
}

// What the argument block of every kernel outside the step family opens with: the world, the
// batch, the draw key and the bound state (host.h's env_args fills it from an se_env). A kernel's
// own arguments derive from it.
struct EnvArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n, env_base;
    uint64_t seed;
    se_state st;
};

__device__ __forceinline__ Key env_key(uint64_t seed, int64_t env) {
    Key k;
    k.k0 = (uint32_t)seed;
    k.k1 = (uint32_t)(seed >> 32);
    k.e0 = (uint32_t)(uint64_t)env;
    k.e1 = (uint32_t)((uint64_t)env >> 32);
    return k;
}

// 32-bit uniform in [0, 1): u = w * 2^-32 (exact in f64)
__device__ __forceinline__ double u32(uint32_t w) { return (double)w * (1.0 / 4294967296.0); }

// Loss type on the LOSS word w (u = w * 2^-32, :180-188): u < 0.1 <=> w < kTypeLo,
// u > 0.9 <=> w > kTypeHi. Both products by 2^32 are exact and not integers.
constexpr uint32_t kTypeLo = (uint32_t)(0.1 * 4294967296.0) + 1u;  // 429496730
constexpr uint32_t kTypeHi = (uint32_t)(0.9 * 4294967296.0);       // 3865470566
static_assert(0.1 * 4294967296.0 != (double)(uint32_t)(0.1 * 4294967296.0), "bound is an integer");
static_assert(0.9 * 4294967296.0 != (double)(uint32_t)(0.9 * 4294967296.0), "bound is an integer");
enum LossKind : int { kLossNone = 0, kLossPartial = 1, kLossTotal = 2 };

// sqrt of a non-negative integer, correctly rounded (np.sqrt on the int sum of
// squares, shipping/util.py:4). Unit moves take the exact fast path.
__host__ __device__ __forceinline__ double int_sqrt_rn(int v) {
    return v == 1 ? 1.0 : sqrt_rn((double)v);
}

// Does this env's step draw a gate that can change anything? (a MOVE that passes
// its checks with 0 < cargo < 50; cargo 0 never loses, cargo >= 50 always fires)
template <bool kUnitMoves>
__device__ __forceinline__ bool needs_gate(const LdsWorld& w, const Ship& s, int type, int a, int b) {
    if (kUnitMoves) {
        const int nx = s.x + a, ny = s.y + b;
        return (type == 1) & (s.dest != SE_NONE) & ((unsigned)nx < (unsigned)w.H) &
               ((unsigned)ny < (unsigned)w.W) & (s.cargo > 0) & (s.cargo < 50);
    }
    return (type == 1) & (s.cargo > 0) & (s.cargo < 50);  // typed form: draw whenever possible
}

// One env's step between its two halves.
struct Pending {
    double r;     // reward so far, in the reference's add order
    int e;        // SE_ERR_*
    bool mv;      // a MOVE that passed its checks (:276-284)
    bool moved;   // ... and left its cell (not blocked by ground, :293-300)
    bool fires;   // the cargo-loss gate fired (:318-323)
    bool arrive;  // the move ends on the destination port (:325)
    bool dead;    // out of fuel: the step returns done (:288-290)
};

// First half of one env's step (:359-376) for a typed action (shipping/type.py:1-5):
// everything that needs no optional draw, as selects over the three action
// families so a wave runs one straight path. On return `s` holds the state after
// the move / select / take; env_finish applies cargo loss and arrival. An error
// leaves s untouched (the reference raises before mutating: :284 before :287,
// :266-269, :342-346). The gate (:318-323, random() <= cargo/50) tests the tape's
// f64 u_gate in replay and the Philox word gw in production: w <= floor(fl(c/50)
// * 2^32) is the same test on u = w * 2^-32. Production skips the cargo-0 case (a
// firing gate then loses nothing, :180-181); replay keeps it because the reference
// still draws the loss type there (:177) and replay tracks every draw. From cargo
// 50 on the gate always fires (random() < 1 <= cargo/50); below 0 it never does
// (cargo/50 < 0 <= random()), in replay as in production.
// u_fuel: replay, the tape's f64 uniform; production, the Philox word w as a double
// (u = w * 2^-32), so 0.2 * u is one product with 0.2 * 2^-32: scaling by a power of
// two is exact, so fl(w * fl(0.2) * 2^-32) == fl(fl(0.2) * u) bit for bit.
constexpr double kFifthPerWord = 0x1.999999999999ap-35;  // fl(0.2) * 2^-32
static_assert(kFifthPerWord * 4294967296.0 == 0.2, "0.2 * 2^-32 must be exact");

// kUnitCost: the caller knows the move, if the action is one, is a unit move (distance 1: no
// square root); it follows kUnitMoves unless a caller has checked its arbitrary moves itself.
template <bool kUnitMoves, bool kReplay, bool kUnitCost = kUnitMoves>
__host__ __device__ __forceinline__ Pending env_begin(const LdsWorld& w, Ship& s, int e_in, int type, int a,
                                             int b, double u_fuel, double u_gate, uint32_t gw) {
    // --- MOVE (_move_ship :273-339)
    const bool no_dest = s.dest == SE_NONE;                                      // :276
    const bool big = !kUnitMoves & ((a < -256) | (a > 256) | (b < -256) | (b > 256));  // surely OOB
    const int nx = s.x + (big ? 0 : a), ny = s.y + (big ? 0 : b);
    const bool oob = big | ((unsigned)nx >= (unsigned)w.H) | ((unsigned)ny >= (unsigned)w.W);  // :284
    const bool mv_ok = !no_dest & !oob;
    const int cx = mv_ok ? nx : s.x, cy = mv_ok ? ny : s.y;  // in-range cell for the lookups
    // fuel cost (:103-104): dist * (1 + uniform(-0.1, 0.1)), uniform = -0.1 + 0.2*u, unfused
    const double fifth_u = kReplay ? 0.2 * u_fuel : u_fuel * kFifthPerWord;
    const double scale = 1.0 + (-0.1 + fifth_u);
    const double cost = kUnitCost ? scale : int_sqrt_rn(big ? 1 : a * a + b * b) * scale;
    const bool out_of_fuel = s.fuel < cost;  // :288-290
    const bool ground = w.is_ground(cx, cy);  // :293: blocked (-5) or moved (-0.0001 then -1)
    const int mx = ground ? s.x : cx, my = ground ? s.y : cy;
    // :307-315 old cell vs ATTEMPTED cell; sqrt is monotone and the squared
    // distances are small integers, so comparing them is exact
    const int dcl = no_dest ? 0 : s.dest;
    const int px = w.px(dcl), py = w.py(dcl);
    const int d_old = mul24i(s.x - px, s.x - px) + mul24i(s.y - py, s.y - py);  // |d| < 256
    const int d_new = mul24i(cx - px, cx - px) + mul24i(cy - py, cy - py);
    const bool closer = d_old > d_new;

    // --- SELECT_PORT (_select_port :265-271); an agent index always names a port in range
    const int e_same = s.origin == a ? SE_ERR_SAME_PORT : SE_ERR_OK;
    const int e_sel = (!kUnitMoves & ((a < 0) | (a >= w.P))) ? SE_ERR_PORT_RANGE : e_same;
    // --- TAKE_FUEL / TAKE_CARGO (:341-357)
    const int idx = w.port_at(s.x, s.y);
    const int sidx = idx < 0 ? 0 : idx;
    const int2 st2 = w.stock[sidx];
    const int stock = type == 4 ? st2.y : st2.x;
    const int e_amount = ((a <= 0) | (a > stock)) ? SE_ERR_AMOUNT : SE_ERR_OK;
    const int e_take = idx < 0 ? SE_ERR_NOT_AT_PORT : e_amount;
    const int e_oob = oob ? SE_ERR_OOB : SE_ERR_OK;
    const int e_move = no_dest ? SE_ERR_NO_DEST : e_oob;

    // Every ternary below has named values as arms: clang emits a nested or
    // computing arm as control flow, which becomes a divergent branch.
    // :373-374; an agent index always decodes to a category in 1..4
    const int e4 = (kUnitMoves | (type == 3) | (type == 4)) ? e_take : SE_ERR_BAD_CATEGORY;
    const int e3 = type == 2 ? e_sel : e4;
    const int e2 = type == 1 ? e_move : e3;
    const int e1 = w.P == 0 ? SE_ERR_NO_PORTS : e2;  // :360
    Pending p;
    p.e = e_in != SE_ERR_OK ? e_in : e1;  // the decode runs before env.step (agents/dqn.py:286-287)
    const bool ok = p.e == SE_ERR_OK;
    const bool do_move = ok & (type == 1);

    const int ci = ((s.cargo > 0) & (s.cargo < 50)) ? s.cargo : 0;
    bool fires;
    if constexpr (kReplay) {
        const double lk = w.likelihood(ci);
        // cargo < 0: random() <= cargo / 50 is false for every draw (u_gate 0.0 included),
        // and ci = 0 above stands for cargo 0 only
        fires = (s.cargo >= 50) | ((s.cargo >= 0) & (u_gate <= lk));
    } else {
        const uint32_t thr = w.gate_thr[ci];
        fires = (s.cargo >= 50) | ((s.cargo > 0) & (gw <= thr));
    }

    p.mv = do_move;
    p.moved = do_move & !ground;
    p.fires = do_move & fires;
    p.arrive = do_move & (mx == px) & (my == py);
    p.dead = do_move & out_of_fuel;
    const bool take_fuel = ok & (type == 3), take_cargo = ok & (type == 4);
    // reward before loss / arrival from the table the host summed in the reference's order
    const int r_move = ((int)out_of_fuel << 2) | ((int)ground << 1) | (int)closer;
    const int r_other = (take_fuel | take_cargo) ? 8 : 9;
    p.r = w.rtab[do_move ? r_move : r_other];
    s.x = do_move ? mx : s.x;
    s.y = do_move ? my : s.y;
    const double burnt = s.fuel - cost, filled = s.fuel + (double)a;
    const double fuel_mv = (do_move & !ground) ? burnt : s.fuel;  // moves and takes exclude
    s.fuel = take_fuel ? filled : fuel_mv;
    const int loaded = s.cargo + a;
    s.cargo = take_cargo ? loaded : s.cargo;
    s.dest = (ok & (type == 2)) ? a : s.dest;
    return p;
}

// int(beta * cargo) (:195-197) for beta = m * 2^-32 (production: m the median word).
// While m * cargo < 2^53 the f64 product is exact, and scaling by 2^-32 is too, so
// the truncation is the high word of the 64-bit product: one v_mul_hi_u32 in place
// of three conversions and a multiply. Larger cargo takes the f64 path.
__device__ __forceinline__ int beta_part(uint32_t m, int cargo) {
    const int hi = (int)__umulhi(m, (uint32_t)cargo);
    const int f = (int)(((double)m * (1.0 / 4294967296.0)) * (double)cargo);
    return cargo < (1 << 21) ? hi : f;
}

// Second half: cargo loss (_calculate_cargo_loss :169-200) of kind none / partial
// (part = int(beta * cargo), :195-197) / total, then arrival (:325-337) with the
// redrawn destination. Selects only.
__host__ __device__ __forceinline__ void env_finish(Ship& s, Pending& p, int kind, int part, int new_dest,
                                           bool fires, bool arrive) {
    const int some = kind == kLossTotal ? s.cargo : part;
    const int loss = kind == kLossNone ? 0 : some;
    const double rl = p.r + (double)(-3 * loss);
    const int kept = s.cargo - loss;
    p.r = fires ? rl : p.r;
    s.cargo = fires ? kept : s.cargo;
    const double ra = (p.r + (double)(2 * s.cargo)) + 10.0;
    p.r = arrive ? ra : p.r;
    s.cargo = arrive ? 0 : s.cargo;
    const int dest = s.dest;
    s.dest = arrive ? new_dest : dest;
    s.origin = arrive ? dest : s.origin;
}

// utils/preprocessing.py:111-137 (moves N, E, S, W; Python wraps -4..-1), in
// integer arithmetic: the compiler turns nested ternaries into divergent branches.
//   act < 4: MOVE k = act & 3, N (0,-1) E (-1,0) S (0,1) W (1,0)
//   [4, 4+P): SELECT_PORT act-4   [4+P, 54+P): TAKE_CARGO   [54+P, ...): TAKE_FUEL
__device__ __forceinline__ int decode_agent(int P, int act, int& type, int& a, int& b) {
    const int k = act & 3;  // -4..-1 -> 0..3 like Python's negative list index
    const int move = act < 4, sel = act < 4 + P, cargo = act < 54 + P;
    type = move ? 1 : 3 + cargo - 2 * sel;
    const int val = act - 4 - (1 - sel) * P - (1 - cargo) * 50;
    const int odd = k & 1;
    const int dx = odd * (k - 2);   // EAST = (-1, 0), WEST = (1, 0)
    a = move ? dx : val;
    b = move * (1 - odd) * (k - 1);  // NORTH = (0, -1), SOUTH = (0, 1)
    return act < -4 ? SE_ERR_BAD_INDEX : SE_ERR_OK;
}

// One env's replayed step (se_step_replay; se_host_step_replay runs the same code on the
// host): the reference's draws come from the tape record tp (uf / ug its u_fuel / u_gate,
// read by the caller). Returns the SE_USED_* bits of the draws the reference made. A
// variate the step needs but the record lacks (NaN, arrive_dest < 0) leaves the env
// untouched with SE_ERR_NEED_DRAW, reward 0 and done 0.
__host__ __device__ __forceinline__ uint32_t replay_env(const LdsWorld& w, Ship& s, Pending& p, int er, int ty,
                                                        int va, int vb, double uf, double ug,
                                                        const se_tape* tp) {
    const Ship s0 = s;
    p = env_begin<false, true>(w, s, er, ty, va, vb, uf, ug, 0u);
    uint32_t used = p.mv ? (kUsedFuelGate | (p.moved ? kUsedMoved : 0u)) : 0u;
    bool need = p.mv && (uf != uf || ug != ug);
    int kind = kLossNone, nd = 0;
    double beta = 0.0;
    if (p.fires) {
        used |= kUsedLossType;
        const double lt = tp->u_type;
        const bool partial = s.cargo != 0 && lt >= 0.1 && lt <= 0.9;
        if (partial) {
            used |= kUsedBeta;
            beta = tp->beta;
        }
        need = need || lt != lt || (partial && beta != beta);
        kind = lt < 0.1 ? kLossNone : (lt > 0.9 ? kLossTotal : kLossPartial);
    }
    if (p.arrive) {
        used |= kUsedArrive;
        nd = tp->arrive_dest;
        need = need || nd < 0;
    }
    env_finish(s, p, kind, (int)(beta * (double)s.cargo), nd, p.fires, p.arrive);
    if (need) {  // ask the caller for the next variate; change nothing
        s = s0;
        p.r = 0.0;
        p.dead = false;
        p.e = SE_ERR_NEED_DRAW;
    }
    return used;
}

// reset (:227-243) from two Philox words
__device__ __forceinline__ void reset_ship(const LdsWorld& w, Ship& s, uint32_t r0, uint32_t r1) {
    s.origin = uniform_int(r0, (uint32_t)w.P);
    s.dest = pick_other(r1, w.P, s.origin);
    s.cargo = 0;
    s.fuel = kFuelInit;
    s.x = w.px(s.origin);
    s.y = w.py(s.origin);
}

// number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t count_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
