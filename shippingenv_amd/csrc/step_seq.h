#pragma once
// step_seq.h — se_step_seq's fused run of steps with the state in registers:
// Carried, the state-only step_group_state and its regular form on the bordered cell table,
// step_group_ring, stock_by_code, the GATE pool, step_seq_kernel and the partial last group's
// step_tail_seq_kernel.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (the image's tables, staging), env_core.h (env_key, beta_part),
// step_io.h (StepArgs, Group, At, ld4_full / st4*_full), step_group.h (BlockStats,
// Finished), step_agent.h (the packed helpers, early_draws, step_group_agent: the
// run's last step) and step_kernel.h (step_tail_envs).

// The pieces of the pooled loop that can be compiled out, each to the form before it (A/B builds:
// SHIPENV_HIPCC_DEFINES=-DSHIPENV_SEQ_...=0; results are the same bits either way).
#ifndef SHIPENV_SEQ_WINDOW_DIV
#define SHIPENV_SEQ_WINDOW_DIV 1  // the window's length is min(16, 64 / m), its entries offset-major (0: 8 or 4 steps, carrier-major)
#endif
#ifndef SHIPENV_SEQ_CARGO_CUT
#define SHIPENV_SEQ_CARGO_CUT 1  // a window ends only after a passed take of cargo (0: after any step whose take block ran)
#endif
#ifndef SHIPENV_SEQ_ARRIVE_CODE
#define SHIPENV_SEQ_ARRIVE_CODE 1  // the regular step tests an arrival by the cell code where it may (0: by the position, always)
#endif
#ifndef SHIPENV_SEQ_CELL_ADDR
#define SHIPENV_SEQ_CELL_ADDR 1  // a regular wave of a map up to 125 wide carries the ship's cell address in the bordered table (0: the packed position, always)
#endif

// The state-only step: a step of a fused sequence before its last, for a full group, Philox
// draws, no auto-reset. Nothing can read an inner step's reward, done or err, and the next state
// needs neither the out-of-fuel flag (a dead ship keeps moving) nor which error was raised, only
// whether one was. So there is no reward, no out-of-fuel compare, and the action's checks are two
// bits. The state arithmetic, its order and every Philox counter are step_group_agent's.
// Position, origin and dest live in Carried from step to step, one register per env, so
// consecutive steps neither unpack nor pack bytes; fuel, cargo and the action are G's (of G the
// step touches f, c and a only). The cell code under the ship is carried too (after a move
// it is the byte the ground test read at the cell moved to), so a step makes one cell lookup per
// env, with the table's LDS address riding in the dot product (lds_cell). The action is decoded
// by two unsigned range compares on act - 4 (the move's against a bound computed once per launch),
// the fuel scale is one FMA and one add and the fuel update one FMA (step_lean.h); the four cell
// lookups of a step are issued together and waited for once; each env's gate
// threshold is carried and looked up again only where its cargo changes. The caller draws FUEL
// and GATE together (fb, gb: philox.h, draw2), or takes gb from its wave's GATE pool and lets
// `late` draw FUEL (below). The ranked LOSS draw is step_group_agent's, line
// for line: as a shared helper it compiled to another instruction order in both steps.
// The take and the arrival test run only for a wave that needs them (two ballots per step,
// scalar branches). Ships are mostly at sea, so most wave-steps run neither
// (profiles/seq_guard/freq.json). The result says whether the take block ran (wave-uniform): the
// only place where an env's cargo can become positive, which the caller's GATE pool needs.
struct Carried {
    uint32_t pos[4];  // x | y << 16; in a regular wave (step_group_ring) biased: x + 1 | y + 1 << 16, or (kAddr) the LDS
                      // address of the ship's cell in the bordered table: ring0 + (x + 1) (W + 2) + (y + 1)
    int org[4], dst[4];
    uint32_t code[4];   // the cell code under the ship, w.cell[cell_of(pos)]
    bool near;          // step_group_ring: some env of the wave is on a non-water cell (wave-uniform)
    bool bycode;        // step_group_ring: the wave tests an arrival by the cell code (wave-uniform, set where Carried is filled)
    uint32_t thr[4];    // the gate threshold of the env's cargo, gate_thr_of(w, cargo)
    const int2* take;   // the block's stocks by cell code (stock_by_code), the same for every env
};
// Carried::thr. Cargo changes in three places only, all rare and each behind a branch (a passed
// take, a loss, an arrival), so the threshold is looked up there and where Carried is filled, and
// the gate test of every step reads a register. Entry 0 is 0, which a word can equal: the test
// keeps its cargo > 0.
__device__ __forceinline__ uint32_t gate_thr_of(const LdsWorld& w, int cargo) {
    return w.gate_thr[min(max(cargo, 0), 50)];
}
// The launch's invariants of the state-only steps: the Philox key schedule in vector registers
// (philox.h; the pooled loop's FUEL draw, a pool refill and the rare LOSS_r / ARRIVE draws read
// it, so they compute no key add) and the move test's bound (step_lean.h), a scalar.
// kSched = false (the kernel without the pool, whose draw2 keeps its scalar keys and which has no
// 20 registers to spare under 128): no schedule, the rare draws are draw()'s.
template <bool kSched>
struct SeqInv {
    KeySched ks;
    uint32_t move_bound;
    uint32_t ring0;  // the bordered cell table's LDS address (step_group_ring)
    uint32_t delta0; // the move deltas' LDS address, 4-byte aligned (step_group_ring<kAddr>)
    __device__ __forceinline__ U4 block(const Key& qk, uint32_t t, uint32_t slot) const {
        if constexpr (kSched) return draw_sched(ks, qk, t, slot);
        else return draw(qk, t, slot);
    }
};
// `late` runs after the take block and may set fb: the pooled kernel draws FUEL there and pins
// the words, which keeps the draw out of the step's last block and, as it happens, cargo and fuel
// in their registers across the take block (drawn before the call the loop had 10 VALU more, 7
// of them copies where the skipped take block's path joins: profiles/seq_gatepool/isa.json).
struct NoLateDraw {
    __device__ __forceinline__ void operator()(U4&) const {}
};
template <bool kNt, bool kSched, typename Late = NoLateDraw>
__device__ __forceinline__ bool step_group_state(const LdsWorld& w, const SeqInv<kSched>& I, const Key& qk, uint32_t t, U4 fb,
                                                 const U4& gb, Group<false, false, kNt>& G, Carried& U, Late late = Late{}) {
    const int P = w.P;
    const uint32_t lim = (uint32_t)(w.H - 1) | ((uint32_t)(w.W - 1) << 16);
    const uint32_t wh = (uint32_t)w.W | (1u << 16);
    const uint32_t pm1 = P > 0 ? (uint32_t)(P - 1) : 0u;  // clamp for table reads whose value an error discards
    // The take guard. A take passes only for a ship on a port cell, so a wave none of whose
    // envs has a take action on a non-water cell (code != 0: wider than "a port's code", so
    // ground and codes past P only send their wave here) skips the whole take: the stock
    // read, the amount checks, the cargo add and the fuel's f64 conversion. The vote is a
    // ballot, so the branch is scalar; it reads this step's actions and the codes before
    // the move. A passed take changes only cargo and fuel, and its env neither moves nor
    // selects, so it is applied here and the step below runs without it: cargo is what the
    // full step's `tc_ok ? cargo + amount : cargo` gives, and fuel reaches the fuel update as
    // fuel + amount, to which that update adds -0.0, which changes no bit of any value.
    bool take_any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) take_any |= (G.a[j] >= 4 + P) & (U.code[j] != 0);
    const bool take_ran = __builtin_amdgcn_ballot_w64(take_any) != 0;
    if (take_ran) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int act = G.a[j];
            const bool lt_tc = act < 54 + P;
            const int amount = act - (lt_tc ? 4 + P : 54 + P);
            // the stocks by the carried cell code, zero off a port: 0 < amount <= stock
            // then holds at a port with the stock only (and never when P == 0)
            const int2 st2 = U.take[U.code[j]];
            const int stock = lt_tc ? st2.y : st2.x;
            const bool ok_take = (act >= 4 + P) & (amount > 0) & (amount <= stock);
            G.c[j] = (ok_take & lt_tc) ? G.c[j] + amount : G.c[j];
            G.f[j] = (ok_take & !lt_tc) ? G.f[j] + (double)amount : G.f[j];
            U.thr[j] = gate_thr_of(w, G.c[j]);
        }
    }
    late(fb);
    uint32_t pos[4], cp[4], code_cp[4];
    int dst[4], cg[4];
    bool do_move[4], moved[4], inb[4], nodest[4];
    // MOVE (_move_ship :273-339): the four cell lookups first, so their LDS reads are in flight
    // together and a wave waits for one latency, not four
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t dxy = w.moves[G.a[j] & 3];
        const uint32_t p = U.pos[j];
        dst[j] = U.dst[j];
        const uint32_t np = pk_add_u16(p, dxy);
        inb[j] = pk_min_u16(np, lim) == np;  // _is_within_map (:284); -1 wraps to 0xffff
        nodest[j] = dst[j] == SE_NONE;       // :276
        cp[j] = (!nodest[j] & inb[j]) ? np : p;  // in-range cell for the lookup
        code_cp[j] = lds_cell(lds_address(w.cell), cp[j], wh);
    }
    // carried as full registers (as bytes they are masked again before every select); pinned in
    // one statement, which is the one wait for the four reads
    asm("" : "+v"(code_cp[0]), "+v"(code_cp[1]), "+v"(code_cp[2]), "+v"(code_cp[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // [0,4) moves (-4..-1 wrap), [4, 4+P) SELECT; the takes are done
        const int act = G.a[j];
        const int val = (int)((uint32_t)act - 4u);  // the move test and a select read it
        const uint32_t p = U.pos[j];
        cg[j] = G.c[j];
        const bool ground = code_cp[j] == kCellGround;  // :293
        // step_group_agent's error cascade as the two bits the next state needs (step_lean.h):
        // a move that passed its checks, a SELECT that passed its own (mask arithmetic, no
        // ?: : a branch here would take the LDS lookups with it). A take is not among them: the
        // take guard has applied it, and nothing below reads whether a take passed.
        const bool same = U.org[j] == val;
        do_move[j] = lean_do_move_val(val, I.move_bound, nodest[j], inb[j]);
        moved[j] = do_move[j] & !ground;
        const bool sel_ok = lean_sel_ok(act, P, same);
        pos[j] = moved[j] ? cp[j] : p;
        U.code[j] = moved[j] ? code_cp[j] : U.code[j];  // the ground test's read
        dst[j] = sel_ok ? val : dst[j];
    }
    uint32_t fire = 0, arrive = 0;
    // The arrival guard. An arrival (:325) happens on a port's cell, and the world image
    // stamps every port's cell with a non-zero code, so a wave none of whose movers is on
    // a non-water cell after the move has no arrival and reads no destination position.
    // The vote is a ballot (a scalar branch) over the codes as the move left them. The
    // test itself stays the position compare: two ports may share a cell, and dest may
    // hold anything a caller loaded. (A mover selects nothing, so dst is still its dest.)
    bool arrive_any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) arrive_any |= do_move[j] & (U.code[j] != 0);
    if (__builtin_amdgcn_ballot_w64(arrive_any) != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            arrive |= (uint32_t)(do_move[j] & (pos[j] == w.pos[min((uint32_t)dst[j], pm1)])) << j;
    }
    double f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // fuel cost (:103-104); a ship that does not move adds -0.0, which leaves every value as it is
        f[j] = lean_fuel(G.f[j], lean_fuel_scale(fb.v[j], kFifthPerWord), moved[j]);
        // the gate (:318-323), as step_group_agent tests it, against the carried threshold
        const bool fires = do_move[j] & (cg[j] > 0) & (gb.v[j] <= U.thr[j]);
        fire |= (uint32_t)fires << j;
    }
    // the flags travel as opaque VGPR bit masks (no lane masks live in SGPR pairs
    // across the draw blocks below)
    asm volatile("" : "+v"(fire), "+v"(arrive));
    int org[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        org[j] = U.org[j];
        U.pos[j] = pos[j];
        G.f[j] = f[j];
    }
    // cargo loss and arrival, only in waves with a firing gate / an arrival
    if (fire) {
        uint32_t lt[4], v1[4], v2[4], v3[4];
        const uint32_t rk[4] = {0u, fire & 1u, (uint32_t)__popc(fire & 3u), (uint32_t)__popc(fire & 7u)};
        U4 rr = I.block(qk, t, loss_slot(0));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lt[j] = rr.v[0];
            v1[j] = rr.v[1];
            v2[j] = rr.v[2];
            v3[j] = rr.v[3];
        }
#pragma unroll
        for (uint32_t q = 1; q < 4; ++q) {
            if (__popc(fire) > q) {
                rr = I.block(qk, t, loss_slot(q));
#pragma unroll
                for (int j = (int)q; j < 4; ++j) {
                    const bool take = rk[j] >= q;
                    lt[j] = take ? rr.v[0] : lt[j];
                    v1[j] = take ? rr.v[1] : v1[j];
                    v2[j] = take ? rr.v[2] : v2[j];
                    v3[j] = take ? rr.v[3] : v3[j];
                }
            }
        }
        // the tail of env j only in a wave where env j of some lane fired: mostly one of the four
        // (a lane whose env j did not fire keeps its cargo, and with it the carried threshold)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (__builtin_amdgcn_ballot_w64((fire >> j) & 1u) == 0) continue;
            // beta = the median of the three words * 2^-32 (the conversion is monotone)
            const uint32_t lo = min(v1[j], v2[j]), hi = max(v1[j], v2[j]);
            const uint32_t med = max(lo, min(hi, v3[j]));  // v_med3_u32
            const int part = beta_part(med, cg[j]);
            const int some = lt[j] > kTypeHi ? cg[j] : part;
            const int loss = lt[j] < kTypeLo ? 0 : some;
            const bool fj = (fire >> j) & 1u;
            cg[j] = fj ? cg[j] - loss : cg[j];
            U.thr[j] = gate_thr_of(w, cg[j]);
        }
    }
    if (arrive) {
        const U4 ab = I.block(qk, t, kSlotArrive);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool aj = (arrive >> j) & 1u;
            const int nd = pick_other(ab.v[j], P, dst[j]);
            cg[j] = aj ? 0 : cg[j];
            U.thr[j] = gate_thr_of(w, cg[j]);
            org[j] = aj ? dst[j] : org[j];
            dst[j] = aj ? nd : dst[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        U.org[j] = org[j];
        U.dst[j] = dst[j];
        G.c[j] = cg[j];
    }
    return take_ran;
}

// The regular form of the state-only step, for a wave all of whose envs are regular: inside the
// map and with a destination. No state-only step makes a regular env irregular (a select writes a
// port's index, an arrival pick_other's result, and a move changes the position only to a cell
// of the map), so the wave's one ballot where Carried is filled holds for the whole run. The
// same next state as step_group_state, bit for bit, from less work per step:
//   * U.pos is biased by one in both halves and the one cell lookup reads the bordered table
//     (step_lean.h) at the move's target, always: the target's code says "off the map"
//     (kRingBorder: the action is an error, no gate, no arrival), "ground" (a move that stays)
//     or neither. No bounds test, no test for a destination, no select of the cell to read.
//   * U.near: does any lane of the wave hold an env on a non-water cell (a ballot of the OR of
//     the lane's four carried codes, taken after the move). It is this step's arrival vote, a
//     conservative one (it also passes for a ship that stays on a port: the test inside is the
//     position compare, as before), and the next step's first take vote: a take passes only on a
//     port's cell, so the exact vote over the actions runs only behind it. The result is whether
//     some env's cargo rose in the take block (the GATE pool's windows end on it).
//   * behind `near` a wave with U.bycode tests an arrival by the cell code (step_lean.h,
//     arrive_by_code); the others, and every wave of a world with two ports on one cell, by the position.
//   * the firing gates and the arrivals stay lane masks until a wave has one: the loss and
//     arrival blocks build their bit words themselves.
//   * the GATE words come from `gate`. GateDrawn: the caller drew them, and the step tests them.
//     GateScreened (the pooled window, below): the refill has screened the window's words, and on a
//     cold step (hot false, wave-uniform), where no gate of the wave can fire, the step reads no
//     word, tests no gate and has no loss block; do_move is then made only behind `near`, where
//     the arrival test reads it.
struct GateDrawn {
    static constexpr bool kScreened = false;
    const U4& gb;
    __device__ __forceinline__ bool hot() const { return true; }
    __device__ __forceinline__ U4 words() const { return gb; }
};
// A value as the branch it is read in sees it: the two places where a screened step makes do_move
// (behind `near`, on a hot step) each compare their own copy, so the compares stay inside their
// branches; written on the plain value they were hoisted into the step's main block, where a cold
// step away from the ports paid for them.
__device__ __forceinline__ uint32_t here(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <typename Read>
struct GateScreened {
    static constexpr bool kScreened = true;
    bool is_hot;
    Read read;  // the lane's pool entry for this step
    __device__ __forceinline__ bool hot() const { return is_hot; }
    __device__ __forceinline__ U4 words() const { return read(); }
};
// kAddr: U.pos is the cell's LDS address (step_lean.h): the target is the address plus the action's
// delta, and its code the byte there.
typedef __attribute__((address_space(3))) const int8_t lds_i8;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x2 lds_u32x2;
__device__ __forceinline__ uint32_t ring_address(uint32_t ring0, uint32_t bp, uint32_t wh) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, bp), __builtin_bit_cast(u16x2, wh), ring0, false);
}
template <bool kAddr, bool kNt, bool kSched, typename Gate, typename Late = NoLateDraw>
__device__ __forceinline__ bool step_group_ring(const LdsWorld& w, const SeqInv<kSched>& I, const Key& qk, uint32_t t, U4 fb,
                                                const Gate& gate, Group<false, false, kNt>& G, Carried& U, Late late = Late{}) {
    const int P = w.P;
    const uint32_t wh = (uint32_t)(w.W + 2) | (1u << 16);
    const uint32_t pm1 = P > 0 ? (uint32_t)(P - 1) : 0u;  // clamp for table reads whose value an error discards
    bool take_ran = false;
    if (U.near) {  // wave-uniform: some env of the wave is on a non-water cell
        bool take_any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) take_any |= (G.a[j] >= 4 + P) & (U.code[j] != 0);
        take_ran = __builtin_amdgcn_ballot_w64(take_any) != 0;
        if (take_ran) {
            bool rose = false;  // some env of the lane took cargo
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int act = G.a[j];
                const bool lt_tc = act < 54 + P;
                const int amount = act - (lt_tc ? 4 + P : 54 + P);
                const int2 st2 = U.take[U.code[j]];
                const int stock = lt_tc ? st2.y : st2.x;
                const bool ok_take = (act >= 4 + P) & (amount > 0) & (amount <= stock);
                rose |= ok_take & lt_tc;
                G.c[j] = (ok_take & lt_tc) ? G.c[j] + amount : G.c[j];
                G.f[j] = (ok_take & !lt_tc) ? G.f[j] + (double)amount : G.f[j];
                U.thr[j] = gate_thr_of(w, G.c[j]);
            }
#if SHIPENV_SEQ_CARGO_CUT
            // the result: did some env's cargo rise (a take of fuel and a refused take change no
            // cargo, no threshold and no carrier: the pool's window and its screen stay good)
            take_ran = __builtin_amdgcn_ballot_w64(rose) != 0;
#else
            (void)rose;
#endif
        }
    }
    late(fb);
    uint32_t np[4], code_t[4];
    // MOVE: the four lookups at the targets first, in flight together
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (kAddr) {
            const int8_t d = *(lds_i8*)(uintptr_t)(((uint32_t)G.a[j] & 3u) | I.delta0);
            np[j] = U.pos[j] + (uint32_t)(int32_t)d;
            code_t[j] = *(lds_u8*)(uintptr_t)np[j];
        } else {
            np[j] = pk_add_u16(U.pos[j], w.moves[G.a[j] & 3]);
            code_t[j] = lds_cell(I.ring0, np[j], wh);
        }
    }
    asm("" : "+v"(code_t[0]), "+v"(code_t[1]), "+v"(code_t[2]), "+v"(code_t[3]));
    int dst[4], cg[4];
    bool do_move[4], moved[4], fires[4];
    double f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int act = G.a[j];
        const int val = (int)((uint32_t)act - 4u);
        cg[j] = G.c[j];
        const bool same = U.org[j] == val;
        if constexpr (!Gate::kScreened) do_move[j] = ring_do_move(val, I.move_bound, code_t[j]);
        moved[j] = ring_moved(val, I.move_bound, code_t[j]);
        const bool sel_ok = lean_sel_ok(act, P, same);
        U.pos[j] = moved[j] ? np[j] : U.pos[j];
        U.code[j] = moved[j] ? code_t[j] : U.code[j];
        dst[j] = sel_ok ? val : U.dst[j];
        f[j] = lean_fuel(G.f[j], lean_fuel_scale(fb.v[j], kFifthPerWord), moved[j]);
        if constexpr (!Gate::kScreened) fires[j] = do_move[j] & (cg[j] > 0) & (gate.words().v[j] <= U.thr[j]);
    }
    // the vote word: this step's arrival vote and the next step's first take vote
    const bool near = __builtin_amdgcn_ballot_w64((U.code[0] | U.code[1] | U.code[2] | U.code[3]) != 0) != 0;
    U.near = near;
    uint32_t arrive = 0;
    if (near) {
        // (a mover selects nothing, so dst is still its dest)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if constexpr (Gate::kScreened) do_move[j] = ring_do_move((int)((uint32_t)G.a[j] - 4u), I.move_bound, here(code_t[j]));
#if SHIPENV_SEQ_ARRIVE_CODE
        // U.bycode (wave-uniform): the launch has at least two ports, all on distinct cells, and
        // every env of the wave has dest < P, which no state-only step then undoes (a select writes
        // val < P, an arrival pick_other's result, below P for P >= 2; with one port pick_other
        // gives 1 = P, which the position compare clamps to port 0, so such a launch never has the
        // bit). The ship is then on its destination's cell iff the code under it is dest + 1
        // (step_lean.h): no position read, no clamp, no bias. Every other wave keeps the position
        // compare: two ports may share a cell, and dest may hold anything a caller loaded.
        if (U.bycode) {
#pragma unroll
            for (int j = 0; j < 4; ++j) arrive |= (uint32_t)arrive_by_code(do_move[j], U.code[j], dst[j]) << j;
        } else
#endif
        {
            // the port's position biased as the ship's is (kAddr: its cell's address, made here from the
            // table's address and (W + 2) | 1 << 16 as the words behind the deltas hold them: nothing
            // else in a step reads either, and kept in scalar registers for this branch alone they
            // were spilled and read back inside the loop)
            [[maybe_unused]] u32x2 rw = {0u, 0u};
            if constexpr (kAddr) rw = *(lds_u32x2*)(uintptr_t)(I.delta0 + 8u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t port = ring_bias(w.pos[min((uint32_t)dst[j], pm1)]);
                if constexpr (kAddr) port = ring_address(rw.x, port, rw.y);
                arrive |= (uint32_t)(do_move[j] & (U.pos[j] == port)) << j;
            }
        }
    }
    int org[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        org[j] = U.org[j];
        G.f[j] = f[j];
    }
    // cargo loss and arrival, only in waves with a firing gate / an arrival
    bool any_fire = false;  // wave-uniform
    if constexpr (Gate::kScreened) {
        if (gate.hot()) {  // wave-uniform: the refill's screen passed for this step
            const U4 gb = gate.words();
#pragma unroll
            for (int j = 0; j < 4; ++j)
                fires[j] = ring_do_move((int)((uint32_t)G.a[j] - 4u), I.move_bound, here(code_t[j])) & (cg[j] > 0) & (gb.v[j] <= U.thr[j]);
            any_fire = __builtin_amdgcn_ballot_w64(fires[0] | fires[1] | fires[2] | fires[3]) != 0;
        }
    } else {
        any_fire = __builtin_amdgcn_ballot_w64(fires[0] | fires[1] | fires[2] | fires[3]) != 0;
    }
    if (any_fire) {
        uint32_t fire = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) fire |= (uint32_t)fires[j] << j;
        asm volatile("" : "+v"(fire));
        uint32_t lt[4], v1[4], v2[4], v3[4];
        const uint32_t rk[4] = {0u, fire & 1u, (uint32_t)__popc(fire & 3u), (uint32_t)__popc(fire & 7u)};
        U4 rr = I.block(qk, t, loss_slot(0));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lt[j] = rr.v[0];
            v1[j] = rr.v[1];
            v2[j] = rr.v[2];
            v3[j] = rr.v[3];
        }
#pragma unroll
        for (uint32_t q = 1; q < 4; ++q) {
            if (__popc(fire) > q) {
                rr = I.block(qk, t, loss_slot(q));
#pragma unroll
                for (int j = (int)q; j < 4; ++j) {
                    const bool take = rk[j] >= q;
                    lt[j] = take ? rr.v[0] : lt[j];
                    v1[j] = take ? rr.v[1] : v1[j];
                    v2[j] = take ? rr.v[2] : v2[j];
                    v3[j] = take ? rr.v[3] : v3[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (__builtin_amdgcn_ballot_w64((fire >> j) & 1u) == 0) continue;
            const uint32_t lo = min(v1[j], v2[j]), hi = max(v1[j], v2[j]);
            const uint32_t med = max(lo, min(hi, v3[j]));  // v_med3_u32
            const int part = beta_part(med, cg[j]);
            const int some = lt[j] > kTypeHi ? cg[j] : part;
            const int loss = lt[j] < kTypeLo ? 0 : some;
            const bool fj = (fire >> j) & 1u;
            cg[j] = fj ? cg[j] - loss : cg[j];
            U.thr[j] = gate_thr_of(w, cg[j]);
        }
    }
    if (arrive) {
        const U4 ab = I.block(qk, t, kSlotArrive);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool aj = (arrive >> j) & 1u;
            const int nd = pick_other(ab.v[j], P, dst[j]);
            cg[j] = aj ? 0 : cg[j];
            U.thr[j] = gate_thr_of(w, cg[j]);
            org[j] = aj ? dst[j] : org[j];
            dst[j] = aj ? nd : dst[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        U.org[j] = org[j];
        U.dst[j] = dst[j];
        G.c[j] = cg[j];
    }
    return take_ran;
}

// The stocks by cell code for the state-only steps' take checks: 256 (fuel, cargo) pairs,
// port i's at code i + 1 and zeros at every other code (0 water, kCellGround, codes past P),
// so `0 < amount <= stock` is false wherever the ship is on no port. One entry per thread of
// the block, read from the staged image; the caller holds the barrier.
constexpr size_t kStockByCodeBytes = 256 * sizeof(int2);
static_assert(kStepBlock == 256, "stock_by_code: one cell code per thread");
__device__ __forceinline__ void stock_by_code(const LdsWorld& w, int2* take) {
    const uint32_t k = threadIdx.x - 1u, P = (uint32_t)w.P;
    const int2 s = w.stock[min(k, P > 0 ? P - 1 : 0u)];  // P = 0: a word of the image, unused
    take[threadIdx.x] = k < P ? s : make_int2(0, 0);
}

// The wave's GATE pool (step_seq_kernel<kNt, kPool = true>). A GATE word is read only by
// `fires = do_move & (cargo > 0) & (word <= thr)`, and in the flagship run about 7 of a wave's 64
// lanes hold an env with cargo (profiles/seq_gatepool/carriers.json), so most lanes draw a block
// nobody reads. The block depends on the quad's key and the counter alone, so any lane can draw
// it ahead of time. When its pool is empty the wave votes: M = ballot(any of the lane's four
// cargo > 0), m = popc(M).
//   m == 0           no GATE draw, until a take ends the window;
//   0 < m <= limit   a window of W = min(16, 64 / m) steps (step_lean.h, gate_window_entry): the
//                    carriers write their GateSeed to the wave's seed row at their rank in M,
//                    lane L = s m + c draws carrier c's block at counter t + s into pool entry L
//                    (offset-major: W is no power of two), and for W steps every lane draws FUEL
//                    alone (draw_fuel) and reads its GATE words from entry offset m + rank (one
//                    ds_read_b128). Late in the flagship run a wave has 4 or 5 carrier lanes: a
//                    window of 8 steps filled half the pool and the wave drew again 8 steps later;
//   m > limit, or a wave with a lane past the last full group: kGateDirectRun steps of draw2,
//                    then another vote.
// A refill costs about two steps' GATE draws, so a wave whose takes keep ending its windows
// (ships in port: right after a reset the take block runs on most wave-steps) must not refill
// every step: after two refilled windows in a row that a take ended within kGateEarlyCut steps,
// the wave draws directly for kGateDirectRun steps, and one more such window sends it there again.
// Cargo rises only in a passed take of cargo, inside the take block (arrival and loss only lower
// it), so between two such takes no env becomes a carrier and no threshold rises: a window ends
// early after a step in which some env's cargo rose (step_group_ring's result, the ballot of
// `ok_take & lt_tc` taken inside the take block: wave-uniform, false where the block did not run)
// and after nothing else; the env that took did not move in that step, so its gate could not fire
// in it. A take of fuel and a refused take change no cargo, no threshold and no carrier, and leave
// the window standing. A lane that lost its cargo keeps a stale entry it no longer tests. A
// window also ends with the run's inner steps (words drawn past them are never read) and with the
// group. The rows are wave-private and one wave's LDS operations execute in order, so there is no
// __syncthreads: wavefront-scope fences and wave barriers keep the compiler's order. Per wave 64
// pool entries and kGatePoolSeeds seed rows of 16 B.
// The screen. The words of a window are known at its refill, up to 16 steps before they are tested,
// and so are the thresholds they can meet: inside a window cargo only falls, and gate_thr never
// rises as cargo falls (step_lean.h, screen_hot). So each carrier also writes its four carried
// thresholds to seed row kGatePoolLimit + rank (rows the limit of 16 leaves unused), the lane
// that drew a block compares its words with that row, and the ballot says on which steps of the
// window a gate of the wave can fire at all: with offset-major entries step s is hot iff bits
// [s m, s m + m) hold a one, so the window shifts the ballot down by m per step and tests its low
// m bits (step_lean.h, gate_screen_step; no fold). A step whose bit is clear is cold: it reads no
// pool entry, tests no gate, has no loss branch, and makes do_move only behind `near`
// (step_group_ring, GateScreened). In the flagship run about 85 % of the wave-steps are cold
// (profiles/seq_windows/freq.json). A window still ends where cargo rose: a take of cargo by a
// lane that carries raises that lane's threshold, and the screen would be stale. m == 0: the
// screen is 0. The launch's screen_all (SHIPENV_SEQ_SCREEN=0: all-ones) is OR-ed into every
// window's screen: every step hot, the loop before the screen. The direct runs test every gate.
// kGatePoolLimit (16 carrier lanes: W >= 4), kGatePoolSeeds (32 seed rows per wave) and kGatePoolRow
// (64 + 32 uint4 entries per wave) are step_lean.h's, beside the window's helpers.
constexpr uint32_t kGateDirectRun = 16;   // steps of the direct draw between two votes
constexpr uint32_t kGateEarlyCut = 2;     // a refilled window that a take ends within this many steps was cut early
constexpr uint32_t kSeqDistinctPorts = 1; // step_seq_kernel's ring_bytes, bit 0: at least two ports, all on distinct cells
static_assert(gate_pool_reads_in_rows(), "GATE pool: a window's reads lie in the wave's rows");  // the host's check (step_lean.h)
constexpr size_t kGatePoolBytes = (kStepBlock / 64) * kGatePoolRow * sizeof(uint4);  // 6 KiB
constexpr int kRingRows = 3;  // (ring_r0 .. ring_r2) 16-byte units of the bordered cell table a thread loads ahead: 12 KiB, the 100 x 100 map's 10.2
constexpr size_t kSeqDeltaBytes = SHIPENV_SEQ_CELL_ADDR ? kRingDeltaBytes : 0;  // the move deltas behind the table (step_lean.h)
static_assert(kGatePoolLimit <= kGatePoolSeeds && kGatePoolLimit <= 32, "GATE pool: a window of at least 2 steps");
static_assert(2 * kGatePoolLimit <= kGatePoolSeeds, "GATE pool: the carriers' threshold rows follow their seed rows");

// se_step_seq without auto-reset, fused: `steps` consecutive steps of the agent path in one
// launch, on step_kernel's grid and ownership. Nothing outside the stream can observe the
// state between two steps of one sequence, and a step reads only x, y, origin, dest, cargo,
// fuel and its action, so a group is loaded once, stepped `steps` times in registers
// (counter A.t + k, action row k at A.act + k * ld) and stored once, with the last step's
// reward, done and err. Against a launch per step that leaves out, per
// step, the launch, the world staging, 32 B of state loads and 38 B of stores per env; what a
// step still moves is its 4 B action. Row k + 1 is loaded before step k's arithmetic, so its
// latency (rows are read once, from HBM) hides behind the step. iters > 1: the group loop is
// the outer one.
// Behind the pools the launch stages the bordered cell table (step_lean.h), built by the host with
// the world image and kept behind it in the world buffer (ring_bytes; 0: no table). A wave whose
// envs are all regular steps with step_group_ring, in the pooled loop and in the direct run; a
// wave with an irregular env, and every wave of a launch without the table, runs
// step_group_state and draws directly for the whole run.
// Only the last step's reward, done and err exist anywhere, so steps 0 .. steps - 2 run the
// state-only step (step_group_state), with x | y, origin and dest unpacked once before them
// and packed once after, and step steps - 1 alone runs the full one (step_group_agent<kKeep>).
// Every launch of a split run therefore ends with a full step; steps == 1 is the full step by
// itself.
// The lane for a group's per-lane addresses. kOpaque (the pooled kernel): read through an empty
// asm where it is used, so the byte offsets derived from it are computed there and not once
// per launch, held across the step loops and spilled.
template <bool kOpaque>
__device__ __forceinline__ uint32_t seq_lane() {
    uint32_t lane = threadIdx.x;
    if constexpr (kOpaque) asm volatile("" : "+v"(lane));
    return lane;
}

// kAddr (the host's choice, for a launch with the table and byte deltas: step_lean.h): the regular
// waves carry the cell address. Four threads derive the move deltas from the image's packed moves
// into the kRingDeltaBytes behind the table, and ring_inv is ring_unindex_mul(W), for the way back
// to x, y after the inner steps.
template <bool kNt, bool kPool, bool kAddr>
__global__ __launch_bounds__(kStepBlock) __attribute__((amdgpu_waves_per_eu(4))) void step_seq_kernel(
    StepArgs A, int32_t steps, int64_t ld, uint32_t ring_bytes, uint32_t screen_all, uint32_t ring_inv) {
    extern __shared__ uint32_t lds[];
    if (steps <= 0) return;  // nothing to store (the host launches no empty run)
    // The bordered cell table (step_lean.h) follows the image in the world buffer; ring_bytes == 0:
    // this launch has none (launch-uniform), and every wave runs the general step.
    // Bit 0 of ring_bytes (kSeqDistinctPorts; the table's size is a multiple of 16): the host found
    // at least two ports, all on distinct cells, so a regular wave may test arrivals by the cell code.
    const uint32_t ring16 = steps > 1 ? ring_bytes >> 4 : 0u;
    const bool has_ring = ring16 != 0;
    [[maybe_unused]] const bool distinct = (ring_bytes & kSeqDistinctPorts) != 0;
    const int64_t full = A.n >> 2;
    const int64_t first = (int64_t)blockIdx.x * A.iters * kStepBlock;  // block-uniform first group

    const Staged st = stage_issue(A.world);
    __builtin_amdgcn_sched_barrier(0);
    // first group: step_kernel's clamped, unconditional load (state and action row 0)
    Group<false, false, kNt> G;
    {
        const int64_t last = full - 1 - first;  // block-uniform
        const uint32_t lane = last < (int64_t)threadIdx.x ? (uint32_t)(last < 0 ? 0 : last) : threadIdx.x;
        G.template load<true>(A, At<true>{last < 0 ? full - 1 : first, 0, A.n}, lane);
    }
    // the table's first kRingRows 16-byte units per thread, in flight behind the group's loads
    // (the 100 x 100 map's are all of it). Clamped and unconditional, so they stay in registers (a
    // launch without the table loads its first unit, which every world buffer has, and drops it)
    const uint4* const ring_g = reinterpret_cast<const uint4*>(A.world + A.dims.padded());
    const uint32_t ring_last = max(ring16, 1u) - 1u;
    const uint4 ring_r0 = ring_g[min(threadIdx.x, ring_last)];
    const uint4 ring_r1 = ring_g[min(threadIdx.x + kStepBlock, ring_last)];
    const uint4 ring_r2 = ring_g[min(threadIdx.x + 2 * kStepBlock, ring_last)];
    __builtin_amdgcn_sched_barrier(0);
    const LdsWorld w = stage_finish(A.world, A.dims, lds, st);
    // the state-only steps' take checks: the stocks by cell code, behind the staged image
    int2* const take = reinterpret_cast<int2*>(lds + A.dims.padded());
    uint4* const gate_pool = reinterpret_cast<uint4*>(take + 256);  // kPool: behind the stock table
    // the bordered cell table: behind the pools
    uint4* const ring_l = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(take + 256) + (kPool ? kGatePoolBytes : 0));
    if (steps > 1) {  // launch-uniform
        stock_by_code(w, take);
        if (has_ring) {
            if (threadIdx.x < ring16) ring_l[threadIdx.x] = ring_r0;
            if (threadIdx.x + kStepBlock < ring16) ring_l[threadIdx.x + kStepBlock] = ring_r1;
            if (threadIdx.x + 2 * kStepBlock < ring16) ring_l[threadIdx.x + 2 * kStepBlock] = ring_r2;
            for (uint32_t i = threadIdx.x + kStepBlock * kRingRows; i < ring16; i += kStepBlock) ring_l[i] = ring_g[i];  // larger maps
            if constexpr (kAddr) {
                // the move deltas, one byte per direction, behind the table's last 16-byte unit; in its
                // second half the table's own LDS address and the index's dot-product factor, for the
                // arrival test by address
                if (threadIdx.x < 4) reinterpret_cast<int8_t*>(ring_l + ring16)[threadIdx.x] = (int8_t)ring_delta(w.moves[threadIdx.x], w.W);
                if (threadIdx.x == 4)
                    reinterpret_cast<uint2*>(ring_l + ring16)[1] = make_uint2(lds_address(reinterpret_cast<const uint8_t*>(ring_l)), (uint32_t)(w.W + 2) | (1u << 16));
            }
        }
        __syncthreads();
    }

    // what the state-only steps read and no step changes: filled once per launch
    SeqInv<kPool> I;
    if (steps > 1) {
        I.move_bound = lean_move_bound(w.P);
        asm volatile("" : "+s"(I.move_bound));
        I.ring0 = lds_address(reinterpret_cast<const uint8_t*>(ring_l));
        I.delta0 = lds_address(reinterpret_cast<const uint8_t*>(ring_l + ring16));
    }

    BlockStats bs;
    Finished F;
    for (int64_t i = 0; i < A.iters; ++i) {
        const int64_t g0 = first + i * kStepBlock, g = g0 + threadIdx.x;
        if (g >= full) break;  // no barrier below
        if (i > 0) {
            // the lane opaque: the loads' per-lane addresses are computed here, once per group,
            // not kept in ~20 VGPRs across the step loop for the next group's sake
            uint32_t lane = threadIdx.x;
            asm volatile("" : "+v"(lane));
            G.template load<true>(A, At<true>{g0, 0, A.n}, lane);
        }
        const uint32_t tl = A.t + (uint32_t)(steps - 1);  // the last step's counter
        if (steps > 1) {
            // steps 0 .. steps - 2, state only: x | y, origin and dest one register per env
            Carried U;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                U.pos[j] = unpack_pos(G.x, G.y, j);
                U.org[j] = byte_of(G.org, j);
                U.dst[j] = byte_of(G.dst, j);
                U.code[j] = w.cell[cell_of(U.pos[j], (uint32_t)w.W | (1u << 16))];
                U.thr[j] = gate_thr_of(w, G.c[j]);
            }
            U.take = take;
            // The wave's path for the run: the regular step on the bordered table where the launch
            // has one and every env of the wave is inside the map with a destination (no state-only
            // step undoes either, step_group_ring), the general step drawing directly otherwise.
            bool irregular = false;
            {
                const uint32_t lim = (uint32_t)(w.H - 1) | ((uint32_t)(w.W - 1) << 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) irregular |= (U.dst[j] == SE_NONE) | (pk_min_u16(U.pos[j], lim) != U.pos[j]);
            }
            const bool ring = has_ring && __builtin_amdgcn_ballot_w64(irregular) == 0;  // wave-uniform
            U.near = __builtin_amdgcn_ballot_w64((U.code[0] | U.code[1] | U.code[2] | U.code[3]) != 0) != 0;
            // the arrival test by the cell code (step_group_ring): the launch's bit and one ballot
            U.bycode = false;
#if SHIPENV_SEQ_ARRIVE_CODE
            if (distinct) {  // launch-uniform
                bool past = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) past |= (uint32_t)U.dst[j] >= (uint32_t)w.P;
                U.bycode = __builtin_amdgcn_ballot_w64(past) == 0;
            }
#endif
            if (ring) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    U.pos[j] = ring_bias(U.pos[j]);
                    if constexpr (kAddr) U.pos[j] = ring_address(I.ring0, U.pos[j], (uint32_t)(w.W + 2) | (1u << 16));
                }
            }
            // the step-invariant parts of the quad's FUEL and GATE blocks (philox.h, draw2),
            // opaque so the loop keeps them in registers as computed here
            const Key qk = env_key(A.seed, (A.env_base + g * 4) >> 2);
            PairInv inv = pair_invariants(qk);
            asm volatile("" : "+v"(inv.hi[0]), "+v"(inv.lo[0]), "+v"(inv.hi[1]), "+v"(inv.lo[1]));
            const int32_t* row = A.act;
            if (!ring) {
                // no key schedule here (the rare draws are draw()'s): a third copy of the step with
                // the schedule's 20 registers live beside it does not fit under 128
                SeqInv<false> Ig;
                Ig.move_bound = I.move_bound;
                const uint32_t lane = seq_lane<kPool>();
                for (uint32_t t = A.t; t != tl; ++t) {
                    // the next row's actions (there is one: the last step follows)
                    row += ld;
                    int32_t nxt[4];
                    ld4_full<kNt>(row, g0, nxt, lane);
                    const U4x2 fg = draw2(qk, inv, t);
                    step_group_state(w, Ig, qk, t, fg.fuel, fg.gate, G, U);
#pragma unroll
                    for (int j = 0; j < 4; ++j) G.a[j] = nxt[j];
                }
            } else if constexpr (!kPool) {
                for (uint32_t t = A.t; t != tl; ++t) {
                    row += ld;
                    int32_t nxt[4];
                    ld4_full<kNt>(row, g0, nxt);
                    const U4x2 fg = draw2(qk, inv, t);
                    step_group_ring<kAddr>(w, I, qk, t, fg.fuel, GateDrawn{fg.gate}, G, U);
#pragma unroll
                    for (int j = 0; j < 4; ++j) G.a[j] = nxt[j];
                }
            } else {
                // the wave's GATE pool (above): vote, then a window from the pool or a few
                // steps of the direct draw, until the run's inner steps are done. The key schedule
                // is filled here, per group, so that it is live in the regular waves' loops alone.
                {
                    const Key sk = env_key(A.seed, 0);
                    I.ks = key_schedule(sk.k0, sk.k1);
                    pin_schedule(I.ks);
                }
                const uint32_t lane = seq_lane<true>(), L = lane & 63u;
                uint4* const pool = gate_pool + (lane >> 6) * kGatePoolRow;
                uint4* const seeds = pool + 64;
                // a wave with a lane past the last full group (the `break` above) has lanes
                // missing from a refill: it draws directly
                const bool whole = __builtin_amdgcn_ballot_w64(true) == ~0ull;
                uint32_t cuts = 0;  // refilled windows in a row that a take cut early
                for (uint32_t t = A.t; t != tl;) {
                    // The pooled steps, window after window in one loop, so the state stays in its
                    // registers from window to window, and only a wave that leaves for the direct
                    // draw moves it: a few steps of it, and the wave votes again.
                    bool pooled = true;
                    do {
                        // the vote
                        const bool carry = (G.c[0] > 0) | (G.c[1] > 0) | (G.c[2] > 0) | (G.c[3] > 0);
                        const uint64_t M = __builtin_amdgcn_ballot_w64(carry);
                        const uint32_t m = (uint32_t)__popcll(M);
                        if (!whole || m > kGatePoolLimit || (cuts >= 2 && m != 0)) {
                            pooled = false;
                            break;
                        }
                        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
#if SHIPENV_SEQ_WINDOW_DIV
                        // the window: W = min(16, 64 / m) steps, and the multiplier of a lane's L / m (step_lean.h)
                        const uint32_t went = gate_window_entry(m);
                        // the window's screen: the refill's ballot itself, m bits per offset (step_lean.h), shifted
                        // down by m per step: can a gate fire on this step? m == 0: no, however long the
                        // window. screen_all (SHIPENV_SEQ_SCREEN=0): every step is hot.
                        uint64_t screen = (uint64_t)(int64_t)(int32_t)screen_all;
                        const uint64_t smask = gate_screen_mask(m);
                        if (m != 0) {
                            if (carry) {
                                seeds[slot] = make_uint4(inv.c3, inv.hi[1], inv.lo[1], qk.e1);
                                // the thresholds at the vote (0 for an env without cargo: gate_thr's entry 0)
                                seeds[kGatePoolLimit + slot] = make_uint4(U.thr[0], U.thr[1], U.thr[2], U.thr[3]);
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            // lane L = so m + of draws carrier of's block at window offset so; the lanes at
                            // or past m W: a carrier's block at an offset past the window, which nobody reads
                            const uint32_t so = gate_lane_offset(L, went), of = gate_lane_carrier(L, so, m);
                            const uint4 sd = seeds[of];
                            const uint4 th = seeds[kGatePoolLimit + of];
                            const U4 gw = draw_gate_pooled_sched(I.ks, GateSeed{sd.x, sd.y, sd.z, sd.w}, t + so);
                            pool[L] = make_uint4(gw.v[0], gw.v[1], gw.v[2], gw.v[3]);
                            // screen_hot (step_lean.h) word by word: four compares into lane masks, OR-ed in scalar code
                            screen |= __builtin_amdgcn_ballot_w64(gw.v[0] <= th.x) | __builtin_amdgcn_ballot_w64(gw.v[1] <= th.y) |
                                      __builtin_amdgcn_ballot_w64(gw.v[2] <= th.z) | __builtin_amdgcn_ballot_w64(gw.v[3] <= th.w);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
                        // a carrier's words for offset s are entry s m + slot < m W <= 64. Another lane's
                        // slot is at most m: it reads an entry up to m W <= 64 < kGatePoolRow (the seeds
                        // follow the pool; a static_assert checks the bound for every m), whose words its gate
                        // never tests. m == 0: entry 0; no entry holds anything, no gate tests a word, and
                        // the window lasts until a take of cargo ends it.
                        const uint32_t win = m != 0 ? min(tl - t, gate_window_len(went)) : tl - t;  // t may wrap 2^32 inside the run
                        uint32_t s = 0;
                        bool took;
                        do {
                            row += ld;
                            int32_t nxt[4];
                            ld4_full<kNt>(row, g0, nxt, lane);
                            // the lane's words, read on a hot step only (the offset read as the hot branch
                            // sees it: the entry's address is made there, not stepped by m on every step)
                            const auto words = [&]() {
                                uint32_t so = s;
                                asm volatile("" : "+s"(so));
                                const uint4 g4 = pool[gate_pool_index(so, m, slot)];
                                return U4{{g4.x, g4.y, g4.z, g4.w}};
                            };
                            // FUEL alone, drawn after the take block (the step's `late`)
                            const auto fuel = [&](U4& fb) {
                                fb = draw_fuel_sched(I.ks, qk, inv, t);
                                asm volatile("" : "+v"(fb.v[0]), "+v"(fb.v[1]), "+v"(fb.v[2]), "+v"(fb.v[3]));
                            };
                            took = step_group_ring<kAddr>(w, I, qk, t, U4{}, GateScreened<decltype(words)>{gate_screen_step(screen, smask), words}, G, U, fuel);
#pragma unroll
                            for (int j = 0; j < 4; ++j) G.a[j] = nxt[j];
                            screen >>= m;
                            ++s;
                            ++t;
                        } while (!took && s != win);
#else
                        // the window: the largest power of two W <= 8 with m W <= 64
                        const uint32_t logw = gate_window_log2(m);
                        const uint32_t wmask = (1u << logw) - 1u;
                        // the window's screen, one bit per offset (step_lean.h): can a gate fire there?
                        // m == 0: no, however long the window (0 or all-ones: any bit of it will do).
                        // screen_all (SHIPENV_SEQ_SCREEN=0): every step is hot.
                        uint32_t screen = screen_all;
                        if (m != 0) {
                            if (carry) {
                                seeds[slot] = make_uint4(inv.c3, inv.hi[1], inv.lo[1], qk.e1);
                                // the thresholds at the vote (0 for an env without cargo: gate_thr's entry 0)
                                seeds[kGatePoolLimit + slot] = make_uint4(U.thr[0], U.thr[1], U.thr[2], U.thr[3]);
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            // lane L draws carrier L >> logw's block at window offset L & (W - 1);
                            // past the last carrier: the last one's again, which nobody's gate reads
                            const uint32_t of = min(L >> logw, m - 1u);
                            const uint4 sd = seeds[of];
                            const uint4 th = seeds[kGatePoolLimit + of];
                            const U4 gw = draw_gate_pooled_sched(I.ks, GateSeed{sd.x, sd.y, sd.z, sd.w}, t + (L & wmask));
                            pool[L] = make_uint4(gw.v[0], gw.v[1], gw.v[2], gw.v[3]);
                            // screen_hot (step_lean.h) word by word: four compares into lane masks, OR-ed in
                            // scalar code (as one bool expression it compiled to 15 VALU of selects and shifts)
                            const uint64_t hot = __builtin_amdgcn_ballot_w64(gw.v[0] <= th.x) | __builtin_amdgcn_ballot_w64(gw.v[1] <= th.y) |
                                                 __builtin_amdgcn_ballot_w64(gw.v[2] <= th.z) | __builtin_amdgcn_ballot_w64(gw.v[3] <= th.w);
                            screen |= screen_fold(hot, logw);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
                        // a carrier's words for offset s are entry slot W + s < 64. Another lane's
                        // slot is at most m: it reads some entry below 64 + W (the seeds follow
                        // the pool), whose words its gate never tests. m == 0: no entry holds
                        // anything, no gate tests a word, and the window lasts until a take ends it.
                        const uint4* const mine = pool + ((slot << logw) & 63u);
                        const uint32_t win = m != 0 ? min(tl - t, wmask + 1u) : tl - t;  // t may wrap 2^32 inside the run
                        // The window's steps, a counted loop that a take leaves early: a take may have
                        // made a carrier, so the wave votes again (wave-uniform).
                        uint32_t s = 0;
                        bool took;
                        do {
                            row += ld;
                            int32_t nxt[4];
                            ld4_full<kNt>(row, g0, nxt, lane);
                            // the lane's words, read on a hot step only
                            const auto words = [&]() {
                                const uint4 g4 = mine[s & wmask];
                                return U4{{g4.x, g4.y, g4.z, g4.w}};
                            };
                            // FUEL alone, drawn after the take block (the step's `late`)
                            const auto fuel = [&](U4& fb) {
                                fb = draw_fuel_sched(I.ks, qk, inv, t);
                                asm volatile("" : "+v"(fb.v[0]), "+v"(fb.v[1]), "+v"(fb.v[2]), "+v"(fb.v[3]));
                            };
                            took = step_group_ring<kAddr>(w, I, qk, t, U4{}, GateScreened<decltype(words)>{((screen >> (s & 31u)) & 1u) != 0, words}, G, U, fuel);
#pragma unroll
                            for (int j = 0; j < 4; ++j) G.a[j] = nxt[j];
                            ++s;
                            ++t;
                        } while (!took && s != win);
#endif
                        // refilled windows in a row that a take cut early
                        cuts = took && m != 0 && s <= kGateEarlyCut ? cuts + 1u : 0u;
                    } while (t != tl);
                    if (pooled) break;
                    cuts = min(cuts, 1u);
                    for (uint32_t n = min(tl - t, kGateDirectRun); n != 0; --n, ++t) {
                        row += ld;
                        int32_t nxt[4];
                        ld4_full<kNt>(row, g0, nxt, lane);
                        const U4x2 fg = draw2(qk, inv, t);
                        step_group_ring<kAddr>(w, I, qk, t, fg.fuel, GateDrawn{fg.gate}, G, U);
#pragma unroll
                        for (int j = 0; j < 4; ++j) G.a[j] = nxt[j];
                    }
                }
            }
            if (ring) {  // the bias comes off once
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (kAddr) U.pos[j] = ring_unindex(U.pos[j] - I.ring0, w.W, ring_inv);
                    U.pos[j] = ring_unbias(U.pos[j]);
                }
            }
            // back into the Group's packed bytes
            pack_pos(U.pos, G.x, G.y);
            G.org = G.dst = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                G.org |= (uint32_t)(U.org[j] & 0xff) << (8 * j);
                G.dst |= (uint32_t)(U.dst[j] & 0xff) << (8 * j);
            }
        }
        // the last step in full: its reward, done and err are the run's
        StepOut O;
        const uint32_t ln = seq_lane<true>();
        const At<true> at{g0, (g0 + ln) * 4, A.n};
        step_group_agent<false, true, kNt, false, false, true>(A, w, G, at, bs, F, early_draws<false>(A, at.base, tl), tl, &O);
        const se_state& S = late_args().st;
        __builtin_amdgcn_sched_barrier(0);  // the fuel halves back to back (store_moved)
        st4u8_full(S.x, g0, G.x, ln);
        st4u8_full(S.y, g0, G.y, ln);
        st4_full(S.fuel, g0, G.f, ln);
        st4u8_full(S.done, g0, O.dn, ln);
        st4u8_full(reinterpret_cast<uint8_t*>(S.err), g0, O.ee, ln);
        __builtin_amdgcn_sched_barrier(0);
        st4u8_full(S.origin, g0, G.org, ln);
        st4u8_full(S.dest, g0, G.dst, ln);
        st4_full(S.cargo, g0, G.c, ln);
        st4_full(S.reward, g0, O.rw, ln);
    }
}

// The partial last group of a fused sequence: one thread steps its at most 3 envs `steps`
// times with step_tail_envs, loading and storing per step.
__global__ __launch_bounds__(64) void step_tail_seq_kernel(StepArgs A, int32_t steps, int64_t ld) {
    if (threadIdx.x != 0) return;
    const LdsWorld w = world_view(A.dims, A.world);
    const int32_t* act = A.act;
    const uint32_t t0 = A.t;
    for (int32_t k = 0; k < steps; ++k) {
        A.act = act + (int64_t)k * ld;
        A.t = t0 + (uint32_t)k;
        step_tail_envs<false, false, false>(A, w);
    }
}
