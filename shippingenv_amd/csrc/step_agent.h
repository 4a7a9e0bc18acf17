#pragma once
// step_agent.h — the production step of one group of 4 envs from agent-index
// actions (se_step, se_step_record): the packed-position helpers, Draws /
// early_draws, the record helpers and step_group_agent.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld, the image's tables), env_core.h (Ship, env_key, beta_part,
// reset_ship), step_io.h (StepArgs, StepRecord, Group, At, the stores) and
// step_group.h (BlockStats, Finished).

// ------------------------------------------------------------------ agent-index path
// The production step for agent-index actions (se_step), written for VALU issue,
// the bound at N = 2^20: the same semantics as env_begin +
// env_finish with kUnitMoves (tests compare it bit for bit with the
// oracle), in a packed form.
//   * A ship position is one register x | y << 16: a move is one v_pk_add_u16 of
//     the action's packed (dx, dy) from the world image, the bounds test one
//     v_pk_min_u16 against (H-1, W-1), a cell index one v_dot2_u32_u16 with (W, 1),
//     the squared distances of the closer/farther test (:307-315) one v_pk_sub_i16
//     and one v_dot2_i32_i16 each, and the arrival test (:325) one compare.
//   * One cell-code byte answers "ground?" for the target cell (:293) and "which
//     port?" for the ship's cell (:145-153).
//   * Fuel changes by one f64 add of a selected delta (-cost, +amount or -0.0, which
//     leaves every fuel value as it is, -0.0 included).
//   * Cargo loss and arrival arithmetic run inside the branches that draw their
//     blocks, so waves without a firing gate / an arrival skip them.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t i16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_add_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
// squared euclidean distance of two packed positions (halves < 256)
__device__ __forceinline__ int dist2(uint32_t a, uint32_t b) {
    const i16x2 d = __builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b);
    return __builtin_amdgcn_sdot2(d, d, 0, false);
}
// cell index x * W + y of a packed position; wh = W | 1 << 16
__device__ __forceinline__ uint32_t cell_of(uint32_t p, uint32_t wh) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, p), __builtin_bit_cast(u16x2, wh), 0u, false);
}

// The byte at index x * W + y of an LDS table, the table's LDS address riding in the dot
// product's accumulator (cell_of, then the pointer add, is one more v_add_u32 of a base that is
// zero). cell0: lds_address(table).
typedef __attribute__((address_space(3))) const uint8_t lds_u8;
__device__ __forceinline__ uint32_t lds_address(const uint8_t* p) { return (uint32_t)(uintptr_t)(lds_u8*)p; }
__device__ __forceinline__ uint32_t lds_cell(uint32_t cell0, uint32_t p, uint32_t wh) {
    const uint32_t a = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, p), __builtin_bit_cast(u16x2, wh), cell0, false);
    return *(lds_u8*)(uintptr_t)a;
}

// The Philox blocks of a group that depend on no state (contract v5: FUEL every step;
// GATE, whose words are the same whether or not an env consumes them; LOSS_0, the
// block of the quad's first firing env, used by most waves): drawn right after the
// group's loads are issued, so their VALU work overlaps the wait for the data
// instead of following it.
// LOSS_0 is drawn early with auto-reset (config 4 measured 12.71 -> 12.44 us at
// 2^20) and on demand without (config 3: 8.48 vs 8.56 us).
struct Draws {
    U4 fuel, gate, loss0, arrive;
};
template <bool kSpecLoss>
__device__ __forceinline__ Draws early_draws(const StepArgs& A, int64_t base, uint32_t t) {
    const Key qk = env_key(A.seed, (A.env_base + base) >> 2);
    Draws d;
    d.fuel = draw(qk, t, kSlotFuel);
    d.gate = draw(qk, t, kSlotGate);
    d.loss0 = kSpecLoss ? draw(qk, t, loss_slot(0)) : U4{{0u, 0u, 0u, 0u}};
    d.arrive = U4{{0u, 0u, 0u, 0u}};
    return d;
}
template <bool kSpecLoss>
__device__ __forceinline__ Draws early_draws(const StepArgs& A, int64_t base) {
    const Key qk = env_key(A.seed, (A.env_base + base) >> 2);
    Draws d;
    d.fuel = draw(qk, A.t, kSlotFuel);
    d.gate = draw(qk, A.t, kSlotGate);
    d.loss0 = kSpecLoss ? draw(qk, A.t, loss_slot(0)) : U4{{0u, 0u, 0u, 0u}};
    d.arrive = U4{{0u, 0u, 0u, 0u}};
    return d;
}

template <bool kAuto>
constexpr bool spec_loss() { return kAuto; }

// The group's x and y bytes (packed u8 x4) and its positions, one register x | y << 16 per env.
__device__ __forceinline__ uint32_t unpack_pos(uint32_t x4, uint32_t y4, int j) {
    return __builtin_amdgcn_perm(y4, x4, (uint32_t)j | 0x0c000c00u | ((uint32_t)(4 + j) << 16));
}
__device__ __forceinline__ void pack_pos(const uint32_t (&pos)[4], uint32_t& x4, uint32_t& y4) {
    const uint32_t t01 = __builtin_amdgcn_perm(pos[1], pos[0], 0x06020400u);  // x0 x1 y0 y1
    const uint32_t t23 = __builtin_amdgcn_perm(pos[3], pos[2], 0x06020400u);  // x2 x3 y2 y3
    x4 = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
    y4 = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
}

// se_step_record, per group of 4 envs at env index base (a full group; head and cap
// multiples of 4, so its ring slots are consecutive): the stores of replay_end4_kernel
// (csrc/replay.h) from the post-step values this thread just computed. After the
// thread's last group, record_restart runs se_replay_end_reset's restart of the cut envs
// (reset_kernel's body, at most one bit per env of the thread's <= 8 groups). Their
// fields were stored by this thread earlier in program order; the restart stores the same
// addresses again, as the separate replay-end launch would after the step. Deferred past
// the loop, the restart's registers do not overlap the group's (inline there it spilled).
__device__ __forceinline__ void record_restart(const StepArgs& A, const LdsWorld& w, uint32_t cuts) {
    const se_state& S = A.st;
    const int64_t first = (int64_t)blockIdx.x * A.iters * kStepBlock;  // step_kernel's first group
    while (cuts) {
        const int b = __builtin_ctz(cuts);
        cuts &= cuts - 1;
        const int64_t i = (first + (int64_t)(b >> 2) * kStepBlock + threadIdx.x) * 4 + (b & 3);
        const U4 o = draw(env_key(A.seed, A.env_base + i), A.rec.epoch, kSlotExplicitReset);
        Ship sh;
        reset_ship(w, sh, o.v[0], o.v[1]);
        S.x[i] = (uint8_t)sh.x;
        S.y[i] = (uint8_t)sh.y;
        S.fuel[i] = sh.fuel;
        S.cargo[i] = sh.cargo;
        S.origin[i] = (uint8_t)sh.origin;
        S.dest[i] = (uint8_t)sh.dest;
        S.ep_return[i] = 0.0f;
        S.ep_start[i] = (int32_t)(A.t + 1u);  // its first step is the next one
        S.done[i] = 0;
        S.err[i] = 0;
        S.reward[i] = 0.0f;
    }
}

__device__ __forceinline__ int64_t record_slot(const StepRecord& R, int64_t base) {
    const int64_t slot = R.head + base;
    return slot - (slot >= R.cap ? R.cap : 0);
}

__device__ __forceinline__ void record_early(const StepArgs& A, int64_t base, uint32_t flags4, const float (&fuel)[4]) {
    const StepRecord& R = A.rec;
    const int64_t slot = record_slot(R, base);
    *reinterpret_cast<uint32_t*>(R.flags + slot) = flags4;
    *reinterpret_cast<float4*>(R.n_fuel + slot) = make_float4(fuel[0], fuel[1], fuel[2], fuel[3]);
}

// returns the cut envs as bits 0-3
__device__ __forceinline__ uint32_t record_group(const StepArgs& A, int64_t base, const float (&rw)[4],
                                                 uint32_t x4, uint32_t y4, uint32_t o4, uint32_t d4,
                                                 uint32_t cut4, const int32_t (&len)[4]) {
    const StepRecord& R = A.rec;
    const int64_t slot = record_slot(R, base);
    uint4 pos;
    uint32_t* pw = &pos.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pw[j] = ((x4 >> (8 * j)) & 0xffu) | ((y4 >> (8 * j)) & 0xffu) << 8 | ((o4 >> (8 * j)) & 0xffu) << 16 |
                ((d4 >> (8 * j)) & 0xffu) << 24;
        if (R.max_steps > 0) cut4 |= (uint32_t)(len[j] >= R.max_steps) << (8 * j);
    }
    *reinterpret_cast<float4*>(R.rew + slot) = make_float4(rw[0], rw[1], rw[2], rw[3]);
    *reinterpret_cast<uint4*>(R.n_pos + slot) = pos;
    *reinterpret_cast<uint32_t*>(R.cut + base) = cut4;
    return (cut4 & 1u) | ((cut4 >> 7) & 2u) | ((cut4 >> 14) & 4u) | ((cut4 >> 21) & 8u);
}

// kReplay (se_step_agent_replay; parity only): the same code with the reference's draws
// from the tape instead of Philox words: u_fuel and u_gate as f64 uniforms (the gate
// tested against fl(c/50) as env_begin<.., kReplay> does, so a cargo-0 ship's gate can
// fire, lose nothing, and still consume the loss-type draw), the loss type, beta and
// the arrival's new destination; SE_USED_* bits back in the tape, and a step that needs
// a variate the tape lacks leaves its env untouched with SE_ERR_NEED_DRAW.
//
// kKeep (step_seq_kernel: a full group, Philox draws, no auto-reset): the step runs at
// counter tk instead of A.t and stores nothing. The post-step x, y, fuel, cargo, origin and
// dest go back into G in its packed form, so the next step of a fused sequence reads them
// from registers, and the step's reward, done bytes and err bytes are returned in *O; the
// caller stores the state and the last step's outputs once. The arithmetic is the per-step
// code's, untouched. (tk and O are trailing defaults, not a wrapper: the per-step
// instantiations then compile to the instructions they had before.)
struct StepOut {
    float rw[4];
    uint32_t dn, ee;  // done / err of the group, packed u8 x4
};
template <bool kAuto, bool kFull, bool kNt, bool kRec = false, bool kReplay = false, bool kKeep = false>
__device__ __forceinline__ void step_group_agent(const StepArgs& A, const LdsWorld& w,
                                                 Group<false, kAuto, kNt>& G, At<kFull> at,
                                                 BlockStats& bs, Finished& F, const Draws& D,
                                                 [[maybe_unused]] uint32_t tk = 0,
                                                 [[maybe_unused]] StepOut* O = nullptr) {
    static_assert(!kReplay || (!kAuto && !kRec), "agent replay: no auto-reset, no ring record");
    static_assert(!kKeep || (kFull && !kAuto && !kRec && !kReplay), "fused sequence: full groups, no auto-reset");
    const int64_t n = A.n, base = at.base;
    const int P = w.P;
    const uint32_t lim = (uint32_t)(w.H - 1) | ((uint32_t)(w.W - 1) << 16);
    const uint32_t wh = (uint32_t)w.W | (1u << 16);
    const uint32_t pm1 = P > 0 ? (uint32_t)(P - 1) : 0u;  // clamp for table reads whose value an error discards
    const Key qk = env_key(A.seed, (A.env_base + base) >> 2);
    const uint32_t t = kKeep ? tk : A.t;  // the step counter: the sequence's, or the launch's
    constexpr bool kSpecLoss = spec_loss<kAuto>();
#if SHIPENV_TRACE
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the group's data has arrived
    TRACE_STAMP(4);
#endif
    // --- first half: everything that needs no optional draw (:359-376, :273-315)
    uint32_t pos[4], pd16[4];
    int val[4], dst[4], cg[4], err[4], ridx[4];
    bool do_move[4], moved[4], tf_ok[4];
    bool gate_needed = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // utils/preprocessing.py:111-137: [0,4) moves N, E, S, W (-4..-1 wrap like a
        // Python index), [4, 4+P) SELECT, [4+P, 54+P) TAKE_CARGO, then TAKE_FUEL
        const int act = G.a[j];
        const bool bad = act < -4;
        const bool is_mv = act < 4, lt_sel = act < 4 + P, lt_tc = act < 54 + P;
        val[j] = act - 4 - (lt_sel ? 0 : P) - (lt_tc ? 0 : 50);
        const uint32_t dxy = w.moves[act & 3];
        const uint32_t p = unpack_pos(G.x, G.y, j);
        dst[j] = byte_of(G.dst, j);
        cg[j] = G.c[j];
        // MOVE (_move_ship :273-339)
        const uint32_t np = pk_add_u16(p, dxy);
        const bool inb = pk_min_u16(np, lim) == np;  // _is_within_map (:284); -1 wraps to 0xffff
        const bool nodest = dst[j] == SE_NONE;       // :276
        const uint32_t cp = (!nodest & inb) ? np : p;  // in-range cell for the lookups
        const bool ground = w.cell[cell_of(cp, wh)] == kCellGround;  // :293
        pd16[j] = w.pos[min((uint32_t)dst[j], pm1)];
        const bool closer = dist2(p, pd16[j]) > dist2(cp, pd16[j]);  // old vs ATTEMPTED cell (:307-315)
        // TAKE_* (:341-357) at the port on the ship's cell; SELECT_PORT (:265-271)
        const int k = (int)w.cell[cell_of(p, wh)] - 1;
        const bool atport = (uint32_t)k < (uint32_t)P;
        const int2 st2 = w.stock[min((uint32_t)k, pm1)];
        const int stock = lt_tc ? st2.y : st2.x;
        const bool amount_bad = (val[j] <= 0) | (val[j] > stock);
        const bool same = byte_of(G.org, j) == val[j];
        const int e_move = nodest ? SE_ERR_NO_DEST : (inb ? SE_ERR_OK : SE_ERR_OOB);
        const int e_sel = same ? SE_ERR_SAME_PORT : SE_ERR_OK;
        const int e_amt = amount_bad ? SE_ERR_AMOUNT : SE_ERR_OK;
        const int e_take = atport ? e_amt : SE_ERR_NOT_AT_PORT;
        const int e_ns = lt_sel ? e_sel : e_take;
        const int e_ty = is_mv ? e_move : e_ns;
        const int e_p = P == 0 ? SE_ERR_NO_PORTS : e_ty;  // :360
        err[j] = bad ? SE_ERR_BAD_INDEX : e_p;            // the decode runs before env.step
        const bool ok = err[j] == SE_ERR_OK;
        do_move[j] = ok & is_mv;
        moved[j] = do_move[j] & !ground;
        const bool take_ok = ok & !lt_sel;
        tf_ok[j] = take_ok & !lt_tc;
        const bool tc_ok = take_ok & lt_tc;
        const bool sel_ok = ok & !is_mv & lt_sel;
        pos[j] = moved[j] ? cp : p;
        cg[j] = tc_ok ? cg[j] + val[j] : cg[j];
        dst[j] = sel_ok ? val[j] : dst[j];
        // reward row before loss / arrival: a move by (out_of_fuel, ground, closer),
        // filled in once fuel is known; a take 0.05; anything else 0
        const int r_rest = take_ok ? 8 : 9;
        ridx[j] = do_move[j] ? (((int)ground << 1) | (int)closer) : r_rest;
        gate_needed |= !bad & is_mv & !nodest & inb & (G.c[j] > 0) & (G.c[j] < 50);
    }
    TRACE_STAMP(5);
    // GATE is drawn early (early_draws) whether or not an env needs it. The dead expression
    // stays: without it the compiler schedules the replay kernel's instructions in another order.
    (void)gate_needed;
    const U4 fb = D.fuel;
    const U4 gb = D.gate;
    uint32_t fire = 0, arrive = 0, fin = 0, dead = 0;
    double f[4], r[4];
    // kReplay: the group's tape records (the partial last group's missing envs read none)
    [[maybe_unused]] double tu[4], tg[4], tt[4], tb[4];
    [[maybe_unused]] int td[4];
    [[maybe_unused]] uint32_t need = 0;  // kReplay: envs whose step needs a variate the tape lacks
    if constexpr (kReplay) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool live = kFull || base + j < n;
            const se_tape* tp = A.tape + (live ? base + j : 0);
            tu[j] = tp->u_fuel;
            tg[j] = tp->u_gate;
            tt[j] = tp->u_type;
            tb[j] = tp->beta;
            td[j] = tp->arrive_dest;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // fuel cost (:103-104): 1 * (1 + uniform(-0.1, 0.1)), uniform = -0.1 + 0.2 u
        double scale;
        if constexpr (kReplay) scale = 1.0 + (-0.1 + 0.2 * tu[j]);
        else scale = 1.0 + (-0.1 + (double)fb.v[j] * kFifthPerWord);
        const bool oof = G.f[j] < scale;  // :288-290 (the ship still moves)
        const double take = tf_ok[j] ? (double)val[j] : -0.0;
        f[j] = G.f[j] + (moved[j] ? -scale : take);
        // the gate random() <= cargo / 50 (:318-323) as w <= floor(fl(c/50) 2^32); the
        // table's entry 50 is all ones (cargo >= 50 always fires); cargo 0 loses nothing
        bool fires;
        if constexpr (kReplay) {
            const double ug = tg[j];
            const int ci = ((cg[j] > 0) & (cg[j] < 50)) ? cg[j] : 0;
            // cargo < 0 never fires (env_begin): ci = 0 stands for cargo 0 only
            fires = do_move[j] & ((cg[j] >= 50) | ((cg[j] >= 0) & (ug <= w.likelihood(ci))));
            need |= (uint32_t)(do_move[j] & ((tu[j] != tu[j]) | (ug != ug))) << j;
        } else {
            const uint32_t thr = w.gate_thr[min(max(cg[j], 0), 50)];
            fires = do_move[j] & (cg[j] > 0) & (gb.v[j] <= thr);
        }
        r[j] = w.rtab[ridx[j] | ((int)(do_move[j] & oof) << 2)];
        fire |= (uint32_t)fires << j;
        arrive |= (uint32_t)(do_move[j] & (pos[j] == pd16[j])) << j;  // :325
        dead |= (uint32_t)(do_move[j] & oof) << j;
        fin |= (uint32_t)((kFull || base + j < n) & do_move[j] & oof) << j;
    }
    // the flags travel as opaque VGPR bit masks (no lane masks live in SGPR pairs
    // across the draw blocks below)
    asm volatile("" : "+v"(fire), "+v"(arrive), "+v"(fin), "+v"(dead));
    int org[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) org[j] = byte_of(G.org, j);

    // auto-reset (:227-243) of the envs that ran out of fuel: position and fuel now,
    // cargo / origin / dest after the second half (whose reward the finished episode
    // still collects). Contract v5: the r-th finishing env of the quad takes RESET_r.
    uint32_t reset_o = 0, reset_d = 0;
    if constexpr (kAuto) {
        if (fin) {
            uint32_t ow[4], dw[4];
            const uint32_t rk[4] = {0u, fin & 1u, (uint32_t)__popc(fin & 3u), (uint32_t)__popc(fin & 7u)};
            U4 rr = draw(qk, t, reset_slot(0));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ow[j] = rr.v[0];
                dw[j] = rr.v[1];
            }
#pragma unroll
            for (uint32_t q = 1; q < 4; ++q) {
                if (__popc(fin) > q) {
                    rr = draw(qk, t, reset_slot(q));
#pragma unroll
                    for (int j = (int)q; j < 4; ++j) {
                        ow[j] = rk[j] >= q ? rr.v[0] : ow[j];
                        dw[j] = rk[j] >= q ? rr.v[1] : dw[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = uniform_int(ow[j], (uint32_t)P);
                const int d = pick_other(dw[j], P, o);
                reset_o |= (uint32_t)o << (8 * j);
                reset_d |= (uint32_t)d << (8 * j);
                const bool fj = (fin >> j) & 1u;
                pos[j] = fj ? w.pos[o] : pos[j];
                f[j] = fj ? kFuelInit : f[j];
            }
        }
        G.template load_episode<kRec>(late_args(), at, stamp_lane(fin));
    }
    // x, y, fuel, done and err are final here (cargo loss and arrival change none)
    uint32_t rec_x = 0, rec_y = 0, rec_cut = 0;
    uint32_t ox, oy, dn = 0, ee = 0;
    pack_pos(pos, ox, oy);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dn |= ((dead >> j) & 1u) << (8 * j);
        ee |= (uint32_t)(err[j] & 0xff) << (8 * j);
    }
    if constexpr (kRec) {  // replay_end4_kernel's flags and s' fuel now; x / y held to the end
        rec_x = ox;
        rec_y = oy;
        uint32_t flags4 = 0;
        float nf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool raised = err[j] != SE_ERR_OK;
            nf[j] = (float)f[j];
            flags4 |= (((dead >> j) & 1u ? (uint32_t)kRecDone : 0u) | (raised ? (uint32_t)kRecInvalid : 0u)) << (8 * j);
            rec_cut |= (uint32_t)raised << (8 * j);
        }
        record_early(late_args(), base, flags4, nf);
    }
    if constexpr (kKeep) {
        G.x = ox;
        G.y = oy;
#pragma unroll
        for (int j = 0; j < 4; ++j) G.f[j] = f[j];
        O->dn = dn;
        O->ee = ee;
    } else {
        const se_state& S = A.st;
        __builtin_amdgcn_sched_barrier(0);  // the fuel halves back to back (store_moved)
        store4u8(S.x, at, ox);
        store4u8(S.y, at, oy);
        store4(S.fuel, at, f);
        store4u8(S.done, at, dn);
        store4u8(reinterpret_cast<uint8_t*>(S.err), at, ee);
        __builtin_amdgcn_sched_barrier(0);
        // (these seven lines shared with store_moved as one forceinline helper: tried, and the
        // three agent step_tail_kernel instantiations compiled to other code; the rest did not)
    }
    TRACE_STAMP(6);

    // --- second half: cargo loss (_calculate_cargo_loss :169-200), contract v5: the
    // r-th env of the quad whose gate fired takes block LOSS_r (word 0 the loss type,
    // words 1-3 the Beta(2, 2) uniforms); only waves with a firing gate run it
    [[maybe_unused]] uint32_t used_loss = 0, used_beta = 0;
    if constexpr (kReplay) {
        if (fire) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool fj = (fire >> j) & 1u;
                const double lt = tt[j], beta = tb[j];
                const bool partial = (cg[j] != 0) & (lt >= 0.1) & (lt <= 0.9);
                const int part = (int)(beta * (double)cg[j]);  // int(betavariate(2,2) * cargo) (:195-197)
                const int some = lt > 0.9 ? cg[j] : part;
                const int loss = ((lt < 0.1) | (cg[j] == 0)) ? 0 : some;
                const double rl = r[j] + (double)loss * -3.0;
                r[j] = fj ? rl : r[j];
                cg[j] = fj ? cg[j] - loss : cg[j];
                used_loss |= (uint32_t)fj << j;
                used_beta |= (uint32_t)(fj & partial) << j;
                need |= (uint32_t)(fj & ((lt != lt) | (partial & (beta != beta)))) << j;
            }
        }
    } else if (fire) {
        uint32_t lt[4], v1[4], v2[4], v3[4];
        const uint32_t rk[4] = {0u, fire & 1u, (uint32_t)__popc(fire & 3u), (uint32_t)__popc(fire & 7u)};
        U4 rr = kSpecLoss ? D.loss0 : draw(qk, t, loss_slot(0));
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
                rr = draw(qk, t, loss_slot(q));
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
            // beta = the median of the three words * 2^-32 (the conversion is monotone)
            const uint32_t lo = min(v1[j], v2[j]), hi = max(v1[j], v2[j]);
            const uint32_t med = max(lo, min(hi, v3[j]));  // v_med3_u32
            const int part = beta_part(med, cg[j]);
            const int some = lt[j] > kTypeHi ? cg[j] : part;
            const int loss = lt[j] < kTypeLo ? 0 : some;
            const bool fj = (fire >> j) & 1u;
            const double rl = r[j] + (double)loss * -3.0;  // int(loss * -3) exactly, then += (:323)
            r[j] = fj ? rl : r[j];
            cg[j] = fj ? cg[j] - loss : cg[j];
        }
    }
    // arrival (:325-337): +2 cargo, cargo 0, origin = dest, a new destination != origin
    if (arrive) {
        [[maybe_unused]] U4 ab{{0u, 0u, 0u, 0u}};
        if constexpr (!kReplay) ab = draw(qk, t, kSlotArrive);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool aj = (arrive >> j) & 1u;
            const double ra = (r[j] + (double)(2 * cg[j])) + 10.0;
            int nd;
            if constexpr (kReplay) {
                nd = td[j];
                need |= (uint32_t)(aj & (nd < 0)) << j;
            } else {
                nd = pick_other(ab.v[j], P, dst[j]);
            }
            r[j] = aj ? ra : r[j];
            cg[j] = aj ? 0 : cg[j];
            org[j] = aj ? dst[j] : org[j];
            dst[j] = aj ? nd : dst[j];
        }
    }
    float rw[4], epr[4];
    int32_t epl[4];  // kRec: the running length after this step (0 for a finished episode)
    uint32_t oo = 0, od = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rw[j] = (float)r[j];  // one rounding of the reference's f64 reward
        epr[j] = 0.0f;
        epl[j] = 0;
        if constexpr (kAuto) {
            const bool fj = (fin >> j) & 1u;
            F.ret[j] = G.e[j] + rw[j];
            F.len[j] = (int32_t)(t + 1u - G.l[j]);  // stamps are loaded where fin (kRec: everywhere)
            if (fj) {
                bs.ret += (double)F.ret[j];
                bs.eps += 1;
                bs.len += F.len[j];
            }
            epr[j] = fj ? 0.0f : F.ret[j];
            epl[j] = fj ? 0 : F.len[j];
            cg[j] = fj ? 0 : cg[j];
            org[j] = fj ? byte_of(reset_o, j) : org[j];
            dst[j] = fj ? byte_of(reset_d, j) : dst[j];
        }
        oo |= (uint32_t)(org[j] & 0xff) << (8 * j);
        od |= (uint32_t)(dst[j] & 0xff) << (8 * j);
    }
    if constexpr (kAuto) F.mask = fin;
    if constexpr (kKeep) {
        G.org = oo;
        G.dst = od;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            G.c[j] = cg[j];
            O->rw[j] = rw[j];
        }
        return;
    }
    const se_state& S = late_args().st;
    store4u8(S.origin, at, oo);
    store4u8(S.dest, at, od);
    store4(S.cargo, at, cg);
    store4(S.reward, at, rw);
    if constexpr (kAuto) {
        store4(S.ep_return, at, epr);
        store_stamps(S, at, G.l, fin, t, stamp_lane(fin));
    }
    if constexpr (kRec) F.cut = record_group(late_args(), base, rw, rec_x, rec_y, oo, od, rec_cut, epl);
    if constexpr (kReplay) {
        se_tape* tp = A.tape + base;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(kFull || base + j < n)) continue;
            const bool mv = do_move[j];
            tp[j].used = (int32_t)((mv ? (uint32_t)kUsedFuelGate : 0u) | (moved[j] ? (uint32_t)kUsedMoved : 0u) |
                                   (((used_loss >> j) & 1u) ? (uint32_t)kUsedLossType : 0u) |
                                   (((used_beta >> j) & 1u) ? (uint32_t)kUsedBeta : 0u) |
                                   (((arrive >> j) & 1u) ? (uint32_t)kUsedArrive : 0u));
            if ((need >> j) & 1u) {  // the env as it was: later stores of this thread win
                const int64_t i = base + j;
                S.x[i] = (uint8_t)byte_of(G.x, j);
                S.y[i] = (uint8_t)byte_of(G.y, j);
                S.fuel[i] = G.f[j];
                S.cargo[i] = G.c[j];
                S.origin[i] = (uint8_t)byte_of(G.org, j);
                S.dest[i] = (uint8_t)byte_of(G.dst, j);
                S.reward[i] = 0.0f;
                S.done[i] = 0;
                S.err[i] = (int8_t)SE_ERR_NEED_DRAW;
            }
        }
    }
}
