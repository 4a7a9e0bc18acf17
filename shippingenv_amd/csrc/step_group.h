#pragma once
// step_group.h — the step of one group of 4 envs from typed actions, with Philox
// draws or a replayed tape: BlockStats, Finished, store_moved / store_rest and
// step_group (se_step_typed, se_step_replay, se_step_agent_replay).
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld), env_core.h (env_begin / env_finish, replay_env,
// decode_agent, reset_ship) and step_io.h (StepArgs, Group, At, the stores).

// Per-thread episode statistics of the finished episodes. Counts are integers:
// summed as doubles they were exact anyway, and they hold two fewer registers.
struct BlockStats {
    double ret = 0.0;
    int32_t eps = 0;
    int64_t len = 0;
};

// Finished episodes of one group (auto-reset): bit j of `mask` for env base+j.
struct Finished {
    uint32_t mask = 0;
    float ret[4];
    int32_t len[4];
    uint32_t cut = 0;  // se_step_record: bit j = env j of the group restarts (cut)
};

// x, y, fuel, done, err of a group's 4 envs: final once the first half has run
// (cargo loss and arrival change none of them).
template <bool kFull>
__device__ __forceinline__ void store_moved(const se_state& S, At<kFull> at, const Ship (&s)[4],
                                            const Pending (&p)[4]) {
    uint32_t ox = 0, oy = 0, dn = 0, ee = 0;
    double fuel[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t sh = 8u * (uint32_t)j;
        ox |= (uint32_t)(s[j].x & 0xff) << sh;
        oy |= (uint32_t)(s[j].y & 0xff) << sh;
        dn |= (uint32_t)p[j].dead << sh;
        ee |= (uint32_t)(p[j].e & 0xff) << sh;
        fuel[j] = s[j].fuel;
    }
    // The two 16-byte halves of a lane's 32 bytes of fuel are two store
    // instructions, each writing every other 16 bytes of the wave's span. Issued
    // apart, the nontemporal halves reach memory as separate partial-line writes
    // (measured: +4.5 MB per launch at N = 2^20); the scheduling barriers keep the
    // pair, and the whole group of stores, back to back.
    __builtin_amdgcn_sched_barrier(0);
    store4u8(S.x, at, ox);
    store4u8(S.y, at, oy);
    store4(S.fuel, at, fuel);
    store4u8(S.done, at, dn);
    store4u8(reinterpret_cast<uint8_t*>(S.err), at, ee);
    __builtin_amdgcn_sched_barrier(0);
}

// cargo, origin, dest, reward (+ the running returns): final after the second half.
template <bool kAuto, bool kFull>
__device__ __forceinline__ void store_rest(const se_state& S, At<kFull> at, const Ship (&s)[4],
                                           const float (&rw)[4], const float (&epr)[4]) {
    uint32_t oo = 0, od = 0;
    int32_t cargo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t sh = 8u * (uint32_t)j;
        oo |= (uint32_t)(s[j].origin & 0xff) << sh;
        od |= (uint32_t)(s[j].dest & 0xff) << sh;
        cargo[j] = s[j].cargo;
    }
    store4u8(S.origin, at, oo);
    store4u8(S.dest, at, od);
    store4(S.cargo, at, cargo);
    store4(S.reward, at, rw);
    if constexpr (kAuto) store4(S.ep_return, at, epr);
}

// Step the 4 envs 4k..4k+3 of one group (base = 4k). Production draws are Philox
// quad blocks at counter (k, t, slot): word j belongs to env 4k+j (RNG contract,
// DESIGN.md). Each block is drawn only when some env of the quad consumes it, so
// the draws are lane-uniform branches instead of a branch per env and draw:
//   FUEL   every step           GATE    a move with 0 < cargo < 50
//   LOSS   the gate fired       BETA1-3 a partial loss (Beta(2,2) = median of 3)
//   ARRIVE an arrival           RESET, RESET_DEST  an auto-reset
// Replay takes every variate from the env's tape record instead.
// Registers: x, y, fuel, done and err are stored as soon as the first half has
// run (and auto-reset has replaced the finished envs' positions), so only cargo,
// origin, dest and the reward stay live across the loss / arrival blocks.
template <bool kTyped, bool kReplay, bool kAuto, bool kFull, bool kNt = false>
__device__ __forceinline__ void step_group(const StepArgs& A, const LdsWorld& w,
                                           Group<kTyped, kAuto, kNt>& G, At<kFull> at, BlockStats& bs,
                                           Finished& F) {
    const se_state& S = A.st;
    const int64_t n = A.n, base = at.base;
    int ty[4], va[4], vb[4], er[4];
    Ship s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (kTyped) {
            ty[j] = G.a[j];
            va[j] = G.p[j];
            vb[j] = G.q[j];
            er[j] = SE_ERR_OK;
        } else {
            er[j] = decode_agent(w.P, G.a[j], ty[j], va[j], vb[j]);
        }
        s[j] = Ship{byte_of(G.x, j), byte_of(G.y, j), G.f[j], G.c[j], byte_of(G.org, j), byte_of(G.dst, j)};
    }
    const Key qk = env_key(A.seed, (A.env_base + base) >> 2);
    const uint32_t t = A.t;
    Pending p[4];

    if constexpr (kReplay) {
        // one env at a time; a missing variate (NEED_DRAW) leaves its env untouched
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = base + j;
            const bool live = kFull || i < n;
            se_tape* tp = A.tape + (live ? i : 0);
            const double uf = live ? tp->u_fuel : 0.0, ug = live ? tp->u_gate : 0.0;
            const uint32_t used = replay_env(w, s[j], p[j], er[j], ty[j], va[j], vb[j], uf, ug, tp);
            if (live) {
                tp->used = (int32_t)used;
                if (S.reward64) S.reward64[i] = p[j].r;
            }
        }
        store_moved(S, at, s, p);
        float rw[4], none[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) rw[j] = (float)p[j].r;
        store_rest<false>(S, at, s, rw, none);
        (void)bs;
        (void)F;
    } else {
        bool gate_needed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            gate_needed |= (er[j] == SE_ERR_OK) & needs_gate<!kTyped>(w, s[j], ty[j], va[j], vb[j]);
        const U4 fb = draw(qk, t, kSlotFuel);
        U4 gb{{0u, 0u, 0u, 0u}};
        if (gate_needed) gb = draw(qk, t, kSlotGate);
        uint32_t fire = 0, arrive = 0, fin = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = env_begin<!kTyped, false>(w, s[j], er[j], ty[j], va[j], vb[j], (double)fb.v[j], 0.0, gb.v[j]);
            fire |= (uint32_t)p[j].fires << j;
            arrive |= (uint32_t)p[j].arrive << j;
            fin |= (uint32_t)((kFull || base + j < n) & p[j].dead) << j;
        }
        // The per-env flags travel as these VGPR bit masks from here on: opaque to
        // the compiler, so it does not keep 4 x 3 lane masks (SGPR pairs) live
        // across the draw blocks below, which spilled them to VGPR lanes.
        asm volatile("" : "+v"(fire), "+v"(arrive), "+v"(fin));
        // auto-reset (:227-243) of the envs that ran out of fuel: their position and
        // fuel now, cargo / origin / dest after the second half (whose reward the
        // finished episode still collects). Contract v5: the r-th finishing env of the
        // quad takes block RESET_r (word 0 origin, word 1 destination), as LOSS_r.
        uint32_t reset_o = 0, reset_d = 0;  // reset origin / dest bytes of the 4 envs
        if constexpr (kAuto) {
            if (fin) {
                uint32_t ow[4], dw[4];
                {
                    const uint32_t rk[4] = {0u, fin & 1u, (uint32_t)__popc(fin & 3u), (uint32_t)__popc(fin & 7u)};
                    U4 r = draw(qk, t, reset_slot(0));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ow[j] = r.v[0];
                        dw[j] = r.v[1];
                    }
#pragma unroll
                    for (uint32_t q = 1; q < 4; ++q) {
                        if (__popc(fin) > q) {
                            r = draw(qk, t, reset_slot(q));
#pragma unroll
                            for (int j = (int)q; j < 4; ++j) {
                                ow[j] = rk[j] >= q ? r.v[0] : ow[j];
                                dw[j] = rk[j] >= q ? r.v[1] : dw[j];
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    Ship r;
                    reset_ship(w, r, ow[j], dw[j]);
                    reset_o |= (uint32_t)r.origin << (8 * j);
                    reset_d |= (uint32_t)r.dest << (8 * j);
                    const bool f = (fin >> j) & 1u;
                    s[j].x = f ? r.x : s[j].x;
                    s[j].y = f ? r.y : s[j].y;
                    s[j].fuel = f ? r.fuel : s[j].fuel;
                }
            }
            G.load_episode(late_args(), at, stamp_lane(fin));
        }
        store_moved(S, at, s, p);

        // Cargo loss (contract v5): the r-th env of the quad whose gate fired takes
        // the whole block LOSS_r: word 0 the loss type, words 1-3 the Beta(2, 2)
        // uniforms. LOSS_0 runs whenever any env of the wave fired; LOSS_1..3 only
        // where a quad had two or more (a few percent of waves). Envs take the
        // words of the block matching their rank; non-firing envs ignore theirs.
        uint32_t lt[4], v1[4], v2[4], v3[4];
        {
            const uint32_t f1 = fire & 1u, f2 = __popc(fire & 3u), f3 = __popc(fire & 7u);
            const uint32_t rk[4] = {0u, f1, f2, f3};
            U4 r{{0u, 0u, 0u, 0u}};
            if (fire) r = draw(qk, t, loss_slot(0));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lt[j] = r.v[0];
                v1[j] = r.v[1];
                v2[j] = r.v[2];
                v3[j] = r.v[3];
            }
#pragma unroll
            for (uint32_t q = 1; q < 4; ++q) {
                if (fire >> q) {  // some env after the first fired too: rank q exists
                    if (__popc(fire) > q) {
                        r = draw(qk, t, loss_slot(q));
#pragma unroll
                        for (int j = (int)q; j < 4; ++j) {
                            const bool take = rk[j] >= q;
                            lt[j] = take ? r.v[0] : lt[j];
                            v1[j] = take ? r.v[1] : v1[j];
                            v2[j] = take ? r.v[2] : v2[j];
                            v3[j] = take ? r.v[3] : v3[j];
                        }
                    }
                }
            }
        }
        int kind[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int total = lt[j] > kTypeHi ? kLossTotal : kLossPartial;
            kind[j] = lt[j] < kTypeLo ? kLossNone : total;
        }
        U4 ab{{0u, 0u, 0u, 0u}};
        if (arrive) ab = draw(qk, t, kSlotArrive);
        float rw[4], epr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // beta = the median of the three words * 2^-32 (the conversion is monotone)
            const uint32_t lo = min(v1[j], v2[j]), hi = max(v1[j], v2[j]);
            const uint32_t med = max(lo, min(hi, v3[j]));  // v_med3_u32
            env_finish(s[j], p[j], kind[j], beta_part(med, s[j].cargo), pick_other(ab.v[j], w.P, s[j].dest),
                       (fire >> j) & 1u, (arrive >> j) & 1u);
            rw[j] = (float)p[j].r;  // one rounding of the reference's f64 reward
            epr[j] = 0.0f;
            if constexpr (kAuto) {
                const bool f = (fin >> j) & 1u;
                F.ret[j] = G.e[j] + rw[j];
                F.len[j] = (int32_t)(t + 1u - G.l[j]);  // stamps are loaded where fin
                if (f) {
                    bs.ret += (double)F.ret[j];
                    bs.eps += 1;
                    bs.len += F.len[j];
                }
                epr[j] = f ? 0.0f : F.ret[j];
                s[j].cargo = f ? 0 : s[j].cargo;
                s[j].origin = f ? byte_of(reset_o, j) : s[j].origin;
                s[j].dest = f ? byte_of(reset_d, j) : s[j].dest;
            }
        }
        if constexpr (kAuto) F.mask = fin;
        store_rest<kAuto>(late_args().st, at, s, rw, epr);
        if constexpr (kAuto) store_stamps(late_args().st, at, G.l, fin, t, stamp_lane(fin));
    }
}
