#pragma once
// qnet_parts.h — the device pieces the DQN kernels share (policy_kernel, policy_x3_kernel,
// qnet_rollout_kernel, qtrain.h's tile kernel): the vector types, the three-way bf16 split (split3,
// split3x2), the bf16 kernels' fc1 operand (obs_frag), bias
// fragments, relu + packing, an env's valid rows (EnvValid), the masked first-maximum argmax,
// the policy kernels' argument block and epilogue (PolicyArgs, merge_halves, explore_choice,
// choose_store), and the split-bf16 k-step (mfma_bf16, khalf_x3, x3_frags, split_pair).
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace after qnet_image.h: not a stand-alone header. Uses qnet_image.h (QnetDims), world.h
// (WorldDims, LdsWorld), env_core.h (env_key), philox.h (draw, u32, uniform_int, kSlotPolicy) and
// include/shipenv.h (se_state).

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// v = p0 + p1 + p2, each the bf16 rounding of the remainder (exact f32 subtractions)
__device__ __forceinline__ void split3(float v, __bf16& p0, __bf16& p1, __bf16& p2) {
    p0 = (__bf16)v;
    const float r1 = v - (float)p0;
    p1 = (__bf16)r1;
    p2 = (__bf16)(r1 - (float)p1);
}

// fc1's B operand of lane half h, the observation row (preprocess_state) in fc1_col's order:
// ff is torch's .float() of the f64 fuel, as bf16 hi + lo so fc1 sees ~16 bits of it; lane half 1
// holds 1.0 at k = 8..10 against the three bf16 parts of b1 that the kernels' staging loops put there
__device__ __forceinline__ bf16x8 obs_frag(int x, int y, float ff, int origin, int dest, int h) {
    const __bf16 fh = (__bf16)ff, fl = (__bf16)(ff - (float)fh);
    bf16x8 ob;
    ob[0] = (__bf16)(float)x;
    ob[1] = (__bf16)(float)y;
    ob[2] = fh;
    ob[3] = fl;
    ob[4] = fh;
    ob[5] = fl;
    ob[6] = (__bf16)(float)origin;
    ob[7] = (__bf16)(float)dest;
    if (h) {  // k = 8..10: 1.0 against the bias parts, 11..15 padding
        ob = bf16x8{};
        ob[0] = ob[1] = ob[2] = (__bf16)1.0f;
    }
    return ob;
}

// accumulator initial value: bias rows (reg & 3) + 8 (reg >> 2) + 4h of a 32-row tile
__device__ __forceinline__ f32x16 bias_frag(const float* b) {
    const float4 a = *reinterpret_cast<const float4*>(b), c = *reinterpret_cast<const float4*>(b + 8),
                 d = *reinterpret_cast<const float4*>(b + 16), e = *reinterpret_cast<const float4*>(b + 24);
    return f32x16{a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y, e.z, e.w};
}

// registers 8s..8s+7 -> the bf16 B fragment of k-step s, then relu. Rounding to bf16
// keeps the sign (a small negative value rounds to -0), so relu after the rounding
// gives the bits relu before it did. The relu is a signed integer max with 0 on each
// bf16 pattern (a non-negative value orders like its int16 pattern, a negative one has
// the sign bit), two lanes per op: v_cvt_pk_bf16_f32 + v_pk_max_i16, 16 ops per
// 32-row tile where an f32 max per register took 24.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
// a - b on two f32 lanes as two v_sub_f32: the vector form compiles to v_pk_add_f32, whose
// issue beside MFMAs costs more than two scalar subtractions (MI355X_MICROARCH.md,
// per-instruction constants; measured about even, profiles/r05/ab_policy_f32_scalarsub.jsonl).
__device__ __forceinline__ f32x2 sub2(f32x2 a, f32x2 b) {
    float r0, r1;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r0) : "v"(a[0]), "v"(b[0]));
    asm("v_sub_f32 %0, %1, %2" : "=v"(r1) : "v"(a[1]), "v"(b[1]));
    return f32x2{r0, r1};
}
// split3 on two f32 lanes: v = p0 + p1 + p2, the remainders by sub2
__device__ __forceinline__ void split3x2(f32x2 v, bf16x2& p0, bf16x2& p1, bf16x2& p2) {
    p0 = __builtin_convertvector(v, bf16x2);
    const f32x2 r1 = sub2(v, __builtin_convertvector(p0, f32x2));
    p1 = __builtin_convertvector(r1, bf16x2);
    p2 = __builtin_convertvector(sub2(r1, __builtin_convertvector(p1, f32x2)), bf16x2);
}
typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
__device__ __forceinline__ void relu_pack(const f32x16& c, bf16x8 (&out)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        u32x4 w;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const bf16x2 b = __builtin_convertvector(f32x2{c[8 * s + 2 * p], c[8 * s + 2 * p + 1]}, bf16x2);
            const i16x2 i = __builtin_elementwise_max(__builtin_bit_cast(i16x2, b), i16x2{0, 0});
            w[p] = __builtin_bit_cast(uint32_t, i);
        }
        out[s] = __builtin_bit_cast(bf16x8, w);
    }
}

// bits i of [0, 32) with lo <= i <= hi
__device__ __forceinline__ uint32_t range_bits(int lo, int hi) {
    lo = max(lo, 0);
    hi = min(hi, 31);
    const uint32_t top = hi >= 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u);
    const uint32_t low = lo >= 32 ? 0xffffffffu : ((1u << lo) - 1u);
    return lo > hi ? 0u : (top & ~low);
}

// is_valid_action (dqn.py:125-175) of one env, as row ranges of a fc3 layout: moves
// always; SELECT p at the ship's cell and != origin; TAKE_CARGO / TAKE_FUEL at a port
// with 0 < amount <= stock. These helpers are the f32 policy kernel's form of the bf16
// kernel's inline epilogue (policy_bf16.h's policy_kernel keeps it inline: in helper form the
// compiler unrolled its fc3 loop and spilled SGPRs at its 128-VGPR budget); the GPU tests
// require both kernels to choose the same first maximum from the same Q rows.
struct EnvValid {
    int cur, cst, fst;       // port on the ship's cell (-1), its stocks capped to the amounts
    int c_lo, f_lo;          // the layout's first TAKE_CARGO / TAKE_FUEL rows (wave-uniform)
    __device__ __forceinline__ int c_hi() const { return c_lo + cst - 1; }
    __device__ __forceinline__ int f_hi() const { return f_lo + fst - 1; }
    uint64_t sel;            // SELECT: bit p for each port on the ship's cell other than the origin
};
__device__ __forceinline__ EnvValid env_valid(const LdsWorld& w, const QnetDims& q, const uint64_t* SAME, int x,
                                              int y, int origin) {
    EnvValid v;
    v.cur = w.port_at(x, y);
    v.cst = v.cur >= 0 ? min(w.pcargo(max(v.cur, 0)), 49) : 0;
    v.fst = v.cur >= 0 ? min(w.pfuel(max(v.cur, 0)), 199) : 0;
    v.c_lo = q.cargo_row1();
    v.f_lo = q.fuel_row1();
    v.sel = v.cur >= 0 ? SAME[max(v.cur, 0)] & ~(origin >= 0 ? 1ull << origin : 0ull) : 0ull;
    return v;
}

// env_valid from the ship's cell code and the stocks of its first port (read earlier, so
// the two dependent world reads are in flight during MFMA work)
__device__ __forceinline__ EnvValid env_valid_from(const LdsWorld& w, const QnetDims& q, const uint64_t* SAME, int code,
                                                   int2 stock, int origin) {
    EnvValid v;
    v.cur = w.port_of_code(code);
    v.cst = v.cur >= 0 ? min(stock.y, 49) : 0;
    v.fst = v.cur >= 0 ? min(stock.x, 199) : 0;
    v.c_lo = q.cargo_row1();
    v.f_lo = q.fuel_row1();
    v.sel = v.cur >= 0 ? SAME[max(v.cur, 0)] & ~(origin >= 0 ? 1ull << origin : 0ull) : 0ull;
    return v;
}

// can any row of tile mt be valid for this env (a tile no env of the wave can choose from
// is skipped, MFMAs included)
__device__ __forceinline__ bool tile_maybe(const EnvValid& v, int mt, int P) {
    const int base = mt * 32, top = base + 31;
    return (int)(mt == 0) | (int)((v.cur >= 0) & (base < 4 + P)) |
           (int)((v.cst > 0) & (v.c_lo <= top) & (v.c_hi() >= base)) | (int)((v.fst > 0) & (v.f_lo <= top) & (v.f_hi() >= base));
}

// valid rows of tile mt as bits of the tile
__device__ __forceinline__ uint32_t tile_mask(const EnvValid& v, int mt, int P) {
    const int base = mt * 32;
    uint32_t m = range_bits(-base, 3 - base) | range_bits(v.c_lo - base, v.c_hi() - base) |
                 range_bits(v.f_lo - base, v.f_hi() - base);
    if (base < 4 + P) {  // SELECT rows 4 + p live in this tile (uniform): sel shifted by 4 - base
        const int sh = base - 4;
        m |= (uint32_t)(sh < 0 ? v.sel << -sh : (sh < 64 ? v.sel >> sh : 0ull));
    }
    return m;
}

// the masked first maximum over one fc3 tile's accumulator (ascending rows), registers
// outside the wave-uniform mask rm skipped
__device__ __forceinline__ void tile_argmax(const f32x16& c, uint32_t m, uint32_t rm, int base, int h, float& best,
                                            int& bidx) {
    m >>= 4 * h;  // register reg holds row base + 4h + (reg & 3) + 8 (reg >> 2)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        if (!((rm >> reg) & 1u)) continue;
        const int i = (reg & 3) + 8 * (reg >> 2);
        const bool better = ((m >> i) & 1u) && c[reg] > best;  // ascending rows: first max
        best = better ? c[reg] : best;
        bidx = better ? base + 4 * h + i : bidx;
    }
}

// bias rows of a fc3 tile, -inf where bit (reg & 3) + 8 (reg >> 2) of m is clear (the row
// is invalid for this env): its Q stays -inf through the MFMAs and never wins the argmax.
// Two VALU per register, a sign-extended one-bit field (v_bfe_i32) and a bitwise select
// (v_bfi_b32): no compare, so no VALU-written lane mask and none of the wait states a
// compare -> v_cndmask pair costs. The select is inline asm: written as (c & t) | (~t & -inf)
// in C, ROCm 7.2's hipcc folds it into v_bitop3_b32 chains that read ONE bias dword for all 16
// registers (a miscompile, reproduced in a 20-line kernel; tests/test_gpu_policy.py catches it).
__device__ __forceinline__ f32x16 masked_bias(const float* b, uint32_t m) {
    f32x16 c = bias_frag(b);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = (reg & 3) + 8 * (reg >> 2);
        const uint32_t t = (uint32_t)((int32_t)(m << (31 - i)) >> 31);  // all ones: row valid
        float r;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(t), "v"(c[reg]), "v"(0xff800000u));
        c[reg] = r;
    }
    return c;
}

// the first maximum over registers 4j..4j+3 of a masked tile (invalid rows are -inf: one
// compare and two selects per register, no validity test and no per-register branch), the
// winner's tile-local row kept as an inline constant (bt); after part 3 the caller adds the
// tile's base once if the tile raised the maximum (best != best0)
__device__ __forceinline__ void argmax_local_part(const f32x16& c, float& best, int& bt, int j) {
#pragma unroll
    for (int reg = 4 * j; reg < 4 * j + 4; ++reg) {
        const bool better = c[reg] > best;
        best = better ? c[reg] : best;
        bt = better ? (reg & 3) + 8 * (reg >> 2) : bt;
    }
}

// A fuel that is not finite (inf or NaN as f32) makes every Q of its env NaN in exact
// arithmetic (its bf16 parts are inf and inf - inf); the ReLUs here do not keep every NaN
// (relu_pack is an integer max on the bf16 bits, which sends a NaN with the sign bit set to 0), so
// the rule is applied where the env's results leave the kernel: its q_out row is NaN and it has
// no row above -inf, so it plays action 0 (include/shipenv.h).
__device__ __forceinline__ bool fuel_finite(float ff) { return fabsf(ff) < INFINITY; }

__device__ __forceinline__ void tile_q_out(float* q_out, int64_t ldq, int rows, const f32x16& c, int64_t e, int base,
                                           int h, float ff) {
    const bool fin = fuel_finite(ff);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {  // the full layout: row = action
        const int row = base + 4 * h + (reg & 3) + 8 * (reg >> 2);
        if (row < rows) q_out[e * ldq + row] = fin ? c[reg] : NAN;
    }
}

// ------------------------------------------------------------------ the policy step
struct PolicyArgs {
    const uint32_t* world;
    WorldDims dims;
    const uint4* qimg;
    QnetDims q;
    int64_t n, env_base;
    uint64_t seed;
    uint32_t t;
    double eps;
    se_state st;
    int32_t* actions;
    float* q_out;
    int64_t ldq;
    // remember's state and action (se_policy_record): the replay ring's s / a columns
    // at slot (rec_head + env) mod rec_cap, or null
    uint32_t* rec_pos;
    float* rec_fuel;
    int32_t* rec_act;
    int64_t rec_head, rec_cap;
    // the visiting order (order_chunk): null = position order; else workgroup b visits the
    // envs [b * chunk, (b + 1) * chunk) in the order it writes to order[b * chunk ...]
    uint32_t* order;
    int64_t chunk;
    int32_t lds_list;  // >= 0: the bf16 kernel keeps the list in LDS at this byte offset (u16 per env)
};

// the two lane halves hold the same env: larger value, then lower index (both halves end with
// the same winner); returns the winner's row
__device__ __forceinline__ int merge_halves(float best, int bidx) {
    const float ob2 = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bidx, 32);
    if (ob2 > best || (ob2 == best && oi < bidx)) {
        best = ob2;
        bidx = oi;
    }
    return bidx;
}

// random.choice(valid_actions) (agents/dqn.py:192) by the word `pick`: the k-th valid action,
// ascending, of the 4 moves, the SELECT ports of sel and the amounts 1..cst, 1..fst
__device__ __forceinline__ int explore_choice(uint64_t sel, int cst, int fst, int P, uint32_t pick) {
    const int nsel = __popcll(sel);
    int k = uniform_int(pick, (uint32_t)(4 + nsel + cst + fst));
    if (k < 4) return k;
    if ((k -= 4) < nsel) {  // the k-th port of sel, ascending
        uint64_t b = sel;
        for (; k > 0; --k) b &= b - 1;
        return 4 + __builtin_ctzll(b);
    }
    k -= nsel;
    return k < cst ? 5 + P + k : 55 + P + (k - cst);  // amounts k + 1 (action space)
}

// epsilon-greedy on the merged winner row bidx (choose_action :186-203) and the action / replay
// record stores, by lane half 0 of a live env
#define CHOOSE_STORE(sel, cst, fst, e, live, h, bidx, x8, y8, o8, d8, ff)                                        \
    choose_store(q, sel, cst, fst, e, live, h, bidx, x8, y8, o8, d8, ff, A.actions, A.eps, A.seed, A.env_base, A.t, \
                 A.rec_pos, A.rec_fuel, A.rec_act, A.rec_head, A.rec_cap)
__device__ __forceinline__ void choose_store(const QnetDims& q, uint64_t sel, int cst, int fst, int64_t e, bool live,
                                             int h, int bidx, uint32_t x8, uint32_t y8, uint32_t o8, uint32_t d8,
                                             float ff, int32_t* actions, double eps, uint64_t seed, int64_t env_base,
                                             uint32_t t, uint32_t* rec_pos, float* rec_fuel, int32_t* rec_act,
                                             int64_t rec_head, int64_t rec_cap) {
    if (h == 0 && live) {
        // no valid action, or a fuel that is not finite: 0 (:188-189)
        int act = ((bidx == 0x7fffffff) | !fuel_finite(ff)) ? 0 : q.action_of_row(bidx);
        if (eps > 0.0) {
            const U4 d = draw(env_key(seed, env_base + e), t, kSlotPolicy);
            // np.random.rand() <= epsilon (:191)
            if (u32(d.v[0]) <= eps) act = explore_choice(sel, cst, fst, q.P, d.v[1]);
        }
        actions[e] = act;
        if (rec_pos) {  // replay_begin_kernel's record, from the state already in registers
            int64_t slot = rec_head + e;
            slot -= slot >= rec_cap ? rec_cap : 0;
            rec_pos[slot] = x8 | y8 << 8 | o8 << 16 | d8 << 24;
            rec_fuel[slot] = ff;
            rec_act[slot] = act;
        }
    }
}

// an env's epilogue: its two lane halves merged, then choose_store
#define FINISH_ENV(v, e, live, h, best, bidx, x8, y8, o8, d8, ff) \
    CHOOSE_STORE(v.sel, v.cst, v.fst, e, live, h, merge_halves(best, bidx), x8, y8, o8, d8, ff)

// relu as a signed integer max with 0 on the f32 pattern (a non-negative float orders like
// its int pattern; a negative one, -0 included, becomes +0): one v_max_i32, where fmaxf
// also canonicalised its operand (two v_max_f32 per element)
__device__ __forceinline__ float relu_bits(float x) {
    return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0));
}

// pair q (0..7) of the relu + 3-way split of tile c into out: elements 2p, 2p + 1 of
// k-step s (q = 4s + p), both stages (relu_split3 in 8 pieces of about 11 VALU)
__device__ __forceinline__ void split_pair(const f32x16& c, bf16x8 (&out)[2][3], int q) {
    const int s = q >> 2, p = q & 3;
    bf16x2 a, b, e;
    split3x2(f32x2{relu_bits(c[8 * s + 2 * p]), relu_bits(c[8 * s + 2 * p + 1])}, a, b, e);
    out[s][0][2 * p] = a[0];
    out[s][0][2 * p + 1] = a[1];
    out[s][1][2 * p] = b[0];
    out[s][1][2 * p + 1] = b[1];
    out[s][2][2 * p] = e[0];
    out[s][2][2 * p + 1] = e[1];
}

// relu of one 32-row f32 tile, split into the three bf16 B fragments of its two k-steps
__device__ __forceinline__ void relu_split3(const f32x16& c, bf16x8 (&out)[2][3]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) split_pair(c, out, q);
}

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// the three part fragments of fragment f (image order [f][part][lane])
__device__ __forceinline__ void x3_frags(const bf16x8* W, int f, int lane, bf16x8 (&wf)[3]) {
    wf[0] = W[f * 192 + lane];
    wf[1] = W[f * 192 + 64 + lane];
    wf[2] = W[f * 192 + 128 + lane];
}

// c + W x over one k-step as its two halves: the six part products, smallest first
__device__ __forceinline__ f32x16 khalf_x3(const bf16x8 (&w)[3], const bf16x8 (&x)[3], f32x16 c, int half) {
    if (half == 0) {
        c = mfma_bf16(w[0], x[2], c);
        c = mfma_bf16(w[1], x[1], c);
        c = mfma_bf16(w[2], x[0], c);
    } else {
        c = mfma_bf16(w[0], x[1], c);
        c = mfma_bf16(w[1], x[0], c);
        c = mfma_bf16(w[0], x[0], c);
    }
    return c;
}

// tile_argmax over registers 4j..4j+3 only (j = 0..3 in order is tile_argmax)
__device__ __forceinline__ void tile_argmax_part(const f32x16& c, uint32_t m, uint32_t rm, int base, int h,
                                                 float& best, int& bidx, int j) {
    m >>= 4 * h;
#pragma unroll
    for (int reg = 4 * j; reg < 4 * j + 4; ++reg) {
        if (!((rm >> reg) & 1u)) continue;
        const int i = (reg & 3) + 8 * (reg >> 2);
        const bool better = ((m >> i) & 1u) && c[reg] > best;
        best = better ? c[reg] : best;
        bidx = better ? base + 4 * h + i : bidx;
    }
}
