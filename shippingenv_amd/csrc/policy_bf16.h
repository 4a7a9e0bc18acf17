#pragma once
// policy_bf16.h — policy_kernel, the bf16 policy step (se_policy): the shape of the work is in
// qpolicy.h's head.
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace after its other fragments: not a stand-alone header. Uses qnet_image.h (QnetDims),
// qnet_parts.h (PolicyArgs, split3, obs_frag, bias_frag, masked_bias, relu_pack, range_bits,
// argmax_local_part, fuel_finite, choose_store), qnet_order.h (OrderRun), qnet_trace.h
// (X3STAMP), world.h (stage_world, LdsWorld), env_core.h (env_key) and philox.h.

// 16 waves (4 per SIMD, <= 128 VGPRs, no scratch) share one LDS copy of the network.
// Measured per launch at 2^20 envs when it was chosen (round 1 kernel): 512 threads
// 108.8 us, 768 (3 waves per SIMD, 165 VGPRs) 92.5 us, 1024 87.2 us: the fourth wave
// covers the others' MFMA -> relu -> MFMA stalls.
constexpr int kPolicyBlock = 1024;
constexpr int kPolicyWgPerCu = 1;  // resident workgroups per CU (each stages its own network copy)
constexpr int kPolicyWaves = kPolicyBlock / 64;

template <bool kQout>
__global__ __launch_bounds__(kPolicyBlock)
void policy_kernel(PolicyArgs A) {
    extern __shared__ uint4 smem[];
    X3STAMP_ANY(9);
    const QnetDims q = A.q;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t tiles = (A.n + 31) >> 5;
    // env state of one tile (lane & 31 = env); the next tile's is loaded while this one
    // computes, so the wave does not wait on HBM at the top of every tile. The first tile's
    // loads go out before the network image and the world are staged, so they overlap.
    struct EnvIn {
        double fuel;
        uint32_t x, y, o8, d8;
        int64_t e;  // the env (A.order), past A.n for the last tile's idle lanes
    };
    // the visiting order: this workgroup's chunk and its list (null: position order)
    const uint16_t* ord16 = nullptr;  // or in LDS (chunk indices)
    const uint32_t* ord = nullptr;
    int64_t c0 = 0;
    int len = 0;
    OrderRun orun;
    if (A.order) {  // loaded here, counted and placed once the image and the world are staged
        c0 = (int64_t)blockIdx.x * A.chunk;
        len = __builtin_amdgcn_readfirstlane((int)min(A.chunk, A.n - c0));  // uniform: an SGPR
        orun.load<kPolicyBlock>(A.st.x, A.st.y, c0, len);
    }
    auto load_env = [&](int64_t tile) {
        const int64_t p = tile * 32 + r;
        int64_t ei;
        bool live;
        if (ord16) {  // p < the chunk's whole tiles: its tail reads 0xffff
            const uint32_t v = ord16[p];
            live = v != 0xffffu;
            ei = live ? c0 + (int64_t)v : A.n - 1;
        } else if (ord) {  // the same in global memory, kOrderNone
            const uint32_t v = ord[p];
            live = v != kOrderNone;
            ei = live ? (int64_t)v : A.n - 1;
        } else {
            live = p < A.n;
            ei = live ? p : A.n - 1;
        }
        return EnvIn{A.st.fuel[ei], A.st.x[ei], A.st.y[ei], A.st.origin[ei], A.st.dest[ei], live ? ei : A.n};
    };
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 12) __builtin_amdgcn_s_setprio(1);
    // (the staging loop stands in qnet_rollout_kernel too: as one helper it moved this kernel's registers)
    const int qwords = q.bytes() / 16;
    // fc1's bias rides in the padding half of its single k-step: lanes 32-63 of each W1
    // fragment (k = 8..15, zero in the packed image) get the three bf16 parts of their row's
    // b1 at elements 0-2, and the input's k = 8..10 are 1.0, so the chain starts at 0 and the
    // bias is not read per tile (4 x 16-byte LDS reads per row tile)
    const int w1w = q.w1() / 16, b1f = q.b1() / 4;
    for (int i = threadIdx.x; i < qwords; i += kPolicyBlock) {
        const int k = i - w1w;  // W1 fragment (mt, lane) = k: mt = k >> 6, lane = k & 63
        if ((unsigned)k < 4u * 64u && (k & 32)) {
            const float b = reinterpret_cast<const float*>(A.qimg)[b1f + (k >> 6) * 32 + (k & 31)];
            __bf16 p0, p1, p2;
            split3(b, p0, p1, p2);
            bf16x8 v{};
            v[0] = p0;
            v[1] = p1;
            v[2] = p2;
            smem[i] = __builtin_bit_cast(uint4, v);
        } else {
            smem[i] = A.qimg[i];
        }
    }
    const LdsWorld w = stage_world(A.world, A.dims, reinterpret_cast<uint32_t*>(smem + qwords));
    if (A.order) {
        uint32_t* list = A.order + c0;
        uint64_t* wsum = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(smem) +
                                                     ((q.bytes() + 4 * A.dims.padded() + 7) & ~7));
        orun.count<kPolicyBlock>(w, A.st.x, A.st.y, c0);  // the cell codes from LDS
        if (A.lds_list >= 0) {  // the list in LDS: no global stores, fence or list reads from L2
            uint16_t* list16 = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(smem) + A.lds_list);
            orun.place<kPolicyBlock>(w, A.st.x, A.st.y, c0, len, list16, wsum);
            ord16 = list16;
        } else {
            orun.place<kPolicyBlock>(w, A.st.x, A.st.y, c0, len, list, wsum);
            ord = list;
        }
    }
    X3STAMP_ANY(10);
    [[maybe_unused]] int tile_iter = 0;  // SHIPENV_X3_TRACE: the wave's 4th tile is stamped
    const uint8_t* qb = reinterpret_cast<const uint8_t*>(smem);
    const bf16x8* W1f = reinterpret_cast<const bf16x8*>(qb + q.w1());
    const bf16x8* W2f = reinterpret_cast<const bf16x8*>(qb + q.w2());
    const bf16x8* W3f = reinterpret_cast<const bf16x8*>(qb + q.w3());
    [[maybe_unused]] const float* B1 = reinterpret_cast<const float*>(qb + q.b1());
    [[maybe_unused]] const float* B2 = reinterpret_cast<const float*>(qb + q.b2());
    const float* B3 = reinterpret_cast<const float*>(qb + q.b3());
    const uint64_t* SAME = reinterpret_cast<const uint64_t*>(qb + q.same());
    const uint32_t* REGM = reinterpret_cast<const uint32_t*>(qb + q.regm());

    const int P = q.P;
    // tiles: the chunk's (waves round robin) or all of them (striding over the grid); after
    // the order is placed (A.order: the tile loop reads the list)
    const bool ordered = A.order != nullptr;
    const int64_t my_tiles = ordered ? (len + 31) >> 5 : tiles;
    int64_t tile = ordered ? (threadIdx.x >> 6) : (int64_t)blockIdx.x * kPolicyWaves + (threadIdx.x >> 6);
    const int64_t stride = ordered ? kPolicyWaves : (int64_t)gridDim.x * kPolicyWaves;
    EnvIn nxt = load_env(tile < my_tiles ? tile : 0);
    for (; tile < my_tiles; tile += stride, ++tile_iter) {
        X3STAMP(0);
        const EnvIn cur_in = nxt;
        if (tile + stride < my_tiles) nxt = load_env(tile + stride);
        const int64_t e = cur_in.e;
        const bool live = e < A.n;
        const int x = (int)cur_in.x, y = (int)cur_in.y;
        const int origin = cur_in.o8 == SE_NONE ? -1 : (int)cur_in.o8;
        const int dest = cur_in.d8 == SE_NONE ? -1 : (int)cur_in.d8;
        const float ff = (float)cur_in.fuel;  // torch's .float() of the f64 fuel
        const bf16x8 ob = obs_frag(x, y, ff, origin, dest, h);

        bf16x8 h1[4][2], h2[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {  // fc1 + relu
            f32x16 c = {};
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1f[mt * 64 + lane], ob, c, 0, 0, 0);
            relu_pack(c, h1[mt]);
        }
        X3STAMP(1);
        // fc2 + relu one row tile per pass: no spills at 128 VGPRs (2 tiles a pass spill 7
        // registers, 4 spill 14); a pass's relu issues in the shadow of the next pass's MFMAs
        constexpr int kFc2Passes = 4, kFc2Tiles = 4 / kFc2Passes;
#pragma unroll
        for (int pass = 0; pass < kFc2Passes; ++pass) {
            f32x16 c2[kFc2Tiles];
#pragma unroll
            for (int i = 0; i < kFc2Tiles; ++i)
                c2[i] = bias_frag(B2 + (pass * kFc2Tiles + i) * 32 + 4 * h);
            static_assert(kFc2Tiles == 1, "the fragment lookahead is written for one tile per pass");
            // the tile's 8 fragments read L k-steps ahead of their MFMA, pinned in that order
            // (one LDS read, one MFMA): left to itself the compiler read each fragment right
            // before its MFMA and waited out the LDS round trip every time (L = 2 and 3
            // measure even, profiles/r05/ab_policy_bf16_la.jsonl)
            constexpr int L = 1;
            bf16x8 wf[8];
#pragma unroll
            for (int k = 0; k < L; ++k) wf[k] = W2f[(pass * 8 + k) * 64 + lane];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k + L < 8) wf[k + L] = W2f[(pass * 8 + k + L) * 64 + lane];
                c2[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k], h1[k >> 1][k & 1], c2[0], 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < L; ++k) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k + L < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
#pragma unroll
            for (int i = 0; i < kFc2Tiles; ++i) relu_pack(c2[i], h2[pass * kFc2Tiles + i]);
        }

        X3STAMP(2);
        // is_valid_action (dqn.py:125-175): moves always; SELECT p at the ship's cell
        // and != origin; TAKE_CARGO / TAKE_FUEL at a port with 0 < amount <= stock
        const int cur = w.port_at(x, y);
        const int cst = cur >= 0 ? min(w.pcargo(max(cur, 0)), 49) : 0;
        const int fst = cur >= 0 ? min(w.pfuel(max(cur, 0)), 199) : 0;
        // valid TAKE rows of this env in the layout's row space
        const int c_lo = q.cargo_row1(), c_hi = c_lo + cst - 1, f_lo = q.fuel_row1(), f_hi = f_lo + fst - 1;
        // SELECT: bit p for each port on the ship's cell other than the origin (P <= 64)
        const uint64_t sel = cur >= 0 ? SAME[max(cur, 0)] & ~(origin >= 0 ? 1ull << origin : 0ull) : 0ull;
        // (compact layouts of at most 64 rows, every greedy call of the bench) the env's valid
        // rows as one 64-bit word, built once per env tile: a fc3 tile's mask is then a shift
        // of it and "any row of this tile valid" its being nonzero, where the per-tile form
        // rebuilt three ranges and the SELECT shift for each fc3 tile
        const bool use64 = !kQout && q.mt3 <= 2;  // uniform
        uint64_t v64 = 0;
        if (use64) {
            auto range64 = [](int lo, int hi) {  // bits lo..hi, 0 <= lo, hi <= 63; empty if hi < lo
                const uint64_t top = hi >= 63 ? ~0ull : ((2ull << (hi & 63)) - 1ull);
                const uint64_t low = (1ull << (lo & 63)) - 1ull;
                return hi < lo ? 0ull : (top & ~low);
            };
            v64 = 0xfull | (sel << 4) | range64(c_lo, c_hi) | range64(f_lo, f_hi);
        }
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        if (use64) {
            // compact layouts of at most 64 rows (the bench's greedy and epsilon calls): rows
            // this env cannot take start at -inf (masked_bias, two VALU per register), so the
            // first maximum is a compare and two selects per register with no validity test and
            // no per-register branch, and fc3 tile 0's argmax runs beside tile 1's MFMAs
            constexpr int L3 = 2;  // fragments read L3 k-steps ahead (a 3-slot ring: 12 VGPRs)
            bf16x8 wf[L3 + 1];
#pragma unroll
            for (int k = 0; k < L3; ++k) wf[k] = W3f[k * 64 + lane];
            // a tile of ships at sea only (uniform; the visiting order makes them ~3 in 4):
            // rows 0-3, the moves, are each env's valid rows, registers 0-3 of lane half 0
            const bool sea = !__any(cur >= 0);
            f32x16 c = sea ? bias_frag(B3 + 4 * h) : masked_bias(B3 + 4 * h, (uint32_t)v64 >> (4 * h));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k + L3 < 8) wf[(k + L3) % (L3 + 1)] = W3f[(k + L3) * 64 + lane];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k % (L3 + 1)], h2[k >> 1][k & 1], c, 0, 0, 0);
            }
            int bt = 0, pbase = 0;
            if (sea) {
                argmax_local_part(c, best, bt, 0);
                best = h ? -INFINITY : best;  // lane half 1 holds rows 4-7
                bidx = best != -INFINITY ? bt : bidx;
            } else if (q.mt3 > 1 && __any((uint32_t)(v64 >> 32) != 0u)) {  // fc3 tile 1 (uniform)
#pragma unroll
                for (int k = 0; k < L3; ++k) wf[k] = W3f[(8 + k) * 64 + lane];
                f32x16 c1 = masked_bias(B3 + 32 + 4 * h, (uint32_t)(v64 >> 32) >> (4 * h));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k + L3 < 8) wf[(k + L3) % (L3 + 1)] = W3f[(8 + k + L3) * 64 + lane];
                    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k % (L3 + 1)], h2[k >> 1][k & 1], c1, 0, 0, 0);
                    if (k < 4) argmax_local_part(c, best, bt, k);  // tile 0's, beside tile 1's chain
                    __builtin_amdgcn_sched_barrier(0);
                }
                bidx = best != -INFINITY ? bt : bidx;
                c = c1;
                pbase = 32;
            }
            if (!sea) {
                const float best0 = best;
#pragma unroll
                for (int g = 0; g < 4; ++g) argmax_local_part(c, best, bt, g);
                bidx = best != best0 ? pbase + bt : bidx;
                bidx += bidx == 0x7fffffff ? 0 : 4 * h;  // the lane half's rows (argmax_local_part omits 4h)
            }
        }
        for (int mt = 0; mt < (use64 ? 0 : q.mt3); ++mt) {  // fc3 + the masked first-maximum argmax (other layouts)
            const int base = mt * 32, top = base + 31;
            // a tile no env of the wave can choose from is skipped, MFMAs included
            // (exact: its rows are invalid for all 32 envs); with port stocks <= 20
            // (add_port's randint(5, 20)) the valid rows sit in the first few tiles
            const bool maybe = (mt == 0) | ((cur >= 0) & (base < 4 + P)) |
                               ((cst > 0) & (c_lo <= top) & (c_hi >= base)) |
                               ((fst > 0) & (f_lo <= top) & (f_hi >= base));
            if (!kQout && !__any(maybe)) continue;
            uint32_t m = range_bits(-base, 3 - base) | range_bits(c_lo - base, c_hi - base) |
                         range_bits(f_lo - base, f_hi - base);
            if (base < 4 + P) {  // SELECT rows 4 + p live in this tile (uniform): sel shifted by 4 - base
                const int sh = base - 4;
                m |= (uint32_t)(sh < 0 ? sel << -sh : (sh < 64 ? sel >> sh : 0ull));
            }
            // registers that hold no valid action for any env are skipped (wave-uniform)
            const uint32_t rm = __builtin_amdgcn_readfirstlane(REGM[mt]);
            bf16x8 wf[8];  // the tile's 8 fragments, read before the chain consumes them
#pragma unroll
            for (int k = 0; k < 8; ++k) wf[k] = W3f[(mt * 8 + k) * 64 + lane];
            f32x16 c = bias_frag(B3 + mt * 32 + 4 * h);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k], h2[k >> 1][k & 1], c, 0, 0, 0);
            m >>= 4 * h;  // register reg holds row base + 4h + (reg & 3) + 8 (reg >> 2)
            {
                // the winning register's tile-local row as an inline constant, the tile's base
                // added once if the tile raised the maximum (strict >: the first maximum stays)
                const float best0 = best;
                int bt = 0;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    if (!((rm >> reg) & 1u)) continue;
                    const int i = (reg & 3) + 8 * (reg >> 2);
                    const bool better = ((m >> i) & 1u) && c[reg] > best;  // ascending rows: first max
                    best = better ? c[reg] : best;
                    bt = better ? i : bt;
                }
                bidx = best != best0 ? base + 4 * h + bt : bidx;
            }
            if (kQout && live) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {  // the full layout: row = action
                    const int row = base + 4 * h + (reg & 3) + 8 * (reg >> 2);
                    if (row < q.rows) A.q_out[e * A.ldq + row] = fuel_finite(ff) ? c[reg] : NAN;
                }
            }
        }
        X3STAMP(3);
        // the next tile's env loads (issued a tile ago) are waited for here, before this
        // tile's stores: stores count in vmcnt too, so a wait at the loop's back edge would
        // wait out the action / record stores' round trip as well
        asm volatile("" ::"v"(nxt.fuel), "v"(nxt.x), "v"(nxt.y), "v"(nxt.o8), "v"(nxt.d8));
        // the two lane halves hold the same env: larger value, then lower index (merge_halves, inline:
        // called as the helper this kernel spilled, <true> 10 VGPRs and 40 SGPRs where it had none)
        const float ob2 = __shfl_xor(best, 32);
        const int oi = __shfl_xor(bidx, 32);
        if (ob2 > best || (ob2 == best && oi < bidx)) {
            best = ob2;
            bidx = oi;
        }
        CHOOSE_STORE(sel, cst, fst, e, live, h, bidx, cur_in.x, cur_in.y, cur_in.o8, cur_in.d8, ff);
        X3STAMP(4);
    }
    X3STAMP_ANY(11);
}
